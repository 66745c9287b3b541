/*
 * ORACLE -- test infrastructure only.  Never linked into, imported by or executed
 * from the product path (deseq2_amd/ and its libdeseq2_mi355x.so); only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
 *
 * Plain-C restatement of the three native entry points of thelovelab/DESeq2
 * (/root/reference/src/DESeq2.cpp):
 *     fitDisp      DESeq2.cpp:164-277   (+ log_posterior :31-64, dlog_posterior
 *                                          :68-107, d2log_posterior :111-158)
 *     fitBeta      DESeq2.cpp:283-465
 *     fitDispGrid  DESeq2.cpp:469-513
 * Same control flow, same counters, same break conditions, same clamps.  Each block
 * cites the reference lines it follows.
 *
 * PARITY STATUS: PINNED by the reference's own tests and by its own source compiled against stand-ins.
 * src/DESeq2.cpp includes RcppArmadillo.h, R.h, Rmath.h and R_ext/Utils.h (:16,23-25): R, Rcpp,
 * RcppArmadillo and Armadillo are external libraries this image lacks and no R runs here, so no
 * output of real R is in the tree.  What pins this file:
 *   (0) src/DESeq2.cpp itself, compiled where it lies against the stand-in headers of oracle/shim/
 *       (oracle/Makefile `ref`): the reference's control flow executed unchanged over stand-in linear
 *       algebra and binary128 special functions -- not R's nmath, not Armadillo's LAPACK.  Its recorded
 *       outputs (tests/golden/reference/) and, where the library is built, live runs:
 *       tests/test_oracle_vs_reference.py, tests/test_gpu_reference.py;
 *   (1) the reference's known-answer tests (tests/testthat/test_results.R:9,43-50;
 *       test_optim.R:30-39) and the cross-implementation properties its tests assert
 *       (test_betaFitting.R:2-47, test_dispersions.R:35-111, test_QR.R, test_weights.R:9-19)
 *       re-run with scipy / mpmath as the independent side -- tests/test_oracle_properties.py
 *       (SURVEY.md 8c lists them; the R tests' own seeds are R-RNG specific);
 *   (2) mpmath accuracy tests of every scalar primitive restated from R's nmath
 *       (tests/golden/nmath_golden.json, tests/test_oracle_math.py);
 *   (3) an independently written numpy restatement of the three routines over real LAPACK and
 *       scipy's special functions (oracle/lapack_oracle.py): iteration and accept counts equal
 *       outside ulp-level Armijo ties, values within 1e-7 / 1e-8 (tests/test_oracle_vs_lapack.py).
 * NOT pinned: iteration counts against a run of real R (the reference's tests assert none but
 * betaIter == 100 in test_optim.R:35); where the reference's formulas are themselves rounding
 * noise (alpha ~ 1e-8: dlog_posterior scales digamma differences by alpha^-2, DESeq2.cpp:90-96)
 * only the implementation-independent facts are asserted.  The R-side callers restated later in
 * this file (moments, trend fit, Cook's distance, replaceOutliers) are R code in the reference;
 * they are checked against independent numpy statements of the R lines cited.
 *
 * ARITHMETIC SPEC (what "the same result" means for the GPU):
 *   - all arithmetic IEEE binary64, no FMA contraction, fma() only where written;
 *   - scalar transcendental functions from orc_nmath.c;
 *   - every sum over the m samples of a gene is taken in WAVE ORDER: 64 partial
 *     sums, partial l accumulating samples l, l+64, l+128, ... in that order from
 *     0.0, then a butterfly v[l] += v[l^off] for off = 1,2,4,8,16,32.  The
 *     reference's own summation order is unspecified (Rcpp sugar / BLAS dgemm /
 *     LAPACK, all implementation-dependent), so fixing one is within its contract.
 *     sum_mode = 1 switches to plain serial sums, used only to measure how many
 *     iteration counts move between two equally valid orders.  ONE exception (round 3): the Cox-Reid Gram sums of
 *     fitDisp in general mode (no design cells) with p >= 7 and m <= 256 (p >= 10: m <= 1024) are serial sums in
 *     sample order (cr_gram);
 *   - p x p work: LU with partial pivoting (first maximum wins), reciprocal
 *     pivots, as LAPACK dgetf2; QR by unblocked Householder reflections as LAPACK
 *     dgeqr2/dlarfg (what qr_econ reaches for p < 32).
 */
#include "../include/dsq_arith_spec.h"   /* where a sum's order depends on the shape: one definition with the kernels */
#include "orc_nmath.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define ORC_PMAX 64

/* ------------------------------------------------------------ wave sums ---- */
typedef struct { double part[64]; int serial; double sacc; } wsum_t;

static inline void wsum_init(wsum_t *s, int serial) {
    for (int l = 0; l < 64; l++) s->part[l] = 0.0;
    s->serial = serial; s->sacc = 0.0;
}
static inline void wsum_add(wsum_t *s, long j, double t) {
    if (s->serial) s->sacc += t; else s->part[j & 63] += t;
}
static inline double wsum_total(const wsum_t *s) {
    if (s->serial) return s->sacc;
    double v[64], w[64];
    memcpy(v, s->part, sizeof v);
    for (int off = 1; off < 64; off <<= 1) {
        for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ off];
        memcpy(v, w, sizeof v);
    }
    return v[0];
}

/* ---------------------------------------------------------- small p x p ---- */
/* LU with partial pivoting, in place, row-major a[q*q]; rdiag[i] = 1/U_ii.
 * Returns the permutation sign (+1/-1).  (arma::det/inv/solve -> LAPACK dgetrf;
 * DESeq2.cpp:46,85,86,130,133-135,398,439,452)                                 */
static int lu_decomp(int q, double *a, int *piv, double *rdiag) {
    int sign = 1;
    for (int k = 0; k < q; k++) {
        int pr = k; double best = fabs(a[k * q + k]);
        for (int i = k + 1; i < q; i++) {
            double v = fabs(a[i * q + k]);
            if (v > best) { best = v; pr = i; }
        }
        piv[k] = pr;
        if (pr != k) {
            for (int j = 0; j < q; j++) { double t = a[k * q + j]; a[k * q + j] = a[pr * q + j]; a[pr * q + j] = t; }
            sign = -sign;
        }
        double rinv = 1.0 / a[k * q + k];
        rdiag[k] = rinv;
        for (int i = k + 1; i < q; i++) {
            double l = a[i * q + k] * rinv;
            a[i * q + k] = l;
            for (int j = k + 1; j < q; j++) a[i * q + j] = fma(-l, a[k * q + j], a[i * q + j]);
        }
    }
    return sign;
}
static double lu_det(int q, const double *lu, int sign) {
    if (q == 0) return 1.0;   /* every row below the weight threshold (:41-43): det of the 0 x 0 matrix is 1 */
    double d = lu[0];
    for (int i = 1; i < q; i++) d = d * lu[i * q + i];
    return sign < 0 ? -d : d;
}
/* solve LU x = P b in place (b -> x) */
static void lu_solve(int q, const double *lu, const int *piv, const double *rdiag, double *b) {
    for (int k = 0; k < q; k++) { int pr = piv[k]; if (pr != k) { double t = b[k]; b[k] = b[pr]; b[pr] = t; } }
    for (int i = 0; i < q; i++) {
        double t = b[i];
        for (int j = 0; j < i; j++) t = fma(-lu[i * q + j], b[j], t);
        b[i] = t;
    }
    for (int i = q - 1; i >= 0; i--) {
        double t = b[i];
        for (int j = i + 1; j < q; j++) t = fma(-lu[i * q + j], b[j], t);
        b[i] = t * rdiag[i];
    }
}
/* inverse of a (row-major q x q) into inv; returns det through *det if non-NULL */
static void mat_inverse(int q, const double *a, double *inv, double *det) {
    double lu[ORC_PMAX * ORC_PMAX]; int piv[ORC_PMAX]; double rdiag[ORC_PMAX], col[ORC_PMAX];
    memcpy(lu, a, sizeof(double) * q * q);
    int sign = lu_decomp(q, lu, piv, rdiag);
    if (det) *det = lu_det(q, lu, sign);
    for (int c = 0; c < q; c++) {
        for (int i = 0; i < q; i++) col[i] = (i == c) ? 1.0 : 0.0;
        lu_solve(q, lu, piv, rdiag, col);
        for (int i = 0; i < q; i++) inv[i * q + c] = col[i];
    }
}
static double mat_det(int q, const double *a) {
    double lu[ORC_PMAX * ORC_PMAX]; int piv[ORC_PMAX]; double rdiag[ORC_PMAX];
    memcpy(lu, a, sizeof(double) * q * q);
    int sign = lu_decomp(q, lu, piv, rdiag);
    return lu_det(q, lu, sign);
}
static void mat_mul(int q, const double *a, const double *b, double *c) {
    for (int i = 0; i < q; i++)
        for (int j = 0; j < q; j++) {
            double acc = 0.0;
            for (int k = 0; k < q; k++) acc = fma(a[i * q + k], b[k * q + j], acc);
            c[i * q + j] = acc;
        }
}
/* trace(a*b) without forming the product */
static double trace_prod(int q, const double *a, const double *b) {
    double acc = 0.0;
    for (int i = 0; i < q; i++)
        for (int k = 0; k < q; k++) acc = fma(a[i * q + k], b[k * q + i], acc);
    return acc;
}

/* trace(A B) for a SYMMETRIC B: the sum over the columns k (ascending) of t_k = sum_i fma(A[i][k], B[i][k]) -- the form
 * the engine evaluates with one matrix column per lane (trace(B^-1 dB) of the Cox-Reid derivative, DESeq2.cpp:85,133) */
static double trace_sym(int q, const double *a, const double *b) {
    double tr = 0.0;
    for (int k = 0; k < q; k++) {
        double t = 0.0;
        for (int i = 0; i < q; i++) t = fma(a[i * q + k], b[i * q + k], t);
        tr = tr + t;
    }
    return tr;
}

#define ORC_CMAX 32
/* which designs take the cell-collapsed paths (the engine's rule): fitBeta at every width, the Cox-Reid
 * matrices of fitDisp from 4 columns up (below that the per-sample accumulation of the p(p+1)/2 <= 6 entries is
 * cheaper than the per-cell passes) */
#define ORC_BETA_CELL_MAXP DSQ_SPEC_BETA_CELL_MAXP
#define ORC_DISP_CELL_MINP 4
static int design_cells(int m, int p, const double *x, int cmax, int *perm, int *start, double *xc);

/* ------------------------------------------------ one gene's row context ---- */
typedef struct {
    int m, p;
    const double *y;      /* m */
    const double *mu;     /* m */
    const double *w;      /* m observation weights (ignored unless useWeights) */
    const double *x;      /* m x p column-major (R layout) */
    double prior_mean, prior_sigmasq;
    int usePrior, useWeights, useCR;
    double weightThreshold;
    int serial;
    /* derived once per gene: CR row/column subsets (DESeq2.cpp:41-43) */
    int q;                /* number of kept columns */
    int keepcol[ORC_PMAX];
    const unsigned char *keeprow; /* m, or NULL = all */
    /* unweighted genes: the DISTINCT count values (ascending) and their multiplicities -- the lgamma / digamma
     * terms of the likelihood depend on the sample only through its count, so they are evaluated once per distinct
     * value (see log_posterior).  NULL with observation weights. */
    int nv;
    const double *dv, *dc;
    /* design cells (0 = general path): the Cox-Reid matrices X' diag(wd) X are assembled from per-cell sums of wd */
    int C;
    const int *cperm, *cstart;
    const double *xc;
} gene_t;

static int cmp_count(const void *a, const void *b) {
    double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

/* vbuf, cbuf: m doubles each */
static void gene_setup_distinct(gene_t *g, double *vbuf, double *cbuf) {
    g->nv = 0; g->dv = NULL; g->dc = NULL;
    if (g->useWeights) return;
    memcpy(vbuf, g->y, sizeof(double) * g->m);
    qsort(vbuf, g->m, sizeof(double), cmp_count);
    int nv = 0;
    for (int j = 0; j < g->m; j++) {
        if (nv > 0 && vbuf[j] == vbuf[nv - 1]) cbuf[nv - 1] += 1.0;
        else { vbuf[nv] = vbuf[j]; cbuf[nv] = 1.0; nv++; }
    }
    g->nv = nv; g->dv = vbuf; g->dc = cbuf;
}

static void gene_setup_cr(gene_t *g, unsigned char *rowbuf) {
    g->keeprow = NULL;
    g->q = g->p;
    for (int c = 0; c < g->p; c++) g->keepcol[c] = c;
    if (g->useCR && g->useWeights) {
        /* x = x.rows(find(wts > weightThreshold)); x = x.cols(find(sum(abs(x)) > 0.0)); */
        for (int j = 0; j < g->m; j++) rowbuf[j] = (g->w[j] > g->weightThreshold);
        g->keeprow = rowbuf;
        int q = 0;
        for (int c = 0; c < g->p; c++) {
            /* sum(abs(x)) > 0 over kept rows: any non-zero entry (exact, order-free) */
            int any = 0;
            for (int j = 0; j < g->m; j++)
                if (rowbuf[j] && fabs(g->x[j + (long)g->m * c]) > 0.0) { any = 1; break; }
            if (any) g->keepcol[q++] = c;
        }
        g->q = q;
    }
}

/* B = X' diag(wd) X over kept rows / kept columns, wave order by sample index.
 * term = x_ja * (x_jb * wd_j)   (b = x.t() * (x.each_col() % w_diag), :45,83,129) */
static void cr_gram(const gene_t *g, const double *wd, double *B) {
    int q = g->q, m = g->m;
    if (g->C > 0) {
        /* CELL MODE: every sample of a cell has the same design row x_c, so X' diag(wd) X = sum_c S_c x_c x_c' with
         * S_c = sum of wd over the kept samples of the cell (wave order over the position k in the cell-sorted
         * sequence), the outer
         * products added serially in cell order */
        double S[ORC_CMAX];
        for (int c = 0; c < g->C; c++) {
            wsum_t s; wsum_init(&s, g->serial);
            for (int k = g->cstart[c]; k < g->cstart[c + 1]; k++) {
                int j = g->cperm[k];
                if (g->keeprow && !g->keeprow[j]) continue;
                wsum_add(&s, k, wd[j]);
            }
            S[c] = wsum_total(&s);
        }
        for (int a = 0; a < q; a++)
            for (int b = a; b < q; b++) {
                double v = 0.0;
                for (int c = 0; c < g->C; c++)
                    v += (g->xc[c * g->p + g->keepcol[a]] * g->xc[c * g->p + g->keepcol[b]]) * S[c];
                B[a * q + b] = v; B[b * q + a] = v;
            }
        return;
    }
    /* general mode from 7 design columns up, rows of at most 256 samples (1024 from 10 columns up): the engine takes
     * these sums one matrix entry per lane, SERIALLY over the samples (csrc/fit_disp.hip: disp_serial_gram,
     * DispGene::pass) -- the order is part of the arithmetic spec, so the checker takes them serially under the same
     * condition */
    const int serial_gram = g->serial || (g->p >= DSQ_SPEC_SERIAL_GRAM_MINP &&
                                          m <= (g->p >= DSQ_SPEC_SERIAL_GRAM_WIDE_P ? DSQ_SPEC_SERIAL_GRAM_MAXM : DSQ_SPEC_SERIAL_GRAM_MAXM_NARROW));
    for (int a = 0; a < q; a++)
        for (int b = a; b < q; b++) {
            const double *xa = g->x + (long)m * g->keepcol[a];
            const double *xb = g->x + (long)m * g->keepcol[b];
            wsum_t s; wsum_init(&s, serial_gram);
            for (int j = 0; j < m; j++) {
                if (g->keeprow && !g->keeprow[j]) continue;
                wsum_add(&s, j, xa[j] * (xb[j] * wd[j]));
            }
            double v = wsum_total(&s);
            B[a * q + b] = v; B[b * q + a] = v;
        }
}

/* DESeq2.cpp:31-64 */
/* the sample at position k of a per-sample sum: the natural order, or -- with design cells -- the cell-sorted sequence
 * (one fused pass over the samples then feeds the likelihood sums and the per-cell Cox-Reid sums) */
#define POS_J(g, k) ((g)->C > 0 ? (g)->cperm[k] : (k))

static double log_posterior(double log_alpha, const gene_t *g, double *scratch) {
    double prior_part, cr_term;
    double alpha = orc_exp(log_alpha);
    int m = g->m;
    if (g->useCR) {
        double *wd = scratch;
        /* :36  w = 1 / (1/mu + alpha) = mu r,  r = 1 / (1 + mu alpha): the reciprocal the likelihood derivative uses */
        for (int j = 0; j < m; j++) wd[j] = g->mu[j] * (1.0 / (1.0 + g->mu[j] * alpha));
        double B[ORC_PMAX * ORC_PMAX];
        cr_gram(g, wd, B);                                                       /* :45 */
        cr_term = -0.5 * orc_log(mat_det(g->q, B));                              /* :46 */
    } else cr_term = 0.0;
    double alpha_neg1 = 1.0 / alpha;                                             /* :50 R_pow_di(alpha,-1) */
    double lg_an1 = orc_lgamma(alpha_neg1);
    /* :53,55  sum_j [w_j] ( lgamma(y_j + 1/a) - lgamma(1/a) - y_j log(mu_j + 1/a) - (1/a) log(1 + mu_j a) ), with
     *   log(mu + 1/a) = log(1 + mu a) - log a      (one logarithm per sample instead of two), and, without weights,
     *   sum_j (lgamma(y_j + 1/a) - lgamma(1/a)) = sum_v c_v (lgamma(v + 1/a) - lgamma(1/a))  over the distinct
     *   counts v with multiplicity c_v (one lgamma per distinct count instead of one per sample); distinct value i
     *   goes to partial i + 1 (slot 0 of the engine's first trip evaluates lgamma(1/a) itself).                 */
    wsum_t s; wsum_init(&s, g->serial);
    double ll_part;
    if (g->dv) {
        wsum_t sv; wsum_init(&sv, g->serial);
        for (int i = 0; i < g->nv; i++)
            wsum_add(&sv, i + 1, g->dc[i] * (orc_lgamma(g->dv[i] + alpha_neg1) - lg_an1));
        for (int k = 0; k < m; k++) {
            const int j = POS_J(g, k);
            double y = g->y[j], mu = g->mu[j];
            double l1 = orc_log(1.0 + mu * alpha);
            wsum_add(&s, k, -(y * (l1 - log_alpha)) - alpha_neg1 * l1);
        }
        ll_part = wsum_total(&sv) + wsum_total(&s);
    } else {
        for (int k = 0; k < m; k++) {
            const int j = POS_J(g, k);
            double y = g->y[j], mu = g->mu[j];
            double l1 = orc_log(1.0 + mu * alpha);
            double t = orc_lgamma(y + alpha_neg1) - lg_an1 - y * (l1 - log_alpha) - alpha_neg1 * l1;
            wsum_add(&s, k, g->w[j] * t);
        }
        ll_part = wsum_total(&s);
    }
    if (g->usePrior) {
        double d = log_alpha - g->prior_mean;
        prior_part = -0.5 * (d * d) / g->prior_sigmasq;                          /* :58 */
    } else prior_part = 0.0;
    return ll_part + prior_part + cr_term;                                       /* :62 */
}

/* DESeq2.cpp:68-107 */
static double dlog_posterior(double log_alpha, const gene_t *g, double *scratch) {
    double prior_part, cr_term;
    double alpha = orc_exp(log_alpha);
    int m = g->m;
    if (g->useCR) {
        double *wd = scratch, *dwd = scratch + m;
        for (int j = 0; j < m; j++) {
            double w0 = g->mu[j] * (1.0 / (1.0 + g->mu[j] * alpha));
            wd[j] = w0;                                                          /* :73  1 / (1/mu + alpha) */
            dwd[j] = -(w0 * w0);                                                 /* :74  -(1/mu + alpha)^-2 */
        }
        int q = g->q;
        double B[ORC_PMAX * ORC_PMAX], dB[ORC_PMAX * ORC_PMAX], Bi[ORC_PMAX * ORC_PMAX], detb;
        cr_gram(g, wd, B); cr_gram(g, dwd, dB);                                  /* :83,84 */
        mat_inverse(q, B, Bi, &detb);
        double ddetb = detb * trace_sym(q, Bi, dB);                              /* :85 */
        cr_term = -0.5 * ddetb / detb;                                           /* :86 */
    } else cr_term = 0.0;
    double alpha_neg1 = 1.0 / alpha;
    double alpha_neg2 = 1.0 / (alpha * alpha);                                   /* :91 R_pow_di(alpha,-2) */
    double dg_an1 = orc_digamma(alpha_neg1);
    /* :94,96  sum_j [w_j] ( digamma(1/a) + log(1 + mu a) - mu a / (1 + mu a) - digamma(y + 1/a) + y / (mu + 1/a) ),
     * with r = 1 / (1 + mu a):  mu a / (1 + mu a) = (mu a) r,  1 / (mu + 1/a) = a r  (one division per sample), and
     * the digamma terms over the distinct counts when there are no weights (see log_posterior).                */
    wsum_t s; wsum_init(&s, g->serial);
    double ll_sum;
    if (g->dv) {
        wsum_t sv; wsum_init(&sv, g->serial);
        for (int i = 0; i < g->nv; i++)
            wsum_add(&sv, i + 1, g->dc[i] * (dg_an1 - orc_digamma(g->dv[i] + alpha_neg1)));
        for (int k = 0; k < m; k++) {
            const int j = POS_J(g, k);
            double y = g->y[j], mu = g->mu[j];
            double ma = mu * alpha;
            double r = 1.0 / (1.0 + ma);
            wsum_add(&s, k, orc_log(1.0 + ma) - ma * r + y * (alpha * r));
        }
        ll_sum = wsum_total(&sv) + wsum_total(&s);
    } else {
        for (int k = 0; k < m; k++) {
            const int j = POS_J(g, k);
            double y = g->y[j], mu = g->mu[j];
            double ma = mu * alpha;
            double r = 1.0 / (1.0 + ma);
            double t = dg_an1 + orc_log(1.0 + ma) - ma * r - orc_digamma(y + alpha_neg1) + y * (alpha * r);
            wsum_add(&s, k, g->w[j] * t);
        }
        ll_sum = wsum_total(&s);
    }
    double ll_part = alpha_neg2 * ll_sum;
    if (g->usePrior) prior_part = -1.0 * (log_alpha - g->prior_mean) / g->prior_sigmasq; /* :100 */
    else prior_part = 0.0;
    return (ll_part + cr_term) * alpha + prior_part;                             /* :105 */
}

/* DESeq2.cpp:111-158 */
static double d2log_posterior(double log_alpha, const gene_t *g, double *scratch) {
    double prior_part, cr_term;
    double alpha = orc_exp(log_alpha);
    int m = g->m;
    if (g->useCR) {
        double *wd = scratch, *dwd = scratch + m, *d2wd = scratch + 2 * (long)m;
        for (int j = 0; j < m; j++) {
            double w0 = g->mu[j] * (1.0 / (1.0 + g->mu[j] * alpha));
            wd[j] = w0;                                                          /* :117 */
            dwd[j] = -(w0 * w0);                                                 /* :118 */
            d2wd[j] = 2.0 * (w0 * (w0 * w0));                                    /* :119 */
        }
        int q = g->q;
        double B[ORC_PMAX * ORC_PMAX], dB[ORC_PMAX * ORC_PMAX], d2B[ORC_PMAX * ORC_PMAX];
        double Bi[ORC_PMAX * ORC_PMAX], M[ORC_PMAX * ORC_PMAX], detb;
        cr_gram(g, wd, B); cr_gram(g, dwd, dB); cr_gram(g, d2wd, d2B);           /* :129-132 */
        mat_inverse(q, B, Bi, &detb);
        double tr1 = trace_sym(q, Bi, dB);
        double ddetb = detb * tr1;                                               /* :133 */
        mat_mul(q, Bi, dB, M);
        double tr2 = trace_prod(q, M, M);                  /* trace(b_i*db*b_i*db) */
        double tr3 = trace_sym(q, Bi, d2B);
        double d2detb = detb * (tr1 * tr1 - tr2 + tr3);                          /* :134 */
        double rr = ddetb / detb;
        cr_term = 0.5 * (rr * rr) - 0.5 * d2detb / detb;                         /* :135 */
    } else cr_term = 0.0;
    double alpha_neg1 = 1.0 / alpha;
    double alpha_neg2 = 1.0 / (alpha * alpha);
    double alpha_neg3 = 1.0 / (alpha * (alpha * alpha));   /* R_pow_di(alpha,-3): xn=x; x=x*x; xn*=x */
    double dg_an1 = orc_digamma(alpha_neg1), tg_an1 = orc_trigamma(alpha_neg1);
    wsum_t s1, s2; wsum_init(&s1, g->serial); wsum_init(&s2, g->serial);
    for (int k = 0; k < m; k++) {                                                /* :143,145 */
        const int j = POS_J(g, k);
        double y = g->y[j], mu = g->mu[j];
        double ma = mu * alpha, opm = 1.0 + ma, mpa = mu + alpha_neg1;
        double t1 = dg_an1 + orc_log(opm) - ma * (1.0 / opm)
                    - orc_digamma(y + alpha_neg1) + y * (1.0 / mpa);
        double t2 = -1.0 * alpha_neg2 * tg_an1 + (mu * mu) * alpha * (1.0 / (opm * opm))
                    + alpha_neg2 * orc_trigamma(y + alpha_neg1)
                    + alpha_neg2 * y * (1.0 / (mpa * mpa));
        if (g->useWeights) { t1 = g->w[j] * t1; t2 = g->w[j] * t2; }
        wsum_add(&s1, k, t1); wsum_add(&s2, k, t2);
    }
    double ll_part = -2.0 * alpha_neg3 * wsum_total(&s1) + alpha_neg2 * wsum_total(&s2);
    if (g->usePrior) prior_part = -1.0 / g->prior_sigmasq;                       /* :149 */
    else prior_part = 0.0;
    /* :156 -- the inner dlog_posterior call has usePrior = false and the full x */
    gene_t g0 = *g; g0.usePrior = 0;
    double dlp0 = dlog_posterior(log_alpha, &g0, scratch);
    return ((ll_part + cr_term) * (alpha * alpha) + dlp0) + prior_part;
}

/* ================================================================ fitDisp ==
 * DESeq2.cpp:164-277.  All matrices in R layout (column-major, gene fastest).  */
int orc_fit_disp(int n, int m, int p,
                 const double *y, const double *x, const double *mu_hat,
                 const double *log_alpha_in, const double *log_alpha_prior_mean,
                 double log_alpha_prior_sigmasq, double min_log_alpha, double kappa_0,
                 double tol, int maxit, int usePrior,
                 const double *weights, int useWeights, double weightThreshold, int useCR,
                 double *log_alpha_out, int *iter, int *iter_accept, double *last_change,
                 double *initial_lp, double *initial_dlp, double *last_lp,
                 double *last_dlp, double *last_d2lp, int sum_mode, int cell_mode) {
    if (p > ORC_PMAX) return -1;
    const double epsilon = 1.0e-4;                                               /* :175 */
    int *cperm = malloc(sizeof(int) * (m > 0 ? m : 1)), cstart[ORC_CMAX + 1];
    double *xc = malloc(sizeof(double) * ORC_CMAX * ORC_PMAX);
    const int C = (cell_mode && p >= ORC_DISP_CELL_MINP) ? design_cells(m, p, x, ORC_CMAX, cperm, cstart, xc) : 0;
#pragma omp parallel
    {
    double *yrow = malloc(sizeof(double) * m), *murow = malloc(sizeof(double) * m);
    double *wrow = malloc(sizeof(double) * m), *scratch = malloc(sizeof(double) * 3 * (size_t)m);
    unsigned char *rowbuf = malloc(m);
    double *vbuf = malloc(sizeof(double) * m), *cbuf = malloc(sizeof(double) * m);
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {                                                /* :194 */
        for (int j = 0; j < m; j++) {
            yrow[j] = y[i + (long)n * j]; murow[j] = mu_hat[i + (long)n * j];
            wrow[j] = weights ? weights[i + (long)n * j] : 1.0;
        }
        gene_t g; memset(&g, 0, sizeof g);
        g.m = m; g.p = p; g.y = yrow; g.mu = murow; g.w = wrow; g.x = x;
        g.prior_mean = log_alpha_prior_mean[i]; g.prior_sigmasq = log_alpha_prior_sigmasq;
        g.usePrior = usePrior; g.useWeights = useWeights; g.useCR = useCR;
        g.weightThreshold = weightThreshold; g.serial = sum_mode;
        g.C = C; g.cperm = cperm; g.cstart = cstart; g.xc = xc;
        gene_setup_cr(&g, rowbuf);
        gene_setup_distinct(&g, vbuf, cbuf);
        double a = log_alpha_in[i];                                              /* :201 */
        double lp = log_posterior(a, &g, scratch);                               /* :205 */
        double dlp = dlog_posterior(a, &g, scratch);                             /* :206 */
        double kappa = kappa_0, lpnew, change = -1.0;                            /* :207-211 */
        initial_lp[i] = lp; initial_dlp[i] = dlp;
        int it = 0, it_acc = 0;
        for (int t = 0; t < maxit; t++) {                                        /* :212 */
            it++;                                                                /* :214 */
            double a_propose = a + kappa * dlp;                                  /* :215 */
            if (a_propose < -30.0) kappa = (-30.0 - a) / dlp;                    /* :218-220 */
            if (a_propose > 10.0) kappa = (10.0 - a) / dlp;                      /* :222-224 */
            double theta_kappa = -1.0 * log_posterior(a + kappa * dlp, &g, scratch);   /* :225 */
            double theta_hat_kappa = -1.0 * lp - kappa * epsilon * (dlp * dlp);  /* :226 */
            if (theta_kappa <= theta_hat_kappa) {                                /* :229 */
                it_acc++;                                                        /* :231 */
                a = a + kappa * dlp;                                             /* :232 */
                lpnew = log_posterior(a, &g, scratch);                           /* :233 */
                change = lpnew - lp;                                             /* :235 */
                if (change < tol) { lp = lpnew; break; }                         /* :236-239 */
                if (a < min_log_alpha) break;                                    /* :242-244 */
                lp = lpnew;                                                      /* :245 */
                dlp = dlog_posterior(a, &g, scratch);                            /* :246 */
                kappa = fmin(kappa * 1.1, kappa_0);                              /* :249 */
                if (it_acc % 5 == 0) kappa = kappa / 2.0;                        /* :253-255 */
            } else {
                kappa = kappa / 2.0;                                             /* :257 */
            }
        }
        last_lp[i] = lp; last_dlp[i] = dlp;                                      /* :260-261 */
        last_d2lp[i] = d2log_posterior(a, &g, scratch);                          /* :262 */
        log_alpha_out[i] = a;                                                    /* :263 */
        last_change[i] = change;                                                 /* :265 */
        iter[i] = it; iter_accept[i] = it_acc;
    }
    free(yrow); free(murow); free(wrow); free(scratch); free(rowbuf); free(vbuf); free(cbuf);
    }
    free(cperm); free(xc);
    return 0;
}

/* ============================================================ fitDispGrid ==
 * DESeq2.cpp:469-513 */
int orc_fit_disp_grid(int n, int m, int p,
                      const double *y, const double *x, const double *mu_hat,
                      const double *disp_grid, int ngrid,
                      const double *log_alpha_prior_mean, double log_alpha_prior_sigmasq,
                      int usePrior, const double *weights, int useWeights,
                      double weightThreshold, int useCR, double *log_alpha_out, int sum_mode, int cell_mode) {
    if (p > ORC_PMAX || ngrid < 2 || ngrid > 1024) return -1;
    double delta = disp_grid[1] - disp_grid[0];                                  /* :480 */
    int *cperm = malloc(sizeof(int) * (m > 0 ? m : 1)), cstart[ORC_CMAX + 1];
    double *xc = malloc(sizeof(double) * ORC_CMAX * ORC_PMAX);
    const int C = (cell_mode && p >= ORC_DISP_CELL_MINP) ? design_cells(m, p, x, ORC_CMAX, cperm, cstart, xc) : 0;
#pragma omp parallel
    {
    double *yrow = malloc(sizeof(double) * m), *murow = malloc(sizeof(double) * m);
    double *wrow = malloc(sizeof(double) * m), *scratch = malloc(sizeof(double) * 3 * (size_t)m);
    unsigned char *rowbuf = malloc(m);
    double *lpv = malloc(sizeof(double) * ngrid), *fine = malloc(sizeof(double) * ngrid);
    double *vbuf = malloc(sizeof(double) * m), *cbuf = malloc(sizeof(double) * m);
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {                                                /* :492 */
        for (int j = 0; j < m; j++) {
            yrow[j] = y[i + (long)n * j]; murow[j] = mu_hat[i + (long)n * j];
            wrow[j] = weights ? weights[i + (long)n * j] : 1.0;
        }
        gene_t g; memset(&g, 0, sizeof g);
        g.m = m; g.p = p; g.y = yrow; g.mu = murow; g.w = wrow; g.x = x;
        g.prior_mean = log_alpha_prior_mean[i]; g.prior_sigmasq = log_alpha_prior_sigmasq;
        g.usePrior = usePrior; g.useWeights = useWeights; g.useCR = useCR;
        g.weightThreshold = weightThreshold; g.serial = sum_mode;
        g.C = C; g.cperm = cperm; g.cstart = cstart; g.xc = xc;
        gene_setup_cr(&g, rowbuf);
        gene_setup_distinct(&g, vbuf, cbuf);
        for (int t = 0; t < ngrid; t++) lpv[t] = log_posterior(disp_grid[t], &g, scratch);  /* :496-500 */
        int idx = 0; double best = lpv[0];                                       /* :501 .max(idxmax) */
        for (int t = 1; t < ngrid; t++) if (lpv[t] > best) { best = lpv[t]; idx = t; }
        double a_hat = disp_grid[idx];                                           /* :502 */
        /* arma::linspace(a_hat - delta, a_hat + delta, ngrid)                      :503 */
        double start = a_hat - delta, end = a_hat + delta;
        double step = (end >= start) ? (end - start) / (double)(ngrid - 1)
                                     : -(start - end) / (double)(ngrid - 1);
        for (int t = 0; t < ngrid - 1; t++) fine[t] = start + (double)t * step;
        fine[ngrid - 1] = end;
        for (int t = 0; t < ngrid; t++) lpv[t] = log_posterior(fine[t], &g, scratch);       /* :504-507 */
        idx = 0; best = lpv[0];
        for (int t = 1; t < ngrid; t++) if (lpv[t] > best) { best = lpv[t]; idx = t; }
        log_alpha_out[i] = fine[idx];                                            /* :509 */
    }
    free(yrow); free(murow); free(wrow); free(scratch); free(rowbuf); free(lpv); free(fine); free(vbuf); free(cbuf);
    }
    free(cperm); free(xc);
    return 0;
}

/* ------------------------------------------------------------- design cells ----
 * Samples with identical model-matrix rows form a design CELL (modelMatrixGroups, R/core.R:2450).  Every factor
 * design has a handful; a continuous covariate gives one cell per sample.  Cells are numbered in order of first
 * appearance; xc[c*p + k] is the row of cell c; perm lists the samples grouped by cell (ascending sample index
 * inside a cell), start[c] .. start[c+1] the members of cell c.  Returns the number of cells, or 0 when there are
 * more than cmax (the callers then take the general per-sample path).                                           */
static int design_cells(int m, int p, const double *x, int cmax, int *perm, int *start, double *xc) {
    int *cell_of = malloc(sizeof(int) * (m > 0 ? m : 1));
    int C = 0;
    for (int j = 0; j < m; j++) {
        int c;
        for (c = 0; c < C; c++) {
            int same = 1;
            for (int k = 0; k < p; k++) if (x[j + (long)m * k] != xc[c * p + k]) { same = 0; break; }
            if (same) break;
        }
        if (c == C) {
            if (C == cmax) { free(cell_of); return 0; }
            for (int k = 0; k < p; k++) xc[C * p + k] = x[j + (long)m * k];
            C++;
        }
        cell_of[j] = c;
    }
    for (int c = 0; c <= C; c++) start[c] = 0;
    for (int j = 0; j < m; j++) start[cell_of[j] + 1]++;
    for (int c = 0; c < C; c++) start[c + 1] += start[c];
    int fill[ORC_CMAX];
    for (int c = 0; c < C; c++) fill[c] = start[c];
    for (int j = 0; j < m; j++) perm[fill[cell_of[j]]++] = j;
    free(cell_of);
    return C;
}

static void householder_ls(int M, int p, double *A, double *b, double *beta, int serial);

/* 0: the sample's log density follows the closed split of fit_beta_gene_cells (a zero count, or a count on the general
 * branch of dnbinom_mu); 1: evaluate dnbinom_mu in full (tiny count / size ratios, degenerate size) */
static int cell_dev_class(double y, double size, int fast) {
    if (!fast) return 1;
    if (y == 0.0) return 0;
    const double n = y + size;
    const int gen = (y > 0.0) && isfinite(y) && !(y < 1e-10 * size) && (n != size) && isfinite(n);
    return gen ? 0 : 1;
}

/* K = sum_j [wts_j] K_j, the mu-independent part of the IRLS deviance (see fit_beta_gene_cells), samples in their
 * natural order; 0 when the closed split does not apply (fast = 0) */
static double irls_constants(int m, const double *yrow, const double *nfrow, const double *wts, int useWeights,
                             double alpha, double size, int fast, int sum_mode) {
    if (!fast) return 0.0;
    const double st_size = orc_stirlerr(size);
    wsum_t sk; wsum_init(&sk, sum_mode);
    for (int j = 0; j < m; j++) {
        double kj = 0.0;
        if (yrow[j] != 0.0 && cell_dev_class(yrow[j], size, fast) == 0) {
            /* saddle-point constants of dnbinom_mu with their logarithms folded: log(size/(size+y)) = -L and
             * log1p(-size/n) = log y - log size - L,  L = log1p(alpha y)  -- three logarithms per sample */
            const double y = yrow[j], n = y + size;
            const double L = orc_log1p(alpha * y), ly = orc_log(y);
            const double c0 = orc_stirlerr(n) - st_size - orc_stirlerr(n - size);
            kj = -L + (c0 - 0.5 * (1.837877066409345483560659472811 /* ln 2 pi */ + ly - L)) + ((n * L - y * ly) + y * orc_log(nfrow[j]));
        }
        wsum_add(&sk, j, useWeights ? wts[j] * kj : kj);
    }
    return wsum_total(&sk);
}

/* fitBeta in CELL MODE (at most ORC_CMAX design cells).  Within a cell every sample has the same design row x_c, so
 *   - the linear predictor is one value eta_c per cell, mu_j = max(nf_j exp(eta_c), minmu)       (:324-327, bits as
 *     in the general path);
 *   - the weighted least squares of an IRLS step depends on the samples only through S_c = sum_{j in c} w_j and
 *     T_c = sum_{j in c} w_j z_j: it is solved on the COLLAPSED (C + p) x p system with rows sqrt(S_c) x_c and
 *     right-hand side T_c / sqrt(S_c) -- the normal equations X'WX + ridge, X'Wz of :344-356 / :398 -- by the same
 *     Householder QR (useQR) or LU; z_j = eta_c + (y_j - mu_j)/mu_j where mu_j is not clamped (log(mu/nf) = eta_c);
 *   - the deviance -2 sum [wts] log NB(y; 1/alpha, mu): on the saddle-point form of dnbinom_mu the two bd0 terms are
 *     -bd0(size, n p) - bd0(y, n q) = -n [log1p(alpha mu) - log1p(alpha y)] - y [log y - log mu]  (n = y + size), so
 *     log f_j = K_j + y_j lg_j - n_j log1p(alpha mu_j)  with lg_j = log(mu_j / nf_j) (the value z_j already uses) and
 *     K_j = [saddle-point constants] + n log1p(alpha y) - y log y + y log nf_j  independent of mu; K = sum K_j once
 *     per gene, one logarithm per sample and iteration: dev = -2 (K + D).  (y = 0: K_j = 0, same D_j.)  The split
 *     keeps every logarithm on an argument that carries full relative accuracy (log1p forms), so dev agrees with the
 *     bd0 evaluation to ~1e-14 relative -- six orders below the convergence tolerance it is compared with;
 *   - post-loop: X'WX = sum_c S_c x_c x_c', hat diagonal h_j = w_j x_c'(X'WX + ridge)^-1 x_c.
 * Sums over the samples run cell by cell, in wave order over the POSITION k of the sample in the cell-sorted sequence
 * (partial k mod 64; the 64 partials of the deviance keep accumulating across the cells); K runs over the samples in
 * their natural order.  Every convergence rule is that of the general path.                                */
static void fit_beta_gene_cells(int m, int p, int C, const int *perm, const int *start, const double *xc,
                                const double *yrow, const double *nfrow, const double *wts, int useWeights,
                                double alpha, const double *lambda, const double *contrast, double *beta_hat,
                                double tol, int maxit, int useQR, double minmu, int sum_mode,
                                double *A, double *bb, double *beta_var, double *it_out, double *hat,
                                double *cnum, double *cden, double *dev_out) {
    const double large = 30.0;
    const double size = 1.0 / alpha;
    double eta_c[ORC_CMAX], exp_c[ORC_CMAX], exp_prev[ORC_CMAX], Sc[ORC_CMAX], Tc[ORC_CMAX];
    double K = 0.0;
    #define CELL_ETA() \
        for (int c = 0; c < C; c++) { \
            double eta = xc[c * p] * beta_hat[0]; \
            for (int k = 1; k < p; k++) eta = fma(xc[c * p + k], beta_hat[k], eta); \
            eta_c[c] = eta; exp_c[c] = orc_exp(eta); }
    /* one sweep over the samples at the current beta: S_c, T_c (for the next least squares / the post-loop block)
     * and, when asked, the deviance parts */
    #define CELL_SWEEP(WITH_DEV) do { \
        wsum_t sd; wsum_init(&sd, sum_mode); \
        for (int c = 0; c < C; c++) { \
            wsum_t s1, s2; wsum_init(&s1, sum_mode); wsum_init(&s2, sum_mode); \
            for (int k = start[c]; k < start[c + 1]; k++) { \
                const int j = perm[k], r = k;   /* wave order over the position in the cell-sorted sequence */ \
                const double raw = nfrow[j] * exp_c[c]; \
                const double mu = fmax(raw, minmu); \
                const double am = alpha * mu, opm = 1.0 + am, rcp = 1.0 / opm; \
                const double rw = useWeights ? wts[j] * rcp : rcp; \
                const double wv = mu * rw; \
                const double lg = (raw >= minmu) ? eta_c[c] : orc_log(mu / nfrow[j]); \
                /* w z = w log(mu/nf) + w (y - mu)/mu, and w / mu = [wts] / (1 + alpha mu): no second division */ \
                wsum_add(&s1, r, wv); wsum_add(&s2, r, wv * lg + rw * (yrow[j] - mu)); \
                if (WITH_DEV) { \
                    double t; \
                    if (cell_dev_class(yrow[j], size, fast) == 0) { \
                        /* log1p(alpha mu) from the rounded 1 + alpha mu and its rounding residual */ \
                        const double l1p = orc_log(opm) + (am - (opm - 1.0)) * rcp; \
                        t = yrow[j] * lg - (yrow[j] + size) * l1p; \
                    } else t = orc_dnbinom_mu_log(yrow[j], size, mu); \
                    wsum_add(&sd, r, useWeights ? wts[j] * t : t); \
                } \
            } \
            Sc[c] = wsum_total(&s1); Tc[c] = wsum_total(&s2); \
        } \
        if (WITH_DEV) dev = -2.0 * (K + wsum_total(&sd)); \
    } while (0)
    const int fast = (alpha > 0.0) && isfinite(alpha) && isfinite(size) && (size > 0.0);
    double dev = 0.0, dev_old = 0.0, it = 0.0;
    if (maxit > 0) K = irls_constants(m, yrow, nfrow, wts, useWeights, alpha, size, fast, sum_mode);
    CELL_ETA();
    CELL_SWEEP(0);
    for (int t = 0; t < maxit; t++) {
        it += 1.0;
        for (int c = 0; c < C; c++) exp_prev[c] = exp_c[c];
        if (useQR) {
            for (int c = 0; c < C; c++) {
                double sS = sqrt(Sc[c]);
                for (int k = 0; k < p; k++) A[(long)c * p + k] = xc[c * p + k] * sS;
                bb[c] = (sS > 0.0) ? Tc[c] / sS : 0.0;
            }
            for (int r = 0; r < p; r++) {
                for (int c = 0; c < p; c++) A[(long)(C + r) * p + c] = (r == c) ? sqrt(lambda[c]) : 0.0;
                bb[C + r] = 0.0;
            }
            householder_ls(C + p, p, A, bb, beta_hat, sum_mode);
        } else {
            double G[ORC_PMAX * ORC_PMAX], rhs[ORC_PMAX];
            for (int a = 0; a < p; a++) {
                for (int b = a; b < p; b++) {
                    double v = 0.0;
                    for (int c = 0; c < C; c++) v += (xc[c * p + a] * xc[c * p + b]) * Sc[c];
                    G[a * p + b] = v; G[b * p + a] = v;
                }
                double v = 0.0;
                for (int c = 0; c < C; c++) v += xc[c * p + a] * Tc[c];
                rhs[a] = v;
            }
            for (int a = 0; a < p; a++) G[a * p + a] = G[a * p + a] + lambda[a];
            int piv[ORC_PMAX]; double rdiag[ORC_PMAX];
            lu_decomp(p, G, piv, rdiag);
            lu_solve(p, G, piv, rdiag, rhs);
            for (int a = 0; a < p; a++) beta_hat[a] = rhs[a];
        }
        int toolarge = 0;
        for (int c = 0; c < p; c++) if (fabs(beta_hat[c]) > large) toolarge++;
        if (toolarge > 0) {                  /* :357-360: beta is kept, mu (and so S_c) stay those of the last update */
            it = (double)maxit;
            for (int c = 0; c < C; c++) exp_c[c] = exp_prev[c];
            break;
        }
        CELL_ETA();
        CELL_SWEEP(1);
        double conv_test = fabs(dev - dev_old) / (fabs(dev) + 0.1);
        if (isnan(conv_test)) { it = (double)maxit; break; }
        if ((t > 0) & (conv_test < tol)) break;
        dev_old = dev;
    }
    *dev_out = dev; *it_out = it;
    /* post-loop (:427-455) from the cell sums of the final mu */
    double G[ORC_PMAX * ORC_PMAX], Gr[ORC_PMAX * ORC_PMAX], Gi[ORC_PMAX * ORC_PMAX];
    for (int a = 0; a < p; a++)
        for (int b = a; b < p; b++) {
            double v = 0.0;
            for (int c = 0; c < C; c++) v += (xc[c * p + a] * xc[c * p + b]) * Sc[c];
            G[a * p + b] = v; G[b * p + a] = v;
        }
    memcpy(Gr, G, sizeof(double) * p * p);
    for (int a = 0; a < p; a++) Gr[a * p + a] = Gr[a * p + a] + lambda[a];
    mat_inverse(p, Gr, Gi, NULL);
    for (int c = 0; c < C; c++) {
        double h = 0.0;
        for (int i1 = 0; i1 < p; i1++)
            for (int i2 = 0; i2 < p; i2++) h += xc[c * p + i1] * (xc[c * p + i2] * Gi[i2 * p + i1]);
        for (int k = start[c]; k < start[c + 1]; k++) {
            const int j = perm[k];
            const double mu = fmax(nfrow[j] * exp_c[c], minmu);
            const double rcp = 1.0 / (1.0 + alpha * mu);
            const double wv = mu * (useWeights ? wts[j] * rcp : rcp);
            hat[j] = wv * h;
        }
    }
    double T[ORC_PMAX * ORC_PMAX], Sg[ORC_PMAX * ORC_PMAX];
    mat_mul(p, Gi, G, T); mat_mul(p, T, Gi, Sg);
    double cn = 0.0;
    for (int c = 0; c < p; c++) cn = fma(contrast[c], beta_hat[c], cn);
    *cnum = cn;
    double cd = 0.0;
    for (int b = 0; b < p; b++) {
        double r = 0.0;
        for (int a = 0; a < p; a++) r = fma(contrast[a], Sg[a * p + b], r);
        cd = fma(r, contrast[b], cd);
    }
    *cden = sqrt(cd);
    for (int c = 0; c < p; c++) beta_var[c] = Sg[c * p + c];
    #undef CELL_ETA
    #undef CELL_SWEEP
}

/* ================================================================ fitBeta ==
 * DESeq2.cpp:283-465 */

/* Least squares  min || [sqrt(w) X; sqrt(ridge)] beta - [sqrt(w) z; 0] ||  by
 * unblocked Householder QR of the (m+p) x p matrix (DESeq2.cpp:344-356: join_cols,
 * qr_econ, gamma_hat = q.t() * big_z_sqrt_w, solve(beta_hat, r, gamma_hat)).
 * A: (m+p) x p row-major work matrix, b: (m+p) rhs.  Reflector k is generated as
 * LAPACK dlarfg does (beta = -sign(alpha) ||col||, tau = (beta-alpha)/beta,
 * v = col/(alpha-beta)), with the column dot products S_kj = sum_{i>k} a_ik a_ij
 * taken in wave order over the row index i.                                    */
static void householder_ls(int M, int p, double *A, double *b, double *beta, int serial) {
    for (int k = 0; k < p; k++) {
        double S[ORC_PMAX + 1];
        for (int j = k; j <= p; j++) {
            wsum_t s; wsum_init(&s, serial);
            for (int i = k + 1; i < M; i++) {
                double aik = A[(long)i * p + k];
                double other = (j < p) ? A[(long)i * p + j] : b[i];
                wsum_add(&s, i, aik * other);
            }
            S[j] = wsum_total(&s);
        }
        double alpha = A[(long)k * p + k];
        double tau, scal, bet;
        if (S[k] == 0.0) { tau = 0.0; scal = 0.0; bet = alpha; }
        else {
            bet = -copysign(sqrt(alpha * alpha + S[k]), alpha);
            tau = (bet - alpha) / bet;
            scal = 1.0 / (alpha - bet);
        }
        double tvec[ORC_PMAX + 1];
        for (int j = k + 1; j <= p; j++) {
            double akj = (j < p) ? A[(long)k * p + j] : b[k];
            double wj = akj + scal * S[j];
            tvec[j] = -tau * wj;
        }
        for (int i = k + 1; i < M; i++) {
            double v = A[(long)i * p + k] * scal;
            for (int j = k + 1; j < p; j++) A[(long)i * p + j] = fma(v, tvec[j], A[(long)i * p + j]);
            b[i] = fma(v, tvec[p], b[i]);
        }
        for (int j = k + 1; j < p; j++) A[(long)k * p + j] = A[(long)k * p + j] + tvec[j];
        b[k] = b[k] + tvec[p];
        A[(long)k * p + k] = bet;
    }
    for (int i = p - 1; i >= 0; i--) {
        double t = b[i];
        for (int j = i + 1; j < p; j++) t = fma(-A[(long)i * p + j], beta[j], t);
        beta[i] = t / A[(long)i * p + i];
    }
}

int orc_fit_beta(int n, int m, int p,
                 const double *y, const double *x, const double *nf, const double *alpha_hat,
                 const double *contrast, const double *beta_init, const double *lambda,
                 const double *weights, int useWeights, double tol, int maxit, int useQR,
                 double minmu,
                 double *beta_mat, double *beta_var_mat, double *iter, double *hat_diagonals,
                 double *contrast_num, double *contrast_denom, double *deviance, int sum_mode, int cell_mode) {
    if (p > ORC_PMAX) return -1;
    const double large = 30.0;                                                   /* :316 */
    int *cperm = malloc(sizeof(int) * (m > 0 ? m : 1)), cstart[ORC_CMAX + 1];
    double *xc = malloc(sizeof(double) * ORC_CMAX * ORC_PMAX);
    const int C = (cell_mode && p <= ORC_BETA_CELL_MAXP) ? design_cells(m, p, x, ORC_CMAX, cperm, cstart, xc) : 0;
#pragma omp parallel
    {
    int M = m + p;
    double *yrow = malloc(sizeof(double) * m), *nfrow = malloc(sizeof(double) * m);
    double *wts = malloc(sizeof(double) * m), *mu = malloc(sizeof(double) * m);
    double *w_vec = malloc(sizeof(double) * m), *w_sqrt = malloc(sizeof(double) * m);
    double *z = malloc(sizeof(double) * m);
    double *A = malloc(sizeof(double) * ((size_t)M * p + (size_t)(ORC_CMAX + p) * p + 2 * (size_t)m)), *bb = malloc(sizeof(double) * (M + ORC_CMAX));
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {                                                /* :319 */
        double beta_hat[ORC_PMAX];
        for (int j = 0; j < m; j++) {
            yrow[j] = y[i + (long)n * j]; nfrow[j] = nf[i + (long)n * j];
            wts[j] = weights ? weights[i + (long)n * j] : 1.0;
        }
        for (int c = 0; c < p; c++) beta_hat[c] = beta_init[i + (long)n * c];    /* :323 */
        double alpha = alpha_hat[i];
        if (C > 0) {
            double bvar[ORC_PMAX], itv, cn_, cd_, dv_;
            fit_beta_gene_cells(m, p, C, cperm, cstart, xc, yrow, nfrow, wts, useWeights, alpha, lambda, contrast,
                                beta_hat, tol, maxit, useQR, minmu, sum_mode, A, bb, bvar, &itv, z, &cn_, &cd_, &dv_);
            for (int c = 0; c < p; c++) { beta_mat[i + (long)n * c] = beta_hat[c]; beta_var_mat[i + (long)n * c] = bvar[c]; }
            for (int j = 0; j < m; j++) hat_diagonals[i + (long)n * j] = z[j];
            iter[i] = itv; contrast_num[i] = cn_; contrast_denom[i] = cd_; deviance[i] = dv_;
            continue;
        }
        /* mu_hat = nfrow % exp(x * beta_hat), clamped                            :324-327 */
        #define ORC_UPDATE_MU() \
            for (int j = 0; j < m; j++) { \
                double eta = x[j] * beta_hat[0]; \
                for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], beta_hat[c], eta); \
                mu[j] = fmax(nfrow[j] * orc_exp(eta), minmu); }
        /* w_vec, w_sqrt_vec                                            :336-342,390-396 */
        #define ORC_UPDATE_W() \
            for (int j = 0; j < m; j++) { \
                double wv = useWeights ? (wts[j] * mu[j]) / (1.0 + alpha * mu[j]) \
                                       : mu[j] / (1.0 + alpha * mu[j]); \
                w_vec[j] = wv; w_sqrt[j] = sqrt(wv); }
        ORC_UPDATE_MU();
        const double gsize = 1.0 / alpha;
        const int gfast = (alpha > 0.0) && isfinite(alpha) && isfinite(gsize) && (gsize > 0.0);
        const double gK = maxit > 0 ? irls_constants(m, yrow, nfrow, wts, useWeights, alpha, gsize, gfast, sum_mode) : 0.0;
        double dev = 0.0, dev_old = 0.0;                                         /* :329-330 */
        double it = 0.0;
        for (int t = 0; t < maxit; t++) {                                        /* :334 / :388 */
            it += 1.0;                                                           /* :335 / :389 */
            ORC_UPDATE_W();
            for (int j = 0; j < m; j++)                                          /* :349 / :397 */
                z[j] = orc_log(mu[j] / nfrow[j]) + (yrow[j] - mu[j]) / mu[j];
            if (useQR) {
                /* weighted_x_ridge = join_cols(x.each_col() % w_sqrt_vec, sqrt(ridge)) :344 */
                for (int j = 0; j < m; j++) {
                    for (int c = 0; c < p; c++) A[(long)j * p + c] = x[j + (long)m * c] * w_sqrt[j];
                    bb[j] = z[j] * w_sqrt[j];                                    /* :351-353 */
                }
                for (int r = 0; r < p; r++) {
                    for (int c = 0; c < p; c++) A[(long)(m + r) * p + c] = (r == c) ? sqrt(lambda[c]) : 0.0;
                    bb[m + r] = 0.0;
                }
                householder_ls(M, p, A, bb, beta_hat, sum_mode);                 /* :345-356 */
            } else {
                /* solve(beta_hat, x.t() * (x.each_col() % w_vec) + ridge, x.t() * (z % w_vec)) :398 */
                double G[ORC_PMAX * ORC_PMAX], rhs[ORC_PMAX];
                for (int a = 0; a < p; a++) {
                    for (int b = a; b < p; b++) {
                        wsum_t s; wsum_init(&s, sum_mode);
                        for (int j = 0; j < m; j++)
                            wsum_add(&s, j, x[j + (long)m * a] * (x[j + (long)m * b] * w_vec[j]));
                        double v = wsum_total(&s);
                        G[a * p + b] = v; G[b * p + a] = v;
                    }
                    wsum_t s; wsum_init(&s, sum_mode);
                    for (int j = 0; j < m; j++) wsum_add(&s, j, x[j + (long)m * a] * (z[j] * w_vec[j]));
                    rhs[a] = wsum_total(&s);
                }
                for (int a = 0; a < p; a++) G[a * p + a] = G[a * p + a] + lambda[a];
                int piv[ORC_PMAX]; double rdiag[ORC_PMAX];
                lu_decomp(p, G, piv, rdiag);
                lu_solve(p, G, piv, rdiag, rhs);
                for (int a = 0; a < p; a++) beta_hat[a] = rhs[a];
            }
            int toolarge = 0;                                                    /* :357 / :399 */
            for (int c = 0; c < p; c++) if (fabs(beta_hat[c]) > large) toolarge++;
            if (toolarge > 0) { it = (double)maxit; break; }                     /* :358-359 */
            ORC_UPDATE_MU();                                                     /* :361-364 */
            /* :365-373  dev = -2 sum [wts] log NB(y; 1/alpha, mu) = -2 (K + D): the closed split of the cell path (see
             * fit_beta_gene_cells), lg = log(mu/nf) -- the value z uses */
            wsum_t s; wsum_init(&s, sum_mode);
            for (int j = 0; j < m; j++) {
                double tj;
                if (cell_dev_class(yrow[j], gsize, gfast) == 0) {
                    const double am = alpha * mu[j], opm = 1.0 + am, rcp = 1.0 / opm;
                    const double l1p = orc_log(opm) + (am - (opm - 1.0)) * rcp;
                    tj = yrow[j] * orc_log(mu[j] / nfrow[j]) - (yrow[j] + gsize) * l1p;
                } else tj = orc_dnbinom_mu_log(yrow[j], gsize, mu[j]);
                wsum_add(&s, j, useWeights ? wts[j] * tj : tj);
            }
            dev = -2.0 * (gK + wsum_total(&s));
            double conv_test = fabs(dev - dev_old) / (fabs(dev) + 0.1);          /* :374 */
            if (isnan(conv_test)) { it = (double)maxit; break; }                 /* :375-378 */
            if ((t > 0) & (conv_test < tol)) break;                              /* :379-381 */
            dev_old = dev;                                                       /* :382 */
        }
        deviance[i] = dev;                                                       /* :427 */
        for (int c = 0; c < p; c++) beta_mat[i + (long)n * c] = beta_hat[c];     /* :428 */
        iter[i] = it;
        ORC_UPDATE_W();                                                          /* :430-436 */
        /* xtwxr_inv = (x.t() * (x.each_col() % w_vec) + ridge).i()                :439 */
        double G[ORC_PMAX * ORC_PMAX], Gr[ORC_PMAX * ORC_PMAX], Gi[ORC_PMAX * ORC_PMAX];
        for (int a = 0; a < p; a++)
            for (int b = a; b < p; b++) {
                wsum_t s; wsum_init(&s, sum_mode);
                for (int j = 0; j < m; j++)
                    wsum_add(&s, j, x[j + (long)m * a] * (x[j + (long)m * b] * w_vec[j]));
                double v = wsum_total(&s);
                G[a * p + b] = v; G[b * p + a] = v;
            }
        memcpy(Gr, G, sizeof(double) * p * p);
        for (int a = 0; a < p; a++) Gr[a * p + a] = Gr[a * p + a] + lambda[a];
        mat_inverse(p, Gr, Gi, NULL);
        /* hat diagonal, loop order of :443-449 */
        for (int jp = 0; jp < m; jp++) {
            double h = 0.0;
            for (int idx1 = 0; idx1 < p; idx1++)
                for (int idx2 = 0; idx2 < p; idx2++) {
                    double xw1 = x[jp + (long)m * idx1] * w_sqrt[jp];
                    double xw2 = x[jp + (long)m * idx2] * w_sqrt[jp];
                    h += xw1 * (xw2 * Gi[idx2 * p + idx1]);
                }
            hat_diagonals[i + (long)n * jp] = h;                                 /* :450 */
        }
        /* sigma = Gi * G * Gi                                                     :452 */
        double T[ORC_PMAX * ORC_PMAX], Sg[ORC_PMAX * ORC_PMAX];
        mat_mul(p, Gi, G, T); mat_mul(p, T, Gi, Sg);
        double cn = 0.0;                                                         /* :453 */
        for (int c = 0; c < p; c++) cn = fma(contrast[c], beta_hat[c], cn);
        contrast_num[i] = cn;
        double cd = 0.0;                                                         /* :454 */
        for (int b = 0; b < p; b++) {
            double r = 0.0;
            for (int a = 0; a < p; a++) r = fma(contrast[a], Sg[a * p + b], r);
            cd = fma(r, contrast[b], cd);
        }
        contrast_denom[i] = sqrt(cd);
        for (int c = 0; c < p; c++) beta_var_mat[i + (long)n * c] = Sg[c * p + c];   /* :455 */
    }
    free(yrow); free(nfrow); free(wts); free(mu); free(w_vec); free(w_sqrt); free(z); free(A); free(bb);
    }
    free(cperm); free(xc);
    return 0;
}

/* ================================================ rows the IRLS did not fit ==
 * R/fitNbinomGLMs.R:340-407 (fitNbinomGLMsOptim): rows with betaConv = FALSE, NA coefficients or a non-positive
 * variance are re-fitted by maximising the penalised log posterior  sum [w] log NB(y; mu = nf 2^(x beta), 1/alpha) +
 * sum log N(beta_k; 0, 1/lambda_k)  over beta in [-30, 30]^p.  The reference hands this to stats::optim(method =
 * "L-BFGS-B") with a numerical gradient -- R's lbfgsb.c is not in the reference tree and its iterates cannot be
 * reproduced.  The engine maximises the SAME objective over the SAME box with a damped Fisher-scoring iteration
 * (analytic score X'[w (y - mu)/(1 + alpha mu)] - ridge beta, information X' diag(w mu/(1 + alpha mu)) X + ridge,
 * step halving until the objective decreases, projection onto the box), which converges to the same optimum; the
 * test suite checks its objective value against scipy's L-BFGS-B on the same rows.  betaConv = the relative decrease
 * fell under 1e-10 (or no descent step exists) within 100 iterations (optim's convergence == 0).  Everything after
 * the optimum -- mu, betaSE from (X'WX + ridge)^-1 X'WX (X'WX + ridge)^-1 at mu clamped to minmu, logLike at the
 * clamped mu -- follows :382-400.  Natural-log scale inside, log2 in and out like the reference.  Wave-order sums. */
static double optim_objective(int m, int p, const double *x, const double *yrow, const double *nfrow, const double *wts,
                              int useWeights, double size, const double *lamnat, const double *gam, int sum_mode) {
    wsum_t s; wsum_init(&s, sum_mode);
    for (int j = 0; j < m; j++) {
        double eta = x[j] * gam[0];
        for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], gam[c], eta);
        double d = orc_dnbinom_mu_log(yrow[j], size, nfrow[j] * orc_exp(eta));
        wsum_add(&s, j, useWeights ? wts[j] * d : d);
    }
    double pen = 0.0;
    for (int c = 0; c < p; c++) pen = fma(0.5 * lamnat[c], gam[c] * gam[c], pen);
    double f = pen - wsum_total(&s);
    return isfinite(f) ? f : 1e300;                                             /* :369 */
}

int orc_optim_rows(int n, int m, int p, const double *y, const double *x, const double *nf, const double *alpha_hat,
                   const double *lamnat, const double *weights, int useWeights, const double *beta_start, double minmu,
                   double *beta_out, double *betaSE, int *conv, double *mu_out, double *loglike, int sum_mode) {
    if (p > ORC_PMAX) return -1;
    const double ln2 = 0.6931471805599453, log2e = 1.4426950408889634;
    const double bound = 30.0 * ln2;
#pragma omp parallel
    {
    double *yrow = malloc(sizeof(double) * m), *nfrow = malloc(sizeof(double) * m), *wts = malloc(sizeof(double) * m);
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {
        double gam[ORC_PMAX], trial[ORC_PMAX];
        for (int j = 0; j < m; j++) {
            yrow[j] = y[i + (long)n * j]; nfrow[j] = nf[i + (long)n * j];
            wts[j] = weights ? weights[i + (long)n * j] : 1.0;
        }
        const double alpha = alpha_hat[i], size = 1.0 / alpha;
        for (int c = 0; c < p; c++) gam[c] = fmin(fmax(beta_start[i + (long)n * c] * ln2, -bound), bound);
        double F = optim_objective(m, p, x, yrow, nfrow, wts, useWeights, size, lamnat, gam, sum_mode);
        int converged = 0;
        for (int it = 0; it < 100 && !converged; it++) {
            double G[ORC_PMAX * ORC_PMAX], rhs[ORC_PMAX];
            for (int a = 0; a < p; a++) {
                for (int b = a; b < p; b++) {
                    wsum_t s; wsum_init(&s, sum_mode);
                    for (int j = 0; j < m; j++) {
                        double eta = x[j] * gam[0];
                        for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], gam[c], eta);
                        double mu = nfrow[j] * orc_exp(eta);
                        double wv = useWeights ? (wts[j] * mu) / (1.0 + alpha * mu) : mu / (1.0 + alpha * mu);
                        wsum_add(&s, j, x[j + (long)m * a] * (x[j + (long)m * b] * wv));
                    }
                    double v = wsum_total(&s);
                    G[a * p + b] = v; G[b * p + a] = v;
                }
                wsum_t s; wsum_init(&s, sum_mode);
                for (int j = 0; j < m; j++) {
                    double eta = x[j] * gam[0];
                    for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], gam[c], eta);
                    double mu = nfrow[j] * orc_exp(eta);
                    double rv = useWeights ? (wts[j] * (yrow[j] - mu)) / (1.0 + alpha * mu) : (yrow[j] - mu) / (1.0 + alpha * mu);
                    wsum_add(&s, j, x[j + (long)m * a] * rv);
                }
                rhs[a] = wsum_total(&s) - lamnat[a] * gam[a];
            }
            for (int a = 0; a < p; a++) G[a * p + a] = G[a * p + a] + lamnat[a];
            int piv[ORC_PMAX]; double rdiag[ORC_PMAX];
            lu_decomp(p, G, piv, rdiag);
            lu_solve(p, G, piv, rdiag, rhs);                       /* rhs <- Fisher-scoring step */
            double t = 1.0, Ft = 0.0;
            int accepted = 0;
            for (int h = 0; h < 40; h++) {
                for (int c = 0; c < p; c++) trial[c] = fmin(fmax(gam[c] + t * rhs[c], -bound), bound);
                Ft = optim_objective(m, p, x, yrow, nfrow, wts, useWeights, size, lamnat, trial, sum_mode);
                if (Ft < F) { accepted = 1; break; }
                t = t * 0.5;
            }
            if (!accepted) { converged = 1; break; }               /* no descent along the scoring direction */
            double dec = F - Ft;
            for (int c = 0; c < p; c++) gam[c] = trial[c];
            F = Ft;
            if (dec <= 1e-10 * (fabs(F) + 1e-10)) converged = 1;
        }
        conv[i] = converged;
        /* :382-400 */
        double G[ORC_PMAX * ORC_PMAX], Gr[ORC_PMAX * ORC_PMAX], Gi[ORC_PMAX * ORC_PMAX], T[ORC_PMAX * ORC_PMAX], Sg[ORC_PMAX * ORC_PMAX];
        for (int a = 0; a < p; a++)
            for (int b = a; b < p; b++) {
                wsum_t s; wsum_init(&s, sum_mode);
                for (int j = 0; j < m; j++) {
                    double eta = x[j] * gam[0];
                    for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], gam[c], eta);
                    double muc = fmax(nfrow[j] * orc_exp(eta), minmu);
                    double wv = useWeights ? wts[j] / (1.0 / muc + alpha) : 1.0 / (1.0 / muc + alpha);
                    wsum_add(&s, j, x[j + (long)m * a] * (x[j + (long)m * b] * wv));
                }
                double v = wsum_total(&s);
                G[a * p + b] = v; G[b * p + a] = v;
            }
        memcpy(Gr, G, sizeof(double) * p * p);
        for (int a = 0; a < p; a++) Gr[a * p + a] = Gr[a * p + a] + lamnat[a];
        mat_inverse(p, Gr, Gi, NULL);
        mat_mul(p, Gi, G, T); mat_mul(p, T, Gi, Sg);
        wsum_t sl; wsum_init(&sl, sum_mode);
        for (int j = 0; j < m; j++) {
            double eta = x[j] * gam[0];
            for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], gam[c], eta);
            double mu = nfrow[j] * orc_exp(eta);
            mu_out[i + (long)n * j] = mu;
            double d = orc_dnbinom_mu_log(yrow[j], size, fmax(mu, minmu));
            wsum_add(&sl, j, useWeights ? wts[j] * d : d);
        }
        loglike[i] = wsum_total(&sl);
        for (int c = 0; c < p; c++) {
            beta_out[i + (long)n * c] = log2e * gam[c];
            betaSE[i + (long)n * c] = log2e * sqrt(fmax(Sg[c * p + c], 0.0));
        }
    }
    free(yrow); free(nfrow); free(wts);
    }
    return 0;
}

/* ======================================================== nbinomLogLike ==
 * R/core.R:2208-2217: rowSums([weights *] dnbinom(counts, mu = mu, size = 1/disp, log = TRUE)).
 * (called from R/fitNbinomGLMs.R:182 and, per model, from nbinomLRT R/core.R:1850-1877)
 * dnbinom(.., mu=) is nmath's dnbinom_mu, the same function fitBeta's deviance uses. */
/* Round 4: evaluated on the closed split of the density that fitBeta's deviance uses (fit_beta_gene_cells above):
 *   log f_j = K'_j + y_j log mu_j - (y_j + size) log1p(alpha mu_j),
 *   K'_j = [saddle-point constants, logarithms folded] + n log1p(alpha y) - y log y   (0 for y = 0; the K_j of the
 *   deviance without its y log nf_j -- the likelihood is given mu, not nf),
 * a sample outside the split (cell_dev_class != 0) keeps dnbinom_mu.  The row's value is K' + D: two sums over the samples
 * in their natural order, added once.  Against 40-digit arithmetic the split's terms cancel four to five digits where
 * dnbinom_mu's bd0 loses none (error ~ 4e-12 on a log likelihood of -430 against 5e-13); at the dispersion floor (size 1e8)
 * dnbinom_mu's log1p(-x/n) loses nine (~ 6e-10 per sample, a term of (y, size): the same in every model of a gene) and
 * the split none -- tests/test_loglike_cpu.py pins all three.  The engine pays a third of the instructions. */
int orc_nbinom_loglike(int n, int m, const double *y, const double *mu, const double *disp,
                       const double *weights, int useWeights, double *loglike, int sum_mode) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++) {
        const double alpha = disp[i], size = 1.0 / alpha;
        const int fast = (alpha > 0.0) && isfinite(alpha) && isfinite(size) && (size > 0.0);
        const double st_size = fast ? orc_stirlerr(size) : 0.0;
        wsum_t sk, sd; wsum_init(&sk, sum_mode); wsum_init(&sd, sum_mode);
        for (int j = 0; j < m; j++) {
            const double yy = y[i + (long)n * j], mm = mu[i + (long)n * j];
            const double w = useWeights ? weights[i + (long)n * j] : 1.0;
            const int cls = cell_dev_class(yy, size, fast);
            double kj = 0.0, d;
            if (cls == 0) {
                if (yy != 0.0) {
                    const double nn = yy + size;
                    const double L = orc_log1p(alpha * yy), ly = orc_log(yy);
                    const double c0 = orc_stirlerr(nn) - st_size - orc_stirlerr(nn - size);
                    kj = (-L + (c0 - 0.5 * (1.837877066409345483560659472811 /* ln 2 pi */ + ly - L))) + (nn * L - yy * ly);
                }
                const double am = alpha * mm, opm = 1.0 + am, rcp = 1.0 / opm;
                const double l1p = orc_log(opm) + (am - (opm - 1.0)) * rcp;
                d = (yy == 0.0) ? -(size * l1p) : yy * orc_log(mm) - (yy + size) * l1p;
            } else d = orc_dnbinom_mu_log(yy, size, mm);
            if (fast) wsum_add(&sk, j, useWeights ? w * kj : kj);
            wsum_add(&sd, j, useWeights ? w * d : d);
        }
        loglike[i] = (fast ? wsum_total(&sk) : 0.0) + wsum_total(&sd);
    }
    return 0;
}

/* ========================================================= pre-fit moments ==
 * The O(n m p) host steps that feed the native fits, one pass per gene:
 *   baseMean, baseVar, allZero     getBaseMeansAndVariances   R/core.R:2138-2146
 *   roughDisp                      roughDispEstimate          R/core.R:2422-2437
 *                                  (linearModelMu :2454-2463: mu = (y Q)(X R^-1)')
 *   beta_init                      QR least squares on log(K/s + 0.1), R/fitNbinomGLMs.R:139-145
 * q  : m x p (column-major) thin-QR Q of the model matrix,  a : m x p = X R^-1,
 * r  : p x p upper-triangular R (column-major).  All three are computed by the caller from the
 * m x p design (stats::qr in the reference).  Weights only enter baseMean / baseVar (:2140-2143).
 * Sums over samples in wave order; rowVars as the two-pass sum((x-mean)^2)/(m-1).           */
int orc_prefit_moments(int n, int m, int p, const double *y, const double *nf, const double *weights,
                       int useWeights, const double *q, const double *a, const double *r,
                       double *baseMean, double *baseVar, int *allZero, double *roughDisp,
                       double *beta_init, int sum_mode) {
    if (p > ORC_PMAX) return -1;
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++) {
        double t[ORC_PMAX], u[ORC_PMAX];
        wsum_t sm, sy; wsum_init(&sm, sum_mode); wsum_init(&sy, sum_mode);
        for (int j = 0; j < m; j++) {
            double yy = y[i + (long)n * j];
            double cn = yy / nf[i + (long)n * j];
            if (useWeights) cn = weights[i + (long)n * j] * cn;
            wsum_add(&sm, j, cn); wsum_add(&sy, j, yy);
        }
        double mean = wsum_total(&sm) / (double)m;
        baseMean[i] = mean;
        allZero[i] = (wsum_total(&sy) == 0.0);
        wsum_t sv; wsum_init(&sv, sum_mode);
        for (int j = 0; j < m; j++) {
            double cn = y[i + (long)n * j] / nf[i + (long)n * j];
            if (useWeights) cn = weights[i + (long)n * j] * cn;
            double dlt = cn - mean;
            wsum_add(&sv, j, dlt * dlt);
        }
        baseVar[i] = wsum_total(&sv) / (double)(m - 1);
        /* t = yn' Q ; u = log(yn + 0.1)' Q */
        for (int c = 0; c < p; c++) {
            wsum_t s1, s2; wsum_init(&s1, sum_mode); wsum_init(&s2, sum_mode);
            for (int j = 0; j < m; j++) {
                double yn = y[i + (long)n * j] / nf[i + (long)n * j];
                wsum_add(&s1, j, yn * q[j + (long)m * c]);
                wsum_add(&s2, j, orc_log(yn + 0.1) * q[j + (long)m * c]);
            }
            t[c] = wsum_total(&s1); u[c] = wsum_total(&s2);
        }
        wsum_t se; wsum_init(&se, sum_mode);
        for (int j = 0; j < m; j++) {
            double yn = y[i + (long)n * j] / nf[i + (long)n * j];
            double mu = t[0] * a[j];
            for (int c = 1; c < p; c++) mu = fma(t[c], a[j + (long)m * c], mu);
            mu = fmax(1.0, mu);                                                  /* :2426 */
            double d = yn - mu;
            wsum_add(&se, j, (d * d - mu) / (mu * mu));                          /* :2435 */
        }
        roughDisp[i] = fmax(wsum_total(&se) / (double)(m - p), 0.0);             /* :2435-2436 */
        /* beta_init = solve(R, u): back substitution */
        double b[ORC_PMAX];
        for (int c = p - 1; c >= 0; c--) {
            double v = u[c];
            for (int k = c + 1; k < p; k++) v = fma(-r[c + (long)p * k], b[k], v);
            b[c] = v / r[c + (long)p * c];
        }
        for (int c = 0; c < p; c++) beta_init[i + (long)n * c] = b[c];
    }
    return 0;
}

/* linearModelMuNormalized (R/core.R:2454-2471): mu = nf * ((yn Q) (X R^-1)'), floored at mu_floor when > 0
 * (R/core.R:763).  q = Q, a = X R^-1 of the thin QR of the design; same sums as the moments above. */
int orc_linear_mu(int n, int m, int p, const double *y, const double *nf, const double *q, const double *a,
                  double mu_floor, double *mu, int sum_mode) {
    if (p > ORC_PMAX) return -1;
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++) {
        double t[ORC_PMAX];
        for (int c = 0; c < p; c++) {
            wsum_t s1; wsum_init(&s1, sum_mode);
            for (int j = 0; j < m; j++) wsum_add(&s1, j, (y[i + (long)n * j] / nf[i + (long)n * j]) * q[j + (long)m * c]);
            t[c] = wsum_total(&s1);
        }
        for (int j = 0; j < m; j++) {
            double v = t[0] * a[j];
            for (int c = 1; c < p; c++) v = fma(t[c], a[j + (long)m * c], v);
            v = v * nf[i + (long)n * j];
            if (mu_floor > 0.0) v = fmax(v, mu_floor);
            mu[i + (long)n * j] = v;
        }
    }
    return 0;
}

/* fitted means from the final coefficients: mu = nf * exp(x beta) (R/fitNbinomGLMs.R:180), optionally
 * floored (R/core.R:763).  eta is accumulated as in fitBeta (:324), exp is the restated one.   */
int orc_fitted_mu(int n, int m, int p, const double *x, const double *nf, const double *beta,
                  double mu_floor, double *mu) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) {
            double eta = x[j] * beta[i];
            for (int c = 1; c < p; c++) eta = fma(x[j + (long)m * c], beta[i + (long)n * c], eta);
            double v = nf[i + (long)n * j] * orc_exp(eta);
            if (mu_floor > 0.0) v = fmax(v, mu_floor);
            mu[i + (long)n * j] = v;
        }
    return 0;
}

/* ================================================ intercept-only closed form ==
 * R/fitNbinomGLMs.R:99-137: design ~ 1 with the wide prior needs no IRLS.
 *   betaMatrix = log2(mean of normalized counts)   [weighted: sum(w K/s) / sum(w)]     (:104-111)
 *   mu = nf * 2^beta                                                                      (:112)
 *   w = [weights] (mu^-1 + alpha)^-1 ; xtwx = rowSums(w) ; sigma = xtwx^-1               (:118-124)
 *   betaSE = log2(e) sqrt(sigma) ; hat = w * xtwx^-1                                      (:125-126)
 * Restated on the natural-log scale with the engine's log / exp: b = log(mean), betaMatrix = log2(e) b,
 * mu = nf exp(b).  mu_out (optional) is floored at mu_floor when > 0 (the caller's fitMu[fitMu < minmu] <- minmu,
 * R/core.R:763); betaSE / hat use the unfloored mu, as in R.  Sums over samples in wave order.   */
int orc_intercept_fit(int n, int m, const double *y, const double *nf, const double *weights, int useWeights,
                      const double *alpha, double mu_floor, double *beta_log2, double *betaSE, double *mu_out,
                      double *hat, int sum_mode) {
    const double log2e = 1.4426950408889634;
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; i++) {
        wsum_t s1, s0; wsum_init(&s1, sum_mode); wsum_init(&s0, sum_mode);
        for (int j = 0; j < m; j++) {
            double cn = y[i + (long)n * j] / nf[i + (long)n * j];
            if (useWeights) { double w = weights[i + (long)n * j]; cn = w * cn; wsum_add(&s0, j, w); }
            wsum_add(&s1, j, cn);
        }
        double mean = wsum_total(&s1) / (useWeights ? wsum_total(&s0) : (double)m);
        double b = orc_log(mean);
        double eb = orc_exp(b);
        wsum_t sw; wsum_init(&sw, sum_mode);
        for (int j = 0; j < m; j++) {
            double mu = nf[i + (long)n * j] * eb;
            double wd = 1.0 / (1.0 / mu + alpha[i]);
            if (useWeights) wd = weights[i + (long)n * j] * wd;
            wsum_add(&sw, j, wd);
        }
        double xtwx = wsum_total(&sw);
        beta_log2[i] = log2e * b;
        betaSE[i] = log2e * sqrt(1.0 / xtwx);
        for (int j = 0; j < m; j++) {
            double mu = nf[i + (long)n * j] * eb;
            if (hat) {
                double wd = 1.0 / (1.0 / mu + alpha[i]);
                if (useWeights) wd = weights[i + (long)n * j] * wd;
                hat[i + (long)n * j] = wd / xtwx;
            }
            if (mu_out) mu_out[i + (long)n * j] = (mu_floor > 0.0) ? fmax(mu, mu_floor) : mu;
        }
    }
    return 0;
}

/* ==================================================== fitType = "mean" ==
 * R/core.R:894-899: mean(dispGeneEst[dispGeneEst > 10 minDisp], na.rm = TRUE, trim = 0.001).  base::mean.default drops
 * floor(N trim) order statistics from either end and hands the rest to a long-double mean with a correction pass: to
 * double precision the correctly rounded mean of the kept values.  The shared specification of kernel, mirror and this
 * restatement: every kept value as the integer floor(x 2^128) (exact from 2^-75 up), the integers added exactly, the
 * quotient by the count rounded ONCE to nearest-even -- no order of summation to specify.  Means below 2^-75 (no
 * dispersion estimate is: minDisp = 1e-8) are the truncated quotient.  Returns the number of kept values (0: none).  */
static int cmp_double(const void *a, const void *b) {
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}
long orc_trimmed_mean_fit(long n, const double *disps, double minDisp, double *mean_out) {
    double *v = malloc((n > 0 ? n : 1) * sizeof(double));
    long N = 0;
    for (long i = 0; i < n; i++) if (disps[i] > 10.0 * minDisp) v[N++] = disps[i];       /* (NaN: dropped, na.rm) */
    *mean_out = NAN;
    if (N == 0) { free(v); return 0; }
    qsort(v, N, sizeof(double), cmp_double);
    const long k = (long)floor((double)N * 0.001);
    const long lo = k, hi = N - k;                       /* kept: v[lo .. hi) */
    const long cnt = hi - lo;
    /* sum of floor(x 2^128): the low 64 bits and the part above them accumulated apart (no carries to propagate) */
    unsigned __int128 low = 0, high = 0;
    for (long i = lo; i < hi; i++) {
        int e;
        const double fr = frexp(v[i], &e);               /* x = fr 2^e, fr in [0.5, 1) */
        const unsigned long long M = (unsigned long long)ldexp(fr, 53);       /* 53-bit integer */
        const int sh = e - 53 + 128;                     /* floor(x 2^128) = M 2^sh */
        if (sh >= 64) high += (unsigned __int128)M << (sh - 64);
        else if (sh >= 0) { high += (unsigned __int128)(sh ? M >> (64 - sh) : 0); low += (unsigned long long)(M << sh); }
        else if (-sh < 64) low += M >> (-sh);
    }
    high += low >> 64;
    const unsigned long long low64 = (unsigned long long)low;
    /* (high 2^64 + low64) / cnt by two-limb long division */
    const unsigned __int128 qh = high / (unsigned long)cnt, r1 = high % (unsigned long)cnt;
    const unsigned __int128 t = (r1 << 64) | low64;
    const unsigned long long ql = (unsigned long long)(t / (unsigned long)cnt);
    const int inexact = (t % (unsigned long)cnt) != 0;
    /* the quotient's 53 leading bits, round to nearest, ties to even */
    int h = -1;
    for (int b = 127; b >= 0 && h < 0; b--) if ((qh >> b) & 1) h = b + 64;
    for (int b = 63; b >= 0 && h < 0; b--) if ((ql >> b) & 1) h = b;
    if (h < 0) { *mean_out = 0.0; free(v); return cnt; }
#define QBIT(i) ((i) >= 64 ? (int)((qh >> ((i) - 64)) & 1) : (int)((ql >> (i)) & 1))
    double mean;
    if (h <= 52) mean = ldexp((double)ql, -128);
    else {
        const int shift = h - 52;
        unsigned long long mant = 0;
        for (int b = 52; b >= 0; b--) mant = (mant << 1) | (unsigned)QBIT(shift + b);
        int below = inexact;
        for (int i = 0; i < shift - 1 && !below; i++) below = QBIT(i);
        if (QBIT(shift - 1) && (below || (mant & 1))) mant++;
        mean = ldexp((double)mant, shift - 128);
    }
#undef QBIT
    *mean_out = mean;
    free(v);
    return cnt;
}

/* ==================================================== parametricDispersionFit ==
 * R/core.R:2166-2190: disps ~ asymptDisp + extraPois / means by stats::glm(family =
 * Gamma(link = "identity"), start = coefs) inside the outlier-filter loop.  glm.fit's IRLS is
 * restated for this two-column model: working response = y, working weights = 1/mu^2, stop when
 * |dev - devold| / (|dev| + 0.1) < 1e-8 (glm.control), at most 25 iterations; devold starts at the
 * deviance of the start values.  Sums over the genes in BLOCK ORDER: 16384 partial sums, partial q
 * taking elements q, q+16384, ...; q = (block 0..15, wave 0..15, lane 0..63).  The 64 partials of a wave
 * are butterflied (xor 1..32), the 16 wave sums of a block added in order, then the 16 block sums added
 * in order -- the order the 16-workgroup kernel uses, independent of the number of genes.
 * status: 0 ok, 1 "parametric dispersion fit failed" (a coefficient <= 0 or an invalid mean),
 * 2 "dispersion fit did not converge" (more than 10 outer rounds).                            */
#define BSUM_PARTS 16384
typedef struct { double part[BSUM_PARTS]; } bsum_t;
static void bsum_init(bsum_t *s) { for (int t = 0; t < BSUM_PARTS; t++) s->part[t] = 0.0; }
static double bsum_total(const bsum_t *s) {
    double grand = 0.0;
    for (int b = 0; b < 16; b++) {
        double tot = 0.0;
        for (int g = 0; g < 16; g++) {
            double v[64], w[64];
            memcpy(v, s->part + 1024 * b + 64 * g, sizeof v);
            for (int off = 1; off < 64; off <<= 1) {
                for (int l = 0; l < 64; l++) w[l] = v[l] + v[l ^ off];
                memcpy(v, w, sizeof v);
            }
            tot = (g == 0) ? v[0] : tot + v[0];
        }
        grand = (b == 0) ? tot : grand + tot;
    }
    return grand;
}

int orc_parametric_dispersion_fit(long n, const double *means, const double *disps, double *coefs_out,
                                  int *status) {
    double c0 = 0.1, c1 = 1.0;
    unsigned char *good = malloc(n > 0 ? n : 1);
    int iter = 0;
    *status = 0;
    for (;;) {
        for (long i = 0; i < n; i++) {
            double res = disps[i] / (c0 + c1 / means[i]);                          /* :2170 */
            good[i] = (res > 1e-4) && (res < 15.0);                                /* :2171 */
        }
        double b0 = c0, b1 = c1;
        int converged = 0, invalid = 0;
        double devold = 0.0;
        for (int pass = -1; pass < 25 && !invalid; pass++) {
            if (pass >= 0) {
                /* weighted least squares step */
                bsum_t *bs = malloc(5 * sizeof(bsum_t));
#define s0 bs[0]
#define s1 bs[1]
#define s2 bs[2]
#define t0 bs[3]
#define t1 bs[4]
                bsum_init(&s0); bsum_init(&s1); bsum_init(&s2); bsum_init(&t0); bsum_init(&t1);
                for (long i = 0; i < n; i++) {
                    if (!good[i]) continue;
                    double x = 1.0 / means[i], y = disps[i];
                    double mu = b0 + b1 * x;
                    double wgt = 1.0 / (mu * mu);
                    double wx = wgt * x;
                    int t = (int)(i & (BSUM_PARTS - 1));
                    s0.part[t] += wgt; s1.part[t] += wx; s2.part[t] += wx * x;
                    t0.part[t] += wgt * y; t1.part[t] += wx * y;
                }
                double S0 = bsum_total(&s0), S1 = bsum_total(&s1), S2 = bsum_total(&s2);
                double T0 = bsum_total(&t0), T1 = bsum_total(&t1);
#undef s0
#undef s1
#undef s2
#undef t0
#undef t1
                free(bs);
                double det = S0 * S2 - S1 * S1;
                b0 = (S2 * T0 - S1 * T1) / det;
                b1 = (S0 * T1 - S1 * T0) / det;
            }
            /* deviance at the current coefficients (pass = -1: at the start values) */
            bsum_t *bd = malloc(2 * sizeof(bsum_t));
#define d1 bd[0]
#define d2 bd[1]
            bsum_init(&d1); bsum_init(&d2);
            for (long i = 0; i < n; i++) {
                if (!good[i]) continue;
                double mu = b0 + b1 * (1.0 / means[i]);
                if (!(mu > 0.0)) { invalid = 1; break; }
                double r = disps[i] / mu;
                int t = (int)(i & (BSUM_PARTS - 1));
                d1.part[t] += orc_log(r); d2.part[t] += r - 1.0;
            }
            double dsum1 = bsum_total(&d1), dsum2 = bsum_total(&d2);
#undef d1
#undef d2
            free(bd);
            if (invalid) break;
            double dev = -2.0 * (dsum1 - dsum2);
            if (pass >= 0 && fabs(dev - devold) / (fabs(dev) + 0.1) < 1e-8) { converged = 1; break; }
            devold = dev;
        }
        if (invalid) { *status = 1; break; }
        double o0 = c0, o1 = c1;
        c0 = b0; c1 = b1;
        if (!(c0 > 0.0 && c1 > 0.0)) { *status = 1; break; }                       /* :2177-2178 */
        double l0 = orc_log(c0 / o0), l1 = orc_log(c1 / o1);
        if ((l0 * l0 + l1 * l1 < 1e-6) && converged) break;                        /* :2179-2180 */
        iter++;
        if (iter > 10) { *status = 2; break; }                                     /* :2182-2183 */
    }
    coefs_out[0] = c0; coefs_out[1] = c1;
    free(good);
    return 0;
}

/* ============================================================ outlier machinery ==
 * calculateCooksDistance (R/core.R:2333-2340) with robustMethodOfMomentsDisp
 * (:2277-2299) / trimmedCellVariance (:2301-2324) / trimmedVariance (:2326-2331),
 * recordMaxCooks (:2349-2359) and replaceOutliers (:2069-2115).
 *
 * Cells = groups of identical model-matrix rows; `cell_of[j]` in 0..ncell-1 gives sample j's cell.
 * R's mean(x, trim): lo = floor(n*trim)+1, hi = n+1-lo, mean of the order statistics lo..hi.
 * The sum of those order statistics is taken in wave order over the RANK (sorted position),
 * partial l taking ranks lo-1+l, lo-1+l+64, ...                                               */
static int cmp_dbl(const void *a, const void *b) {
    double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}
static double trimmed_mean_sorted(const double *sorted, int n, double trim, int sum_mode) {
    int lo = (int)floor((double)n * trim) + 1, hi = n + 1 - lo;
    wsum_t s; wsum_init(&s, sum_mode);
    for (int r = lo; r <= hi; r++) wsum_add(&s, r - lo, sorted[r - 1]);
    return wsum_total(&s) / (double)(hi - lo + 1);
}
static int trimfn(int n) { return n <= 3 ? 0 : (n <= 23 ? 1 : 2); }      /* cut(n, c(0,3.5,23.5,Inf)) */

int orc_cooks_distance(int n, int m, int p, const double *y, const double *nf, const double *mu,
                       const double *H, const int *cell_of, int ncell,
                       double *cooks, double *maxCooks, double *robustDisp, int sum_mode) {
    static const double trimratio[3] = {1.0 / 3.0, 1.0 / 4.0, 1.0 / 8.0};
    static const double scale_c[3] = {2.04, 1.86, 1.51};
    int *csize = calloc(ncell, sizeof(int));
    for (int j = 0; j < m; j++) csize[cell_of[j]]++;
    int any3 = 0;
    for (int c = 0; c < ncell; c++) if (csize[c] >= 3) any3 = 1;
#pragma omp parallel
    {
    double *cn = malloc(sizeof(double) * m), *buf = malloc(sizeof(double) * m);
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {
        wsum_t sm; wsum_init(&sm, sum_mode);
        for (int j = 0; j < m; j++) { cn[j] = y[i + (long)n * j] / nf[i + (long)n * j]; wsum_add(&sm, j, cn[j]); }
        double mean_all = wsum_total(&sm) / (double)m;                        /* rowMeans(cnts) :2293 */
        double v;
        if (any3) {                                                          /* trimmedCellVariance */
            v = -INFINITY;
            for (int c = 0; c < ncell; c++) {
                int nc = csize[c];
                if (nc < 3) continue;
                int tf = trimfn(nc), k = 0;
                for (int j = 0; j < m; j++) if (cell_of[j] == c) buf[k++] = cn[j];
                qsort(buf, nc, sizeof(double), cmp_dbl);
                double cm = trimmed_mean_sorted(buf, nc, trimratio[tf], sum_mode);       /* :2305-2309 */
                k = 0;
                for (int j = 0; j < m; j++) if (cell_of[j] == c) { double d = cn[j] - cm; buf[k++] = d * d; }
                qsort(buf, nc, sizeof(double), cmp_dbl);
                double ve = scale_c[tf] * trimmed_mean_sorted(buf, nc, trimratio[tf], sum_mode);   /* :2313-2319 */
                if (ve > v) v = ve;                                          /* rowMax :2322 */
            }
        } else {                                                             /* trimmedVariance :2326 */
            memcpy(buf, cn, sizeof(double) * m);
            qsort(buf, m, sizeof(double), cmp_dbl);
            double rm = trimmed_mean_sorted(buf, m, 1.0 / 8.0, sum_mode);
            for (int j = 0; j < m; j++) { double d = cn[j] - rm; buf[j] = d * d; }
            qsort(buf, m, sizeof(double), cmp_dbl);
            v = 1.51 * trimmed_mean_sorted(buf, m, 1.0 / 8.0, sum_mode);
        }
        double alpha = (v - mean_all) / (mean_all * mean_all);               /* :2294 */
        alpha = fmax(alpha, 0.04);                                           /* :2297-2298 */
        robustDisp[i] = alpha;
        double mx = -INFINITY; int anyc = 0;
        for (int j = 0; j < m; j++) {
            double mj = mu[i + (long)n * j], hj = H[i + (long)n * j], yj = y[i + (long)n * j];
            double V = mj + alpha * (mj * mj);                                /* :2336 */
            double d = yj - mj;
            double pr = (d * d) / V;                                         /* :2337 */
            double omh = 1.0 - hj;
            double ck = pr / (double)p * hj / (omh * omh);                   /* :2338 */
            cooks[i + (long)n * j] = ck;
            if (csize[cell_of[j]] >= 3) { anyc = 1; if (ck > mx || ck != ck) mx = (ck != ck) ? ck : (mx != mx ? mx : ck); }
        }
        maxCooks[i] = (m > p && anyc) ? mx : NAN;                            /* :2353-2357 */
    }
    free(cn); free(buf);
    }
    free(csize);
    return 0;
}

/* replaceOutliers, R/core.R:2069-2115: counts with a Cook's distance above the cutoff are
 * replaced by as.integer(trimmed mean (trim = .2) of the normalized counts * nf) in the samples
 * whose cell has >= minReplicates members; `replace` flags genes with ANY distance above it. */
int orc_replace_outliers(int n, int m, const double *y, const double *nf, const double *cooks,
                         double cooksCutoff, const int *replaceable, double trim,
                         int *newCounts, int *replace, int sum_mode) {
#pragma omp parallel
    {
    double *buf = malloc(sizeof(double) * m);
#pragma omp for schedule(static)
    for (int i = 0; i < n; i++) {
        int any = 0;
        for (int j = 0; j < m; j++) {
            buf[j] = y[i + (long)n * j] / nf[i + (long)n * j];
            if (cooks[i + (long)n * j] > cooksCutoff) any = 1;
        }
        replace[i] = any;                                                    /* :2086 */
        qsort(buf, m, sizeof(double), cmp_dbl);
        double tbm = trimmed_mean_sorted(buf, m, trim, sum_mode);            /* :2088 */
        for (int j = 0; j < m; j++) {
            int orig = (int)y[i + (long)n * j];
            int rep = (int)(tbm * nf[i + (long)n * j]);                      /* as.integer: truncation, :2090-2095 */
            newCounts[i + (long)n * j] =
                (cooks[i + (long)n * j] > cooksCutoff && replaceable[j]) ? rep : orig;   /* :2098-2112 */
        }
    }
    free(buf);
    }
    return 0;
}
