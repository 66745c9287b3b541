/*
 * deseq2_mi355x.h -- C ABI of libdeseq2_mi355x.so, the MI355X (gfx950) engine that
 * replaces the three native entry points of thelovelab/DESeq2:
 *
 *   reference routine (src/RcppExports.cpp:84-89)      replaced by
 *   _DESeq2_fitBeta      (src/DESeq2.cpp:283-465)      dsq_fit_beta      / dsq_fit_beta_dev
 *   _DESeq2_fitDisp      (src/DESeq2.cpp:164-277)      dsq_fit_disp      / dsq_fit_disp_dev
 *   _DESeq2_fitDispGrid  (src/DESeq2.cpp:469-513)      dsq_fit_disp_grid / dsq_fit_disp_grid_dev
 *
 * Plain pointers and sizes only.  Two families:
 *   dsq_fit_*      : every array pointer is a HOST pointer in R's layout (what a
 *                    .Call shim gets from REAL()/INTEGER()); the call uploads, runs
 *                    the HIP kernels, downloads and returns synchronously.  This is
 *                    what src/r_shim.c binds.
 *   dsq_fit_*_dev  : every array pointer is a DEVICE pointer; work is enqueued on
 *                    `stream` (a hipStream_t passed as void*, NULL = default stream)
 *                    and the call returns without synchronising.  Used by the
 *                    Python host mirror and bench.py to keep Y / nf / weights / mu
 *                    resident in HBM across the four calls of one DESeq() fit.
 *
 * Matrix layouts (the `layout` field):
 *   DSQ_LAYOUT_R           n x m matrices are column-major as in R: (i,j) at i + n*j
 *   DSQ_LAYOUT_GENE_MAJOR  n x m matrices are row-major with leading dimension `ld`
 *                          (elements): (i,j) at i*ld + j.  This is the engine's
 *                          native layout (one wavefront per gene reads a coalesced
 *                          row); R-layout inputs are transposed on the device first.
 * n x p matrices (beta_mat, beta_var_mat) and n-vectors are ALWAYS in R layout
 * (column-major n x p).  x is m x p column-major, contrast/lambda are p-vectors.
 *
 * Semantics (argument meaning, iteration counters, break conditions, clamps, output
 * list members) follow the reference line by line; see DESIGN.md.  Inputs are
 * borrowed and never written.  No CPU fallback exists: without a usable gfx950
 * device every call fails with DSQ_ERR_DEVICE.
 *
 * Memory contract of the core _dev entries (dsq_fit_beta_dev, dsq_fit_disp_dev, dsq_fit_disp_grid_dev,
 * dsq_prefit_moments_dev, dsq_linear_mu_dev, dsq_nbinom_loglike_dev, dsq_intercept_fit_dev,
 * dsq_parametric_dispersion_fit_dev, dsq_cooks_distance_dev, dsq_replace_outliers_dev, dsq_weights_prep_dev, dsq_xim_dev,
 * the layout helpers, dsq_beta_prior_var_dev, dsq_deseq_dev): padding columns m .. ld-1 of gene-major inputs are not
 * read, of gene-major outputs not written.  Outputs and workspaces need not be initialised: every element the entry
 * defines is written before it is read, whatever the buffer held.  The two exceptions are flags the library ORs into,
 * which the caller zeroes first: *any_negative of dsq_weights_prep_dev and *bad of dsq_counts_f64_to_gene_major_i32.
 * Nothing outside the buffers handed over (at the sizes stated here) is written.  tests/test_gpu_entry_memory.py and tests/test_gpu_chain_memory.py hold the library
 * to this on poisoned memory.
 *
 * Stream-order contract of every _dev entry: all the work of a call -- kernels, memsets, copies, the uploads of its small
 * host tables (design cells, `replaceable`, a spline table, contrasts' cells) -- is ordered on `stream` behind whatever the
 * caller enqueued there before the call, and is complete, for the stream, in front of whatever the caller enqueues there
 * after it.  So device inputs may still be in the making on `stream` when the call is issued, and inputs, outputs and a
 * caller-provided workspace may be reused on `stream` the moment the call returns.  Where the library forks to a stream of
 * its own (the outlier refit of dsq_deseq_dev) the fork waits for `stream` and is joined back into it before the call's
 * last command.  Host arrays (tables, argument blocks) are read before the call returns and may be rewritten at once: a
 * table travels through pinned buffers of the (device, stream) context, never from the caller's or the library's pageable
 * memory at a later time.  The call does not wait for the device: it returns while `stream` is still busy.  The exceptions
 * state it at their entry: dsq_sf_iterate_dev, dsq_ash_dev and dsq_beta_prior_var_dev read results back (dsq_ash_dev: the
 * host decides every step of its iteration from a small record, so the call SYNCHRONISES `stream` (a few dozen times) and
 * the outputs are complete on return); the fit and aux entries that
 * take `y_type` (dsq_fit_beta_dev .. dsq_replace_outliers_dev):
 * given DSQ_Y_FLOAT64 counts they check the counts on the device and WAIT for `stream` once, at their end, to return
 * DSQ_ERR_VALUE (int32 counts: no wait); and a workspace slot of the context that has to GROW is reallocated behind a
 * device synchronisation (the first call of a shape on a stream, not the steady state).  Calls on different streams share
 * nothing that is in flight.  tests/test_gpu_stream_order.py holds the library to this on a stream that is kept busy,
 * with inputs that arrive late and buffers recycled early (tests/stream_hold.py); tests/test_stream_cases_cpu.py holds
 * that test's cases to the conditions under which it can fail.
 */
#ifndef DESEQ2_MI355X_H
#define DESEQ2_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSQ_VERSION 100

enum {
    DSQ_OK = 0,
    DSQ_ERR_ARG = 1,         /* bad size / NULL pointer / inconsistent arguments          */
    DSQ_ERR_UNSUPPORTED = 2, /* p or m outside the compiled kernel range                  */
    DSQ_ERR_DEVICE = 3,      /* no gfx950 device, HIP runtime error, kernel launch error  */
    DSQ_ERR_NOMEM = 4,       /* device or host allocation failed                          */
    DSQ_ERR_VALUE = 5,       /* non-integer / negative count in a REALSXP count matrix    */
    DSQ_ERR_FIT = 6          /* dsq_deseq: a condition the reference turns into an R error or a change of method
                                (all rows zero; no gene above 100 * minDisp; the parametric dispersion trend failed,
                                R/core.R:885-893) -- the caller falls back to the call-by-call routines          */
};

enum { DSQ_LAYOUT_R = 0, DSQ_LAYOUT_GENE_MAJOR = 1 };
enum { DSQ_Y_INT32 = 0, DSQ_Y_FLOAT64 = 1 }; /* R INTSXP or REALSXP count matrix */

#define DSQ_MAX_P 64 /* largest number of design columns served: 1..10 by register-resident kernels (one per
                       width), 11..64 by kernels over the design zero-padded to 16, 24, 32, 48 or 64 columns (the reference
                       itself has no limit, src/DESeq2.cpp:283-465).  49..64 columns: fitDisp / fitDispGrid take rows of
                       at most 1024 samples whose working set fits a CU's LDS (else DSQ_ERR_UNSUPPORTED) */

/* ---- fitBeta ------------------------------------------------------------------
 * reference: List fitBeta(ySEXP, xSEXP, nfSEXP, alpha_hatSEXP, contrastSEXP,
 *   beta_matSEXP, lambdaSEXP, weightsSEXP, useWeightsSEXP, tolSEXP, maxitSEXP,
 *   useQRSEXP, minmuSEXP)                                   src/DESeq2.cpp:283        */
typedef struct {
    int32_t n, m, p;
    int32_t layout;         /* DSQ_LAYOUT_* for y / nf / weights / hat_diagonals / mu      */
    int64_t ld;             /* leading dimension for DSQ_LAYOUT_GENE_MAJOR (>= m)          */
    const void *y;          /* n x m counts                                                */
    int32_t y_type;         /* DSQ_Y_INT32 or DSQ_Y_FLOAT64                                */
    const double *x;        /* m x p design, column-major                                  */
    const double *nf;       /* n x m normalization factors, or (nf_is_vector) m size factors */
    int32_t nf_is_vector;   /* extension: 1 = nf points at m size factors shared by all genes */
    const double *alpha_hat;/* n                                                           */
    const double *contrast; /* p                                                           */
    const double *beta_mat; /* n x p initial beta (natural-log scale), column-major        */
    const double *lambda;   /* p ridge values (natural-log scale)                          */
    const double *weights;  /* n x m observation weights; may be NULL when useWeights == 0 */
    int32_t useWeights;
    double tol;
    int32_t maxit;          /* 0 is valid: only the post-loop block runs (R/results.R:797) */
    int32_t useQR;
    double minmu;
    /* extension: design cells.  HOST array of m labels, samples with identical rows of x carrying the same label
     * (any numbering), ncell = number of labels; NULL / 0 = not known.  With at most 32 cells the cell-collapsed
     * kernel runs.  The host-pointer entry point derives the cells from x itself when this is NULL.  */
    const int32_t *cell_of;
    int32_t ncell;
} DsqFitBetaArgs;

typedef struct {
    /* members of the reference's return list (src/DESeq2.cpp:458-464); caller-allocated */
    double *beta_mat;       /* n x p column-major                                          */
    double *beta_var_mat;   /* n x p column-major                                          */
    double *iter;           /* n (double, as the reference's NumericVector)                */
    double *hat_diagonals;  /* n x m in `layout`; may be NULL to skip the 8*m bytes/gene   */
    double *contrast_num;   /* n                                                           */
    double *contrast_denom; /* n                                                           */
    double *deviance;       /* n                                                           */
    /* extension: fitted means, so R/fitNbinomGLMs.R:180 need not redo
     * nf * exp(x beta) on the host.  mu = max(nf*exp(x beta), mu_floor); NULL = skip.   */
    double *mu;             /* n x m in `layout`                                           */
    double mu_floor;        /* 0 = unclamped (fitNbinomGLMs.R:180); minmu = core.R:763     */
} DsqFitBetaOut;

int dsq_fit_beta(const DsqFitBetaArgs *args, const DsqFitBetaOut *out);
int dsq_fit_beta_dev(const DsqFitBetaArgs *args, const DsqFitBetaOut *out, void *stream);

/* ---- fitDisp ------------------------------------------------------------------
 * reference: List fitDisp(ySEXP, xSEXP, mu_hatSEXP, log_alphaSEXP,
 *   log_alpha_prior_meanSEXP, log_alpha_prior_sigmasqSEXP, min_log_alphaSEXP,
 *   kappa_0SEXP, tolSEXP, maxitSEXP, usePriorSEXP, weightsSEXP, useWeightsSEXP,
 *   weightThresholdSEXP, useCRSEXP)                         src/DESeq2.cpp:164        */
typedef struct {
    int32_t n, m, p;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *x;                    /* m x p column-major                              */
    const double *mu_hat;               /* n x m                                           */
    const double *log_alpha;            /* n initial values                                */
    const double *log_alpha_prior_mean; /* n                                               */
    double log_alpha_prior_sigmasq;
    double min_log_alpha;
    double kappa_0;
    double tol;
    int32_t maxit;
    int32_t usePrior;
    const double *weights;              /* n x m; may be NULL when useWeights == 0         */
    int32_t useWeights;
    double weightThreshold;
    int32_t useCR;
    const int32_t *cell_of;             /* extension: design cells, as in DsqFitBetaArgs (HOST, may be NULL)   */
    int32_t ncell;
} DsqFitDispArgs;

typedef struct {
    /* members of the reference's return list (src/DESeq2.cpp:268-276); each n long */
    double *log_alpha;
    int32_t *iter;
    int32_t *iter_accept;
    double *last_change;
    double *initial_lp;
    double *initial_dlp;
    double *last_lp;
    double *last_dlp;
    double *last_d2lp;   /* may be NULL (device entry point): the second-derivative launch is skipped */
} DsqFitDispOut;

int dsq_fit_disp(const DsqFitDispArgs *args, const DsqFitDispOut *out);
int dsq_fit_disp_dev(const DsqFitDispArgs *args, const DsqFitDispOut *out, void *stream);

/* ---- fitDispGrid --------------------------------------------------------------
 * reference: List fitDispGrid(ySEXP, xSEXP, mu_hatSEXP, disp_gridSEXP,
 *   log_alpha_prior_meanSEXP, log_alpha_prior_sigmasqSEXP, usePriorSEXP, weightsSEXP,
 *   useWeightsSEXP, weightThresholdSEXP, useCRSEXP)         src/DESeq2.cpp:469        */
typedef struct {
    int32_t n, m, p;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *x;
    const double *mu_hat;
    const double *disp_grid;            /* ngrid log-alpha values (R/wrappers.R:70-72)     */
    int32_t ngrid;
    const double *log_alpha_prior_mean; /* n                                               */
    double log_alpha_prior_sigmasq;
    int32_t usePrior;
    const double *weights;
    int32_t useWeights;
    double weightThreshold;
    int32_t useCR;
    const int32_t *cell_of;             /* extension: design cells (HOST, may be NULL)                         */
    int32_t ncell;
} DsqFitDispGridArgs;

typedef struct {
    double *log_alpha;                  /* n (src/DESeq2.cpp:512)                          */
} DsqFitDispGridOut;

int dsq_fit_disp_grid(const DsqFitDispGridArgs *args, const DsqFitDispGridOut *out);
int dsq_fit_disp_grid_dev(const DsqFitDispGridArgs *args, const DsqFitDispGridOut *out, void *stream);

/* The same three routines on the gene rows [row_lo, row_lo + row_cnt) of the SAME full n x . arrays (inputs read, outputs
 * written at those rows only).  Genes are independent (src/DESeq2.cpp:194,319,492), so a caller may walk a large
 * problem range by range -- the R shim does, polling R_CheckUserInterrupt() between ranges as the reference does every
 * 100 genes (:195,320,493).  dsq_fit_*(a, o) == dsq_fit_*_rows(a, o, 0, a->n).                                     */
int dsq_fit_beta_rows(const DsqFitBetaArgs *args, const DsqFitBetaOut *out, int64_t row_lo, int64_t row_cnt);
int dsq_fit_disp_rows(const DsqFitDispArgs *args, const DsqFitDispOut *out, int64_t row_lo, int64_t row_cnt);
int dsq_fit_disp_grid_rows(const DsqFitDispGridArgs *args, const DsqFitDispGridOut *out, int64_t row_lo, int64_t row_cnt);

/* ---- extensions beyond the three .Call routines ----------------------
 * dsq_prefit_moments: what estimateDispersionsGeneEst / fitNbinomGLMs compute in R before the
 * first native call -- baseMean, baseVar, allZero (R/core.R:2138-2146), roughDispEstimate
 * (R/core.R:2422-2437) and the QR least-squares start values (R/fitNbinomGLMs.R:139-145).
 * q (m x p), a = X R^-1 (m x p) and r (p x p) come from the thin QR of the model matrix
 * (stats::qr on the host, as in the reference), all column-major.                          */
typedef struct {
    int32_t n, m, p;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *nf;
    int32_t nf_is_vector;
    const double *weights;   /* only enter baseMean / baseVar; may be NULL */
    int32_t useWeights;
    const double *q, *a, *r;
} DsqPrefitArgs;

typedef struct {
    double *baseMean;    /* n */
    double *baseVar;     /* n */
    int32_t *allZero;    /* n */
    double *roughDisp;   /* n */
    double *beta_init;   /* n x p column-major (natural-log scale) */
} DsqPrefitOut;

int dsq_prefit_moments(const DsqPrefitArgs *args, const DsqPrefitOut *out);
int dsq_prefit_moments_dev(const DsqPrefitArgs *args, const DsqPrefitOut *out, void *stream);

/* dsq_linear_mu: linearModelMuNormalized (R/core.R:2454-2471), mu = nf * ((y/nf) Q)(X R^-1)', the closed-form
 * fitted means estimateDispersionsGeneEst uses when the design is a set of groups (R/core.R:735-760); floored at
 * mu_floor when > 0 (:763).  Takes the q / a fields of DsqPrefitArgs (r, weights unused).  mu: n x m.      */
int dsq_linear_mu(const DsqPrefitArgs *args, double mu_floor, double *mu);
int dsq_linear_mu_dev(const DsqPrefitArgs *args, double mu_floor, double *mu, void *stream);

/* dsq_nbinom_loglike: nbinomLogLike (R/core.R:2208-2217), rowSums([w *] dnbinom(y, mu, 1/disp, log)) */
typedef struct {
    int32_t n, m;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *mu;        /* n x m */
    const double *disp;      /* n */
    const double *weights;
    int32_t useWeights;
} DsqLogLikeArgs;

int dsq_nbinom_loglike(const DsqLogLikeArgs *args, double *loglike);
int dsq_nbinom_loglike_dev(const DsqLogLikeArgs *args, double *loglike, void *stream);

/* dsq_intercept_fit: the closed form fitNbinomGLMs takes for an intercept-only design with the wide prior
 * (R/fitNbinomGLMs.R:99-137; nbinomLRT's reduced = ~1 reaches it for every gene): betaMatrix = log2 of the
 * [weighted] mean normalized count, mu = nf 2^beta, betaSE and hat from w = [weights] / (1/mu + alpha).
 * Outputs: beta_log2, betaSE (n); mu, hat (n x m, either may be NULL).  mu is floored at mu_floor when > 0.   */
typedef struct {
    int32_t n, m;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *nf;
    int32_t nf_is_vector;
    const double *weights;
    int32_t useWeights;
    const double *alpha;     /* n */
    double mu_floor;
} DsqInterceptArgs;

typedef struct {
    double *beta_log2, *betaSE;   /* n */
    double *mu, *hat;             /* n x m or NULL */
} DsqInterceptOut;

int dsq_intercept_fit(const DsqInterceptArgs *args, const DsqInterceptOut *out);
int dsq_intercept_fit_dev(const DsqInterceptArgs *args, const DsqInterceptOut *out, void *stream);

/* dsq_optim_rows: fitNbinomGLMsOptim (R/fitNbinomGLMs.R:340-407) -- the rows fitBeta left unconverged (or with NA /
 * non-positive variance) re-fitted by maximising the penalised NB log posterior over beta in [-30, 30]^p.  The
 * reference runs stats::optim(method = "L-BFGS-B") per row in R; here one wavefront per row runs a damped
 * Fisher-scoring iteration on the same objective over the same box.  The caller passes ONLY those rows
 * (n of them).  lambda: prior precisions on the log2 scale (R's `lambda`); beta_start / beta / betaSE on the log2
 * scale; conv = optim's convergence == 0; mu = nf 2^(x beta) unclamped (:386); logLike at mu clamped to minmu (:398). */
typedef struct {
    int32_t n, m, p;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *x;
    const double *nf;
    int32_t nf_is_vector;
    const double *alpha_hat;   /* n */
    const double *lambda;      /* p */
    const double *weights;
    int32_t useWeights;
    const double *beta_start;  /* n x p column-major */
    double minmu;
} DsqOptimArgs;

typedef struct {
    double *beta, *betaSE;     /* n x p column-major */
    int32_t *conv;             /* n */
    double *mu;                /* n x m */
    double *logLike;           /* n */
} DsqOptimOut;

int dsq_optim_rows(const DsqOptimArgs *args, const DsqOptimOut *out);

/* dsq_parametric_dispersion_fit: parametricDispersionFit (R/core.R:2166-2190), the all-gene Gamma-GLM
 * trend disp ~ asymptDisp + extraPois/mean between the two dispersion passes.  means / disps: n values
 * (the genes with dispGeneEst > 100*minDisp, R/core.R:870).  coefs: 2 doubles.  *status: 0 ok,
 * 1 = "parametric dispersion fit failed", 2 = "dispersion fit did not converge" (the caller then falls
 * back as R/core.R:885-893 does).  _dev: device pointers (coefs, status on the device too).        */
int dsq_parametric_dispersion_fit(const double *means, const double *disps, int64_t n, double *coefs, int32_t *status);
int dsq_parametric_dispersion_fit_dev(const double *means, const double *disps, int64_t n, double *coefs,
                                      int32_t *status, void *stream);

/* dsq_cooks_distance: calculateCooksDistance (R/core.R:2333-2340) with its robust method-of-moments
 * dispersion (robustMethodOfMomentsDisp :2277-2299, trimmedCellVariance :2301-2324, trimmedVariance
 * :2326-2331) and recordMaxCooks (:2349-2359), called from nbinomWaldTest (:1457-1460) and nbinomLRT
 * (:1888-1891).  `cell_of` is ALWAYS a host pointer (m design-cell ids 0..ncell-1: samples with identical
 * rows of the dispersion model matrix share a cell, nOrMoreInCell :2366-2371); p = ncol of that matrix.
 * maxCooks is NaN (R: NA) when m <= p or no cell has 3 members.                                      */
typedef struct {
    int32_t n, m, p;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *nf;
    int32_t nf_is_vector;
    const double *mu;        /* n x m fitted means (assays "mu") */
    const double *H;         /* n x m hat diagonals (fitBeta's hat_diagonals) */
    const int32_t *cell_of;  /* m, HOST */
    int32_t ncell;
} DsqCooksArgs;
typedef struct {
    double *cooks;       /* n x m, layout of the inputs */
    double *maxCooks;    /* n */
    double *robustDisp;  /* n (may be NULL) */
} DsqCooksOut;
int dsq_cooks_distance(const DsqCooksArgs *args, const DsqCooksOut *out);
int dsq_cooks_distance_dev(const DsqCooksArgs *args, const DsqCooksOut *out, void *stream);

/* dsq_replace_outliers: replaceOutliers (R/core.R:2069-2115).  newCounts = counts, except where
 * cooks > cooksCutoff in a `replaceable` sample: there as.integer(trimmed mean (trim) of the normalized
 * counts * nf).  replace[i] = any(cooks[i,] > cooksCutoff) (:2086).  `replaceable` is a host pointer
 * (m flags, nOrMoreInCell(modelMatrix, minReplicates)).                                              */
typedef struct {
    int32_t n, m;
    int32_t layout;
    int64_t ld;
    const void *y;
    int32_t y_type;
    const double *nf;
    int32_t nf_is_vector;
    const double *cooks;        /* n x m */
    double cooksCutoff;         /* qf(.99, p, m - p) by default (:2081) */
    double trim;                /* .2 */
    const int32_t *replaceable; /* m, HOST */
} DsqReplaceArgs;
typedef struct {
    int32_t *newCounts;  /* n x m int32, layout of the inputs */
    int32_t *replace;    /* n */
} DsqReplaceOut;
int dsq_replace_outliers(const DsqReplaceArgs *args, const DsqReplaceOut *out);
int dsq_replace_outliers_dev(const DsqReplaceArgs *args, const DsqReplaceOut *out, void *stream);

/* getAndCheckWeights (R/core.R:2697-2751) on resident gene-major weights: w_norm = w / rowmax (:2702), w_floor =
 * pmax(w_norm, 1e-6) (:702), weightsFail[i] = 1 when the weights of gene i leave a degenerate design (the two per-gene
 * qr() rank tests of :2711-2722, full-rank model matrices, p <= DSQ_MAX_P), *any_negative |= 1 when a weight is negative
 * (the caller zeroes it first).  All device pointers; x: m x p column-major.                                      */
int dsq_weights_prep_dev(const double *weights_raw, const double *x, int32_t n, int32_t m, int32_t p, int64_t ld,
                         double weightThreshold, double *w_norm, double *w_floor, int32_t *weightsFail,
                         int32_t *any_negative, void *stream);
/* momentsDispEstimate's xim for a resident normalization-factor matrix (R/core.R:2440-2444): mean over the samples of
 * 1 / colMeans(nf), every column summed down the genes in gene order.  scratch_m: m doubles; *out on the device.  */
int dsq_xim_dev(const double *nf, int32_t n, int32_t m, int64_t ld, double *scratch_m, double *out, void *stream);

/* ---- layout helpers (device pointers, async on stream) --------------------------
 * R layout (column-major n x m) <-> gene-major (row-major, leading dimension ld).   */
int dsq_to_gene_major_f64(const double *src_r, double *dst_gm, int32_t n, int32_t m, int64_t ld, void *stream);
int dsq_to_gene_major_i32(const int32_t *src_r, int32_t *dst_gm, int32_t n, int32_t m, int64_t ld, void *stream);
/* REALSXP counts -> int32 gene-major; *bad (device int32) is set non-zero if any value
 * is negative, non-finite or non-integer                                             */
int dsq_counts_f64_to_gene_major_i32(const double *src_r, int32_t *dst_gm, int32_t n, int32_t m,
                                     int64_t ld, int32_t *bad, void *stream);
int dsq_from_gene_major_f64(const double *src_gm, double *dst_r, int32_t n, int32_t m, int64_t ld, void *stream);

/* ---- misc ---------------------------------------------------------------------- */
int dsq_version(void);
const char *dsq_last_error(void);        /* thread-local message of the last failing call  */
int dsq_device_count(void);              /* number of visible HIP devices (0 if none)      */
int dsq_set_device(int device);          /* device used by subsequent calls on this thread */
int dsq_release_workspace(void);         /* free the cached device workspaces              */

/* Kernel timing for bench.py's roofline: when enabled, every dsq_fit_*_dev call brackets its
 * fit kernel launch with HIP events on the launch stream; dsq_profile_last_ms() waits for the
 * most recent one and returns its duration in milliseconds (negative if none was recorded).  */
int dsq_profile_enable(int on);
double dsq_profile_last_ms(void);

/* Parity hook for tests: evaluate one scalar primitive of the device math library on
 * the GPU (op: 0 exp, 1 log, 2 log1p, 3 lgamma, 4 digamma, 5 trigamma, 6 stirlerr,
 * 7 bd0(a,b), 8 dnbinom_mu_log(a=x, b=size, c=mu), 9 2 pnorm(-|a|), 10 pt(a, df = b, lower.tail = FALSE), 11 pt(a, df = b);
 * the variants the kernels call: 12 log_full, 13 log_pn (positive normal a), 14 rcp_n, 15 div_n(a, b) = a / b, 16 stirlerr_n
 * (0 < a < 1e100), 17 bd0_fast(a, b), 18 / 19 the lgamma / digamma output of the paired routine, 20 pnorm(a), 21 pnorm(a,
 * lower.tail = FALSE), 22 nb_split(a = y, b = alpha, c = mu): one sample of nbinomLogLike on the closed split, 23 sf_log,
 * 24 sf_exp, 25 order_key (the key's 64 bits in the double), 26 order_unkey(order_key(a))).  Ops 7, 8, 10, 11, 15, 17, 22
 * need b; 8 and 22 need c.  Element i is evaluated by thread i: wave w of the launch holds elements [64 w, 64 w + 64).
 * HOST pointers, n elements.                                                              */
int dsq_test_math(int op, const double *a, const double *b, const double *c, double *out, int64_t n);

/* ---- dsq_deseq_dev: the whole DESeq() chain, device-driven ---------------------------
 * estimateDispersionsGeneEst (R/core.R:657-860) -> estimateDispersionsFit (:864-939, parametric) +
 * estimateDispersionsPriorVar (:1135-1208) -> estimateDispersionsMAP (:943-1131) -> nbinomWaldTest (:1332-1565)
 * or nbinomLRT against ~1 (:1787-2012) -> replaceOutliers / refitWithoutOutliers (:2069-2115, :2484-2563) on
 * matrices resident in HBM in the gene-major layout.  The per-gene decision rules R applies between the native
 * calls (clamps, accept / convergence / refit rules, dispOutlier, betaConv ...) run as small kernels, the rows a
 * rule sends to fitDispGrid or to the outlier refit are compacted on the device and fitted by row-listed launches
 * of the same kernels, so a phase needs no host round trip.  Rows that need R's host-side fallback (the
 * L-BFGS-B rows of fitNbinomGLMsOptim) are only FLAGGED (optim_* outputs): the caller re-does them through the
 * per-call entry points.  Phases (bit mask), each asynchronous on `stream`:
 *   DSQ_PH_GENE_EST   counts -> baseMean .. dispGeneEst, mu-hat
 *   DSQ_PH_TREND      dispersion trend (fitType: parametric / mean) + prior variance over (trend_mean, trend_disp) [n_trend on the device] or,
 *                     when those are NULL, over this call's own genes (multi-GPU: the gathered vectors)
 *   DSQ_PH_MAP_TEST   dispFit, MAP dispersions, final GLM fit [+ the reduced-model fit], Wald statistics / logLik pair
 *   DSQ_PH_OUTLIERS   Cook's distances, replaceOutliers, refit of the replaced rows, maxCooks
 *   DSQ_PH_FINISH     (gene-sharding callers only, see below)
 * status[] (int32, device): see DSQ_ST_*; scalars[] (double, device): see DSQ_SC_*.                            */
#define DSQ_PH_GENE_EST 1
#define DSQ_PH_TREND    2
#define DSQ_PH_MAP_TEST 4
#define DSQ_PH_OUTLIERS 8
/* DSQ_PH_OUTLIERS in two calls, for a caller that brings its own dispersion trend (dispFit_in) AND wants the replaced rows
 * refitted on the chain (refitWithoutOutliers evaluates dispersionFunction(object) at the NEW means, R/core.R:2512):
 *   DSQ_PH_OUTLIERS_DETECT  Cook's distances, replaceOutliers, baseMean / baseVar / allZero of the replaced rows (:2488-2491)
 *   -- the caller reads `replace`, `allZero`, `baseMean`, writes its trend at the rows with replace = 1, allZero = 0 into dispFit_in --
 *   DSQ_PH_OUTLIERS_REFIT   the refit of those rows and the closing steps (:2496-2546)                                   */
#define DSQ_PH_OUTLIERS_DETECT 64
#define DSQ_PH_OUTLIERS_REFIT 128
#define DSQ_PH_PRIOR    32   /* betaPrior = TRUE: the second pass of fitGLMsWithPrior (R/fitNbinomGLMs.R:311-325) with
                                lambda_prior = 1 / betaPriorVar; DSQ_PH_MAP_TEST has run the MLE pass (:256-260) and the
                                caller has turned mle_beta into the prior variance (estimateBetaPriorVar, R/core.R:1601-1689:
                                an all-gene weighted quantile, host code).  Runs before DSQ_PH_OUTLIERS.                */
#define DSQ_PH_FINISH   16   /* the two closing steps of refitWithoutOutliers that depend on whether ANY row of the whole
                                analysis was refitted (R/core.R:2496, 2535-2546: NA results on rows that became all zero,
                                maxCooks): part of DSQ_PH_OUTLIERS unless defer_finish is set -- a caller that shards the
                                genes sets it, adds up N_REFIT over its shards and runs this phase with the total       */

enum { DSQ_ST_N_NONZERO = 0, DSQ_ST_N_GRID_GENEEST, DSQ_ST_N_TREND, DSQ_ST_TREND_STATUS, DSQ_ST_N_ABOVE_MIN,
       DSQ_ST_N_GRID_MAP, DSQ_ST_N_OPTIM_GENEEST, DSQ_ST_N_OPTIM_TEST, DSQ_ST_N_REPLACE, DSQ_ST_N_REFIT,
       DSQ_ST_N_GRID_GENEEST_REFIT, DSQ_ST_N_GRID_MAP_REFIT, DSQ_ST_N_OPTIM_GENEEST_REFIT, DSQ_ST_N_OPTIM_TEST_REFIT,
       DSQ_ST_COUNT = 16 };        /* (14, 15: counters of the chain's own) */
/* estimateDispersionsFit's fitType (R/core.R:864-939).  "local" is no DSQ_FIT_* value: the chain sees it as a given trend
 * (dispFit_in), which dsq_local_fit_dev below computes on the device from the gene-estimate phase's baseMean / dispGeneEst.
 * A caller that wants the reference's automatic substitution asks for DSQ_FIT_PARAMETRIC, gets DSQ_ERR_FIT when the trend
 * does not fit and takes that route (or its own); DSQ_FIT_PARAMETRIC_OR_MEAN substitutes the mean on the device.   */
#define DSQ_FIT_PARAMETRIC          0
#define DSQ_FIT_MEAN                1    /* mean(dispGeneEst[dispGeneEst > 10 minDisp], trim = 0.001), R/core.R:894-899 */
#define DSQ_FIT_PARAMETRIC_OR_MEAN  2
#define DSQ_FIT_GIVEN               3    /* (reported in DSQ_SC_FIT_USED only) the caller's trend values: dispFit_in        */
enum { DSQ_SC_COEF0 = 0, DSQ_SC_COEF1, DSQ_SC_VAR_LOG_DISP, DSQ_SC_DISP_PRIOR_VAR,
       DSQ_SC_FIT_USED,            /* the trend the analysis ended up with: DSQ_FIT_PARAMETRIC (0.0) or DSQ_FIT_MEAN (1.0:
                                      COEF0 is the mean, COEF1 zero)                                               */
       DSQ_SC_COUNT = 8 };

typedef struct {
    int32_t n, m, p;
    int64_t ld;
    int32_t phases;
    const int32_t *y;              /* n x ld gene-major counts                                                  */
    const double *nf;              /* n x ld normalization factors, or m size factors (nf_is_vector)            */
    int32_t nf_is_vector;
    int32_t useWeights;
    const double *weights_raw;     /* assays[["weights"]] as given: enters baseMean / baseVar (R/core.R:2140)   */
    const double *weights_norm;    /* / row max (R/core.R:2702): GLM fits, MAP, logLik                           */
    const double *weights_floor;   /* pmax(weights_norm, 1e-6) (R/core.R:702): gene-wise dispersion search       */
    const int32_t *force_zero;     /* n flags or NULL: rows treated as all-zero (weightsFail, R/core.R:2737)     */
    const double *x;               /* m x p design, column-major                                                 */
    const double *q, *a, *r;       /* thin QR of the design: Q, X R^-1 (m x p), R (p x p), column-major          */
    double xim;                    /* momentsDispEstimate's mean(1 / sizeFactors) (R/core.R:2440-2444); with a
                                      normalization-factor MATRIX (nf_is_vector = 0) it is not read: the chain takes
                                      mean(1 / colMeans(nf)) over the rows that are not all zero itself              */
    int32_t linearMu;              /* R/core.R:735-742                                                           */
    double minDisp, kappa_0, dispTol, weightThreshold, outlierSD, betaTol, minmu;
    int32_t maxit, useCR, useQR, betaMaxit;
    const double *disp_grid;       /* ngrid log-alpha grid points of fitDispGridWrapper (R/wrappers.R:70-72)     */
    int32_t ngrid;
    double expVarLogDisp;          /* trigamma((m - p) / 2) (R/core.R:1196); ignored when m <= p                  */
    const double *trend_mean, *trend_disp;   /* device vectors of n_trend values, or NULL                        */
    int32_t n_trend;
    const double *lambda;          /* HOST: p ridge values on the natural-log scale (R/fitNbinomGLMs.R:162)      */
    double min_log_alpha;          /* log(minDisp / 10) (R/core.R:775)                                           */
    void *workspace;               /* device, dsq_deseq_workspace_bytes(...): holds the row lists and counters of
                                      the analysis between phases -- the same buffer for all its phases.  It need
                                      not be initialised: the first phase of an analysis (DSQ_PH_GENE_EST) reads
                                      nothing of it that it has not written, so between two analyses it may hold
                                      anything -- another analysis' vectors included                              */
    int64_t workspace_bytes;
    int32_t test;                  /* 0 Wald, 1 LRT (reduced = ~1 unless x_red is given)                         */
    /* outlier phase (all host arrays; R/core.R:2081,2101,2366-2371) */
    const int32_t *cell_of;        /* HOST: design cell of each sample                                           */
    int32_t ncell;
    const int32_t *replaceable;    /* HOST: m flags nOrMoreInCell(x, minReplicatesForReplace)                    */
    double cooksCutoff, trim;
    int32_t do_replace;            /* 0: Cook's distances only                                                   */
    /* nbinomLRT against a reduced model that is not ~1 (R/core.R:1856-1868): its m x p_red model matrix, the thin QR
     * of it (start values, R/fitNbinomGLMs.R:139-145) and its design cells; all NULL / 0 = the intercept-only closed form */
    const double *x_red, *q_red, *a_red, *r_red;   /* device, column-major                                      */
    int32_t p_red;
    const int32_t *cell_of_red;    /* HOST                                                                       */
    int32_t ncell_red;
    int32_t defer_finish;          /* see DSQ_PH_FINISH                                                          */
    const int32_t *n_refit_global; /* device int32 for DSQ_PH_FINISH: refitted rows over ALL shards (NULL: this call's) */
    /* nbinomWaldTest(betaPrior = TRUE) (R/core.R:1416-1432, R/fitNbinomGLMs.R:242-337), Wald only: the model matrix of
     * the prior pass -- the design itself (modelMatrixType "standard") or the expanded one (R/expanded.R:1-18, rank
     * deficient: start values of :146-155) -- with the same design cells as x; p, p_prior <= 10; the workspace is asked
     * for with max(p, p_prior) columns.  beta / betaSE / stat / pvalue are then n x p_prior.                            */
    int32_t betaPrior;
    const double *x_prior;         /* device, m x p_prior column-major                                           */
    int32_t p_prior, prior_expanded, prior_intercept;   /* expanded: rank-deficient start values; first column all ones */
    const double *lambda_prior;    /* HOST, p_prior: 1 / betaPriorVar / log(2)^2; read by DSQ_PH_PRIOR / _OUTLIERS */
    int32_t fitType;               /* DSQ_FIT_*: read by DSQ_PH_TREND                                             */
    /* the caller's dispersion trend -- fitType = "local" (R/core.R:889-893: dsq_local_fit_dev evaluates it on the device) or
     * `dispersionFunction(dds) <- f` (R/methods.R:142-190) --, evaluated by the caller at the baseMean of every gene (the
     * DSQ_PH_GENE_EST phase gives baseMean and dispGeneEst): device, n values.  DSQ_PH_TREND then fits nothing and takes
     * varLogDispEsts / the prior variance from the residuals against it (against trend_fit_in, n_trend values aligned with
     * trend_mean / trend_disp, when those are given); DSQ_PH_MAP_TEST takes dispFit from it.  The refit of replaced rows
     * needs the trend at means the caller has not seen: either do_replace = 0 (the caller refits, R/core.R:2484-2563) or the
     * outlier phase in its two halves, DSQ_PH_OUTLIERS_DETECT / _REFIT above.                                          */
    const double *dispFit_in, *trend_fit_in;
    /* estimateDispersionsMAP(dispPriorVar = x) (R/core.R:970,989-994): > 0 = the caller's prior variance, taken instead of
     * the estimate (varLogDispEsts is still computed: the dispOutlier rule reads it).  The way residual df <= 3 runs on the
     * chain: R's estimate there is a seeded Monte-Carlo match (R/core.R:1155-1190, R's RNG + loess), the caller's job.   */
    double dispPriorVar_in;
} DsqDeseqArgs;

typedef struct {
    /* per-gene results, device, caller-allocated; rows that are all-zero come back NaN / -1.  None of the outputs need
     * be initialised.  Written whole: every per-gene column (logLikeReduced under the Wald test too: NA), status,
     * mle_beta, and the rows of mu, H and cooks over the columns 0 .. m-1 (NA in the all-zero rows).  Left as it was:
     *   scalars        DSQ_SC_COEF0 .. DSQ_SC_FIT_USED are written, the spare entries behind them are not;
     *   mu_hat         rows of all-zero genes (allZero = 1 after DSQ_PH_GENE_EST, weightsFail rows included) are left as
     *                  they were;
     *   replaceCounts  only the rows with replace != 0 are written;
     *   all five n x ld matrices: the padding columns m .. ld-1 are not written.                                       */
    double *baseMean, *baseVar;
    int32_t *allZero;
    double *dispGeneEst;
    int32_t *dispGeneIter;
    double *dispFit, *dispMAP, *dispersion;
    int32_t *dispIter, *dispOutlier;
    double *beta, *betaSE, *stat, *pvalue;      /* n x p column-major, log2 scale; stat / pvalue Wald only        */
    int32_t *betaConv;
    double *betaIter, *logLike, *logLikeReduced, *maxCooks;
    int32_t *replace;
    int32_t *optim_geneest, *optim_test;        /* n flags: rows R hands to the L-BFGS-B fallback                 */
    /* n x ld gene-major */
    double *mu_hat;                             /* clamped fitted means of the gene-wise fit (assays mu of GeneEst) */
    double *mu, *H, *cooks;
    int32_t *replaceCounts;
    int32_t *status;                            /* DSQ_ST_COUNT */
    double *scalars;                            /* DSQ_SC_COUNT */
    double *mle_beta;                           /* betaPrior: n x p, the MLE coefficients (mcols MLE_*), log2 scale */
} DsqDeseqOut;

int dsq_deseq_dev(const DsqDeseqArgs *args, const DsqDeseqOut *out, void *stream);
int64_t dsq_deseq_workspace_bytes(int32_t n, int32_t m, int32_t p, int32_t n_trend);

/* ---- dsq_size_factors: estimateSizeFactors on the device --------------------------------------
 * estimateSizeFactorsForMatrix (R/core.R:535-578), estimateNormFactors (R/core.R:2159-2163) and the dispatch of
 * estimateSizeFactors.DESeqDataSet (R/methods.R:363-406): sf_j = exp(median over {i : loggeomeans_i finite, k_ij > 0
 * [, control_i]} of (log k_ij - loggeomeans_i)), the median an EXACT order statistic found by radix selection over
 * order-preserving 64-bit keys (no sort).
 *   DSQ_SF_RATIO      loggeomeans_i = mean_j log k_ij (-Inf when the gene has a zero)
 *   DSQ_SF_POSCOUNTS  geoMeans_i = exp(sum of log over the positive counts / m), 0 for an all-zero row (R/methods.R:377-382),
 *                     then as a caller's geoMeans
 *   geoMeans given    loggeomeans = log(geoMeans); the result is divided by exp(mean(log sf)) (R/core.R:573-576)
 * normMatrix: the size factors of counts / normMatrix, then normalizationFactors = normMatrix * sf per column, each row
 * divided by its geometric mean.  A sample with an empty selection gets NaN (R: NA).
 * _dev: device pointers, asynchronous on `stream`, no host synchronisation and no allocation: the workspace
 * (dsq_size_factors_workspace_bytes) is the caller's.  Counts may be int32 or float64 in either layout (gene-major is
 * the fast one: a wavefront reads 64 consecutive samples of a gene).                                                  */
enum { DSQ_SF_RATIO = 0, DSQ_SF_POSCOUNTS = 1 };
typedef struct {
    int32_t n, m;
    int32_t layout;            /* DSQ_LAYOUT_* of y / normMatrix / normalizationFactors                             */
    int64_t ld;                /* leading dimension for DSQ_LAYOUT_GENE_MAJOR (>= m)                                */
    const void *y;             /* n x m counts                                                                      */
    int32_t y_type;            /* DSQ_Y_INT32 or DSQ_Y_FLOAT64                                                      */
    int32_t type;              /* DSQ_SF_RATIO or DSQ_SF_POSCOUNTS                                                  */
    const double *geoMeans;    /* n, or NULL (ignored by DSQ_SF_POSCOUNTS, which computes its own, R/methods.R:381) */
    const int32_t *control;    /* n flags (controlGenes as a logical vector), or NULL = every gene                  */
    const double *normMatrix;  /* n x m in `layout`, or NULL                                                        */
    void *workspace;           /* device; dsq_size_factors: ignored                                                 */
    int64_t workspace_bytes;
} DsqSizeFactorArgs;

typedef struct {
    double *sizeFactors;           /* m                                                                             */
    double *loggeomeans;           /* n, or NULL                                                                    */
    double *normalizationFactors;  /* n x m in `layout`: required if and only if normMatrix is given                */
    int32_t *status;               /* 1 value: 0 ok, 1 = every gene contains at least one zero (R/core.R:557-559)   */
} DsqSizeFactorOut;

int dsq_size_factors_dev(const DsqSizeFactorArgs *args, const DsqSizeFactorOut *out, void *stream);
/* host pointers in R layout, one device, synchronous; DSQ_ERR_FIT when *status comes back 1 */
int dsq_size_factors(const DsqSizeFactorArgs *args, const DsqSizeFactorOut *out);
int64_t dsq_size_factors_workspace_bytes(int32_t n, int32_t m);

/* ---- dsq_vst: the variance stabilizing transformation and its relatives ------------------------
 * getVarianceStabilizedData (R/vst.R:146-193), normTransform (R/helper.R:421-436) and counts(normalized = TRUE): ONE pass
 * over the counts, q_ij = k_ij / nf_ij (one IEEE division; nf = the m size factors or an n x m matrix), then by `kind`
 *   DSQ_VST_PARAMETRIC  log((1 + e + 2 a q + 2 sqrt(a q (1 + e + a q))) / (4 a)) / log(2)     a = asymptDisp, e = extraPois
 *                       (R/vst.R:151-156)
 *   DSQ_VST_MEAN        (2 asinh(sqrt(alpha q)) - log(alpha) - log(4)) / log(2)                 (R/vst.R:184-189)
 *   DSQ_VST_SPLINE      eta * S(asinh(q)) + xi, S the piecewise cubic of the caller's table: what splinefun() returned
 *                       for the numerically integrated trend of fitType "local" (R/vst.R:157-183)
 *   DSQ_VST_LOG2        log2(q + pc)                                                            (R/helper.R:421-436)
 *   DSQ_VST_NORMALIZED  q                                                                       (counts(normalized = TRUE))
 * every operation rounded once in the order the R expression evaluates it; log / log1p are the library's (dsq_math.hpp),
 * asinh is built from them.  The spline table is a HOST array of 5 * nknots doubles, x | y | b | c | d
 * (knots ascending, value and the three polynomial coefficients of each knot): S(u) = y + dx (b + dx (c + dx d)) with
 * dx = u - x_i, i the largest index with x_i <= u, the first knot left of all of them (cubic extrapolation on both sides).
 * dsq_vst_rowstats_dev (host pointers: dsq_vst with rowMean / rowMax given, out NULL or not): rowMeans and row maxima of q (vst()'s gene subset, R/vst.R:239, and max / quantiles of the spline
 * path, :166,175-176): the mean is the wave-order sum over the samples divided by m, the maximum is exact (NaN if the row
 * holds one).
 * _dev: device pointers (the table excepted), asynchronous on `stream`, no host synchronisation; a float64 count that is
 * negative, non-finite or non-integer sets *bad (when given) to 1 and is transformed as it stands.  The host entry
 * returns DSQ_ERR_VALUE for such a matrix.  Padding columns m .. ld-1 of a gene-major output are not written.          */
enum { DSQ_VST_PARAMETRIC = 0, DSQ_VST_MEAN = 1, DSQ_VST_SPLINE = 2, DSQ_VST_LOG2 = 3, DSQ_VST_NORMALIZED = 4 };
#define DSQ_VST_MAX_KNOTS 1600 /* the table lives in LDS: 40 bytes per knot, 64 000 bytes (62.5 KiB) per workgroup at most */
typedef struct {
    int32_t n, m;
    int32_t layout;            /* DSQ_LAYOUT_* of y / nf (matrix) / out                                             */
    int64_t ld;                /* leading dimension for DSQ_LAYOUT_GENE_MAJOR (>= m)                                */
    const void *y;             /* n x m counts                                                                      */
    int32_t y_type;            /* DSQ_Y_INT32 or DSQ_Y_FLOAT64                                                      */
    const double *nf;          /* m size factors (nf_is_vector) or n x m normalization factors in `layout`          */
    int32_t nf_is_vector;
    int32_t kind;              /* DSQ_VST_*                                                                         */
    double asymptDisp, extraPois;  /* DSQ_VST_PARAMETRIC: both finite, asymptDisp > 0                               */
    double alpha;              /* DSQ_VST_MEAN: finite, > 0                                                         */
    double pc;                 /* DSQ_VST_LOG2: the pseudocount                                                     */
    const double *spline;      /* DSQ_VST_SPLINE: HOST pointer, 5 * nknots doubles x | y | b | c | d                */
    int32_t nknots;            /* 2 .. DSQ_VST_MAX_KNOTS                                                            */
    double eta, xi;            /* DSQ_VST_SPLINE: the affine rescaling (R/vst.R:177-178)                            */
} DsqVstArgs;

typedef struct {
    double *out;               /* n x m in `layout` (dsq_vst[_dev]); dsq_vst: may be NULL when only the row statistics are wanted */
    double *rowMean;           /* n (dsq_vst_rowstats_dev; dsq_vst: optional, both or neither)                      */
    double *rowMax;            /* n (dsq_vst_rowstats_dev; dsq_vst: optional, both or neither)                      */
    int32_t *bad;              /* _dev: one device int32 the CALLER has zeroed, or NULL; host entries: ignored      */
} DsqVstOut;

int dsq_vst_dev(const DsqVstArgs *args, const DsqVstOut *out, void *stream);
int dsq_vst_rowstats_dev(const DsqVstArgs *args, const DsqVstOut *out, void *stream);   /* kind and its scalars are ignored */
/* host pointers in R layout, one device, synchronous: the transform into out (if non-NULL) and the row statistics (if non-NULL) */
int dsq_vst(const DsqVstArgs *args, const DsqVstOut *out);

/* ---- dsq_rlog: the regularized-logarithm fit of rlogData (R/rlog.R:172-272) ----------------------
 * One ridge-penalised coefficient per sample, for ANY number of samples: the design is [1 | I_m] (form A, intercept
 * NULL) or I_m with the caller's per-gene intercept folded into the factors, nf_ij 2^intercept_i (form B, the rlog of
 * new samples on a frozen intercept), so an IRLS step of src/DESeq2.cpp:334-383 is two wave-order sums over the
 * samples plus elementwise work.  lambda = 1 / betaPriorVar / log(2)^2 on every sample, 1e-6 / log(2)^2 on the
 * intercept; start values as R/fitNbinomGLMs.R:144-151; |beta| > 30 or a NaN convergence measure end the loop with
 * iter = maxit; maxit = 0 returns the start values.  Output rlog_ij = beta0 log2(e) + beta_j log2(e) (form A),
 * beta_j log2(e) + intercept_i (form B).  Rows that are not fitted -- all counts zero (A), a non-finite intercept (B) --
 * get 0, intercept -Inf, iter 0, flag 1; a finite intercept with all-zero counts IS fitted.  A row that ends with a
 * non-finite coefficient (the rows R/fitNbinomGLMs.R:203-207 hands to optim) comes back NaN with flag 2: the optim
 * refit is not served.  Observation weights are not served.
 * _dev: device pointers, asynchronous on `stream`, no allocation, no host synchronisation, no workspace (rows beyond
 * what registers and LDS hold use their own output row as scratch); padding columns m .. ld-1 of a gene-major output are
 * not written; a negative, non-finite or non-integer float64 count sets *bad.
 * dsq_rlog: host pointers in R layout, ONE device, synchronous; DSQ_ERR_VALUE for such a count matrix, DSQ_ERR_ARG for
 * a NaN or non-positive dispFit on a row that is fitted (R/rlog.R:228).                                                */
typedef struct {
    int32_t n, m;
    int32_t layout;            /* DSQ_LAYOUT_* of y / nf (matrix) / rlog                                            */
    int64_t ld;                /* leading dimension for DSQ_LAYOUT_GENE_MAJOR (>= m)                                */
    const void *y;             /* n x m counts                                                                      */
    int32_t y_type;            /* DSQ_Y_INT32 or DSQ_Y_FLOAT64                                                      */
    const double *nf;          /* m size factors (nf_is_vector) or n x m normalization factors in `layout`          */
    int32_t nf_is_vector;
    const double *dispFit;     /* n: the dispersion trend at the row's mean                                         */
    double betaPriorVar;       /* log2 scale, finite, > 0                                                           */
    const double *intercept;   /* n (log2 scale; non-finite = row not fitted), or NULL for form A                   */
    double tol, minmu;         /* rlogData: 1e-4, 0.5                                                               */
    int32_t maxit;             /* 100                                                                               */
} DsqRlogArgs;

typedef struct {
    double *rlog;              /* n x m in `layout`                                                                 */
    double *intercept;         /* n, form A only (log2 scale; -Inf on an all-zero row); may be NULL                 */
    double *iter;              /* n; betaConv = iter < maxit                                                        */
    int32_t *flag;             /* n: 0 fitted, 1 row not fitted, 2 a non-finite coefficient (row is NaN)            */
    int32_t *bad;              /* _dev: one device int32 the CALLER has zeroed, or NULL; dsq_rlog: ignored          */
} DsqRlogOut;

int dsq_rlog_dev(const DsqRlogArgs *args, const DsqRlogOut *out, void *stream);
int dsq_rlog(const DsqRlogArgs *args, const DsqRlogOut *out);

/* ---- dsq_unmix: unmix() (R/helper.R:70-132) ------------------------------------------------------
 * Sample i, column i of x (n genes x m samples), is unmixed into k pure components (pure: n x k): minimise over the box
 * [lo, 100]^k     L_i(p) = sum_g | v(x_gi) - v(sum_j pure_gj p_j) |^power,     power 1 or 2,     from p = 1, with
 *   alpha given:   v(q) = (2 asinh(sqrt(alpha q)) - log alpha - log 4) / log 2,   lo = 1e-6
 *   shift given:   v(q) = log(q + shift),                                         lo = 0
 * R reaches the minimum by L-BFGS-B on numerical gradients; the library minimises the same objective on the same box by
 * its own deterministic iteration (projected Levenberg-Marquardt on the reweighted Gauss-Newton system, DESIGN.md
 * section 17), every operation rounded once in a stated order.  The caller forms mix = p / sum(p).
 * flag: 0 stopped by the tolerance or for lack of an improving step, 1 maxit reached, 2 the loss at the start is not
 * finite (p and loss of that sample are NaN).
 * _dev: device pointers, asynchronous on `stream`, no allocation, no host synchronisation; x gene-major with leading
 * dimension ld >= m (padding is not read), pure gene-major with k contiguous doubles per gene; workspace: at least
 * dsq_unmix_workspace_bytes(n, m, k) bytes (v(x), sample-major), else DSQ_ERR_ARG.
 * dsq_unmix: host pointers, x and pure in R layout (column-major), ONE device, synchronous; DSQ_ERR_VALUE for a negative
 * or non-finite entry of x or pure.  p comes back with the k values of a sample contiguous in both.
 * DSQ_ERR_ARG: k < 2, both or neither of alpha / shift, a non-positive or non-finite one, power outside {1, 2};
 * DSQ_ERR_UNSUPPORTED: k > DSQ_UNMIX_MAX_K.  All decided before a device is asked for.                                  */
#define DSQ_UNMIX_MAX_K 16
typedef struct {
    int32_t n, m, k;
    int64_t ld;                /* _dev: leading dimension of x (>= m); dsq_unmix: ignored                            */
    const double *x;           /* n x m                                                                             */
    const double *pure;        /* n x k                                                                             */
    int32_t has_alpha, has_shift;  /* exactly one of them                                                           */
    double alpha, shift;       /* the one that is given: finite, > 0                                                */
    int32_t power;             /* 1 or 2                                                                            */
    int32_t maxit;             /* >= 0; unmix(): 200                                                                */
} DsqUnmixArgs;

typedef struct {
    double *p;                 /* m x k, the k coefficients of a sample contiguous                                  */
    double *loss;              /* m                                                                                 */
    int32_t *iter;             /* m: iterations started                                                             */
    int32_t *flag;             /* m                                                                                 */
} DsqUnmixOut;

int64_t dsq_unmix_workspace_bytes(int32_t n, int32_t m, int32_t k);
int32_t dsq_unmix_block_threads(void);   /* the T of the summation order: thread t of T adds genes t, t + T, ...       */
int dsq_unmix_dev(const DsqUnmixArgs *args, const DsqUnmixOut *out, void *workspace, int64_t workspace_bytes, void *stream);
int dsq_unmix(const DsqUnmixArgs *args, const DsqUnmixOut *out);

/* ---- dsq_apeglm: apeglm shrinkage, lfcShrink(type = "apeglm") (R/lfcShrink.R:328-440) ------------
 * Per gene i, the coefficients b (natural-log scale) of a negative binomial GLM with dispersion a_i that minimise
 *     F_i(b) = - sum_j w_ij [ y_ij eta_ij - (y_ij + 1/a_i) log1p(a_i mu_ij) ]
 *              + sum_{k in no_shrink} b_k^2 / (2 no_shrink_scale^2)
 *              + sum_{k not in no_shrink} ((prior_df + 1) / 2) log1p(b_k^2 / (prior_df prior_scale^2)),
 *     eta = x b + log nf,  mu = exp(eta)
 * (a Student t prior, Cauchy at prior_df = 1, on the shrunken coefficients), the Laplace posterior SD
 * sd_k = sqrt((H(map)^-1)_kk) from the observed Hessian, and for the coefficient `coef`: fsr = pnorm(-|map| / sd) and, with
 * a threshold T, thresh = P(|b| < T) under N(map, sd^2).  The package reaches the mode by its own optimiser; the library
 * minimises the same F by its own deterministic damped Newton (Levenberg-Marquardt) iteration from two starts -- the
 * shrunken one (shrunken coefficients 0, column 0 at log(max(weighted mean of y / nf, 0.1)) when it is unshrunken), then
 * `init` clipped to +-30 when given -- and keeps the lower F (a tie: the first), every operation rounded once in a stated
 * order (tests/apeglm_spec.py).  Agreement with the package's numbers is not pinned.
 * conv: 0 an accepted undamped step with max |step| < tol, 1 maxit reached, 2 no acceptable step (or F not finite at the
 * start: objective NaN), + 4 when the Hessian at the point returned is not positive definite (sd, fsr, thresh NaN).
 * start: 0 the shrunken start won, 1 init.  iter: 2 per gene, the iterations from either start (0 without init).
 * A row whose counts are all zero or whose dispersion is NaN, infinite or not positive is not fitted: NaN everywhere.
 * map, sd, init: n x p with the p values of a gene contiguous, in both entries.  x: m x p column-major.
 * _dev: device pointers, asynchronous on `stream`, no allocation, no host synchronisation, no workspace; padding columns
 * m .. ld-1 of gene-major matrices are not read; a negative, non-finite or non-integer float64 count sets *bad.
 * dsq_apeglm: host pointers in R layout, ONE device, synchronous; DSQ_ERR_VALUE for such a count matrix.
 * DSQ_ERR_UNSUPPORTED: p > DSQ_APEGLM_MAX_P.  DSQ_ERR_ARG: coef out of range or inside no_shrink, a scale or df that is
 * not positive and finite, a negative or NaN threshold, tol NaN, maxit < 0.  All decided before a device is asked for. */
#define DSQ_APEGLM_MAX_P 16
typedef struct {
    int32_t n, m, p;
    int32_t layout;            /* DSQ_LAYOUT_* of y / nf (matrix) / weights                                         */
    int64_t ld;                /* leading dimension for DSQ_LAYOUT_GENE_MAJOR (>= m)                                */
    const void *y;             /* n x m counts                                                                      */
    int32_t y_type;            /* DSQ_Y_INT32 or DSQ_Y_FLOAT64                                                      */
    const double *nf;          /* m size factors (nf_is_vector) or n x m normalization factors in `layout`          */
    int32_t nf_is_vector;
    const double *x;           /* m x p design, column-major                                                        */
    const double *weights;     /* n x m in `layout`, >= 0, or NULL (all 1)                                          */
    const double *disp;        /* n                                                                                 */
    const double *init;        /* n x p (natural log), the second start, or NULL                                    */
    int32_t coef;              /* 0-based: the coefficient fsr / thresh are formed for                              */
    uint32_t no_shrink;        /* bit k set: column k gets Normal(0, no_shrink_scale^2); apeglm: column 0           */
    double prior_scale;        /* S > 0                                                                             */
    double prior_df;           /* > 0; apeglm: 1                                                                    */
    double no_shrink_scale;    /* > 0; apeglm: 15                                                                   */
    int32_t has_threshold;
    double threshold;          /* natural-log scale, >= 0; read when has_threshold                                  */
    double tol;                /* 1e-8                                                                              */
    int32_t maxit;             /* >= 0; 100.  0 returns the start                                                   */
} DsqApeglmArgs;

typedef struct {
    double *map;               /* n x p                                                                             */
    double *sd;                /* n x p                                                                             */
    double *fsr;               /* n                                                                                 */
    double *thresh;            /* n (NaN without a threshold)                                                       */
    double *iter;              /* n x 2                                                                             */
    double *conv;              /* n                                                                                 */
    double *start;             /* n                                                                                 */
    double *objective;         /* n: F at map                                                                       */
    int32_t *bad;              /* _dev: one device int32 the CALLER has zeroed, or NULL; dsq_apeglm: ignored        */
} DsqApeglmOut;

int32_t dsq_apeglm_lds_doubles(void);   /* the design is staged in LDS while m * p is at most this; read through L2 beyond */
int dsq_apeglm_dev(const DsqApeglmArgs *args, const DsqApeglmOut *out, void *stream);
int dsq_apeglm(const DsqApeglmArgs *args, const DsqApeglmOut *out);

/* ---- dsq_ash: adaptive shrinkage, lfcShrink(type = "ashr") (R/lfcShrink.R:442-486) -----------------
 * ashr::ash(betahat, sebetahat, mixcompdist = "normal", method = "shrink") as its paper (Stephens 2017) and the call state
 * it, for C independent columns (the K contrasts of one resultsContrasts call) of n rows each: a scale mixture of
 * zero-mean normals sum_k pi_k N(0, sigma_k^2) without a point mass is fitted to the kept rows (betahat finite, sebetahat
 * finite and positive) by maximum likelihood, then every kept row gets its posterior mean, posterior SD, the two sign
 * probabilities, lfsr = the smaller of them and, with a threshold T, P(beta <= T) and P(beta > -T), each as its own one-tail
 * sum.  Rows that are not kept take no part and come back NaN in every per-row output.  The grid is ashr's documented
 * gridmult = sqrt(2) rule from min(sebetahat) / 10 to 2 sqrt(max(betahat^2 - sebetahat^2)) (8 times the lower end when no row
 * has betahat^2 > sebetahat^2), K = npoint + 1 <= DSQ_ASH_MAX_K components, at least 2.  The weights minimise
 * phi(x) = -(1/n) sum_i log (L x)_i + sum_k x_k over x >= 0 by the library's own deterministic sequential quadratic
 * programme (active-set solve on the host, backtracking on the true phi with all step sizes of a search evaluated in one
 * pass), from x = 1/K until min_k g_k >= -1e-8; every operation rounded once in a stated order (DESIGN.md section 23,
 * deseq2_amd/ash_host.py, tests/ash_spec.py).  The ashr package's numbers, its optimiser and its treatment of excluded rows are
 * unpinned.
 * betahat, sebetahat and the seven per-row outputs: column c at [c * ld], ld >= n; rows n .. ld-1 are neither read nor written.
 * pi, sd: C x DSQ_ASH_MAX_K, row c the weights / standard deviations of column c, zero beyond its K.
 * flag: 0 converged, 1 maxit reached, 2 no acceptable step.  iter: the quadratic programmes solved.
 * Every sum over the rows takes them in slices of dsq_ash_slice_rows() consecutive rows, a slice in groups of 16, in an
 * order that depends on n and K alone; no floating-point atomics.
 * _dev: device pointers and the caller's workspace of at least dsq_ash_workspace_bytes(n, C) bytes (else DSQ_ERR_ARG), no
 * allocation.  The host decides every step from a record of (K+1)(K+2)/2 doubles per column, so the call SYNCHRONISES
 * `stream` (a few dozen times) and the outputs are complete on return; it cannot be captured into a graph.
 * dsq_ash: host pointers, ONE device, synchronous.
 * DSQ_ERR_VALUE: a column without a kept row.  DSQ_ERR_UNSUPPORTED: a column whose grid needs more than DSQ_ASH_MAX_K
 * components (max / min near 2^32).  DSQ_ERR_ARG: n or C < 1, ld < n, a NULL array, a negative or NaN threshold, maxit < 0:
 * decided before a device is asked for. */
#define DSQ_ASH_MAX_K 64
typedef struct {
    int32_t n, C;              /* rows, columns                                                                     */
    int64_t ld;                /* column stride of betahat / sebetahat and of the per-row outputs (>= n)            */
    const double *betahat;     /* n x C                                                                             */
    const double *sebetahat;   /* n x C                                                                             */
    int32_t has_threshold;
    double threshold;          /* T >= 0, on the scale of betahat; read when has_threshold                          */
    int32_t maxit;             /* >= 0; 100                                                                         */
} DsqAshArgs;

typedef struct {
    double *PosteriorMean;     /* n x C                                                                             */
    double *PosteriorSD;       /* n x C                                                                             */
    double *NegativeProb;      /* n x C                                                                             */
    double *PositiveProb;      /* n x C                                                                             */
    double *lfsr;              /* n x C                                                                             */
    double *le_T;              /* n x C: P(beta <= T)  (NaN without a threshold)                                    */
    double *gt_mT;             /* n x C: P(beta > -T)  (NaN without a threshold)                                    */
    double *pi;                /* C x DSQ_ASH_MAX_K                                                                 */
    double *sd;                /* C x DSQ_ASH_MAX_K                                                                 */
    int32_t *K;                /* C                                                                                 */
    int32_t *iter;             /* C                                                                                 */
    int32_t *flag;             /* C                                                                                 */
    double *loglik;            /* C: sum over the kept rows of log (L pi)_i + lnorm_i                               */
} DsqAshOut;

int64_t dsq_ash_workspace_bytes(int32_t n, int32_t C);
int32_t dsq_ash_slice_rows(void);
int dsq_ash_dev(const DsqAshArgs *args, const DsqAshOut *out, void *workspace, int64_t workspace_bytes, void *stream);
int dsq_ash(const DsqAshArgs *args, const DsqAshOut *out);

/* ---- dsq_sf_iterate: the solve of estimateSizeFactors(type = "iterate") (R/core.R:2600-2611) ------
 * One outer round of estimateSizeFactorsIterate fixes the counts k, q_ij = mu_ij / sf_j and the dispersions a_i over the
 * rows whose flag is set, and maximises over s (sum s = 0)
 *     F(s) = sum of L_i over the rows with L_i > quantile(L, Q),    L_i = sum_j log NB(k_ij; mu = q_ij exp(s_j), size = 1/a_i)
 * R hands F to optim(method = "L-BFGS-B") with numerical gradients; the library maximises the same F by its own
 * deterministic iteration -- on the kept set the objective separates in the samples, so Newton's step under the gauge is
 * closed, and an Armijo test on the true F (cut re-evaluated at every trial) safeguards it --, every operation rounded
 * once in a stated order (tests/sf_iterate_spec.py).
 * flag: 0 stopped by the tolerance, for lack of an ascent direction or on an empty kept set, 1 maxit reached or no
 * acceptable step, 2 F at the start is not finite.  iter: iterations started; evals: evaluations of F.
 * _dev: device pointers; y int32 and mu double, gene-major with leading dimension ld >= m (padding is not read; neither
 * buffer is written); the dispersion of a row whose flag is 0 is not read.  The host decides every step from a small
 * record it reads back, so the call SYNCHRONISES `stream` (a few dozen times) and the outputs are complete on return.
 * workspace: at least dsq_sf_iterate_workspace_bytes(n, m) bytes, else DSQ_ERR_ARG.
 * dsq_sf_iterate: host pointers, y and mu in R layout (column-major), ONE device, synchronous; DSQ_ERR_VALUE for a
 * negative count, a negative or non-finite mu, a size factor that is not positive and finite.
 * The column sums of the gradient add the genes in slices of dsq_sf_iterate_slice_genes() consecutive genes, each slice in
 * gene order, then the slices in order: the constant is part of the summation order.                                   */
typedef struct {
    int32_t n, m;
    int64_t ld;                /* _dev: leading dimension of y and mu (>= m); dsq_sf_iterate: ignored               */
    const int32_t *y;          /* n x m counts                                                                      */
    const double *mu;          /* n x m fitted means of the round                                                   */
    const double *sf;          /* m: the size factors mu was fitted with; the start is log(sf) - mean(log(sf))      */
    const double *disp;        /* n                                                                                 */
    const int32_t *rows;       /* n: non-zero = the row takes part (rowSums(counts) > 0)                            */
    double Q;                  /* in [0, 1); estimateSizeFactorsIterate(): 0.05                                     */
    int32_t maxit;             /* >= 0; optim(): 100                                                                */
} DsqSfIterateArgs;

typedef struct {
    double *s;                 /* m: the centred log size factors                                                   */
    double *sf;                /* m: exp(s)                                                                         */
    double *F;                 /* 1                                                                                 */
    int32_t *iter, *evals, *flag;   /* 1 each                                                                       */
} DsqSfIterateOut;

int64_t dsq_sf_iterate_workspace_bytes(int32_t n, int32_t m);
int32_t dsq_sf_iterate_slice_genes(void);
int dsq_sf_iterate_dev(const DsqSfIterateArgs *args, const DsqSfIterateOut *out, void *workspace, int64_t workspace_bytes, void *stream);
int dsq_sf_iterate(const DsqSfIterateArgs *args, const DsqSfIterateOut *out);

/* ---- dsq_top_var, dsq_sample_pairs: sample PCA and sample distances on a transform (R/plots.R:239-291, dist(t(assay(vsd)));
 *      DESIGN.md section 19) -------------------------------------------------------------------------------------------
 * x: n genes x m samples of float64 (what vst / rlog / normalized counts leave resident), m >= 2.
 * dsq_top_var: rowMean = (wave-order sum over the samples) / m, rowVar = (wave-order sum of (a - mean) (a - mean)) / (m - 1)
 * (matrixStats::rowVars as documented), and select = the first min(ntop, n) entries of order(rowVar, decreasing = TRUE):
 * ties by ascending row, NaN variances after every number by ascending row.  ntop = 0: the row statistics alone (select
 * may be NULL).
 * dsq_sample_pairs: out (m x m, symmetric on the bits) over the rows listed (`rows`, nrows entries, repeats allowed; NULL:
 * all n rows in order, nrows 0 or n):
 *   DSQ_PAIRS_DIST2   out[i,j] = sum_g (x[g,i] - x[g,j]) (x[g,i] - x[g,j]), the diagonal +0
 *   DSQ_PAIRS_DIST    its square root: as.matrix(dist(t(x))), method "euclidean" (dist's NA rescaling is not mirrored: a
 *                     NaN in a sample gives NaN in every pair with another sample)
 *   DSQ_PAIRS_GRAM    out[i,j] = sum_t c[t,i] c[t,j], c[t,.] = x[rows[t],.] - centre[t] (centre: one value per LISTED row,
 *                     or NULL: nothing is subtracted)
 * The order of every sum is part of the interface and depends on (rows summed, m) only: slices of
 * dsq_sample_pairs_slice_rows(rows summed, m) consecutive listed rows, each added in list order from +0.0, then the slice
 * partials in slice order.  No float atomics.
 * _dev: device pointers, asynchronous on `stream`; x gene-major with leading dimension ld >= m (padding is not read);
 * scratch comes from the workspace of the stream's context.  A listed row outside [0, n) is not read: its sums are NaN.
 * dsq_top_var / dsq_sample_pairs: host pointers, x in R layout (column-major), ONE device, synchronous; a listed row
 * outside [0, n) is DSQ_ERR_ARG.
 * DSQ_ERR_ARG: struct_size not sizeof the block, n < 1, m < 2, ld < m (_dev), ntop < 0, an unknown kind, nrows without rows
 * other than 0 or n, rows with nrows < 1, a NULL x or output.  All decided before a device is asked for.              */
#define DSQ_PAIRS_DIST2 0
#define DSQ_PAIRS_DIST 1
#define DSQ_PAIRS_GRAM 2
typedef struct {
    uint32_t struct_size;      /* sizeof(DsqTopVarArgs)                                                             */
    int32_t n, m;
    int64_t ld;                /* _dev: leading dimension of x (>= m); dsq_top_var: ignored                          */
    const double *x;           /* n x m                                                                             */
    int32_t ntop;              /* >= 0; min(ntop, n) entries of select are written; plotPCA(): 500                  */
} DsqTopVarArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqTopVarOut)                                                              */
    double *rowMean;           /* n                                                                                 */
    double *rowVar;            /* n                                                                                 */
    int32_t *select;           /* min(ntop, n) row indices (0-based); may be NULL when ntop = 0                     */
} DsqTopVarOut;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqSamplePairsArgs)                                                        */
    int32_t n, m;
    int64_t ld;                /* _dev: leading dimension of x (>= m); dsq_sample_pairs: ignored                     */
    const double *x;           /* n x m                                                                             */
    int32_t kind;              /* DSQ_PAIRS_*                                                                       */
    int32_t nrows;             /* entries of rows (and centre); without rows: 0 or n                                */
    const int32_t *rows;       /* nrows row indices (0-based), or NULL: every row                                   */
    const double *centre;      /* DSQ_PAIRS_GRAM: one value per listed row, or NULL; other kinds: ignored           */
} DsqSamplePairsArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqSamplePairsOut)                                                         */
    double *out;               /* m x m                                                                             */
} DsqSamplePairsOut;

int64_t dsq_sample_pairs_slice_rows(int64_t rows_summed, int32_t m);   /* the L of the summation order               */
int32_t dsq_row_vars_register_width(void);   /* rows of up to this many samples are read once by the row-variance kernel */
int dsq_top_var_dev(const DsqTopVarArgs *args, const DsqTopVarOut *out, void *stream);
int dsq_top_var(const DsqTopVarArgs *args, const DsqTopVarOut *out);
int dsq_sample_pairs_dev(const DsqSamplePairsArgs *args, const DsqSamplePairsOut *out, void *stream);
int dsq_sample_pairs(const DsqSamplePairsArgs *args, const DsqSamplePairsOut *out);

/* ---- dsq_collapse, dsq_col_sums, dsq_fpm: collapseReplicates, colSums and fpm / fpkm on the count matrix
 *      (R/helper.R:187-216, 291-391) ---------------------------------------------------------------
 * y: n genes x m samples of int32 counts.
 * dsq_collapse: out[i,c] = the sum over the samples of group c of y[i,.] (sapply(sp, function(i) rowSums(y[,i])) with
 * mode "integer"), accumulated in int64.  The g groups are split(seq(along = groupby), groupby) as a CSR pair: members
 * holds the m sample indices (0-based), group 0's in ascending order, then group 1's, ...; offsets holds g + 1 entries,
 * offsets[0] = 0, offsets[g] = m, group c = members[offsets[c] .. offsets[c+1]).  A sum that is no int32 (R: NA from
 * mode<-) ORs 1 into *status and leaves that element unspecified.
 * dsq_col_sums: sums[j] = the sum over the genes of y[.,j] in int64: exact, whatever the order (integer atomics).  The
 * double colSums() returns is (double)sums[j]: one rounding, to nearest even.
 * dsq_fpm: one elementwise pass, every operation IEEE double in R's order and rounded once (no reciprocal, no folded
 * constant); k = (double)y[i,j]:
 *   DSQ_FPM             out[i,j] = 1e6 * (k / lib[j])                              R/helper.R:390
 *   DSQ_FPKM_BASEPAIRS  out[i,j] = 1e3 * ((1e6 * (k / lib[j])) / basepairs[i])     R/helper.R:322
 *   DSQ_FPKM_TXLEN      out[i,j] = (1e3 * (1e6 * (k / lib[j]))) / txlen[i,j]       R/helper.R:294
 * lib: the m library sizes (colSums, or sizeFactors * exp(mean(log(colSums))): the caller's m numbers).  A zero library
 * size gives NaN (0/0) or Inf, a NaN one NaN, as in R.
 * _dev: device pointers, asynchronous on `stream`, nothing allocated, no host synchronisation; y gene-major with leading
 * dimension ld >= m (padding is neither read nor written); txlen and the output of dsq_fpm_dev share y's ld; the output
 * of dsq_collapse_dev has its own (>= g).  *status is zeroed by the caller.  members and offsets are device memory the
 * entry cannot look at: an offset outside [0, m] is clipped, a member outside [0, m) is not read, and either ORs 2 into
 * *status.
 * dsq_collapse / dsq_col_sums / dsq_fpm: host pointers, matrices in R layout (column-major), ONE device, synchronous.
 * dsq_collapse returns DSQ_ERR_VALUE when a sum is no int32 (out is then unspecified) and refuses members / offsets
 * that are not such a CSR pair with DSQ_ERR_ARG.
 * DSQ_ERR_ARG: struct_size not sizeof the block, n < 1, m < 1, g < 1 or g > m, ld < m or an output ld < g (_dev), an
 * unknown kind, a NULL pointer the kind needs.  All decided before a device is asked for.                              */
#define DSQ_FPM 0
#define DSQ_FPKM_BASEPAIRS 1
#define DSQ_FPKM_TXLEN 2
typedef struct {
    uint32_t struct_size;      /* sizeof(DsqCollapseArgs)                                                           */
    int32_t n, m, g;           /* genes, samples, groups (1 <= g <= m)                                              */
    int64_t ld;                /* _dev: leading dimension of y (>= m); dsq_collapse: ignored                         */
    const int32_t *y;          /* n x m                                                                             */
    const int32_t *members;    /* m sample indices, group by group                                                  */
    const int32_t *offsets;    /* g + 1                                                                             */
} DsqCollapseArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqCollapseOut)                                                            */
    int64_t ld;                /* _dev: leading dimension of out (>= g); dsq_collapse: ignored                       */
    int32_t *out;              /* n x g                                                                             */
    int32_t *status;           /* _dev: one word, zeroed by the caller; dsq_collapse: may be NULL                   */
} DsqCollapseOut;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqColSumsArgs)                                                            */
    int32_t n, m;
    int64_t ld;                /* _dev: leading dimension of y (>= m); dsq_col_sums: ignored                         */
    const int32_t *y;          /* n x m                                                                             */
} DsqColSumsArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqColSumsOut)                                                             */
    int64_t *sums;             /* m                                                                                 */
} DsqColSumsOut;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqFpmArgs)                                                                */
    int32_t n, m;
    int64_t ld;                /* _dev: leading dimension of y, txlen and out (>= m); dsq_fpm: ignored               */
    const int32_t *y;          /* n x m                                                                             */
    int32_t kind;              /* DSQ_FPM, DSQ_FPKM_BASEPAIRS, DSQ_FPKM_TXLEN                                       */
    const double *lib;         /* m library sizes                                                                   */
    const double *basepairs;   /* DSQ_FPKM_BASEPAIRS: n feature lengths; other kinds: ignored                       */
    const double *txlen;       /* DSQ_FPKM_TXLEN: n x m average transcript lengths; other kinds: ignored            */
} DsqFpmArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqFpmOut)                                                                 */
    double *out;               /* n x m                                                                             */
} DsqFpmOut;

int dsq_collapse_dev(const DsqCollapseArgs *args, const DsqCollapseOut *out, void *stream);
int dsq_collapse(const DsqCollapseArgs *args, const DsqCollapseOut *out);
int dsq_col_sums_dev(const DsqColSumsArgs *args, const DsqColSumsOut *out, void *stream);
int dsq_col_sums(const DsqColSumsArgs *args, const DsqColSumsOut *out);
int dsq_fpm_dev(const DsqFpmArgs *args, const DsqFpmOut *out, void *stream);
int dsq_fpm(const DsqFpmArgs *args, const DsqFpmOut *out);

/* ---- dsq_local_fit: the local-regression dispersion trend, estimateDispersionsFit(fitType = "local") (R/core.R:889-893,
 *      localDispersionFit :2194-2203) ------------------------------------------------------------
 * The estimator behind locfit(logDisps ~ logMeans, weights = means) with locfit's defaults: nearest-neighbour fraction 0.7,
 * local quadratic, tricube kernel, Gaussian family, prior weights times kernel weights -- evaluated directly at every
 * requested mean (locfit's ev = dat()).  locfit evaluates on the vertices of an adaptive tree and interpolates: agreement
 * with its interpolated values is not claimed.
 * means / disps: what the caller offers to the fit (R: the useForFit rows).  The fit set is the rows with
 * 10 minDisp <= disps < Inf and 0 < means < Inf, N of them: x = log(means), y = log(disps), w = means, sorted by x, ties by
 * row.  N = 0 (all below the floor): the trend is the constant minDisp.  k = floor(7 N / 10) points per window; k < 3 is
 * "fewer than 3 points in a window": every value NaN, DSQ_ERR_FIT from the host entry.
 * At a mean q, z = log(q): the k nearest x are a window [l, l + k) of the sorted set, h the k-th smallest |x - z|,
 * t = (x - z) / h, W = w (1 - |t|^3)^3 for |t| < 1; S_r = sum W t^r (r = 0..4), T_r = sum W t^r y (r = 0..2); the value is
 * exp(a0), a0 the intercept of the 3 x 3 normal equations by elimination without pivoting.  A window with fewer than three
 * distinct x of positive weight, or a pivot that is not > 0, gives NaN and is counted; so does a q that is NaN, <= 0 or Inf
 * (not counted).  log / exp: the library's pinned arithmetic.
 * The order of the eight sums is part of the interface and depends on (l, k) only: dsq_local_fit_lanes() partial sums,
 * partial (j mod lanes) adds the window's points in ascending sorted index j from +0.0; the partials are then added
 * pairwise, partial i with partial i xor 1, then xor 2, 4, 8, 16, 32.  No atomics.
 * The fit handle: out->fit, dsq_local_fit_block_doubles(n) doubles (a header, then x | y | w in sorted order).  A later call
 * with args->fit_in pointing at it (and the same n) evaluates without fitting again: the same bits as a fresh call.
 * Evaluation points: eval_means (n_eval of them); eval_means NULL and dispFit given: the n means themselves.  dispFit NULL:
 * the fit is built and nothing is evaluated.
 * status[0..3]: N, k, the number of singular evaluation points, 1 when all rows were below the floor.
 * _dev: device pointers, asynchronous on `stream`, no host synchronisation: N and k stay on the device between the fit and
 * the evaluation.  out->fit NULL: the block lives in the workspace of the stream's context until the next call.
 * dsq_local_fit: host pointers, ONE device, synchronous; fit / fit_in are host copies of the block.
 * DSQ_ERR_ARG: struct_size not sizeof the block, n < 1, a NULL status, means / disps NULL without fit_in, fit_in without
 * eval_means and dispFit, n_eval < 0 or without eval_means, minDisp not > 0.  All decided before a device is asked for.    */
typedef struct {
    uint32_t struct_size;      /* sizeof(DsqLocalFitArgs)                                                           */
    int32_t n;                 /* rows of means / disps; with fit_in: the n its block was built with                */
    const double *means;       /* n, or NULL with fit_in                                                            */
    const double *disps;       /* n, or NULL with fit_in                                                            */
    double minDisp;            /* R: 1e-8                                                                           */
    const double *fit_in;      /* NULL: fit (means, disps); else the block of an earlier call: evaluate only        */
    int32_t n_eval;            /* entries of eval_means (0 without)                                                 */
    const double *eval_means;  /* n_eval means, or NULL: evaluate at `means`                                        */
} DsqLocalFitArgs;

typedef struct {
    uint32_t struct_size;      /* sizeof(DsqLocalFitOut)                                                            */
    double *fit;               /* dsq_local_fit_block_doubles(n), or NULL: not kept                                 */
    double *dispFit;           /* one value per evaluation point, or NULL: fit only                                 */
    int32_t *status;           /* 4 words                                                                           */
} DsqLocalFitOut;

int32_t dsq_local_fit_lanes(void);                  /* the partial sums of the summation order                       */
int64_t dsq_local_fit_block_doubles(int32_t n);     /* the size of a fit handle, in doubles                           */
int dsq_local_fit_dev(const DsqLocalFitArgs *args, const DsqLocalFitOut *out, void *stream);
int dsq_local_fit(const DsqLocalFitArgs *args, const DsqLocalFitOut *out);

/* ---- dsq_results: results() for one coefficient (R/results.R:443-575, 638-740) -------------------
 * The table -- baseMean, log2FoldChange, lfcSE, stat, pvalue of design column c --, the threshold tests of :484-515 under
 * the normal distribution, pvalue NA where na_mask is set (the Cook's filter of :520-564 is the caller's: a host decision
 * over a handful of rows), the nowZero fill of :567-575, then independent filtering: cutoffs = quantile(filter, theta)
 * (type 7), filtPadj[, k] = p.adjust(pvalue[filter >= cutoffs[k]], "BH") for all K cutoffs from ONE radix sort of the
 * p-values, numRej[k] = sum(filtPadj[, k] < alpha, na.rm = TRUE).  Which column becomes padj (the lowess rule of :661-692)
 * is the caller's decision over K numbers.  independentFiltering = 0: K = 1, theta ignored, filtPadj is p.adjust(pvalue, "BH").
 * NA is NaN.  BH is global over the genes: nothing here is sharded, dsq_results runs on ONE device.
 * Wald: beta, betaSE, stat, pvalue are n x p column-major and column c is read; LRT: stat / pvalue are the n-vectors
 * LRTStatistic / LRTPvalue.  A threshold test (lfcThreshold > 0 or altHypothesis != DSQ_ALT_GREATER_ABS) recomputes stat and
 * pvalue from log2FoldChange and lfcSE and needs test = DSQ_TEST_WALD.
 * _dev: device pointers (theta too), asynchronous on `stream`, no allocation, no host synchronisation.  What cannot be seen
 * without reading device memory comes back in *status: bit 0 = NaN in filter, bit 1 = a theta outside [0, 1]; dsq_results
 * checks both on the host and returns DSQ_ERR_ARG.  workspace: dsq_results_workspace_bytes(n, K) bytes =
 * dsq_results_workspace_bytes(n, 0) for the sort + n K doubles, where filtPadj lives when out.filtPadj is NULL.        */
enum { DSQ_TEST_WALD = 0, DSQ_TEST_LRT = 1 };
enum { DSQ_ALT_GREATER_ABS = 0, DSQ_ALT_LESS_ABS = 1, DSQ_ALT_GREATER = 2, DSQ_ALT_LESS = 3, DSQ_ALT_GREATER_ABS_2014 = 4 };
#define DSQ_RESULTS_MAX_K 4096
typedef struct {
    int32_t n, p, c;               /* genes, design columns, the coefficient 0 .. p-1                                */
    int32_t test;                  /* DSQ_TEST_*                                                                     */
    const double *beta, *betaSE;   /* n x p column-major, log2 scale                                                 */
    const double *stat, *pvalue;   /* Wald: n x p column-major; LRT: n                                               */
    const double *baseMean;        /* n                                                                              */
    const int32_t *replace;        /* n (1 = replaced; anything else, NA = -1 included, is not), or NULL             */
    const int32_t *na_mask;        /* n flags: pvalue <- NA, or NULL                                                 */
    double lfcThreshold;           /* >= 0                                                                           */
    int32_t altHypothesis;         /* DSQ_ALT_*                                                                      */
    int32_t independentFiltering;  /* 0: K must be 1                                                                 */
    const double *filter;          /* n, or NULL = baseMean; no NaN                                                  */
    const double *theta;           /* K quantile levels in [0, 1] (independentFiltering = 0: ignored, may be NULL)   */
    int32_t K;                     /* 2 .. DSQ_RESULTS_MAX_K, or 1 with independentFiltering = 0                     */
    double alpha;                  /* in (0, 1)                                                                      */
    void *workspace;               /* device; dsq_results: ignored                                                   */
    int64_t workspace_bytes;
    const double *df;              /* n degrees of freedom (a useT analysis, mcols tDegreesFreedom): the threshold tests
                                      take pt(., df[i]) for pnorm (R/results.R:477-515), NaN df = NaN pvalue; NULL: normal */
} DsqResultsArgs;

typedef struct {
    double *baseMean, *log2FoldChange, *lfcSE, *stat, *pvalue;   /* n each                                           */
    double *filtPadj;              /* n x K column-major (one cutoff = one contiguous column); _dev: NULL = in the workspace */
    int32_t *numRej;               /* K                                                                              */
    double *cutoffs;               /* K (independentFiltering = 0: -Inf)                                             */
    int32_t *status;               /* 1 value, see above                                                             */
} DsqResultsOut;

int dsq_results_dev(const DsqResultsArgs *args, const DsqResultsOut *out, void *stream);
/* host pointers, one device, synchronous */
int dsq_results(const DsqResultsArgs *args, const DsqResultsOut *out);
int64_t dsq_results_workspace_bytes(int32_t n, int32_t K);

/* ---- dsq_contrasts: K contrasts of the fitted coefficients from ONE covariance pass per gene ----
 * getContrast (R/results.R:760-827) re-enters fitBeta with maxit = 0 once per contrast; everything in front of the pair
 * (c' beta, sqrt(c' Sigma c)) -- the fitted means mu = max(nf exp(x beta), minmu), w = [weights] mu / (1 + alpha mu),
 * G = X'WX, Gi = (G + diag(lambda))^-1, Sigma = (Gi G) Gi (src/DESeq2.cpp:430-455) -- is the same for every contrast and
 * is built here once per gene.  Per contrast k: log2FoldChange = L c_k' beta, lfcSE = L sqrt(c_k' Sigma c_k) with
 * L = log2(exp(1)), stat = log2FoldChange / lfcSE, pvalue = 2 pnorm(|stat|, lower.tail = FALSE) (:809-817), each the bits
 * of dsq_fit_beta_dev(contrast = c_k, maxit = 0): the Gram sums take the cell-collapsed form for the designs that entry
 * fits on design cells (cell_of given, at most 32 cells, p <= 32) and the per-sample wave-order form otherwise.
 * The all-zero rule of cleanContrast (:1021-1028): where rule_applies[k] is set and every count of the gene under
 * sample_mask[k] is 0, contrastAllZero = 1 and log2FoldChange = 0, stat = 0, pvalue = 1 (lfcSE keeps its value).  The
 * masks read `counts` -- the ORIGINAL counts, as contrastAllZeroCharacter / contrastAllZeroNumeric do (:1239, :1268); the
 * covariance reads no counts at all (at maxit = 0 nothing does).  Rows flagged in allZero: NaN in the four columns, flag 0.
 * contrasts == NULL with masks given: flags only -- no covariance, the four table outputs are not written (may be NULL).
 * n x m matrices (nf as a matrix, weights, counts) are gene-major with leading dimension ld; x is m x p column-major,
 * beta n x p column-major on the NATURAL-log scale, contrasts p x K column-major (contrast k at contrasts + k p),
 * sample_mask K x m with mask k at sample_mask + k m; outputs n x K column-major.  K has no upper limit.
 * _dev: device pointers (cell_of excepted), asynchronous on `stream`, no host synchronisation, no float atomics.  The
 * p x p matrices of a gene live in LDS next to its m weights: m <= dsq_contrasts_max_m(p) on the per-sample path (7712 at
 * p = 64, 17040 at p = 32), else DSQ_ERR_UNSUPPORTED; the cell path has no such limit.
 * dsq_contrasts: host pointers, n x m matrices in R layout (column-major), ONE device, synchronous; the design cells are
 * derived from x when cell_of is NULL, as dsq_fit_beta does.                                                            */
typedef struct {
    int32_t n, m, p, K;
    int64_t ld;                    /* _dev: leading dimension of the gene-major n x m matrices (>= m); dsq_contrasts: ignored */
    const double *x;               /* m x p model matrix the coefficients were fitted on, column-major                  */
    const double *nf;              /* n x m normalization factors, or (nf_is_vector) the m size factors                 */
    int32_t nf_is_vector;
    const double *alpha_hat;       /* n dispersions                                                                     */
    const double *beta;            /* n x p column-major, natural-log scale (log(2) * mcols beta)                       */
    const double *lambda;          /* p ridge values, natural-log scale (1 / (log(2)^2 betaPriorVar))                   */
    const double *weights;         /* n x m observation weights (normalised, R/results.R:787-795); NULL when useWeights == 0 */
    int32_t useWeights;
    double minmu;
    const double *contrasts;       /* p x K column-major, or NULL: flags only                                           */
    const int32_t *allZero;        /* n flags, or NULL                                                                  */
    const int32_t *counts;         /* n x m int32 ORIGINAL counts; needed if and only if sample_mask is given           */
    const int32_t *sample_mask;    /* K x m of 0 / 1, or NULL: no all-zero rule                                         */
    const int32_t *rule_applies;   /* K flags (with sample_mask)                                                        */
    const int32_t *cell_of;        /* extension: design cells as in DsqFitBetaArgs (HOST, m labels, may be NULL)        */
    int32_t ncell;
    const double *df;              /* n degrees of freedom or NULL.  Given: pvalue = 2 pt(|stat|, df[i], lower.tail = FALSE)
                                      (R/results.R:812-815) by a dsq_pt_dev pass behind the kernel; entries the all-zero
                                      rule has set to 1 keep it even where df is NA                                     */
} DsqContrastsArgs;

typedef struct {
    double *log2FoldChange, *lfcSE, *stat, *pvalue;   /* n x K column-major (flags only: not written, may be NULL)      */
    int32_t *contrastAllZero;                         /* n x K column-major; may be NULL when no mask is given          */
} DsqContrastsOut;

int dsq_contrasts_dev(const DsqContrastsArgs *args, const DsqContrastsOut *out, void *stream);
int dsq_contrasts(const DsqContrastsArgs *args, const DsqContrastsOut *out);
int32_t dsq_contrasts_max_m(int32_t p);   /* longest row the per-sample path takes at p design columns */

/* ---- dsq_pt: Student's t distribution function, elementwise ---------------------------------
 * out[i + n k] = pt(q[i + n k], df[i]) for real df > 0 in the engine's pinned f64 arithmetic (deseq2_amd/student_t.py states
 * it operation for operation): q and out n x K column-major, row i's df for every column.  As R's pt: NaN in either
 * argument or df <= 0 gives NaN, q = -Inf / +Inf the lower tail 0 / 1, df = +Inf the normal distribution; the lower tail of q
 * has the bits of the upper tail of -q.  Relative error: the tests assert 1e-12 wherever the exact value is a normal number
 * (tails of 1e-300 included; q^2 may overflow); measured on their 2374-point grid against 50-digit values: 1.4e-13 at most.  keep: n x K flags or NULL -- where non-zero, out is not written.  out == q is allowed.
 * _dev: device pointers, asynchronous on `stream`, no allocation, no host synchronisation, one thread per entry.
 * dsq_pt: host pointers, one device, synchronous.                                                                       */
enum { DSQ_PT_LOWER = 0, DSQ_PT_UPPER = 1, DSQ_PT_TWO_SIDED = 2 };   /* TWO_SIDED: 2 * upper(|q|) */
int dsq_pt_dev(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const int32_t *keep, double *out,
               void *stream);
int dsq_pt(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const int32_t *keep, double *out);

/* ---- dsq_deseq: DESeq() behind ONE host-pointer call ------------------------------------------------------------
 * What an R session binds as .Call("_DESeq2_mi355x_DESeq", ...) in place of the body of DESeq() between
 * estimateSizeFactors (dsq_size_factors above) and the final bookkeeping (R/core.R:388-426: estimateDispersions -> nbinomWaldTest / nbinomLRT
 * -> refitWithoutOutliers): every array is a HOST pointer in R's layout (what INTEGER() / REAL() give), the call
 * uploads the count matrix ONCE through pinned staging, runs the device-driven chain of dsq_deseq_dev (all four
 * phases, the optim-fallback rows included, no host decision in between), and downloads the per-gene columns; the
 * n x m assays (mu, H, cooks, replaceCounts) come down only when their output pointer is non-NULL.  Like the three
 * classic routines it cuts the genes into the contiguous ranges of R/parallel.R:10, one per visible device
 * (DSQ_HOST_DEVICES / DSQ_HOST_SHARDS as there); the ranges exchange the two n-vectors of the dispersion trend
 * through host memory, as DESeqParallel does (R/parallel.R:27-40).
 * Covers what the fused chain covers: parametric trend, fitType "mean" or the caller's own trend (geneEstOnly / dispFit), Wald (also with betaPrior = TRUE) or LRT (any nested reduced model), p <= DSQ_MAX_P
 * (wide designs, 10 < p, included: observation weights, reduced models of any width < p and the beta-prior pass since round 5),
 * m - p > 3, size factors or a normalization-factor matrix, observation weights; anything else returns
 * DSQ_ERR_UNSUPPORTED and the caller keeps to the three classic routines.  The design-only quantities R has functions
 * for are passed in: qr.Q / qr.R of the model matrix (R/fitNbinomGLMs.R:139-143), qf(.99, p, m - p) (R/core.R:2081),
 * trigamma((m - p) / 2) (R/core.R:1196).
 * NA convention of the outputs: NaN in double columns, -1 in int32 columns (allZero rows; R/core.R:2534-2536).     */
typedef struct {
    int32_t n, m, p;
    const void *counts;            /* n x m column-major                                                          */
    int32_t y_type;                /* DSQ_Y_INT32 (counts(dds)) or DSQ_Y_FLOAT64                                  */
    const double *x;               /* m x p model matrix, column-major, full rank                                 */
    const double *sizeFactors;     /* m, or NULL when normalizationFactors is given                               */
    const double *normalizationFactors;  /* n x m column-major (normalizationFactors(object)), or NULL.  With a matrix the
                                      genes stay in ONE range (momentsDispEstimate averages the factors over all non-zero
                                      rows -- and, in the outlier refit, over the refitted rows, R/core.R:2440-2444 --
                                      sums a split could only reproduce in another order)                            */
    const double *weights;         /* n x m column-major (assays(object)[["weights"]]), or NULL                   */
    const double *q, *r;           /* qr.Q(qr(x)) (m x p) and qr.R(qr(x)) (p x p), column-major                   */
    const double *xrinv;           /* x %*% solve(R) (m x p), or NULL: computed here by back substitution         */
    int32_t test;                  /* 0 Wald, 1 LRT (reduced = ~1 unless x_reduced is given)                      */
    const double *x_reduced;       /* LRT: the reduced model matrix (m x p_reduced, nested in x, full rank) with its  */
    const double *q_reduced, *r_reduced;   /* qr.Q / qr.R, or all NULL for reduced = ~1 (R/core.R:1856-1868)          */
    int32_t p_reduced;
    double minReplicatesForReplace;/* 7 by default; +Inf switches replaceOutliers / the refit off                 */
    double cooksCutoff;            /* qf(.99, p, m - p)                                                           */
    double expVarLogDisp;          /* trigamma((m - p) / 2)                                                       */
    double betaTol, minmu;         /* nbinomWaldTest / nbinomLRT: 1e-8, 0.5                                       */
    int32_t maxit, useQR;          /* 100, TRUE                                                                   */
    int32_t disp_maxit, useCR;     /* estimateDispersions: 100, TRUE                                              */
    const double *disp_grid;       /* fitDispGridWrapper's seq(log(1e-8), log(max(10, m)), length = 20) (R/wrappers.R:70-72) */
    int32_t ngrid;                 /*   as the caller's own log() gives it; NULL / 0: computed here                */
    /* nbinomWaldTest(betaPrior = TRUE) (R/core.R:1416-1432 -> fitGLMsWithPrior, R/fitNbinomGLMs.R:242-337), Wald only:
     * the MLE pass on x, the all-gene prior variance (estimateBetaPriorVar, R/core.R:1601-1689: dsq_beta_prior_var
     * below, run inside the call on the MLE coefficients of ALL gene ranges), then the pass with lambda = 1 /
     * betaPriorVar on the standard model matrix (x_prior NULL) or on the expanded one (R/expanded.R:1-18).  beta,
     * betaSE, stat and pvalue are then n x p_prior.  The refit of the replaced rows reuses the prior variance
     * (R/core.R:2521-2527).                                                                                        */
    int32_t betaPrior;
    const double *x_prior;         /* expanded model matrix, m x p_prior column-major (same design cells as x), or NULL  */
    int32_t p_prior;               /* columns of x_prior (ignored when x_prior is NULL: p)                         */
    const int32_t *coef_factor;    /* p: what each column of x is -- 0 the intercept, f >= 1 an indicator of a level of
                                      design factor f, -1 anything else (numeric covariate, interaction)            */
    const int32_t *prior_coef_factor;  /* p_prior, the same for the columns of x_prior (expanded only)               */
    const int32_t *prior_coef_src;     /* p_prior: for the -1 columns of x_prior the column of x with the same name   */
    const double *betaPriorVar;    /* optional, p_prior values: the caller's prior variance (nbinomWaldTest's argument);
                                      NULL = estimated                                                              */
    int32_t fitType;               /* DSQ_FIT_PARAMETRIC (0, the default of DESeq()), DSQ_FIT_MEAN, DSQ_FIT_PARAMETRIC_OR_MEAN;
                                      dispersionFunction[DSQ_SC_FIT_USED] says which trend the results carry          */
    /* a trend this entry does not fit -- fitType = "local" (R/core.R:889-893: dsq_local_fit between the two calls, or R's own
     * locfit) or `dispersionFunction<-` (R/methods.R:142-190) -- in two calls: geneEstOnly = 1 runs estimateDispersionsGeneEst only (baseMean, baseVar,
     * allZero, dispGeneEst, dispGeneIter come back; every other column NA); the caller fits its trend and calls again with
     * dispFit = its values at baseMean (host, n; rows that are all zero: anything).  Count outliers are then flagged by
     * Cook's distance as always, but NOT replaced: the refit needs the trend at the new means of the replaced rows, so the
     * caller runs refitWithoutOutliers itself on the (few) rows concerned (R/core.R:2484-2563, unchanged code).        */
    const double *dispFit;
    int32_t geneEstOnly;
    double dispPriorVar;           /* > 0: estimateDispersionsMAP(dispPriorVar = x), R/core.R:989-994 -- required when m - p <= 3
                                      (R's estimate there is a seeded Monte-Carlo match over the residuals of the trend,
                                      R/core.R:1155-1190: after the geneEstOnly call the caller has what it needs)       */
} DsqDeseqHostArgs;

typedef struct {
    /* mcols(dds): n each (beta .. pvalue: n x p column-major, log2 scale; stat / pvalue Wald only, else NULL)     */
    double *baseMean, *baseVar;
    int32_t *allZero;
    double *dispGeneEst;
    int32_t *dispGeneIter;
    double *dispFit, *dispMAP, *dispersion;
    int32_t *dispIter, *dispOutlier;
    double *beta, *betaSE, *stat, *pvalue;
    int32_t *betaConv;
    double *betaIter, *logLike, *logLikeReduced /* LRT only, else NULL */, *maxCooks;
    int32_t *replace;              /* NA (-1) on rows that were all zero from the start                           */
    int32_t *weightsFail;          /* optional (NULL): rows whose weights leave a degenerate design, treated as all zero
                                      (getAndCheckWeights, R/core.R:2736-2747)                                    */
    /* assays, n x m column-major, each optional (NULL = stays on the device)                                      */
    double *mu, *H, *cooks;
    int32_t *replaceCounts;
    /* dispersionFunction(dds), indexed by DSQ_SC_*: coefficients asymptDisp / extraPois (fitType "mean": the mean, 0),
     * varLogDispEsts, dispPriorVar, the fit type used                                                             */
    double dispersionFunction[8];
    int32_t status[16];            /* DSQ_ST_*                                                                    */
    /* betaPrior = TRUE: the prior variance used (attr(object, "betaPriorVar")) and, optionally, the n x p MLE
     * coefficients (mcols MLE_*, log2 scale)                                                                      */
    double betaPriorVar[DSQ_MAX_P];
    double *mle_beta;
} DsqDeseqHostOut;

int dsq_deseq(const DsqDeseqHostArgs *args, DsqDeseqHostOut *out);

/* estimateBetaPriorVar (R/core.R:1601-1689, betaPriorMethod = "weighted", upperQuantile = 0.05) on HOST arrays: the
 * n x p MLE coefficients (log2 scale, column-major), baseMean, dispFit, the all-zero flags of the rows; the column
 * coding of DsqDeseqHostArgs.  No device work (an all-gene step on n-vectors like the dispersion trend; a stable radix
 * sort and sequential sums).  betaPriorVar: p values, or p_prior for the expanded model matrix.                    */
typedef struct {
    int32_t n, p;
    const double *mle_beta, *baseMean, *dispFit;
    const int32_t *allZero;
    const int32_t *coef_factor;
    int32_t expanded, p_prior;
    const int32_t *prior_coef_factor, *prior_coef_src;
    double upperQuantile;
} DsqBetaPriorArgs;
int dsq_beta_prior_var(const DsqBetaPriorArgs *args, double *betaPriorVar);

/* The device twin (csrc/beta_prior.hip): the same definition, the same bits.  mle_beta, baseMean,
 * dispFit and allZero are DEVICE pointers (the n x p matrix column-major = coefficient-major, as the fits leave it); the
 * column coding (coef_factor, prior_coef_factor, prior_coef_src) and betaPriorVar stay HOST arrays of a few values.  The
 * matched columns -- the p design columns, then for the expanded matrix the differences beta_i - beta_j of every pair of
 * a factor's level columns in addAllContrasts' order (R/expanded.R:76-98), formed in the kernel and never stored -- are
 * sorted a batch at a time by the radix sort of results(), the order-sensitive sums (sum of the weights in row order, the
 * weight sums of equal values and their running total in sorted order) are carried by one wave per column, add for add
 * as dsq_beta_prior_var states them.  dsq_beta_prior_var_columns(args) such columns; workspace: device memory of
 * dsq_beta_prior_var_workspace_bytes(n, columns) bytes (bounded in n x columns: the columns go through in batches).
 * Enqueues on `stream`, waits for it ONCE to bring the `columns` variances down, and runs the O(columns) closing steps
 * (the intercept's 1e6, averagePriorsOverLevels) on the host exactly as dsq_beta_prior_var does.                     */
int dsq_beta_prior_var_dev(const DsqBetaPriorArgs *args, double *betaPriorVar, void *workspace, int64_t workspace_bytes,
                           void *stream);
int32_t dsq_beta_prior_var_columns(const DsqBetaPriorArgs *args);    /* reads n, p, coef_factor, expanded; 0: bad args */
int64_t dsq_beta_prior_var_workspace_bytes(int32_t n, int32_t columns);

/* kernel timings of the calls since dsq_profile_enable(1): one entry per bracketed launch */
int dsq_profile_count(void);
int dsq_profile_get(int i, char *name, int cap, int32_t *genes, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* DESEQ2_MI355X_H */
