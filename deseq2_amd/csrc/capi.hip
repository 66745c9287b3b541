// capi.hip -- the C ABI of libdeseq2_mi355x.so (include/deseq2_mi355x.h), device-pointer half.
//
// Host side of the engine, in three files:
//   ctx.hip        the per-(device, stream) context (workspace slots, pinned upload ring, side stream), the error text,
//                  the tuning knobs, the profile list and the entry points that manage them;
//   capi.hip       (this file) each call's argument checks (check_<call>: stated once, used by both halves), layout
//                  conversion (R column-major <-> gene-major: GmIn for the inputs, GmOut for the n x m outputs), kernel
//                  dispatch on the design width p, and the device-pointer entry points dsq_*_dev (dev_entry);
//   capi_host.hip  the host-pointer entry points the R .Call shim binds: staging (struct Stage), gene ranges, worker threads.
// A body here reads: check_<call>, the device, an empty call returns DSQ_OK, inputs, outputs, launch, finish.
// No CPU fallback: if HIP cannot give us a device, every entry point fails with DSQ_ERR_DEVICE.
#include "capi.hpp"

#include <cstring>
#include <map>
#include <vector>

namespace dsq {

// counts -> int32 gene-major.  Returns the pointer to use and its ld.
int prep_counts(const void *y, int y_type, int layout, long ld_in, int n, int m, hipStream_t st,
                       const int32_t **out, long *ld_out, bool *checked_async) {
    *checked_async = false;
    if (layout == DSQ_LAYOUT_GENE_MAJOR) {
        if (y_type != DSQ_Y_INT32)
            return capi_fail(DSQ_ERR_UNSUPPORTED, "gene-major counts must be int32 (y_type = DSQ_Y_INT32)");
        *out = (const int32_t *)y;
        *ld_out = ld_in;
        return DSQ_OK;
    }
    long ld = round_ld(m);
    void *buf;
    int rc = capi_ws_get(WS_Y, (size_t)n * ld * sizeof(int32_t), &buf);
    if (rc) return rc;
    if (y_type == DSQ_Y_INT32) {
        DSQ_HIP(launch_transpose_r_to_gm_i32((const int32_t *)y, (int32_t *)buf, n, m, ld, st));
    } else if (y_type == DSQ_Y_FLOAT64) {
        void *bad;
        rc = capi_ws_get(WS_BAD, sizeof(int32_t), &bad);
        if (rc) return rc;
        DSQ_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
        DSQ_HIP(launch_counts_f64_to_gm_i32((const double *)y, (int32_t *)buf, n, m, ld, (int32_t *)bad, st));
        *checked_async = true;
    } else {
        return capi_fail(DSQ_ERR_ARG, "unknown y_type %d", y_type);
    }
    *out = (const int32_t *)buf;
    *ld_out = ld;
    return DSQ_OK;
}

int prep_matrix(const double *src, int layout, long ld_in, int n, int m, int slot, hipStream_t st,
                       const double **out, long ld_expected) {
    if (layout == DSQ_LAYOUT_GENE_MAJOR) {
        (void)ld_in;
        *out = src;
        return DSQ_OK;
    }
    void *buf;
    int rc = capi_ws_get(slot, (size_t)n * ld_expected * sizeof(double), &buf);
    if (rc) return rc;
    DSQ_HIP(launch_transpose_r_to_gm_f64(src, (double *)buf, n, m, ld_expected, st));
    *out = (const double *)buf;
    return DSQ_OK;
}

// zeroed counters for the dynamic gene scheduling of the persistent fit kernels (dsq_wave.hpp next_gene)
static int work_counter(hipStream_t st, int **out) {
    *out = nullptr;
    if (!tuning().dynamic) return DSQ_OK;
    void *v;
    int rc = capi_ws_get(WS_COUNTER, 4 * sizeof(int), &v);
    if (rc) return rc;
    DSQ_HIP(hipMemsetAsync(v, 0, 4 * sizeof(int), st));
    *out = (int *)v;
    return DSQ_OK;
}

template <int P>
struct DispatchP {
    static hipError_t beta(int p, const BetaKernelParams &kp, hipStream_t st, bool *ok) {
        if (p == P) { *ok = true; return launch_fit_beta_p<P>(kp, st); }
        return DispatchP<P - 1>::beta(p, kp, st, ok);
    }
    static void beta_scratch(int p, int n, int m, int useW, size_t *slab, size_t *cscr) {
        if (p == P) { fit_beta_scratch_doubles<P>(n, m, useW, slab, cscr); return; }
        DispatchP<P - 1>::beta_scratch(p, n, m, useW, slab, cscr);
    }
    static hipError_t disp(int p, const DispKernelParams &kp, hipStream_t st, bool grid, bool *ok) {
        if (p == P) { *ok = true; return launch_fit_disp_p<P>(kp, st, grid); }
        return DispatchP<P - 1>::disp(p, kp, st, grid, ok);
    }
    static hipError_t optim(int p, const OptimKernelParams &kp, hipStream_t st, bool *ok) {
        if (p == P) { *ok = true; return launch_optim_p<P>(kp, st); }
        return DispatchP<P - 1>::optim(p, kp, st, ok);
    }
};
template <>
struct DispatchP<0> {
    static hipError_t beta(int, const BetaKernelParams &, hipStream_t, bool *ok) { *ok = false; return hipSuccess; }
    static void beta_scratch(int, int, int, int, size_t *slab, size_t *cscr) { *slab = 0; *cscr = 0; }
    static hipError_t disp(int, const DispKernelParams &, hipStream_t, bool, bool *ok) { *ok = false; return hipSuccess; }
    static hipError_t optim(int, const OptimKernelParams &, hipStream_t, bool *ok) { *ok = false; return hipSuccess; }
};

// (wide designs: the caller passes the PADDED width, one of DSQ_WIDE_LIST -- the chain of pipeline.hip, dsq_optim_rows)
hipError_t dispatch_fit_beta(int p, const BetaKernelParams &kp, hipStream_t st, bool *ok) {
#define DSQ_X(W) if (p == W) { *ok = true; return launch_fit_beta_p<W>(kp, st); }
    DSQ_WIDE_LIST(DSQ_X)
#undef DSQ_X
    return DispatchP<DSQ_P_REG>::beta(p, kp, st, ok);
}
void dispatch_beta_scratch(int p, int n, int m, int useW, size_t *slab, size_t *cscr) {
#define DSQ_X(W) if (p == W) { fit_beta_scratch_doubles<W>(n, m, useW, slab, cscr); return; }
    DSQ_WIDE_LIST(DSQ_X)
#undef DSQ_X
    DispatchP<DSQ_P_REG>::beta_scratch(p, n, m, useW, slab, cscr);
}
hipError_t dispatch_fit_disp(int p, const DispKernelParams &kp, hipStream_t st, bool grid, bool *ok) {
    // (beyond DSQ_DISP_PERWIDTH_MAX columns the rolled kernel of fit_disp_wide.hip is the only one: what it does not take --
    //  rows of more than 1024 samples, a working set beyond the LDS -- is refused)
    if (p > DSQ_DISP_PERWIDTH_MAX && !fit_disp_rolled_applies(kp, nullptr)) { *ok = false; return hipSuccess; }
#define DSQ_X(W) if (p == W) { *ok = true; return launch_fit_disp_p<W>(kp, st, grid); }
    DSQ_WIDE_LIST(DSQ_X)
#undef DSQ_X
    return DispatchP<DSQ_P_REG>::disp(p, kp, st, grid, ok);
}
hipError_t dispatch_optim_rows(int p, const OptimKernelParams &kp, hipStream_t st, bool *ok) {
    // (wide designs: the caller passes the padded width, dsq_optim_rows)
#define DSQ_X(W) if (p == W) { *ok = true; return launch_optim_p<W>(kp, st); }
    DSQ_WIDE_LIST(DSQ_X)
#undef DSQ_X
    return DispatchP<DSQ_P_REG>::optim(p, kp, st, ok);
}

// ---- wide designs (DSQ_P_REG < p <= DSQ_P_WIDE): zero-padded to DSQ_P_WIDE columns --------------------------
// A padded coefficient has an all-zero design column, ridge 1 and start value 0: its estimate is exactly 0 and the
// Gram / QR / LU arithmetic of the real coefficients sees only extra exact zeros (x + 0 = x, 0 * y = 0), so their
// results keep their bits (tests/test_gpu_wide.py compares with the oracle run at the true p).

int capi_pad_design(int slot, const double *src, size_t rows, int p, int pw, hipStream_t st, const double **out) {
    // column-major rows x p  ->  rows x pw in the slot, new columns zero
    void *b;
    int rc = capi_ws_get(slot, rows * (size_t)pw * sizeof(double), &b);
    if (rc) return rc;
    DSQ_HIP(hipMemsetAsync(b, 0, rows * (size_t)pw * sizeof(double), st));
    DSQ_HIP(hipMemcpyAsync(b, src, rows * (size_t)p * sizeof(double), hipMemcpyDeviceToDevice, st));
    *out = (const double *)b;
    return DSQ_OK;
}

// design cells -> device arrays for the cell-collapsed fitBeta kernel: cells renumbered in order of first appearance,
// samples grouped by cell (ascending inside a cell).  labels: m host ints (any numbering).  Returns the number of
// cells (0: more than DSQ_CMAX, or cells switched off) and the device pointers.
int capi_upload_cells(const int32_t *labels, int m, int slot, hipStream_t st, const int32_t **perm_dev,
                      const int32_t **start_dev) {
    *perm_dev = *start_dev = nullptr;
    if (!labels || !tuning().beta_cells) return 0;
    if (m >= (1 << 26)) return 0;      // the kernels pack (sample | cell << 26) into one int32
    static thread_local std::vector<int32_t> buf;
    std::map<int32_t, int> id;
    std::vector<int> cell(m);
    int C = 0;
    for (int j = 0; j < m; j++) {
        auto it = id.find(labels[j]);
        if (it == id.end()) {
            if (C == DSQ_CMAX) return 0;
            it = id.emplace(labels[j], C++).first;
        }
        cell[j] = it->second;
    }
    buf.assign((size_t)m + C + 1, 0);
    int32_t *start = buf.data(), *perm = buf.data() + C + 1;
    for (int j = 0; j < m; j++) start[cell[j] + 1]++;
    for (int c = 0; c < C; c++) start[c + 1] += start[c];
    std::vector<int> fill(start, start + C);
    for (int j = 0; j < m; j++) perm[fill[cell[j]]++] = j;
    void *v;
    if (capi_upload_table(slot, buf.data(), buf.size() * sizeof(int32_t), st, &v)) return 0;
    *start_dev = (const int32_t *)v;
    *perm_dev = (const int32_t *)v + C + 1;
    return C;
}

// =============================================================== each call's checks, stated once
// check_<call>(args, out): everything that can be decided from the argument block alone.  Both halves of the ABI call it
// first; a host entry adds only what is its own (R layout, the row range).  One skeleton: the call's own conditions, sizes,
// NULL pointers, weights, ld / layout -- all DSQ_ERR_ARG -- and, when nothing else is wrong, a design wider than the
// kernels (DSQ_ERR_UNSUPPORTED; p = 0: the call has no such limit of its own).
#define DSQ_NEED(cond, what) do { if (!(cond)) return capi_fail(DSQ_ERR_ARG, what); } while (0)
static int too_wide(int p) {
    return capi_fail(DSQ_ERR_UNSUPPORTED, "p=%d design columns: kernels are compiled for 1..%d", p, DSQ_P_WIDE);
}
static int check_layout(int layout, long ld, int m, bool known_only) {
    if (layout == DSQ_LAYOUT_GENE_MAJOR && ld < m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", ld, m);
    if (known_only && layout != DSQ_LAYOUT_R && layout != DSQ_LAYOUT_GENE_MAJOR) return capi_fail(DSQ_ERR_ARG, "unknown layout %d", layout);
    return DSQ_OK;
}
template <class A>
static int check_block(const A *a, bool dims_ok, int p, bool inputs, const double *weights, int useWeights, bool outputs,
                       bool known_layout_only) {
    if (a->n < 0 || a->m < 1 || !dims_ok) return capi_fail(DSQ_ERR_ARG, "bad dimensions n=%d m=%d p=%d", a->n, a->m, p);
    DSQ_NEED(inputs, "NULL input array");
    DSQ_NEED(!useWeights || weights, "useWeights set but weights is NULL");
    DSQ_NEED(outputs, "NULL output array");
    if (int rc = check_layout(a->layout, a->ld, a->m, known_layout_only)) return rc;
    return p > DSQ_P_WIDE ? too_wide(p) : DSQ_OK;
}

int check_host_layout(int layout) {
    DSQ_NEED(layout == DSQ_LAYOUT_R, "host entry points take R layout only");
    return DSQ_OK;
}
int check_fit_beta(const DsqFitBetaArgs *a, const DsqFitBetaOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    DSQ_NEED(a->maxit >= 0, "maxit < 0");
    return check_block(a, a->p >= 1, a->p, a->y && a->x && a->nf && a->alpha_hat && a->contrast && a->beta_mat && a->lambda,
                       a->weights, a->useWeights,
                       o->beta_mat && o->beta_var_mat && o->iter && o->contrast_num && o->contrast_denom && o->deviance, true);
}
int check_fit_disp(const DsqFitDispArgs *a, const DsqFitDispOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    DSQ_NEED(a->maxit >= 0, "maxit < 0");
    return check_block(a, a->p >= 1, a->p, a->y && a->x && a->mu_hat && a->log_alpha && a->log_alpha_prior_mean, a->weights,
                       a->useWeights,          // (last_d2lp may be NULL in the device entry: its kernel is then skipped)
                       o->log_alpha && o->iter && o->iter_accept && o->last_change && o->initial_lp && o->initial_dlp &&
                           o->last_lp && o->last_dlp, true);
}
int check_fit_disp_grid(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    DSQ_NEED(a->ngrid >= 2, "disp_grid needs at least 2 points");
    return check_block(a, a->p >= 1, a->p, a->y && a->x && a->mu_hat && a->disp_grid && a->log_alpha_prior_mean, a->weights,
                       a->useWeights, o->log_alpha != nullptr, true);
}
int check_trend_fit(const double *means, const double *disps, int64_t n, const double *coefs, const int32_t *status) {
    DSQ_NEED(means && disps && coefs && status && n >= 1, "bad arguments");
    return DSQ_OK;
}
int check_prefit(const DsqPrefitArgs *a, const DsqPrefitOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    return check_block(a, a->m >= 2 && a->p >= 1 && a->m > a->p, 0, a->y && a->nf && a->q && a->a && a->r, a->weights, a->useWeights,
                       o->baseMean && o->baseVar && o->allZero && o->roughDisp && o->beta_init, false);
}
int check_linear_mu(const DsqPrefitArgs *a, const double *mu) {
    DSQ_NEED(a && mu, "NULL args/out");
    return check_block(a, a->p >= 1, 0, a->y && a->nf && a->q && a->a, nullptr, 0, true, false);
}
int check_loglike(const DsqLogLikeArgs *a, const double *out) {
    DSQ_NEED(a && out, "NULL args/out");
    return check_block(a, true, 0, a->y && a->mu && a->disp, a->weights, a->useWeights, true, false);
}
int check_intercept(const DsqInterceptArgs *a, const DsqInterceptOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    return check_block(a, true, 0, a->y && a->nf && a->alpha, a->weights, a->useWeights, o->beta_log2 && o->betaSE, false);
}
int check_optim(const DsqOptimArgs *a, const DsqOptimOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    return check_block(a, a->p >= 1, a->p, a->y && a->x && a->nf && a->alpha_hat && a->lambda && a->beta_start, a->weights,
                       a->useWeights, o->beta && o->betaSE && o->conv && o->mu && o->logLike, false);
}
int check_cooks(const DsqCooksArgs *a, const DsqCooksOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    if (int rc = check_block(a, a->p >= 1 && a->ncell >= 1, 0, a->y && a->nf && a->mu && a->H && a->cell_of, nullptr, 0,
                             o->cooks && o->maxCooks, false)) return rc;
    for (int j = 0; j < a->m; j++)          // (cell_of is a host array in both halves)
        if (a->cell_of[j] < 0 || a->cell_of[j] >= a->ncell) return capi_fail(DSQ_ERR_VALUE, "cell_of[%d] out of range", j);
    return DSQ_OK;
}
int check_replace(const DsqReplaceArgs *a, const DsqReplaceOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    DSQ_NEED(a->trim >= 0.0 && a->trim < 0.5, "trim must be in [0, 0.5)");
    return check_block(a, true, 0, a->y && a->nf && a->cooks && a->replaceable, nullptr, 0, o->newCounts && o->replace, false);
}
// a body's opening after its check: the device; *empty: the call has no genes and returns DSQ_OK
static int dev_ready(int check_rc, int n, bool *empty) {
    *empty = n == 0;
    return check_rc ? check_rc : capi_check_device();
}

// =============================================================== the n x m arrays of a call, into and out of gene-major
// Inputs: the counts first (they fix ld), then each matrix into its slot (prep_matrix: as it is when gene-major).
struct GmIn {
    int layout, n, m;
    long ld_in;
    hipStream_t st;
    long ld = 0;
    bool ycheck = false;        // float64 counts: their validity flag is read back by finish_ycheck
    GmIn(int layout_, int n_, int m_, long ld_, hipStream_t st_) : layout(layout_), n(n_), m(m_), ld_in(ld_), st(st_) {}
    template <class A>
    GmIn(const A *a, hipStream_t st_) : GmIn(a->layout, a->n, a->m, a->ld, st_) {}
    int counts(const void *y, int y_type, const int32_t **out, long *ld_out) {
        int rc = prep_counts(y, y_type, layout, ld_in, n, m, st, out, &ld, &ycheck);
        *ld_out = ld;
        return rc;
    }
    int matrix(const double *src, int slot, const double **out) const { return prep_matrix(src, layout, ld_in, n, m, slot, st, out, ld); }
    // size factors (m of them, used as they are) or an n x m matrix of normalization factors
    int nf(const double *src, int is_vector, const double **out, int *flag) const {
        *flag = is_vector ? 1 : 0;
        if (is_vector) { *out = src; return DSQ_OK; }
        return matrix(src, WS_NF, out);
    }
    int weights(const double *src, int use, const double **out, int *flag) const {
        *flag = use ? 1 : 0;
        return use ? matrix(src, WS_W, out) : DSQ_OK;
    }
    bool gene_major() const { return layout == DSQ_LAYOUT_GENE_MAJOR; }
};

static hipError_t transpose_back(const double *gm, double *r, int n, int m, long ld, hipStream_t st) {
    return launch_transpose_gm_to_r_f64(gm, r, n, m, ld, st);
}
static hipError_t transpose_back(const int32_t *gm, int32_t *r, int n, int m, long ld, hipStream_t st) {
    return launch_transpose_gm_to_r_i32(gm, r, n, m, ld, st);
}

// An n x m output: the kernel writes the caller's buffer when that is gene-major, else a workspace slot that finish()
// transposes back into it after the launch.  A NULL buffer (an output not asked for) stays NULL.
template <class T>
struct GmOut {
    T *user = nullptr, *ws = nullptr;
    int bind(const GmIn &g, T *dst, int slot, T **kernel_ptr) {
        user = dst;
        *kernel_ptr = dst;
        if (!dst || g.gene_major()) return DSQ_OK;
        void *b;
        if (int rc = capi_ws_get(slot, (size_t)g.n * g.ld * sizeof(T), &b)) return rc;
        *kernel_ptr = ws = (T *)b;
        return DSQ_OK;
    }
    int finish(const GmIn &g) {
        if (ws) DSQ_HIP(transpose_back(ws, user, g.n, g.m, g.ld, g.st));
        return DSQ_OK;
    }
};

int finish_ycheck(bool ycheck, hipStream_t st) {
    if (!ycheck) return DSQ_OK;
    int32_t bad = 0;
    void *badp;
    int rc = capi_ws_get(WS_BAD, sizeof(int32_t), &badp);
    if (rc) return rc;
    DSQ_HIP(hipMemcpyAsync(&bad, badp, sizeof bad, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    if (bad) return capi_fail(DSQ_ERR_VALUE, "count matrix holds negative, non-finite or non-integer values");
    return DSQ_OK;
}

// =============================================================== fitBeta (device)
int fit_beta_dev_locked(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_fit_beta(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;

    BetaKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = a->p;
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    if ((rc = in.weights(a->weights, a->useWeights, &kp.weights, &kp.useWeights))) return rc;
    kp.x = a->x; kp.alpha_hat = a->alpha_hat; kp.contrast = a->contrast; kp.beta_init = a->beta_mat;
    kp.lambda = a->lambda;
    kp.tol = a->tol; kp.minmu = a->minmu; kp.mu_floor = o->mu_floor;
    kp.maxit = a->maxit; kp.useQR = a->useQR ? 1 : 0;
    kp.ablate = tuning().ablate; kp.force_iters = tuning().force_iters;
    rc = work_counter(st, &kp.work_counter); if (rc) return rc;
    if (a->cell_of && a->ncell > 0)
        kp.ncell = capi_upload_cells(a->cell_of, a->m, WS_CELLS_BETA, st, &kp.cell_perm, &kp.cell_start);
    kp.beta_mat = o->beta_mat; kp.beta_var_mat = o->beta_var_mat; kp.iter = o->iter;
    kp.contrast_num = o->contrast_num; kp.contrast_denom = o->contrast_denom; kp.deviance = o->deviance;
    const bool wide = is_wide(a->p);
    const int pk = wide ? wide_width(a->p) : a->p;       // the kernel's design width
    double *wide_out = nullptr;
    if (wide) {
        rc = capi_pad_design(WS_PAD_X, a->x, (size_t)a->m, a->p, pk, st, &kp.x); if (rc) return rc;
        static thread_local double ones[DSQ_P_WIDE];
        for (int c = 0; c < DSQ_P_WIDE; c++) ones[c] = 1.0;
        void *v;
        rc = capi_ws_get(WS_PAD_VEC, 2 * DSQ_P_WIDE * sizeof(double), &v); if (rc) return rc;
        double *vec = (double *)v;
        DSQ_HIP(hipMemcpyAsync(vec, ones, sizeof ones, hipMemcpyHostToDevice, st));                 // ridge 1 on padding
        DSQ_HIP(hipMemcpyAsync(vec, a->lambda, a->p * sizeof(double), hipMemcpyDeviceToDevice, st));
        DSQ_HIP(hipMemsetAsync(vec + DSQ_P_WIDE, 0, DSQ_P_WIDE * sizeof(double), st));
        DSQ_HIP(hipMemcpyAsync(vec + DSQ_P_WIDE, a->contrast, a->p * sizeof(double), hipMemcpyDeviceToDevice, st));
        kp.lambda = vec; kp.contrast = vec + DSQ_P_WIDE;
        const size_t npw = (size_t)a->n * pk;
        rc = capi_ws_get(WS_PAD_BETA, 3 * npw * sizeof(double), &v); if (rc) return rc;
        double *bb = (double *)v;
        DSQ_HIP(hipMemsetAsync(bb, 0, npw * sizeof(double), st));
        DSQ_HIP(hipMemcpyAsync(bb, a->beta_mat, (size_t)a->n * a->p * sizeof(double), hipMemcpyDeviceToDevice, st));
        kp.beta_init = bb; kp.beta_mat = bb + npw; kp.beta_var_mat = bb + 2 * npw;
        kp.p_true = a->p;
        wide_out = bb + npw;
        kp.p = pk;
    }
    GmOut<double> hat, mu;
    if ((rc = hat.bind(in, o->hat_diagonals, WS_HAT, &kp.hat_diagonals))) return rc;
    if ((rc = mu.bind(in, o->mu, WS_MUOUT, &kp.mu_out))) return rc;
    size_t slab_d = 0, cscr_d = 0;
    dispatch_beta_scratch(pk, a->n, a->m, a->useWeights, &slab_d, &cscr_d);
    {
        void *b; rc = capi_ws_get(WS_SCRATCH, (slab_d + cscr_d) * sizeof(double) + 64, &b); if (rc) return rc;
        kp.scratch = (double *)b;
        kp.cscratch = (double *)b + slab_d;
    }
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(dispatch_fit_beta(pk, kp, st, &ok));
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "no kernel for p=%d", a->p);
    if (wide) {     // the real coefficients are the leading columns of the padded n x 16 results
        const size_t npw = (size_t)a->n * pk, npp = (size_t)a->n * a->p * sizeof(double);
        DSQ_HIP(hipMemcpyAsync(o->beta_mat, wide_out, npp, hipMemcpyDeviceToDevice, st));
        DSQ_HIP(hipMemcpyAsync(o->beta_var_mat, wide_out + npw, npp, hipMemcpyDeviceToDevice, st));
    }
    if ((rc = hat.finish(in))) return rc;
    if ((rc = mu.finish(in))) return rc;
    return finish_ycheck(in.ycheck, st);
}

// =============================================================== fitDisp (device)
// the part of the kernel parameters fitDisp and fitDispGrid share (the caller has run its check and found n > 0)
static int disp_common(int n, int m, int p, int layout, long ld_in, const void *y, int y_type, const double *x,
                       const double *mu_hat, const double *weights, int useWeights, hipStream_t st,
                       DispKernelParams *kp, bool *ycheck, const int32_t *cell_of, int ncell) {
    memset(kp, 0, sizeof *kp);
    kp->n = n; kp->m = m; kp->p = p;
    GmIn in(layout, n, m, ld_in, st);
    int rc = in.counts(y, y_type, &kp->y, &kp->ld);
    *ycheck = in.ycheck;
    if (rc) return rc;
    if ((rc = in.matrix(mu_hat, WS_MU, &kp->mu_hat))) return rc;
    if ((rc = in.weights(weights, useWeights, &kp->weights, &kp->useWeights))) return rc;
    kp->x = x;
    if (cell_of && ncell > 0 && p >= tuning().disp_cell_minp)
        kp->ncell = capi_upload_cells(cell_of, m, WS_CELLS_BETA, st, &kp->cell_perm, &kp->cell_start);
    if (is_wide(p)) {           // zero-padded design, unit diagonal on the padding in the Cox-Reid matrix
        kp->p = wide_width(p);
        rc = capi_pad_design(WS_PAD_X, x, (size_t)m, p, kp->p, st, &kp->x);
        if (rc) return rc;
        kp->padmask = dsq_low_bits(kp->p) & ~dsq_low_bits(p);
    }
    return DSQ_OK;
}

int fit_disp_dev_locked(const DsqFitDispArgs *a, const DsqFitDispOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_fit_disp(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    DispKernelParams kp;
    bool ycheck = false;
    rc = disp_common(a->n, a->m, a->p, a->layout, a->ld, a->y, a->y_type, a->x, a->mu_hat, a->weights,
                     a->useWeights, st, &kp, &ycheck, a->cell_of, a->ncell);
    if (rc) return rc;
    kp.log_alpha_in = a->log_alpha; kp.prior_mean = a->log_alpha_prior_mean;
    kp.prior_sigmasq = a->log_alpha_prior_sigmasq; kp.min_log_alpha = a->min_log_alpha;
    kp.kappa_0 = a->kappa_0; kp.tol = a->tol; kp.weightThreshold = a->weightThreshold;
    kp.maxit = a->maxit; kp.usePrior = a->usePrior ? 1 : 0; kp.useCR = a->useCR ? 1 : 0;
    kp.ablate = tuning().ablate; kp.force_iters = tuning().force_iters;
    rc = work_counter(st, &kp.work_counter); if (rc) return rc;
    kp.log_alpha = o->log_alpha; kp.iter = o->iter; kp.iter_accept = o->iter_accept;
    kp.last_change = o->last_change; kp.initial_lp = o->initial_lp; kp.initial_dlp = o->initial_dlp;
    kp.last_lp = o->last_lp; kp.last_dlp = o->last_dlp; kp.last_d2lp = o->last_d2lp;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(dispatch_fit_disp(kp.p, kp, st, false, &ok));       // (kp.p: the padded width for a wide design)
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "no kernel for p=%d, m=%d (49..%d columns: rows of at most 1024 samples whose working set fits the LDS)", a->p, a->m, DSQ_P_WIDE);
    return finish_ycheck(ycheck, st);
}

int fit_disp_grid_dev_locked(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_fit_disp_grid(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    DispKernelParams kp;
    bool ycheck = false;
    rc = disp_common(a->n, a->m, a->p, a->layout, a->ld, a->y, a->y_type, a->x, a->mu_hat, a->weights,
                     a->useWeights, st, &kp, &ycheck, a->cell_of, a->ncell);
    if (rc) return rc;
    kp.prior_mean = a->log_alpha_prior_mean; kp.prior_sigmasq = a->log_alpha_prior_sigmasq;
    kp.weightThreshold = a->weightThreshold;
    kp.usePrior = a->usePrior ? 1 : 0; kp.useCR = a->useCR ? 1 : 0;
    kp.grid = a->disp_grid; kp.ngrid = a->ngrid; kp.log_alpha = o->log_alpha;
    rc = work_counter(st, &kp.work_counter); if (rc) return rc;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(dispatch_fit_disp(kp.p, kp, st, true, &ok));       // (kp.p: the padded width for a wide design)
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "no kernel for p=%d", a->p);
    return finish_ycheck(ycheck, st);
}

// =============================================================== extensions (device)
int prefit_dev_locked(const DsqPrefitArgs *a, const DsqPrefitOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_prefit(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    PrefitKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = a->p;
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    if ((rc = in.weights(a->weights, a->useWeights, &kp.weights, &kp.useWeights))) return rc;
    kp.q = a->q; kp.a = a->a; kp.r = a->r;
    kp.baseMean = o->baseMean; kp.baseVar = o->baseVar; kp.allZero = o->allZero; kp.roughDisp = o->roughDisp;
    kp.beta_init = o->beta_init;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(launch_prefit(kp, st, &ok));
    prof_end(st);
    if (!ok) return too_wide(a->p);
    return finish_ycheck(in.ycheck, st);
}

int linear_mu_dev_locked(const DsqPrefitArgs *a, double mu_floor, double *mu, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_linear_mu(a, mu), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    PrefitKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = a->p;
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    kp.q = a->q; kp.a = a->a;
    GmOut<double> out;
    double *dst;
    if ((rc = out.bind(in, mu, WS_MUOUT, &dst))) return rc;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(launch_linear_mu(kp, mu_floor, dst, st, &ok));
    prof_end(st);
    if (!ok) return too_wide(a->p);
    if ((rc = out.finish(in))) return rc;
    return finish_ycheck(in.ycheck, st);
}

int loglike_dev_locked(const DsqLogLikeArgs *a, double *out, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_loglike(a, out), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    LogLikeKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m;
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.matrix(a->mu, WS_MU, &kp.mu))) return rc;
    if ((rc = in.weights(a->weights, a->useWeights, &kp.weights, &kp.useWeights))) return rc;
    kp.disp = a->disp; kp.loglike = out;
    prof_begin(st);
    DSQ_HIP(launch_loglike(kp, st));
    prof_end(st);
    return finish_ycheck(in.ycheck, st);
}

int intercept_dev_locked(const DsqInterceptArgs *a, const DsqInterceptOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_intercept(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    InterceptKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m;
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    if ((rc = in.weights(a->weights, a->useWeights, &kp.weights, &kp.useWeights))) return rc;
    kp.alpha = a->alpha; kp.mu_floor = a->mu_floor;
    kp.beta_log2 = o->beta_log2; kp.betaSE = o->betaSE;
    GmOut<double> mu, hat;
    if ((rc = mu.bind(in, o->mu, WS_MUOUT, &kp.mu_out))) return rc;
    if ((rc = hat.bind(in, o->hat, WS_HAT, &kp.hat))) return rc;
    prof_begin(st);
    DSQ_HIP(launch_intercept_fit(kp, st));
    prof_end(st);
    if ((rc = mu.finish(in))) return rc;
    if ((rc = hat.finish(in))) return rc;
    return finish_ycheck(in.ycheck, st);
}

// =============================================================== Cook's distances / replaceOutliers
static int next_pow2(int n) { int v = 2; while (v < n) v <<= 1; return v; }

int cooks_dev_locked(const DsqCooksArgs *a, const DsqCooksOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_cooks(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    const int m = a->m;
    // design cells -> sample permutation grouped by cell, offsets, ">= 3 in cell" flags
    static thread_local std::vector<int32_t> meta;
    meta.assign((size_t)2 * m + a->ncell + 1, 0);
    int32_t *perm = meta.data(), *in3 = perm + m, *start = in3 + m;
    for (int j = 0; j < m; j++) start[a->cell_of[j] + 1]++;
    int maxcell = 0, any3 = 0;
    for (int c = 0; c < a->ncell; c++) {
        int sz = start[c + 1];
        if (sz > maxcell) maxcell = sz;
        if (sz >= 3) any3 = 1;
        start[c + 1] += start[c];
    }
    {
        std::vector<int32_t> fill(start, start + a->ncell);
        for (int j = 0; j < m; j++) perm[fill[a->cell_of[j]]++] = j;
    }
    for (int j = 0; j < m; j++) in3[j] = (start[a->cell_of[j] + 1] - start[a->cell_of[j]]) >= 3;
    CooksKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = m; kp.p = a->p; kp.ncell = a->ncell; kp.any3 = any3;
    kp.sortcap = next_pow2(any3 ? maxcell : m);
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    if ((rc = in.matrix(a->mu, WS_MU, &kp.mu))) return rc;
    if ((rc = in.matrix(a->H, WS_W, &kp.H))) return rc;
    // the slot: the table, then n doubles for robustDisp when the caller wants none.  The table goes through the pinned
    // ring (capi_upload_table): `meta` is rewritten by the next call on this thread, maybe before this copy has run
    void *v;
    rc = capi_ws_get(WS_CELLS, meta.size() * sizeof(int32_t) + (size_t)a->n * 8, &v); if (rc) return rc;
    rc = capi_upload_table(WS_CELLS, meta.data(), meta.size() * sizeof(int32_t), st, &v); if (rc) return rc;
    kp.perm = (int32_t *)v; kp.in3 = kp.perm + m; kp.cell_start = kp.in3 + m;
    kp.maxCooks = o->maxCooks;
    if (o->robustDisp) kp.robustDisp = o->robustDisp;
    else kp.robustDisp = (double *)((char *)v + ((meta.size() * sizeof(int32_t) + 7) & ~(size_t)7));
    GmOut<double> cooks;
    if ((rc = cooks.bind(in, o->cooks, WS_HAT, &kp.cooks))) return rc;
    bool ok = true;
    prof_begin(st);
    DSQ_HIP(launch_cooks(kp, st, &ok));
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "m=%d samples: a gene row plus its sort buffer exceeds the 160 KiB LDS", m);
    if ((rc = cooks.finish(in))) return rc;
    return finish_ycheck(in.ycheck, st);
}

int replace_dev_locked(const DsqReplaceArgs *a, const DsqReplaceOut *o, hipStream_t st) {
    bool empty;
    int rc = dev_ready(check_replace(a, o), a ? a->n : 0, &empty);
    if (rc || empty) return rc;
    const int m = a->m;
    ReplaceKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = m; kp.cutoff = a->cooksCutoff; kp.trim = a->trim; kp.sortcap = next_pow2(m);
    GmIn in(a, st);
    if ((rc = in.counts(a->y, a->y_type, &kp.y, &kp.ld))) return rc;
    if ((rc = in.nf(a->nf, a->nf_is_vector, &kp.nf, &kp.nf_is_vector))) return rc;
    if ((rc = in.matrix(a->cooks, WS_COOKS_IN, &kp.cooks))) return rc;
    static thread_local std::vector<int32_t> flags;
    flags.assign(a->replaceable, a->replaceable + m);
    void *v;            // (through the pinned ring, as the cells of cooks_dev_locked: `flags` is the next call's too)
    rc = capi_upload_table(WS_CELLS, flags.data(), (size_t)m * sizeof(int32_t), st, &v); if (rc) return rc;
    kp.replaceable = (int32_t *)v;
    kp.replace = o->replace;
    GmOut<int32_t> counts;
    if ((rc = counts.bind(in, o->newCounts, WS_HAT, &kp.newCounts))) return rc;
    bool ok = true;
    prof_begin(st);
    DSQ_HIP(launch_replace(kp, st, &ok));
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "m=%d samples: the sort buffer exceeds the 160 KiB LDS", m);
    if ((rc = counts.finish(in))) return rc;
    return finish_ycheck(in.ycheck, st);
}

int size_factors_check(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !o->sizeFactors || !o->status) return capi_fail(DSQ_ERR_ARG, "NULL counts, sizeFactors or status");
    if (a->y_type != DSQ_Y_INT32 && a->y_type != DSQ_Y_FLOAT64) return capi_fail(DSQ_ERR_ARG, "unknown y_type %d", a->y_type);
    if (a->type != DSQ_SF_RATIO && a->type != DSQ_SF_POSCOUNTS)
        return capi_fail(DSQ_ERR_ARG, "type %d: DSQ_SF_RATIO or DSQ_SF_POSCOUNTS (\"iterate\" is not served)", a->type);
    if ((a->normMatrix != nullptr) != (o->normalizationFactors != nullptr))
        return capi_fail(DSQ_ERR_ARG, "normalizationFactors is required if and only if normMatrix is given");
    return DSQ_OK;
}

int size_factors_dev_locked(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o, hipStream_t st) {
    if (int rc = size_factors_check(a, o)) return rc;
    if (int rc = check_layout(a->layout, a->ld, a->m, true)) return rc;
    const size_t need = size_factors_workspace_bytes(a->n, a->m);
    if (!a->workspace || a->workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: dsq_size_factors_workspace_bytes(n, m) = %zu", (long long)a->workspace_bytes, need);
    if (int rc = capi_check_device()) return rc;
    SizeFactorKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m;
    kp.y = a->y;
    const bool gm = a->layout == DSQ_LAYOUT_GENE_MAJOR;
    kp.y_si = gm ? (long)a->ld : 1L;  kp.y_sj = gm ? 1L : (long)a->n;
    kp.nm = a->normMatrix; kp.nm_si = kp.y_si; kp.nm_sj = kp.y_sj;
    kp.type = a->type;
    kp.geoMeans = a->type == DSQ_SF_POSCOUNTS ? nullptr : a->geoMeans;
    kp.stabilize = a->type == DSQ_SF_POSCOUNTS || a->geoMeans != nullptr;
    kp.control = a->control;
    kp.sf = o->sizeFactors; kp.lgm_out = o->loggeomeans; kp.nf_out = o->normalizationFactors; kp.status = o->status;
    capi_prof_begin("size_factors", a->n, st);
    DSQ_HIP(launch_size_factors(kp, a->y_type == DSQ_Y_FLOAT64, a->workspace, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// the variance stabilizing transformation (vst.hip): what both entries check before anything is launched
int vst_check(const DsqVstArgs *a, const DsqVstOut *o, bool transform, bool stats) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf) return capi_fail(DSQ_ERR_ARG, "NULL counts or size / normalization factors");
    if (a->y_type != DSQ_Y_INT32 && a->y_type != DSQ_Y_FLOAT64) return capi_fail(DSQ_ERR_ARG, "unknown y_type %d", a->y_type);
    if (stats && (!o->rowMean || !o->rowMax)) return capi_fail(DSQ_ERR_ARG, "NULL rowMean or rowMax");
    if (!transform) return DSQ_OK;
    if (!o->out) return capi_fail(DSQ_ERR_ARG, "NULL output matrix");
    const auto finite = [](double v) { return v - v == 0.0; };
    switch (a->kind) {
    case DSQ_VST_PARAMETRIC:
        if (!(a->asymptDisp > 0.0) || !finite(a->asymptDisp) || !finite(a->extraPois))
            return capi_fail(DSQ_ERR_ARG, "parametric: asymptDisp = %g must be positive, extraPois = %g finite", a->asymptDisp, a->extraPois);
        break;
    case DSQ_VST_MEAN:
        if (!(a->alpha > 0.0) || !finite(a->alpha)) return capi_fail(DSQ_ERR_ARG, "mean: alpha = %g must be positive", a->alpha);
        break;
    case DSQ_VST_SPLINE:
        if (!a->spline || a->nknots < 2) return capi_fail(DSQ_ERR_ARG, "spline: a table of at least two knots is needed");
        if (a->nknots > DSQ_VST_MAX_KNOTS)
            return capi_fail(DSQ_ERR_UNSUPPORTED, "spline: %d knots (at most %d: the table is held in LDS)", a->nknots, DSQ_VST_MAX_KNOTS);
        for (int k = 0; k + 1 < a->nknots; k++)
            if (!(a->spline[k] < a->spline[k + 1])) return capi_fail(DSQ_ERR_ARG, "spline: knots must be strictly ascending (knot %d)", k + 1);
        if (!finite(a->spline[0]) || !finite(a->spline[a->nknots - 1])) return capi_fail(DSQ_ERR_ARG, "spline: knots must be finite");
        break;
    case DSQ_VST_LOG2:
        if (a->pc != a->pc) return capi_fail(DSQ_ERR_ARG, "log2: the pseudocount is NaN");
        break;
    case DSQ_VST_NORMALIZED:
        break;
    default:
        return capi_fail(DSQ_ERR_ARG, "unknown kind %d", a->kind);
    }
    return DSQ_OK;
}

int vst_dev_locked(const DsqVstArgs *a, const DsqVstOut *o, bool transform, bool stats, hipStream_t st) {
    if (int rc = vst_check(a, o, transform, stats)) return rc;
    if (int rc = check_layout(a->layout, a->ld, a->m, true)) return rc;
    if (int rc = capi_check_device()) return rc;
    VstKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m;
    kp.y = a->y;
    const bool gm = a->layout == DSQ_LAYOUT_GENE_MAJOR;
    kp.si = gm ? (long)a->ld : 1L;  kp.sj = gm ? 1L : (long)a->n;
    kp.nf = a->nf; kp.nf_is_vector = a->nf_is_vector ? 1 : 0;
    kp.kind = a->kind;
    kp.a = a->asymptDisp; kp.e = a->extraPois; kp.alpha = a->alpha; kp.pc = a->pc;
    kp.nknots = a->nknots; kp.eta = a->eta; kp.xi = a->xi;
    kp.out = o->out; kp.rowMean = o->rowMean; kp.rowMax = o->rowMax;
    kp.bad = a->y_type == DSQ_Y_FLOAT64 ? o->bad : nullptr;
    if (transform && a->kind == DSQ_VST_SPLINE) {
        // the slot is sized for the largest table at once: a later, longer table never takes the grow path (which synchronises)
        void *tab;
        if (int rc = capi_ws_get(WS_VST_TABLE, (size_t)DSQ_VST_MAX_KNOTS * 5 * sizeof(double), &tab)) return rc;
        if (int rc = capi_upload_table(WS_VST_TABLE, a->spline, (size_t)a->nknots * 5 * sizeof(double), st, &tab)) return rc;
        kp.table = (const double *)tab;
    }
    if (stats) {
        capi_prof_begin("vst_rowstats", a->n, st);
        DSQ_HIP(launch_vst_rowstats(kp, a->y_type == DSQ_Y_FLOAT64, st));
        capi_prof_end(st);
    }
    if (transform) {
        capi_prof_begin("vst_transform", a->n, st);
        DSQ_HIP(launch_vst_transform(kp, a->y_type == DSQ_Y_FLOAT64, st));
        capi_prof_end(st);
    }
    return DSQ_OK;
}

// the rlog fit (rlog.hip): what both entries check before anything is launched
int rlog_check(const DsqRlogArgs *a, const DsqRlogOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->dispFit) return capi_fail(DSQ_ERR_ARG, "NULL counts, size / normalization factors or dispFit");
    if (a->y_type != DSQ_Y_INT32 && a->y_type != DSQ_Y_FLOAT64) return capi_fail(DSQ_ERR_ARG, "unknown y_type %d", a->y_type);
    if (!o->rlog || !o->iter || !o->flag) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (a->intercept && o->intercept) return capi_fail(DSQ_ERR_ARG, "an intercept is given: none is fitted");
    if (!(a->betaPriorVar > 0.0) || a->betaPriorVar - a->betaPriorVar != 0.0)
        return capi_fail(DSQ_ERR_ARG, "betaPriorVar = %g must be positive and finite", a->betaPriorVar);
    if (a->maxit < 0 || a->tol != a->tol || a->minmu != a->minmu) return capi_fail(DSQ_ERR_ARG, "bad tol / maxit / minmu");
    return DSQ_OK;
}

int rlog_dev_locked(const DsqRlogArgs *a, const DsqRlogOut *o, hipStream_t st) {
    if (int rc = rlog_check(a, o)) return rc;
    if (int rc = check_layout(a->layout, a->ld, a->m, true)) return rc;
    if (int rc = capi_check_device()) return rc;
    RlogKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m;
    kp.y = a->y;
    const bool gm = a->layout == DSQ_LAYOUT_GENE_MAJOR;
    kp.si = gm ? (long)a->ld : 1L;  kp.sj = gm ? 1L : (long)a->n;
    kp.nf = a->nf; kp.nf_is_vector = a->nf_is_vector ? 1 : 0;
    kp.dispFit = a->dispFit; kp.intercept = a->intercept;
    // lambdaNatLogScale <- lambda / log(2)^2 (R/fitNbinomGLMs.R:162), lambda = 1 / betaPriorVar, 1e-6 on the intercept (R/rlog.R:243-247)
    const double ln2 = 6.93147180559945286227e-01, ln2sq = ln2 * ln2;
    kp.lambda = (1.0 / a->betaPriorVar) / ln2sq; kp.lambda0 = 1e-6 / ln2sq;
    kp.tol = a->tol; kp.minmu = a->minmu; kp.maxit = a->maxit;
    kp.out = o->rlog; kp.intercept_out = o->intercept; kp.iter = o->iter; kp.flag = o->flag;
    kp.bad = a->y_type == DSQ_Y_FLOAT64 ? o->bad : nullptr;
    capi_prof_begin("rlog", a->n, st);
    DSQ_HIP(launch_rlog(kp, a->y_type == DSQ_Y_FLOAT64, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// apeglm shrinkage (apeglm.hip): what both entries check before anything is launched
int apeglm_check(const DsqApeglmArgs *a, const DsqApeglmOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->p > DSQ_APEGLM_MAX_P) return capi_fail(DSQ_ERR_UNSUPPORTED, "p = %d design columns: at most %d", a->p, DSQ_APEGLM_MAX_P);
    if (!a->y || !a->nf || !a->x || !a->disp) return capi_fail(DSQ_ERR_ARG, "NULL counts, size / normalization factors, design or dispersions");
    if (a->y_type != DSQ_Y_INT32 && a->y_type != DSQ_Y_FLOAT64) return capi_fail(DSQ_ERR_ARG, "unknown y_type %d", a->y_type);
    if (!o->map || !o->sd || !o->fsr || !o->thresh || !o->iter || !o->conv || !o->start || !o->objective)
        return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (a->coef < 0 || a->coef >= a->p) return capi_fail(DSQ_ERR_ARG, "coef = %d is outside [0, %d)", a->coef, a->p);
    if ((a->no_shrink >> a->coef) & 1u) return capi_fail(DSQ_ERR_ARG, "coef = %d is among the columns that are not shrunk", a->coef);
    if (a->p < 32 && (a->no_shrink >> a->p)) return capi_fail(DSQ_ERR_ARG, "no_shrink names a column beyond p = %d", a->p);
    const auto positive = [](double v) { return v > 0.0 && v - v == 0.0; };
    if (!positive(a->prior_scale) || !positive(a->prior_df) || !positive(a->no_shrink_scale))
        return capi_fail(DSQ_ERR_ARG, "prior_scale = %g, prior_df = %g, no_shrink_scale = %g must be positive and finite", a->prior_scale,
                         a->prior_df, a->no_shrink_scale);
    if (a->has_threshold && !(a->threshold >= 0.0)) return capi_fail(DSQ_ERR_ARG, "threshold = %g must not be negative", a->threshold);
    if (a->maxit < 0 || a->tol != a->tol) return capi_fail(DSQ_ERR_ARG, "bad tol / maxit");
    return DSQ_OK;
}

int apeglm_dev_locked(const DsqApeglmArgs *a, const DsqApeglmOut *o, hipStream_t st) {
    if (int rc = apeglm_check(a, o)) return rc;
    if (int rc = check_layout(a->layout, a->ld, a->m, true)) return rc;
    if (int rc = capi_check_device()) return rc;
    ApeglmKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = a->p;
    kp.y = a->y;
    const bool gm = a->layout == DSQ_LAYOUT_GENE_MAJOR;
    kp.si = gm ? (long)a->ld : 1L;  kp.sj = gm ? 1L : (long)a->n;
    kp.nf = a->nf; kp.nf_is_vector = a->nf_is_vector ? 1 : 0;
    kp.x = a->x; kp.weights = a->weights; kp.disp = a->disp; kp.init = a->init;
    kp.coef = a->coef; kp.no_shrink = a->no_shrink;
    kp.prior_scale = a->prior_scale; kp.prior_df = a->prior_df; kp.no_shrink_scale = a->no_shrink_scale;
    kp.has_threshold = a->has_threshold ? 1 : 0; kp.threshold = a->threshold;
    kp.tol = a->tol; kp.maxit = a->maxit;
    kp.map = o->map; kp.sd = o->sd; kp.fsr = o->fsr; kp.thresh = o->thresh; kp.iter = o->iter; kp.conv = o->conv;
    kp.start = o->start; kp.objective = o->objective;
    kp.bad = a->y_type == DSQ_Y_FLOAT64 ? o->bad : nullptr;
    capi_prof_begin("apeglm", a->n, st);
    DSQ_HIP(launch_apeglm(kp, a->y_type == DSQ_Y_FLOAT64, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// adaptive shrinkage (ash.hip): what both entries check before anything is launched
int ash_check(const DsqAshArgs *a, const DsqAshOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->C < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->ld < a->n) return capi_fail(DSQ_ERR_ARG, "ld = %lld < n = %d", (long long)a->ld, a->n);
    if (!a->betahat || !a->sebetahat) return capi_fail(DSQ_ERR_ARG, "NULL betahat or sebetahat");
    if (!o->PosteriorMean || !o->PosteriorSD || !o->NegativeProb || !o->PositiveProb || !o->lfsr || !o->le_T || !o->gt_mT || !o->pi ||
        !o->sd || !o->K || !o->iter || !o->flag || !o->loglik)
        return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (a->has_threshold && !(a->threshold >= 0.0)) return capi_fail(DSQ_ERR_ARG, "threshold = %g must not be negative", a->threshold);
    if (a->maxit < 0) return capi_fail(DSQ_ERR_ARG, "maxit = %d is negative", a->maxit);
    return DSQ_OK;
}

int ash_dev_locked(const DsqAshArgs *a, const DsqAshOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st) {
    if (int rc = ash_check(a, o)) return rc;
    const size_t need = ash_workspace_bytes(a->n, a->C);
    if (!workspace || workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: %zu are needed (dsq_ash_workspace_bytes)", (long long)workspace_bytes, need);
    if (int rc = capi_check_device()) return rc;
    AshKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.C = a->C; kp.ld = (long)a->ld;
    kp.b = a->betahat; kp.s = a->sebetahat;
    kp.has_threshold = a->has_threshold ? 1 : 0; kp.threshold = a->threshold; kp.maxit = a->maxit;
    kp.pm = o->PosteriorMean; kp.psd = o->PosteriorSD; kp.neg = o->NegativeProb; kp.pos = o->PositiveProb; kp.lfsr = o->lfsr;
    kp.le_t = o->le_T; kp.gt_mt = o->gt_mT;
    kp.pi = o->pi; kp.sd = o->sd; kp.K = o->K; kp.iter = o->iter; kp.flag = o->flag; kp.loglik = o->loglik;
    capi_prof_begin("ash", a->n, st);
    const int rc = launch_ash(kp, workspace, st);
    capi_prof_end(st);
    return rc;
}

// unmix() (unmix.hip): what both entries check before anything is launched
int unmix_check(const DsqUnmixArgs *a, const DsqUnmixOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->k < 2) return capi_fail(DSQ_ERR_ARG, "k = %d pure components: at least two are needed", a->k);
    if (a->k > DSQ_UNMIX_MAX_K) return capi_fail(DSQ_ERR_UNSUPPORTED, "k = %d pure components: at most %d", a->k, DSQ_UNMIX_MAX_K);
    if (!a->x || !a->pure) return capi_fail(DSQ_ERR_ARG, "NULL x or pure");
    if (!o->p || !o->loss || !o->iter || !o->flag) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (!a->has_alpha == !a->has_shift) return capi_fail(DSQ_ERR_ARG, "exactly one of alpha and shift is to be given");
    const double v = a->has_alpha ? a->alpha : a->shift;
    if (!(v > 0.0) || v - v != 0.0) return capi_fail(DSQ_ERR_ARG, "%s = %g must be positive and finite", a->has_alpha ? "alpha" : "shift", v);
    if (a->power != 1 && a->power != 2) return capi_fail(DSQ_ERR_ARG, "power = %d: 1 or 2", a->power);
    if (a->maxit < 0) return capi_fail(DSQ_ERR_ARG, "maxit = %d is negative", a->maxit);
    return DSQ_OK;
}

int unmix_dev_locked(const DsqUnmixArgs *a, const DsqUnmixOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st) {
    if (int rc = unmix_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    const size_t need = unmix_workspace_bytes(a->n, a->m);
    if (!workspace || workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: %zu are needed (dsq_unmix_workspace_bytes)", (long long)workspace_bytes, need);
    if (int rc = capi_check_device()) return rc;
    UnmixKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.k = a->k; kp.ld = (long)a->ld;
    kp.x = a->x; kp.pure = a->pure;
    kp.alpha_form = a->has_alpha ? 1 : 0;
    kp.a = a->has_alpha ? a->alpha : a->shift;
    kp.power = a->power; kp.maxit = a->maxit;
    kp.vx = (double *)workspace;
    kp.p = o->p; kp.loss = o->loss; kp.iter = o->iter; kp.flag = o->flag;
    capi_prof_begin("unmix", a->m, st);
    DSQ_HIP(launch_unmix(kp, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// sample PCA / sample distances (explore.hip): what both entries check before anything is launched
int top_var_check(const DsqTopVarArgs *a, const DsqTopVarOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->m < 2) return capi_fail(DSQ_ERR_ARG, "m = %d samples: a variance needs at least two", a->m);
    if (a->ntop < 0) return capi_fail(DSQ_ERR_ARG, "ntop = %d is negative", a->ntop);
    if (!a->x) return capi_fail(DSQ_ERR_ARG, "NULL x");
    if (!o->rowMean || !o->rowVar || (a->ntop > 0 && !o->select)) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    return DSQ_OK;
}

int top_var_dev_locked(const DsqTopVarArgs *a, const DsqTopVarOut *o, hipStream_t st) {
    if (int rc = top_var_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (int rc = capi_check_device()) return rc;
    RowVarsKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.ld = (long)a->ld; kp.x = a->x;
    kp.rowMean = o->rowMean; kp.rowVar = o->rowVar;
    capi_prof_begin("top_var", a->n, st);
    DSQ_HIP(launch_row_vars(kp, st));
    const int k = a->ntop < a->n ? a->ntop : a->n;
    if (k > 0) {
        void *w;
        if (int rc = capi_ws_get(WS_SCRATCH, top_var_workspace_bytes(a->n), &w)) return rc;
        DSQ_HIP(launch_top_var_order(o->rowVar, a->n, k, o->select, w, st));
    }
    capi_prof_end(st);
    return DSQ_OK;
}

int sample_pairs_check(const DsqSamplePairsArgs *a, const DsqSamplePairsOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->m < 2) return capi_fail(DSQ_ERR_ARG, "m = %d samples: pairs need at least two", a->m);
    if (a->kind != DSQ_PAIRS_DIST2 && a->kind != DSQ_PAIRS_DIST && a->kind != DSQ_PAIRS_GRAM) return capi_fail(DSQ_ERR_ARG, "unknown kind %d", a->kind);
    if (!a->x) return capi_fail(DSQ_ERR_ARG, "NULL x");
    if (a->rows ? a->nrows < 1 : (a->nrows != 0 && a->nrows != a->n))
        return capi_fail(DSQ_ERR_ARG, "nrows = %d: %s", a->nrows, a->rows ? "a row list has at least one entry" : "0 or n without a row list");
    if (!o->out) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    return DSQ_OK;
}

int sample_pairs_dev_locked(const DsqSamplePairsArgs *a, const DsqSamplePairsOut *o, hipStream_t st) {
    if (int rc = sample_pairs_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (int rc = capi_check_device()) return rc;
    PairKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.ld = (long)a->ld; kp.x = a->x;
    kp.kind = a->kind == DSQ_PAIRS_GRAM ? PAIR_GRAM : PAIR_DIST2;
    kp.root = a->kind == DSQ_PAIRS_DIST ? 1 : 0;
    kp.R = a->rows ? a->nrows : a->n;
    kp.rows = a->rows;
    kp.centre = a->kind == DSQ_PAIRS_GRAM ? a->centre : nullptr;
    PairSlices ps;
    pair_slices(kp.R, kp.m, &ps);
    kp.nb = ps.nb; kp.ntiles = ps.ntiles; kp.L = ps.L; kp.S = ps.S;
    void *w;
    if (int rc = capi_ws_get(WS_SCRATCH, pair_workspace_bytes(kp.R, kp.m), &w)) return rc;
    kp.partial = (double *)w;
    kp.out = o->out;
    capi_prof_begin("sample_pairs", a->m, st);
    DSQ_HIP(launch_pair_sums(kp, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// the local-regression dispersion trend (local_fit.hip): what both entries check before anything is launched
int local_fit_check(const DsqLocalFitArgs *a, const DsqLocalFitOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!o->status) return capi_fail(DSQ_ERR_ARG, "NULL status");
    if (!(a->minDisp > 0.0)) return capi_fail(DSQ_ERR_ARG, "minDisp must be > 0");
    if (a->n_eval < 0 || (a->eval_means ? a->n_eval < 1 : a->n_eval != 0))
        return capi_fail(DSQ_ERR_ARG, "n_eval = %d: %s", a->n_eval, a->eval_means ? "an evaluation list has at least one entry" : "0 without eval_means");
    if (a->fit_in) {
        if (!a->eval_means || !o->dispFit) return capi_fail(DSQ_ERR_ARG, "fit_in: eval_means and dispFit are needed");
    } else if (!a->means || !a->disps) return capi_fail(DSQ_ERR_ARG, "NULL means or disps");
    if (a->eval_means && !o->dispFit) return capi_fail(DSQ_ERR_ARG, "eval_means without dispFit");
    return DSQ_OK;
}

int local_fit_dev_locked(const DsqLocalFitArgs *a, const DsqLocalFitOut *o, hipStream_t st) {
    if (int rc = local_fit_check(a, o)) return rc;
    if (int rc = capi_check_device()) return rc;
    const double *block = a->fit_in;
    capi_prof_begin("local_fit", a->n, st);
    if (!block) {
        void *w, *b = o->fit;
        if (int rc = capi_ws_get(WS_SCRATCH, local_fit_workspace_bytes(a->n), &w)) return rc;
        if (!b)
            if (int rc = capi_ws_get(WS_TREND, (kLocalFitHeaderDoubles + 3 * (size_t)a->n) * 8, &b)) return rc;
        DSQ_HIP(launch_local_fit_build(a->means, a->disps, a->n, a->minDisp, (double *)b, w, st));
        block = (const double *)b;
    }
    const double *q = a->eval_means ? a->eval_means : a->means;
    const long nq = !o->dispFit ? 0 : a->eval_means ? a->n_eval : a->n;
    DSQ_HIP(launch_local_fit_eval(block, q, nq, o->dispFit, o->status, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// collapseReplicates / colSums / fpm / fpkm (count_helpers.hip): what both entries check before anything is launched
int collapse_check(const DsqCollapseArgs *a, const DsqCollapseOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->g < 1 || a->g > a->m) return capi_fail(DSQ_ERR_ARG, "g = %d groups of m = %d samples", a->g, a->m);
    if (!a->y || !a->members || !a->offsets) return capi_fail(DSQ_ERR_ARG, "NULL counts, members or offsets");
    if (!o->out) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    return DSQ_OK;
}

int collapse_dev_locked(const DsqCollapseArgs *a, const DsqCollapseOut *o, hipStream_t st) {
    if (int rc = collapse_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (o->ld < a->g) return capi_fail(DSQ_ERR_ARG, "output ld = %ld < g = %d", (long)o->ld, a->g);
    if (!o->status) return capi_fail(DSQ_ERR_ARG, "NULL status");
    if (int rc = capi_check_device()) return rc;
    CollapseKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.g = a->g; kp.ld = (long)a->ld; kp.ldo = (long)o->ld;
    kp.y = a->y; kp.members = a->members; kp.offsets = a->offsets;
    kp.out = o->out; kp.status = o->status;
    capi_prof_begin("collapse", a->n, st);
    DSQ_HIP(launch_collapse(kp, st));
    capi_prof_end(st);
    return DSQ_OK;
}

int col_sums_check(const DsqColSumsArgs *a, const DsqColSumsOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y) return capi_fail(DSQ_ERR_ARG, "NULL counts");
    if (!o->sums) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    return DSQ_OK;
}

int col_sums_dev_locked(const DsqColSumsArgs *a, const DsqColSumsOut *o, hipStream_t st) {
    if (int rc = col_sums_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (int rc = capi_check_device()) return rc;
    ColSumsKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.ld = (long)a->ld; kp.y = a->y;
    kp.sums = (long long *)o->sums;
    capi_prof_begin("col_sums", a->n, st);
    DSQ_HIP(launch_col_sums(kp, st));
    capi_prof_end(st);
    return DSQ_OK;
}

int fpm_check(const DsqFpmArgs *a, const DsqFpmOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->struct_size != sizeof *a || o->struct_size != sizeof *o) return capi_fail(DSQ_ERR_ARG, "struct_size is not sizeof the block");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->kind != DSQ_FPM && a->kind != DSQ_FPKM_BASEPAIRS && a->kind != DSQ_FPKM_TXLEN) return capi_fail(DSQ_ERR_ARG, "unknown kind %d", a->kind);
    if (!a->y || !a->lib) return capi_fail(DSQ_ERR_ARG, "NULL counts or library sizes");
    if (a->kind == DSQ_FPKM_BASEPAIRS && !a->basepairs) return capi_fail(DSQ_ERR_ARG, "DSQ_FPKM_BASEPAIRS: NULL basepairs");
    if (a->kind == DSQ_FPKM_TXLEN && !a->txlen) return capi_fail(DSQ_ERR_ARG, "DSQ_FPKM_TXLEN: NULL txlen");
    if (!o->out) return capi_fail(DSQ_ERR_ARG, "NULL output matrix");
    return DSQ_OK;
}

int fpm_dev_locked(const DsqFpmArgs *a, const DsqFpmOut *o, hipStream_t st) {
    if (int rc = fpm_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (int rc = capi_check_device()) return rc;
    FpmKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.ld = (long)a->ld; kp.y = a->y;
    kp.kind = a->kind;
    kp.lib = a->lib;
    kp.basepairs = a->kind == DSQ_FPKM_BASEPAIRS ? a->basepairs : nullptr;
    kp.txlen = a->kind == DSQ_FPKM_TXLEN ? a->txlen : nullptr;
    kp.out = o->out;
    capi_prof_begin("fpm", a->n, st);
    DSQ_HIP(launch_fpm(kp, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// the solve of estimateSizeFactors(type = "iterate") (sf_iterate.hip): what both entries check before anything is launched
int sf_iterate_check(const DsqSfIterateArgs *a, const DsqSfIterateOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->mu || !a->sf || !a->disp || !a->rows) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (!o->s || !o->sf || !o->F || !o->iter || !o->evals || !o->flag) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (!(a->Q >= 0.0 && a->Q < 1.0)) return capi_fail(DSQ_ERR_ARG, "Q = %g: a probability below 1", a->Q);
    if (a->maxit < 0) return capi_fail(DSQ_ERR_ARG, "maxit = %d is negative", a->maxit);
    return DSQ_OK;
}

int sf_iterate_dev_locked(const DsqSfIterateArgs *a, const DsqSfIterateOut *o, void *workspace, int64_t workspace_bytes, hipStream_t st) {
    if (int rc = sf_iterate_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    const size_t need = sf_iterate_workspace_bytes(a->n, a->m);
    if (!workspace || workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: %zu are needed (dsq_sf_iterate_workspace_bytes)", (long long)workspace_bytes, need);
    if (int rc = capi_check_device()) return rc;
    SfIterateKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.ld = (long)a->ld;
    kp.y = a->y; kp.mu = a->mu; kp.sf = a->sf; kp.disp = a->disp; kp.rows = a->rows;
    kp.Q = a->Q; kp.maxit = a->maxit;
    kp.s_out = o->s; kp.sf_out = o->sf; kp.F_out = o->F;
    kp.iter_out = o->iter; kp.evals_out = o->evals; kp.flag_out = o->flag;
    capi_prof_begin("sf_iterate", a->n, st);
    DSQ_HIP(launch_sf_iterate(kp, workspace, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// results() (results.hip): what both entries check before anything is launched
int results_check(const DsqResultsArgs *a, const DsqResultsOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1) return capi_fail(DSQ_ERR_ARG, "n = %d: at least one gene is needed", a->n);
    if (a->p < 1 || a->c < 0 || a->c >= a->p) return capi_fail(DSQ_ERR_ARG, "coefficient c = %d outside 0 .. p - 1 (p = %d)", a->c, a->p);
    if (!a->beta || !a->betaSE || !a->stat || !a->pvalue || !a->baseMean)
        return capi_fail(DSQ_ERR_ARG, "NULL beta, betaSE, stat, pvalue or baseMean");
    if (!o->baseMean || !o->log2FoldChange || !o->lfcSE || !o->stat || !o->pvalue || !o->numRej || !o->cutoffs || !o->status)
        return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (a->test != DSQ_TEST_WALD && a->test != DSQ_TEST_LRT) return capi_fail(DSQ_ERR_ARG, "unknown test %d", a->test);
    if (a->altHypothesis < DSQ_ALT_GREATER_ABS || a->altHypothesis > DSQ_ALT_GREATER_ABS_2014)
        return capi_fail(DSQ_ERR_ARG, "unknown altHypothesis %d", a->altHypothesis);
    if (!(a->alpha > 0.0 && a->alpha < 1.0)) return capi_fail(DSQ_ERR_ARG, "alpha = %g must lie in (0, 1)", a->alpha);
    if (!(a->lfcThreshold >= 0.0)) return capi_fail(DSQ_ERR_ARG, "lfcThreshold = %g must be >= 0", a->lfcThreshold);
    if (a->lfcThreshold == 0.0 && a->altHypothesis == DSQ_ALT_LESS_ABS)
        return capi_fail(DSQ_ERR_ARG, "altHypothesis lessAbs needs a positive lfcThreshold");
    if (a->test == DSQ_TEST_LRT && !(a->lfcThreshold == 0.0 && a->altHypothesis == DSQ_ALT_GREATER_ABS))
        return capi_fail(DSQ_ERR_ARG, "tests of log fold change above or below a threshold must be Wald tests");
    if (a->independentFiltering) {
        if (a->K < 2 || a->K > DSQ_RESULTS_MAX_K) return capi_fail(DSQ_ERR_ARG, "K = %d thresholds: 2 .. %d", a->K, DSQ_RESULTS_MAX_K);
        if (!a->theta) return capi_fail(DSQ_ERR_ARG, "NULL theta");
    } else if (a->K != 1) return capi_fail(DSQ_ERR_ARG, "K = %d: independentFiltering = 0 takes K = 1", a->K);
    return DSQ_OK;
}

int results_dev_locked(const DsqResultsArgs *a, const DsqResultsOut *o, hipStream_t st) {
    if (int rc = results_check(a, o)) return rc;
    const size_t sortb = results_sort_workspace_bytes(a->n);
    const size_t need = sortb + (o->filtPadj ? 0 : (size_t)a->n * a->K * 8);
    if (!a->workspace || a->workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: %zu are needed (dsq_results_workspace_bytes)", (long long)a->workspace_bytes, need);
    if (int rc = capi_check_device()) return rc;
    ResultsKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.p = a->p; kp.c = a->c;
    kp.lrt = a->test == DSQ_TEST_LRT;
    kp.alt = a->altHypothesis;
    kp.threshold = !(a->lfcThreshold == 0.0 && a->altHypothesis == DSQ_ALT_GREATER_ABS);      // R/results.R:464
    kp.T = a->lfcThreshold; kp.alpha = a->alpha;
    kp.beta = a->beta; kp.betaSE = a->betaSE; kp.stat = a->stat; kp.pvalue = a->pvalue; kp.baseMean = a->baseMean;
    kp.replace = a->replace; kp.na_mask = a->na_mask; kp.df = a->df;
    kp.filter = a->filter ? a->filter : a->baseMean;
    kp.theta = a->independentFiltering ? a->theta : nullptr;
    kp.K = a->K;
    kp.o_baseMean = o->baseMean; kp.o_lfc = o->log2FoldChange; kp.o_se = o->lfcSE; kp.o_stat = o->stat; kp.o_pvalue = o->pvalue;
    kp.filtPadj = o->filtPadj ? o->filtPadj : (double *)((char *)a->workspace + sortb);
    kp.numRej = o->numRej; kp.cutoffs = o->cutoffs; kp.status = o->status;
    capi_prof_begin("results", a->n, st);
    DSQ_HIP(launch_results(kp, a->workspace, st));
    capi_prof_end(st);
    return DSQ_OK;
}

// contrasts (contrasts.hip): what both entries check; a pointer is needed only by the mode that reads it (contrasts == NULL:
// the all-zero flags alone)
int contrasts_check(const DsqContrastsArgs *a, const DsqContrastsOut *o) {
    DSQ_NEED(a && o, "NULL args/out");
    if (a->n < 0 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions n=%d m=%d p=%d", a->n, a->m, a->p);
    if (a->K < 1) return capi_fail(DSQ_ERR_ARG, "K = %d: at least one contrast is needed", a->K);
    DSQ_NEED(a->contrasts || a->sample_mask, "neither contrasts nor sample_mask given");
    DSQ_NEED(!a->contrasts || (a->x && a->nf && a->alpha_hat && a->beta && a->lambda), "NULL input array");
    DSQ_NEED(!a->contrasts || !a->useWeights || a->weights, "useWeights set but weights is NULL");
    DSQ_NEED(!a->sample_mask || a->counts, "sample_mask given without counts");
    DSQ_NEED(!a->sample_mask || a->rule_applies, "sample_mask given without rule_applies");
    DSQ_NEED(!a->contrasts || (o->log2FoldChange && o->lfcSE && o->stat && o->pvalue), "NULL output array");
    DSQ_NEED(!a->sample_mask || o->contrastAllZero, "sample_mask given but contrastAllZero is NULL");
    return a->p > DSQ_P_WIDE ? too_wide(a->p) : DSQ_OK;
}

int pt_check(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const double *out) {
    if (n < 0 || K < 0) return capi_fail(DSQ_ERR_ARG, "bad dimensions n=%d K=%d", n, K);
    if (tail < DSQ_PT_LOWER || tail > DSQ_PT_TWO_SIDED) return capi_fail(DSQ_ERR_ARG, "unknown tail %d", tail);
    if ((int64_t)n * K > 0 && (!q || !df || !out)) return capi_fail(DSQ_ERR_ARG, "NULL q, df or out");
    if (((int64_t)n * K + 255) / 256 > 0x7fffffffLL) return capi_fail(DSQ_ERR_ARG, "n K = %lld entries: too many for one launch", (long long)n * K);
    return DSQ_OK;
}

int contrasts_dev_locked(const DsqContrastsArgs *a, const DsqContrastsOut *o, hipStream_t st) {
    if (int rc = contrasts_check(a, o)) return rc;
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld = %ld < m = %d", (long)a->ld, a->m);
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    ContrastsKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = a->p; kp.K = a->K; kp.ld = (long)a->ld;
    kp.x = a->x; kp.nf = a->nf; kp.nf_is_vector = a->nf_is_vector ? 1 : 0;
    kp.alpha_hat = a->alpha_hat; kp.beta = a->beta; kp.lambda = a->lambda;
    kp.useWeights = a->useWeights ? 1 : 0;
    kp.weights = kp.useWeights ? a->weights : nullptr;
    kp.minmu = a->minmu;
    kp.contrasts = a->contrasts; kp.allZero = a->allZero;
    kp.counts = a->sample_mask ? a->counts : nullptr;
    kp.sample_mask = a->sample_mask; kp.rule_applies = a->sample_mask ? a->rule_applies : nullptr;
    kp.lfc = o->log2FoldChange; kp.se = o->lfcSE; kp.stat = o->stat; kp.pvalue = o->pvalue; kp.flags = o->contrastAllZero;
    // the Gram sums' form is the one dsq_fit_beta_dev takes for this design (fit_beta_on_cells at the kernel width)
    const int pk = is_wide(a->p) ? wide_width(a->p) : a->p;
    if (a->contrasts && a->cell_of && a->ncell > 0 && fit_beta_on_cells(pk, 1)) {
        const int C = capi_upload_cells(a->cell_of, a->m, WS_CELLS_BETA, st, &kp.cell_perm, &kp.cell_start);
        kp.ncell = fit_beta_on_cells(pk, C) ? C : 0;
    }
    bool ok = false;
    capi_prof_begin("contrasts", a->n, st);
    DSQ_HIP(launch_contrasts(kp, st, &ok));
    // a useT analysis: 2 pt(|stat|, df, lower.tail = FALSE) over the stat column (R/results.R:812-815); the entries the
    // all-zero rule has set to 1 stay (cleanContrast runs after getContrast), rows flagged allZero hold NaN in stat
    if (ok && a->df && a->contrasts)
        DSQ_HIP(launch_pt(o->stat, a->df, a->n, a->K, DSQ_PT_TWO_SIDED, a->sample_mask ? o->contrastAllZero : nullptr, o->pvalue, st));
    capi_prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "rows of m=%d samples at p=%d: the per-sample path takes at most %d", a->m, a->p,
                              contrasts_max_m(a->p));
    return DSQ_OK;
}

}  // namespace dsq

using namespace dsq;

// a `_dev` entry point: the call lock, the stream's context latched for the call, then the body
template <class F>
static int dev_entry(void *stream, F &&body) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws((hipStream_t)stream);
    return body((hipStream_t)stream);
}

extern "C" {

#define DSQ_DEV(name, A, O, call) \
    int name(const A *a, O o, void *s) { return dev_entry(s, [&](hipStream_t st) { return call; }); }
DSQ_DEV(dsq_fit_beta_dev, DsqFitBetaArgs, const DsqFitBetaOut *, fit_beta_dev_locked(a, o, st))
DSQ_DEV(dsq_fit_disp_dev, DsqFitDispArgs, const DsqFitDispOut *, fit_disp_dev_locked(a, o, st))
DSQ_DEV(dsq_fit_disp_grid_dev, DsqFitDispGridArgs, const DsqFitDispGridOut *, fit_disp_grid_dev_locked(a, o, st))
DSQ_DEV(dsq_prefit_moments_dev, DsqPrefitArgs, const DsqPrefitOut *, prefit_dev_locked(a, o, st))
DSQ_DEV(dsq_nbinom_loglike_dev, DsqLogLikeArgs, double *, loglike_dev_locked(a, o, st))
DSQ_DEV(dsq_intercept_fit_dev, DsqInterceptArgs, const DsqInterceptOut *, intercept_dev_locked(a, o, st))
DSQ_DEV(dsq_cooks_distance_dev, DsqCooksArgs, const DsqCooksOut *, cooks_dev_locked(a, o, st))
DSQ_DEV(dsq_replace_outliers_dev, DsqReplaceArgs, const DsqReplaceOut *, replace_dev_locked(a, o, st))
DSQ_DEV(dsq_size_factors_dev, DsqSizeFactorArgs, const DsqSizeFactorOut *, size_factors_dev_locked(a, o, st))
DSQ_DEV(dsq_vst_dev, DsqVstArgs, const DsqVstOut *, vst_dev_locked(a, o, true, false, st))
DSQ_DEV(dsq_vst_rowstats_dev, DsqVstArgs, const DsqVstOut *, vst_dev_locked(a, o, false, true, st))
DSQ_DEV(dsq_rlog_dev, DsqRlogArgs, const DsqRlogOut *, rlog_dev_locked(a, o, st))
DSQ_DEV(dsq_apeglm_dev, DsqApeglmArgs, const DsqApeglmOut *, apeglm_dev_locked(a, o, st))
DSQ_DEV(dsq_results_dev, DsqResultsArgs, const DsqResultsOut *, results_dev_locked(a, o, st))
DSQ_DEV(dsq_contrasts_dev, DsqContrastsArgs, const DsqContrastsOut *, contrasts_dev_locked(a, o, st))
DSQ_DEV(dsq_top_var_dev, DsqTopVarArgs, const DsqTopVarOut *, top_var_dev_locked(a, o, st))
DSQ_DEV(dsq_sample_pairs_dev, DsqSamplePairsArgs, const DsqSamplePairsOut *, sample_pairs_dev_locked(a, o, st))
DSQ_DEV(dsq_collapse_dev, DsqCollapseArgs, const DsqCollapseOut *, collapse_dev_locked(a, o, st))
DSQ_DEV(dsq_col_sums_dev, DsqColSumsArgs, const DsqColSumsOut *, col_sums_dev_locked(a, o, st))
DSQ_DEV(dsq_fpm_dev, DsqFpmArgs, const DsqFpmOut *, fpm_dev_locked(a, o, st))
DSQ_DEV(dsq_local_fit_dev, DsqLocalFitArgs, const DsqLocalFitOut *, local_fit_dev_locked(a, o, st))
#undef DSQ_DEV
int dsq_linear_mu_dev(const DsqPrefitArgs *a, double mu_floor, double *mu, void *s) {
    return dev_entry(s, [&](hipStream_t st) { return linear_mu_dev_locked(a, mu_floor, mu, st); });
}
int dsq_parametric_dispersion_fit_dev(const double *means, const double *disps, int64_t n, double *coefs, int32_t *status,
                                      void *s) {
    return dev_entry(s, [&](hipStream_t st) -> int {
        if (int rc = check_trend_fit(means, disps, n, coefs, status)) return rc;
        if (int rc = capi_check_device()) return rc;
        prof_begin(st);
        void *tws;
        if (int rc = capi_ws_get(WS_TREND, trend_fit_workspace_bytes(), &tws)) return rc;
        DSQ_HIP(launch_trend_fit(means, disps, (long)n, coefs, status, tws, st));
        prof_end(st);
        return DSQ_OK;
    });
}

int dsq_unmix_dev(const DsqUnmixArgs *a, const DsqUnmixOut *o, void *workspace, int64_t workspace_bytes, void *s) {
    return dev_entry(s, [&](hipStream_t st) { return unmix_dev_locked(a, o, workspace, workspace_bytes, st); });
}
int32_t dsq_apeglm_lds_doubles(void) { return kApeXLdsDoubles; }
int dsq_ash_dev(const DsqAshArgs *a, const DsqAshOut *o, void *workspace, int64_t workspace_bytes, void *s) {
    return dev_entry(s, [&](hipStream_t st) { return ash_dev_locked(a, o, workspace, workspace_bytes, st); });
}
int64_t dsq_ash_workspace_bytes(int32_t n, int32_t C) {
    if (n < 1 || C < 1) return 0;
    return (int64_t)ash_workspace_bytes(n, C);
}
int32_t dsq_ash_slice_rows(void) { return kAshSliceRows; }
int64_t dsq_unmix_workspace_bytes(int32_t n, int32_t m, int32_t k) {
    if (n < 1 || m < 1 || k < 1) return 0;
    return (int64_t)unmix_workspace_bytes(n, m);
}
int32_t dsq_unmix_block_threads(void) { return kUnmixThreads; }

int dsq_sf_iterate_dev(const DsqSfIterateArgs *a, const DsqSfIterateOut *o, void *workspace, int64_t workspace_bytes, void *s) {
    return dev_entry(s, [&](hipStream_t st) { return sf_iterate_dev_locked(a, o, workspace, workspace_bytes, st); });
}
int64_t dsq_sf_iterate_workspace_bytes(int32_t n, int32_t m) {
    if (n < 1 || m < 1) return 0;
    return (int64_t)sf_iterate_workspace_bytes(n, m);
}
int32_t dsq_sf_iterate_slice_genes(void) { return kSfIterSliceGenes; }

int64_t dsq_sample_pairs_slice_rows(int64_t rows_summed, int32_t m) {
    if (rows_summed < 1 || m < 1) return 0;
    PairSlices ps;
    pair_slices((long)rows_summed, m, &ps);
    return (int64_t)ps.L;
}
int32_t dsq_row_vars_register_width(void) { return row_vars_register_width(); }

int32_t dsq_local_fit_lanes(void) { return kLocalFitLanes; }
int64_t dsq_local_fit_block_doubles(int32_t n) { return n < 1 ? 0 : kLocalFitHeaderDoubles + 3 * (int64_t)n; }

int64_t dsq_size_factors_workspace_bytes(int32_t n, int32_t m) {
    if (n < 0 || m < 0) return 0;
    return (int64_t)size_factors_workspace_bytes(n, m);
}

int32_t dsq_contrasts_max_m(int32_t p) { return contrasts_max_m(p); }

int dsq_pt_dev(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const int32_t *keep, double *out,
               void *stream) {
    if (int rc = pt_check(q, df, n, K, tail, out)) return rc;
    if (int rc = capi_check_device()) return rc;
    DSQ_HIP(launch_pt(q, df, n, K, tail, keep, out, (hipStream_t)stream));
    return DSQ_OK;
}

int64_t dsq_results_workspace_bytes(int32_t n, int32_t K) {
    if (n < 0 || K < 0) return 0;
    const size_t sortb = results_sort_workspace_bytes(n);
    return (int64_t)(((sortb + 7) & ~(size_t)7) + (size_t)n * K * 8);
}

int dsq_weights_prep_dev(const double *weights_raw, const double *x, int32_t n, int32_t m, int32_t p, int64_t ld,
                         double weightThreshold, double *w_norm, double *w_floor, int32_t *weightsFail,
                         int32_t *any_negative, void *stream) {
    if (!weights_raw || !x || !w_norm || !w_floor || !weightsFail || !any_negative || n < 0 || m < 1 || ld < m)
        return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (p < 1 || p > DSQ_P_WIDE) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_weights_prep_dev: p=%d design columns (1..%d)", p, DSQ_P_WIDE);
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    DSQ_HIP(launch_weights_prep(weights_raw, x, n, m, p, ld, weightThreshold, w_norm, w_floor, weightsFail, any_negative,
                                (hipStream_t)stream));
    return DSQ_OK;
}
int dsq_xim_dev(const double *nf, int32_t n, int32_t m, int64_t ld, double *scratch_m, double *out, void *stream) {
    if (!nf || !scratch_m || !out || n < 1 || m < 1 || ld < m) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    DSQ_HIP(launch_xim(nf, n, m, ld, scratch_m, out, (hipStream_t)stream));
    return DSQ_OK;
}

int dsq_to_gene_major_f64(const double *src_r, double *dst_gm, int32_t n, int32_t m, int64_t ld, void *stream) {
    if (!src_r || !dst_gm || n < 0 || m < 1 || ld < m) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    DSQ_HIP(launch_transpose_r_to_gm_f64(src_r, dst_gm, n, m, ld, (hipStream_t)stream));
    return DSQ_OK;
}
int dsq_to_gene_major_i32(const int32_t *src_r, int32_t *dst_gm, int32_t n, int32_t m, int64_t ld, void *stream) {
    if (!src_r || !dst_gm || n < 0 || m < 1 || ld < m) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    DSQ_HIP(launch_transpose_r_to_gm_i32(src_r, dst_gm, n, m, ld, (hipStream_t)stream));
    return DSQ_OK;
}
int dsq_counts_f64_to_gene_major_i32(const double *src_r, int32_t *dst_gm, int32_t n, int32_t m, int64_t ld,
                                     int32_t *bad, void *stream) {
    if (!src_r || !dst_gm || !bad || n < 0 || m < 1 || ld < m) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    DSQ_HIP(launch_counts_f64_to_gm_i32(src_r, dst_gm, n, m, ld, bad, (hipStream_t)stream));
    return DSQ_OK;
}
int dsq_from_gene_major_f64(const double *src_gm, double *dst_r, int32_t n, int32_t m, int64_t ld, void *stream) {
    if (!src_gm || !dst_r || n < 0 || m < 1 || ld < m) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    DSQ_HIP(launch_transpose_gm_to_r_f64(src_gm, dst_r, n, m, ld, (hipStream_t)stream));
    return DSQ_OK;
}

}  // extern "C"
