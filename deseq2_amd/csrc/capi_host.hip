// capi_host.hip -- the host-pointer entry points of the C ABI (what r_shim.c binds: R memory in, R memory out,
// synchronous); see capi.hip for the three files of the host side.
//
// Genes are independent inside every native routine (src/DESeq2.cpp:194,319,492) and the reference's only parallelism
// splits them into contiguous ranges (R/parallel.R:10).  The host-pointer entry points do the same INSIDE the library:
// [0, n) is cut into one range per visible device (idx <- sort(rep(seq_len(G), length.out = n))), each range is
// uploaded / fitted / downloaded by a persistent worker thread bound to its device and its own stream, so an
// unchanged R session calling .Call("fitBeta", ...) uses every GPU of the node.  DSQ_HOST_DEVICES caps the number
// of devices, DSQ_HOST_SHARDS forces a number of ranges (ranges beyond the device count share devices: used by the
// tests to exercise the split on one GPU).
#include "capi.hpp"

#include <cstdio>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <thread>
#include <vector>

namespace dsq {

static int up(int slot, const void *host, size_t bytes, hipStream_t st, void **dev) {
    int rc = capi_ws_get(slot, bytes ? bytes : 8, dev);
    if (rc) return rc;
    if (bytes) return stage_h2d(*dev, host, 1, bytes, 0, bytes, 1, st);
    return DSQ_OK;
}
// device -> pageable host memory, complete on return
static int down(void *host, const void *dev, size_t bytes, hipStream_t st) {
    return stage_d2h(host, dev, 1, bytes, 0, bytes, 1, st);
}

// cell labels of a HOST design matrix (m x p column-major): rows compared exactly
static void cells_of_host_design(const double *x, int m, int p, std::vector<int32_t> *labels) {
    labels->assign(m, 0);
    std::vector<int> reps;
    for (int j = 0; j < m; j++) {
        int found = -1;
        for (size_t c = 0; c < reps.size() && found < 0; c++) {
            bool same = true;
            for (int k = 0; k < p && same; k++) same = x[j + (size_t)m * k] == x[reps[c] + (size_t)m * k];
            if (same) found = (int)c;
        }
        if (found < 0) { found = (int)reps.size(); reps.push_back(j); }
        (*labels)[j] = found;
        if ((int)reps.size() > DSQ_CMAX) { labels->clear(); return; }
    }
}

// rows [lo, lo + cnt) of a column-major n x cols host matrix <-> a column-major cnt x cols device matrix
static int up_rows(int slot, const void *host, size_t elem, size_t n, size_t lo, size_t cnt, size_t cols, hipStream_t st,
                   void **dev) {
    int rc = capi_ws_get(slot, cnt * cols * elem ? cnt * cols * elem : 8, dev);
    if (rc) return rc;
    return stage_h2d(*dev, host, elem, n, lo, cnt, cols, st);
}
static int down_rows(void *host, const void *dev, size_t elem, size_t n, size_t lo, size_t cnt, size_t cols, hipStream_t st) {
    return stage_d2h(host, dev, elem, n, lo, cnt, cols, st);
}

static int fit_beta_host_range(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, size_t lo, size_t cnt, hipStream_t st,
                               const int32_t *cells, int ncell) {
    const size_t n = a->n, m = a->m, p = a->p;
    const size_t ye = a->y_type == DSQ_Y_INT32 ? 4 : 8;
    DsqFitBetaArgs d = *a;
    DsqFitBetaOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    void *v;
    int rc;
    if ((rc = up_rows(WS_H_Y, a->y, ye, n, lo, cnt, m, st, &v))) return rc; d.y = v;
    // x, alpha_hat, contrast, beta_mat, lambda share one staging buffer
    size_t off_x = 0, off_alpha = off_x + m * p, off_con = off_alpha + cnt, off_beta = off_con + p,
           off_lam = off_beta + cnt * p, tot = off_lam + p;
    if ((rc = capi_ws_get(WS_H_VEC, tot * 8, &v))) return rc;
    double *vec = (double *)v;
    DSQ_HIP(hipMemcpyAsync(vec + off_x, a->x, m * p * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_alpha, a->alpha_hat + lo, cnt * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_con, a->contrast, p * 8, hipMemcpyHostToDevice, st));
    if (cnt == n) DSQ_HIP(hipMemcpyAsync(vec + off_beta, a->beta_mat, n * p * 8, hipMemcpyHostToDevice, st));
    else DSQ_HIP(hipMemcpy2DAsync(vec + off_beta, cnt * 8, a->beta_mat + lo, n * 8, cnt * 8, p, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_lam, a->lambda, p * 8, hipMemcpyHostToDevice, st));
    d.x = vec + off_x; d.alpha_hat = vec + off_alpha; d.contrast = vec + off_con; d.beta_mat = vec + off_beta;
    d.lambda = vec + off_lam;
    if (a->nf_is_vector) { if ((rc = up_rows(WS_H_NF, a->nf, 8, m, 0, m, 1, st, &v))) return rc; }
    else if ((rc = up_rows(WS_H_NF, a->nf, 8, n, lo, cnt, m, st, &v))) return rc;
    d.nf = (double *)v;
    if (a->useWeights) { if ((rc = up_rows(WS_H_W, a->weights, 8, n, lo, cnt, m, st, &v))) return rc; d.weights = (double *)v; }
    else d.weights = nullptr;
    // outputs
    size_t o_beta = 0, o_var = o_beta + cnt * p, o_iter = o_var + cnt * p, o_cn = o_iter + cnt, o_cd = o_cn + cnt,
           o_dev = o_cd + cnt, o_tot = o_dev + cnt;
    if ((rc = capi_ws_get(WS_H_OUTVEC, o_tot * 8, &v))) return rc;
    double *ov = (double *)v;
    od.beta_mat = ov + o_beta; od.beta_var_mat = ov + o_var; od.iter = ov + o_iter; od.contrast_num = ov + o_cn;
    od.contrast_denom = ov + o_cd; od.deviance = ov + o_dev;
    double *hat_d = nullptr, *mu_d = nullptr;
    if (o->hat_diagonals) { if ((rc = capi_ws_get(WS_H_OUTMAT, cnt * m * 8, &v))) return rc; hat_d = (double *)v; }
    if (o->mu) { if ((rc = capi_ws_get(WS_H_OUTMAT2, cnt * m * 8, &v))) return rc; mu_d = (double *)v; }
    od.hat_diagonals = hat_d; od.mu = mu_d;
    rc = fit_beta_dev_locked(&d, &od, st);
    if (rc) return rc;
    if ((rc = down_rows(o->beta_mat, od.beta_mat, 8, n, lo, cnt, p, st))) return rc;
    if ((rc = down_rows(o->beta_var_mat, od.beta_var_mat, 8, n, lo, cnt, p, st))) return rc;
    DSQ_HIP(hipMemcpyAsync(o->iter + lo, od.iter, cnt * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->contrast_num + lo, od.contrast_num, cnt * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->contrast_denom + lo, od.contrast_denom, cnt * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->deviance + lo, od.deviance, cnt * 8, hipMemcpyDeviceToHost, st));
    if (hat_d && (rc = down_rows(o->hat_diagonals, hat_d, 8, n, lo, cnt, m, st))) return rc;
    if (mu_d && (rc = down_rows(o->mu, mu_d, 8, n, lo, cnt, m, st))) return rc;
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

static int disp_host_stage(size_t n, size_t lo, size_t cnt, int m_, int p_, const void *y, int y_type, const double *x,
                           const double *mu_hat, const double *weights, int useWeights, hipStream_t st, const void **yd,
                           const double **xd, const double **mud, const double **wd) {
    const size_t m = m_, p = p_;
    void *v;
    int rc;
    if ((rc = up_rows(WS_H_Y, y, y_type == DSQ_Y_INT32 ? 4 : 8, n, lo, cnt, m, st, &v))) return rc; *yd = v;
    if ((rc = up_rows(WS_H_X, x, 8, m, 0, m, p, st, &v))) return rc; *xd = (double *)v;
    if ((rc = up_rows(WS_H_MU, mu_hat, 8, n, lo, cnt, m, st, &v))) return rc; *mud = (double *)v;
    if (useWeights) { if ((rc = up_rows(WS_H_W, weights, 8, n, lo, cnt, m, st, &v))) return rc; *wd = (double *)v; }
    else *wd = nullptr;
    return DSQ_OK;
}

static int fit_disp_host_range(const DsqFitDispArgs *a, const DsqFitDispOut *o, size_t lo, size_t cnt, hipStream_t st,
                               const int32_t *cells, int ncell) {
    const size_t n = a->n;
    DsqFitDispArgs d = *a;
    DsqFitDispOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    int rc = disp_host_stage(n, lo, cnt, a->m, a->p, a->y, a->y_type, a->x, a->mu_hat, a->weights, a->useWeights, st,
                             &d.y, &d.x, &d.mu_hat, &d.weights);
    if (rc) return rc;
    void *v;
    if ((rc = capi_ws_get(WS_H_VEC, 2 * cnt * 8 + 8, &v))) return rc;
    double *vec = (double *)v;
    DSQ_HIP(hipMemcpyAsync(vec, a->log_alpha + lo, cnt * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + cnt, a->log_alpha_prior_mean + lo, cnt * 8, hipMemcpyHostToDevice, st));
    d.log_alpha = vec; d.log_alpha_prior_mean = vec + cnt;
    if ((rc = capi_ws_get(WS_H_OUTVEC, 8 * cnt * 8 + 8, &v))) return rc;
    double *ov = (double *)v;
    od.log_alpha = ov; od.last_change = ov + cnt; od.initial_lp = ov + 2 * cnt; od.initial_dlp = ov + 3 * cnt;
    od.last_lp = ov + 4 * cnt; od.last_dlp = ov + 5 * cnt; od.last_d2lp = ov + 6 * cnt;
    od.iter = (int32_t *)(ov + 7 * cnt); od.iter_accept = od.iter + cnt;
    rc = fit_disp_dev_locked(&d, &od, st);
    if (rc) return rc;
    double *const dst[7] = {o->log_alpha, o->last_change, o->initial_lp, o->initial_dlp, o->last_lp, o->last_dlp, o->last_d2lp};
    for (int k = 0; k < 7; k++) DSQ_HIP(hipMemcpyAsync(dst[k] + lo, ov + k * cnt, cnt * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->iter + lo, od.iter, cnt * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->iter_accept + lo, od.iter_accept, cnt * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

static int fit_disp_grid_host_range(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, size_t lo, size_t cnt,
                                    hipStream_t st, const int32_t *cells, int ncell) {
    const size_t n = a->n, ng = a->ngrid;
    DsqFitDispGridArgs d = *a;
    DsqFitDispGridOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    int rc = disp_host_stage(n, lo, cnt, a->m, a->p, a->y, a->y_type, a->x, a->mu_hat, a->weights, a->useWeights, st,
                             &d.y, &d.x, &d.mu_hat, &d.weights);
    if (rc) return rc;
    void *v;
    if ((rc = capi_ws_get(WS_H_VEC, (cnt + ng) * 8, &v))) return rc;
    double *vec = (double *)v;
    DSQ_HIP(hipMemcpyAsync(vec, a->log_alpha_prior_mean + lo, cnt * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + cnt, a->disp_grid, ng * 8, hipMemcpyHostToDevice, st));
    d.log_alpha_prior_mean = vec; d.disp_grid = vec + cnt;
    if ((rc = capi_ws_get(WS_H_OUTVEC, cnt * 8 + 8, &v))) return rc;
    od.log_alpha = (double *)v;
    rc = fit_disp_grid_dev_locked(&d, &od, st);
    if (rc) return rc;
    DSQ_HIP(hipMemcpyAsync(o->log_alpha + lo, od.log_alpha, cnt * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

// ---- worker threads: one per (device, lane); each owns a stream and, latched afresh for every job, that stream's context ----
struct HostWorker {
    int dev = 0;
    hipStream_t st = nullptr;
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false;
    int rc = 0;
    char err[512] = "";
    void loop() {
        (void)hipSetDevice(dev);
        (void)hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (;;) {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return has_job; });
            std::function<int()> j = std::move(job);
            has_job = false;
            lk.unlock();
            capi_latch_stream(st);
            int r = j();
            lk.lock();
            rc = r;
            snprintf(err, sizeof err, "%s", g_err);
            done = true;
            cv.notify_all();
        }
    }
};
static std::vector<HostWorker *> g_workers;      // grown under g_mu; worker k serves device k % ndev

static HostWorker *host_worker(int k, int ndev) {
    while ((int)g_workers.size() <= k) {
        HostWorker *w = new HostWorker();
        w->dev = (int)g_workers.size() % ndev;
        w->th = std::thread([w] { w->loop(); });
        w->th.detach();
        g_workers.push_back(w);
    }
    return g_workers[k];
}

// number of gene ranges of a host-pointer call over n genes, and the devices they go to
static void host_plan(size_t n, int *nshards, int *ndev) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 1) cnt = 1;
    const int cap = env_int("DSQ_HOST_DEVICES", 0);
    if (cap > 0 && cap < cnt) cnt = cap;
    int s = env_int("DSQ_HOST_SHARDS", 0);
    if (s <= 0) s = cnt;
    if ((size_t)s > n) s = (int)n;
    if (s < 1) s = 1;
    *nshards = s; *ndev = cnt;
}

// run f(lo, cnt, stream, range index, number of ranges) over the ranges of R/parallel.R:10; one range: on the caller's
// thread, device and null stream
template <class F>
static int host_sharded_ix(size_t row_lo, size_t n, F &&f0, int max_shards = 0) {
    int S, ndev;
    host_plan(n, &S, &ndev);
    if (max_shards > 0 && S > max_shards) S = max_shards;
    auto f = [&](size_t lo, size_t cnt, hipStream_t st, int k) { return f0(row_lo + lo, cnt, st, k, S < 1 ? 1 : S); };
    if (S <= 1) return f((size_t)0, n, (hipStream_t) nullptr, 0);
    std::vector<HostWorker *> ws(S);
    const size_t big = n / S + 1, nbig = n % S, small = n / S;      // the first n %% S ranges hold one gene more
    size_t lo = 0;
    for (int k = 0; k < S; k++) {
        const size_t cnt = (size_t)k < nbig ? big : small;
        HostWorker *w = ws[k] = host_worker(k, ndev);
        {
            std::lock_guard<std::mutex> lk(w->m);
            w->job = [&f, lo, cnt, w, k] { return f(lo, cnt, w->st, k); };
            w->has_job = true; w->done = false;
        }
        w->cv.notify_all();
        lo += cnt;
    }
    int rc = DSQ_OK;
    for (int k = 0; k < S; k++) {
        HostWorker *w = ws[k];
        std::unique_lock<std::mutex> lk(w->m);
        w->cv.wait(lk, [&] { return w->done; });
        if (w->rc && !rc) { rc = w->rc; snprintf(g_err, sizeof g_err, "%s", w->err); }
    }
    return rc;
}

template <class F>
static int host_sharded(size_t row_lo, size_t n, F &&f0) {
    return host_sharded_ix(row_lo, n, [&](size_t lo, size_t cnt, hipStream_t st, int, int) { return f0(lo, cnt, st); });
}
// (deseq_host.hip) the caller holds the library's call lock
int capi_host_sharded(size_t n, const std::function<int(size_t, size_t, hipStream_t, int, int)> &f, int max_shards) {
    return host_sharded_ix((size_t)0, n, f, max_shards);
}
int capi_host_shards(size_t n) {
    int S, ndev;
    host_plan(n, &S, &ndev);
    return S < 1 ? 1 : S;
}

static void host_cells(const double *x, int m, int p, const int32_t *given, int ngiven, std::vector<int32_t> *labels,
                       const int32_t **cells, int *ncell) {
    *cells = given; *ncell = ngiven;
    if (given) return;
    cells_of_host_design(x, m, p, labels);          // R hands over the design matrix itself: find its cells here
    if (!labels->empty()) { *cells = labels->data(); *ncell = 1 + *std::max_element(labels->begin(), labels->end()); }
}

}  // namespace dsq

using namespace dsq;

extern "C" {

int dsq_fit_beta(const DsqFitBetaArgs *a, const DsqFitBetaOut *o) { return dsq_fit_beta_rows(a, o, 0, a ? a->n : 0); }

int dsq_fit_beta_rows(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, int64_t row_lo, int64_t row_cnt) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->x || !a->nf || !a->alpha_hat || !a->contrast || !a->beta_mat || !a->lambda)
        return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (!o->beta_mat || !o->beta_var_mat || !o->iter || !o->contrast_num || !o->contrast_denom || !o->deviance)
        return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (row_lo < 0 || row_cnt < 0 || row_lo + row_cnt > a->n) return capi_fail(DSQ_ERR_ARG, "row range outside [0, n)");
    if (row_cnt == 0) return DSQ_OK;
    std::vector<int32_t> labels;
    const int32_t *cells; int ncell;
    host_cells(a->x, a->m, a->p, a->cell_of, a->ncell, &labels, &cells, &ncell);
    if (row_lo == 0) {          // the n x m results land in fresh pages: take the faults while the inputs go up (stage.hip)
        stage_prefault(o->hat_diagonals, (size_t)a->n * a->m * 8);
        stage_prefault(o->mu, (size_t)a->n * a->m * 8);
    }
    return host_sharded((size_t)row_lo, (size_t)row_cnt, [&](size_t lo, size_t cnt, hipStream_t st) {
        return fit_beta_host_range(a, o, lo, cnt, st, cells, ncell);
    });
}

int dsq_fit_disp(const DsqFitDispArgs *a, const DsqFitDispOut *o) { return dsq_fit_disp_rows(a, o, 0, a ? a->n : 0); }

int dsq_fit_disp_rows(const DsqFitDispArgs *a, const DsqFitDispOut *o, int64_t row_lo, int64_t row_cnt) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->x || !a->mu_hat || !a->log_alpha || !a->log_alpha_prior_mean)
        return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (!o->log_alpha || !o->iter || !o->iter_accept || !o->last_change || !o->initial_lp || !o->initial_dlp ||
        !o->last_lp || !o->last_dlp || !o->last_d2lp)
        return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (row_lo < 0 || row_cnt < 0 || row_lo + row_cnt > a->n) return capi_fail(DSQ_ERR_ARG, "row range outside [0, n)");
    if (row_cnt == 0) return DSQ_OK;
    std::vector<int32_t> labels;
    const int32_t *cells; int ncell;
    host_cells(a->x, a->m, a->p, a->cell_of, a->ncell, &labels, &cells, &ncell);
    return host_sharded((size_t)row_lo, (size_t)row_cnt, [&](size_t lo, size_t cnt, hipStream_t st) {
        return fit_disp_host_range(a, o, lo, cnt, st, cells, ncell);
    });
}

int dsq_fit_disp_grid(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o) { return dsq_fit_disp_grid_rows(a, o, 0, a ? a->n : 0); }

int dsq_fit_disp_grid_rows(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, int64_t row_lo, int64_t row_cnt) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1 || a->p < 1 || a->ngrid < 2) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->x || !a->mu_hat || !a->disp_grid || !a->log_alpha_prior_mean || !o->log_alpha)
        return capi_fail(DSQ_ERR_ARG, "NULL array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (int rc = capi_check_device()) return rc;
    if (row_lo < 0 || row_cnt < 0 || row_lo + row_cnt > a->n) return capi_fail(DSQ_ERR_ARG, "row range outside [0, n)");
    if (row_cnt == 0) return DSQ_OK;
    std::vector<int32_t> labels;
    const int32_t *cells; int ncell;
    host_cells(a->x, a->m, a->p, a->cell_of, a->ncell, &labels, &cells, &ncell);
    return host_sharded((size_t)row_lo, (size_t)row_cnt, [&](size_t lo, size_t cnt, hipStream_t st) {
        return fit_disp_grid_host_range(a, o, lo, cnt, st, cells, ncell);
    });
}

int dsq_parametric_dispersion_fit(const double *means, const double *disps, int64_t n, double *coefs, int32_t *status) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!means || !disps || !coefs || !status || n < 1) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    hipStream_t st = nullptr;
    void *v;
    int rc;
    if ((rc = capi_ws_get(WS_H_VEC, (2 * (size_t)n + 4) * 8, &v))) return rc;
    double *d = (double *)v;
    DSQ_HIP(hipMemcpyAsync(d, means, n * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(d + n, disps, n * 8, hipMemcpyHostToDevice, st));
    void *tws;
    if ((rc = capi_ws_get(WS_TREND, trend_fit_workspace_bytes(), &tws))) return rc;
    DSQ_HIP(launch_trend_fit(d, d + n, (long)n, d + 2 * n, (int32_t *)(d + 2 * n + 2), tws, st));
    DSQ_HIP(hipMemcpyAsync(coefs, d + 2 * n, 16, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(status, d + 2 * n + 2, 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_prefit_moments(const DsqPrefitArgs *a, const DsqPrefitOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 2 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->q || !a->a || !a->r) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (!o->baseMean || !o->baseVar || !o->allZero || !o->roughDisp || !o->beta_init) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m, p = a->p;
    DsqPrefitArgs d = *a;
    DsqPrefitOut od = *o;
    void *v;
    int rc;
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_NF, a->nf, (a->nf_is_vector ? m : n * m) * 8, st, &v))) return rc; d.nf = (double *)v;
    if (a->useWeights) { if ((rc = up(WS_H_W, a->weights, n * m * 8, st, &v))) return rc; d.weights = (double *)v; }
    else d.weights = nullptr;
    size_t tot = 2 * m * p + p * p;
    if ((rc = capi_ws_get(WS_H_VEC, tot * 8, &v))) return rc;
    double *vec = (double *)v;
    DSQ_HIP(hipMemcpyAsync(vec, a->q, m * p * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + m * p, a->a, m * p * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + 2 * m * p, a->r, p * p * 8, hipMemcpyHostToDevice, st));
    d.q = vec; d.a = vec + m * p; d.r = vec + 2 * m * p;
    if ((rc = capi_ws_get(WS_H_OUTVEC, (4 * n + n * p) * 8, &v))) return rc;
    double *ov = (double *)v;
    od.baseMean = ov; od.baseVar = ov + n; od.roughDisp = ov + 2 * n; od.allZero = (int32_t *)(ov + 3 * n);
    od.beta_init = ov + 4 * n;
    rc = prefit_dev_locked(&d, &od, st);
    if (rc) return rc;
    DSQ_HIP(hipMemcpyAsync(o->baseMean, od.baseMean, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->baseVar, od.baseVar, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->roughDisp, od.roughDisp, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->allZero, od.allZero, n * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->beta_init, od.beta_init, n * p * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_linear_mu(const DsqPrefitArgs *a, double mu_floor, double *mu) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !mu) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->q || !a->a) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m, p = a->p;
    DsqPrefitArgs d = *a;
    void *v;
    int rc;
    stage_prefault(mu, n * m * 8);
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_NF, a->nf, (a->nf_is_vector ? m : n * m) * 8, st, &v))) return rc; d.nf = (double *)v;
    if ((rc = capi_ws_get(WS_H_VEC, 2 * m * p * 8, &v))) return rc;
    double *vec = (double *)v;
    DSQ_HIP(hipMemcpyAsync(vec, a->q, m * p * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + m * p, a->a, m * p * 8, hipMemcpyHostToDevice, st));
    d.q = vec; d.a = vec + m * p;
    if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &v))) return rc;
    rc = linear_mu_dev_locked(&d, mu_floor, (double *)v, st);
    if (rc) return rc;
    return down(mu, v, n * m * 8, st);
}

int dsq_nbinom_loglike(const DsqLogLikeArgs *a, double *loglike) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !loglike) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->mu || !a->disp) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    DsqLogLikeArgs d = *a;
    void *v;
    int rc;
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_MU, a->mu, n * m * 8, st, &v))) return rc; d.mu = (double *)v;
    if (a->useWeights) { if ((rc = up(WS_H_W, a->weights, n * m * 8, st, &v))) return rc; d.weights = (double *)v; }
    else d.weights = nullptr;
    if ((rc = up(WS_H_VEC, a->disp, n * 8, st, &v))) return rc; d.disp = (double *)v;
    if ((rc = capi_ws_get(WS_H_OUTVEC, n * 8, &v))) return rc;
    rc = loglike_dev_locked(&d, (double *)v, st);
    if (rc) return rc;
    DSQ_HIP(hipMemcpyAsync(loglike, v, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_intercept_fit(const DsqInterceptArgs *a, const DsqInterceptOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->alpha) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (!o->beta_log2 || !o->betaSE) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    DsqInterceptArgs d = *a;
    DsqInterceptOut od = *o;
    void *v;
    int rc;
    stage_prefault(o->mu, n * m * 8);
    stage_prefault(o->hat, n * m * 8);
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_NF, a->nf, (a->nf_is_vector ? m : n * m) * 8, st, &v))) return rc; d.nf = (double *)v;
    if (a->useWeights) { if ((rc = up(WS_H_W, a->weights, n * m * 8, st, &v))) return rc; d.weights = (double *)v; }
    else d.weights = nullptr;
    if ((rc = up(WS_H_VEC, a->alpha, n * 8, st, &v))) return rc; d.alpha = (double *)v;
    if ((rc = capi_ws_get(WS_H_OUTVEC, 2 * n * 8, &v))) return rc;
    od.beta_log2 = (double *)v; od.betaSE = (double *)v + n;
    od.mu = od.hat = nullptr;
    if (o->mu) { if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &v))) return rc; od.mu = (double *)v; }
    if (o->hat) { if ((rc = capi_ws_get(WS_H_OUTMAT2, n * m * 8, &v))) return rc; od.hat = (double *)v; }
    rc = intercept_dev_locked(&d, &od, st);
    if (rc) return rc;
    DSQ_HIP(hipMemcpyAsync(o->beta_log2, od.beta_log2, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->betaSE, od.betaSE, n * 8, hipMemcpyDeviceToHost, st));
    if (o->mu && (rc = down(o->mu, od.mu, n * m * 8, st))) return rc;
    if (o->hat && (rc = down(o->hat, od.hat, n * m * 8, st))) return rc;
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_optim_rows(const DsqOptimArgs *a, const DsqOptimOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1 || a->p < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (a->p > DSQ_P_WIDE) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_optim_rows: p=%d > %d design columns", a->p, DSQ_P_WIDE);
    if (!a->y || !a->x || !a->nf || !a->alpha_hat || !a->lambda || !a->beta_start) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (a->useWeights && !a->weights) return capi_fail(DSQ_ERR_ARG, "useWeights set but weights is NULL");
    if (!o->beta || !o->betaSE || !o->conv || !o->mu || !o->logLike) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    // wide designs (see above): the kernel runs at the padded width pk -- zero design columns, ridge 1, start value 0
    const size_t n = a->n, m = a->m, p = a->p, pk = is_wide(a->p) ? wide_width(a->p) : a->p;
    void *v;
    int rc;
    OptimKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = (int)pk; kp.minmu = a->minmu;
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc;
    bool ycheck = false;
    long ld = 0;
    rc = prep_counts(v, a->y_type, DSQ_LAYOUT_R, 0, a->n, a->m, st, &kp.y, &ld, &ycheck);
    if (rc) return rc;
    kp.ld = ld;
    if (a->nf_is_vector) { if ((rc = up(WS_H_NF, a->nf, m * 8, st, &v))) return rc; kp.nf = (double *)v; kp.nf_is_vector = 1; }
    else {
        if ((rc = up(WS_H_NF, a->nf, n * m * 8, st, &v))) return rc;
        if ((rc = prep_matrix((double *)v, DSQ_LAYOUT_R, 0, a->n, a->m, WS_NF, st, &kp.nf, ld))) return rc;
    }
    if (a->useWeights) {
        if ((rc = up(WS_H_W, a->weights, n * m * 8, st, &v))) return rc;
        if ((rc = prep_matrix((double *)v, DSQ_LAYOUT_R, 0, a->n, a->m, WS_W, st, &kp.weights, ld))) return rc;
        kp.useWeights = 1;
    }
    // x | alpha | lambda (natural-log scale) | beta_start
    const size_t off_x = 0, off_al = m * pk, off_lam = off_al + n, off_b = off_lam + pk, tot = off_b + n * pk;
    if ((rc = capi_ws_get(WS_H_VEC, tot * 8, &v))) return rc;
    double *vec = (double *)v;
    static thread_local double lamnat[DSQ_P_WIDE];
    const double ln2 = 0.6931471805599453;
    for (size_t c = 0; c < pk; c++) lamnat[c] = c < p ? a->lambda[c] / (ln2 * ln2) : 1.0;
    if (pk != p) DSQ_HIP(hipMemsetAsync(vec, 0, tot * 8, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_x, a->x, m * p * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_al, a->alpha_hat, n * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_lam, lamnat, pk * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(vec + off_b, a->beta_start, n * p * 8, hipMemcpyHostToDevice, st));
    kp.x = vec + off_x; kp.alpha_hat = vec + off_al; kp.lamnat = vec + off_lam; kp.beta_start = vec + off_b;
    // outputs: beta | betaSE | loglike | conv ; mu (gene-major, then R layout)
    if ((rc = capi_ws_get(WS_H_OUTVEC, (2 * n * pk + 2 * n) * 8, &v))) return rc;
    double *ov = (double *)v;
    kp.beta = ov; kp.betaSE = ov + n * pk; kp.loglike = ov + 2 * n * pk; kp.conv = (int32_t *)(ov + 2 * n * pk + n);
    void *mu_gm, *mu_r;
    if ((rc = capi_ws_get(WS_MUOUT, n * (size_t)ld * 8, &mu_gm))) return rc;
    if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &mu_r))) return rc;
    kp.mu_out = (double *)mu_gm;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(dispatch_optim_rows((int)pk, kp, st, &ok));
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "no kernel for p=%d", a->p);
    DSQ_HIP(launch_transpose_gm_to_r_f64(kp.mu_out, (double *)mu_r, a->n, a->m, ld, st));
    DSQ_HIP(hipMemcpyAsync(o->beta, kp.beta, n * p * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->betaSE, kp.betaSE, n * p * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->logLike, kp.loglike, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->conv, kp.conv, n * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->mu, mu_r, n * m * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return finish_ycheck(ycheck, st);
}

int dsq_cooks_distance(const DsqCooksArgs *a, const DsqCooksOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->mu || !a->H || !a->cell_of) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (!o->cooks || !o->maxCooks) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    DsqCooksArgs d = *a;
    DsqCooksOut od = *o;
    void *v;
    int rc;
    stage_prefault(o->cooks, n * m * 8);
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_NF, a->nf, (a->nf_is_vector ? m : n * m) * 8, st, &v))) return rc; d.nf = (double *)v;
    if ((rc = up(WS_H_MU, a->mu, n * m * 8, st, &v))) return rc; d.mu = (double *)v;
    if ((rc = up(WS_H_W, a->H, n * m * 8, st, &v))) return rc; d.H = (double *)v;
    if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &v))) return rc; od.cooks = (double *)v;
    if ((rc = capi_ws_get(WS_H_OUTVEC, 2 * n * 8, &v))) return rc;
    od.maxCooks = (double *)v; od.robustDisp = (double *)v + n;
    rc = cooks_dev_locked(&d, &od, st);
    if (rc) return rc;
    if ((rc = down(o->cooks, od.cooks, n * m * 8, st))) return rc;
    DSQ_HIP(hipMemcpyAsync(o->maxCooks, od.maxCooks, n * 8, hipMemcpyDeviceToHost, st));
    if (o->robustDisp) DSQ_HIP(hipMemcpyAsync(o->robustDisp, od.robustDisp, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_replace_outliers(const DsqReplaceArgs *a, const DsqReplaceOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (a->n < 0 || a->m < 1) return capi_fail(DSQ_ERR_ARG, "bad dimensions");
    if (!a->y || !a->nf || !a->cooks || !a->replaceable) return capi_fail(DSQ_ERR_ARG, "NULL input array");
    if (!o->newCounts || !o->replace) return capi_fail(DSQ_ERR_ARG, "NULL output array");
    if (int rc = capi_check_device()) return rc;
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    DsqReplaceArgs d = *a;
    DsqReplaceOut od = *o;
    void *v;
    int rc;
    stage_prefault(o->newCounts, n * m * 4);
    if ((rc = up(WS_H_Y, a->y, n * m * (a->y_type == DSQ_Y_INT32 ? 4 : 8), st, &v))) return rc; d.y = v;
    if ((rc = up(WS_H_NF, a->nf, (a->nf_is_vector ? m : n * m) * 8, st, &v))) return rc; d.nf = (double *)v;
    if ((rc = up(WS_H_MU, a->cooks, n * m * 8, st, &v))) return rc; d.cooks = (double *)v;
    if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 4, &v))) return rc; od.newCounts = (int32_t *)v;
    if ((rc = capi_ws_get(WS_H_OUTVEC, n * 4, &v))) return rc; od.replace = (int32_t *)v;
    rc = replace_dev_locked(&d, &od, st);
    if (rc) return rc;
    if ((rc = down(o->newCounts, od.newCounts, n * m * 4, st))) return rc;
    DSQ_HIP(hipMemcpyAsync(o->replace, od.replace, n * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_test_math(int op, const double *a, const double *b, const double *c, double *out, int64_t n) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (!a || !out || n < 0 || ((op == 7 || op == 8) && !b) || (op == 8 && !c)) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    if (int rc = capi_check_device()) return rc;
    if (n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    void *v;
    int rc;
    if ((rc = capi_ws_get(WS_H_VEC, 4 * (size_t)n * 8, &v))) return rc;
    double *d = (double *)v;
    DSQ_HIP(hipMemcpyAsync(d, a, n * 8, hipMemcpyHostToDevice, st));
    if (b) DSQ_HIP(hipMemcpyAsync(d + n, b, n * 8, hipMemcpyHostToDevice, st));
    if (c) DSQ_HIP(hipMemcpyAsync(d + 2 * n, c, n * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(launch_test_math(op, d, d + n, d + 2 * n, d + 3 * n, n, st));
    DSQ_HIP(hipMemcpyAsync(out, d + 3 * n, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

}  // extern "C"

extern "C" {

int dsq_size_factors(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    if (int rc = size_factors_check(a, o)) return rc;
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (int rc = capi_check_device()) return rc;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    const size_t ye = a->y_type == DSQ_Y_INT32 ? 4 : 8;
    DsqSizeFactorArgs d = *a;
    DsqSizeFactorOut od = *o;
    void *v, *g;
    int rc;
    // counts and normMatrix: up in R layout, turned gene-major on the device (rows of 64 consecutive samples)
    if ((rc = up(WS_H_Y, a->y, n * m * ye, st, &v))) return rc;
    if ((rc = capi_ws_get(WS_Y, n * ld * ye, &g))) return rc;
    if (ye == 4) DSQ_HIP(launch_transpose_r_to_gm_i32((const int32_t *)v, (int32_t *)g, a->n, a->m, ld, st));
    else DSQ_HIP(launch_transpose_r_to_gm_f64((const double *)v, (double *)g, a->n, a->m, ld, st));
    d.y = g; d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    double *nf_gm = nullptr;
    if (a->normMatrix) {
        if ((rc = up(WS_H_NF, a->normMatrix, n * m * 8, st, &v))) return rc;
        if ((rc = capi_ws_get(WS_NF, n * ld * 8, &g))) return rc;
        DSQ_HIP(launch_transpose_r_to_gm_f64((const double *)v, (double *)g, a->n, a->m, ld, st));
        d.normMatrix = (const double *)g;
        if ((rc = capi_ws_get(WS_MUOUT, n * ld * 8, &g))) return rc;
        nf_gm = (double *)g;
        od.normalizationFactors = nf_gm;
    }
    // geoMeans (n f64) | control (n i32)
    if ((rc = capi_ws_get(WS_H_VEC, n * 12 + 8, &v))) return rc;
    if (a->geoMeans) { DSQ_HIP(hipMemcpyAsync(v, a->geoMeans, n * 8, hipMemcpyHostToDevice, st)); d.geoMeans = (const double *)v; }
    if (a->control) {
        DSQ_HIP(hipMemcpyAsync((char *)v + n * 8, a->control, n * 4, hipMemcpyHostToDevice, st));
        d.control = (const int32_t *)((char *)v + n * 8);
    }
    const size_t wsb = size_factors_workspace_bytes(a->n, a->m);
    if ((rc = capi_ws_get(WS_SCRATCH, wsb, &v))) return rc;
    d.workspace = v; d.workspace_bytes = (int64_t)wsb;
    // sizeFactors (m f64) | loggeomeans (n f64) | status
    if ((rc = capi_ws_get(WS_H_OUTVEC, (m + n + 1) * 8, &v))) return rc;
    double *ov = (double *)v;
    od.sizeFactors = ov; od.loggeomeans = ov + m; od.status = (int32_t *)(ov + m + n);
    if ((rc = size_factors_dev_locked(&d, &od, st))) return rc;
    DSQ_HIP(hipMemcpyAsync(o->sizeFactors, od.sizeFactors, m * 8, hipMemcpyDeviceToHost, st));
    if (o->loggeomeans) DSQ_HIP(hipMemcpyAsync(o->loggeomeans, od.loggeomeans, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->status, od.status, 4, hipMemcpyDeviceToHost, st));
    if (nf_gm) {
        if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &v))) return rc;
        DSQ_HIP(launch_transpose_gm_to_r_f64(nf_gm, (double *)v, a->n, a->m, ld, st));
        if ((rc = down(o->normalizationFactors, v, n * m * 8, st))) return rc;
    }
    DSQ_HIP(hipStreamSynchronize(st));
    if (*o->status == 1)
        return capi_fail(DSQ_ERR_FIT, "every gene contains at least one zero, cannot compute log geometric means");
    return DSQ_OK;
}

int dsq_vst(const DsqVstArgs *a, const DsqVstOut *o) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    const bool transform = o && o->out, stats = o && (o->rowMean || o->rowMax);
    if (o && !transform && !stats) return capi_fail(DSQ_ERR_ARG, "neither an output matrix nor row statistics asked for");
    if (int rc = vst_check(a, o, transform, stats)) return rc;
    if (a->layout != DSQ_LAYOUT_R) return capi_fail(DSQ_ERR_ARG, "host entry points take R layout only");
    if (int rc = capi_check_device()) return rc;
    hipStream_t st = nullptr;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    const size_t ye = a->y_type == DSQ_Y_INT32 ? 4 : 8;
    DsqVstArgs d = *a;
    DsqVstOut od = *o;
    void *v, *g;
    int rc;
    if (transform) stage_prefault(o->out, n * m * 8);
    // counts and a normalization-factor matrix: up in R layout, turned gene-major on the device
    if ((rc = up(WS_H_Y, a->y, n * m * ye, st, &v))) return rc;
    if ((rc = capi_ws_get(WS_Y, n * ld * ye, &g))) return rc;
    if (ye == 4) DSQ_HIP(launch_transpose_r_to_gm_i32((const int32_t *)v, (int32_t *)g, a->n, a->m, ld, st));
    else DSQ_HIP(launch_transpose_r_to_gm_f64((const double *)v, (double *)g, a->n, a->m, ld, st));
    d.y = g; d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    if (a->nf_is_vector) {
        if ((rc = up(WS_H_NF, a->nf, m * 8, st, &v))) return rc;
        d.nf = (const double *)v;
    } else {
        if ((rc = up(WS_H_NF, a->nf, n * m * 8, st, &v))) return rc;
        if ((rc = capi_ws_get(WS_NF, n * ld * 8, &g))) return rc;
        DSQ_HIP(launch_transpose_r_to_gm_f64((const double *)v, (double *)g, a->n, a->m, ld, st));
        d.nf = (const double *)g;
    }
    // rowMean (n f64) | rowMax (n f64) | the bad-count flag
    if ((rc = capi_ws_get(WS_H_OUTVEC, (2 * n + 1) * 8, &v))) return rc;
    double *ov = (double *)v;
    od.rowMean = ov; od.rowMax = ov + n; od.bad = (int32_t *)(ov + 2 * n);
    DSQ_HIP(hipMemsetAsync(od.bad, 0, 8, st));
    double *out_gm = nullptr;
    if (transform) {
        if ((rc = capi_ws_get(WS_MUOUT, n * ld * 8, &g))) return rc;
        od.out = out_gm = (double *)g;
    }
    if ((rc = vst_dev_locked(&d, &od, transform, stats, st))) return rc;
    int32_t bad = 0;
    DSQ_HIP(hipMemcpyAsync(&bad, od.bad, 4, hipMemcpyDeviceToHost, st));
    if (o->rowMean) DSQ_HIP(hipMemcpyAsync(o->rowMean, od.rowMean, n * 8, hipMemcpyDeviceToHost, st));
    if (o->rowMax) DSQ_HIP(hipMemcpyAsync(o->rowMax, od.rowMax, n * 8, hipMemcpyDeviceToHost, st));
    if (out_gm) {
        if ((rc = capi_ws_get(WS_H_OUTMAT, n * m * 8, &v))) return rc;
        DSQ_HIP(launch_transpose_gm_to_r_f64(out_gm, (double *)v, a->n, a->m, ld, st));
        if ((rc = down(o->out, v, n * m * 8, st))) return rc;
    }
    DSQ_HIP(hipStreamSynchronize(st));
    if (bad) return capi_fail(DSQ_ERR_VALUE, "count matrix holds negative, non-finite or non-integer values");
    return DSQ_OK;
}

}  // extern "C"
