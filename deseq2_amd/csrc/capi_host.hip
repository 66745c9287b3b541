// capi_host.hip -- the host-pointer entry points of the C ABI (what r_shim.c binds: R memory in, R memory out,
// synchronous); see capi.hip for the three files of the host side.
//
// Every entry point reads the same way: the call's checks (check_<call> of capi.hip, plus "R layout only" and the row
// range), the list of its inputs, the list of its outputs, the device-pointer body of capi.hip, finish().  The lists are
// calls on a Stage (below), which owns the workspace slots, the offsets inside the two packed buffers and the downloads.
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

// ---- the traffic of one host-pointer call, or of one gene range [lo, lo + cnt) of its n genes ---------------------------
// Three mechanisms, and every array keeps its own:
//   n x m matrices     a slot each, through the pinned chunks of stage.hip (stage_h2d up, stage_d2h down);
//   vectors, n x p     consecutive pieces of ONE packed buffer per direction (WS_H_VEC up, WS_H_OUTVEC down), one plain
//                      async copy each;
//   rows of an n x p   (beta_mat of a gene range) a 2-D copy up, stage_d2h down.
// A `field` is the address of the pointer member of the device-side argument block that is to receive the device address.
// Inputs go up in the order listed (the packed ones when pack_in() is reached); outputs are listed with their host
// destination and come down, in the order listed, in flush() / finish().  An output whose host pointer is NULL is not
// downloaded (a matrix not even given a slot: its field becomes NULL).
struct Stage {
    enum { kMaxPieces = 12 };
    enum How { PLAIN, ROWS };
    struct Piece { void *field; char *host; char *dev; size_t bytes, reserve, elem, cols; How how; };
    hipStream_t st;
    size_t n, lo, cnt;
    Piece in[kMaxPieces], out[kMaxPieces];
    int nin = 0, nout = 0;
    bool full = false;              // a list outgrew kMaxPieces: pack_in / pack_out / flush refuse

    Stage(hipStream_t s, size_t n_) : st(s), n(n_), lo(0), cnt(n_) {}
    Stage(hipStream_t s, size_t n_, size_t lo_, size_t cnt_) : st(s), n(n_), lo(lo_), cnt(cnt_) {}
    static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }
    void add(Piece *list, int *k, const Piece &p) { if (*k < kMaxPieces) list[(*k)++] = p; else full = true; }
    int refuse_full() const { return full ? capi_fail(DSQ_ERR_ARG, "Stage: more than %d pieces listed", (int)kMaxPieces) : DSQ_OK; }

    // -- matrices: rows [r0, r0 + r) of a column-major rows x cols host matrix into a slot
    template <class T> int up(int slot, T **field, const void *host, size_t elem, size_t rows, size_t r0, size_t r, size_t cols) {
        void *dev;
        const size_t bytes = r * cols * elem;
        if (int rc = capi_ws_get(slot, bytes ? bytes : 8, &dev)) return rc;
        *field = (T *)dev;
        return stage_h2d(dev, host, elem, rows, r0, r, cols, st);
    }
    template <class T> int genes_up(int slot, T **field, const void *host, size_t elem, size_t cols) { return up(slot, field, host, elem, n, lo, cnt, cols); }
    template <class T> int table_up(int slot, T **field, const void *host, size_t elem, size_t rows, size_t cols = 1) {
        return up(slot, field, host, elem, rows, 0, rows, cols);
    }
    template <class T> int counts_up(T **field, const void *y, int y_type, size_t m) { return genes_up(WS_H_Y, field, y, y_type == DSQ_Y_INT32 ? 4 : 8, m); }
    int nf_up(const double **field, const double *nf, int is_vector, size_t m) {
        return is_vector ? table_up(WS_H_NF, field, nf, 8, m) : genes_up(WS_H_NF, field, nf, 8, m);
    }
    int weights_up(const double **field, const double *w, int use, size_t m) {
        *field = nullptr;
        return use ? genes_up(WS_H_W, field, w, 8, m) : DSQ_OK;
    }

    // -- packed inputs: a fixed piece (NULL host: room kept, nothing copied), the call's genes of an n-vector, of an n x cols matrix
    template <class T> void vec(T **field, const void *host, size_t bytes, size_t reserve = 0) {
        add(in, &nin, {field, (char *)host, nullptr, bytes, pad8(reserve ? reserve : bytes), 0, 0, PLAIN});
    }
    void gene_vec(const double **field, const double *host) { vec(field, host + lo, cnt * 8); }
    void gene_cols(const double **field, const double *host, size_t cols) {
        add(in, &nin, {field, (char *)host, nullptr, cnt * cols * 8, cnt * cols * 8, 8, cols, ROWS});
    }
    int pack_in(bool zero_first = false) {
        if (int rc = refuse_full()) return rc;
        size_t total = 0;
        for (int k = 0; k < nin; k++) total += in[k].reserve;
        void *v;
        if (int rc = capi_ws_get(WS_H_VEC, total ? total : 8, &v)) return rc;
        if (zero_first) DSQ_HIP(hipMemsetAsync(v, 0, total, st));
        char *dev = (char *)v;
        for (int k = 0; k < nin; dev += in[k++].reserve) {
            const Piece &p = in[k];
            if (!p.host) continue;
            memcpy(p.field, &dev, sizeof dev);
            if (p.how == PLAIN || cnt == n) DSQ_HIP(hipMemcpyAsync(dev, p.host, p.bytes, hipMemcpyHostToDevice, st));
            else DSQ_HIP(hipMemcpy2DAsync(dev, cnt * 8, p.host + lo * 8, n * 8, cnt * 8, p.cols, hipMemcpyHostToDevice, st));
        }
        nin = 0;
        return DSQ_OK;
    }

    // -- outputs: packed pieces get their places in WS_H_OUTVEC in pack_out(); a matrix gets a slot of its own at once
    template <class T> void out_vec(T **field, void *host, size_t bytes, size_t reserve = 0) {
        add(out, &nout, {field, (char *)host, nullptr, bytes, pad8(reserve ? reserve : bytes), 0, 0, PLAIN});
    }
    template <class T> void out_gene_vec(T **field, T *host) { out_vec(field, host ? host + lo : nullptr, cnt * sizeof(T)); }
    void out_gene_cols(double **field, double *host, size_t cols) {
        add(out, &nout, {field, (char *)host, nullptr, cnt * cols * 8, cnt * cols * 8, 8, cols, ROWS});
    }
    int pack_out() {
        if (int rc = refuse_full()) return rc;
        size_t total = 0;
        for (int k = 0; k < nout; k++) if (!out[k].dev) total += out[k].reserve;
        void *v;
        if (int rc = capi_ws_get(WS_H_OUTVEC, total ? total : 8, &v)) return rc;
        char *dev = (char *)v;
        for (int k = 0; k < nout; k++) {
            if (out[k].dev) continue;
            out[k].dev = dev;
            memcpy(out[k].field, &dev, sizeof dev);
            dev += out[k].reserve;
        }
        return DSQ_OK;
    }
    // an n x cols output matrix of the call's genes (not asked for: no slot, *field NULL)
    template <class T> int out_mat(int slot, T **field, T *host, size_t cols, How how = ROWS) {
        void *dev = nullptr;
        if (host) {
            if (int rc = capi_ws_get(slot, cnt * cols * sizeof(T), &dev)) return rc;
            add(out, &nout, {field, (char *)host, (char *)dev, cnt * cols * sizeof(T), 0, sizeof(T), cols, how});
        }
        *field = (T *)dev;
        return DSQ_OK;
    }
    // the downloads listed so far, in the order listed; finish(): and the one synchronisation of the call
    int flush() {
        if (int rc = refuse_full()) return rc;
        for (int k = 0; k < nout; k++) {
            const Piece &p = out[k];
            if (!p.host) continue;
            if (p.how == PLAIN) DSQ_HIP(hipMemcpyAsync(p.host, p.dev, p.bytes, hipMemcpyDeviceToHost, st));
            else if (int rc = stage_d2h(p.host, p.dev, p.elem, n, lo, cnt, p.cols, st)) return rc;
        }
        nout = 0;
        return DSQ_OK;
    }
    int finish() {
        if (int rc = flush()) return rc;
        DSQ_HIP(hipStreamSynchronize(st));
        return DSQ_OK;
    }
};
#define DSQ_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

// what every single-range host entry holds while it runs: the call lock, the context of the null stream
struct HostCall {
    std::lock_guard<std::mutex> lk{g_mu};
    WsScope ws{nullptr};
    hipStream_t st = nullptr;
};
// after the call's check: R layout only, then the device
static int host_ready(int check_rc, int layout) {
    if (check_rc) return check_rc;
    if (int rc = check_host_layout(layout)) return rc;
    return capi_check_device();
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

static int fit_beta_host_range(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, size_t lo, size_t cnt, hipStream_t st,
                               const int32_t *cells, int ncell) {
    const size_t m = a->m, p = a->p;
    DsqFitBetaArgs d = *a;
    DsqFitBetaOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    Stage s(st, a->n, lo, cnt);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    s.vec(&d.x, a->x, m * p * 8);
    s.gene_vec(&d.alpha_hat, a->alpha_hat);
    s.vec(&d.contrast, a->contrast, p * 8);
    s.gene_cols(&d.beta_mat, a->beta_mat, p);
    s.vec(&d.lambda, a->lambda, p * 8);
    DSQ_TRY(s.pack_in());
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    DSQ_TRY(s.weights_up(&d.weights, a->weights, a->useWeights, m));
    s.out_gene_cols(&od.beta_mat, o->beta_mat, p);
    s.out_gene_cols(&od.beta_var_mat, o->beta_var_mat, p);
    s.out_gene_vec(&od.iter, o->iter);
    s.out_gene_vec(&od.contrast_num, o->contrast_num);
    s.out_gene_vec(&od.contrast_denom, o->contrast_denom);
    s.out_gene_vec(&od.deviance, o->deviance);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &od.hat_diagonals, o->hat_diagonals, m));
    DSQ_TRY(s.out_mat(WS_H_OUTMAT2, &od.mu, o->mu, m));
    DSQ_TRY(fit_beta_dev_locked(&d, &od, st));
    return s.finish();
}

// what fitDisp and fitDispGrid stage alike: counts, design, mu-hat, weights
template <class A>
static int disp_inputs_up(Stage &s, const A *a, A *d) {
    const size_t m = a->m, p = a->p;
    DSQ_TRY(s.counts_up(&d->y, a->y, a->y_type, m));
    DSQ_TRY(s.table_up(WS_H_X, &d->x, a->x, 8, m, p));
    DSQ_TRY(s.genes_up(WS_H_MU, &d->mu_hat, a->mu_hat, 8, m));
    return s.weights_up(&d->weights, a->weights, a->useWeights, m);
}

static int fit_disp_host_range(const DsqFitDispArgs *a, const DsqFitDispOut *o, size_t lo, size_t cnt, hipStream_t st,
                               const int32_t *cells, int ncell) {
    DsqFitDispArgs d = *a;
    DsqFitDispOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    Stage s(st, a->n, lo, cnt);
    DSQ_TRY(disp_inputs_up(s, a, &d));
    s.gene_vec(&d.log_alpha, a->log_alpha);
    s.gene_vec(&d.log_alpha_prior_mean, a->log_alpha_prior_mean);
    DSQ_TRY(s.pack_in());
    s.out_gene_vec(&od.log_alpha, o->log_alpha);
    s.out_gene_vec(&od.last_change, o->last_change);
    s.out_gene_vec(&od.initial_lp, o->initial_lp);
    s.out_gene_vec(&od.initial_dlp, o->initial_dlp);
    s.out_gene_vec(&od.last_lp, o->last_lp);
    s.out_gene_vec(&od.last_dlp, o->last_dlp);
    s.out_gene_vec(&od.last_d2lp, o->last_d2lp);
    s.out_gene_vec(&od.iter, o->iter);
    s.out_gene_vec(&od.iter_accept, o->iter_accept);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(fit_disp_dev_locked(&d, &od, st));
    return s.finish();
}

static int fit_disp_grid_host_range(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, size_t lo, size_t cnt,
                                    hipStream_t st, const int32_t *cells, int ncell) {
    DsqFitDispGridArgs d = *a;
    DsqFitDispGridOut od = *o;
    d.n = (int32_t)cnt;
    d.cell_of = cells; d.ncell = ncell;
    Stage s(st, a->n, lo, cnt);
    DSQ_TRY(disp_inputs_up(s, a, &d));
    s.gene_vec(&d.log_alpha_prior_mean, a->log_alpha_prior_mean);
    s.vec(&d.disp_grid, a->disp_grid, (size_t)a->ngrid * 8);
    DSQ_TRY(s.pack_in());
    s.out_gene_vec(&od.log_alpha, o->log_alpha);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(fit_disp_grid_dev_locked(&d, &od, st));
    return s.finish();
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

// fitBeta / fitDisp / fitDispGrid over the gene rows [row_lo, row_lo + row_cnt): the range is cut further, one piece per
// device (host_sharded); `announce` runs once before the pieces start
template <class A, class O, class Check, class Range, class Announce>
static int fit_rows(const A *a, const O *o, int64_t row_lo, int64_t row_cnt, Check check, Range range, Announce announce) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    DSQ_TRY(host_ready(check(a, o), a ? a->layout : 0));
    if (row_lo < 0 || row_cnt < 0 || row_lo + row_cnt > a->n)
        return capi_fail(DSQ_ERR_ARG, "row range [%lld, %lld) outside [0, %d)", (long long)row_lo, (long long)(row_lo + row_cnt), a->n);
    if (row_cnt == 0) return DSQ_OK;
    std::vector<int32_t> labels;
    const int32_t *cells; int ncell;
    host_cells(a->x, a->m, a->p, a->cell_of, a->ncell, &labels, &cells, &ncell);
    announce();
    return host_sharded((size_t)row_lo, (size_t)row_cnt, [&](size_t lo, size_t cnt, hipStream_t st) {
        return range(a, o, lo, cnt, st, cells, ncell);
    });
}

// R-layout counts (or an n x m matrix of doubles) up into `h_slot`, then gene-major into `gm_slot` with leading dimension ld
template <class T>
static int up_gene_major(Stage &s, int h_slot, int gm_slot, const void *host, size_t elem, int n, int m, long ld, const T **gm) {
    const void *r;
    void *g;
    DSQ_TRY(s.genes_up(h_slot, &r, host, elem, m));
    DSQ_TRY(capi_ws_get(gm_slot, (size_t)n * ld * elem, &g));
    if (elem == 4) DSQ_HIP(launch_transpose_r_to_gm_i32((const int32_t *)r, (int32_t *)g, n, m, ld, s.st));
    else DSQ_HIP(launch_transpose_r_to_gm_f64((const double *)r, (double *)g, n, m, ld, s.st));
    *gm = (const T *)g;
    return DSQ_OK;
}
// normalization factors: a vector of m size factors as it is, or an n x m matrix in R layout, which goes up gene-major
static int nf_up_gene_major(Stage &s, const double **field, const double *nf, int is_vector, int n, int m, long ld) {
    if (is_vector) return s.nf_up(field, nf, 1, m);
    return up_gene_major(s, WS_H_NF, WS_NF, nf, 8, n, m, ld, field);
}
// an n x m result that the kernels write gene-major: its slot, taken before the launch; and, after flush(), its way back to
// the caller's matrix in R layout (which comes down in finish())
static int gm_result_slot(size_t n, long ld, double **field) {
    void *w;
    DSQ_TRY(capi_ws_get(WS_MUOUT, n * ld * 8, &w));
    *field = (double *)w;
    return DSQ_OK;
}
static int gm_result_down(Stage &s, const double *gm, double *host, int n, int m, long ld) {
    double *r;
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &r, host, m));
    DSQ_HIP(launch_transpose_gm_to_r_f64(gm, r, n, m, ld, s.st));
    return DSQ_OK;
}

extern "C" {

int dsq_fit_beta(const DsqFitBetaArgs *a, const DsqFitBetaOut *o) { return dsq_fit_beta_rows(a, o, 0, a ? a->n : 0); }
int dsq_fit_disp(const DsqFitDispArgs *a, const DsqFitDispOut *o) { return dsq_fit_disp_rows(a, o, 0, a ? a->n : 0); }
int dsq_fit_disp_grid(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o) { return dsq_fit_disp_grid_rows(a, o, 0, a ? a->n : 0); }

int dsq_fit_beta_rows(const DsqFitBetaArgs *a, const DsqFitBetaOut *o, int64_t row_lo, int64_t row_cnt) {
    return fit_rows(a, o, row_lo, row_cnt, check_fit_beta, fit_beta_host_range, [&] {
        if (row_lo != 0) return;      // the n x m results land in fresh pages: take the faults while the inputs go up (stage.hip)
        stage_prefault(o->hat_diagonals, (size_t)a->n * a->m * 8);
        stage_prefault(o->mu, (size_t)a->n * a->m * 8);
    });
}

int dsq_fit_disp_rows(const DsqFitDispArgs *a, const DsqFitDispOut *o, int64_t row_lo, int64_t row_cnt) {
    const auto check = [](const DsqFitDispArgs *a_, const DsqFitDispOut *o_) {
        DSQ_TRY(check_fit_disp(a_, o_));
        return o_->last_d2lp ? DSQ_OK : capi_fail(DSQ_ERR_ARG, "NULL output array");      // (optional for the device entry only)
    };
    return fit_rows(a, o, row_lo, row_cnt, check, fit_disp_host_range, [] {});
}

int dsq_fit_disp_grid_rows(const DsqFitDispGridArgs *a, const DsqFitDispGridOut *o, int64_t row_lo, int64_t row_cnt) {
    return fit_rows(a, o, row_lo, row_cnt, check_fit_disp_grid, fit_disp_grid_host_range, [] {});
}

// (this entry and dsq_test_math keep inputs and results in ONE slot, WS_H_VEC: written out, not a Stage)
int dsq_parametric_dispersion_fit(const double *means, const double *disps, int64_t n, double *coefs, int32_t *status) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    DSQ_TRY(check_trend_fit(means, disps, n, coefs, status));
    DSQ_TRY(capi_check_device());
    hipStream_t st = nullptr;
    void *v;
    DSQ_TRY(capi_ws_get(WS_H_VEC, (2 * (size_t)n + 4) * 8, &v));
    double *d = (double *)v;
    DSQ_HIP(hipMemcpyAsync(d, means, n * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(d + n, disps, n * 8, hipMemcpyHostToDevice, st));
    void *tws;
    DSQ_TRY(capi_ws_get(WS_TREND, trend_fit_workspace_bytes(), &tws));
    DSQ_HIP(launch_trend_fit(d, d + n, (long)n, d + 2 * n, (int32_t *)(d + 2 * n + 2), tws, st));
    DSQ_HIP(hipMemcpyAsync(coefs, d + 2 * n, 16, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(status, d + 2 * n + 2, 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_prefit_moments(const DsqPrefitArgs *a, const DsqPrefitOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(check_prefit(a, o), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m, p = a->p;
    DsqPrefitArgs d = *a;
    DsqPrefitOut od = *o;
    Stage s(st, n);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    DSQ_TRY(s.weights_up(&d.weights, a->weights, a->useWeights, m));
    s.vec(&d.q, a->q, m * p * 8);
    s.vec(&d.a, a->a, m * p * 8);
    s.vec(&d.r, a->r, p * p * 8);
    DSQ_TRY(s.pack_in());
    s.out_gene_vec(&od.baseMean, o->baseMean);
    s.out_gene_vec(&od.baseVar, o->baseVar);
    s.out_gene_vec(&od.roughDisp, o->roughDisp);
    s.out_gene_vec(&od.allZero, o->allZero);
    s.out_vec(&od.beta_init, o->beta_init, n * p * 8);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(prefit_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_linear_mu(const DsqPrefitArgs *a, double mu_floor, double *mu) {
    HostCall hc;
    DSQ_TRY(host_ready(check_linear_mu(a, mu), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m, p = a->p;
    DsqPrefitArgs d = *a;
    double *mu_d;
    Stage s(st, n);
    stage_prefault(mu, n * m * 8);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    s.vec(&d.q, a->q, m * p * 8);
    s.vec(&d.a, a->a, m * p * 8);
    DSQ_TRY(s.pack_in());
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &mu_d, mu, m));
    DSQ_TRY(linear_mu_dev_locked(&d, mu_floor, mu_d, st));
    return s.flush();          // (the staged download of a matrix is complete on return)
}

int dsq_nbinom_loglike(const DsqLogLikeArgs *a, double *loglike) {
    HostCall hc;
    DSQ_TRY(host_ready(check_loglike(a, loglike), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    DsqLogLikeArgs d = *a;
    double *out_d;
    Stage s(st, n);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.genes_up(WS_H_MU, &d.mu, a->mu, 8, m));
    DSQ_TRY(s.weights_up(&d.weights, a->weights, a->useWeights, m));
    DSQ_TRY(s.table_up(WS_H_VEC, &d.disp, a->disp, 8, n));
    s.out_gene_vec(&out_d, loglike);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(loglike_dev_locked(&d, out_d, st));
    return s.finish();
}

int dsq_intercept_fit(const DsqInterceptArgs *a, const DsqInterceptOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(check_intercept(a, o), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    DsqInterceptArgs d = *a;
    DsqInterceptOut od = *o;
    Stage s(st, n);
    stage_prefault(o->mu, n * m * 8);
    stage_prefault(o->hat, n * m * 8);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    DSQ_TRY(s.weights_up(&d.weights, a->weights, a->useWeights, m));
    DSQ_TRY(s.table_up(WS_H_VEC, &d.alpha, a->alpha, 8, n));
    s.out_gene_vec(&od.beta_log2, o->beta_log2);
    s.out_gene_vec(&od.betaSE, o->betaSE);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &od.mu, o->mu, m));
    DSQ_TRY(s.out_mat(WS_H_OUTMAT2, &od.hat, o->hat, m));
    DSQ_TRY(intercept_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_optim_rows(const DsqOptimArgs *a, const DsqOptimOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(check_optim(a, o), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    // wide designs (see capi.hip): the kernel runs at the padded width pk -- zero design columns, ridge 1, start value 0
    const size_t n = a->n, m = a->m, p = a->p, pk = is_wide(a->p) ? wide_width(a->p) : a->p;
    OptimKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.m = a->m; kp.p = (int)pk; kp.minmu = a->minmu;
    Stage s(st, n);
    const void *v;
    DSQ_TRY(s.counts_up(&v, a->y, a->y_type, m));
    bool ycheck = false;
    long ld = 0;
    DSQ_TRY(prep_counts(v, a->y_type, DSQ_LAYOUT_R, 0, a->n, a->m, st, &kp.y, &ld, &ycheck));
    kp.ld = ld;
    kp.nf_is_vector = a->nf_is_vector ? 1 : 0;
    DSQ_TRY(s.nf_up(&kp.nf, a->nf, a->nf_is_vector, m));
    if (!a->nf_is_vector) DSQ_TRY(prep_matrix(kp.nf, DSQ_LAYOUT_R, 0, a->n, a->m, WS_NF, st, &kp.nf, ld));
    kp.useWeights = a->useWeights ? 1 : 0;
    DSQ_TRY(s.weights_up(&kp.weights, a->weights, a->useWeights, m));
    if (a->useWeights) DSQ_TRY(prep_matrix(kp.weights, DSQ_LAYOUT_R, 0, a->n, a->m, WS_W, st, &kp.weights, ld));
    // x | alpha | lambda (natural-log scale) | beta_start, each at the padded width
    static thread_local double lamnat[DSQ_P_WIDE];
    const double ln2 = 0.6931471805599453;
    for (size_t c = 0; c < pk; c++) lamnat[c] = c < p ? a->lambda[c] / (ln2 * ln2) : 1.0;
    s.vec(&kp.x, a->x, m * p * 8, m * pk * 8);
    s.vec(&kp.alpha_hat, a->alpha_hat, n * 8);
    s.vec(&kp.lamnat, lamnat, pk * 8);
    s.vec(&kp.beta_start, a->beta_start, n * p * 8, n * pk * 8);
    DSQ_TRY(s.pack_in(pk != p));
    // beta | betaSE (n x pk: the real coefficients are the leading columns) | loglike | conv ; mu gene-major, then R layout
    s.out_vec(&kp.beta, o->beta, n * p * 8, n * pk * 8);
    s.out_vec(&kp.betaSE, o->betaSE, n * p * 8, n * pk * 8);
    s.out_vec(&kp.loglike, o->logLike, n * 8);
    s.out_vec(&kp.conv, o->conv, n * 4);
    DSQ_TRY(s.pack_out());
    void *mu_gm;
    double *mu_r;
    DSQ_TRY(capi_ws_get(WS_MUOUT, n * (size_t)ld * 8, &mu_gm));
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &mu_r, o->mu, m, Stage::PLAIN));
    kp.mu_out = (double *)mu_gm;
    bool ok = false;
    prof_begin(st);
    DSQ_HIP(dispatch_optim_rows((int)pk, kp, st, &ok));
    prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "no kernel for p=%d", a->p);
    DSQ_HIP(launch_transpose_gm_to_r_f64(kp.mu_out, mu_r, a->n, a->m, ld, st));
    DSQ_TRY(s.finish());
    return finish_ycheck(ycheck, st);
}

int dsq_cooks_distance(const DsqCooksArgs *a, const DsqCooksOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(check_cooks(a, o), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    DsqCooksArgs d = *a;
    DsqCooksOut od = *o;
    Stage s(st, n);
    stage_prefault(o->cooks, n * m * 8);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    DSQ_TRY(s.genes_up(WS_H_MU, &d.mu, a->mu, 8, m));
    DSQ_TRY(s.genes_up(WS_H_W, &d.H, a->H, 8, m));
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &od.cooks, o->cooks, m));
    s.out_gene_vec(&od.maxCooks, o->maxCooks);
    s.out_gene_vec(&od.robustDisp, o->robustDisp);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(cooks_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_replace_outliers(const DsqReplaceArgs *a, const DsqReplaceOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(check_replace(a, o), a ? a->layout : 0));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    DsqReplaceArgs d = *a;
    DsqReplaceOut od = *o;
    Stage s(st, n);
    stage_prefault(o->newCounts, n * m * 4);
    DSQ_TRY(s.counts_up(&d.y, a->y, a->y_type, m));
    DSQ_TRY(s.nf_up(&d.nf, a->nf, a->nf_is_vector, m));
    DSQ_TRY(s.genes_up(WS_H_MU, &d.cooks, a->cooks, 8, m));
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &od.newCounts, o->newCounts, m));
    s.out_gene_vec(&od.replace, o->replace);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(replace_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_test_math(int op, const double *a, const double *b, const double *c, double *out, int64_t n) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    const bool need_b = op == 7 || op == 8 || op == 10 || op == 11 || op == 15 || op == 17 || op == 22;
    const bool need_c = op == 8 || op == 22;
    if (!a || !out || n < 0 || (need_b && !b) || (need_c && !c)) return capi_fail(DSQ_ERR_ARG, "bad arguments");
    DSQ_TRY(capi_check_device());
    if (n == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    void *v;
    DSQ_TRY(capi_ws_get(WS_H_VEC, 4 * (size_t)n * 8, &v));
    double *d = (double *)v;
    DSQ_HIP(hipMemcpyAsync(d, a, n * 8, hipMemcpyHostToDevice, st));
    if (b) DSQ_HIP(hipMemcpyAsync(d + n, b, n * 8, hipMemcpyHostToDevice, st));
    if (c) DSQ_HIP(hipMemcpyAsync(d + 2 * n, c, n * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(launch_test_math(op, d, d + n, d + 2 * n, d + 3 * n, n, st));
    DSQ_HIP(hipMemcpyAsync(out, d + 3 * n, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

// (inputs and results in ONE slot, as dsq_test_math: q | out | df | keep)
int dsq_pt(const double *q, const double *df, int32_t n, int32_t K, int32_t tail, const int32_t *keep, double *out) {
    std::lock_guard<std::mutex> lk(g_mu);
    WsScope ws(nullptr);
    DSQ_TRY(pt_check(q, df, n, K, tail, out));
    DSQ_TRY(capi_check_device());
    const size_t e = (size_t)n * K;
    if (e == 0) return DSQ_OK;
    hipStream_t st = nullptr;
    void *v;
    DSQ_TRY(capi_ws_get(WS_H_VEC, (2 * e + (size_t)n) * 8 + e * 4, &v));
    double *dq = (double *)v, *dout = dq + e, *ddf = dout + e;
    int32_t *dkeep = keep ? (int32_t *)(ddf + n) : nullptr;
    DSQ_HIP(hipMemcpyAsync(dq, q, e * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemcpyAsync(ddf, df, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (keep) {      // the kept entries of out are not written: they go up and come back as they are
        DSQ_HIP(hipMemcpyAsync(dkeep, keep, e * 4, hipMemcpyHostToDevice, st));
        DSQ_HIP(hipMemcpyAsync(dout, out, e * 8, hipMemcpyHostToDevice, st));
    }
    DSQ_HIP(launch_pt(dq, ddf, n, K, tail, dkeep, dout, st));
    DSQ_HIP(hipMemcpyAsync(out, dout, e * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_size_factors(const DsqSizeFactorArgs *a, const DsqSizeFactorOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(size_factors_check(a, o), a ? a->layout : 0));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    DsqSizeFactorArgs d = *a;
    DsqSizeFactorOut od = *o;
    Stage s(st, n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, a->y_type == DSQ_Y_INT32 ? 4 : 8, a->n, a->m, ld, &d.y));
    d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    if (a->normMatrix) {
        DSQ_TRY(up_gene_major(s, WS_H_NF, WS_NF, a->normMatrix, 8, a->n, a->m, ld, &d.normMatrix));
        DSQ_TRY(gm_result_slot(n, ld, &od.normalizationFactors));
    }
    s.vec(&d.geoMeans, a->geoMeans, n * 8);
    s.vec(&d.control, a->control, n * 4);
    DSQ_TRY(s.pack_in());
    const size_t wsb = size_factors_workspace_bytes(a->n, a->m);
    DSQ_TRY(capi_ws_get(WS_SCRATCH, wsb, &d.workspace));
    d.workspace_bytes = (int64_t)wsb;
    s.out_vec(&od.sizeFactors, o->sizeFactors, m * 8);
    s.out_gene_vec(&od.loggeomeans, o->loggeomeans);
    s.out_vec(&od.status, o->status, 4);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(size_factors_dev_locked(&d, &od, st));
    DSQ_TRY(s.flush());
    if (a->normMatrix) DSQ_TRY(gm_result_down(s, od.normalizationFactors, o->normalizationFactors, a->n, a->m, ld));
    DSQ_TRY(s.finish());
    if (*o->status == 1)
        return capi_fail(DSQ_ERR_FIT, "every gene contains at least one zero, cannot compute log geometric means");
    return DSQ_OK;
}

int dsq_vst(const DsqVstArgs *a, const DsqVstOut *o) {
    const bool transform = o && o->out, stats = o && (o->rowMean || o->rowMax);
    const auto check = [&] {
        if (o && !transform && !stats) return capi_fail(DSQ_ERR_ARG, "neither an output matrix nor row statistics asked for");
        return vst_check(a, o, transform, stats);
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), a ? a->layout : 0));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    DsqVstArgs d = *a;
    DsqVstOut od = *o;
    Stage s(st, n);
    if (transform) stage_prefault(o->out, n * m * 8);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, a->y_type == DSQ_Y_INT32 ? 4 : 8, a->n, a->m, ld, &d.y));
    d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    DSQ_TRY(nf_up_gene_major(s, &d.nf, a->nf, a->nf_is_vector, a->n, a->m, ld));
    int32_t bad = 0;
    s.out_vec(&od.bad, &bad, 4, 8);
    s.out_gene_vec(&od.rowMean, o->rowMean);
    s.out_gene_vec(&od.rowMax, o->rowMax);
    DSQ_TRY(s.pack_out());
    DSQ_HIP(hipMemsetAsync(od.bad, 0, 8, st));
    if (transform) DSQ_TRY(gm_result_slot(n, ld, &od.out));
    DSQ_TRY(vst_dev_locked(&d, &od, transform, stats, st));
    DSQ_TRY(s.flush());
    if (transform) DSQ_TRY(gm_result_down(s, od.out, o->out, a->n, a->m, ld));
    DSQ_TRY(s.finish());
    if (bad) return capi_fail(DSQ_ERR_VALUE, "count matrix holds negative, non-finite or non-integer values");
    return DSQ_OK;
}

int dsq_rlog(const DsqRlogArgs *a, const DsqRlogOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(rlog_check(a, o), a ? a->layout : 0));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    // stopifnot(all(!is.na(dispFit))) on the rows that are fitted (R/rlog.R:227-228); a non-positive value has no fit either
    for (size_t i = 0; i < n; i++) {
        if (a->dispFit[i] > 0.0 && a->dispFit[i] - a->dispFit[i] == 0.0) continue;
        bool fitted = false;
        if (a->intercept) fitted = a->intercept[i] - a->intercept[i] == 0.0;
        else for (size_t j = 0; j < m && !fitted; j++)
            fitted = a->y_type == DSQ_Y_INT32 ? ((const int32_t *)a->y)[i + n * j] != 0 : ((const double *)a->y)[i + n * j] != 0.0;
        if (fitted) return capi_fail(DSQ_ERR_ARG, "dispFit[%zu] = %g on a row that is fitted", i, a->dispFit[i]);
    }
    const long ld = round_ld(a->m);
    DsqRlogArgs d = *a;
    DsqRlogOut od = *o;
    Stage s(st, n);
    stage_prefault(o->rlog, n * m * 8);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, a->y_type == DSQ_Y_INT32 ? 4 : 8, a->n, a->m, ld, &d.y));
    d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    DSQ_TRY(nf_up_gene_major(s, &d.nf, a->nf, a->nf_is_vector, a->n, a->m, ld));
    s.gene_vec(&d.dispFit, a->dispFit);
    if (a->intercept) s.gene_vec(&d.intercept, a->intercept);
    DSQ_TRY(s.pack_in());
    int32_t bad = 0;
    s.out_vec(&od.bad, &bad, 4, 8);
    if (o->intercept) s.out_gene_vec(&od.intercept, o->intercept);
    s.out_gene_vec(&od.iter, o->iter);
    s.out_gene_vec(&od.flag, o->flag);
    DSQ_TRY(s.pack_out());
    DSQ_HIP(hipMemsetAsync(od.bad, 0, 8, st));
    DSQ_TRY(gm_result_slot(n, ld, &od.rlog));
    DSQ_TRY(rlog_dev_locked(&d, &od, st));
    DSQ_TRY(s.flush());
    DSQ_TRY(gm_result_down(s, od.rlog, o->rlog, a->n, a->m, ld));
    DSQ_TRY(s.finish());
    if (bad) return capi_fail(DSQ_ERR_VALUE, "count matrix holds negative, non-finite or non-integer values");
    return DSQ_OK;
}

int dsq_apeglm(const DsqApeglmArgs *a, const DsqApeglmOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(apeglm_check(a, o), a ? a->layout : 0));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m, p = a->p;
    const long ld = round_ld(a->m);
    DsqApeglmArgs d = *a;
    DsqApeglmOut od = *o;
    Stage s(st, n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, a->y_type == DSQ_Y_INT32 ? 4 : 8, a->n, a->m, ld, &d.y));
    d.layout = DSQ_LAYOUT_GENE_MAJOR; d.ld = ld;
    DSQ_TRY(nf_up_gene_major(s, &d.nf, a->nf, a->nf_is_vector, a->n, a->m, ld));
    if (a->weights) DSQ_TRY(up_gene_major(s, WS_H_W, WS_W, a->weights, 8, a->n, a->m, ld, &d.weights));
    s.vec(&d.x, a->x, m * p * 8);
    s.gene_vec(&d.disp, a->disp);
    if (a->init) s.vec(&d.init, a->init, n * p * 8);
    DSQ_TRY(s.pack_in());
    int32_t bad = 0;
    s.out_vec(&od.bad, &bad, 4, 8);
    s.out_vec(&od.map, o->map, n * p * 8);
    s.out_vec(&od.sd, o->sd, n * p * 8);
    s.out_gene_vec(&od.fsr, o->fsr);
    s.out_gene_vec(&od.thresh, o->thresh);
    s.out_vec(&od.iter, o->iter, n * 2 * 8);
    s.out_gene_vec(&od.conv, o->conv);
    s.out_gene_vec(&od.start, o->start);
    s.out_gene_vec(&od.objective, o->objective);
    DSQ_TRY(s.pack_out());
    DSQ_HIP(hipMemsetAsync(od.bad, 0, 8, st));
    DSQ_TRY(apeglm_dev_locked(&d, &od, st));
    DSQ_TRY(s.finish());
    if (bad) return capi_fail(DSQ_ERR_VALUE, "count matrix holds negative, non-finite or non-integer values");
    return DSQ_OK;
}

int dsq_unmix(const DsqUnmixArgs *a, const DsqUnmixOut *o) {
    const auto check = [&]() -> int {
        if (int rc = unmix_check(a, o)) return rc;
        // (R would carry a negative or missing value into optim's objective; here it is refused)
        const size_t nx = (size_t)a->n * a->m, np = (size_t)a->n * a->k;
        for (size_t t = 0; t < nx; t++)
            if (!(a->x[t] >= 0.0) || a->x[t] - a->x[t] != 0.0) return capi_fail(DSQ_ERR_VALUE, "x holds a negative or non-finite value");
        for (size_t t = 0; t < np; t++)
            if (!(a->pure[t] >= 0.0) || a->pure[t] - a->pure[t] != 0.0) return capi_fail(DSQ_ERR_VALUE, "pure holds a negative or non-finite value");
        return DSQ_OK;
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t m = a->m, k = a->k;
    const long ld = round_ld(a->m);
    DsqUnmixArgs d = *a;
    DsqUnmixOut od = *o;
    Stage s(st, a->n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->x, 8, a->n, a->m, ld, &d.x));
    d.ld = ld;
    DSQ_TRY(up_gene_major(s, WS_H_X, WS_PAD_X, a->pure, 8, a->n, a->k, (long)k, &d.pure));
    s.out_vec(&od.p, o->p, m * k * 8);
    s.out_vec(&od.loss, o->loss, m * 8);
    s.out_vec(&od.iter, o->iter, m * 4);
    s.out_vec(&od.flag, o->flag, m * 4);
    DSQ_TRY(s.pack_out());
    const size_t wsb = unmix_workspace_bytes(a->n, a->m);
    void *w;
    DSQ_TRY(capi_ws_get(WS_SCRATCH, wsb, &w));
    DSQ_TRY(unmix_dev_locked(&d, &od, w, (int64_t)wsb, st));
    return s.finish();
}

int dsq_top_var(const DsqTopVarArgs *a, const DsqTopVarOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(top_var_check(a, o), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const long ld = round_ld(a->m);
    const size_t k = a->ntop < a->n ? a->ntop : a->n;
    DsqTopVarArgs d = *a;
    DsqTopVarOut od = *o;
    Stage s(st, a->n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->x, 8, a->n, a->m, ld, &d.x));
    d.ld = ld;
    s.out_gene_vec(&od.rowMean, o->rowMean);
    s.out_gene_vec(&od.rowVar, o->rowVar);
    if (k) s.out_vec(&od.select, o->select, k * 4);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(top_var_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_sample_pairs(const DsqSamplePairsArgs *a, const DsqSamplePairsOut *o) {
    const auto check = [&]() -> int {
        if (int rc = sample_pairs_check(a, o)) return rc;
        for (int t = 0; a->rows && t < a->nrows; t++)
            if (a->rows[t] < 0 || a->rows[t] >= a->n) return capi_fail(DSQ_ERR_ARG, "rows[%d] = %d is outside [0, %d)", t, a->rows[t], a->n);
        return DSQ_OK;
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const long ld = round_ld(a->m);
    const size_t m = a->m, R = a->rows ? a->nrows : a->n;
    DsqSamplePairsArgs d = *a;
    DsqSamplePairsOut od = *o;
    Stage s(st, a->n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->x, 8, a->n, a->m, ld, &d.x));
    d.ld = ld;
    if (a->rows) s.vec(&d.rows, a->rows, R * 4);
    if (a->kind == DSQ_PAIRS_GRAM && a->centre) s.vec(&d.centre, a->centre, R * 8);
    DSQ_TRY(s.pack_in());
    s.out_vec(&od.out, o->out, m * m * 8);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(sample_pairs_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_local_fit(const DsqLocalFitArgs *a, const DsqLocalFitOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(local_fit_check(a, o), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, blockb = (kLocalFitHeaderDoubles + 3 * n) * 8;
    const size_t nq = !o->dispFit ? 0 : a->eval_means ? (size_t)a->n_eval : n;
    DsqLocalFitArgs d = *a;
    DsqLocalFitOut od = *o;
    int32_t status[4] = {0, 0, 0, 0};
    Stage s(st, n);
    if (a->fit_in) s.vec(&d.fit_in, a->fit_in, blockb);
    else {
        s.vec(&d.means, a->means, n * 8);
        s.vec(&d.disps, a->disps, n * 8);
    }
    if (a->eval_means) s.vec(&d.eval_means, a->eval_means, nq * 8);
    DSQ_TRY(s.pack_in());
    if (!a->fit_in) s.out_vec(&od.fit, o->fit, blockb);
    if (nq) s.out_vec(&od.dispFit, o->dispFit, nq * 8);
    s.out_vec(&od.status, status, sizeof status);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(local_fit_dev_locked(&d, &od, st));
    DSQ_TRY(s.finish());
    memcpy(o->status, status, sizeof status);
    if (status[0] > 0 && status[1] < 3) return capi_fail(DSQ_ERR_FIT, "local dispersion fit: fewer than 3 points in a window");
    return DSQ_OK;
}

int dsq_collapse(const DsqCollapseArgs *a, const DsqCollapseOut *o) {
    const auto check = [&]() -> int {
        if (int rc = collapse_check(a, o)) return rc;
        // split(seq(along = groupby), groupby): every sample once, ascending inside a group, no empty group (droplevels)
        if (a->offsets[0] != 0 || a->offsets[a->g] != a->m) return capi_fail(DSQ_ERR_ARG, "offsets run from %d to %d, not from 0 to m = %d", a->offsets[0], a->offsets[a->g], a->m);
        std::vector<char> seen(a->m, 0);
        for (int c = 0; c < a->g; c++) {
            if (a->offsets[c + 1] <= a->offsets[c]) return capi_fail(DSQ_ERR_ARG, "group %d is empty or offsets descend", c);
            for (int k = a->offsets[c]; k < a->offsets[c + 1]; k++) {
                const int j = a->members[k];
                if (j < 0 || j >= a->m || seen[j]) return capi_fail(DSQ_ERR_ARG, "members[%d] = %d is outside [0, %d) or listed twice", k, j, a->m);
                if (k > a->offsets[c] && j < a->members[k - 1]) return capi_fail(DSQ_ERR_ARG, "members of group %d are not ascending", c);
                seen[j] = 1;
            }
        }
        return DSQ_OK;
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m, g = a->g;
    const long ld = round_ld(a->m), ldo = round_ld(a->g);
    DsqCollapseArgs d = *a;
    DsqCollapseOut od = *o;
    Stage s(st, n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, 4, a->n, a->m, ld, &d.y));
    d.ld = ld;
    s.vec(&d.members, a->members, m * 4);
    s.vec(&d.offsets, a->offsets, (g + 1) * 4);
    DSQ_TRY(s.pack_in());
    int32_t status = 0;
    s.out_vec(&od.status, &status, 4, 8);
    DSQ_TRY(s.pack_out());
    DSQ_HIP(hipMemsetAsync(od.status, 0, 8, st));
    void *gm;
    DSQ_TRY(capi_ws_get(WS_MUOUT, n * ldo * 4, &gm));
    od.out = (int32_t *)gm;
    od.ld = ldo;
    DSQ_TRY(collapse_dev_locked(&d, &od, st));
    DSQ_TRY(s.flush());
    int32_t *r;
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &r, o->out, g));
    DSQ_HIP(launch_transpose_gm_to_r_i32(od.out, r, a->n, a->g, ldo, st));
    DSQ_TRY(s.finish());
    if (o->status) *o->status = status;
    if (status & 1) return capi_fail(DSQ_ERR_VALUE, "a group sum exceeds the largest integer (2147483647)");
    return DSQ_OK;
}

int dsq_col_sums(const DsqColSumsArgs *a, const DsqColSumsOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(col_sums_check(a, o), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const long ld = round_ld(a->m);
    DsqColSumsArgs d = *a;
    DsqColSumsOut od = *o;
    Stage s(st, a->n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, 4, a->n, a->m, ld, &d.y));
    d.ld = ld;
    s.out_vec(&od.sums, o->sums, (size_t)a->m * 8);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(col_sums_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_fpm(const DsqFpmArgs *a, const DsqFpmOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(fpm_check(a, o), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    DsqFpmArgs d = *a;
    DsqFpmOut od = *o;
    Stage s(st, n);
    stage_prefault(o->out, n * m * 8);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, 4, a->n, a->m, ld, &d.y));
    d.ld = ld;
    if (a->kind == DSQ_FPKM_TXLEN) DSQ_TRY(up_gene_major(s, WS_H_NF, WS_NF, a->txlen, 8, a->n, a->m, ld, &d.txlen));
    s.vec(&d.lib, a->lib, m * 8);                  // first in the packed buffer: 16-byte aligned, as the paired loads want
    if (a->kind == DSQ_FPKM_BASEPAIRS) s.gene_vec(&d.basepairs, a->basepairs);
    DSQ_TRY(s.pack_in());
    DSQ_TRY(gm_result_slot(n, ld, &od.out));
    DSQ_TRY(fpm_dev_locked(&d, &od, st));
    DSQ_TRY(gm_result_down(s, od.out, o->out, a->n, a->m, ld));
    return s.finish();
}

int dsq_ash(const DsqAshArgs *a, const DsqAshOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(ash_check(a, o), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, C = a->C, nC = n * C;
    // what goes up: the two matrices, packed to a column stride of n; what comes down: seven n x C matrices, pi, sd, loglik
    // and the three int32 vectors, one block
    void *vin, *vout, *w;
    DSQ_TRY(capi_ws_get(WS_H_VEC, 2 * nC * 8, &vin));
    const size_t small = 2 * C * DSQ_ASH_MAX_K + C;
    DSQ_TRY(capi_ws_get(WS_H_OUTVEC, (7 * nC + small) * 8 + 3 * C * 4, &vout));
    double *db = (double *)vin, *ds = db + nC;
    for (size_t c = 0; c < C; c++) {
        DSQ_HIP(hipMemcpyAsync(db + c * n, a->betahat + c * a->ld, n * 8, hipMemcpyHostToDevice, st));
        DSQ_HIP(hipMemcpyAsync(ds + c * n, a->sebetahat + c * a->ld, n * 8, hipMemcpyHostToDevice, st));
    }
    DsqAshArgs d = *a;
    DsqAshOut od;
    d.betahat = db; d.sebetahat = ds; d.ld = (int64_t)n;
    double *p = (double *)vout;
    double **rows[7] = {&od.PosteriorMean, &od.PosteriorSD, &od.NegativeProb, &od.PositiveProb, &od.lfsr, &od.le_T, &od.gt_mT};
    double *const host_rows[7] = {o->PosteriorMean, o->PosteriorSD, o->NegativeProb, o->PositiveProb, o->lfsr, o->le_T, o->gt_mT};
    for (int k = 0; k < 7; k++, p += nC) *rows[k] = p;
    od.pi = p; p += C * DSQ_ASH_MAX_K;
    od.sd = p; p += C * DSQ_ASH_MAX_K;
    od.loglik = p; p += C;
    od.K = (int32_t *)p; od.iter = od.K + C; od.flag = od.iter + C;
    const size_t wsb = ash_workspace_bytes(a->n, a->C);
    DSQ_TRY(capi_ws_get(WS_SCRATCH, wsb, &w));
    DSQ_TRY(ash_dev_locked(&d, &od, w, (int64_t)wsb, st));
    for (int k = 0; k < 7; k++)
        for (size_t c = 0; c < C; c++)
            DSQ_HIP(hipMemcpyAsync(host_rows[k] + c * a->ld, *rows[k] + c * n, n * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->pi, od.pi, C * DSQ_ASH_MAX_K * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->sd, od.sd, C * DSQ_ASH_MAX_K * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->loglik, od.loglik, C * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->K, od.K, C * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->iter, od.iter, C * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipMemcpyAsync(o->flag, od.flag, C * 4, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

int dsq_sf_iterate(const DsqSfIterateArgs *a, const DsqSfIterateOut *o) {
    const auto check = [&]() -> int {
        if (int rc = sf_iterate_check(a, o)) return rc;
        const size_t nm = (size_t)a->n * a->m;
        for (size_t t = 0; t < nm; t++) {
            if (a->y[t] < 0) return capi_fail(DSQ_ERR_VALUE, "the count matrix holds a negative value");
            if (!(a->mu[t] >= 0.0) || a->mu[t] - a->mu[t] != 0.0) return capi_fail(DSQ_ERR_VALUE, "mu holds a negative or non-finite value");
        }
        for (int j = 0; j < a->m; j++)
            if (!(a->sf[j] > 0.0) || a->sf[j] - a->sf[j] != 0.0) return capi_fail(DSQ_ERR_VALUE, "sf[%d] = %g is not positive and finite", j, a->sf[j]);
        return DSQ_OK;
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m;
    const long ld = round_ld(a->m);
    DsqSfIterateArgs d = *a;
    DsqSfIterateOut od = *o;
    Stage s(st, n);
    DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->y, 4, a->n, a->m, ld, &d.y));
    d.ld = ld;
    DSQ_TRY(up_gene_major(s, WS_H_NF, WS_NF, a->mu, 8, a->n, a->m, ld, &d.mu));
    s.vec(&d.sf, a->sf, m * 8);
    s.vec(&d.disp, a->disp, n * 8);
    s.vec(&d.rows, a->rows, n * 4);
    DSQ_TRY(s.pack_in());
    s.out_vec(&od.s, o->s, m * 8);
    s.out_vec(&od.sf, o->sf, m * 8);
    s.out_vec(&od.F, o->F, 8);
    s.out_vec(&od.iter, o->iter, 4);
    s.out_vec(&od.evals, o->evals, 4);
    s.out_vec(&od.flag, o->flag, 4);
    DSQ_TRY(s.pack_out());
    const size_t wsb = sf_iterate_workspace_bytes(a->n, a->m);
    void *w;
    DSQ_TRY(capi_ws_get(WS_SCRATCH, wsb, &w));
    DSQ_TRY(sf_iterate_dev_locked(&d, &od, w, (int64_t)wsb, st));
    return s.finish();
}

int dsq_results(const DsqResultsArgs *a, const DsqResultsOut *o) {
    const auto check = [&]() -> int {
        if (int rc = results_check(a, o)) return rc;
        if (!o->filtPadj) return capi_fail(DSQ_ERR_ARG, "NULL filtPadj");
        if (!a->independentFiltering) return DSQ_OK;
        const double *f = a->filter ? a->filter : a->baseMean;
        for (int32_t i = 0; i < a->n; i++)
            if (f[i] != f[i]) return capi_fail(DSQ_ERR_ARG, "filter[%d] is NaN", i);
        for (int32_t k = 0; k < a->K; k++)
            if (!(a->theta[k] >= 0.0 && a->theta[k] <= 1.0)) return capi_fail(DSQ_ERR_ARG, "theta[%d] = %g outside [0, 1]", k, a->theta[k]);
        return DSQ_OK;
    };
    HostCall hc;
    DSQ_TRY(host_ready(check(), DSQ_LAYOUT_R));
    hipStream_t st = hc.st;
    const size_t n = a->n, p = a->p, K = a->K;
    const size_t tcols = a->test == DSQ_TEST_LRT ? 1 : p;
    DsqResultsArgs d = *a;
    DsqResultsOut od = *o;
    Stage s(st, n);
    DSQ_TRY(s.table_up(WS_H_MU, &d.beta, a->beta, 8, n, p));
    DSQ_TRY(s.table_up(WS_H_W, &d.betaSE, a->betaSE, 8, n, p));
    DSQ_TRY(s.table_up(WS_H_NF, &d.stat, a->stat, 8, n, tcols));
    DSQ_TRY(s.table_up(WS_H_Y, &d.pvalue, a->pvalue, 8, n, tcols));
    s.vec(&d.baseMean, a->baseMean, n * 8);
    s.vec(&d.replace, a->replace, n * 4);
    s.vec(&d.na_mask, a->na_mask, n * 4);
    s.vec(&d.filter, a->filter, n * 8);
    s.vec(&d.df, a->df, n * 8);
    if (a->independentFiltering) s.vec(&d.theta, a->theta, K * 8);
    DSQ_TRY(s.pack_in());
    const size_t wsb = results_sort_workspace_bytes(a->n);
    DSQ_TRY(capi_ws_get(WS_SCRATCH, wsb, &d.workspace));
    d.workspace_bytes = (int64_t)wsb;
    s.out_gene_vec(&od.baseMean, o->baseMean);
    s.out_gene_vec(&od.log2FoldChange, o->log2FoldChange);
    s.out_gene_vec(&od.lfcSE, o->lfcSE);
    s.out_gene_vec(&od.stat, o->stat);
    s.out_gene_vec(&od.pvalue, o->pvalue);
    s.out_vec(&od.numRej, o->numRej, K * 4);
    s.out_vec(&od.cutoffs, o->cutoffs, K * 8);
    s.out_vec(&od.status, o->status, 4, 8);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(s.out_mat(WS_H_OUTMAT, &od.filtPadj, o->filtPadj, K));
    DSQ_TRY(results_dev_locked(&d, &od, st));
    return s.finish();
}

int dsq_contrasts(const DsqContrastsArgs *a, const DsqContrastsOut *o) {
    HostCall hc;
    DSQ_TRY(host_ready(contrasts_check(a, o), DSQ_LAYOUT_R));
    if (a->n == 0) return DSQ_OK;
    hipStream_t st = hc.st;
    const size_t n = a->n, m = a->m, p = a->p, K = a->K;
    const long ld = round_ld(a->m);
    DsqContrastsArgs d = *a;
    DsqContrastsOut od = *o;
    d.ld = ld;
    std::vector<int32_t> labels;
    Stage s(st, n);
    if (a->sample_mask) {
        DSQ_TRY(up_gene_major(s, WS_H_Y, WS_Y, a->counts, 4, a->n, a->m, ld, &d.counts));
        s.vec(&d.sample_mask, a->sample_mask, K * m * 4);
        s.vec(&d.rule_applies, a->rule_applies, K * 4);
    }
    if (a->allZero) s.vec(&d.allZero, a->allZero, n * 4);
    if (a->contrasts) {
        host_cells(a->x, a->m, a->p, a->cell_of, a->ncell, &labels, &d.cell_of, &d.ncell);
        DSQ_TRY(nf_up_gene_major(s, &d.nf, a->nf, a->nf_is_vector, a->n, a->m, ld));
        if (a->useWeights) DSQ_TRY(up_gene_major(s, WS_H_W, WS_W, a->weights, 8, a->n, a->m, ld, &d.weights));
        s.vec(&d.x, a->x, m * p * 8);
        s.vec(&d.alpha_hat, a->alpha_hat, n * 8);
        s.vec(&d.beta, a->beta, n * p * 8);
        s.vec(&d.lambda, a->lambda, p * 8);
        s.vec(&d.contrasts, a->contrasts, p * K * 8);
        s.vec(&d.df, a->df, n * 8);
        s.out_vec(&od.log2FoldChange, o->log2FoldChange, n * K * 8);
        s.out_vec(&od.lfcSE, o->lfcSE, n * K * 8);
        s.out_vec(&od.stat, o->stat, n * K * 8);
        s.out_vec(&od.pvalue, o->pvalue, n * K * 8);
    }
    DSQ_TRY(s.pack_in());
    if (o->contrastAllZero) s.out_vec(&od.contrastAllZero, o->contrastAllZero, n * K * 4);
    DSQ_TRY(s.pack_out());
    DSQ_TRY(contrasts_dev_locked(&d, &od, st));
    return s.finish();
}

}  // extern "C"
