// beta_prior.hip -- dsq_beta_prior_var: estimateBetaPriorVar (R/core.R:1601-1689) on the n x p matrix of MLE
// coefficients, for the betaPrior = TRUE branch of nbinomWaldTest inside dsq_deseq (deseq_host.hip).
//
// An all-gene step on n-vectors like the dispersion trend: per model-matrix column (and, for the expanded model matrix,
// per pairwise contrast of a factor's levels, addAllContrasts R/expanded.R:76-98) the prior variance is
//     matchWeightedUpperQuantileForVariance(x, w)  =  (wtd.quantile(|x|, w, 1 - 0.05, normwt = TRUE) / qnorm(1 - 0.05 / 2))^2
// (R/core.R:2416-2419) over the rows with |x| < 10 (:1651), w = 1 / (1 / baseMean + dispFit) (:1641-1642), the intercept
// set to 1e6 (:1669-1671), and for the expanded matrix the mean over a factor's level and contrast variances handed to all
// of its level columns (averagePriorsOverLevels, R/expanded.R:20-73).  Hmisc's wtd.quantile (R/core.R:2762-2800) is a
// stable sort of the values, the weight sums of the distinct values, their running sum and a step interpolation.
//
// Host code: the inputs are what the chain brings down anyway (n (p + 3) doubles), the sort is a stable LSD radix sort on
// the bit patterns (|x| >= 0: the patterns order like the values), every sum is SEQUENTIAL in the order stated below --
// the one definition deseq2_amd/core.py (estimateBetaPriorVar / Hmisc_wtd_quantile) follows as well, so the two give the
// same bits (tests/test_capi_cpu.py::test_beta_prior_var_equals_the_host_mirror).  Columns are independent: a few
// threads take them in turn.
//
// dsq_beta_prior_var_dev, further down: the same definition on resident inputs (lfcShrink's expanded matrix has a column
// per pair of levels: hundreds of weighted quantiles), the same bits.
#include "../../include/deseq2_mi355x.h"
#include "dsq_internal.hpp"
#include "dsq_wave.hpp"

#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

namespace dsq {
namespace {

const double kQnorm975 = 1.959963984540054;      // qnorm(1 - 0.05 / 2)

// stable ascending order of non-negative doubles: 8 passes of 8 bits over the bit patterns
static void radix_order(const std::vector<double> &v, std::vector<uint32_t> *order) {
    const size_t n = v.size();
    std::vector<uint64_t> key(n), key2(n);
    std::vector<uint32_t> idx(n), idx2(n);
    for (size_t i = 0; i < n; i++) { memcpy(&key[i], &v[i], 8); idx[i] = (uint32_t)i; }
    for (int pass = 0; pass < 8; pass++) {
        const int sh = 8 * pass;
        size_t cnt[257];
        memset(cnt, 0, sizeof cnt);
        for (size_t i = 0; i < n; i++) cnt[((key[i] >> sh) & 0xff) + 1]++;
        bool trivial = false;
        for (int b = 0; b < 256; b++) { if (cnt[b + 1] == n) trivial = true; cnt[b + 1] += cnt[b]; }
        if (trivial) continue;                       // all keys share this digit: the pass is the identity
        for (size_t i = 0; i < n; i++) {
            const size_t d = cnt[(key[i] >> sh) & 0xff]++;
            key2[d] = key[i]; idx2[d] = idx[i];
        }
        key.swap(key2); idx.swap(idx2);
    }
    order->swap(idx);
}

// Hmisc::wtd.quantile(x, weights, probs = prob, normwt = TRUE) for ONE probability (R/core.R:2762-2800)
static double wtd_quantile(std::vector<double> &x, std::vector<double> &w, double prob) {
    // rows with NA or zero weight are dropped (:2771-2775)
    size_t N = 0;
    for (size_t i = 0; i < x.size(); i++)
        if (!(std::isnan(w[i]) || w[i] == 0.0)) { x[N] = x[i]; w[N] = w[i]; N++; }
    x.resize(N); w.resize(N);
    if (N == 0) return NAN;
    double wsum = 0.0;                               // sum(weights), in row order
    for (size_t i = 0; i < N; i++) wsum += w[i];
    for (size_t i = 0; i < N; i++) w[i] = w[i] * (double)N / wsum;      // weights * length(x) / sum(weights)
    std::vector<uint32_t> o;
    radix_order(x, &o);
    // distinct values (ascending) with the sums of their weights, each in sorted order; cs = their running sum
    std::vector<double> ux, cs;
    ux.reserve(N); cs.reserve(N);
    double run = 0.0, tot = 0.0;
    for (size_t k = 0; k < N; k++) {
        const double v = x[o[k]];
        run += w[o[k]];
        if (k + 1 == N || x[o[k + 1]] != v) {
            tot += run;
            ux.push_back(v); cs.push_back(tot);
            run = 0.0;
        }
    }
    const double n = tot;
    const double order = 1.0 + (n - 1.0) * prob;
    const double fl = std::floor(order);
    const double low = fl > 1.0 ? fl : 1.0;
    const double high = (low + 1.0 < n) ? low + 1.0 : n;
    const double frac = std::fmod(order, 1.0);
    auto stepq = [&](double q) {                     // approx(cumsum(wts), x, method = "constant", f = 1, rule = 2)
        size_t lo = 0, hi = cs.size();
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if (cs[mid] < q) lo = mid + 1; else hi = mid; }
        return ux[lo < ux.size() ? lo : ux.size() - 1];
    };
    return (1.0 - frac) * stepq(low) + frac * stepq(high);
}

// the columns whose variance is matched: the p design columns, then (expanded) the level contrasts factor by factor
struct Col { int i, j; };                            // value = beta[, i] - (j >= 0 ? beta[, j] : 0)
struct Columns {
    std::vector<Col> cols;
    std::vector<int> col_factor;
    int nfac = 0;
};

static Columns list_columns(const DsqBetaPriorArgs *a) {
    const int p = a->p;
    Columns L;
    for (int c = 0; c < p; c++) L.cols.push_back({c, -1});
    for (int c = 0; c < p; c++) if (a->coef_factor[c] > L.nfac) L.nfac = a->coef_factor[c];
    L.col_factor.assign(a->coef_factor, a->coef_factor + p);
    if (a->expanded)
        for (int f = 1; f <= L.nfac; f++) {
            std::vector<int> idx;
            for (int c = 0; c < p; c++) if (a->coef_factor[c] == f) idx.push_back(c);
            for (size_t j = 0; j + 1 < idx.size(); j++)
                for (size_t i = j + 1; i < idx.size(); i++) { L.cols.push_back({idx[i], idx[j]}); L.col_factor.push_back(f); }
        }
    return L;
}

static int close_columns(const DsqBetaPriorArgs *a, const Columns &L, const std::vector<double> &pv, double *out);

}  // namespace

int beta_prior_var(const DsqBetaPriorArgs *a, double *out) {
    const int n = a->n;
    const Columns L = list_columns(a);
    const std::vector<Col> &cols = L.cols;
    // rows that enter: the ones that are not all zero (objectNZ, R/core.R:1610); weights 1 / (1 / baseMean + dispFit)
    std::vector<int> rows;
    rows.reserve(n);
    for (int g = 0; g < n; g++) if (!a->allZero[g]) rows.push_back(g);
    std::vector<double> wrow(rows.size());
    for (size_t k = 0; k < rows.size(); k++) wrow[k] = 1.0 / (1.0 / a->baseMean[rows[k]] + a->dispFit[rows[k]]);
    std::vector<double> pv(cols.size(), 0.0);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        std::vector<double> x, w;
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= cols.size()) break;
            if (cols[c].j < 0 && a->coef_factor[cols[c].i] == 0) { pv[c] = 1e6; continue; }      // the intercept (:1669-1671)
            x.clear(); w.clear();
            const double *bi = a->mle_beta + (size_t)n * cols[c].i, *bj = cols[c].j >= 0 ? a->mle_beta + (size_t)n * cols[c].j : nullptr;
            if (rows.size() == 1) {                               // a one-gene object: (betaMatrix)^2 (R/core.R:1647,1662)
                const double v = bj ? bi[rows[0]] - bj[rows[0]] : bi[rows[0]];
                pv[c] = v * v;
                continue;
            }
            for (size_t k = 0; k < rows.size(); k++) {
                const double v = bj ? bi[rows[k]] - bj[rows[k]] : bi[rows[k]];
                const double av = std::fabs(v);
                if (av < 10.0) { x.push_back(av); w.push_back(wrow[k]); }                          // useFinite (:1651)
            }
            if (x.empty()) { pv[c] = 1e6; continue; }                                               // :1652-1653
            const double sd = wtd_quantile(x, w, 1.0 - a->upperQuantile) / kQnorm975;
            pv[c] = sd * sd;
        }
    };
    {
        unsigned hw = std::thread::hardware_concurrency();
        size_t T = cols.size() < 8 ? cols.size() : 8;
        if (hw && T > hw) T = hw;
        if ((size_t)n * cols.size() < 400000) T = 1;
        std::vector<std::thread> th;
        for (size_t t = 1; t < T; t++) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
    }
    return close_columns(a, L, pv, out);
}

namespace {

// the O(columns) closing steps on the column variances: the standard matrix keeps them; the expanded one takes
// averagePriorsOverLevels (R/expanded.R:20-73): a factor's level columns all get the mean of its level and contrast
// variances (summed in column order, the contrasts after the design columns); other columns keep theirs
static int close_columns(const DsqBetaPriorArgs *a, const Columns &L, const std::vector<double> &pv, double *out) {
    const int p = a->p, nfac = L.nfac;
    if (!a->expanded) {
        for (int c = 0; c < p; c++) out[c] = pv[c];
        return DSQ_OK;
    }
    std::vector<double> meanvar(nfac + 1, 0.0);
    for (int f = 1; f <= nfac; f++) {
        double s = 0.0;
        int k = 0;
        for (size_t c = 0; c < L.cols.size(); c++) if (L.col_factor[c] == f) { s += pv[c]; k++; }
        meanvar[f] = k ? s / (double)k : 0.0;
    }
    for (int j = 0; j < a->p_prior; j++) {
        const int f = a->prior_coef_factor[j];
        if (f == 0) out[j] = 1e6;
        else if (f > 0) out[j] = (f <= nfac) ? meanvar[f] : 0.0;
        else {
            const int s = a->prior_coef_src ? a->prior_coef_src[j] : -1;
            out[j] = (s >= 0 && s < p) ? pv[s] : 0.0;
        }
        if (!(out[j] > 0.0)) return capi_fail(DSQ_ERR_FIT, "beta prior is not greater than 0 (column %d of the expanded model matrix)", j);
    }
    return DSQ_OK;
}

}  // namespace

// ---- the device twin ----------------------------------------------------------------------------------
// The same definition on resident inputs:
//   1. once, for all columns: one wave per column walks the rows in ROW order -- |beta_i - beta_j| formed from the
//      coefficient-major matrix, never stored --, counts the rows under the |x| < 10 rule and the rows kept (not all zero,
//      |x| < 10, weight neither NaN nor 0) and carries sum(weights) over the kept rows.  The columns these counts decide
//      (1e6, NaN, the one-gene rule) are finished here.
//   then, a batch of columns at a time (the workspace is bounded in n x columns):
//   2. keys: a kept row gets the bit pattern of |x|, any other row the largest key, so the kept rows come first after the
//      sort, in the stable order of |x|;
//   3. the radix sort of results.hip over the batch's columns at once (radix_sort_columns), the row as payload;
//   4. the operands in sorted order: w N / wsum per sorted position (one thread each), into the sort's spare key buffer;
//   5. one wave per column carries the weight sum of each run of equal values from 0.0 and the runs' running total, then
//      the step function, the interpolation and (. / qnorm(0.975))^2.
// The order-sensitive sums of 1 and 5 are taken add for add as stated above: the lanes of the wave stage 64 operands (the
// next 64 are in flight meanwhile), the accumulator is wave-uniform -- per operand one v_readlane and one add, in index
// order, unrolled over the 64 lanes without a branch; no tree, no atomics on doubles.
constexpr int kBpvBatchMax = 64;                     // columns per batch
constexpr long kBpvBatchKeys = 1L << 21;             // keys per batch, as far as whole columns allow

struct BpvParams {
    int n, c0;                                       // rows; the first column of the batch
    const double *beta, *baseMean, *dispFit;
    const int32_t *allZero;
    const int2 *pairs;                               // per column: value = beta[, x] - (y >= 0 ? beta[, y] : 0)
    unsigned long long *keyA, *keyB;                 // the batch's buffers
    unsigned int *rowA, *rowB;
    unsigned int *kept;                              // per column: rows kept; 0: the column is finished (step 1)
    double *wsum;                                    // per column: sum(weights) over the kept rows
    unsigned int *nz;                                // the rows that are not all zero: how many, the first one
    double *pv;                                      // per column: the variance
    double prob;
};

DSQ_DEV double bpv_value(const BpvParams &kp, int2 pr, long g) {
    const double v = kp.beta[(long)kp.n * pr.x + g];
    return pr.y >= 0 ? v - kp.beta[(long)kp.n * pr.y + g] : v;
}
DSQ_DEV double bpv_weight(const BpvParams &kp, long g) { return 1.0 / (1.0 / kp.baseMean[g] + kp.dispFit[g]); }
// useFinite (a NaN is not < 10) on the rows that are not all zero; then Hmisc drops a weight that is NaN or 0
DSQ_DEV void bpv_row(const BpvParams &kp, int2 pr, long g, double *w, bool *use, bool *kept) {
    *w = 0.0; *use = false; *kept = false;
    if (g >= kp.n) return;
    *w = bpv_weight(kp, g);
    *use = !kp.allZero[g] && fabs(bpv_value(kp, pr, g)) < 10.0;
    *kept = *use && !(*w != *w || *w == 0.0);
}

__global__ void __launch_bounds__(256) bpv_rows_kernel(const int32_t *allZero, int n, unsigned int *nz) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < n && !allZero[g];
    const unsigned long long b = __ballot(live);
    if (b && (threadIdx.x & 63) == __ffsll((long long)b) - 1) {
        atomicAdd(&nz[0], (unsigned int)__popcll(b));
        atomicMin(&nz[1], (unsigned int)g);
    }
}

// step 1: grid = all columns, one wave each
__global__ void __launch_bounds__(64) bpv_wsum_kernel(BpvParams kp) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int2 pr = kp.pairs[c];
    if (kp.nz[0] == 1u) {                                // a one-gene object: (betaMatrix)^2
        if (lane == 0) { const double v = bpv_value(kp, pr, kp.nz[1]); kp.pv[c] = v * v; kp.kept[c] = 0u; }
        return;
    }
    double w, wsum = 0.0;
    bool use, kept;
    unsigned int n_use = 0u, n_kept = 0u;
    bpv_row(kp, pr, lane, &w, &use, &kept);
    for (long base = 0; base < kp.n; base += 64) {
        double w1;
        bool use1, kept1;
        bpv_row(kp, pr, base + 64 + lane, &w1, &use1, &kept1);           // in flight while this chunk is summed
        n_use += (unsigned int)__popcll(__ballot(use));
        n_kept += (unsigned int)__popcll(__ballot(kept));
        // sum(weights), in row order.  A row that is not kept contributes +0.0, which changes no bit of the sum: the
        // accumulator starts at +0.0 and a sum rounds to -0.0 only from two -0.0 operands, so it is never -0.0, and
        // x + 0.0 == x for every other x (NaN and Inf included).  No branch: 64 x (v_readlane, add).
        const double wk = kept ? w : 0.0;
#pragma unroll
        for (int l = 0; l < 64; l++) wsum += lane_read(wk, l);
        w = w1; use = use1; kept = kept1;
    }
    if (lane != 0) return;
    if (n_use == 0u) { kp.pv[c] = 1e6; kp.kept[c] = 0u; }                                     // R/core.R:1652-1653
    else if (n_kept == 0u) { kp.pv[c] = __longlong_as_double(0x7ff8000000000000LL); kp.kept[c] = 0u; }
    else { kp.kept[c] = n_kept; kp.wsum[c] = wsum; }
}

// step 2: grid = (row blocks, the batch's columns)
__global__ void __launch_bounds__(256) bpv_keys_kernel(BpvParams kp) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= kp.n) return;
    const int2 pr = kp.pairs[kp.c0 + blockIdx.y];
    double w;
    bool use, kept;
    bpv_row(kp, pr, g, &w, &use, &kept);
    const long e = (long)blockIdx.y * kp.n + g;
    kp.keyA[e] = kept ? (unsigned long long)__double_as_longlong(fabs(bpv_value(kp, pr, g))) : ~0ull;
    kp.rowA[e] = (unsigned int)g;
}

// step 4: weights * length(x) / sum(weights) of the row at each sorted position, into the spare key buffer
__global__ void __launch_bounds__(256) bpv_stage_kernel(BpvParams kp) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = kp.c0 + blockIdx.y;
    const long N = kp.kept[c];
    if (k >= N) return;
    const long e = (long)blockIdx.y * kp.n + k;
    ((double *)kp.keyB)[e] = bpv_weight(kp, kp.rowA[e]) * (double)N / kp.wsum[c];
}

// step 5: grid = the batch's columns, one wave each
__global__ void __launch_bounds__(64) bpv_column_kernel(BpvParams kp) {
    const int c = kp.c0 + blockIdx.x, lane = threadIdx.x;
    const long N = kp.kept[c];
    if (N == 0) return;
    const long col0 = (long)blockIdx.x * kp.n;
    const unsigned long long *key = kp.keyA + col0;
    double *cs = (double *)(kp.keyB + col0);             // in: the operands; out: the running total at the end of run d (d <= k)
    unsigned int *ends = kp.rowB + col0;                 // sorted position of the end of run d (its value: key[ends[d]])
    auto stage = [&](long k, double *wn, bool *last) {
        *wn = 0.0; *last = false;
        if (k < N) { *wn = cs[k]; *last = k + 1 == N || key[k + 1] != key[k]; }
    };
    double run = 0.0, tot = 0.0, wn;
    bool last;
    int D = 0;
    stage(lane, &wn, &last);
    for (long base = 0; base < N; base += 64) {
        double wn1;
        bool last1;
        stage(base + 64 + lane, &wn1, &last1);           // in flight while this chunk is summed
        const unsigned long long ends_here = __ballot(last);
        double my_cs = 0.0;                              // lane l: the total and the run index at position base + l
        int my_d = 0;
        // no branch: 64 x (v_readlane, add, and at a run's end -- a wave-uniform select -- the add into the total).  The
        // positions past N in the last chunk hold +0.0 and no run end: they touch `run` after its last use only.
#pragma unroll
        for (int l = 0; l < 64; l++) {
            run += lane_read(wn, l);
            const bool end = (ends_here >> l) & 1ull;
            const double t = tot + run;
            tot = end ? t : tot;
            run = end ? 0.0 : run;
            int lv = lane;
            asm volatile("" : "+v"(lv));                 // (keeps the 64 lane masks from being hoisted out of the chunk loop)
            if (lv == l) { my_cs = tot; my_d = D; }
            D += end ? 1 : 0;
        }
        if (last) { cs[my_d] = my_cs; ends[my_d] = (unsigned int)(base + lane); }       // (my_d <= base + lane: read already)
        wn = wn1; last = last1;
    }
    __threadfence_block();
    __syncthreads();
    if (lane != 0) return;
    const double n_eff = tot;
    const double order = 1.0 + (n_eff - 1.0) * kp.prob;
    const double fl = floor(order);
    const double low = fl > 1.0 ? fl : 1.0;
    const double high = (low + 1.0 < n_eff) ? low + 1.0 : n_eff;
    const double frac = fmod(order, 1.0);
    double q[2] = {low, high}, ux[2];
    for (int t = 0; t < 2; t++) {                        // approx(cumsum(wts), x, method = "constant", f = 1, rule = 2)
        int lo = 0, hi = D;
        while (lo < hi) { const int mid = (lo + hi) / 2; if (cs[mid] < q[t]) lo = mid + 1; else hi = mid; }
        ux[t] = __longlong_as_double((long long)key[ends[lo < D ? lo : D - 1]]);
    }
    const double sd = ((1.0 - frac) * ux[0] + frac * ux[1]) / kQnorm975;
    kp.pv[c] = sd * sd;
}

static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }
static int bpv_batch(long n, long columns) {
    long B = kBpvBatchKeys / (n > 0 ? n : 1);
    if (B < 1) B = 1;
    if (B > kBpvBatchMax) B = kBpvBatchMax;
    return (int)(B < columns ? B : (columns > 0 ? columns : 1));
}

// the batch: keys A, B | rows A, B | the (digit, tile) tables | copy flags;  then nz | per column: pair, kept, wsum, variance
size_t beta_prior_workspace_bytes(long n, long columns) {
    const size_t B = bpv_batch(n, columns);
    return 2 * B * (size_t)n * 8 + 2 * pad8(B * (size_t)n * 4) + pad8(B * sort_hist_entries(n) * 4) + pad8(B * 4) + 8
           + (size_t)columns * 8 + pad8((size_t)columns * 4) + 2 * (size_t)columns * 8;
}

namespace {
struct SyncOnExit {                                      // an early return leaves no copy from this frame's memory in flight
    hipStream_t st;
    ~SyncOnExit() { (void)hipStreamSynchronize(st); }
};
}  // namespace

int beta_prior_var_dev(const DsqBetaPriorArgs *a, double *out, void *workspace, int64_t workspace_bytes, hipStream_t st) {
    const Columns L = list_columns(a);
    std::vector<int> todo;                               // (the intercept is not matched: 1e6, R/core.R:1669-1671)
    std::vector<double> pv(L.cols.size(), 0.0);
    for (size_t c = 0; c < L.cols.size(); c++) {
        if (L.cols[c].j < 0 && a->coef_factor[L.cols[c].i] == 0) pv[c] = 1e6;
        else todo.push_back((int)c);
    }
    const size_t need = beta_prior_workspace_bytes(a->n, (long)L.cols.size());
    if (!workspace || workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes: %zu are needed (dsq_beta_prior_var_workspace_bytes)",
                         (long long)workspace_bytes, need);
    if (todo.empty()) return close_columns(a, L, pv, out);
    if (int rc = capi_check_device()) return rc;
    const size_t n = a->n, columns = L.cols.size(), B = bpv_batch(a->n, (long)columns);
    BpvParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = a->n; kp.beta = a->mle_beta; kp.baseMean = a->baseMean; kp.dispFit = a->dispFit; kp.allZero = a->allZero;
    kp.prob = 1.0 - a->upperQuantile;
    char *w = (char *)workspace;
    kp.keyA = (unsigned long long *)w;  w += B * n * 8;
    kp.keyB = (unsigned long long *)w;  w += B * n * 8;
    kp.rowA = (unsigned int *)w;        w += pad8(B * n * 4);
    kp.rowB = (unsigned int *)w;        w += pad8(B * n * 4);
    unsigned int *hist = (unsigned int *)w;          w += pad8(B * sort_hist_entries(a->n) * 4);
    unsigned int *const_digit = (unsigned int *)w;   w += pad8(B * 4);
    kp.nz = (unsigned int *)w;          w += 8;
    int2 *pairs_d = (int2 *)w;          w += columns * 8;
    kp.pairs = pairs_d;
    kp.kept = (unsigned int *)w;        w += pad8(columns * 4);
    kp.wsum = (double *)w;              w += columns * 8;
    kp.pv = (double *)w;
    std::vector<int2> pairs(todo.size());
    for (size_t k = 0; k < todo.size(); k++) pairs[k] = make_int2(L.cols[todo[k]].i, L.cols[todo[k]].j);
    std::vector<double> got(todo.size());
    SyncOnExit guard{st};
    DSQ_HIP(hipMemcpyAsync(pairs_d, pairs.data(), todo.size() * 8, hipMemcpyHostToDevice, st));
    DSQ_HIP(hipMemsetAsync(kp.nz, 0, 4, st));
    DSQ_HIP(hipMemsetAsync(kp.nz + 1, 0xff, 4, st));
    const int gblocks = (int)((n + 255) / 256);
    hipLaunchKernelGGL(bpv_rows_kernel, dim3(gblocks), dim3(256), 0, st, a->allZero, a->n, kp.nz);
    hipLaunchKernelGGL(bpv_wsum_kernel, dim3((unsigned)todo.size()), dim3(64), 0, st, kp);
    for (size_t c0 = 0; c0 < todo.size(); c0 += B) {
        const int nb = (int)(todo.size() - c0 < B ? todo.size() - c0 : B);
        kp.c0 = (int)c0;
        hipLaunchKernelGGL(bpv_keys_kernel, dim3(gblocks, nb), dim3(256), 0, st, kp);
        radix_sort_columns(kp.keyA, kp.keyB, kp.rowA, kp.rowB, hist, const_digit, a->n, nb, st);
        hipLaunchKernelGGL(bpv_stage_kernel, dim3(gblocks, nb), dim3(256), 0, st, kp);
        hipLaunchKernelGGL(bpv_column_kernel, dim3(nb), dim3(64), 0, st, kp);
    }
    DSQ_HIP(hipGetLastError());
    DSQ_HIP(hipMemcpyAsync(got.data(), kp.pv, todo.size() * 8, hipMemcpyDeviceToHost, st));
    DSQ_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < todo.size(); k++) pv[todo[k]] = got[k];
    return close_columns(a, L, pv, out);
}

}  // namespace dsq

static int beta_prior_check(const DsqBetaPriorArgs *a, const char *who) {
    using namespace dsq;
    if (a->n < 1 || a->p < 1 || !a->mle_beta || !a->baseMean || !a->dispFit || !a->allZero || !a->coef_factor)
        return capi_fail(DSQ_ERR_ARG, "%s: NULL input or bad dimensions", who);
    if (a->expanded && (a->p_prior < 1 || !a->prior_coef_factor)) return capi_fail(DSQ_ERR_ARG, "expanded model matrix: p_prior / prior_coef_factor");
    if (!(a->upperQuantile > 0.0 && a->upperQuantile < 1.0)) return capi_fail(DSQ_ERR_ARG, "upperQuantile");
    if (a->upperQuantile != 0.05) return capi_fail(DSQ_ERR_UNSUPPORTED, "upperQuantile = %g: only the default 0.05 (qnorm(0.975) is a constant here)", a->upperQuantile);
    return DSQ_OK;
}

extern "C" int dsq_beta_prior_var_dev(const DsqBetaPriorArgs *a, double *betaPriorVar, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    using namespace dsq;
    if (!a || !betaPriorVar) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (int rc = beta_prior_check(a, "dsq_beta_prior_var_dev")) return rc;
    if (a->p > 32767) return capi_fail(DSQ_ERR_UNSUPPORTED, "p = %d columns: at most 32767", a->p);
    return beta_prior_var_dev(a, betaPriorVar, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int32_t dsq_beta_prior_var_columns(const DsqBetaPriorArgs *a) {
    if (!a || a->n < 1 || a->p < 1 || !a->coef_factor) return 0;
    return (int32_t)dsq::list_columns(a).cols.size();
}

extern "C" int64_t dsq_beta_prior_var_workspace_bytes(int32_t n, int32_t columns) {
    if (n < 1 || columns < 1) return 0;
    return (int64_t)dsq::beta_prior_workspace_bytes(n, columns);
}

extern "C" int dsq_beta_prior_var(const DsqBetaPriorArgs *a, double *betaPriorVar) {
    using namespace dsq;
    if (!a || !betaPriorVar) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (int rc = beta_prior_check(a, "dsq_beta_prior_var")) return rc;
    return beta_prior_var(a, betaPriorVar);
}
