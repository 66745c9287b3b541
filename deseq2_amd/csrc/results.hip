// results.hip -- results() on the device.
//
// R/results.R:443-575 and :638-740 for one coefficient, without contrasts:
//   1. the table: column c of beta / betaSE / statistic / p-value (or LRTStatistic / LRTPvalue), the threshold tests of
//      :484-515 under the normal distribution, pvalue NA where the caller's mask says so (:564), the nowZero fill (:567-575);
//      one thread per gene.
//   2. cutoffs = quantile(filter, theta), type 7, from the sorted filter; K threads.
//   3. filtered_p (:721-740) with p.adjust(., "BH"): R runs one adjustment per cutoff over `filter >= cutoff`.  All K share
//      ONE ascending sort of the non-NA p-values: for a cutoff, r = the inclusive count of used rows up to a sorted
//      position, mS = their number, v = (mS / r) p on the used rows, padj = pmin(1, suffix minimum of v).  Integer counts
//      and min are exact in any order, so the result equals the K separate adjustments bit for bit.  One 1024-thread
//      workgroup per cutoff walks the sorted order in chunks of 4096 (four positions per thread) from the END: a count
//      pass gives mS; then per chunk one block scan gives the used rows behind a position (r = what is left before the
//      chunk's end minus those), a second one the running minimum, both carried from chunk to chunk.  The filter
//      statistic is gathered into the sorted order once, for all cutoffs.
// The sort: 64-bit order-preserving keys (order_key, NaN -> the largest key, counted) with an optional 32-bit row payload,
// least-significant-digit radix, 8 bits per pass: per pass a histogram per tile of 2048 keys, one exclusive scan of the
// (digit, tile) table, and a scatter that ranks the keys of a tile stably (wave ballots per digit bit, the waves of a
// workgroup in order through LDS).  A pass whose digit is the same for every key only copies.  Deterministic: no
// float atomics, integer atomics only into counts.
#include "dsq_internal.hpp"
#include "dsq_math.hpp"

namespace dsq {

constexpr int kSortThreads = 256, kSortItems = 8, kSortTile = kSortThreads * kSortItems;
constexpr int kBhThreads = 1024;
enum { CNT_NAN_FILTER = 0, CNT_NAN_P = 1, CNT_CONST_DIGIT = 2, CNT_COUNT = 16 };

// ---- 1. the table --------------------------------------------------------------------------------------------------------
// R's pmax / pmin on doubles (na.rm = FALSE): NA if either is, else the second unless the first is larger / smaller
DSQ_DEV double r_pmax(double a, double b) { return (a != a || b != b) ? dnan() : (a > b ? a : b); }
DSQ_DEV double r_pmin(double a, double b) { return (a != a || b != b) ? dnan() : (a < b ? a : b); }
DSQ_DEV double r_sign(double v) { return v != v ? v : (v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0)); }
// pnorm(x, mean = 0, sd = se) with pnorm5's rules around the quotient
DSQ_DEV double pnorm_sd(double x, double se) {
    if (x != x || se != se || se < 0.0) return dnan();
    const double q = x / se;
    if (se == 0.0 || !dfinite(q)) return x < 0.0 ? 0.0 : 1.0;
    return dpnorm_lower(q);
}

// the same five tests with pt(., df) in place of pnorm (R/results.R:477-515 under useT): plain quotients -- pnorm_sd's rules
// about sd belong to pnorm5 --, gene i with df[i] (the diagonal of what the reference's greaterAbs branch returns, DESIGN.md
// section 15); a NaN df gives a NaN p-value
DSQ_DEV void threshold_tests_t(int alt, double lfc, double se, double T, double df, double &stat, double &pv) {
    switch (alt) {
    case 0: {
        stat = lfc / se;
        const double a = -__builtin_fabs(lfc) + T, b = -__builtin_fabs(lfc) - T;
        pv = dpt_lower(a / se, df) + dpt_lower(b / se, df);
        break;
    }
    case 4: {
        const double q = (__builtin_fabs(lfc) - T) / se;
        stat = r_sign(lfc) * r_pmax(q, 0.0);
        pv = r_pmin(1.0, 2.0 * dpt_upper(q, df));
        break;
    }
    case 1: {
        const double qa = (T - lfc) / se, qb = (lfc + T) / se;
        stat = r_pmin(r_pmax(qa, 0.0), r_pmax(qb, 0.0));
        pv = r_pmax(dpt_upper(qa, df), dpt_upper(qb, df));
        break;
    }
    case 2: {
        const double q = (lfc - T) / se;
        stat = r_pmax(q, 0.0);
        pv = dpt_upper(q, df);
        break;
    }
    default: {
        stat = r_pmin((lfc + T) / se, 0.0);
        pv = dpt_upper((-T - lfc) / se, df);
        break;
    }
    }
}

// kT: the threshold tests under Student's t with kp.df (launched only when df is given and a threshold test is asked for)
template <bool kT>
__global__ void __launch_bounds__(256) results_table_kernel(ResultsKernelParams kp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kp.n) return;
    const long ic = i + (long)kp.n * kp.c;
    double lfc = kp.beta[ic], se = kp.betaSE[ic];
    double stat = kp.lrt ? kp.stat[i] : kp.stat[ic];
    double pv = kp.lrt ? kp.pvalue[i] : kp.pvalue[ic];
    const double bm = kp.baseMean[i];
    if (kp.threshold) {
        const double T = kp.T;
        if constexpr (kT) threshold_tests_t(kp.alt, lfc, se, T, kp.df[i], stat, pv);
        else
        switch (kp.alt) {
        case 0: {   // greaterAbs (:484-497)
            stat = lfc / se;
            const double a = -__builtin_fabs(lfc) + T, b = -__builtin_fabs(lfc) - T;
            pv = pnorm_sd(a, se) + pnorm_sd(b, se);
            break;
        }
        case 4: {   // greaterAbs2014 (:498-501)
            const double q = (__builtin_fabs(lfc) - T) / se;
            stat = r_sign(lfc) * r_pmax(q, 0.0);
            pv = r_pmin(1.0, 2.0 * dpnorm_upper(q));
            break;
        }
        case 1: {   // lessAbs (:502-508)
            const double qa = (T - lfc) / se, qb = (lfc + T) / se;
            stat = r_pmin(r_pmax(qa, 0.0), r_pmax(qb, 0.0));
            pv = r_pmax(dpnorm_upper(qa), dpnorm_upper(qb));
            break;
        }
        case 2: {   // greater (:509-511)
            const double q = (lfc - T) / se;
            stat = r_pmax(q, 0.0);
            pv = dpnorm_upper(q);
            break;
        }
        default: {  // less (:512-514)
            stat = r_pmin((lfc + T) / se, 0.0);
            pv = dpnorm_upper((-T - lfc) / se);
            break;
        }
        }
    }
    if (kp.na_mask && kp.na_mask[i] != 0) pv = dnan();                                  // :564
    if (kp.replace && kp.replace[i] == 1 && bm == 0.0) { lfc = 0.0; se = 0.0; stat = 0.0; pv = 1.0; }   // :567-575 (NA: not filled)
    kp.o_baseMean[i] = bm; kp.o_lfc[i] = lfc; kp.o_se[i] = se; kp.o_stat[i] = stat; kp.o_pvalue[i] = pv;
}

// ---- 2. the sort ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sort_keys_kernel(const double *v, int n, unsigned long long *key, unsigned int *row,
                                                        unsigned int *nan_count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = v[i];
    const bool isnan = d != d;
    key[i] = isnan ? ~0ull : order_key(d);
    if (row) row[i] = (unsigned int)i;
    if (isnan) atomicAdd(nan_count, 1u);
}

// The three pass kernels sort blockIdx.y INDEPENDENT columns of n keys each (radix_sort_columns; results() has one):
// column c's keys (and rows) start c n entries into their arrays, its table 256 nblk entries into hist, its copy flag is
// const_digit[c].
// hist[digit * nblk + tile]: the keys of the tile with that digit
__global__ void __launch_bounds__(kSortThreads) sort_hist_kernel(const unsigned long long *key, int n, int shift,
                                                                 unsigned int *hist, int nblk) {
    __shared__ unsigned int h[256];
    key += (long)blockIdx.y * n;
    hist += (long)blockIdx.y * 256 * nblk;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const long base = (long)blockIdx.x * kSortTile;
    for (int it = 0; it < kSortItems; it++) {
        const long i = base + it * kSortThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(unsigned)((key[i] >> shift) & 255ull)], 1u);
    }
    __syncthreads();
    hist[(long)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// inclusive sum over the 1024 threads of a workgroup (wave shuffles, then the 16 wave totals through LDS); *total: the sum
DSQ_DEV unsigned int block_inclusive_sum(unsigned int x, unsigned int *lds16, unsigned int *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(x, off, 64);
        if (lane >= off) x += t;
    }
    __syncthreads();                     // (the table may still be read from the call before)
    if (lane == 63) lds16[wave] = x;
    __syncthreads();
    unsigned int before = 0u, all = 0u;
    for (int w = 0; w < nwave; w++) {
        const unsigned int t = lds16[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return x + before;
}

// exclusive scan of the table in (digit, tile) order, in place: one workgroup, a contiguous piece per thread.  Sets
// *const_digit when one digit holds every key (the scatter then only copies).
__global__ void __launch_bounds__(kBhThreads) sort_scan_kernel(unsigned int *hist, int nblk, int n, unsigned int *const_digit) {
    __shared__ unsigned int lds16[16];
    const long total = 256L * nblk;
    hist += (long)blockIdx.y * total;
    const_digit += blockIdx.y;
    const long per = (total + kBhThreads - 1) / kBhThreads;
    const long lo = (long)threadIdx.x * per, hi = lo + per < total ? lo + per : total;
    unsigned int s = 0u;
    for (long e = lo; e < hi; e++) s += hist[e];
    unsigned int all;
    unsigned int run = block_inclusive_sum(s, lds16, &all) - s;
    for (long e = lo; e < hi; e++) {
        const unsigned int h = hist[e];
        hist[e] = run;
        run += h;
    }
    if (threadIdx.x == 0) *const_digit = 0u;
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < 256) {
        const unsigned int first = hist[(long)threadIdx.x * nblk];
        const unsigned int next = threadIdx.x == 255 ? (unsigned int)n : hist[(long)(threadIdx.x + 1) * nblk];
        if (next - first == (unsigned int)n) *const_digit = 1u;
    }
}

__global__ void __launch_bounds__(kSortThreads) sort_scatter_kernel(const unsigned long long *kin, const unsigned int *rin,
                                                                    unsigned long long *kout, unsigned int *rout, int n,
                                                                    int shift, const unsigned int *offs, int nblk,
                                                                    const unsigned int *const_digit) {
    __shared__ unsigned int base[256];
    __shared__ unsigned int wcnt[kSortThreads / 64][256];
    const long tile0 = (long)blockIdx.x * kSortTile;
    {
        const long col0 = (long)blockIdx.y * n;
        kin += col0; kout += col0;
        if (rin) { rin += col0; rout += col0; }
        offs += (long)blockIdx.y * 256 * nblk;
    }
    if (const_digit[blockIdx.y]) {                          // (uniform over the column's blocks)
        for (int it = 0; it < kSortItems; it++) {
            const long i = tile0 + it * kSortThreads + threadIdx.x;
            if (i < n) { kout[i] = kin[i]; if (rin) rout[i] = rin[i]; }
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    base[threadIdx.x] = offs[(long)threadIdx.x * nblk + blockIdx.x];
    for (int it = 0; it < kSortItems; it++) {
        for (int w = 0; w < kSortThreads / 64; w++) wcnt[w][threadIdx.x] = 0u;
        __syncthreads();
        const long i = tile0 + it * kSortThreads + threadIdx.x;
        const bool valid = i < n;
        const unsigned long long key = valid ? kin[i] : 0ull;
        const unsigned int d = (unsigned int)((key >> shift) & 255ull);
        // the lanes of this wave that hold the same digit
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned int rank = (unsigned int)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wcnt[wave][d] = (unsigned int)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned int pos = base[d] + rank;
            for (int w = 0; w < wave; w++) pos += wcnt[w][d];
            kout[pos] = key;
            if (rin) rout[pos] = rin[i];
        }
        __syncthreads();
        unsigned int add = 0u;
        for (int w = 0; w < kSortThreads / 64; w++) add += wcnt[w][threadIdx.x];
        base[threadIdx.x] += add;
        __syncthreads();
    }
}

// ---- 3. the cutoffs ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) results_quantile_kernel(ResultsKernelParams kp) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kp.K) return;
    if (!kp.theta) { kp.cutoffs[k] = -kInf; return; }
    if (k == 0 && kp.counters[CNT_NAN_FILTER] != 0u) atomicOr(kp.status, 1);
    const double t = kp.theta[k];
    if (!(t >= 0.0 && t <= 1.0)) { atomicOr(kp.status, 2); kp.cutoffs[k] = dnan(); return; }
    const double h = (double)(kp.n - 1) * t;
    const double fl = __builtin_floor(h);
    long lo = (long)fl, hi = (long)__builtin_ceil(h);
    if (hi > kp.n - 1) hi = kp.n - 1;
    if (lo > kp.n - 1) lo = kp.n - 1;
    const double g = h - fl;
    const double a = order_unkey(kp.keyA[lo]), b = order_unkey(kp.keyA[hi]);
    kp.cutoffs[k] = (g == 0.0 || b == a) ? a : (1.0 - g) * a + g * b;
}

// ---- 4. Benjamini-Hochberg over the K nested subsets -----------------------------------------------------------------------
// the filter statistic in the sorted order of the p-values, once for all cutoffs (into the sort's spare key buffer)
__global__ void __launch_bounds__(256) results_gather_kernel(ResultsKernelParams kp, double *fs) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < kp.n) fs[s] = kp.filter[kp.rowA[s]];
}

// minimum over the threads BEFORE this one (+Inf for thread 0); *total: the minimum over all
DSQ_DEV double block_exclusive_min(double x, double *lds16, double *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(x, off, 64);
        if (lane >= off && t < x) x = t;
    }
    const double prev = __shfl_up(x, 1, 64);
    __syncthreads();
    if (lane == 63) lds16[wave] = x;
    __syncthreads();
    double before = lane == 0 ? kInf : prev, all = kInf;
    for (int w = 0; w < nwave; w++) {
        const double t = lds16[w];
        if (w < wave && t < before) before = t;
        if (t < all) all = t;
    }
    *total = all;
    return before;
}

constexpr int kBhItems = 4, kBhChunk = kBhThreads * kBhItems;

__global__ void __launch_bounds__(kBhThreads) results_bh_kernel(ResultsKernelParams kp, const double *fs) {
    __shared__ unsigned int lds_u[16];
    __shared__ double lds_d[16];
    const int k = blockIdx.x;
    const long n = kp.n;
    const long nv = n - (long)kp.counters[CNT_NAN_P];       // the sorted positions [0, nv) hold the non-NA p-values
    const bool filtering = kp.theta != nullptr;
    const double cutoff = kp.cutoffs[k];
    double *out = kp.filtPadj + n * k;
    // rows with an NA p-value
    for (long s = nv + threadIdx.x; s < n; s += kBhThreads) out[kp.rowA[s]] = dnan();
    // mS
    unsigned int mine = 0u;
    for (long s = threadIdx.x; s < nv; s += kBhThreads)
        if (!filtering || fs[s] >= cutoff) mine++;
    unsigned int mS;
    block_inclusive_sum(mine, lds_u, &mS);
    const double dmS = (double)mS;
    unsigned int left = mS;            // used rows at the positions before the end of the current chunk
    double carry = kInf;               // minimum of v over the chunks behind
    unsigned int rej = 0u;
    const long nchunk = (nv + kBhChunk - 1) / kBhChunk;
    for (long c = nchunk - 1; c >= 0; c--) {
        // thread t, item j take the position kBhChunk - 1 - (kBhItems t + j) of the chunk: "behind a position" is "an earlier
        // item of this thread or any item of a thread before it"
        const long s0 = c * kBhChunk + (kBhChunk - 1 - (long)kBhItems * threadIdx.x);
        unsigned int row[kBhItems];
        double p[kBhItems];
        bool use[kBhItems];
        unsigned int own = 0u;
        for (int j = 0; j < kBhItems; j++) {
            const long s = s0 - j;
            use[j] = false; row[j] = 0u; p[j] = 0.0;
            if (s < nv) {
                row[j] = kp.rowA[s];
                p[j] = order_unkey(kp.keyA[s]);
                use[j] = !filtering || fs[s] >= cutoff;
            }
            own += use[j] ? 1u : 0u;
        }
        unsigned int cnt;
        unsigned int behind = block_inclusive_sum(own, lds_u, &cnt) - own;     // used rows of the threads before this one
        double v[kBhItems], tmin = kInf;
        for (int j = 0; j < kBhItems; j++) {
            const unsigned int r = left - behind;                              // inclusive rank of the position among the used rows
            v[j] = use[j] ? (dmS / (double)r) * p[j] : kInf;
            if (use[j]) behind++;
            if (v[j] < tmin) tmin = v[j];
        }
        double cmin;
        double m = block_exclusive_min(tmin, lds_d, &cmin);
        if (carry < m) m = carry;
        for (int j = 0; j < kBhItems; j++) {
            if (v[j] < m) m = v[j];
            if (s0 - j < nv) {
                const double padj = m < 1.0 ? m : 1.0;
                out[row[j]] = use[j] ? padj : dnan();
                if (use[j] && padj < kp.alpha) rej++;
            }
        }
        if (cmin < carry) carry = cmin;
        left -= cnt;
    }
    unsigned int nrej;
    block_inclusive_sum(rej, lds_u, &nrej);
    if (threadIdx.x == 0) kp.numRej[k] = (int32_t)nrej;
}

// ---- launch ----------------------------------------------------------------------------------------------------------------
static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }
static int sort_tiles(long n) { return (int)((n + kSortTile - 1) / kSortTile); }

size_t results_sort_workspace_bytes(long n) {
    // keys A, B (n u64 each) | rows A, B (n u32 each) | the (digit, tile) table | counters
    return 2 * (size_t)n * 8 + 2 * pad8((size_t)n * 4) + (size_t)256 * sort_tiles(n) * 4 + CNT_COUNT * 4;
}

size_t sort_hist_entries(long n) { return (size_t)256 * sort_tiles(n); }

// sorts each of the ncols columns of keyA (and rowA, unless nullptr) ascending; 8 passes A -> B -> A ..., so the result is
// back in A
void radix_sort_columns(unsigned long long *ka, unsigned long long *kb, unsigned int *ra, unsigned int *rb, unsigned int *hist,
                        unsigned int *const_digit, int n, int ncols, hipStream_t st) {
    const int nblk = sort_tiles(n);
    for (int pass = 0; pass < 8; pass++) {
        const int shift = 8 * pass;
        hipLaunchKernelGGL(sort_hist_kernel, dim3(nblk, ncols), dim3(kSortThreads), 0, st, ka, n, shift, hist, nblk);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(1, ncols), dim3(kBhThreads), 0, st, hist, nblk, n, const_digit);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3(nblk, ncols), dim3(kSortThreads), 0, st, ka, ra, kb, rb, n, shift, hist, nblk,
                           const_digit);
        unsigned long long *tk = ka; ka = kb; kb = tk;
        unsigned int *tr = ra; ra = rb; rb = tr;
    }
}

static void radix_sort(const ResultsKernelParams &kp, bool with_rows, hipStream_t st) {
    radix_sort_columns(kp.keyA, kp.keyB, with_rows ? kp.rowA : nullptr, with_rows ? kp.rowB : nullptr, kp.hist,
                       kp.counters + CNT_CONST_DIGIT, kp.n, 1, st);
}

// carves the caller's workspace (results_sort_workspace_bytes) and enqueues the chain
hipError_t launch_results(ResultsKernelParams kp, void *workspace, hipStream_t st) {
    const size_t n = kp.n;
    char *w = (char *)workspace;
    kp.keyA = (unsigned long long *)w;   w += n * 8;
    kp.keyB = (unsigned long long *)w;   w += n * 8;
    kp.rowA = (unsigned int *)w;         w += pad8(n * 4);
    kp.rowB = (unsigned int *)w;         w += pad8(n * 4);
    kp.hist = (unsigned int *)w;         w += (size_t)256 * sort_tiles(kp.n) * 4;
    kp.counters = (unsigned int *)w;
    hipError_t e = hipMemsetAsync(kp.counters, 0, CNT_COUNT * 4, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(kp.status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const int gblocks = (kp.n + 255) / 256;
    if (kp.df && kp.threshold) hipLaunchKernelGGL(results_table_kernel<true>, dim3(gblocks), dim3(256), 0, st, kp);
    else hipLaunchKernelGGL(results_table_kernel<false>, dim3(gblocks), dim3(256), 0, st, kp);
    if (kp.theta) {
        hipLaunchKernelGGL(sort_keys_kernel, dim3(gblocks), dim3(256), 0, st, kp.filter, kp.n, kp.keyA, (unsigned int *)nullptr,
                           kp.counters + CNT_NAN_FILTER);
        radix_sort(kp, false, st);
    }
    hipLaunchKernelGGL(results_quantile_kernel, dim3((kp.K + 255) / 256), dim3(256), 0, st, kp);
    hipLaunchKernelGGL(sort_keys_kernel, dim3(gblocks), dim3(256), 0, st, (const double *)kp.o_pvalue, kp.n, kp.keyA, kp.rowA,
                       kp.counters + CNT_NAN_P);
    radix_sort(kp, true, st);
    double *fs = (double *)kp.keyB;                                        // (8 passes: the sorted keys are in A, B is free)
    if (kp.theta) hipLaunchKernelGGL(results_gather_kernel, dim3(gblocks), dim3(256), 0, st, kp, fs);
    hipLaunchKernelGGL(results_bh_kernel, dim3(kp.K), dim3(kBhThreads), 0, st, kp, (const double *)fs);
    return hipGetLastError();
}

}  // namespace dsq
