// pipeline.hip -- dsq_deseq_dev: the whole DESeq() chain driven from the device (include/deseq2_mi355x.h).
//
// The reference's R code between the native calls is per-gene arithmetic on n-vectors (clamps, accept /
// convergence / refit rules: R/core.R:727-728, 785, 826-848, 1019-1024, 1048-1063, 1099-1115; betaConv, log2
// rescaling, Wald statistic: R/fitNbinomGLMs.R:185-198, R/core.R:1471,1507) plus two all-gene steps
// (parametricDispersionFit R/core.R:2166-2190, mad of the log residuals R/methods.R:180).  Here each rule is a
// small elementwise kernel, the rows a rule sends on (fitDispGrid stragglers, replaced-outlier rows) are
// compacted on the device and fitted by ROW-LISTED launches of the same fit kernels (DispKernelParams::rows /
// n_dev), and the all-gene steps are kernels of one or sixteen workgroups (trend.hip), so a phase is one uninterrupted
// stream of launches: no host decision, no device-to-host copy.  Every formula is evaluated with the operations of the
// host mirror (deseq2_amd/core.py: IEEE + - * / sqrt, the engine's dlog / dexp, numpy's NaN-propagating
// minimum / maximum), so the results equal the call-by-call chain bit for bit (tests/test_gpu_fused.py).
#include "capi.hpp"
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace dsq {

// numpy.minimum / numpy.maximum: NaN if either operand is NaN
DSQ_DEV double np_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }
DSQ_DEV double np_max(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

struct Rows {                 // the genes a rule kernel covers: rows[0 .. *n_dev) or 0 .. n-1
    const int32_t *rows;
    const int32_t *n_dev;
    int n;
};
DSQ_DEV int rows_count(const Rows &r) { return r.n_dev ? *r.n_dev : r.n; }
DSQ_DEV int rows_gene(const Rows &r, int i) { return r.rows ? r.rows[i] : i; }

// ---- ordered compaction on many workgroups (the trend fit sums its input in index order) -----------------------
// mode 0: keep = !(allZero | force_zero) -> rows; also folds force_zero into allZero
// mode 1: keep = disp > thresh -> (means, disps) pairs (useForFit, R/core.R:870)
// Tiles of kCompactTile consecutive elements, one workgroup each, in TWO launches: the first counts the kept elements of
// every tile (tile_cnt: one int per tile), the second adds up the counts of the tiles in front of its own -- a few dozen
// integers at 50 000 genes --, ranks its kept elements by wave ballots and a 16-entry prefix, and writes.  No workgroup ever
// waits for another one: the only order between them is that of the two launches.  (One workgroup walking all tiles was
// 39 - 52 us of latency at 50 000 genes, twice per analysis, with the rest of the device idle.)
constexpr int kCompactTile = 1024;
struct CompactParams {
    int mode, n;
    int32_t *allZero;
    const int32_t *force_zero;
    const double *mean_in, *disp_in;
    double thresh;
    int32_t *tile_cnt;
    int32_t *rows_out;
    double *mean_out, *disp_out;
    int32_t *count_out;
};
DSQ_DEV bool compact_keep(const CompactParams &c, int i) {
    if (i >= c.n) return false;
    if (c.mode == 0) return !(c.allZero[i] | (c.force_zero ? c.force_zero[i] : 0));
    return c.disp_in[i] > c.thresh;
}
__global__ void __launch_bounds__(kCompactTile) compact_count_kernel(CompactParams c) {
    __shared__ int wcnt[kCompactTile / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long mask = __ballot(compact_keep(c, blockIdx.x * kCompactTile + t));
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int w = 0; w < kCompactTile / 64; w++) s += wcnt[w];
        c.tile_cnt[blockIdx.x] = s;
    }
}
__global__ void __launch_bounds__(kCompactTile) compact_write_kernel(CompactParams c) {
    __shared__ int wcnt[kCompactTile / 64];
    __shared__ int base_s;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * kCompactTile + t;
    const bool keep = compact_keep(c, i);
    if (c.mode == 0 && c.force_zero && i < c.n) c.allZero[i] = keep ? 0 : 1;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    if (wave == 0) {                                    // the kept elements of the tiles in front of this one
        int s = 0;
        for (int k = lane; k < (int)blockIdx.x; k += 64) s += c.tile_cnt[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) base_s = s;
    }
    __syncthreads();
    int mine = base_s, total = base_s;
    for (int w = 0; w < kCompactTile / 64; w++) { const int k = wcnt[w]; if (w < wave) mine += k; total += k; }
    mine += __popcll(mask & ((1ull << lane) - 1ull));
    if (keep) {
        if (c.mode == 0) c.rows_out[mine] = i;
        else { c.mean_out[mine] = c.mean_in[i]; c.disp_out[mine] = c.disp_in[i]; }
    }
    if (t == 0 && blockIdx.x == gridDim.x - 1) *c.count_out = total;
}
// tile_cnt: (n + kCompactTile - 1) / kCompactTile ints of device memory that nothing else uses until both launches are done
static hipError_t launch_compact(CompactParams c, hipStream_t st) {
    const int tiles = c.n > 0 ? (c.n + kCompactTile - 1) / kCompactTile : 1;
    hipLaunchKernelGGL(compact_count_kernel, dim3(tiles), dim3(kCompactTile), 0, st, c);
    hipLaunchKernelGGL(compact_write_kernel, dim3(tiles), dim3(kCompactTile), 0, st, c);
    return hipGetLastError();
}

// ---- the bucket key of a launch order (see "longest-expected-first order" below) --------------------------------------
// A launch order is a counting order of the rows over kLptBins buckets, bucket kLptBins - 1 first.  The key is one of:
//   LPT_MEAN_UP     a mean count, the rows with FEW counts first: sixths of an octave of 1 + mean
//   LPT_MEAN_DOWN   the same buckets taken from the other end
//   LPT_ITER        an iteration count (int32), clamped
//   LPT_ITER_F64    an iteration count kept as a double (the IRLS's)
//   LPT_ITER_MEAN   the product of an iteration count and log2(2 + mean), in steps of 4
//   LPT_DIST        the distance |a - b| of two doubles, in steps of 1 / 16
// NaN counts as long (an aborted fit).
constexpr int kLptBins = 128;
enum { LPT_NONE = 0, LPT_MEAN_UP = 1, LPT_MEAN_DOWN = 2, LPT_ITER = 3, LPT_ITER_F64 = 4, LPT_ITER_MEAN = 5, LPT_DIST = 6 };
struct LptKey {
    int kind;
    const int32_t *ki;
    const double *kd, *kd2;
};
DSQ_DEV int lpt_bin(const LptKey &k, int g) {
    double kd;
    if (k.kind == LPT_MEAN_UP || k.kind == LPT_MEAN_DOWN) {
        kd = 127.0 - 8.656170245333781 * dlog(1.0 + k.kd[g]);      // 6 / ln 2: a mean of 2^21 reaches bin 0
        if (kd < 0.0) kd = 0.0;
        if (k.kind == LPT_MEAN_DOWN) kd = 127.0 - kd;
    } else if (k.kind == LPT_ITER) {
        kd = (double)k.ki[g];
    } else if (k.kind == LPT_ITER_MEAN) {
        kd = 0.25 * (double)k.ki[g] * (1.4426950408889634 * dlog(2.0 + k.kd[g]));
    } else if (k.kind == LPT_DIST) {
        kd = 16.0 * __builtin_fabs(k.kd[g] - k.kd2[g]);
    } else {
        kd = k.kd[g];
    }
    if (!(kd >= 0.0)) kd = 127.0;             // (NaN: an aborted fit -- treat as long)
    return kd > 127.0 ? 127 : (int)kd;
}
// the histogram of a block's rows (bin < 0: this thread has none) in LDS, then one atomic add per occupied bin: called by
// every thread of the block
DSQ_DEV void lpt_block_hist(int bin, int *bins) {
    __shared__ int h[kLptBins];
    for (int k = threadIdx.x; k < kLptBins; k += blockDim.x) h[k] = 0;
    __syncthreads();
    if (bin >= 0) atomicAdd(&h[bin], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < kLptBins; k += blockDim.x)
        if (h[k]) atomicAdd(&bins[k], h[k]);
}

// ---- per-gene rules ----------------------------------------------------------------------------------------------
struct RuleParams {
    Rows rw;
    int n;                       // capacity / leading dimension of the n x p matrices
    int p;
    double minDisp, maxDisp, xim, outlierSD;
    const double *xim_dev;       // normalization-factor matrix: xim over the non-zero rows, computed by the chain
    int maxit, betaMaxit;
    const double *baseMean, *baseVar, *roughDisp;
    double *alpha_init, *la0;
    // fitDisp outputs
    const double *la_out, *initial_lp, *last_lp;
    const int32_t *iter;
    const double *la_grid;
    double *dge;
    int32_t *dispGeneIter;
    int32_t *grid_flag, *grid_rows, *grid_count;
    const double *scalars;
    double *dispFit, *log_dfit, *la_init, *dispMAP, *dispersion;
    const double *dispFit_in;      // DSQ_FIT_GIVEN: the caller's trend values, per gene
    int32_t *dispIter, *dispOutlier;
    // GLM fit
    const double *beta_nat, *beta_var, *beta_iter, *logLike;
    double *beta, *betaSE, *stat, *pvalue, *betaIter_out;
    int32_t *betaConv, *optim_flag, *optim_count;
    int32_t *optim_rows;           // the flagged rows, listed (any order) for the row-listed optim launch
    int wald;
    // the rows fitNbinomGLMsOptim re-fits (R/fitNbinomGLMs.R:340-407)
    const double *beta_init;       // the IRLS start values (natural-log scale)
    double *opt_start;             // n x p, log2 scale
    const int32_t *opt_conv;
    // the rule kernel in front of an ordered fit launch also builds the histogram of that launch's key (kind = LPT_NONE:
    // no order): alpha_init_kernel, map_init_kernel, map_final_kernel
    LptKey lpt;
    int *lpt_bins;                 // kLptBins zeroed counts
};

// alpha_hat <- pmin(roughDisp, momentsDisp), bounded to [minDisp, maxDisp] (R/core.R:713-728, :2439-2448)
__global__ void alpha_init_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < rows_count(q.rw);
    const int g = on ? rows_gene(q.rw, i) : 0;
    if (on) {
        const double bm = q.baseMean[g], bv = q.baseVar[g];
        const double xim = q.xim_dev ? *q.xim_dev : q.xim;
        const double mom = (bv - xim * bm) / (bm * bm);
        double a = np_min(q.roughDisp[g], mom);
        a = np_min(np_max(q.minDisp, a), q.maxDisp);
        q.alpha_init[g] = a;
        q.la0[g] = dlog(a);
    }
    if (q.lpt.kind != LPT_NONE) lpt_block_hist(on ? lpt_bin(q.lpt, g) : -1, q.lpt_bins);
}

// after the gene-wise fitDisp: accept / convergence / refit rules (R/core.R:785, 826-835)
__global__ void gene_est_post_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(q.rw)) return;
    const int g = rows_gene(q.rw, i);
    double d = np_min(dexp(q.la_out[g]), q.maxDisp);
    const double ilp = q.initial_lp[g];
    if (q.last_lp[g] < ilp + __builtin_fabs(ilp) / 1e6) d = q.alpha_init[g];      // noIncrease
    const int it = q.iter[g];
    q.dispGeneIter[g] = it;
    const bool conv = (it < q.maxit) && !(it == 1);
    const bool refit = !conv && (d > q.minDisp * 10.0);
    q.dge[g] = d;
    q.grid_flag[g] = refit ? 1 : 0;
    if (refit) q.grid_rows[atomicAdd(q.grid_count, 1)] = g;
}

// dispGeneEst[refitDisp] <- exp(grid); final clamp (R/core.R:846-848)
__global__ void gene_est_final_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(q.rw)) return;
    const int g = rows_gene(q.rw, i);
    double d = q.dge[g];
    if (q.grid_flag[g]) d = dexp(q.la_grid[g]);
    q.dge[g] = np_min(np_max(d, q.minDisp), q.maxDisp);
}

// dispFit from the trend; start value and prior mean of the MAP search (R/core.R:1019-1024)
__global__ void map_init_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < rows_count(q.rw);
    const int g = on ? rows_gene(q.rw, i) : 0;
    if (on) {
        const double fit = q.dispFit_in ? q.dispFit_in[g] : q.scalars[DSQ_SC_COEF0] + q.scalars[DSQ_SC_COEF1] / q.baseMean[g];
        const double d = q.dge[g];
        double init = (d > 0.1 * fit) ? d : fit;
        if (init != init) init = fit;
        q.dispFit[g] = fit;
        q.log_dfit[g] = dlog(fit);
        q.la_init[g] = dlog(init);
    }
    // (LPT_DIST reads log_dfit / la_init of the thread's own row back)
    if (q.lpt.kind != LPT_NONE) lpt_block_hist(on ? lpt_bin(q.lpt, g) : -1, q.lpt_bins);
}

// after the MAP fitDisp: dispMAP, convergence, stragglers to the grid (R/core.R:1042-1050)
__global__ void map_post_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(q.rw)) return;
    const int g = rows_gene(q.rw, i);
    const int it = q.iter[g];
    q.dispMAP[g] = dexp(q.la_out[g]);
    q.dispIter[g] = it;
    const bool refit = !(it < q.maxit);
    q.grid_flag[g] = refit ? 1 : 0;
    if (refit) q.grid_rows[atomicAdd(q.grid_count, 1)] = g;
}

// dispMAP[refit] <- exp(grid); clamp; dispOutlier; final dispersion (R/core.R:1061-1063, 1099-1115)
__global__ void map_final_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = i < rows_count(q.rw);
    const int g = on ? rows_gene(q.rw, i) : 0;
    if (on) {
        double dm = q.dispMAP[g];
        if (q.grid_flag[g]) dm = dexp(q.la_grid[g]);
        dm = np_min(np_max(dm, q.minDisp), q.maxDisp);
        q.dispMAP[g] = dm;
        const double d = q.dge[g];
        const double sd = __builtin_sqrt(q.scalars[DSQ_SC_VAR_LOG_DISP]);
        const bool outlier = dlog(d) > q.log_dfit[g] + q.outlierSD * sd;       // NaN compares false, as the mirror's mask
        q.dispOutlier[g] = outlier ? 1 : 0;
        q.dispersion[g] = outlier ? d : dm;
    }
    if (q.lpt.kind != LPT_NONE) lpt_block_hist(on ? lpt_bin(q.lpt, g) : -1, q.lpt_bins);
}

// the host half of fitNbinomGLMs (R/fitNbinomGLMs.R:185-211) + Wald statistic and p-value (R/core.R:1471,1507)
__global__ void beta_post_kernel(RuleParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(q.rw)) return;
    const int g = rows_gene(q.rw, i);
    const double log2e = 1.4426950408889634;
    bool stable = true, varpos = true;
    for (int c = 0; c < q.p; c++) {
        const double b = q.beta_nat[(size_t)g + (size_t)q.n * c], v = q.beta_var[(size_t)g + (size_t)q.n * c];
        if (b != b) stable = false;
        if (v <= 0.0) varpos = false;
        if (q.beta) {
            const double bl = log2e * b;
            const double se = log2e * __builtin_sqrt(np_max(v, 0.0));
            q.beta[(size_t)g + (size_t)q.n * c] = bl;
            q.betaSE[(size_t)g + (size_t)q.n * c] = se;
            if (q.wald) {
                const double z = bl / se;
                q.stat[(size_t)g + (size_t)q.n * c] = z;
                q.pvalue[(size_t)g + (size_t)q.n * c] = dpnorm_upper2(z);
            }
        }
    }
    const double it = q.beta_iter[g];
    const bool conv = it < (double)q.betaMaxit;
    if (q.betaConv) q.betaConv[g] = conv ? 1 : 0;
    if (q.betaIter_out) q.betaIter_out[g] = it;
    const bool optim = !conv || !stable || !varpos;
    q.optim_flag[g] = optim ? 1 : 0;
    if (optim) {
        const int k = atomicAdd(q.optim_count, 1);
        if (q.optim_rows) q.optim_rows[k] = g;
        // start values of the fallback (:350-355): the IRLS estimate (log2 scale) when it is finite and inside the box,
        // else the IRLS's own start values -- on the natural-log scale, as the reference passes them
        bool usable = stable;
        for (int c = 0; c < q.p && usable; c++)
            usable = __builtin_fabs(log2e * q.beta_nat[(size_t)g + (size_t)q.n * c]) < 30.0;
        for (int c = 0; c < q.p; c++)
            q.opt_start[(size_t)g + (size_t)q.n * c] = usable ? log2e * q.beta_nat[(size_t)g + (size_t)q.n * c]
                                                              : q.beta_init[(size_t)g + (size_t)q.n * c];
    }
}

// after the fallback: betaConv[row] <- TRUE where optim converged (:378-380); Wald statistic and p-value from its
// coefficients (the optim kernel has written beta / betaSE / logLike / mu of these rows in place)
__global__ void optim_post_kernel(RuleParams q) {
    const int cnt = rows_count(q.rw);                       // (a handful: the grid is small and strides)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const int g = rows_gene(q.rw, i);
        if (q.betaConv && q.opt_conv[g]) q.betaConv[g] = 1;
        if (q.wald && q.stat) {
            for (int c = 0; c < q.p; c++) {
                const double z = q.beta[(size_t)g + (size_t)q.n * c] / q.betaSE[(size_t)g + (size_t)q.n * c];
                q.stat[(size_t)g + (size_t)q.n * c] = z;
                q.pvalue[(size_t)g + (size_t)q.n * c] = dpnorm_upper2(z);
            }
        }
    }
}

// rows flagged -> list (order irrelevant: the listed launches write results at the gene's own position)
__global__ void list_kernel(Rows rw, const int32_t *flag, int want, int32_t *rows_out, int32_t *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(rw)) return;
    const int g = rows_gene(rw, i);
    if ((flag[g] != 0) == (want != 0)) rows_out[atomicAdd(count, 1)] = g;
}

// the rows that can hold a count outlier (the fit's bound, BetaKernelParams.cand_flag) and the rows the optim fallback has
// rewritten (their stored means are no longer the ones the bound saw) -> list, and the flags once more in a vector that
// nothing writes until the phase is over (the grid flags go back to the refit's searches)
__global__ void cand_list_kernel(Rows rw, const int32_t *bound_flag, const int32_t *optim_flag, int32_t *flag_out, int32_t *rows_out,
                                 int32_t *count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(rw)) return;
    const int g = rows_gene(rw, i);
    const int f = (bound_flag[g] != 0 || optim_flag[g] != 0) ? 1 : 0;
    flag_out[g] = f;
    if (f) rows_out[atomicAdd(count, 1)] = g;
}

// refitWithoutOutliers: result columns of rows that became all-zero are NA (R/core.R:2535), only when some row
// is actually refitted (:2496)
struct NaRowsParams {
    Rows rw;
    int n, p;
    const int32_t *allZero, *n_refit;
    double *beta, *betaSE, *stat, *pvalue, *betaIter, *logLike, *logLikeReduced, *maxCooks;
    int32_t *betaConv;
};
__global__ void na_rows_kernel(NaRowsParams q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(q.rw) || *q.n_refit <= 0) return;
    const int g = rows_gene(q.rw, i);
    if (!q.allZero[g]) return;
    const double nan = dnan();
    for (int c = 0; c < q.p; c++) {
        q.beta[(size_t)g + (size_t)q.n * c] = nan;
        q.betaSE[(size_t)g + (size_t)q.n * c] = nan;
        if (q.stat) { q.stat[(size_t)g + (size_t)q.n * c] = nan; q.pvalue[(size_t)g + (size_t)q.n * c] = nan; }
    }
    q.betaIter[g] = nan; q.logLike[g] = nan; q.maxCooks[g] = nan;
    if (q.logLikeReduced) q.logLikeReduced[g] = nan;
    q.betaConv[g] = -1;
}

// the n x m assays of the rows that were never fitted (all-zero counts, or weights that leave a degenerate design): NA, as
// buildMatrixWithNARows leaves them in R -- the kernels skip those rows, so without this they keep whatever the buffer
// held (found by the 8-range host-entry test of round 5: two calls returned different garbage there)
__global__ void __launch_bounds__(256) na_assay_rows_kernel(int n, int m, long ld, const int32_t *allZero, double *a0, double *a1,
                                                            int32_t *zero_p = nullptr, int zero_n = 0) {
    // (zero_p: the row-list counters of the outlier phase that follows in the same call -- a memset of 8 int32 at an odd
    //  offset is three fill commands of the runtime)
    if (blockIdx.x == 0 && (int)threadIdx.x < zero_n) zero_p[threadIdx.x] = 0;
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;            // one gene per lane for the flag ...
    unsigned long long todo = __ballot(g < n && allZero[g] != 0);
    const int base = g - lane;
    const double nan = dnan();
    while (todo) {                                                  // ... the (few) flagged rows of the wave written by all lanes
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1;
        const size_t row = (size_t)(base + l) * ld;
        for (int j = lane; j < m; j += 64) {
            if (a0) a0[row + j] = nan;
            if (a1) a1[row + j] = nan;
        }
    }
}

// maxCooks after the refit (R/core.R:2538-2546): NA everywhere when every sample is replaceable, else the row
// maximum of the ORIGINAL Cook's distances over the samples in cells of >= 3, replaceable samples zeroed
__global__ void __launch_bounds__(256) masked_max_kernel(Rows rw, int m, long ld, const double *cooks, const int32_t *use,
                                                         const int32_t *zero, int all_replaceable, int valid,
                                                         const int32_t *n_refit, double *maxCooks) {
    if (*n_refit <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int nw = rows_count(rw);
    for (int wi = blockIdx.x * waves + wave; wi < nw; wi += gridDim.x * waves) {
        const int g = rows_gene(rw, wi);
        if (all_replaceable || !valid) {
            if (lane == 0) maxCooks[g] = dnan();
            continue;
        }
        const double *ck = cooks + (size_t)g * ld;
        double mx = -__builtin_inf();
        int isnan_ = 0;
        for (int j = lane; j < m; j += 64) {
            if (!use[j]) continue;
            double v = zero[j] ? 0.0 : ck[j];
            if (v != v) isnan_ = 1;
            if (v > mx) mx = v;
        }
        double o, a, b;
        o = lane_xor1(mx); mx = (o > mx) ? o : mx;
        o = lane_xor2(mx); mx = (o > mx) ? o : mx;
        o = lane_xor4(mx); mx = (o > mx) ? o : mx;
        o = lane_xor8(mx); mx = (o > mx) ? o : mx;
        lane_pair16(mx, a, b); mx = (b > a) ? b : a;
        lane_pair32(mx, a, b); mx = (b > a) ? b : a;
        if (lane == 0) maxCooks[g] = __any(isnan_) ? dnan() : mx;
    }
}

// ---- longest-expected-first order of a full-size fit launch ---------------------------------------------------------
// The persistent fit kernels hand out genes in list order through a counter.  Once the counter runs dry the device empties
// out while the last genes finish, and nothing else can start: the next launch depends on this one through a rule kernel or
// the trend.  So every full-size fit launch pays a drain of about one slow gene, four times per step, and what the order
// decides is which genes are the last: with the slow ones drawn first, the quick ones fill the gaps (longest-processing-
// time-first).  At one rank's share of an 8-GPU run (6 250 genes on 3 072 wave slots, two genes per slot) two slow genes that
// meet in one slot set the time of the launch (fit_beta 0.30 ms in list order, 0.21 ms ordered); at 50 000 genes the drain is
// a few per cent of a launch (figures per launch and per key: profiles/launch_order.md).
// Every gene's results are written at its own position and no kernel couples two genes, so the order changes no bit
// (tests/test_gpu_launch_order.py).
// What an order can and cannot do at 6 250 genes on 3 072 slots (a simulation on the iteration counts of that workload,
// cost = iterations): fit_beta in list order ends at 2.5x the ideal, longest-first at 1.8x = the slowest single gene (19
// iterations) -- the floor of any order; the dispersion searches end at 1.4x either way: 6 250 = 2.03 x 3 072, the last
// hundred genes are a third round whatever the order.
// The keys (lpt_bin): the second fit of a gene costs about what its first one did (the test's IRLS after the gene-wise IRLS:
// same counts, nearly the same dispersion), so the test's fit goes by DESCENDING iteration count of the first; the gene-wise
// IRLS has no earlier fit to go by, its iteration count falls with log(baseMean) (correlation -0.84 at C3): ascending mean;
// an evaluation of the dispersion search costs more the more distinct counts a row has: descending mean.
// The order is a counting order in two passes over the rows, both of as many blocks as the rule kernels have.  The
// histogram is built by the rule kernel that runs over the same rows just in front (lpt_block_hist: per-block LDS bins,
// one atomic add per occupied bin and block), so an order adds ONE small launch: lpt_scatter_kernel, in which every block
// rescans the bins for the buckets' start positions, reserves its share of each bucket with one atomic add and writes its
// rows there.  The order inside a bucket is whatever the atomics give.  `rev` (optional): the same list read backwards,
// for a launch that wants the other end of the same key first.
__global__ void __launch_bounds__(256) lpt_scatter_kernel(Rows rw, LptKey key, const int *bins, int *cursor, int32_t *out, int32_t *rev) {
    __shared__ int h[kLptBins], tot[kLptBins], base[kLptBins];
    const int cnt = rows_count(rw);
    if ((int)(blockIdx.x * blockDim.x) >= cnt) return;              // (the whole block)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = threadIdx.x; k < kLptBins; k += blockDim.x) { h[k] = 0; tot[k] = bins[k]; }
    __syncthreads();
    const bool on = i < cnt;
    const int g = on ? rows_gene(rw, i) : 0;
    const int b = on ? lpt_bin(key, g) : 0;
    const int mine = on ? atomicAdd(&h[b], 1) : 0;
    __syncthreads();
    for (int k = threadIdx.x; k < kLptBins; k += blockDim.x) {
        int start = 0;
        for (int j = kLptBins - 1; j > k; j--) start += tot[j];     // bucket kLptBins - 1 comes first
        base[k] = start + (h[k] ? atomicAdd(&cursor[k], h[k]) : 0);
    }
    __syncthreads();
    if (!on) return;
    const int pos = base[b] + mine;
    if (pos >= cnt) return;            // (cannot happen while the bins are the histogram of this key over these rows)
    out[pos] = g;
    if (rev) rev[cnt - 1 - pos] = g;
}

// ---- the fills in front of a call's first kernel, as ONE launch ----------------------------------------------------
// A chain used to open with a dozen memset / copy commands (the NA patterns of the result columns, the status block, the
// dynamic-scheduling counters, the ridge / contrast block): ~ 5 us of dependent dispatch each -- 0.11 ms of a 2.7 ms step
// at one rank's share of C3.  The segments (4-byte aligned, word patterns) and the small block (by value) ride in the
// kernel's arguments: no host buffer is read after the launch returns.
// The result columns the gene-wise phase pre-fills, by pattern (rows that turn out all-zero keep it: 0xFF bytes are a NaN /
// -1).  kInitSegMax counts the regions ONE call can ask for when no two of them are neighbours, so a column added to a
// list below grows InitParams::seg with it.
typedef double *DsqDeseqOut::*OutF64;
typedef int32_t *DsqDeseqOut::*OutI32;
static constexpr OutF64 kNaVectors[] = {&DsqDeseqOut::dispGeneEst, &DsqDeseqOut::dispFit, &DsqDeseqOut::dispMAP, &DsqDeseqOut::dispersion,
                                        &DsqDeseqOut::betaIter, &DsqDeseqOut::logLike, &DsqDeseqOut::maxCooks, &DsqDeseqOut::logLikeReduced};
static constexpr OutF64 kNaMatrices[] = {&DsqDeseqOut::beta, &DsqDeseqOut::betaSE, &DsqDeseqOut::stat, &DsqDeseqOut::pvalue};
static constexpr OutI32 kNaInts[] = {&DsqDeseqOut::dispGeneIter, &DsqDeseqOut::dispIter, &DsqDeseqOut::dispOutlier, &DsqDeseqOut::betaConv};
static constexpr OutI32 kZeroInts[] = {&DsqDeseqOut::replace, &DsqDeseqOut::optim_geneest, &DsqDeseqOut::optim_test};
template <class T, size_t N> constexpr int count_of(T (&)[N]) { return (int)N; }
static constexpr int kInitSegMax = 1 /* work counters */ + 1 /* launch-order bins */ + 1 /* status */ + count_of(kNaVectors) + count_of(kNaMatrices) + 1 /* mle_beta */ +
                                   count_of(kNaInts) + count_of(kZeroInts) + 1 /* grid flags */ + 3 /* FIT_USED, trend fit, selection */;
struct InitSeg { uint32_t *p; uint32_t words; uint32_t val; };
struct InitParams {
    int nseg;
    InitSeg seg[kInitSegMax];
    double *blk_dst;
    int nblk;
    double blk[3 * DSQ_P_WIDE + 8];
};
static_assert(sizeof(InitParams) <= 4096, "InitParams rides in the kernel arguments");
__global__ void __launch_bounds__(256) chain_init_kernel(InitParams q) {
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    for (int s = 0; s < q.nseg; s++) {
        uint32_t *p = q.seg[s].p;
        const uint32_t v = q.seg[s].val, w = q.seg[s].words;
        for (uint32_t i = tid; i < w; i += nth) p[i] = v;
    }
    if (tid < (unsigned)q.nblk) q.blk_dst[tid] = q.blk[tid];
}

// ---- orchestration -----------------------------------------------------------------------------------------------
static inline int kern_width(int p) { return p > DSQ_P_REG ? dsq_wide_width(p) : p; }

struct Pipe {
    const DsqDeseqArgs *a;
    const DsqDeseqOut *o;
    hipStream_t st;
    int n, m, p;
    long ld;
    double maxDisp, min_log_alpha;
    // workspace (device)
    double *roughDisp, *beta_init, *alpha_init, *la0, *la_out, *last_change, *initial_lp, *initial_dlp, *last_lp, *last_dlp;
    double *la_grid, *log_dfit, *la_init, *beta_nat, *beta_var, *beta_iter, *cnum, *cden, *dev, *lam, *contrast, *resbuf;
    double *trend_mean_c, *trend_disp_c, *robustDisp, *scratch, *cscratch;
    double *kconst;              // n: K' of each row from its last fitBeta launch (-> LogLikeKernelParams.kconst)
    double *opt_start, *opt_beta, *opt_se, *opt_ll;
    int32_t *iter, *iter_accept, *grid_flag, *rows_nz, *rows_grid, *rows_rep, *rows_refit, *counters, *work_counters;
    int32_t *rows_opt, *opt_conv;
    int32_t *rows_lpt;             // the non-zero rows in the order of the next fit launch (lpt_scatter_kernel)
    // launch orders of this call: kLptBuilds x (kLptBins counts | kLptBins cursors), zeroed by the init launch, behind the
    // fit kernels' scratch; the reversed list of the gene-wise order while it is alive (it borrows rows_grid); the order of
    // the test's fit, whose histogram map_final_kernel has built
    int *lpt_bins;
    int lpt_next;
    const int32_t *rows_rev;
    LptKey lpt_test;
    int *lpt_test_bins;
    double *lam_prior;             // betaPrior: 1 / betaPriorVar on the natural-log scale (device copy of a->lambda_prior)
    // WIDE designs (10 < p <= 48): the fit kernels run at the padded width pk = 16 / 24 / 32 / 48 on the design zero-padded to pk
    // columns (ridge 1, start value 0, contrast 0 on the padding: the real coefficients keep their bits, csrc/capi.hip
    // "wide designs"); the n x . work matrices have pk columns, the rule kernels and the results keep the true p
    int pk;
    const double *x_k;             // the design at the kernels' width (the caller's, or the padded copy)
    unsigned long long padmask;
    double *xim_cur;               // ... the one the rule kernels read now: over the non-zero rows, or (refit) over the refitted rows
    double *xim_dev;               // normalization-factor matrix: mean(1 / colMeans(nf)) over the non-zero rows (one double
                                   // behind the lambda block of the caller's workspace: it persists between the phases)
    // nbinomLRT against a reduced model that is not ~1 / the beta-prior refit (never both: the prior is Wald only)
    double *red_binit, *red_beta, *red_se, *red_mu;
    // ... a reduced model of more than DSQ_P_REG columns runs at ITS padded width (round 5): the reduced design zero-padded to
    // red_pk columns, ridge 1 on the padding (kept in the lambda block's third part, which only the beta prior uses otherwise)
    int red_pk;
    const double *red_x_k;
    double *red_lam;
    // ... and so does the (expanded) design of the beta-prior pass: pri_pk columns, the padded copy pri_x_k
    int pri_pk;
    const double *pri_x_k;
    const int32_t *red_cell_perm, *red_cell_start;
    int red_ncell;
    int32_t *cells_dev;            // perm | in3 | cell_start | use3 | replaceable
    void *trend_ws, *sel_ws;       // the trend fit's barrier / partial-sum block and the selection workspace of the sixteen-
                                   // workgroup prior variance, both zeroed by the init launch (nullptr: not used by this call)
    int pkp, pmax;                 // the padded width of the beta-prior pass (0: none); the columns of the n x . work matrices
    int next_counter;
    const int32_t *cell_perm, *cell_start;   // design cells for the cell-collapsed fitBeta kernel (ncell = 0: general)
    int ncell;
    const char *tag;               // appended to the profile names of the refit chain's launches
    // settings of the test's GLM fits and the floor of the gene-wise estimate's fitted means.  The main chain takes the
    // caller's (DESeq() hands betaTol / maxit / useQR / minmu to nbinomWaldTest / nbinomLRT and minmu to
    // estimateDispersions -> estimateDispersionsGeneEst, R/core.R:393-405, R/methods.R:552, where it is the floor of
    // :763 -- the IRLS inside that fitNbinomGLMs call keeps its own default minmu = 0.5, :755-757); the refit of the
    // replaced rows runs every step on its DEFAULTS (refitWithoutOutliers passes none of them on, R/core.R:2509-2531)
    double t_tol, t_minmu, ge_floor;
    int t_maxit, t_useQR;
    // the full-row nbinomLogLike of the test's fit on a SIDE stream (overlap below): set while it is in flight
    hipStream_t side;
    hipEvent_t ev_fork, ev_join;
    bool overlap, forked, ll_pending;
    LogLikeKernelParams ll;        // the deferred full-row launch (test_fit -> run_chain)
    // the outlier phase in candidates-first order (phase_outlier_first): asked for by this call; the test's fit has left the
    // candidate flags in grid_flag; the side stream has recorded ev_fork behind the full-row nbinomLogLike
    bool outlier_first, cand_ready, ll_event;
    // host-side facts of the design cells
    int any3, maxcell, all_replaceable;
};

// the row-list counters of the chain ARE the caller's status block (no copies at the end of a call): a counter sits at
// the index of the DSQ_ST_* entry that reports it; the two spare entries count the optim rows of the reduced / MLE fits
enum { CNT_NZ = DSQ_ST_N_NONZERO, CNT_GRID1 = DSQ_ST_N_GRID_GENEEST, CNT_TREND = DSQ_ST_N_TREND, CNT_GRID2 = DSQ_ST_N_GRID_MAP,
       CNT_OPT1 = DSQ_ST_N_OPTIM_GENEEST, CNT_OPT2 = DSQ_ST_N_OPTIM_TEST, CNT_REP = DSQ_ST_N_REPLACE, CNT_REFIT = DSQ_ST_N_REFIT,
       CNT_GRID1R = DSQ_ST_N_GRID_GENEEST_REFIT, CNT_GRID2R = DSQ_ST_N_GRID_MAP_REFIT, CNT_OPT1R = DSQ_ST_N_OPTIM_GENEEST_REFIT,
       CNT_OPT2R = DSQ_ST_N_OPTIM_TEST_REFIT, CNT_OPT3 = 14, CNT_OPT3R = 15, CNT_N = DSQ_ST_COUNT };
static_assert(DSQ_ST_N_OPTIM_TEST_REFIT < 14 && DSQ_ST_COUNT == 16, "status block layout");

static int *next_work_counter(Pipe &P) {
    int *c = P.work_counters + (P.next_counter % 60);
    P.next_counter++;
    return c;
}

static inline dim3 ew_grid(int n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }

// a row list that is expected to be short (stragglers, refits): neither the non-zero rows nor one of their launch orders
static inline int rows_few(const Pipe &P, const Rows &rw) {
    return (rw.rows && rw.rows != P.rows_nz && rw.rows != P.rows_lpt && rw.rows != P.rows_rev) ? 1 : 0;
}

// the fields the parameter blocks of the fit kernels share (everything else zero): shape, counts, normalization factors,
// the weights of this launch when the analysis has any, the rows
template <class KP>
static KP fit_head(const Pipe &P, const Rows &rw, const int32_t *y, const double *weights) {
    KP kp;
    memset(&kp, 0, sizeof kp);
    kp.n = P.n; kp.m = P.m; kp.ld = P.ld;
    kp.y = y; kp.nf = P.a->nf; kp.nf_is_vector = P.a->nf_is_vector;
    kp.weights = P.a->useWeights ? weights : nullptr; kp.useWeights = kp.weights ? 1 : 0;
    kp.rows = rw.rows; kp.n_dev = rw.n_dev;
    return kp;
}

static RuleParams rule_params(const Pipe &P, const Rows &rw) {
    RuleParams q;
    memset(&q, 0, sizeof q);
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    q.rw = rw; q.n = P.n; q.p = P.p;
    q.minDisp = a->minDisp; q.maxDisp = P.maxDisp; q.xim = a->xim; q.outlierSD = a->outlierSD;
    q.xim_dev = a->nf_is_vector ? nullptr : P.xim_cur;
    q.maxit = a->maxit; q.betaMaxit = P.t_maxit;
    q.baseMean = o->baseMean; q.baseVar = o->baseVar; q.roughDisp = P.roughDisp;
    q.alpha_init = P.alpha_init; q.la0 = P.la0;
    q.la_out = P.la_out; q.initial_lp = P.initial_lp; q.last_lp = P.last_lp; q.iter = P.iter; q.la_grid = P.la_grid;
    q.dge = o->dispGeneEst; q.dispGeneIter = o->dispGeneIter;
    q.grid_flag = P.grid_flag; q.grid_rows = P.rows_grid;
    q.scalars = o->scalars;
    q.dispFit_in = a->dispFit_in;
    q.dispFit = o->dispFit; q.log_dfit = P.log_dfit; q.la_init = P.la_init; q.dispMAP = o->dispMAP;
    q.dispersion = o->dispersion; q.dispIter = o->dispIter; q.dispOutlier = o->dispOutlier;
    q.beta_nat = P.beta_nat; q.beta_var = P.beta_var; q.beta_iter = P.beta_iter;
    q.optim_rows = P.rows_opt; q.beta_init = P.beta_init; q.opt_start = P.opt_start; q.opt_conv = P.opt_conv;
    return q;
}

// which model matrix a GLM fit of the chain runs on: the design itself, nbinomLRT's reduced model, or the (expanded)
// design of the beta-prior refit with its ridge 1 / betaPriorVar (R/fitNbinomGLMs.R:311-325)
enum { DES_FULL = 0, DES_REDUCED = 1, DES_PRIOR = 2 };
struct DesignSel {
    const double *x, *beta_init, *lam;
    int p;                         // the width the kernels run at (the padded one for a wide design)
    const int32_t *cperm, *cstart;
    int ncell;
    int p_true;                    // the design's own number of columns
};
static DesignSel design_of(const Pipe &P, int which) {
    const DsqDeseqArgs *a = P.a;
    DesignSel d;
    if (which == DES_REDUCED) d = {P.red_x_k, P.red_binit, P.red_lam, P.red_pk, P.red_cell_perm, P.red_cell_start, P.red_ncell, a->p_red};
    else if (which == DES_PRIOR) d = {P.pri_x_k, a->prior_expanded ? P.red_binit : P.beta_init, P.lam_prior, P.pri_pk,
                                      P.cell_perm, P.cell_start, P.ncell, a->p_prior};
    else d = {P.x_k, P.beta_init, P.lam, P.pk, P.cell_perm, P.cell_start, P.ncell, P.p};
    return d;
}

static int launch_fit_beta(Pipe &P, const Rows &rw, const int32_t *y, const double *alpha, const double *weights,
                           double *mu_out, double mu_floor, double *hat, double tol, int maxit, int useQR, double minmu,
                           const char *name, int which = DES_FULL, bool cand = false) {
    const DesignSel ds = design_of(P, which);
    BetaKernelParams kp = fit_head<BetaKernelParams>(P, rw, y, weights);
    if (cand) { kp.cand_flag = P.grid_flag; kp.cand_cutoff = P.a->cooksCutoff; kp.cand_p = (double)P.p; }
    kp.p = ds.p; kp.x = ds.x; kp.alpha_hat = alpha; kp.contrast = P.contrast;
    kp.beta_init = ds.beta_init; kp.lambda = ds.lam;
    kp.tol = tol; kp.minmu = minmu; kp.mu_floor = mu_floor; kp.maxit = maxit; kp.useQR = useQR ? 1 : 0;
    kp.beta_mat = P.beta_nat; kp.beta_var_mat = P.beta_var; kp.iter = P.beta_iter;
    kp.contrast_num = P.cnum; kp.contrast_denom = P.cden; kp.deviance = P.dev;
    kp.hat_diagonals = hat; kp.mu_out = mu_out;
    kp.kconst_out = P.kconst;            // K' of the rows this launch fits: the nbinomLogLike launch behind it reads it
    kp.scratch = P.scratch; kp.cscratch = P.cscratch;
    kp.work_counter = next_work_counter(P);
    kp.rows_few = rows_few(P, rw);
    kp.cell_perm = ds.cperm; kp.cell_start = ds.cstart; kp.ncell = ds.ncell;
    kp.p_true = ds.p_true;
    bool ok = false;
    char nm[32];
    snprintf(nm, sizeof nm, "%s%s", name, P.tag);
    capi_prof_begin(nm, P.n, P.st);
    DSQ_HIP(dispatch_fit_beta(kp.p, kp, P.st, &ok));
    capi_prof_end(P.st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: no register kernel for p=%d", P.p);
    return DSQ_OK;
}

static int launch_fit_disp(Pipe &P, const Rows &rw, const int32_t *y, const double *mu, const double *la_in,
                           const double *prior_mean, bool usePrior, const double *weights, bool useCR, bool grid,
                           const char *name) {
    const DsqDeseqArgs *a = P.a;
    DispKernelParams kp;
    memset(&kp, 0, sizeof kp);
    kp.n = P.n; kp.m = P.m; kp.p = P.pk; kp.ld = P.ld;
    kp.y = y; kp.mu_hat = mu; kp.weights = a->useWeights ? weights : nullptr; kp.useWeights = a->useWeights ? 1 : 0;
    kp.x = P.x_k; kp.padmask = P.padmask;
    kp.log_alpha_in = la_in; kp.prior_mean = prior_mean;
    kp.prior_sigmasq = 1.0;
    kp.prior_sigmasq_dev = usePrior ? P.o->scalars + DSQ_SC_DISP_PRIOR_VAR : nullptr;
    kp.min_log_alpha = P.min_log_alpha; kp.kappa_0 = a->kappa_0; kp.tol = a->dispTol;
    kp.weightThreshold = a->weightThreshold; kp.maxit = a->maxit;
    kp.usePrior = usePrior ? 1 : 0; kp.useCR = useCR ? 1 : 0;
    kp.work_counter = next_work_counter(P);
    kp.rows = rw.rows; kp.n_dev = rw.n_dev; kp.rows_few = rows_few(P, rw);
    if (P.p >= tuning().disp_cell_minp) { kp.cell_perm = P.cell_perm; kp.cell_start = P.cell_start; kp.ncell = P.ncell; }
    if (grid) {
        kp.grid = a->disp_grid; kp.ngrid = a->ngrid; kp.log_alpha = P.la_grid;
    } else {
        kp.log_alpha = P.la_out; kp.iter = P.iter; kp.iter_accept = P.iter_accept; kp.last_change = P.last_change;
        kp.initial_lp = P.initial_lp; kp.initial_dlp = P.initial_dlp; kp.last_lp = P.last_lp; kp.last_dlp = P.last_dlp;
        kp.last_d2lp = nullptr;          // never read by estimateDispersions* (R/core.R:784-787, 1042)
    }
    bool ok = false;
    char nm[32];
    snprintf(nm, sizeof nm, "%s%s", name, P.tag);
    capi_prof_begin(nm, P.n, P.st);
    DSQ_HIP(dispatch_fit_disp(P.pk, kp, P.st, grid, &ok));
    capi_prof_end(P.st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: no register kernel for p=%d", P.p);
    return DSQ_OK;
}

// the pre-fit kernels on the design itself: Q and X R^-1 of its QR factors, no outputs yet
static PrefitKernelParams prefit_params(const Pipe &P, const Rows &rw, const int32_t *y, const double *weights = nullptr) {
    PrefitKernelParams kp = fit_head<PrefitKernelParams>(P, rw, y, weights);
    kp.p = P.p; kp.q = P.a->q; kp.a = P.a->a;
    return kp;
}
// ... and, unweighted, on ANOTHER model matrix (nbinomLRT's reduced one, the intercept of the expanded prior design): the
// start values go to beta_init, the moments to work vectors that nobody reads (but baseMean = P.cnum, prior_fit)
static PrefitKernelParams prefit_other(const Pipe &P, const Rows &rw, const int32_t *y, int p, const double *q, const double *xr,
                                       const double *r, double *beta_init) {
    PrefitKernelParams kp = fit_head<PrefitKernelParams>(P, rw, y, nullptr);
    kp.p = p; kp.q = q; kp.a = xr; kp.r = r;
    kp.baseMean = P.cnum; kp.baseVar = P.cden; kp.roughDisp = P.dev; kp.allZero = P.opt_conv; kp.beta_init = beta_init;
    return kp;
}
// nbinomLogLike of the rows at the fitted means `mu` and the final dispersions, K' from the fitBeta launch in front of it
static LogLikeKernelParams loglike_params(const Pipe &P, const Rows &rw, const int32_t *y, const double *mu, double *out) {
    LogLikeKernelParams lk;
    memset(&lk, 0, sizeof lk);
    lk.n = P.n; lk.m = P.m; lk.ld = P.ld; lk.y = y; lk.mu = mu; lk.disp = P.o->dispersion;
    lk.weights = P.a->useWeights ? P.a->weights_norm : nullptr; lk.useWeights = P.a->useWeights ? 1 : 0;
    lk.loglike = out; lk.rows = rw.rows; lk.n_dev = rw.n_dev; lk.kconst = P.kconst;
    return lk;
}

static int launch_prefit_rows(Pipe &P, const Rows &rw, const int32_t *y) {
    PrefitKernelParams kp = prefit_params(P, rw, y, P.a->weights_raw);
    kp.r = P.a->r;
    kp.baseMean = P.o->baseMean; kp.baseVar = P.o->baseVar; kp.roughDisp = P.roughDisp; kp.beta_init = P.beta_init;
    kp.allZero = P.o->allZero;
    bool ok = false;
    capi_prof_begin(rw.rows ? "prefit_moments:refit" : "prefit_moments", P.n, P.st);
    DSQ_HIP(launch_prefit(kp, P.st, &ok));
    capi_prof_end(P.st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: p=%d", P.p);
    return DSQ_OK;
}

// the first p columns of two n x . work matrices -> the caller's n x p matrices, for the listed rows
__global__ void copy_rows_cols_kernel(Rows rw, int n, int p, const double *src_a, const double *src_b, double *dst_a, double *dst_b) {
    const int cnt = rows_count(rw);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += gridDim.x * blockDim.x) {
        const int g = rows_gene(rw, i);
        for (int c = 0; c < p; c++) {
            dst_a[(size_t)g + (size_t)n * c] = src_a[(size_t)g + (size_t)n * c];
            dst_b[(size_t)g + (size_t)n * c] = src_b[(size_t)g + (size_t)n * c];
        }
    }
}

// fitNbinomGLMsOptim (R/fitNbinomGLMs.R:340-407) on the rows beta_post_kernel listed (their number lives on the device:
// usually zero, the launch then finds nothing to do): start values from P.opt_start, coefficients / standard errors /
// logLike / fitted means written at the rows' own positions
static int launch_optim(Pipe &P, int cnt_optim, const int32_t *y, const double *alpha, const double *weights, double minmu,
                        double mu_floor, double *beta, double *betaSE, double *loglike, double *mu_out, int which = DES_FULL) {
    const DesignSel ds = design_of(P, which);
    const Rows orw = {P.rows_opt, P.counters + cnt_optim, P.n};
    OptimKernelParams kp = fit_head<OptimKernelParams>(P, orw, y, weights);
    kp.p = ds.p; kp.x = ds.x; kp.alpha_hat = alpha; kp.lamnat = ds.lam; kp.beta_start = P.opt_start;
    kp.minmu = minmu; kp.mu_floor = mu_floor;
    // (a padded design: the kernel writes ds.p columns -- into the work matrices; the listed rows' true columns are copied
    //  to the caller's n x p matrices behind the launch)
    const bool via_work = ds.p != ds.p_true && which != DES_REDUCED && beta != P.opt_beta;     // (the reduced fit's coefficients are work matrices already)
    kp.beta = via_work ? P.opt_beta : beta; kp.betaSE = via_work ? P.opt_se : betaSE;
    kp.conv = P.opt_conv; kp.mu_out = mu_out; kp.loglike = loglike;
    bool ok = false;
    char nm[32];
    snprintf(nm, sizeof nm, "optim_rows%s", P.tag);
    capi_prof_begin(nm, P.n, P.st);
    DSQ_HIP(dispatch_optim_rows(kp.p, kp, P.st, &ok));
    capi_prof_end(P.st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: no optim kernel for p=%d", P.p);
    if (via_work) {
        hipLaunchKernelGGL(copy_rows_cols_kernel, dim3(16), dim3(256), 0, P.st, orw, P.n, ds.p_true, (const double *)P.opt_beta,
                           (const double *)P.opt_se, beta, betaSE);
        DSQ_HIP(hipGetLastError());
    }
    return DSQ_OK;
}

// ---- launch orders, host half (see lpt_scatter_kernel) -----------------------------------------------------------
// DSQ_LPT=0 switches every order off.  Only the full-size launches of the main chain are ordered (the non-zero rows), and
// only from 256 samples: the drain an order can recover is about one slow gene's time, which grows with the row length, and
// an order costs 0.01 ms -- at C2 (20 000 genes, m = 100) the test's fit gains 0.004 ms by its best key and no other launch
// gains anything (DSQ_LPT=2: whatever the row length; the tests order their small inputs that way).  The key of each launch
// is a Tuning field (DSQ_LPT_KEY1 / _KEYD / _KEYM / _KEY2), its default the one that measured best at 50 000, 20 000 and
// 6 250 genes of C3 (m = 500) and at C2 / C4 (profiles/launch_order.md), list order where no key separated from it:
//   gene-wise fit_beta   ascending baseMean (C3: 1.25 -> 1.19 ms at 50 000 genes, 0.60 -> 0.50 at 20 000, 0.30 -> 0.20 at 6 250)
//   gene-wise fit_disp   descending baseMean for rows of 256 .. 1024 samples without weights (C3: 2.48 -> 2.45 ms, 1.23 -> 1.10
//                        at 20 000 genes).  The same order LOSES 0.035 of 0.39 ms at C2 (m = 100) and 0.4 of 11.1 ms at C4
//                        (m = 2000, rows through L2): list order there; with weights the search does not run over the
//                        distinct counts, which is what the mean stands for
//   MAP fit_disp         descending baseMean up to DSQ_LPT_MAXN = 16 384 genes (0.40 -> 0.37 ms at 6 250); from 20 000 genes no
//                        key of the four tried separates from list order, and at 50 000 all four are slower
//   test's fit_beta      ascending baseMean (C3: 1.27 -> 1.22 ms; by the first fit's iterations 1.23; C4: 5.88 -> 5.76)
constexpr int kLptBuilds = 3;          // per call: the gene-wise phase's list (both directions), the MAP search's, the test's fit's
static bool lpt_applies(const Pipe &P, const Rows &rw) {
    return tuning().lpt && rw.rows == P.rows_nz && P.lpt_bins && (tuning().lpt >= 2 || P.m >= 256);
}
static LptKey lpt_key(const Pipe &P, int kind) {
    LptKey k = {kind, nullptr, nullptr, nullptr};
    switch (kind) {
    case LPT_MEAN_UP: case LPT_MEAN_DOWN: k.kd = P.o->baseMean; break;
    case LPT_ITER: k.ki = P.iter; break;                               // the gene-wise search's
    case LPT_ITER_F64: k.kd = P.beta_iter; break;                      // the gene-wise IRLS's
    case LPT_ITER_MEAN: k.ki = P.iter; k.kd = P.o->baseMean; break;
    case LPT_DIST: k.kd = P.la_init; k.kd2 = P.log_dfit; break;        // start value against prior mean
    default: k.kind = LPT_NONE;
    }
    return k;
}
static const char *lpt_key_name(int kind) {
    static const char *const nm[] = {"none", "baseMean ascending", "baseMean descending", "dispersion iterations", "IRLS iterations",
                                     "dispersion iterations x log2 mean", "|start - prior mean|"};
    return kind >= 0 && kind <= LPT_DIST ? nm[kind] : "?";
}
// the rule kernel in front of the launch builds the histogram: its parameter block gets the key and a zeroed bin block
static void lpt_arm(Pipe &P, RuleParams &q, int kind) {
    q.lpt = lpt_key(P, kind);
    if (q.lpt.kind == LPT_NONE || P.lpt_next >= kLptBuilds) { q.lpt.kind = LPT_NONE; return; }
    q.lpt_bins = P.lpt_bins + (size_t)2 * kLptBins * P.lpt_next++;
}
// DSQ_VERBOSE only: one look at a list the chain has built -- a permutation of the launch's rows? -- and one line per launch
static int lpt_verbose(Pipe &P, const char *launch, const char *key, const Rows &rw, const int32_t *list) {
    if (!getenv("DSQ_VERBOSE")) return DSQ_OK;
    DSQ_HIP(hipStreamSynchronize(P.st));
    int cnt = 0;
    DSQ_HIP(hipMemcpy(&cnt, rw.n_dev, sizeof cnt, hipMemcpyDeviceToHost));
    if (cnt < 0 || cnt > P.n) return capi_fail(DSQ_ERR_DEVICE, "launch order of %s: %d rows of %d", launch, cnt, P.n);
    std::vector<int32_t> a((size_t)cnt), b((size_t)cnt);
    if (cnt) {
        DSQ_HIP(hipMemcpy(a.data(), rw.rows, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
        DSQ_HIP(hipMemcpy(b.data(), list, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    if (a != b) return capi_fail(DSQ_ERR_DEVICE, "launch order of %s (key: %s): the list is no permutation of the %d rows", launch, key, cnt);
    fprintf(stderr, "[dsq] launch order: %s by %s, %d rows, permutation ok\n", launch, key, cnt);
    return DSQ_OK;
}
// the second pass: the rows of `rw` by the key of `q` (armed, histogram built by the rule kernel) -> rows_lpt, and backwards
// -> rev
static int lpt_scatter(Pipe &P, const Rows &rw, const RuleParams &q, int32_t *rev) {
    capi_prof_begin("lpt_order", P.n, P.st);
    hipLaunchKernelGGL(lpt_scatter_kernel, ew_grid(P.n), dim3(256), 0, P.st, rw, q.lpt, (const int *)q.lpt_bins, q.lpt_bins + kLptBins,
                       P.rows_lpt, rev);
    capi_prof_end(P.st);
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// estimateDispersionsGeneEst on the rows `rw` of the count matrix y (R/core.R:657-860, niter = 1); mu-hat -> mu_hat
static int gene_est(Pipe &P, const Rows &rw, const int32_t *y, double *mu_hat, int cnt_grid, int cnt_optim,
                    int32_t *optim_flag) {
    const DsqDeseqArgs *a = P.a;
    RuleParams q = rule_params(P, rw);
    // one list by ascending baseMean for the IRLS, read backwards for the search
    const bool ord_beta = lpt_applies(P, rw) && !a->linearMu && tuning().lpt_key1 != 0;
    const bool ord_disp = lpt_applies(P, rw) && (tuning().lpt_keyd == 2 || (tuning().lpt_keyd == 1 && P.m >= 256 && P.m <= 1024 && !a->useWeights));
    if (ord_beta || ord_disp) lpt_arm(P, q, LPT_MEAN_UP);
    hipLaunchKernelGGL(alpha_init_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    int rc;
    const bool ordered = q.lpt.kind != LPT_NONE;
    int32_t *rev = (ordered && ord_disp) ? P.rows_grid : nullptr;        // (free until gene_est_post_kernel lists the stragglers)
    if (ordered && (rc = lpt_scatter(P, rw, q, rev))) return rc;
    const Rows up = {P.rows_lpt, rw.n_dev, rw.n}, down = {rev, rw.n_dev, rw.n};
    q.lpt.kind = LPT_NONE;
    if (a->linearMu) {
        bool ok = false;
        capi_prof_begin("linear_mu", P.n, P.st);
        DSQ_HIP(launch_linear_mu(prefit_params(P, rw, y), P.ge_floor, mu_hat, P.st, &ok));     // minmu of estimateDispersionsGeneEst (:763)
        capi_prof_end(P.st);
        if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: p=%d", P.p);
    } else {
        // fitNbinomGLMs(alpha_hat = alpha_hat) with mu floored at minmu (R/core.R:755-763); rows the IRLS leaves
        // to the optim fallback are flagged for the caller
        // (the arguments of THIS fitNbinomGLMs call are its defaults -- betaTol 1e-8, maxit 100, QR, the IRLS's own minmu
        // 0.5, R/core.R:755-757; the caller's minmu is the FLOOR of the fitted means it hands to the search, :763)
        // (the rows with the fewest counts first -- they take the most iterations; see lpt_scatter_kernel)
        if (ordered && ord_beta && (rc = lpt_verbose(P, "gene-wise fit_beta", lpt_key_name(LPT_MEAN_UP), rw, up.rows))) return rc;
        rc = launch_fit_beta(P, (ordered && ord_beta) ? up : rw, y, P.alpha_init, a->weights_norm, mu_hat, P.ge_floor, nullptr,
                             1e-8, 100, 1, 0.5, "fit_beta");
        if (rc) return rc;
        RuleParams b = rule_params(P, rw);
        b.betaMaxit = 100;
        b.optim_flag = optim_flag; b.optim_count = P.counters + cnt_optim;
        hipLaunchKernelGGL(beta_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, b);
        // rows the IRLS left: the fallback's fitted means (floored at minmu, :763) replace theirs before the search
        rc = launch_optim(P, cnt_optim, y, P.alpha_init, a->weights_norm, 0.5, P.ge_floor, P.opt_beta, P.opt_se, P.opt_ll, mu_hat);
        if (rc) return rc;
    }
    if (rev && (rc = lpt_verbose(P, "gene-wise fit_disp", lpt_key_name(LPT_MEAN_DOWN), rw, rev))) return rc;
    P.rows_rev = rev;
    rc = launch_fit_disp(P, rev ? down : rw, y, mu_hat, P.la0, P.la0, false, a->weights_floor, a->useCR != 0, false, "fit_disp");
    P.rows_rev = nullptr;
    if (rc) return rc;
    q.grid_count = P.counters + cnt_grid;
    hipLaunchKernelGGL(gene_est_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    Rows gr = {P.rows_grid, P.counters + cnt_grid, P.n};
    rc = launch_fit_disp(P, gr, y, mu_hat, P.la0, P.la0, false, a->weights_floor, a->useCR != 0, true, "fit_disp_grid");
    if (rc) return rc;
    hipLaunchKernelGGL(gene_est_final_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// estimateDispersionsMAP (R/core.R:943-1131) on the rows `rw`
static int map_est(Pipe &P, const Rows &rw, const int32_t *y, const double *mu_hat, int cnt_grid) {
    const DsqDeseqArgs *a = P.a;
    RuleParams q = rule_params(P, rw);
    const int keym = (lpt_applies(P, rw) && (tuning().lpt_maxn <= 0 || P.n <= tuning().lpt_maxn)) ? tuning().lpt_keym : 0;
    if (keym) lpt_arm(P, q, keym);
    hipLaunchKernelGGL(map_init_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    int rc;
    const bool ordered = q.lpt.kind != LPT_NONE;
    if (ordered && ((rc = lpt_scatter(P, rw, q, nullptr)) || (rc = lpt_verbose(P, "MAP fit_disp", lpt_key_name(q.lpt.kind), rw, P.rows_lpt)))) return rc;
    q.lpt.kind = LPT_NONE;
    rc = launch_fit_disp(P, ordered ? Rows{P.rows_lpt, rw.n_dev, rw.n} : rw, y, mu_hat, P.la_init, P.log_dfit, true, a->weights_norm,
                         a->useCR != 0, false, "fit_disp");
    if (rc) return rc;
    q.grid_count = P.counters + cnt_grid;
    hipLaunchKernelGGL(map_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    Rows gr = {P.rows_grid, P.counters + cnt_grid, P.n};
    rc = launch_fit_disp(P, gr, y, mu_hat, P.la_init, P.log_dfit, true, a->weights_norm, true, true, "fit_disp_grid");   // useCR = TRUE, :1061
    if (rc) return rc;
    // the test's fit follows on the same rows (test_fit): its order's histogram is this kernel's.  The key: baseMean as for
    // the gene-wise fit, or (DSQ_LPT_KEY2 = 0) the iteration counts of the gene-wise estimate's IRLS when that fit ran
    P.lpt_test.kind = LPT_NONE;
    if (lpt_applies(P, rw) && !a->betaPrior && tuning().lpt_key2 != 2) {
        const int kind = tuning().lpt_key2 == 1 ? LPT_MEAN_UP : (a->linearMu ? LPT_NONE : LPT_ITER_F64);
        lpt_arm(P, q, kind);
        P.lpt_test = q.lpt; P.lpt_test_bins = q.lpt_bins;
    }
    hipLaunchKernelGGL(map_final_kernel, ew_grid(P.n), dim3(256), 0, P.st, q);
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// the start values of a GLM fit on a rank-deficient (expanded) model matrix (R/fitNbinomGLMs.R:146-155): the intercept
// column starts at the log of the UNWEIGHTED mean normalized count, every other coefficient at 0 (or all at 1 when the
// first column is not an intercept)
__global__ void prior_start_kernel(Rows rw, int n, int p, int intercept, const double *bm, double *binit) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_count(rw)) return;
    const int g = rows_gene(rw, i);
    for (int c = 0; c < p; c++) binit[(size_t)g + (size_t)n * c] = intercept ? (c == 0 ? dlog(bm[g]) : 0.0) : 1.0;
}

// fitGLMsWithPrior's first pass (R/fitNbinomGLMs.R:256-260): the MLE fit on the design with the wide prior.  Its fitted
// means and hat diagonals are the ones the object keeps (R/core.R:1429-1431); its coefficients feed the prior variance.
static int mle_fit(Pipe &P, const Rows &rw, const int32_t *y, double *mu_out, double *hat) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    int rc = launch_fit_beta(P, rw, y, o->dispersion, a->weights_norm, mu_out, 0.0, hat, P.t_tol, P.t_maxit, P.t_useQR,
                             P.t_minmu, "fit_beta_mle");
    if (rc) return rc;
    const int cnt3 = P.tag[0] ? CNT_OPT3R : CNT_OPT3;
    RuleParams b = rule_params(P, rw);
    b.beta = o->mle_beta; b.betaSE = P.red_se; b.wald = 0;
    b.optim_flag = P.grid_flag; b.optim_count = P.counters + cnt3;           // (the grid flags are free between the searches)
    hipLaunchKernelGGL(beta_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, b);
    rc = launch_optim(P, cnt3, y, o->dispersion, a->weights_norm, P.t_minmu, 0.0, o->mle_beta, P.red_se, P.opt_ll, mu_out);
    if (rc) return rc;
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// what follows the IRLS of a test's GLM fit on the design `which`: beta_post (log2 scale, Wald columns, betaConv, the rows for
// the optim fallback, R/fitNbinomGLMs.R:185-227) -> the fallback on those rows: coefficients, standard errors, logLike
// (:398-399) and fitted means (:386) in place -> optim_post: betaConv and the Wald columns from them
static int beta_post_optim(Pipe &P, const Rows &rw, const int32_t *y, int which, int wald, int cnt_optim, double *mu_out) {
    const DsqDeseqOut *o = P.o;
    const DesignSel ds = design_of(P, which);
    RuleParams b = rule_params(P, rw);
    b.p = ds.p_true; b.beta_init = ds.beta_init;
    b.beta = o->beta; b.betaSE = o->betaSE; b.stat = o->stat; b.pvalue = o->pvalue; b.wald = wald;
    b.betaConv = o->betaConv; b.betaIter_out = o->betaIter;
    b.optim_flag = o->optim_test; b.optim_count = P.counters + cnt_optim;
    hipLaunchKernelGGL(beta_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, b);
    if (which != DES_FULL && ds.p > ds.p_true)   // (columns p_true .. of the optim start values may hold another fit's: zero on the padding)
        DSQ_HIP(hipMemsetAsync(P.opt_start + (size_t)P.n * ds.p_true, 0, (size_t)P.n * (ds.p - ds.p_true) * sizeof(double), P.st));
    int rc = launch_optim(P, cnt_optim, y, o->dispersion, P.a->weights_norm, P.t_minmu, 0.0, o->beta, o->betaSE, o->logLike, mu_out, which);
    if (rc) return rc;
    const Rows orw = {P.rows_opt, P.counters + cnt_optim, P.n};
    RuleParams ob = rule_params(P, orw);
    ob.p = ds.p_true;
    ob.beta = o->beta; ob.betaSE = o->betaSE; ob.stat = o->stat; ob.pvalue = o->pvalue; ob.wald = wald; ob.betaConv = o->betaConv;
    hipLaunchKernelGGL(optim_post_kernel, dim3(16), dim3(256), 0, P.st, ob);
    return DSQ_OK;
}

// ... and its second pass (:311-325): the fit with lambda = 1 / betaPriorVar on the standard or the expanded model
// matrix; coefficients, standard errors, Wald statistics, betaConv, betaIter and logLike are this fit's
static int prior_fit(Pipe &P, const Rows &rw, const int32_t *y, int cnt_optim) {
    const DsqDeseqArgs *a = P.a;
    int rc;
    if (a->prior_expanded) {
        // getBaseMeansAndVariances without weights on the intercept-only design (only baseMean is read)
        bool ok = false;
        DSQ_HIP(launch_prefit(prefit_other(P, rw, y, 1, a->x_prior, a->x_prior, P.lam, P.opt_ll), P.st, &ok));
        if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: prefit p=1");
        hipLaunchKernelGGL(prior_start_kernel, ew_grid(P.n), dim3(256), 0, P.st, rw, P.n, a->p_prior, a->prior_intercept,
                           (const double *)P.cnum, P.red_binit);
        if (P.pri_pk > a->p_prior)        // (start values 0 on the padding of a wide expanded design)
            DSQ_HIP(hipMemsetAsync(P.red_binit + (size_t)P.n * a->p_prior, 0, (size_t)P.n * (P.pri_pk - a->p_prior) * sizeof(double), P.st));
    }
    rc = launch_fit_beta(P, rw, y, P.o->dispersion, a->weights_norm, P.red_mu, 0.0, nullptr, P.t_tol, P.t_maxit, P.t_useQR,
                         P.t_minmu, "fit_beta_prior", DES_PRIOR);
    if (rc) return rc;
    capi_prof_begin(P.tag[0] ? "nbinom_loglike:refit" : "nbinom_loglike", P.n, P.st);
    DSQ_HIP(launch_loglike(loglike_params(P, rw, y, P.red_mu, P.o->logLike), P.st));
    capi_prof_end(P.st);
    rc = beta_post_optim(P, rw, y, DES_PRIOR, 1, cnt_optim, P.red_mu);
    if (rc) return rc;
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

hipError_t launch_loglike_side(const LogLikeKernelParams &kp, hipStream_t st);       // aux.hip
hipError_t launch_xim_flagged(const double *nf, int n, int m, long ld, const int32_t *want_a, const int32_t *want_b, double *scratch_m,
                              double *out, hipStream_t st);
// the side stream's work has to be finished before anything that rewrites what it reads or reads what it writes
static int join_side(Pipe &P) {
    if (!P.forked) return DSQ_OK;
    P.forked = false;
    DSQ_HIP(hipEventRecord(P.ev_join, P.side));
    DSQ_HIP(hipStreamWaitEvent(P.st, P.ev_join, 0));
    return DSQ_OK;
}

// what the side stream is given from here on runs behind everything enqueued on the chain's stream so far
static int fork_side(Pipe &P) {
    if (P.forked) return DSQ_OK;
    DSQ_HIP(hipEventRecord(P.ev_fork, P.st));
    DSQ_HIP(hipStreamWaitEvent(P.side, P.ev_fork, 0));
    P.forked = true;
    return DSQ_OK;
}

// the deferred full-row nbinomLogLike: on the side stream (forked here) or on the chain's own stream
static int launch_pending_ll(Pipe &P, bool beside) {
    if (!P.ll_pending) return DSQ_OK;
    P.ll_pending = false;
    if (beside) {
        const int rc = fork_side(P);
        if (rc) return rc;
        DSQ_HIP(launch_loglike_side(P.ll, P.side));
    } else {
        DSQ_HIP(launch_loglike(P.ll, P.st));
    }
    return DSQ_OK;
}

// nbinomWaldTest / nbinomLRT(reduced = ~1) on the rows `rw` (R/core.R:1403-1408, 1471, 1507; 1850-1878)
static int test_fit(Pipe &P, const Rows &rw, const int32_t *y, double *mu_out, double *hat, int cnt_optim) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    if (a->betaPrior) return mle_fit(P, rw, y, mu_out, hat);         // (the prior fit follows once lambda is known)
    // (the order map_est has prepared for this launch)
    const bool ordered = P.lpt_test.kind != LPT_NONE && rw.rows == P.rows_nz;
    int rc;
    if (ordered) {
        RuleParams q = rule_params(P, rw);
        q.lpt = P.lpt_test; q.lpt_bins = P.lpt_test_bins;
        P.lpt_test.kind = LPT_NONE;
        if ((rc = lpt_scatter(P, rw, q, nullptr)) || (rc = lpt_verbose(P, "test fit_beta", lpt_key_name(q.lpt.kind), rw, P.rows_lpt))) return rc;
    }
    // (the main chain's fit, when the outlier phase wants the candidate rows first and this fit runs on the kernel that knows
    //  the bound: the flags go to the grid flags, free between the MAP search and the refit's -- not beside nbinomLRT's
    //  reduced fit, which counts its optim rows there)
    const bool cand = P.outlier_first && !P.tag[0] && hat && !(a->test == 1 && a->x_red) && fit_beta_on_cells(P.pk, P.ncell);
    rc = launch_fit_beta(P, ordered ? Rows{P.rows_lpt, rw.n_dev, rw.n} : rw, y, o->dispersion, a->weights_norm, mu_out, 0.0, hat,
                         P.t_tol, P.t_maxit, P.t_useQR, P.t_minmu, "fit_beta", DES_FULL, cand);
    if (rc) return rc;
    if (cand) P.cand_ready = true;
    LogLikeKernelParams lk = loglike_params(P, rw, y, mu_out, o->logLike);
    // OVERLAP (the main chain, when this call also runs the outlier phase): nothing on the way to the refit of the replaced
    // rows reads the log likelihoods -- beta_post / the optim fallback / Cook's distances / replaceOutliers / the refit's
    // own dispersion searches -- and the refit is latency, not throughput: a handful of rows, each one gene's serial search
    // (~0.45 ms of a 12.8 ms step at C3 on an otherwise idle device).  So the full-row nbinomLogLike is DEFERRED: phase_refit
    // launches it on a side stream when the refit starts (beside Cook's distances, another full-size launch, it would only
    // share the device: measured), run() behind everything else when there is no refit.  It leaves the rows flagged for the
    // optim fallback alone (`skip`): the fallback writes their logLike (and rewrites their fitted means) itself,
    // R/fitNbinomGLMs.R:386,398-399.  What it may read half-updated -- the dispersion of a row the refit is re-estimating --
    // only feeds that row's logLike, which the refit's own test fit writes after the join (join_side before its test_fit).
    if (P.overlap && !P.tag[0]) {
        P.ll = lk;
        P.ll.skip = o->optim_test;
        P.ll_pending = true;
    } else {
        capi_prof_begin(P.tag[0] ? "nbinom_loglike:refit" : "nbinom_loglike", P.n, P.st);
        DSQ_HIP(launch_loglike(lk, P.st));
        capi_prof_end(P.st);
    }
    rc = beta_post_optim(P, rw, y, DES_FULL, (a->test == 0) ? 1 : 0, cnt_optim, mu_out);
    if (rc) return rc;
    if (a->test == 1 && a->x_red) {
        // nbinomLRT's reduced fit (R/core.R:1856-1868): fitNbinomGLMs on the reduced model matrix at the same
        // dispersions -- QR start values, IRLS, logLik at its fitted means, its own optim-fallback rows
        bool ok = false;
        capi_prof_begin(P.tag[0] ? "prefit_reduced:refit" : "prefit_reduced", P.n, P.st);
        DSQ_HIP(launch_prefit(prefit_other(P, rw, y, a->p_red, a->q_red, a->a_red, a->r_red, P.red_binit), P.st, &ok));
        capi_prof_end(P.st);
        if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: reduced design with p=%d", a->p_red);
        rc = launch_fit_beta(P, rw, y, o->dispersion, a->weights_norm, P.red_mu, 0.0, nullptr, P.t_tol, P.t_maxit, P.t_useQR,
                             P.t_minmu, "fit_beta_reduced", DES_REDUCED);
        if (rc) return rc;
        lk.mu = P.red_mu; lk.loglike = o->logLikeReduced;
        capi_prof_begin(P.tag[0] ? "nbinom_loglike_red:refit" : "nbinom_loglike_red", P.n, P.st);
        DSQ_HIP(launch_loglike(lk, P.st));
        capi_prof_end(P.st);
        const int cnt3 = P.tag[0] ? CNT_OPT3R : CNT_OPT3;
        RuleParams rb = rule_params(P, rw);
        rb.p = a->p_red; rb.beta_init = P.red_binit;
        rb.optim_flag = P.grid_flag; rb.optim_count = P.counters + cnt3;      // (the grid flags are free between the searches)
        hipLaunchKernelGGL(beta_post_kernel, ew_grid(P.n), dim3(256), 0, P.st, rb);
        if (P.red_pk > a->p_red)         // (columns p_red .. of the start values may hold the full fit's: zero on the padding)
            DSQ_HIP(hipMemsetAsync(P.opt_start + (size_t)P.n * a->p_red, 0, (size_t)P.n * (P.red_pk - a->p_red) * sizeof(double), P.st));
        rc = launch_optim(P, cnt3, y, o->dispersion, a->weights_norm, P.t_minmu, 0.0, P.red_beta, P.red_se, o->logLikeReduced,
                          P.red_mu, DES_REDUCED);
        if (rc) return rc;
    } else if (a->test == 1) {
        InterceptKernelParams ik = fit_head<InterceptKernelParams>(P, rw, y, a->weights_norm);
        ik.alpha = o->dispersion; ik.beta_log2 = P.cnum; ik.betaSE = P.cden;      // not read by nbinomLRT
        ik.loglike = o->logLikeReduced;
        ik.kconst = P.kconst;            // (the full model's fit of the same rows: same counts, dispersions, weights)
        capi_prof_begin("intercept_fit", P.n, P.st);
        DSQ_HIP(launch_intercept_fit(ik, P.st));
        capi_prof_end(P.st);
    }
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// design cells -> sample permutation grouped by cell, offsets, ">= 3 in cell" flags (nOrMoreInCell, R/core.R:2366), the
// replaceable flags: small host arrays, uploaded for the outlier kernels
struct OutlierMeta {
    int32_t *dperm, *din3, *drepl, *duse3, *dstart;
    int maxcell, any3, all_rep;
};
static int outlier_meta(const DsqDeseqArgs *a, int m, hipStream_t st, OutlierMeta *M) {
    static thread_local std::vector<int32_t> meta;   // (capi_upload_table takes its own copy)
    meta.assign((size_t)4 * m + a->ncell + 1, 0);
    int32_t *perm = meta.data(), *in3 = perm + m, *repl = in3 + m, *use3 = repl + m, *start = use3 + m;
    for (int j = 0; j < m; j++) {
        if (a->cell_of[j] < 0 || a->cell_of[j] >= a->ncell) return capi_fail(DSQ_ERR_VALUE, "cell_of[%d] out of range", j);
        start[a->cell_of[j] + 1]++;
    }
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
    int all_rep = 1;
    for (int j = 0; j < m; j++) {
        in3[j] = (start[a->cell_of[j] + 1] - start[a->cell_of[j]]) >= 3;
        use3[j] = in3[j];
        repl[j] = a->replaceable[j] ? 1 : 0;
        if (!repl[j]) all_rep = 0;
    }
    void *mv;
    int rc = capi_upload_table(DSQ_WS_PIPE_OUTLIER_META, meta.data(), meta.size() * sizeof(int32_t), st, &mv);
    if (rc) return rc;
    M->dperm = (int32_t *)mv; M->din3 = M->dperm + m; M->drepl = M->din3 + m; M->duse3 = M->drepl + m; M->dstart = M->duse3 + m;
    M->maxcell = maxcell; M->any3 = any3; M->all_rep = all_rep;
    return DSQ_OK;
}

// the closing steps of refitWithoutOutliers that ask whether ANY row of the analysis was refitted (R/core.R:2496):
// result columns of the rows that became all zero are NA (:2535), maxCooks is recomputed (:2538-2546)
static int outlier_finish(Pipe &P, const Rows &nz, const Rows &rep, const OutlierMeta &M, const int32_t *n_refit) {
    const DsqDeseqOut *o = P.o;
    const int n = P.n, m = P.m, p = P.p;
    NaRowsParams nr;
    memset(&nr, 0, sizeof nr);
    nr.rw = rep; nr.n = n; nr.p = P.a->betaPrior ? P.a->p_prior : p; nr.allZero = o->allZero; nr.n_refit = n_refit;
    nr.beta = o->beta; nr.betaSE = o->betaSE; nr.stat = o->stat; nr.pvalue = o->pvalue; nr.betaIter = o->betaIter;
    nr.logLike = o->logLike; nr.logLikeReduced = o->logLikeReduced; nr.maxCooks = o->maxCooks; nr.betaConv = o->betaConv;
    hipLaunchKernelGGL(na_rows_kernel, ew_grid(n), dim3(256), 0, P.st, nr);
    int grid = (n + 3) / 4, capg = device_cu_count() * 8;
    if (grid > capg) grid = capg;
    hipLaunchKernelGGL(masked_max_kernel, dim3(grid), dim3(256), 0, P.st, nz, m, P.ld, (const double *)o->cooks,
                       (const int32_t *)M.duse3, (const int32_t *)M.drepl, M.all_rep, (m > p && M.any3) ? 1 : 0, n_refit,
                       o->maxCooks);
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

static size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

// ---- the caller's workspace, stated ONCE: every vector of it, in layout order, with its length ----------------------
// The walker below visits the table twice: without a base to size the workspace (dsq_deseq_workspace_bytes, ABI) and with
// one to bind the Pipe's pointers.  Every entry starts on a multiple of 8 elements; all doubles come first, the int32
// entries follow them (so the int base is known when the first of them is visited); 256 spare bytes close it.  The row
// lists and counters persist between the phases of one analysis.  p: the columns of the n x . work matrices.
struct WsWalk {
    double *D;                     // nullptr: size only
    size_t d = 0, i = 0;           // doubles / int32s taken so far
    void operator()(double *&f, size_t k) { if (D) f = D + d; d += align8(k); }
    void operator()(int32_t *&f, size_t k) { if (D) f = (int32_t *)(D + d) + i; i += align8(k); }
    size_t bytes() const { return d * sizeof(double) + i * sizeof(int32_t) + 256; }
};
static size_t workspace_table(Pipe &P, int n, int p, int nt, double *base) {
    const size_t nd = align8((size_t)n), np_ = align8((size_t)n * p), ntd = align8((size_t)nt);
    WsWalk v{base};
    v(P.roughDisp, nd); v(P.beta_init, np_); v(P.alpha_init, nd); v(P.la0, nd); v(P.la_out, nd);
    v(P.last_change, nd); v(P.initial_lp, nd); v(P.initial_dlp, nd); v(P.last_lp, nd); v(P.last_dlp, nd);
    v(P.la_grid, nd); v(P.log_dfit, nd); v(P.la_init, nd); v(P.beta_nat, np_); v(P.beta_var, np_);
    v(P.beta_iter, nd); v(P.cnum, nd); v(P.cden, nd); v(P.dev, nd);
    v(P.lam, 3 * (size_t)p + 8);   // lam | contrast | lam_prior, p each, and the two xim scalars behind them
    v(P.resbuf, ntd); v(P.trend_mean_c, ntd); v(P.trend_disp_c, ntd); v(P.robustDisp, nd);
    v(P.opt_start, np_); v(P.opt_beta, np_); v(P.opt_se, np_); v(P.opt_ll, nd);
    v(P.red_binit, np_); v(P.red_beta, np_); v(P.red_se, np_); v(P.kconst, nd);
    int32_t *spare;                // (16 ints: the row-list counters lived here before they became the caller's status block)
    v(P.iter, nd); v(P.iter_accept, nd); v(P.grid_flag, nd); v(P.rows_nz, nd); v(P.rows_grid, nd);
    v(P.rows_rep, nd); v(P.rows_refit, nd); v(spare, 16); v(P.work_counters, 64);
    v(P.rows_opt, nd); v(P.opt_conv, nd); v(P.rows_lpt, nd);
    return v.bytes();
}

// every validation in front of the first look at the device
static int check_args(const DsqDeseqArgs *a, const DsqDeseqOut *o) {
    if (!a || !o) return capi_fail(DSQ_ERR_ARG, "NULL args/out");
    if (a->n < 1 || a->m < 2 || a->p < 1 || a->m <= a->p) return capi_fail(DSQ_ERR_ARG, "bad dimensions n=%d m=%d p=%d", a->n, a->m, a->p);
    if (a->p > DSQ_P_WIDE) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: p=%d > %d design columns", a->p, DSQ_P_WIDE);
    if (a->betaPrior) {
        if (a->test != 0) return capi_fail(DSQ_ERR_ARG, "betaPrior: Wald test only (R/core.R:1787)");
        if (!a->x_prior || a->p_prior < 1 || !o->mle_beta) return capi_fail(DSQ_ERR_ARG, "betaPrior needs x_prior / p_prior / mle_beta");
        if (a->p_prior > DSQ_P_WIDE) return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: %d columns in the prior pass > %d", a->p_prior, DSQ_P_WIDE);
        if ((a->phases & DSQ_PH_PRIOR) && !a->lambda_prior) return capi_fail(DSQ_ERR_ARG, "DSQ_PH_PRIOR needs lambda_prior");
        if ((a->phases & (DSQ_PH_OUTLIERS | DSQ_PH_OUTLIERS_REFIT)) && a->do_replace && !a->lambda_prior) return capi_fail(DSQ_ERR_ARG, "betaPrior: the outlier refit needs lambda_prior");
    }
    if (a->ld < a->m) return capi_fail(DSQ_ERR_ARG, "ld < m");
    // estimateDispersionsPriorVar's branch for 1..3 residual degrees of freedom matches a seeded Monte-Carlo sample
    // (R/core.R:1155-1190, R's RNG + loess): not reproducible here, so the prior variance is not computed at all
    if ((a->phases & DSQ_PH_TREND) && a->m - a->p <= 3 && !(a->dispPriorVar_in > 0.0))
        return capi_fail(DSQ_ERR_UNSUPPORTED, "dsq_deseq_dev: %d residual degrees of freedom: the prior variance of R/core.R:1155-1190 (seeded Monte-Carlo matching) is the caller's (dispPriorVar_in)", a->m - a->p);
    if (!a->y || !a->nf || !a->x || !a->q || !a->a || !a->r || !a->disp_grid || a->ngrid < 2 || !a->lambda) return capi_fail(DSQ_ERR_ARG, "NULL input");
    if (a->trend_mean && (!a->trend_disp || a->n_trend < 1)) return capi_fail(DSQ_ERR_ARG, "trend vectors");
    if (a->useWeights && (!a->weights_raw || !a->weights_norm || !a->weights_floor)) return capi_fail(DSQ_ERR_ARG, "useWeights without weights");
    if (a->test != 0 && a->test != 1) return capi_fail(DSQ_ERR_ARG, "test must be 0 (Wald) or 1 (LRT)");
    // the chain's nbinomLogLike reads K' (the mu-independent part of the row's log density) from the fitBeta launch in
    // front of it, and that launch forms K' inside its IRLS set-up: a chain without IRLS iterations has no K'
    if (a->betaMaxit < 1) return capi_fail(DSQ_ERR_ARG, "dsq_deseq_dev: betaMaxit must be >= 1 (DESeq() itself runs maxit = 100)");
    if (a->fitType < DSQ_FIT_PARAMETRIC || a->fitType > DSQ_FIT_PARAMETRIC_OR_MEAN) return capi_fail(DSQ_ERR_ARG, "fitType must be one of DSQ_FIT_*");
    if (a->dispFit_in && a->trend_mean && !a->trend_fit_in) return capi_fail(DSQ_ERR_ARG, "dispFit_in with gathered trend vectors needs trend_fit_in");
    if (a->dispFit_in && (a->phases & DSQ_PH_OUTLIERS) && a->do_replace)
        return capi_fail(DSQ_ERR_ARG, "dispFit_in: the refit of replaced rows needs the trend at their NEW means -- split the phase (DSQ_PH_OUTLIERS_DETECT, update dispFit_in at the replaced rows, DSQ_PH_OUTLIERS_REFIT) or run with do_replace = 0");
    if ((a->phases & DSQ_PH_OUTLIERS) && (a->phases & (DSQ_PH_OUTLIERS_DETECT | DSQ_PH_OUTLIERS_REFIT)))
        return capi_fail(DSQ_ERR_ARG, "DSQ_PH_OUTLIERS is both halves: do not combine it with DSQ_PH_OUTLIERS_DETECT / _REFIT");
    if (a->x_red && (a->test != 1 || !a->q_red || !a->a_red || !a->r_red || a->p_red < 1 || a->p_red >= a->p))
        return capi_fail(DSQ_ERR_ARG, "reduced model: LRT only, with its QR factors and 1 <= p_red < p");
    if (!o->baseMean || !o->baseVar || !o->allZero || !o->dispGeneEst || !o->dispGeneIter || !o->dispFit || !o->dispMAP ||
        !o->dispersion || !o->dispIter || !o->dispOutlier || !o->beta || !o->betaSE || !o->betaConv || !o->betaIter ||
        !o->logLike || !o->maxCooks || !o->replace || !o->optim_geneest || !o->optim_test || !o->mu_hat || !o->mu || !o->H ||
        !o->cooks || !o->replaceCounts || !o->status || !o->scalars)
        return capi_fail(DSQ_ERR_ARG, "NULL output");
    if (a->test == 0 && (!o->stat || !o->pvalue)) return capi_fail(DSQ_ERR_ARG, "Wald test needs stat / pvalue outputs");
    if (a->test == 1 && !o->logLikeReduced) return capi_fail(DSQ_ERR_ARG, "LRT needs logLikeReduced");
    if ((a->phases & (DSQ_PH_OUTLIERS | DSQ_PH_OUTLIERS_DETECT | DSQ_PH_OUTLIERS_REFIT | DSQ_PH_FINISH)) && (!a->cell_of || !a->replaceable || a->ncell < 1)) return capi_fail(DSQ_ERR_ARG, "outlier phase needs cell_of / replaceable");
    return DSQ_OK;
}

// the call's settings, the caller's workspace (workspace_table) and the fit kernels' scratch slot -> P
static int bind(Pipe &P, const DsqDeseqArgs *a, const DsqDeseqOut *o, hipStream_t st) {
    P.a = a; P.o = o; P.st = st; P.tag = "";
    P.t_tol = a->betaTol; P.t_maxit = a->betaMaxit; P.t_useQR = a->useQR; P.t_minmu = a->minmu; P.ge_floor = a->minmu;
    // (see test_fit) only when the test's fit and the outlier phase are enqueued by this one call; the profiling passes
    // time every launch on one stream; DSQ_OVERLAP=0 switches it off
    P.overlap = tuning().overlap && !capi_prof_on() && !a->betaPrior && (a->phases & DSQ_PH_MAP_TEST) && (a->phases & DSQ_PH_OUTLIERS);
    if (P.overlap && capi_side_stream(&P.side, &P.ev_fork, &P.ev_join) != DSQ_OK) P.overlap = false;
    // (phase_outlier_first) the whole chain in one call: the gene-wise phase's fills have zeroed the replace flags
    P.outlier_first = P.overlap && tuning().outlier_first && a->do_replace && (a->phases & DSQ_PH_GENE_EST);
    const int n = P.n = a->n, m = P.m = a->m;
    P.p = a->p; P.ld = a->ld;
    P.maxDisp = m > 10 ? (double)m : 10.0;
    P.min_log_alpha = a->min_log_alpha;
    P.pk = kern_width(a->p);
    P.pkp = a->betaPrior ? kern_width(a->p_prior) : 0;
    P.pmax = P.pkp > P.pk ? P.pkp : P.pk;
    const int nt_cap = a->n_trend > n ? a->n_trend : n;      // (n_trend is the capacity even in the phases without a trend)
    const size_t need = workspace_table(P, n, P.pmax, nt_cap, nullptr);
    if (!a->workspace || a->workspace_bytes < (int64_t)need)
        return capi_fail(DSQ_ERR_ARG, "workspace of %lld bytes, dsq_deseq_workspace_bytes() asks for %zu", (long long)a->workspace_bytes, need);
    workspace_table(P, n, P.pmax, nt_cap, (double *)a->workspace);
    P.contrast = P.lam + P.pmax; P.lam_prior = P.contrast + P.pmax; P.xim_dev = P.lam + 3 * (size_t)P.pmax; P.xim_cur = P.xim_dev;
    P.counters = o->status;
    size_t slab_d = 0, cscr_d = 0;
    dispatch_beta_scratch(P.pk, n, m, a->useWeights, &slab_d, &cscr_d);
    if (a->x_red || a->betaPrior) {
        size_t s2 = 0, c2 = 0;
        dispatch_beta_scratch(a->betaPrior ? P.pkp : kern_width(a->p_red), n, m, a->useWeights, &s2, &c2);
        if (s2 > slab_d) slab_d = s2;
        if (c2 > cscr_d) cscr_d = c2;
    }
    void *b;
    const size_t lpt_bytes = tuning().lpt ? (size_t)kLptBuilds * 2 * kLptBins * sizeof(int) : 0;
    int rc = capi_ws_get(DSQ_WS_PIPE_SCRATCH, (slab_d + cscr_d) * sizeof(double) + 64 + lpt_bytes, &b);
    if (rc) return rc;
    P.scratch = (double *)b; P.cscratch = (double *)b + slab_d;
    P.lpt_bins = lpt_bytes ? (int *)((double *)b + slab_d + cscr_d + 8) : nullptr;
    return DSQ_OK;
}

// one more region for chain_init_kernel; neighbouring regions with the same pattern are one segment.  kInitSegMax is
// every region a call can ask for, so the bound cannot be met (`full` would say so at the launch)
struct InitFills {
    InitParams ip;
    bool full;
    void add(void *p_, size_t bytes, uint32_t val) {
        if (!p_ || !bytes) return;
        InitSeg *last = ip.nseg ? &ip.seg[ip.nseg - 1] : nullptr;
        if (last && last->val == val && (char *)last->p + 4 * (size_t)last->words == (char *)p_ && (size_t)last->words + bytes / 4 < 0xFFFFFFFFull)
            last->words += (uint32_t)(bytes / 4);
        else if (ip.nseg < kInitSegMax) ip.seg[ip.nseg++] = {(uint32_t *)p_, (uint32_t)(bytes / 4), val};
        else full = true;
    }
};

// the values the trend phase works on: the gathered vectors of a sharding caller, else this call's genes.  launch_init_fills
// sizes the prior variance's workspace by it and phase_trend launches with it: launch_prior_var chooses its kernel from the
// same number
static int trend_count(const Pipe &P) { return P.a->trend_mean ? P.a->n_trend : P.n; }

// ONE launch for every fill this call needs in front of its first kernel (chain_init_kernel): the dynamic-scheduling
// counters of the fit launches of THIS call, the ridge (R/fitNbinomGLMs.R:73,162) / default contrast (R/wrappers.R:105-108)
// / prior block, -- gene-wise phase -- the NA patterns of the result columns and the status block, -- trend phase -- the
// workspaces of the trend fit and of the sixteen-workgroup prior variance (fetched here, and only here)
static int launch_init_fills(Pipe &P) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    const int n = P.n, p = P.p, pmax = P.pmax;
    static thread_local InitFills f;
    InitParams &ip = f.ip;
    ip.nseg = 0; f.full = false;
    f.add(P.work_counters, 64 * sizeof(int32_t), 0u);
    if (P.lpt_bins && (a->phases & (DSQ_PH_GENE_EST | DSQ_PH_MAP_TEST))) f.add(P.lpt_bins, (size_t)kLptBuilds * 2 * kLptBins * sizeof(int), 0u);
    for (int c = 0; c < pmax; c++) {
        ip.blk[c] = c < p ? a->lambda[c] : (c < P.pk ? 1.0 : 0.0);          // (ridge 1 on the padding of a wide design)
        ip.blk[pmax + c] = (c == 0) ? 1.0 : 0.0;
        ip.blk[2 * pmax + c] = (a->betaPrior && a->lambda_prior) ? (c < a->p_prior ? a->lambda_prior[c] : (c < P.pkp ? 1.0 : 0.0)) : 0.0;
        if (a->x_red) ip.blk[2 * pmax + c] = c < a->p_red ? a->lambda[c] : (c < kern_width(a->p_red) ? 1.0 : 0.0);
    }
    ip.blk_dst = P.lam; ip.nblk = 3 * pmax;
    if (a->phases & DSQ_PH_GENE_EST) {
        // the outputs of a caller usually sit side by side (packed blocks): sorted by address, neighbours with the same
        // pattern merge
        struct Fill { char *p; size_t bytes; uint32_t val; };
        std::vector<Fill> fills;
        auto fill = [&](void *p_, size_t bytes, uint32_t val) { if (p_ && bytes) fills.push_back({(char *)p_, bytes, val}); };
        fill(o->status, DSQ_ST_COUNT * sizeof(int32_t), 0u);
        for (OutF64 v : kNaVectors) fill(o->*v, (size_t)n * sizeof(double), 0xFFFFFFFFu);
        for (OutF64 v : kNaMatrices) fill(o->*v, (size_t)n * (a->betaPrior ? a->p_prior : p) * sizeof(double), 0xFFFFFFFFu);
        if (a->betaPrior) fill(o->mle_beta, (size_t)n * p * sizeof(double), 0xFFFFFFFFu);
        for (OutI32 v : kNaInts) fill(o->*v, (size_t)n * sizeof(int32_t), 0xFFFFFFFFu);
        for (OutI32 v : kZeroInts) fill(o->*v, (size_t)n * sizeof(int32_t), 0u);
        fill(P.grid_flag, (size_t)n * sizeof(int32_t), 0u);
        std::sort(fills.begin(), fills.end(), [](const Fill &x, const Fill &y) { return x.p < y.p; });
        for (const Fill &fl : fills) f.add(fl.p, fl.bytes, fl.val);
    }
    if (a->phases & DSQ_PH_TREND) {
        f.add(o->scalars + DSQ_SC_FIT_USED, sizeof(double), 0u);     // 0.0 = DSQ_FIT_PARAMETRIC
        int rc;
        if (!a->dispFit_in && a->fitType != DSQ_FIT_MEAN) {
            if ((rc = capi_ws_get(DSQ_WS_PIPE_META, trend_fit_workspace_bytes() + 64, &P.trend_ws))) return rc;
            f.add(P.trend_ws, (trend_fit_workspace_bytes() + 3) / 4 * 4, 0u);
        }
        const size_t sel_bytes = prior_var_workspace_bytes(trend_count(P));     // (0: on one workgroup, without)
        if (sel_bytes) {
            if ((rc = capi_ws_get(DSQ_WS_PIPE_SEL, sel_bytes + 64, &P.sel_ws))) return rc;
            f.add(P.sel_ws, (sel_bytes + 3) / 4 * 4, 0u);
        }
    }
    if (f.full) return capi_fail(DSQ_ERR_DEVICE, "dsq_deseq_dev: more than %d init segments", kInitSegMax);
    size_t words = 0;
    for (int sgi = 0; sgi < ip.nseg; sgi++) words += ip.seg[sgi].words;
    unsigned blocks = (unsigned)((words + 256 * 8 - 1) / (256 * 8));
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(chain_init_kernel, dim3(blocks), dim3(256), 0, P.st, ip);
    DSQ_HIP(hipGetLastError());
    return DSQ_OK;
}

// the three designs at their kernels' widths (wide ones: zero-padded copies), the design cells, the reduced / prior fit's
// fitted means
static int prepare_designs(Pipe &P) {
    const DsqDeseqArgs *a = P.a;
    const int n = P.n, m = P.m, p = P.p, pk = P.pk;
    hipStream_t st = P.st;
    int rc;
    P.x_k = a->x;
    if (pk > p) {
        // the padded columns of the start values (the moments kernel writes the true p columns) and of the optim start
        // values are zero
        if ((rc = capi_pad_design(DSQ_WS_PIPE_PADX, a->x, m, p, pk, st, &P.x_k))) return rc;
        P.padmask = dsq_low_bits(pk) & ~dsq_low_bits(p);
        DSQ_HIP(hipMemsetAsync(P.beta_init + (size_t)n * p, 0, (size_t)n * (pk - p) * sizeof(double), st));
        DSQ_HIP(hipMemsetAsync(P.opt_start + (size_t)n * p, 0, (size_t)n * (pk - p) * sizeof(double), st));
    }
    P.red_x_k = a->x_red; P.red_pk = a->x_red ? kern_width(a->p_red) : 0; P.red_lam = a->x_red ? P.lam_prior : P.lam;
    if (P.red_pk > a->p_red) {
        // the reduced design at its own padded width; the padded columns of its start values are zero (the moments kernel
        // writes the true p_red columns; those of the optim start values are cleared in front of the reduced fit)
        if ((rc = capi_pad_design(DSQ_WS_PIPE_PADXR, a->x_red, m, a->p_red, P.red_pk, st, &P.red_x_k))) return rc;
        DSQ_HIP(hipMemsetAsync(P.red_binit + (size_t)n * a->p_red, 0, (size_t)n * (P.red_pk - a->p_red) * sizeof(double), st));
    }
    P.pri_x_k = a->x_prior; P.pri_pk = P.pkp;
    if (a->betaPrior && P.pkp > a->p_prior)      // (the slot: never beside a reduced model, the prior is Wald only)
        if ((rc = capi_pad_design(DSQ_WS_PIPE_PADXR, a->x_prior, m, a->p_prior, P.pkp, st, &P.pri_x_k))) return rc;
    if (a->cell_of && a->ncell > 0)
        P.ncell = capi_upload_cells(a->cell_of, m, DSQ_WS_PIPE_CELLS, st, &P.cell_perm, &P.cell_start);
    if (a->x_red || a->betaPrior) {
        if (a->x_red && a->cell_of_red && a->ncell_red > 0)
            P.red_ncell = capi_upload_cells(a->cell_of_red, m, DSQ_WS_PIPE_CELLS_RED, st, &P.red_cell_perm, &P.red_cell_start);
        void *b;        // the reduced / prior fit's fitted means: read once by its logLik
        if ((rc = capi_ws_get(DSQ_WS_PIPE_RED_MU, (size_t)n * P.ld * sizeof(double), &b))) return rc;
        P.red_mu = (double *)b;
    }
    return DSQ_OK;
}

// m + 8 doubles of scratch for the column sums behind xim (the one place that fetches the slot)
static int xim_scratch(const Pipe &P, double **out) {
    void *b;
    const int rc = capi_ws_get(DSQ_WS_PIPE_XIM_SCRATCH, ((size_t)P.m + 8) * sizeof(double), &b);
    *out = (double *)b;
    return rc;
}

// ---- the phases of DSQ_PH_*, in the chain's order ---------------------------------------------
// gene-wise estimates
static int phase_gene_est(Pipe &P, const Rows &nz) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    const Rows all = {nullptr, nullptr, P.n};
    int rc = launch_prefit_rows(P, all, a->y);                                   // getBaseMeansAndVariances + moments
    if (rc) return rc;
    // (the tile counts borrow the residual buffer of the prior variance, which the trend phase fills after its own compaction)
    CompactParams c;
    memset(&c, 0, sizeof c);
    c.mode = 0; c.n = P.n; c.allZero = o->allZero; c.force_zero = a->force_zero;
    c.tile_cnt = (int32_t *)P.resbuf; c.rows_out = P.rows_nz; c.count_out = P.counters + CNT_NZ;
    DSQ_HIP(launch_compact(c, P.st));
    if (!a->nf_is_vector) {
        // momentsDispEstimate's mean(1 / colMeans(normalizationFactors)) over the rows that are not all zero
        // (R/core.R:2440-2444 on objectNZ): columns summed down the listed genes in gene order
        double *b;
        if ((rc = xim_scratch(P, &b))) return rc;
        DSQ_HIP(launch_xim_rows(a->nf, P.rows_nz, P.counters + CNT_NZ, P.m, P.ld, b, P.xim_dev, P.st));
    }
    return gene_est(P, nz, a->y, o->mu_hat, CNT_GRID1, CNT_OPT1, o->optim_geneest);
}

// dispersion trend + prior variance
static int phase_trend(Pipe &P) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    hipStream_t st = P.st;
    const double *tm = a->trend_mean ? a->trend_mean : o->baseMean;
    const double *td = a->trend_mean ? a->trend_disp : o->dispGeneEst;
    const int nt = trend_count(P);
    if (!(a->phases & DSQ_PH_GENE_EST)) DSQ_HIP(hipMemsetAsync(P.counters + CNT_TREND, 0, sizeof(int32_t), st));      // (else: the status fill)
    CompactParams c;
    memset(&c, 0, sizeof c);
    c.mode = 1; c.n = nt; c.mean_in = tm; c.disp_in = td; c.thresh = 100.0 * a->minDisp;
    c.tile_cnt = (int32_t *)P.resbuf; c.mean_out = P.trend_mean_c; c.disp_out = P.trend_disp_c; c.count_out = P.counters + CNT_TREND;
    DSQ_HIP(launch_compact(c, st));
    capi_prof_begin("trend_fit", nt, st);
    hipError_t e = hipSuccess;
    if (a->dispFit_in) {
        e = launch_trend_given(o->scalars, o->status, st);
    } else {
        if (a->fitType != DSQ_FIT_MEAN)
            e = launch_trend_fit_dev_zeroed(P.trend_mean_c, P.trend_disp_c, P.counters + CNT_TREND, o->scalars + DSQ_SC_COEF0,
                                            o->status + DSQ_ST_TREND_STATUS, P.trend_ws, st);
        if (e == hipSuccess && a->fitType != DSQ_FIT_PARAMETRIC)            // R/core.R:894-899 over the same vector, uncompacted
            e = launch_trend_mean(td, nt, a->minDisp, (int)a->fitType, o->scalars, o->status, st);
    }
    capi_prof_end(st);
    DSQ_HIP(e);
    capi_prof_begin("prior_var", nt, st);
    const double *fin = a->dispFit_in ? (a->trend_mean ? a->trend_fit_in : a->dispFit_in) : (const double *)nullptr;
    e = launch_prior_var(tm, td, nt, a->minDisp, a->expVarLogDisp, (P.m > P.p) ? 1 : 0, P.resbuf, o->scalars, o->status, fin,
                         a->dispPriorVar_in, P.sel_ws, st);
    capi_prof_end(st);
    DSQ_HIP(e);
    return DSQ_OK;
}

// MAP dispersions + test.  *counters_zeroed: this phase's last kernel has zeroed the counters of the outlier phase (REP ..
// OPT3R) -- when that phase follows in this call and no beta-prior pass, which counts into OPT3, comes in between
static int phase_map_test(Pipe &P, const Rows &nz, bool *counters_zeroed) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    if (!(a->phases & DSQ_PH_GENE_EST)) {            // (else still zero from the status fill: nothing in between counts into them)
        DSQ_HIP(hipMemsetAsync(P.counters + CNT_GRID2, 0, sizeof(int32_t), P.st));
        DSQ_HIP(hipMemsetAsync(P.counters + CNT_OPT2, 0, sizeof(int32_t), P.st));
        DSQ_HIP(hipMemsetAsync(P.counters + CNT_OPT3, 0, sizeof(int32_t), P.st));
    }
    int rc = map_est(P, nz, a->y, o->mu_hat, CNT_GRID2);
    if (rc) return rc;
    if ((rc = test_fit(P, nz, a->y, o->mu, o->H, CNT_OPT2))) return rc;
    const bool z = *counters_zeroed = (a->phases & (DSQ_PH_OUTLIERS | DSQ_PH_OUTLIERS_DETECT)) && !((a->phases & DSQ_PH_PRIOR) && a->betaPrior);
    hipLaunchKernelGGL(na_assay_rows_kernel, ew_grid(P.n), dim3(256), 0, P.st, P.n, P.m, P.ld, (const int32_t *)o->allZero, o->mu, o->H,
                       z ? P.counters + CNT_REP : (int32_t *)nullptr, z ? (int)(CNT_N - CNT_REP) : 0);
    return DSQ_OK;
}

// betaPrior: the pass with lambda = 1 / betaPriorVar
static int phase_prior(Pipe &P, const Rows &nz) {
    DSQ_HIP(hipMemsetAsync(P.counters + CNT_OPT2, 0, sizeof(int32_t), P.st));
    return prior_fit(P, nz, P.a->y, CNT_OPT2);
}

// the parameter blocks of the two outlier kernels over the rows `rw`
static CooksKernelParams cooks_params(const Pipe &P, const OutlierMeta &M, const Rows &rw) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    CooksKernelParams ck;
    memset(&ck, 0, sizeof ck);
    ck.n = P.n; ck.m = P.m; ck.p = P.p; ck.ld = P.ld; ck.y = a->y; ck.nf = a->nf; ck.nf_is_vector = a->nf_is_vector;
    ck.mu = o->mu; ck.H = o->H; ck.perm = M.dperm; ck.cell_start = M.dstart; ck.in3 = M.din3; ck.ncell = a->ncell; ck.any3 = M.any3;
    int cap = 2; while (cap < (M.any3 ? M.maxcell : P.m)) cap <<= 1;
    ck.sortcap = cap;
    ck.cooks = o->cooks; ck.maxCooks = o->maxCooks; ck.robustDisp = P.robustDisp;
    ck.rows = rw.rows; ck.n_dev = rw.n_dev;
    return ck;
}
static ReplaceKernelParams replace_params(const Pipe &P, const OutlierMeta &M, const Rows &rw) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    ReplaceKernelParams rk;
    memset(&rk, 0, sizeof rk);
    rk.n = P.n; rk.m = P.m; rk.ld = P.ld; rk.y = a->y; rk.nf = a->nf; rk.nf_is_vector = a->nf_is_vector;
    rk.cooks = o->cooks; rk.cutoff = a->cooksCutoff; rk.trim = a->trim; rk.replaceable = M.drepl;
    int cap2 = 2; while (cap2 < P.m) cap2 <<= 1;
    rk.sortcap = cap2;
    rk.newCounts = o->replaceCounts; rk.replace = o->replace;
    rk.rows = rw.rows; rk.n_dev = rw.n_dev;
    return rk;
}
static int launch_cooks_rows(Pipe &P, const CooksKernelParams &ck, hipStream_t st) {
    bool ok = true;
    capi_prof_begin("cooks_distance", P.n, st);
    DSQ_HIP(launch_cooks(ck, st, &ok));
    capi_prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "m=%d samples: a gene row plus its sort buffer exceeds the 160 KiB LDS", P.m);
    return DSQ_OK;
}
static int launch_replace_rows(Pipe &P, const ReplaceKernelParams &rk, hipStream_t st) {
    bool ok = true;
    capi_prof_begin("replace_outliers", P.n, st);
    DSQ_HIP(launch_replace(rk, st, &ok));
    capi_prof_end(st);
    if (!ok) return capi_fail(DSQ_ERR_UNSUPPORTED, "m=%d samples: the sort buffer exceeds the 160 KiB LDS", P.m);
    return DSQ_OK;
}

// rows with a replacement among `from` (R/core.R:2488-2490) -> their moments on the new counts (:2491) -> the ones that are
// still non-zero are refitted (:2496-2500)
static int list_replaced(Pipe &P, const Rows &from) {
    const DsqDeseqOut *o = P.o;
    hipLaunchKernelGGL(list_kernel, ew_grid(P.n), dim3(256), 0, P.st, from, (const int32_t *)o->replace, 1, P.rows_rep, P.counters + CNT_REP);
    const Rows rep = {P.rows_rep, P.counters + CNT_REP, P.n};
    const int rc = launch_prefit_rows(P, rep, o->replaceCounts);
    if (rc) return rc;
    hipLaunchKernelGGL(list_kernel, ew_grid(P.n), dim3(256), 0, P.st, rep, (const int32_t *)o->allZero, 0, P.rows_refit, P.counters + CNT_REFIT);
    return DSQ_OK;
}

// count outliers, first half: Cook's distances, replaceOutliers, the lists of the replaced rows and of the ones to refit
static int phase_outlier_detect(Pipe &P, const Rows &nz, const OutlierMeta &M, bool counters_zeroed) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    const int n = P.n, m = P.m;
    hipStream_t st = P.st;
    if (!counters_zeroed) DSQ_HIP(hipMemsetAsync(P.counters + CNT_REP, 0, (CNT_N - CNT_REP) * sizeof(int32_t), st));      // REP .. OPT3R
    int rc = launch_cooks_rows(P, cooks_params(P, M, nz), st);
    if (rc) return rc;
    // (before the replacement: allZero still says which rows had no fit -- a row that only BECOMES all zero keeps its assays)
    hipLaunchKernelGGL(na_assay_rows_kernel, ew_grid(n), dim3(256), 0, st, n, m, P.ld, (const int32_t *)o->allZero, o->cooks,
                       (double *)nullptr);
    if (!a->do_replace) return DSQ_OK;
    if ((rc = launch_replace_rows(P, replace_params(P, M, nz), st))) return rc;
    return list_replaced(P, nz);
}

static int phase_outlier_refit(Pipe &P, const Rows &nz, const OutlierMeta &M);

// count outliers, both halves, CANDIDATES FIRST (the whole phase in one call, the test's fit has left the flags).  A row's
// refit needs that row's Cook's distances and replacement and nothing of any other row; the order above waits for the
// distances of every row only because nobody knows which handful will be replaced.  The fit's bound knows a superset
// (cooks_can_exceed, fit_beta.hip): a tenth of a per cent of the rows.  So, once the candidates are listed, two branches:
//   the chain's stream   distances and replacement on the candidates, the lists of the replaced rows, their refit -- a
//                        serial tail of some twenty-five launches of a dozen lone waves;
//   the side stream      the full-row nbinomLogLike, then the distances and the pass-through replacement of all the rows
//                        that are no candidates (`skip`), on half of every CU (launch_outlier: `beside`).
// They meet in front of the closing steps.  Every kernel writes a row's outputs at the row's own position and none couples
// two rows: no bit changes (tests/test_gpu_outlier_first.py).
// What the two streams touch meanwhile: the side stream reads y / mu / H and writes cooks / maxCooks / robustDisp /
// replaceCounts / replace of rows that are NOT candidates; the chain's stream reads and writes columns of candidates, and
// the replace flags, where the side stream only writes the zeros that are there already (the fills of the gene-wise phase:
// the new order is taken only when the call runs that phase too).  The candidate flags sit in rows_lpt (read last by the
// test's fit), the list in rows_grid until the refit's first grid search takes that back.
static int phase_outlier_first(Pipe &P, const Rows &nz, const OutlierMeta &M, bool counters_zeroed) {
    const DsqDeseqOut *o = P.o;
    const int n = P.n, m = P.m;
    hipStream_t st = P.st;
    if (!counters_zeroed) DSQ_HIP(hipMemsetAsync(P.counters + CNT_REP, 0, (CNT_N - CNT_REP) * sizeof(int32_t), st));      // REP .. OPT3R
    int32_t *skip = P.rows_lpt, *n_cand = next_work_counter(P);       // (a counter the init launch has zeroed)
    if (getenv("DSQ_VERBOSE")) fprintf(stderr, "[dsq] outlier phase: candidates first (n=%d)\n", n);
    hipLaunchKernelGGL(cand_list_kernel, ew_grid(n), dim3(256), 0, st, nz, (const int32_t *)P.grid_flag, (const int32_t *)o->optim_test,
                       skip, P.rows_grid, n_cand);
    // (allZero still says which rows had no fit: in front of the moments of the replaced rows, which update it)
    hipLaunchKernelGGL(na_assay_rows_kernel, ew_grid(n), dim3(256), 0, st, n, m, P.ld, (const int32_t *)o->allZero, o->cooks,
                       (double *)nullptr);
    // fork -- the flags are all the other rows' pass needs: full-row log likelihoods (an event behind them: the refit's test
    // fit writes its rows' after them), then Cook's distances and the pass-through replacement of the rows that are no candidates
    int rc;
    if ((rc = fork_side(P)) || (rc = launch_pending_ll(P, true))) return rc;
    DSQ_HIP(hipEventRecord(P.ev_fork, P.side));      // (the fork's wait on this event is enqueued: it keeps the earlier record)
    P.ll_event = true;
    CooksKernelParams ck = cooks_params(P, M, nz);
    ReplaceKernelParams rk = replace_params(P, M, nz);
    ck.skip = rk.skip = skip;
    ck.beside = rk.beside = 1;
    if ((rc = launch_cooks_rows(P, ck, P.side)) || (rc = launch_replace_rows(P, rk, P.side))) return rc;
    // the chain's stream: the candidates, the lists, the refit
    const Rows cand = {P.rows_grid, n_cand, n};
    ck = cooks_params(P, M, cand); rk = replace_params(P, M, cand);
    ck.rows_few = rk.rows_few = 1;
    if ((rc = launch_cooks_rows(P, ck, st)) || (rc = launch_replace_rows(P, rk, st)) || (rc = list_replaced(P, cand))) return rc;
    return phase_outlier_refit(P, nz, M);
}

// the refit of the replaced rows runs every step on its DEFAULTS: refitWithoutOutliers passes none of the caller's betaTol /
// maxit / useQR / minmu on to estimateDispersions / nbinomWaldTest / nbinomLRT (R/core.R:2509-2531)
static void refit_defaults(Pipe &P) {
    P.tag = ":refit";
    P.t_tol = 1e-8; P.t_maxit = 100; P.t_useQR = 1; P.t_minmu = 0.5; P.ge_floor = 0.5;
}

// count outliers, second half: the same chain on the replaced rows that are still non-zero; their mu-hat and fitted means go
// to the (now dead) mu_hat matrix, assays mu / H keep the original fit as in R (the refit runs on a subset object, :2500-2531)
static int phase_outlier_refit(Pipe &P, const Rows &nz, const OutlierMeta &M) {
    const DsqDeseqArgs *a = P.a;
    const DsqDeseqOut *o = P.o;
    const Rows rep = {P.rows_rep, P.counters + CNT_REP, P.n};
    const Rows rf = {P.rows_refit, P.counters + CNT_REFIT, P.n};
    int rc;
    if ((rc = launch_pending_ll(P, true))) return rc;      // the full-row log likelihoods, beside the refit
    refit_defaults(P);
    if (!a->nf_is_vector) {
        // momentsDispEstimate of the refitted subset averages the normalization factors over ITS rows
        // (R/core.R:2440-2444 on objectSub, :2500-2509): the second scalar behind the lambda block
        double *b;
        if ((rc = xim_scratch(P, &b))) return rc;
        DSQ_HIP(launch_xim_flagged(a->nf, P.n, P.m, P.ld, o->replace, o->allZero, b, P.xim_dev + 1, P.st));
        P.xim_cur = P.xim_dev + 1;
    }
    if ((rc = gene_est(P, rf, o->replaceCounts, o->mu_hat, CNT_GRID1R, CNT_OPT1R, o->optim_geneest))) return rc;
    if ((rc = map_est(P, rf, o->replaceCounts, o->mu_hat, CNT_GRID2R))) return rc;
    // the full-row log likelihoods are down before the refit writes its rows' (candidates first: the side stream goes on)
    if (P.ll_event) {
        P.ll_event = false;
        DSQ_HIP(hipStreamWaitEvent(P.st, P.ev_fork, 0));
    } else if ((rc = join_side(P))) return rc;
    if ((rc = test_fit(P, rf, o->replaceCounts, o->mu_hat, nullptr, CNT_OPT2R))) return rc;
    if (a->betaPrior && (rc = prior_fit(P, rf, o->replaceCounts, CNT_OPT2R))) return rc;
    if ((rc = join_side(P))) return rc;          // (candidates first: every row's Cook's distances in front of the closing steps)
    return a->defer_finish ? DSQ_OK : outlier_finish(P, nz, rep, M, P.counters + CNT_REFIT);
}

static int run_chain(const DsqDeseqArgs *a, const DsqDeseqOut *o, hipStream_t st, Pipe &P) {
    int rc = check_args(a, o);
    if (rc || (rc = capi_check_device()) || (rc = bind(P, a, o, st)) || (rc = launch_init_fills(P)) || (rc = prepare_designs(P))) return rc;
    const Rows nz = {P.rows_nz, P.counters + CNT_NZ, P.n};
    const int ph = a->phases;
    if ((ph & DSQ_PH_GENE_EST) && (rc = phase_gene_est(P, nz))) return rc;
    if ((ph & DSQ_PH_TREND) && (rc = phase_trend(P))) return rc;
    bool counters_zeroed = false;          // handed from the MAP / test phase to the outlier phase
    if ((ph & DSQ_PH_MAP_TEST) && (rc = phase_map_test(P, nz, &counters_zeroed))) return rc;
    if ((ph & DSQ_PH_PRIOR) && a->betaPrior && (rc = phase_prior(P, nz))) return rc;
    // (one call: DSQ_PH_OUTLIERS; a caller with its own dispersion trend splits it -- DSQ_PH_OUTLIERS_DETECT up to the moments
    //  of the replaced rows, then, with dispFit_in updated at those rows' new means, DSQ_PH_OUTLIERS_REFIT)
    const bool detect = (ph & (DSQ_PH_OUTLIERS | DSQ_PH_OUTLIERS_DETECT)) != 0, refit = (ph & (DSQ_PH_OUTLIERS | DSQ_PH_OUTLIERS_REFIT)) != 0;
    OutlierMeta M;
    if ((detect || refit || ((ph & DSQ_PH_FINISH) && a->do_replace)) && (rc = outlier_meta(a, P.m, st, &M))) return rc;
    if ((ph & DSQ_PH_OUTLIERS) && P.cand_ready) {
        if ((rc = phase_outlier_first(P, nz, M, counters_zeroed))) return rc;
    } else {
        if (detect && (rc = phase_outlier_detect(P, nz, M, counters_zeroed))) return rc;
        if (refit && a->do_replace && (rc = phase_outlier_refit(P, nz, M))) return rc;
    }
    // (sharding callers) the closing steps, with the number of refitted rows over all shards
    if ((ph & DSQ_PH_FINISH) && a->do_replace)
        return outlier_finish(P, nz, Rows{P.rows_rep, P.counters + CNT_REP, P.n}, M, a->n_refit_global ? a->n_refit_global : P.counters + CNT_REFIT);
    return DSQ_OK;
}

static int run(const DsqDeseqArgs *a, const DsqDeseqOut *o, hipStream_t st) {
    Pipe P;
    memset(&P, 0, sizeof P);
    const int rc = run_chain(a, o, st, P);
    const int rl = rc ? DSQ_OK : launch_pending_ll(P, false);      // (no refit in this analysis: behind everything else)
    const int rj = join_side(P);             // (whatever path the chain left by: nothing stays in flight beside `st`)
    return rc ? rc : (rl ? rl : rj);
}

// (deseq_host.hip: the host-pointer entry drives the same chain from its per-device worker threads, under the call lock)
int pipeline_run(const DsqDeseqArgs *a, const DsqDeseqOut *o, hipStream_t st) { return run(a, o, st); }

}  // namespace dsq

extern "C" int64_t dsq_deseq_workspace_bytes(int32_t n, int32_t m, int32_t p, int32_t n_trend) {
    (void)m;
    if (n < 1 || p < 1) return 0;
    dsq::Pipe P;
    return (int64_t)dsq::workspace_table(P, n, dsq::kern_width(p), n_trend > n ? n_trend : n, nullptr);
}

extern "C" int dsq_deseq_dev(const DsqDeseqArgs *args, const DsqDeseqOut *out, void *stream) {
    std::lock_guard<std::mutex> lk(dsq::g_mu);
    dsq::capi_latch_stream((hipStream_t)stream);
    return dsq::run(args, out, (hipStream_t)stream);
}
