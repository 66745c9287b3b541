// trend.hip -- the device code of DSQ_PH_TREND, the one all-gene step of the DESeq() chain, and its launchers:
//   trend_fit_kernel    parametricDispersionFit (R/core.R:2166-2190), sixteen workgroups
//   trend_mean_kernel   fitType = "mean" (R/core.R:894-899): the trimmed mean, one workgroup
//   trend_given_kernel  the caller's trend: only the scalars that say so
//   prior_var_kernel    stats::mad of the log dispersion residuals + the prior variance (R/methods.R:172-181,
//                       R/core.R:1135-1208): one workgroup, or sixteen from 16 384 values (prior_var_blocks)
// Every rank of a gene-sharded run pays for this phase on the gathered vectors (DESeqParallel, R/parallel.R:27), so it
// must not grow with the node.  The order statistics are taken by radix selection (exact; dsq_select.hpp), the sums of the
// trend fit in a fixed order: the results do not depend on the number of workgroups.
#include "capi.hpp"
#include "dsq_math.hpp"
#include "dsq_select.hpp"
#include "dsq_wave.hpp"

namespace dsq {

// the workgroups of the sixteen-workgroup kernels (trend_fit_kernel, prior_var_kernel<16>); they meet at grid_barrier
// (dsq_select.hpp, which states what that relies on)
static constexpr int kTrendBlocks = 16;

// ---- parametricDispersionFit (R/core.R:2166-2190) -----------------------------------------
// The all-gene step between the two dispersion passes: a Gamma-GLM (identity link) IRLS for
// disp ~ a0 + a1/mean inside the reference's outlier-filter loop.  It touches only two n-vectors:
// kTrendBlocks workgroups of 16 wavefronts keep the whole nested loop on the device (no host round
// trip per iteration) and meet at a grid barrier per reduction.
// Sums in BLOCK ORDER (the oracle's bsum): partial q = i mod 16384 -> (block, wave, lane); wave
// butterfly; the 16 wave sums of a block added in order; the 16 block sums added in order.  Every
// block reads the same block sums in the same order, so all blocks take identical branches.
struct TrendWs {
    GridSync sync;
    unsigned long long sums[2][kTrendBlocks][8];   // bit patterns of doubles, double-buffered by parity
};

template <int K>
DSQ_DEV void grid_sum(double (&v)[K], double (*red)[8], TrendWs *ws, int &parity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_allreduce_many(v, lane);         // (the bits of K butterflies, dsq_wave.hpp)
    __syncthreads();                      // previous use of `red` is complete
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double tot = red[0][threadIdx.x];
        for (int g = 1; g < 16; g++) tot = tot + red[g][threadIdx.x];
        __hip_atomic_store(&ws->sums[parity][blockIdx.x][threadIdx.x], (unsigned long long)__double_as_longlong(tot),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    grid_barrier(&ws->sync, kTrendBlocks);
    // the block sums of every workgroup, added in workgroup order: thread k takes sum k -- its 16 loads in flight together
    // (round 4: every thread used to fetch all K x 16 values itself, two at a time: ~ 60 dependent L2 round trips per pass)
    // -- and hands the total to the block through LDS
    if (threadIdx.x < K) {
        double t[kTrendBlocks];
#pragma unroll
        for (int b = 0; b < kTrendBlocks; b++)
            t[b] = __longlong_as_double((long long)__hip_atomic_load(&ws->sums[parity][b][threadIdx.x], __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT));
        double tot = t[0];
#pragma unroll
        for (int b = 1; b < kTrendBlocks; b++) tot = tot + t[b];
        red[0][threadIdx.x] = tot;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = red[0][k];
    parity ^= 1;
}

__global__ void __launch_bounds__(1024) trend_fit_kernel(const double *means, const double *disps, long n,
                                                         const int32_t *n_dev, double *coefs_out, int32_t *status_out,
                                                         TrendWs *ws) {
    __shared__ double red[16][8];
    if (n_dev) n = (long)*n_dev;            // fused pipeline: the number of genes in the fit lives on the device
    const long first = (long)blockIdx.x * 1024 + threadIdx.x, stride = 1024L * kTrendBlocks;
    int parity = 0;
    double c0 = 0.1, c1 = 1.0;
    int iter = 0, status = 0;
    for (;;) {
        double b0 = c0, b1 = c1;
        bool converged = false, invalid = false;
        double devold = 0.0;
        // One sweep over the genes and ONE grid reduction per IRLS pass: the deviance sums at the current (b0, b1) and
        // the normal-equation sums the NEXT pass solves (they are taken at the same (b0, b1)) are accumulated together.
        // Per sum the same terms in the same order as two separate sweeps give, so the bits are the separate sweeps';
        // the normal-equation sums of a pass that turns out converged / invalid are simply not used.
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int pass = -1; pass < 25 && !invalid; pass++) {
            if (pass >= 0) {
                double det = a[0] * a[2] - a[1] * a[1];
                b0 = (a[2] * a[3] - a[1] * a[4]) / det;
                b1 = (a[0] * a[4] - a[1] * a[3]) / det;
            }
            double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // a[0..5) for the next pass | sum log r, sum (r - 1), # invalid means
#pragma unroll 1
            for (long i = first; i < n; i += stride) {
                double mean = means[i], y = disps[i];
                double res = y / (c0 + c1 / mean);
                if (!((res > 1e-4) && (res < 15.0))) continue;
                double x = 1.0 / mean;
                double mu = b0 + b1 * x;
                double wgt = 1.0 / (mu * mu);
                double wx = wgt * x;
                v[0] += wgt; v[1] += wx; v[2] += wx * x; v[3] += wgt * y; v[4] += wx * y;
                if (!(mu > 0.0)) { v[7] += 1.0; continue; }
                double r = y / mu;
                v[5] += dlog(r); v[6] += r - 1.0;
            }
            grid_sum<8>(v, red, ws, parity);
            for (int k = 0; k < 5; k++) a[k] = v[k];
            if (v[7] > 0.0) { invalid = true; break; }
            double dev = -2.0 * (v[5] - v[6]);
            if (pass >= 0 && __builtin_fabs(dev - devold) / (__builtin_fabs(dev) + 0.1) < 1e-8) { converged = true; break; }
            devold = dev;
        }
        if (invalid) { status = 1; break; }
        double o0 = c0, o1 = c1;
        c0 = b0; c1 = b1;
        if (!(c0 > 0.0 && c1 > 0.0)) { status = 1; break; }
        double l0 = dlog(c0 / o0), l1 = dlog(c1 / o1);
        if ((l0 * l0 + l1 * l1 < 1e-6) && converged) break;
        iter++;
        if (iter > 10) { status = 2; break; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { coefs_out[0] = c0; coefs_out[1] = c1; *status_out = status; }
}

size_t trend_fit_workspace_bytes() { return sizeof(TrendWs); }

hipError_t launch_trend_fit(const double *means, const double *disps, long n, double *coefs, int32_t *status,
                            void *workspace, hipStream_t st) {
    hipError_t e = hipMemsetAsync(workspace, 0, sizeof(TrendWs), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(trend_fit_kernel, dim3(kTrendBlocks), dim3(1024), 0, st, means, disps, n, (const int32_t *)nullptr,
                       coefs, status, (TrendWs *)workspace);
    return hipGetLastError();
}

hipError_t launch_trend_fit_dev(const double *means, const double *disps, const int32_t *n_dev, double *coefs,
                                int32_t *status, void *workspace, hipStream_t st) {
    hipError_t e = hipMemsetAsync(workspace, 0, sizeof(TrendWs), st);
    if (e != hipSuccess) return e;
    return launch_trend_fit_dev_zeroed(means, disps, n_dev, coefs, status, workspace, st);
}

// ... with the workspace already zeroed by the caller (the chain's one init launch, pipeline.hip)
hipError_t launch_trend_fit_dev_zeroed(const double *means, const double *disps, const int32_t *n_dev, double *coefs,
                                       int32_t *status, void *workspace, hipStream_t st) {
    hipLaunchKernelGGL(trend_fit_kernel, dim3(kTrendBlocks), dim3(1024), 0, st, means, disps, 0L, n_dev, coefs, status,
                       (TrendWs *)workspace);
    return hipGetLastError();
}

// ---- stats::mad of the log dispersion residuals + the prior variance (R/methods.R:172-181, R/core.R:1135-1208) ----
// One workgroup spends 0.24 ms on 50 000 genes -- its selection passes and the two logarithms per gene all on one CU;
// sixteen share them from 16 384 values (6 250 genes: 0.116 ms on one workgroup, 0.146 on sixteen; 50 000: 0.243 / 0.124).
// The size rule, in one place: it chooses the instantiation and whether the launch needs the (zeroed) workspace.
static int prior_var_blocks(int n) { return n < 16384 ? 1 : kTrendBlocks; }
size_t prior_var_workspace_bytes(int n) { return prior_var_blocks(n) > 1 ? sizeof(SelWs) : 0; }

template <int BLOCKS>
__global__ void __launch_bounds__(1024) prior_var_kernel(const double *mean, const double *disp, int n, double minDisp,
                                                         double expVarLogDisp, int m_gt_p, double *resbuf, double *scalars,
                                                         int32_t *status, const double *fit_in, double pv_in, SelWs *ws) {
    __shared__ __attribute__((aligned(16))) unsigned hist[2048];
    __shared__ unsigned long long bc[3];
    const double inf = __builtin_inf();
    const double c0 = scalars[DSQ_SC_COEF0], c1 = scalars[DSQ_SC_COEF1];
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)blockDim.x * BLOCKS;
    unsigned long long *kept = &bc[0];                          // the residuals kept, counted where all threads meet
    if constexpr (BLOCKS > 1) {
        kept = &ws->cnt[7];
    } else {
        if (threadIdx.x == 0) *kept = 0ull;
        __syncthreads();
    }
    unsigned long long c = 0;
    for (long i = first; i < n; i += stride) {
        const double d = disp[i];
        const bool above = d >= minDisp * 100.0;                 // aboveMinDisp, R/core.R:897 / :1137
        double r = inf;
        if (above) {
            const double fit = fit_in ? fit_in[i] : c0 + c1 / mean[i];       // (fit_in: the caller's trend, DSQ_FIT_GIVEN)
            r = dlog(d) - dlog(fit);
            c++;
        }
        resbuf[i] = r;                                           // (read back by this thread only)
    }
    if (c) atomicAdd(kept, c);
    if constexpr (BLOCKS > 1) grid_barrier(&ws->sync, BLOCKS);
    else __syncthreads();
    const long k = (long)__hip_atomic_load(kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (writer) status[DSQ_ST_N_ABOVE_MIN] = (int32_t)k;
    if (k == 0) {
        if (writer) { scalars[DSQ_SC_VAR_LOG_DISP] = dnan(); scalars[DSQ_SC_DISP_PRIOR_VAR] = dnan(); }
        return;
    }
    SelState sel = {hist, bc, ws, 0};
    const double med = median<BLOCKS>(n, k, [&](int i) { return resbuf[i]; }, sel, 0);
    const double med2 = median<BLOCKS>(n, k, [&](int i) {
        const double r = resbuf[i];
        return (r == inf) ? inf : __builtin_fabs(r - med);
    }, sel, 1);
    if (writer) {
        const double mad = 1.4826 * med2;
        const double v = mad * mad;
        scalars[DSQ_SC_VAR_LOG_DISP] = v;
        double pv = v;
        if (m_gt_p) {
            const double t = v - expVarLogDisp;
            pv = (0.25 > t) ? 0.25 : t;                           // max(varLogDispEsts - expVarLogDisp, 0.25), :1200
        }
        if (pv_in > 0.0) pv = pv_in;                              // estimateDispersionsMAP(dispPriorVar = x), :989-994
        scalars[DSQ_SC_DISP_PRIOR_VAR] = pv;
    }
}

hipError_t launch_prior_var(const double *mean, const double *disp, int n, double minDisp, double expVarLogDisp, int m_gt_p,
                            double *resbuf, double *scalars, int32_t *status, const double *fit_in, double pv_in,
                            void *workspace, hipStream_t st) {
    if (prior_var_blocks(n) == 1) {
        hipLaunchKernelGGL(prior_var_kernel<1>, dim3(1), dim3(1024), 0, st, mean, disp, n, minDisp, expVarLogDisp, m_gt_p, resbuf,
                           scalars, status, fit_in, pv_in, (SelWs *)nullptr);
    } else {
        if (!workspace) return hipErrorInvalidValue;
        hipLaunchKernelGGL(prior_var_kernel<kTrendBlocks>, dim3(kTrendBlocks), dim3(1024), 0, st, mean, disp, n, minDisp,
                           expVarLogDisp, m_gt_p, resbuf, scalars, status, fit_in, pv_in, (SelWs *)workspace);
    }
    return hipGetLastError();
}

// ---- fitType = "mean" (R/core.R:894-899): mean(dispGeneEst[dispGeneEst > 10 minDisp], trim = 0.001) ----------------
// R: the values between the floor(N trim)-th order statistics from either end, then a long-double mean with a
// correction pass -- to double precision the correctly rounded mean.  Here: the two order statistics by radix selection
// (exact), the sum of the kept values as a 192-bit integer in units of 2^-128 (exact for every value >= 2^-75, and
// independent of the order of the additions: a deterministic result without a specified order), the quotient by long
// division, rounded once to nearest-even.  The mirror (core.py, Python integers) and the oracle restate exactly this.
struct U192 { uint64_t w[3]; };
DSQ_DEV void u192_add(U192 &a, const U192 &b) {
    uint64_t c = 0;
    for (int k = 0; k < 3; k++) {
        const uint64_t s = a.w[k] + b.w[k];
        const uint64_t c1 = s < a.w[k];
        const uint64_t t = s + c;
        c = c1 | (uint64_t)(t < s);
        a.w[k] = t;
    }
}
DSQ_DEV U192 u192_fixed(double x) {           // floor(x 2^128), 0 < x < 2^62 finite
    const uint64_t u = d2bits(x);
    int E = (int)((u >> 52) & 0x7ff);
    uint64_t M = u & ((1ull << 52) - 1ull);
    if (E) M |= 1ull << 52; else E = 1;
    const int sh = E - 1075 + 128;
    U192 r = {{0, 0, 0}};
    if (sh >= 0) {
        const int w = sh >> 6, b = sh & 63;
        if (w < 3) { r.w[w] = M << b; if (b && w + 1 < 3) r.w[w + 1] = M >> (64 - b); }
    } else if (-sh < 64) r.w[0] = M >> (-sh);
    return r;
}
DSQ_DEV U192 u192_times(double x, unsigned long c) {      // c copies of x (ties at the two cut points)
    U192 r = {{0, 0, 0}}, v = u192_fixed(x);
    for (; c; c >>= 1) { if (c & 1ul) u192_add(r, v); U192 d = v; u192_add(v, d); }
    return r;
}
DSQ_DEV double u192_mean(const U192 &S, uint64_t cnt) {   // RN-even(S / cnt) 2^-128 (cnt < 2^32)
    uint32_t q[6];
    uint64_t rem = 0;
    for (int k = 5; k >= 0; k--) {
        const uint64_t limb = (S.w[k >> 1] >> ((k & 1) * 32)) & 0xffffffffull;
        const uint64_t cur = (rem << 32) | limb;
        q[k] = (uint32_t)(cur / cnt);
        rem = cur % cnt;
    }
    int h = -1;
    for (int k = 5; k >= 0 && h < 0; k--) if (q[k]) h = k * 32 + 31 - __builtin_clz(q[k]);
    if (h < 0) return 0.0;
    auto bit_range = [&](int lo, int len) {                // bits [lo, lo + len) of the quotient, len <= 53
        uint64_t v = 0;
        for (int b = len - 1; b >= 0; b--) { const int i = lo + b; v = (v << 1) | ((q[i >> 5] >> (i & 31)) & 1u); }
        return v;
    };
    if (h <= 52) return (double)bit_range(0, h + 1) * bits2d((uint64_t)(1023 - 128) << 52);       // (means below 2^-75: truncated)
    const int shift = h - 52;
    uint64_t mant = bit_range(shift, 53);
    const bool half = (q[(shift - 1) >> 5] >> ((shift - 1) & 31)) & 1u;
    bool below = rem != 0;
    for (int i = 0; i < shift - 1 && !below; i++) below = (q[i >> 5] >> (i & 31)) & 1u;
    if (half && (below || (mant & 1ull))) mant++;
    return (double)mant * bits2d((uint64_t)(1023 + shift - 128) << 52);
}

// mode DSQ_FIT_MEAN: always; DSQ_FIT_PARAMETRIC_OR_MEAN: only when the parametric trend did not fit.  The trend then is
// the constant: COEF0 = the mean, COEF1 = 0 (dispFit = COEF0 + COEF1 / baseMean is that constant, exactly).
__global__ void __launch_bounds__(1024) trend_mean_kernel(const double *disp, int n, double minDisp, int mode, double *scalars,
                                                          int32_t *status) {
    __shared__ __attribute__((aligned(16))) unsigned hist[2048];
    __shared__ unsigned long long bc[3];
    __shared__ unsigned long long cnts[5];
    __shared__ U192 part[1024];
    if (mode == DSQ_FIT_PARAMETRIC_OR_MEAN && status[DSQ_ST_TREND_STATUS] == 0) return;
    const double inf = __builtin_inf(), thr = 10.0 * minDisp;
    auto val = [&](int i) { const double d = disp[i]; return (d > thr) ? d : inf; };       // (NaN: not kept, as na.rm)
    if (threadIdx.x < 5) cnts[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) c += val(i) != inf;
    atomicAdd(&cnts[0], c);
    __syncthreads();
    const long N = (long)cnts[0];
    if (N == 0) {                                           // (cannot happen behind N_TREND > 0; kept a failure)
        if (threadIdx.x == 0) status[DSQ_ST_TREND_STATUS] = 3;
        return;
    }
    const long k = (long)__builtin_floor((double)N * 0.001);
    SelState sel = {hist, bc, nullptr, 0};
    const double a = radix_select<1>(n, k, val, sel, 0);
    const double b = radix_select<1>(n, N - 1 - k, val, sel, 0);
    U192 acc = {{0, 0, 0}};
    unsigned long long la = 0, ca = 0, lb = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = val(i);
        if (v == inf) continue;
        la += v < a; ca += v == a; lb += v < b;
        if (v > a && v < b) { const U192 f = u192_fixed(v); u192_add(acc, f); }
    }
    atomicAdd(&cnts[1], la); atomicAdd(&cnts[2], ca); atomicAdd(&cnts[3], lb);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) u192_add(part[threadIdx.x], part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double mean = a;
        if (a != b) {                                       // sorted positions k .. N-1-k: the copies of a and of b inside
            U192 S = part[0];
            const U192 ta = u192_times(a, (unsigned long)(cnts[1] + cnts[2] - (unsigned long long)k));
            const U192 tb = u192_times(b, (unsigned long)((unsigned long long)(N - k) - cnts[3]));
            u192_add(S, ta); u192_add(S, tb);
            mean = u192_mean(S, (uint64_t)(N - 2 * k));
        }
        scalars[DSQ_SC_COEF0] = mean;
        scalars[DSQ_SC_COEF1] = 0.0;
        status[DSQ_ST_TREND_STATUS] = 0;
        scalars[DSQ_SC_FIT_USED] = (double)DSQ_FIT_MEAN;
    }
}

__global__ void trend_given_kernel(double *scalars, int32_t *status) {
    scalars[DSQ_SC_COEF0] = dnan(); scalars[DSQ_SC_COEF1] = dnan();
    scalars[DSQ_SC_FIT_USED] = (double)DSQ_FIT_GIVEN;
    status[DSQ_ST_TREND_STATUS] = 0;
}

// the caller's trend (fitType "local" evaluated by R, dispersionFunction<-): nothing to fit; the coefficients are NA
hipError_t launch_trend_given(double *scalars, int32_t *status, hipStream_t st) {
    hipLaunchKernelGGL(trend_given_kernel, dim3(1), dim3(1), 0, st, scalars, status);
    return hipGetLastError();
}

hipError_t launch_trend_mean(const double *disp, int n, double minDisp, int mode, double *scalars, int32_t *status,
                             hipStream_t st) {
    hipLaunchKernelGGL(trend_mean_kernel, dim3(1), dim3(1024), 0, st, disp, n, minDisp, mode, scalars, status);
    return hipGetLastError();
}

}  // namespace dsq
