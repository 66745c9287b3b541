// local_fit.hip -- the local-regression dispersion trend, estimateDispersionsFit(fitType = "local") (R/core.R:889-893,
// 2194-2203): the estimator behind locfit(logDisps ~ logMeans, weights = means) with locfit's
// defaults (nearest-neighbour fraction 0.7, local quadratic, tricube kernel, prior weights times kernel weights),
// evaluated directly at every requested mean.  tests/local_fit_spec.py states the arithmetic; this file equals it bit for
// bit.  f64 throughout, no atomics, no MFMA.
//   the fit   keys = order_key(log(mean)) of the rows of the fit set (10 minDisp <= disp < Inf, 0 < mean < Inf), the largest
//     key for every other row, the row index as the payload, through the stable radix sort of results.hip
//     (radix_sort_columns): the fit set comes first, by ascending x, ties by ascending row.  One gather writes the block
//     header | x | y | w in that order: the fit handle.  N, k = floor(7 N / 10) and the all-below-floor flag live in the
//     header, on the device: building and evaluating need no host look in between.
//   local_fit_eval_kernel   one wave per evaluation point, persistent over the points.  The window start by bisection on
//     x[l + k] - z < z - x[l] (wave-uniform: scalar loads), h = max(z - x[l], x[l + k - 1] - z).  The window is swept in
//     chunks of kLocalFitLanes consecutive points ALIGNED to the sorted index (coalesced 512-byte reads of x, y, w): lane
//     (j mod 64) owns point j, so each lane adds its points in ascending j from +0.0 and the order of the eight sums is a
//     function of (l, k) alone -- not of the grid, the block or the evaluation list.  The lanes' partials meet in the
//     butterfly of dsq_wave.hpp (wave_allreduce_many: the bits of wave_allreduce).  Then the 3 x 3 elimination in the
//     specification's order and the exponential.
//     Points with |t| >= 1 (the window edge; every point when h = 0, where t is NaN or infinite) add nothing.  Distinct x of
//     positive weight are counted with a ballot per chunk (a point counts when its left neighbour IN the window differs).
//     Nothing outside [l, l + k) is read, and l + k <= N <= n: no index leaves the block.
//   local_fit_status_kernel   one workgroup: N, k, the singular points (a NaN value at a mean that has a logarithm), the
//     all-below-floor flag.
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr unsigned long long kNotInFit = ~0ull;      // above order_key of every finite x

struct LocalFitHeader {          // the first kLocalFitHeaderDoubles doubles of the block
    int32_t N, k, below, cap;    // fit points, window points, all rows below the floor, the n the block was sized for
    double minDisp;
    double reserved;
};
static_assert(sizeof(LocalFitHeader) == kLocalFitHeaderDoubles * 8, "the header is part of the block's size");

__global__ void __launch_bounds__(256) local_fit_keys_kernel(const double *means, const double *disps, int n, double floor10,
                                                             unsigned long long *key, unsigned int *row) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const double mu = live ? means[i] : 1.0, d = live ? disps[i] : 0.0;
    const bool in = live && d >= floor10 && d < kInf && mu > 0.0 && mu < kInf;
    const double x = dlog(in ? mu : 1.0);             // (every lane: dlog votes across the wave)
    if (live) {
        key[i] = in ? order_key(x) : kNotInFit;
        row[i] = (unsigned int)i;
    }
}

__global__ void __launch_bounds__(256) local_fit_gather_kernel(const unsigned long long *key, const unsigned int *row,
                                                               const double *means, const double *disps, int n, double minDisp,
                                                               double *block) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = j < n && key[j] != kNotInFit;
    const unsigned int r = in ? row[j] : 0u;
    const double mu = in ? means[r] : 1.0, d = in ? disps[r] : 1.0;
    const double x = dlog(mu), y = dlog(d);
    double *xs = block + kLocalFitHeaderDoubles;
    if (in) {
        xs[j] = x;
        xs[(long)n + j] = y;
        xs[2 * (long)n + j] = mu;
    }
    // the one thread that sees the end of the fit set writes the header
    const bool last = in && (j == n - 1 || key[j + 1] == kNotInFit);
    if (last || (j == 0 && !in)) {
        LocalFitHeader h;
        h.N = last ? (int32_t)(j + 1) : 0;
        h.k = (int32_t)((7 * (long)h.N) / 10);
        h.below = h.N == 0;
        h.cap = n;
        h.minDisp = minDisp;
        h.reserved = 0.0;
        *(LocalFitHeader *)block = h;
    }
}

DSQ_DEV double uniform_double(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(256) local_fit_eval_kernel(const double *block, const double *q, long n_eval, double *out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const LocalFitHeader *hd = (const LocalFitHeader *)block;
    const int N = hd->N, k = hd->k, below = hd->below;
    const long cap = hd->cap;
    const double minDisp = hd->minDisp;
    const double *x = block + kLocalFitHeaderDoubles, *y = x + cap, *w = y + cap;
    const long nwave = (long)gridDim.x * 4;
    for (long i = (long)blockIdx.x * 4 + wave; i < n_eval; i += nwave) {
        const double qi = uniform_double(q[i]);
        double res;
        if (below) res = minDisp;
        else if (k < 3 || !(qi > 0.0 && qi < kInf)) res = dnan();
        else {
            const double z = dlog(qi);
            int lo = 0, hi = N - k;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (x[mid + k] - z < z - x[mid]) lo = mid + 1;
                else hi = mid;
            }
            const int l = lo, e = lo + k;
            const double hl = z - x[l], hr = x[e - 1] - z;
            const double h = hl > hr ? hl : hr;           // (both finite: no NaN to order)
            double acc[8];
            _Pragma("unroll")
            for (int r = 0; r < 8; r++) acc[r] = 0.0;
            int distinct = 0;
            for (int c = (l / kLocalFitLanes) * kLocalFitLanes; c < e; c += kLocalFitLanes) {
                const int j = c + lane;
                bool first = false;
                if (j >= l && j < e) {
                    const double xj = x[j];
                    const double t = (xj - z) / h;
                    const double a = __builtin_fabs(t);
                    if (a < 1.0) {
                        const double u = 1.0 - (a * a) * a;
                        const double yj = y[j];
                        const double c0 = w[j] * ((u * u) * u);
                        const double c1 = c0 * t;
                        const double c2 = c1 * t;
                        const double c3 = c2 * t;
                        const double c4 = c3 * t;
                        acc[0] = acc[0] + c0;
                        acc[1] = acc[1] + c1;
                        acc[2] = acc[2] + c2;
                        acc[3] = acc[3] + c3;
                        acc[4] = acc[4] + c4;
                        acc[5] = acc[5] + c0 * yj;
                        acc[6] = acc[6] + c1 * yj;
                        acc[7] = acc[7] + c2 * yj;
                        first = c0 > 0.0 && (j == l || xj != x[j - 1]);
                    }
                }
                distinct += __popcll(__ballot(first));
            }
            wave_allreduce_many<8>(acc, lane);
            const double S0 = acc[0], S1 = acc[1], S2 = acc[2], S3 = acc[3], S4 = acc[4], T0 = acc[5], T1 = acc[6], T2 = acc[7];
            const double m1 = S1 / S0;
            const double m2 = S2 / S0;
            const double A11 = S2 - m1 * S1;
            const double A12 = S3 - m1 * S2;
            const double A22 = S4 - m2 * S2;
            const double b1 = T1 - m1 * T0;
            const double b2 = T2 - m2 * T0;
            const double m3 = A12 / A11;
            const double p2 = A22 - m3 * A12;
            const double c2 = b2 - m3 * b1;
            const double a2 = c2 / p2;
            const double a1 = (b1 - A12 * a2) / A11;
            const double a0 = ((T0 - S1 * a1) - S2 * a2) / S0;
            const bool ok = distinct >= 3 && S0 > 0.0 && A11 > 0.0 && p2 > 0.0;
            res = ok ? sf_exp(a0) : dnan();
        }
        if (lane == 0) out[i] = res;
    }
}

__global__ void __launch_bounds__(256) local_fit_status_kernel(const double *block, const double *q, const double *out, long n_eval,
                                                               int32_t *status) {
    __shared__ int part[256];
    const LocalFitHeader *hd = (const LocalFitHeader *)block;
    int cnt = 0;
    if (!hd->below && hd->k >= 3 && out)
        for (long i = threadIdx.x; i < n_eval; i += 256) {
            const double qi = q[i], v = out[i];
            cnt += (qi > 0.0 && qi < kInf && v != v) ? 1 : 0;
        }
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        status[0] = hd->N;
        status[1] = hd->k;
        status[2] = part[0];
        status[3] = hd->below;
    }
}

static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

size_t local_fit_workspace_bytes(long n) {
    // keys A, B (n u64 each) | rows A, B (n u32 each) | the (digit, tile) table | the sort's copy flag
    return 2 * (size_t)n * 8 + 2 * pad8((size_t)n * 4) + sort_hist_entries(n) * 4 + 8;
}

hipError_t launch_local_fit_build(const double *means, const double *disps, int n, double minDisp, double *block, void *workspace,
                                  hipStream_t st) {
    char *ws = (char *)workspace;
    unsigned long long *ka = (unsigned long long *)ws;   ws += (size_t)n * 8;
    unsigned long long *kb = (unsigned long long *)ws;   ws += (size_t)n * 8;
    unsigned int *ra = (unsigned int *)ws;                ws += pad8((size_t)n * 4);
    unsigned int *rb = (unsigned int *)ws;                ws += pad8((size_t)n * 4);
    unsigned int *hist = (unsigned int *)ws;              ws += sort_hist_entries(n) * 4;
    unsigned int *flag = (unsigned int *)ws;
    const dim3 grid((n + 255) / 256), blk(256);
    hipLaunchKernelGGL(local_fit_keys_kernel, grid, blk, 0, st, means, disps, n, 10 * minDisp, ka, ra);
    radix_sort_columns(ka, kb, ra, rb, hist, flag, n, 1, st);
    hipLaunchKernelGGL(local_fit_gather_kernel, grid, blk, 0, st, (const unsigned long long *)ka, (const unsigned int *)ra, means, disps,
                       n, minDisp, block);
    return hipGetLastError();
}

hipError_t launch_local_fit_eval(const double *block, const double *q, long n_eval, double *out, int32_t *status, hipStream_t st) {
    if (n_eval > 0 && out) {
        long blocks = (n_eval + 3) / 4;
        const long most = 8L * device_cu_count();
        if (blocks > most) blocks = most;
        if (getenv("DSQ_VERBOSE")) fprintf(stderr, "[dsq] local_fit eval: %ld points, blocks %ld, threads 256\n", n_eval, blocks);
        hipLaunchKernelGGL(local_fit_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, st, block, q, n_eval, out);
    }
    hipLaunchKernelGGL(local_fit_status_kernel, dim3(1), dim3(256), 0, st, block, q, (const double *)out, out ? n_eval : 0L, status);
    return hipGetLastError();
}

}  // namespace dsq
