// explore.hip -- sample-level exploration of a resident transform: the row variances and the
// top-ntop order behind plotPCA (R/plots.R:245-254), and the all-pairs sums over genes behind prcomp's Gram matrix and
// dist(t(assay(vsd))).  Every sum has a stated order (tests/explore_spec.py equals it bit for bit); no float atomics, no
// MFMA (its internal accumulation order cannot be stated operation by operation).
//   row_vars_kernel<REG>: one wave per gene, persistent over the genes (vst_rowstats_kernel's launch shape).  The mean is
//     the wave-order sum / m, the variance the wave-order sum of (a - mean) (a - mean) / (m - 1).  REG: rows of up to
//     64 kRvReg samples are read ONCE and kept in registers between the two sums; longer rows are swept twice.
//   the order: keys = ~order_key(variance) (descending), NaN -> the largest key, with the row index as the payload,
//     through the stable radix sort of results.hip (radix_sort_columns): ties and NaNs stay in ascending row order.
//   pair_sums_kernel<KIND>: a workgroup of 256 threads owns one 64 x 64 tile of sample pairs (jb >= ib) and one slice of
//     the rows summed.  Rows go through LDS kPairChunk at a time: the 64 + 64 values of the two sample blocks of a row are
//     contiguous in the gene-major layout (512-byte segments), centred on the way in for the Gram.  Thread (ty, tx) keeps
//     the 4 x 4 accumulators of samples (ty + 16 u, tx + 16 w): the a-values of a half-wave are 2 addresses (broadcast),
//     its b-values 16 consecutive doubles -- no bank conflict under ds_read_b64's 32-lane groups.  Each accumulator adds
//     its slice's rows in row order from +0.0.  The slice partials go to a workspace; pair_finish_kernel adds them in slice
//     order, mirrors the triangle, clears the diagonal of the distances and takes the square root for `dist`.
//     The slice rule (pair_slices) depends on (rows summed, m) alone -- never on the device.
//     Samples past m are not read (their LDS slots hold 0.0 and their accumulators are never written out); rows past the
//     slice end are neither read nor added.  A row index outside [0, n) is not read: it contributes NaN.
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kRvReg = 8;                  // values a lane keeps: rows of up to 512 samples are read once
constexpr int kPairChunk = 16;             // rows staged in LDS per barrier pair
constexpr int kPairThreads = 256;
constexpr int kPairTileElems = kPairTile * kPairTile;

template <bool REG>
__global__ void __launch_bounds__(256) row_vars_kernel(RowVarsKernelParams kp) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwave = gridDim.x * 4;
    const double dm = (double)kp.m, dm1 = (double)(kp.m - 1);
    for (int i = blockIdx.x * 4 + wave; i < kp.n; i += nwave) {
        const double *row = kp.x + (long)i * kp.ld;
        double s = 0.0, ss = 0.0, mean;
        if constexpr (REG) {
            double v[kRvReg];
            _Pragma("unroll")
            for (int q = 0; q < kRvReg; q++) {
                const int j = lane + 64 * q;
                v[q] = j < kp.m ? row[j] : 0.0;
            }
            _Pragma("unroll")
            for (int q = 0; q < kRvReg; q++)
                if (lane + 64 * q < kp.m) s += v[q];
            mean = wave_allreduce(s) / dm;
            _Pragma("unroll")
            for (int q = 0; q < kRvReg; q++)
                if (lane + 64 * q < kp.m) { const double d = v[q] - mean; ss += d * d; }
        } else {
            for (int j = lane; j < kp.m; j += 64) s += row[j];
            mean = wave_allreduce(s) / dm;
            for (int j = lane; j < kp.m; j += 64) { const double d = row[j] - mean; ss += d * d; }
        }
        ss = wave_allreduce(ss);
        if (lane == 0) {
            kp.rowMean[i] = mean;
            kp.rowVar[i] = ss / dm1;
        }
    }
}

int row_vars_register_width() { return 64 * kRvReg; }

hipError_t launch_row_vars(const RowVarsKernelParams &kp, hipStream_t st) {
    int blocks = (kp.n + 3) / 4;
    const int most = 8 * device_cu_count();
    if (blocks > most) blocks = most;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] row_vars n=%d m=%d: blocks %d, threads 256, %s\n", kp.n, kp.m, blocks,
                (kp.m <= 64 * kRvReg) ? "one read" : "two sweeps");
    if ((kp.m <= 64 * kRvReg)) hipLaunchKernelGGL(row_vars_kernel<true>, dim3(blocks), dim3(256), 0, st, kp);
    else hipLaunchKernelGGL(row_vars_kernel<false>, dim3(blocks), dim3(256), 0, st, kp);
    return hipGetLastError();
}

// ---- the top-ntop order ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) top_var_keys_kernel(const double *v, int n, unsigned long long *key, unsigned int *row) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = v[i];
    key[i] = d != d ? ~0ull : ~order_key(d);
    row[i] = (unsigned int)i;
}

__global__ void __launch_bounds__(256) top_var_take_kernel(const unsigned int *row, int k, int32_t *select) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) select[i] = (int32_t)row[i];
}

static size_t pad8(size_t b) { return (b + 7) & ~(size_t)7; }

size_t top_var_workspace_bytes(long n) {
    // keys A, B (n u64 each) | rows A, B (n u32 each) | the (digit, tile) table | the sort's copy flag
    return 2 * (size_t)n * 8 + 2 * pad8((size_t)n * 4) + sort_hist_entries(n) * 4 + 8;
}

hipError_t launch_top_var_order(const double *rowVar, int n, int k, int32_t *select, void *workspace, hipStream_t st) {
    char *w = (char *)workspace;
    unsigned long long *ka = (unsigned long long *)w;   w += (size_t)n * 8;
    unsigned long long *kb = (unsigned long long *)w;   w += (size_t)n * 8;
    unsigned int *ra = (unsigned int *)w;                w += pad8((size_t)n * 4);
    unsigned int *rb = (unsigned int *)w;                w += pad8((size_t)n * 4);
    unsigned int *hist = (unsigned int *)w;              w += sort_hist_entries(n) * 4;
    unsigned int *flag = (unsigned int *)w;
    hipLaunchKernelGGL(top_var_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rowVar, n, ka, ra);
    radix_sort_columns(ka, kb, ra, rb, hist, flag, n, 1, st);
    hipLaunchKernelGGL(top_var_take_kernel, dim3((k + 255) / 256), dim3(256), 0, st, (const unsigned int *)ra, k, select);
    return hipGetLastError();
}

// ---- the all-pairs sums ----------------------------------------------------------------------------------------------------
void pair_slices(long R, int m, PairSlices *ps) {
    ps->nb = (m + kPairTile - 1) / kPairTile;
    ps->ntiles = (long)ps->nb * (ps->nb + 1) / 2;
    const long cap = ps->ntiles >= kPairWork ? 1 : kPairWork / ps->ntiles;
    long L = (R + cap - 1) / cap;
    if (L < kPairMinSlice) L = kPairMinSlice;
    ps->L = L;
    ps->S = R > 0 ? (R + L - 1) / L : 1;
}

size_t pair_workspace_bytes(long R, int m) {
    PairSlices ps;
    pair_slices(R, m, &ps);
    return (size_t)ps.S * (size_t)ps.ntiles * kPairTileElems * sizeof(double);
}

template <int KIND, int NR>
DSQ_DEV void pair_rows(const double (*sa)[kPairTile], const double (*sb)[kPairTile], int nr, int ty, int tx, double (&acc)[4][4]) {
    _Pragma("unroll 4")
    for (int r = 0; r < (NR ? NR : nr); r++) {
        double a[4], b[4];
        _Pragma("unroll")
        for (int u = 0; u < 4; u++) { a[u] = sa[r][ty + 16 * u]; b[u] = sb[r][tx + 16 * u]; }
        _Pragma("unroll")
        for (int u = 0; u < 4; u++) {
            _Pragma("unroll")
            for (int w = 0; w < 4; w++) {
                if constexpr (KIND == PAIR_GRAM) acc[u][w] += a[u] * b[w];
                else { const double d = a[u] - b[w]; acc[u][w] += d * d; }
            }
        }
    }
}

template <int KIND>
__global__ void __launch_bounds__(kPairThreads) pair_sums_kernel(PairKernelParams kp) {
    __shared__ double sa[kPairChunk][kPairTile], sb[kPairChunk][kPairTile];
    const long tile = (long)blockIdx.x % kp.ntiles, slice = (long)blockIdx.x / kp.ntiles;
    int ib = 0;
    long rem = tile;
    while (rem >= kp.nb - ib) { rem -= kp.nb - ib; ib++; }
    const int jb = ib + (int)rem;
    const long r0 = slice * kp.L;
    const long r1 = r0 + kp.L < kp.R ? r0 + kp.L : kp.R;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
    _Pragma("unroll")
    for (int u = 0; u < 4; u++) {
        _Pragma("unroll")
        for (int w = 0; w < 4; w++) acc[u][w] = 0.0;
    }
    // what this thread stages: column c of the 128 (sample block ib | sample block jb), rows threadIdx.x / 128 + 2 q
    const int c = threadIdx.x & 127;
    const int smp = c < kPairTile ? ib * kPairTile + c : jb * kPairTile + (c - kPairTile);
    const bool live = smp < kp.m;
    for (long c0 = r0; c0 < r1; c0 += kPairChunk) {
        const int nr = r1 - c0 < kPairChunk ? (int)(r1 - c0) : kPairChunk;
        _Pragma("unroll")
        for (int q = 0; q < kPairChunk / 2; q++) {
            const int r = (threadIdx.x >> 7) + 2 * q;
            if (r < nr) {
                double v = 0.0;
                if (live) {
                    const long pos = c0 + r;
                    const long g = kp.rows ? (long)kp.rows[pos] : pos;
                    if (g >= 0 && g < kp.n) {
                        v = kp.x[g * kp.ld + smp];
                        if constexpr (KIND == PAIR_GRAM) { if (kp.centre) v = v - kp.centre[pos]; }
                    } else {
                        v = dnan();
                    }
                }
                if (c < kPairTile) sa[r][c] = v; else sb[r][c - kPairTile] = v;
            }
        }
        __syncthreads();
        if (nr == kPairChunk) pair_rows<KIND, kPairChunk>(sa, sb, nr, ty, tx, acc);
        else pair_rows<KIND, 0>(sa, sb, nr, ty, tx, acc);
        __syncthreads();
    }
    double *p = kp.partial + (slice * kp.ntiles + tile) * kPairTileElems;
    _Pragma("unroll")
    for (int u = 0; u < 4; u++) {
        _Pragma("unroll")
        for (int w = 0; w < 4; w++) p[(ty + 16 * u) * kPairTile + tx + 16 * w] = acc[u][w];
    }
}

__global__ void __launch_bounds__(256) pair_finish_kernel(PairKernelParams kp) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long m = kp.m;
    if (e >= m * m) return;
    const long i = e / m, j = e - i * m;
    const long lo = i < j ? i : j, hi = i < j ? j : i;
    const long ib = lo / kPairTile, jb = hi / kPairTile;
    const long tile = ib * kp.nb - ib * (ib - 1) / 2 + (jb - ib);
    const double *p = kp.partial + tile * kPairTileElems + (lo - ib * kPairTile) * kPairTile + (hi - jb * kPairTile);
    const long stride = kp.ntiles * kPairTileElems;
    double s = p[0];
    for (long sl = 1; sl < kp.S; sl++) s = s + p[sl * stride];
    if (kp.kind != PAIR_GRAM && i == j) s = 0.0;
    if (kp.root) s = __builtin_sqrt(s);
    kp.out[e] = s;
}

hipError_t launch_pair_sums(const PairKernelParams &kp, hipStream_t st) {
    const long blocks = kp.S * kp.ntiles;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] pair_sums kind=%d rows=%ld m=%d: tiles %ld, slices %ld of %ld rows, blocks %ld, threads %d\n", kp.kind,
                kp.R, kp.m, kp.ntiles, kp.S, kp.L, blocks, kPairThreads);
    if (kp.kind == PAIR_GRAM) hipLaunchKernelGGL(pair_sums_kernel<PAIR_GRAM>, dim3((unsigned)blocks), dim3(kPairThreads), 0, st, kp);
    else hipLaunchKernelGGL(pair_sums_kernel<PAIR_DIST2>, dim3((unsigned)blocks), dim3(kPairThreads), 0, st, kp);
    const long total = (long)kp.m * kp.m;
    hipLaunchKernelGGL(pair_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, kp);
    return hipGetLastError();
}

}  // namespace dsq
