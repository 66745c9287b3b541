// count_helpers.hip -- the helpers of R/helper.R at the two ends of the workflow, on the resident count matrix (DESIGN.md
// section 20): the grouped column sums of collapseReplicates (R/helper.R:187-216), colSums, and fpm / fpkm
// (R/helper.R:291-391).  Gene-major only: element (i, j) at [i * ld + j], the padding neither read nor written.  Integer
// sums are exact (int64), so their order is free; the quotients are IEEE operations in R's order, one rounding each
// (-ffp-contract=off; no reciprocal, no folded constant).  tests/counts_spec.py states all of it.
//   collapse_kernel: the n x g outputs as a flat list, one thread per output (gene i, group c), consecutive lanes on
//     consecutive groups of a gene and then on the next gene -- at g = 6 a wavefront holds ten genes.  A thread adds its
//     group's counts of its gene in int64 (the gene's row is in cache after the first group touched it) and writes the low
//     32 bits; a sum that is no int32 ORs 1 into the status word.  members / offsets are device memory that the launch
//     cannot look at: a range outside [0, m] is clipped, a member outside [0, m) is not read, and either ORs 2 into status.
//   col_sums_kernel: a workgroup owns a tile of W = min(m, 64) samples and a slice of genes; thread t adds sample t % W
//     of the genes t / W, t / W + R, ... of the slice (R = 256 / W genes per step, so a 12-sample matrix keeps 252 of 256
//     lanes busy on 21 consecutive rows), the R partials of a sample meet in LDS, one 64-bit integer atomic add per
//     (workgroup, sample).  The sums are zeroed on the stream in front of the kernel.
//   fpm_kernel<KIND, VEC>: vst_transform_kernel's walk (flat items, persistent grid; VEC = 2: the pair of samples
//     (2 jp, 2 jp + 1) of a gene by 8-byte count loads, 16-byte loads of lib / L and 16-byte stores where every row
//     starts on a 16-byte boundary; the odd last sample of a row goes alone).
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"

namespace dsq {

constexpr int kCountThreads = 256;

__global__ void __launch_bounds__(kCountThreads) collapse_kernel(CollapseKernelParams kp, unsigned long long total) {
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned int g = (unsigned int)kp.g;
    int flags = 0;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const unsigned long long i = t / g;
        const unsigned int c = (unsigned int)(t - i * g);
        int lo = kp.offsets[c], hi = kp.offsets[c + 1];
        if (lo < 0) { lo = 0; flags |= 2; }
        if (hi > kp.m) { hi = kp.m; flags |= 2; }
        const int32_t *row = kp.y + (long)i * kp.ld;
        long long s = 0;
        for (int k = lo; k < hi; k++) {
            const int j = kp.members[k];
            if ((unsigned int)j < (unsigned int)kp.m) s += (long long)row[j];
            else flags |= 2;
        }
        if (s != (long long)(int32_t)s) flags |= 1;
        kp.out[(long)i * kp.ldo + c] = (int32_t)s;
    }
    if (flags) atomicOr(kp.status, flags);
}

hipError_t launch_collapse(const CollapseKernelParams &kp, hipStream_t st) {
    const unsigned long long total = (unsigned long long)kp.n * (unsigned long long)kp.g;
    unsigned long long blocks = (total + kCountThreads - 1) / kCountThreads;
    const unsigned long long most = 8ull * device_cu_count();
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] collapse n=%d m=%d g=%d: items %llu, blocks %llu, threads %d\n", kp.n, kp.m, kp.g, total, blocks, kCountThreads);
    hipLaunchKernelGGL(collapse_kernel, dim3((unsigned)blocks), dim3(kCountThreads), 0, st, kp, total);
    return hipGetLastError();
}

__global__ void __launch_bounds__(kCountThreads) col_sums_kernel(ColSumsKernelParams kp, int W, int R, int nb, long L) {
    __shared__ long long part[kCountThreads];
    const int tile = blockIdx.x % nb;
    const long slice = blockIdx.x / nb;
    const int t = threadIdx.x;
    const int r = t / W, c = t - r * W;
    const int j = tile * 64 + c;
    const long i0 = slice * L;
    const long i1 = i0 + L < kp.n ? i0 + L : kp.n;
    long long s = 0;
    if (r < R && j < kp.m)
        for (long i = i0 + r; i < i1; i += R) s += (long long)kp.y[i * kp.ld + j];
    part[t] = s;
    __syncthreads();
    if (t < W && j < kp.m) {
        for (int q = 1; q < R; q++) s += part[t + q * W];
        atomicAdd((unsigned long long *)kp.sums + j, (unsigned long long)s);
    }
}

hipError_t launch_col_sums(const ColSumsKernelParams &kp, hipStream_t st) {
    const int W = kp.m < 64 ? kp.m : 64;
    const int R = kCountThreads / W;
    const int nb = (kp.m + 63) / 64;
    // slices of genes: a device round of workgroups over the tiles, no slice shorter than 16 steps of a workgroup
    long S = (8L * device_cu_count()) / nb;
    if (S < 1) S = 1;
    long L = ((long)kp.n + S - 1) / S;
    if (L < 16L * R) L = 16L * R;
    S = ((long)kp.n + L - 1) / L;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] col_sums n=%d m=%d: tiles %d of %d samples, %d genes per step, slices %ld of %ld genes, threads %d\n",
                kp.n, kp.m, nb, W, R, S, L, kCountThreads);
    hipError_t e = hipMemsetAsync(kp.sums, 0, (size_t)kp.m * sizeof(long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(col_sums_kernel, dim3((unsigned)(S * nb)), dim3(kCountThreads), 0, st, kp, W, R, nb, L);
    return hipGetLastError();
}

template <int KIND>
DSQ_DEV double fpm_apply(double k, double lib, double len) {
    const double f = 1e6 * (k / lib);                                            // R/helper.R:390
    if constexpr (KIND == FPM_FPM) return f;
    else if constexpr (KIND == FPM_FPKM_BASEPAIRS) return 1e3 * (f / len);       // R/helper.R:322
    else return (1e3 * f) / len;                                                 // R/helper.R:294
}

template <int KIND, int VEC>
__global__ void __launch_bounds__(kCountThreads) fpm_kernel(FpmKernelParams kp, unsigned long long total, unsigned int inner) {
    const bool small = total <= 0xffffffffull;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        unsigned long long hi, lo;
        if (small) { const unsigned int h = (unsigned int)t / inner; hi = h; lo = (unsigned int)t - h * inner; }
        else { hi = t / inner; lo = t - hi * inner; }
        const long j = VEC * (long)lo;
        const long at = (long)hi * kp.ld + j;
        double len = 1.0;
        if constexpr (KIND == FPM_FPKM_BASEPAIRS) len = kp.basepairs[hi];
        if (VEC == 2 && j + 1 < kp.m) {
            const int2 kk = *(const int2 *)(kp.y + at);
            const double2 lib = *(const double2 *)(kp.lib + j);
            double2 len2 = make_double2(len, len);
            if constexpr (KIND == FPM_FPKM_TXLEN) len2 = *(const double2 *)(kp.txlen + at);
            double2 r;
            r.x = fpm_apply<KIND>((double)kk.x, lib.x, len2.x);
            r.y = fpm_apply<KIND>((double)kk.y, lib.y, len2.y);
            *(double2 *)(kp.out + at) = r;
        } else {
            if constexpr (KIND == FPM_FPKM_TXLEN) len = kp.txlen[at];
            kp.out[at] = fpm_apply<KIND>((double)kp.y[at], kp.lib[j], len);
        }
    }
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int KIND>
static hipError_t launch_fpm_kind(const FpmKernelParams &kp, hipStream_t st) {
    // pairs of samples per lane where every row starts on a 16-byte boundary in the output (and L) and on an 8-byte one in the counts
    const bool vec = kp.m >= 2 && (kp.ld & 1) == 0 && aligned(kp.y, 8) && aligned(kp.out, 16) && aligned(kp.lib, 16) &&
                     (KIND != FPM_FPKM_TXLEN || aligned(kp.txlen, 16));
    const unsigned int inner = vec ? (unsigned int)((kp.m + 1) / 2) : (unsigned int)kp.m;
    const unsigned long long total = (unsigned long long)inner * (unsigned long long)kp.n;
    unsigned long long blocks = (total + kCountThreads - 1) / kCountThreads;
    const unsigned long long most = 8ull * device_cu_count();
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] fpm kind=%d n=%d m=%d: mode %s, items %llu, blocks %llu, threads %d\n", KIND, kp.n, kp.m,
                vec ? "paired" : "single", total, blocks, kCountThreads);
    if (vec) hipLaunchKernelGGL((fpm_kernel<KIND, 2>), dim3((unsigned)blocks), dim3(kCountThreads), 0, st, kp, total, inner);
    else hipLaunchKernelGGL((fpm_kernel<KIND, 1>), dim3((unsigned)blocks), dim3(kCountThreads), 0, st, kp, total, inner);
    return hipGetLastError();
}

hipError_t launch_fpm(const FpmKernelParams &kp, hipStream_t st) {
    switch (kp.kind) {
    case FPM_FPM:            return launch_fpm_kind<FPM_FPM>(kp, st);
    case FPM_FPKM_BASEPAIRS: return launch_fpm_kind<FPM_FPKM_BASEPAIRS>(kp, st);
    case FPM_FPKM_TXLEN:     return launch_fpm_kind<FPM_FPKM_TXLEN>(kp, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace dsq
