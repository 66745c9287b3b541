// vst.hip -- the variance stabilizing transformation and its relatives on the device.
//
// getVarianceStabilizedData (R/vst.R:146-193), normTransform (R/helper.R:421-436), counts(normalized = TRUE): elementwise
// functions of q_ij = k_ij / nf_ij.  ONE pass: every count is read once, every output written once, nothing staged in
// between -- 4 bytes in, 8 bytes out per element (+ 8 with a normalization-factor matrix), against one logarithm, one
// square root and two divisions of f64 arithmetic.
//   vst_transform_kernel<KIND, T, VEC>: the formula is a template argument (one launch = one formula), the scalars of the
//     formula are kernel arguments (SGPRs).  The matrix is walked as a flat list of items, consecutive lanes on
//     consecutive memory in either layout; VEC = 2 (gene-major, even ld, aligned pointers): an item is the pair of samples
//     (2 jp, 2 jp + 1) of a gene -- 8-byte count loads, 16-byte size-factor loads and 16-byte stores; the odd last sample
//     of a row goes alone, so a padding column is neither read as a sample nor written.
//     The spline formula keeps the caller's table (x | y | b | c | d, 40 bytes per knot) in LDS: workgroups of 512
//     lanes, persistent, so that a table of R's 998 knots (39 KiB) leaves room for four workgroups = 32 waves on a CU.
//   vst_rowstats_kernel<T>: one wave per gene, the row mean (wave-order sum / m) and the row maximum of q in one sweep.
//     Gene-major is its layout: in R layout the lanes of a wave read with stride n (a cache line each) -- correct, served
//     for completeness of the _dev entry, not a path to time; the engine and the host entry always hand it gene-major.
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

enum { VST_PARAMETRIC = 0, VST_MEAN = 1, VST_SPLINE = 2, VST_LOG2 = 3, VST_NORMALIZED = 4 };
constexpr double kLn2 = 6.93147180559945286227e-01;      // the double nearest to ln 2: R's log(2)

// asinh for x >= 0 (or NaN) from dlog / dlog1p / sqrt, fdlibm's ranges: x below 2^-28; up to 2 through log1p, so that
// small arguments keep their digits; up to 2^28; beyond
DSQ_DEV double vst_asinh(double x) {
    if (x != x) return x;
    if (x < 3.725290298461914e-09) return x;
    if (x > 268435456.0) return dlog(x) + kLn2;
    const double t = x * x;
    const double r = __builtin_sqrt(t + 1.0);
    if (x > 2.0) return dlog(2.0 * x + 1.0 / (r + x));
    return dlog1p(x + t / (1.0 + r));
}

// the piecewise cubic: R's spline_eval (interval search as written there; no linear tail -- that is method "natural")
DSQ_DEV double vst_spline(const double *tab, int K, double u) {
    int i = 0, j = K;
    while (j > i + 1) {
        const int k = (i + j) >> 1;
        if (u < tab[k]) j = k; else i = k;
    }
    const double dx = u - tab[i];
    return tab[K + i] + dx * (tab[2 * K + i] + dx * (tab[3 * K + i] + dx * tab[4 * K + i]));
}

template <int KIND>
DSQ_DEV double vst_apply(const VstKernelParams &kp, double q, double ope, double a4, double la, double l4, const double *tab) {
    if constexpr (KIND == VST_PARAMETRIC) {
        // log((1 + e + 2 a q + 2 sqrt(a q (1 + e + a q))) / (4 a)) / log(2)                                   R/vst.R:154
        const double aq = kp.a * q;
        const double s1 = ope + (2.0 * kp.a) * q;
        const double v = aq * (ope + aq);
        return dlog((s1 + 2.0 * __builtin_sqrt(v)) / a4) / kLn2;
    } else if constexpr (KIND == VST_MEAN) {
        // (2 asinh(sqrt(alpha q)) - log(alpha) - log(4)) / log(2)                                             R/vst.R:188
        return ((2.0 * vst_asinh(__builtin_sqrt(kp.alpha * q)) - la) - l4) / kLn2;
    } else if constexpr (KIND == VST_SPLINE) {
        return kp.eta * vst_spline(tab, kp.nknots, vst_asinh(q)) + kp.xi;                                    // R/vst.R:180
    } else if constexpr (KIND == VST_LOG2) {
        return dlog(q + kp.pc) / kLn2;
    } else {
        return q;
    }
}

template <typename T> struct VstPair;
template <> struct VstPair<int32_t> { typedef int2 type; };
template <> struct VstPair<double> { typedef double2 type; };

template <int KIND, typename T, int VEC, int GM>
__global__ void __launch_bounds__(KIND == VST_SPLINE ? 512 : 256)
vst_transform_kernel(VstKernelParams kp, unsigned long long total, unsigned int inner) {
    extern __shared__ double vst_tab[];
    if constexpr (KIND == VST_SPLINE) {
        for (int b = threadIdx.x; b < 5 * kp.nknots; b += blockDim.x) vst_tab[b] = kp.table[b];
        __syncthreads();
    }
    // the per-launch scalars (wave-uniform)
    const double ope = 1.0 + kp.e, a4 = 4.0 * kp.a;
    double la = 0.0, l4 = 0.0;
    if constexpr (KIND == VST_MEAN) { la = dlog(kp.alpha); l4 = dlog(4.0); }
    const T *y = (const T *)kp.y;
    const bool small = total <= 0xffffffffull;
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        unsigned long long hi, lo;
        if (small) { const unsigned int h = (unsigned int)t / inner; hi = h; lo = (unsigned int)t - h * inner; }
        else { hi = t / inner; lo = t - hi * inner; }
        if constexpr (VEC == 2) {
            // gene hi, samples 2 lo and 2 lo + 1
            const long j = 2 * (long)lo;
            const long at = (long)hi * kp.si + j;
            if (j + 1 < kp.m) {
                const typename VstPair<T>::type kk = *(const typename VstPair<T>::type *)(y + at);
                const double2 f = *(const double2 *)(kp.nf + (kp.nf_is_vector ? j : at));
                double2 r;
                r.x = vst_apply<KIND>(kp, count_value<T>(kk.x, kp.bad) / f.x, ope, a4, la, l4, vst_tab);
                r.y = vst_apply<KIND>(kp, count_value<T>(kk.y, kp.bad) / f.y, ope, a4, la, l4, vst_tab);
                *(double2 *)(kp.out + at) = r;
            } else {
                const double f = kp.nf[kp.nf_is_vector ? j : at];
                kp.out[at] = vst_apply<KIND>(kp, count_value<T>(y[at], kp.bad) / f, ope, a4, la, l4, vst_tab);
            }
        } else {
            // gene-major: (gene hi, sample lo); R layout: (sample hi, gene lo) -- the fast index runs along memory
            const long i = GM ? (long)hi : (long)lo, j = GM ? (long)lo : (long)hi;
            const long at = i * kp.si + j * kp.sj;
            const double f = kp.nf[kp.nf_is_vector ? j : at];
            kp.out[at] = vst_apply<KIND>(kp, count_value<T>(y[at], kp.bad) / f, ope, a4, la, l4, vst_tab);
        }
    }
}

DSQ_DEV double vst_lane_xor(double v, int off) { return __shfl_xor(v, off, 64); }

template <typename T>
__global__ void __launch_bounds__(256) vst_rowstats_kernel(VstKernelParams kp) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwave = gridDim.x * 4;
    const T *y = (const T *)kp.y;
    for (int i = blockIdx.x * 4 + wave; i < kp.n; i += nwave) {
        double s = 0.0, mx = -kInf, anynan = 0.0;
        for (int j = lane; j < kp.m; j += 64) {
            const long at = (long)i * kp.si + (long)j * kp.sj;
            const double q = count_value<T>(y[at], kp.bad) / kp.nf[kp.nf_is_vector ? (long)j : at];
            s += q;
            if (q != q) anynan = 1.0;
            else if (q > mx) mx = q;
        }
        s = wave_allreduce(s);
        for (int off = 1; off < 64; off <<= 1) {
            const double o = vst_lane_xor(mx, off), on = vst_lane_xor(anynan, off);
            if (o > mx) mx = o;
            if (on > anynan) anynan = on;
        }
        if (lane == 0) {
            kp.rowMean[i] = s / (double)kp.m;
            kp.rowMax[i] = anynan > 0.0 ? dnan() : mx;
        }
    }
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <int KIND, typename T>
static hipError_t launch_vst_kind(const VstKernelParams &kp, hipStream_t st) {
    const bool gm = kp.sj == 1;
    // pairs of samples per lane where every row starts on a 16-byte boundary in all three matrices
    const bool vec = gm && kp.m >= 2 && (kp.si & 1) == 0 && aligned(kp.y, 2 * sizeof(T)) && aligned(kp.out, 16) && aligned(kp.nf, 16);
    const unsigned int inner = vec ? (unsigned int)((kp.m + 1) / 2) : (unsigned int)(gm ? kp.m : kp.n);
    const unsigned long long total = (unsigned long long)inner * (unsigned long long)(gm ? kp.n : kp.m);
    const int threads = KIND == VST_SPLINE ? 512 : 256;
    const size_t lds = KIND == VST_SPLINE ? (size_t)kp.nknots * 5 * sizeof(double) : 0;
    const int cu = device_cu_count();
    // persistent: a round of resident workgroups, grid-stride over the items (the spline table is read once per workgroup)
    unsigned long long blocks = (total + threads - 1) / threads;
    const unsigned long long most = (unsigned long long)cu * (KIND == VST_SPLINE ? 4 : 8);
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] vst kind=%d n=%d m=%d: mode %s, items %llu, blocks %llu, threads %d\n", KIND, kp.n, kp.m,
                vec ? "paired" : gm ? "gene-major" : "r-layout", total, blocks, threads);
    if (vec) hipLaunchKernelGGL((vst_transform_kernel<KIND, T, 2, 1>), dim3((unsigned)blocks), dim3(threads), lds, st, kp, total, inner);
    else if (gm) hipLaunchKernelGGL((vst_transform_kernel<KIND, T, 1, 1>), dim3((unsigned)blocks), dim3(threads), lds, st, kp, total, inner);
    else hipLaunchKernelGGL((vst_transform_kernel<KIND, T, 1, 0>), dim3((unsigned)blocks), dim3(threads), lds, st, kp, total, inner);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_vst_t(const VstKernelParams &kp, hipStream_t st) {
    switch (kp.kind) {
    case VST_PARAMETRIC: return launch_vst_kind<VST_PARAMETRIC, T>(kp, st);
    case VST_MEAN:       return launch_vst_kind<VST_MEAN, T>(kp, st);
    case VST_SPLINE:     return launch_vst_kind<VST_SPLINE, T>(kp, st);
    case VST_LOG2:       return launch_vst_kind<VST_LOG2, T>(kp, st);
    case VST_NORMALIZED: return launch_vst_kind<VST_NORMALIZED, T>(kp, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_vst_transform(const VstKernelParams &kp, int y_f64, hipStream_t st) {
    return y_f64 ? launch_vst_t<double>(kp, st) : launch_vst_t<int32_t>(kp, st);
}

hipError_t launch_vst_rowstats(const VstKernelParams &kp, int y_f64, hipStream_t st) {
    int blocks = (kp.n + 3) / 4;
    const int most = 8 * device_cu_count();
    if (blocks > most) blocks = most;
    if (getenv("DSQ_VERBOSE")) fprintf(stderr, "[dsq] vst_rowstats n=%d m=%d: blocks %d, threads 256\n", kp.n, kp.m, blocks);
    if (y_f64) hipLaunchKernelGGL(vst_rowstats_kernel<double>, dim3(blocks), dim3(256), 0, st, kp);
    else hipLaunchKernelGGL(vst_rowstats_kernel<int32_t>, dim3(blocks), dim3(256), 0, st, kp);
    return hipGetLastError();
}

}  // namespace dsq
