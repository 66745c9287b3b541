// unmix.hip -- unmix() on the device: per-sample mixture fits with the loss in a variance-stabilised space
// (R/helper.R:70-132).
//
// Sample i (column i of x, n genes) is explained by k "pure" columns: minimise over the box [lo, 100]^k
//     L(p) = sum_g | v(x_gi) - v(f_g) |^power,   f_g = sum_j pure_gj p_j,   power 1 or 2,
//     v(q) = (2 asinh(sqrt(alpha q)) - log alpha - log 4) / log 2  (lo = 1e-6)   or   v(q) = log(q + shift)  (lo = 0).
// R hands each sample to optim(method = "L-BFGS-B") with numerical gradients; here the same objective on the same box is
// minimised by a projected Levenberg-Marquardt iteration on the reweighted Gauss-Newton system, stated once in
// tests/unmix_spec.py and equalled bit for bit:
//     r_g = v(x_gi) - v(f_g)   J_gj = v'(f_g) pure_gj   w_g = 1 (power 2), 1 / max(|r_g|, 1e-8) (power 1)
//     A = J'WJ, b = J'Wr over the genes whose v'(f_g) is finite;   (A_FF + lambda diag(A_FF)) d_F = b_F
// Two kernels.  unmix_prep_kernel writes v(x) ONCE, sample-major (m x n), so that the fit reads its target contiguously.
// unmix_fit_kernel gives one workgroup of kUnmixThreads threads to a sample (grid-stride over the samples).  A pass over
// the genes at a point p yields L(p), A(p) and b(p) together -- an accepted trial costs no second pass --: thread t adds
// the genes t, t + T, ... in order from 0.0 into k(k+1)/2 + k + 1 register accumulators, the 64 lanes of a wave combine by
// the xor butterfly of dsq_wave.hpp, the T / 64 wave results add in wave order.  Up to 8 components the whole triangle
// lives in registers (45 accumulators at the padded width 8); at the padded width 16 it would be 153 doubles = 306 VGPRs
// beside the 16-wide row of pure and of J, past the 256 architectural registers of a lane, so the rows of the triangle
// are accumulated in two sweeps over the genes (rows 0-10, rows 11-15: 78 and 75 accumulators) -- every sum keeps its
// own order, so the bits do not depend on the split.  The k x k algebra (Cholesky in one fixed order, the active set on
// the box) is tiny beside the sweeps: every lane runs it redundantly on the reduced system, with its factor in a
// per-wave piece of LDS that a lane only reads back where it wrote itself.
#include "capi.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kUmWaves = kUnmixThreads / 64;
constexpr double kUmLn2 = 6.93147180559945286227e-01;       // the double nearest to ln 2: R's log(2)
constexpr double kUmLn4 = 1.38629436111989057245e+00;       // R's log(4)
constexpr double kUmHi = 100.0;
constexpr double kUmLambda0 = 1e-3, kUmLambdaMin = 1e-9;
constexpr double kUmRelTol = 1e-10;
constexpr double kUmAbsFloor = 1e-8;
constexpr int kUmMaxReject = 30;

struct UmForm { int alpha_form; double a, la; };

// v(q) and v'(q)
DSQ_DEV void um_v(const UmForm &f, double q, double &v, double &d) {
    if (f.alpha_form) {
        const double z = __builtin_sqrt(f.a * q);
        const double s = __builtin_sqrt(z * z + 1.0);
        v = ((2.0 * dlog(z + s) - f.la) - kUmLn4) / kUmLn2;
        d = f.a / ((z * s) * kUmLn2);
    } else {
        const double t = q + f.a;
        v = dlog(t);
        d = 1.0 / t;
    }
}

// ---- v(x), sample-major: 32 x 32 tiles through LDS, reads along the samples, writes along the genes
__global__ void __launch_bounds__(256) unmix_prep_kernel(UnmixKernelParams kp) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long tiles_s = ((long)kp.m + 31) / 32, tiles_g = ((long)kp.n + 31) / 32, total = tiles_s * tiles_g;
    UmForm f;
    f.alpha_form = kp.alpha_form; f.a = kp.a; f.la = kp.alpha_form ? dlog(kp.a) : 0.0;
    for (long ti = blockIdx.x; ti < total; ti += gridDim.x) {
        const long g0 = (ti / tiles_s) * 32, s0 = (ti % tiles_s) * 32;
        for (int r = ty; r < 32; r += 8) {
            const long g = g0 + r, s = s0 + tx;
            double v = 0.0, d;
            if (g < kp.n && s < kp.m) um_v(f, kp.x[g * kp.ld + s], v, d);
            tile[r][tx] = v;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const long s = s0 + r, g = g0 + tx;
            if (s < kp.m && g < kp.n) kp.vx[s * (long)kp.n + g] = tile[tx][r];
        }
        __syncthreads();
    }
}

// ---- one sweep over the genes at the point pt: rows [R0, R1) of the packed lower triangle of A (entry (i, j), j <= i, at
// i (i + 1) / 2 + j), b_i of those rows at NA + i, and with R0 == 0 the loss at NA + KP; each wave leaves its butterfly
// sums in part[wave][.]
template <int KP, int R0, int R1>
DSQ_DEV void um_sweep(const UnmixKernelParams &kp, const UmForm &f, const double *vx, const double (&pt)[KP],
                      double (*part)[KP * (KP + 1) / 2 + KP + 1], int lane, int wave) {
    constexpr int NA = KP * (KP + 1) / 2;
    constexpr int A0 = R0 * (R0 + 1) / 2, A1 = R1 * (R1 + 1) / 2;
    double accA[A1 - A0], accB[R1 - R0], accL = 0.0;
#pragma unroll
    for (int c = 0; c < A1 - A0; c++) accA[c] = 0.0;
#pragma unroll
    for (int c = 0; c < R1 - R0; c++) accB[c] = 0.0;
    const int k = kp.k;
    for (long g = threadIdx.x; g < kp.n; g += kUnmixThreads) {
        const double *row = kp.pure + g * k;
        double pr[KP];
        if (k == KP) {                              // the full width: unguarded loads, which the compiler merges into wide ones
#pragma unroll
            for (int j = 0; j < KP; j++) pr[j] = row[j];
        } else {
#pragma unroll
            for (int j = 0; j < KP; j++) pr[j] = j < k ? row[j] : 0.0;
        }
        double fg = pr[0] * pt[0];
#pragma unroll
        for (int j = 1; j < KP; j++) fg = fg + pr[j] * pt[j];
        double vf, d;
        um_v(f, fg, vf, d);
        const double r = vx[g] - vf;
        const double ar = __builtin_fabs(r);
        if (R0 == 0) accL = accL + (kp.power == 1 ? ar : r * r);
        if (dfinite(d)) {
            const double w = kp.power == 1 ? 1.0 / __builtin_fmax(ar, kUmAbsFloor) : 1.0;
            double J[R1];
#pragma unroll
            for (int j = 0; j < R1; j++) J[j] = d * pr[j];
#pragma unroll
            for (int i = R0; i < R1; i++) {
                const double wi = w * J[i];
                accB[i - R0] = accB[i - R0] + wi * r;
#pragma unroll
                for (int j = 0; j <= i; j++) accA[i * (i + 1) / 2 + j - A0] = accA[i * (i + 1) / 2 + j - A0] + wi * J[j];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < A1 - A0; c++) {
        const double v = wave_allreduce(accA[c]);
        if (lane == 0) part[wave][A0 + c] = v;
    }
#pragma unroll
    for (int c = 0; c < R1 - R0; c++) {
        const double v = wave_allreduce(accB[c]);
        if (lane == 0) part[wave][NA + R0 + c] = v;
    }
    if (R0 == 0) {
        const double v = wave_allreduce(accL);
        if (lane == 0) part[wave][NA + KP] = v;
    }
}

// L, A, b at the point ptw[0 .. KP) (a per-wave copy, the same in every wave) into sys[]; block-uniform
template <int KP>
DSQ_DEV void um_pass(const UnmixKernelParams &kp, const UmForm &f, const double *vx, const double *ptw,
                     double (*part)[KP * (KP + 1) / 2 + KP + 1], double *sys, int lane, int wave) {
    constexpr int NACC = KP * (KP + 1) / 2 + KP + 1;
    double pt[KP];
#pragma unroll
    for (int j = 0; j < KP; j++) pt[j] = ptw[j];
    if constexpr (KP <= 8) um_sweep<KP, 0, KP>(kp, f, vx, pt, part, lane, wave);
    else {
        um_sweep<KP, 0, 11>(kp, f, vx, pt, part, lane, wave);
        um_sweep<KP, 11, KP>(kp, f, vx, pt, part, lane, wave);
    }
    __syncthreads();
    for (int a = threadIdx.x; a < NACC; a += kUnmixThreads) {
        double s = part[0][a];
#pragma unroll
        for (int w = 1; w < kUmWaves; w++) s = s + part[w][a];
        sys[a] = s;
    }
    __syncthreads();
}

// (A_FF + lambda diag(A_FF)) d_F = b_F by Cholesky in one fixed order; the coordinates in `fixed` are identity rows with a
// zero right-hand side.  Lw, dw: the wave's own scratch.  false: a pivot that is not positive.
DSQ_DEV bool um_solve(const double *A, const double *b, int k, double lam, unsigned fixed, double *Lw, double *dw) {
    for (int i = 0; i < k; i++) {
        const bool fi = (fixed >> i) & 1u;
        for (int j = 0; j <= i; j++) {
            const bool fj = (fixed >> j) & 1u;
            double s;
            if (fi || fj) s = i == j ? 1.0 : 0.0;
            else {
                s = A[i * (i + 1) / 2 + j];
                if (i == j) s = s + lam * s;
            }
            for (int t = 0; t < j; t++) s = s - Lw[i * (i + 1) / 2 + t] * Lw[j * (j + 1) / 2 + t];
            if (i == j) {
                if (!(s > 0.0)) return false;
                Lw[i * (i + 1) / 2 + i] = __builtin_sqrt(s);
            } else Lw[i * (i + 1) / 2 + j] = s / Lw[j * (j + 1) / 2 + j];
        }
    }
    for (int i = 0; i < k; i++) {
        double s = ((fixed >> i) & 1u) ? 0.0 : b[i];
        for (int t = 0; t < i; t++) s = s - Lw[i * (i + 1) / 2 + t] * dw[t];
        dw[i] = s / Lw[i * (i + 1) / 2 + i];
    }
    for (int i = k - 1; i >= 0; i--) {
        double s = dw[i];
        for (int t = i + 1; t < k; t++) s = s - Lw[t * (t + 1) / 2 + i] * dw[t];
        dw[i] = s / Lw[i * (i + 1) / 2 + i];
    }
    return true;
}

template <int KP>
__global__ void __launch_bounds__(kUnmixThreads) unmix_fit_kernel(UnmixKernelParams kp) {
    constexpr int NA = KP * (KP + 1) / 2, NACC = NA + KP + 1;
    __shared__ double s_part[kUmWaves][NACC];
    __shared__ double s_try[NACC], s_cur[NACC];
    __shared__ double s_L[kUmWaves][NA], s_d[kUmWaves][KP], s_p[kUmWaves][KP], s_pt[kUmWaves][KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int k = kp.k;
    UmForm f;
    f.alpha_form = kp.alpha_form; f.a = kp.a; f.la = kp.alpha_form ? dlog(kp.a) : 0.0;
    const double lo = kp.alpha_form ? 1e-6 : 0.0;
    double *Lw = s_L[wave], *dw = s_d[wave], *pw = s_p[wave], *ptw = s_pt[wave];
    for (int i = blockIdx.x; i < kp.m; i += gridDim.x) {
        const double *vx = kp.vx + (long)i * kp.n;
        for (int j = 0; j < KP; j++) { pw[j] = j < k ? 1.0 : 0.0; ptw[j] = pw[j]; }
        um_pass<KP>(kp, f, vx, ptw, s_part, s_try, lane, wave);
        double L = s_try[NA + KP];
        int it = 0, flag = 1;
        if (!dfinite(L)) {
            flag = 2;
            L = dnan();
            for (int j = 0; j < k; j++) pw[j] = dnan();
        } else {
            for (int a = threadIdx.x; a < NACC; a += kUnmixThreads) s_cur[a] = s_try[a];
            __syncthreads();
            double lam = kUmLambda0;
            while (it < kp.maxit) {
                it++;
                int rej = 0;
                bool accepted = false;
                double Lt = L;
                for (;;) {
                    // the step on the free set: a coordinate on a bound whose step points outward is fixed, at most k times
                    unsigned fixed = 0;
                    for (int j = 0; j < k; j++) if (!(s_cur[j * (j + 1) / 2 + j] > 0.0)) fixed |= 1u << j;
                    bool ok = false;
                    for (int round = 0; round <= k; round++) {
                        ok = um_solve(s_cur, s_cur + NA, k, lam, fixed, Lw, dw);
                        if (!ok) break;
                        unsigned more = 0;
                        for (int j = 0; j < k; j++) {
                            if ((fixed >> j) & 1u) continue;
                            const double pj = pw[j], dj = dw[j];
                            if ((pj <= lo && dj < 0.0) || (pj >= kUmHi && dj > 0.0)) more |= 1u << j;
                        }
                        if (!more) break;
                        fixed |= more;
                    }
                    if (ok) {
                        bool same = true;
                        for (int j = 0; j < k; j++) {
                            double t = pw[j] + dw[j];
                            if (t < lo) t = lo;
                            if (t > kUmHi) t = kUmHi;
                            ptw[j] = t;
                            same = same && t == pw[j];
                        }
                        if (same) break;                     // no step moves the point: nothing left to try
                        um_pass<KP>(kp, f, vx, ptw, s_part, s_try, lane, wave);
                        Lt = s_try[NA + KP];
                        if (Lt < L) {
                            accepted = true;
                            lam = __builtin_fmax(lam * 0.25, kUmLambdaMin);
                            break;
                        }
                    }
                    lam = 4.0 * lam;
                    if (++rej >= kUmMaxReject) break;
                }
                if (!accepted) { flag = 0; break; }
                const double rel = (L - Lt) / L;
                L = Lt;
                for (int j = 0; j < k; j++) pw[j] = ptw[j];
                for (int a = threadIdx.x; a < NACC; a += kUnmixThreads) s_cur[a] = s_try[a];
                __syncthreads();
                if (rel < kUmRelTol) { flag = 0; break; }
            }
        }
        if (threadIdx.x == 0) {
            for (int j = 0; j < k; j++) kp.p[(long)i * k + j] = pw[j];
            kp.loss[i] = L;
            kp.iter[i] = it;
            kp.flag[i] = flag;
        }
        __syncthreads();
    }
}

size_t unmix_workspace_bytes(int n, int m) { return (size_t)n * (size_t)m * sizeof(double); }

hipError_t launch_unmix(const UnmixKernelParams &kp, hipStream_t st) {
    const int cus = device_cu_count();
    const long tiles = (((long)kp.m + 31) / 32) * (((long)kp.n + 31) / 32);
    const int pblocks = (int)(tiles < 16L * cus ? tiles : 16L * cus);
    int blocks = kp.m < 2 * cus ? kp.m : 2 * cus;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] unmix n=%d m=%d k=%d: prep blocks %d, fit blocks %d, threads %d\n", kp.n, kp.m, kp.k, pblocks,
                blocks, kUnmixThreads);
    hipLaunchKernelGGL(unmix_prep_kernel, dim3(pblocks), dim3(256), 0, st, kp);
    if (kp.k <= 4) hipLaunchKernelGGL(unmix_fit_kernel<4>, dim3(blocks), dim3(kUnmixThreads), 0, st, kp);
    else if (kp.k <= 8) hipLaunchKernelGGL(unmix_fit_kernel<8>, dim3(blocks), dim3(kUnmixThreads), 0, st, kp);
    else hipLaunchKernelGGL(unmix_fit_kernel<16>, dim3(blocks), dim3(kUnmixThreads), 0, st, kp);
    return hipGetLastError();
}

}  // namespace dsq
