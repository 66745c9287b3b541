// apeglm.hip -- apeglm shrinkage on the device: per-gene MAP coefficients of a negative binomial GLM under a Student t
// (Cauchy at prior_df = 1) prior, with the Laplace posterior SD (R/lfcShrink.R:328-440).
//
// Gene i, coefficients b on the natural-log scale, minimises
//     F(b) = - sum_j w_j [ y_j eta_j - (y_j + 1/a) log1p(a mu_j) ]
//            + sum_{k unshrunken} b_k^2 / (2 ns^2) + sum_{k shrunken} ((df + 1) / 2) log1p(b_k^2 / (df S^2)),
//     eta_j = x_j b + log nf_j,  mu_j = exp(eta_j)
// by the library's own deterministic damped Newton (Levenberg-Marquardt) iteration on the closed-form gradient and observed
// Hessian, stated once in tests/apeglm_spec.py and equalled bit for bit:
//     r_j = (y_j - mu_j) / (1 + a mu_j)   h_j = mu_j (1 + a y_j) / (1 + a mu_j)^2
//     g = -X' (w r) + prior',  H = X' diag(w h) X + prior'',  (H + lambda diag|H_kk|) s = -g by Cholesky in one fixed order
// A trial is accepted by the Armijo test on the TRUE objective -- or, when the predicted decrease -g.s is below what F
// resolves (2^-44 of the magnitudes F is summed from: F itself can cancel to nothing), when F did not rise by more than that --; lambda starts at 0, rises on a failed factorisation, a
// non-finite trial or a rejected one, falls after a success; an accepted UNDAMPED step with max |s| < tol ends the search.
// The posterior can have two modes, so the search runs from two starts (the shrunken start, then the caller's init) and
// the lower F is kept.
// One wavefront per gene, four genes per workgroup.  A pass over the gene's row at a point yields F, g and H together (an
// accepted trial costs no second pass): lane l adds the samples l, l + 64, ... in order from 0.0 into 1 + p + p (p + 1) / 2
// register accumulators, which combine by the xor butterfly of dsq_wave.hpp.  At the padded width 16 the triangle is
// accumulated in two sweeps (rows 0-10, rows 11-15), as unmix.hip does, to stay inside the registers of a lane; every sum
// keeps its own order, so the bits do not depend on the split.  The design is staged once per workgroup in LDS while
// m p <= kApeXLdsDoubles and read through L2 beyond; the row (counts, factors, weights) is replayed from memory per
// evaluation.  The p x p algebra runs redundantly in every lane on a per-wave piece of LDS.
#include "capi.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kApeWaves = 4;
constexpr double kApeArmijo = 1e-4;
constexpr double kApeResolution = 5.6843418860808015e-14;      // 2^-44
constexpr double kApeLamFirst = 1e-4, kApeLamUp = 10.0, kApeLamDown = 0.1, kApeLamZero = 1e-7, kApeLamMax = 1e12;
constexpr double kApeClip = 30.0;

// the prior's constants, formed the way the specification forms them
struct ApePrior { double ds2, df1, c, ns2, two_ns2; };

// one sweep over the samples at the point b: rows [R0, R1) of the packed lower triangle of H (entry (i, j), j <= i, at
// 1 + KP + i (i + 1) / 2 + j of sys), g_i of those rows at 1 + i and, with R0 == 0, the likelihood part of F at 0 and the sum
// of the magnitudes it is made of at 1 + KP + NA -- the sums only, signs and prior are added by ape_eval
template <int KP, int R0, int R1, typename T>
DSQ_DEV void ape_sweep(const ApeglmKernelParams &kp, const double *xs, long row, double a, double inva, const double (&b)[KP],
                       double *sys, int lane) {
    constexpr int A0 = R0 * (R0 + 1) / 2, A1 = R1 * (R1 + 1) / 2;
    constexpr int NH = A1 - A0, NG = R1 - R0, N = NH + NG + (R0 == 0 ? 2 : 0), NA = KP * (KP + 1) / 2;
    double acc[N];
#pragma unroll
    for (int c = 0; c < N; c++) acc[c] = 0.0;
    const T *y = (const T *)kp.y;
    const int m = kp.m, p = kp.p;
    for (int j = lane; j < m; j += 64) {
        const long at = row + (long)j * kp.sj;
        const double yj = (double)y[at];
        const double oj = dlog(kp.nf[kp.nf_is_vector ? (long)j : at]);
        double xr[KP];
#pragma unroll
        for (int k = 0; k < KP; k++) xr[k] = k < p ? xs[(long)k * m + j] : 0.0;
        double e = xr[0] * b[0];
#pragma unroll
        for (int k = 1; k < KP; k++) e = e + xr[k] * b[k];
        const double eta = e + oj;
        const double mu = dexp(eta);
        const double am = a * mu;
        const double d1 = 1.0 + am;
        // (no weights: w = 1, and 1.0 * t is t -- the bits of a weights matrix of ones)
        const double wj = kp.weights ? kp.weights[at] : 1.0;
        const double wr = wj * ((yj - mu) / d1);
        const double wh = wj * ((mu * (1.0 + a * yj)) / (d1 * d1));
        if constexpr (R0 == 0) {
            const double t1 = yj * eta, t2 = (yj + inva) * dlog1p(am);
            acc[NH + NG] = acc[NH + NG] + wj * (t1 - t2);
            acc[NH + NG + 1] = acc[NH + NG + 1] + wj * (__builtin_fabs(t1) + t2);       // the magnitude F is summed from
        }
#pragma unroll
        for (int i = R0; i < R1; i++) {
            acc[NH + i - R0] = acc[NH + i - R0] + wr * xr[i];
            const double whx = wh * xr[i];
#pragma unroll
            for (int k = 0; k <= i; k++) acc[i * (i + 1) / 2 + k - A0] = acc[i * (i + 1) / 2 + k - A0] + whx * xr[k];
        }
    }
    wave_allreduce_many<N>(acc, lane);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NH; c++) sys[1 + KP + A0 + c] = acc[c];
#pragma unroll
        for (int c = 0; c < NG; c++) sys[1 + R0 + c] = acc[NH + c];
        if constexpr (R0 == 0) { sys[0] = acc[NH + NG]; sys[1 + KP + NA] = acc[NH + NG + 1]; }
    }
}

// F, g, H at the point bw[0 .. p) (the wave's LDS) into sys[]: sys[0] = F, sys[1 + k] = g_k, sys[1 + KP + i (i + 1) / 2 + j] = H_ij,
// sys[1 + KP + NA] = the magnitude of F: the sum of |y eta| + (y + 1/a) log1p(a mu) and of the prior's terms, which is what F resolves
template <int KP, typename T>
DSQ_DEV void ape_eval(const ApeglmKernelParams &kp, const ApePrior &pr, const double *xs, long row, double a, double inva,
                      const double *bw, double *sys, int lane) {
    double b[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) b[k] = k < kp.p ? bw[k] : 0.0;
    if constexpr (KP <= 8) ape_sweep<KP, 0, KP, T>(kp, xs, row, a, inva, b, sys, lane);
    else {
        ape_sweep<KP, 0, 11, T>(kp, xs, row, a, inva, b, sys, lane);
        ape_sweep<KP, 11, KP, T>(kp, xs, row, a, inva, b, sys, lane);
    }
    wave_lds_sync();
    // signs and the prior: every lane computes the same values; lane 0 stores them
    constexpr int NA = KP * (KP + 1) / 2;
    double F = -sys[0], Fm = sys[1 + KP + NA];
    for (int k = 0; k < kp.p; k++) {
        const int kk = 1 + KP + k * (k + 1) / 2 + k;
        const double bk = bw[k];
        double g = -sys[1 + k], h = sys[kk];
        if ((kp.no_shrink >> k) & 1u) {
            const double t = (bk * bk) / pr.two_ns2;
            F = F + t;
            Fm = Fm + t;
            g = g + bk / pr.ns2;
            h = h + 1.0 / pr.ns2;
        } else {
            const double bb = bk * bk, den = pr.ds2 + bb;
            const double t = pr.c * dlog1p(bb / pr.ds2);
            F = F + t;
            Fm = Fm + t;
            g = g + (pr.df1 * bk) / den;
            h = h + (pr.df1 * (pr.ds2 - bb)) / (den * den);
        }
        wave_lds_sync();
        if (lane == 0) { sys[1 + k] = g; sys[kk] = h; }
    }
    wave_lds_sync();
    if (lane == 0) { sys[0] = F; sys[1 + KP + NA] = Fm; }
    wave_lds_sync();
}

// (H + lam diag|H_kk|) d = rhs by Cholesky in one fixed order; H: the packed lower triangle.  Lw: the wave's scratch (every
// lane writes the same values).  false: a pivot that is not positive and finite.
DSQ_DEV bool ape_solve(const double *H, const double *rhs, int p, double lam, double *Lw, double *d) {
    for (int i = 0; i < p; i++) {
        for (int j = 0; j <= i; j++) {
            double s = H[i * (i + 1) / 2 + j];
            if (i == j) s = s + lam * __builtin_fabs(s);
            for (int t = 0; t < j; t++) s = s - Lw[i * (i + 1) / 2 + t] * Lw[j * (j + 1) / 2 + t];
            if (i == j) {
                if (!(s > 0.0 && s < kInf)) return false;
                Lw[i * (i + 1) / 2 + i] = __builtin_sqrt(s);
            } else Lw[i * (i + 1) / 2 + j] = s / Lw[j * (j + 1) / 2 + j];
        }
    }
    for (int i = 0; i < p; i++) {
        double s = rhs[i];
        for (int t = 0; t < i; t++) s = s - Lw[i * (i + 1) / 2 + t] * d[t];
        d[i] = s / Lw[i * (i + 1) / 2 + i];
    }
    for (int i = p - 1; i >= 0; i--) {
        double s = d[i];
        for (int t = i + 1; t < p; t++) s = s - Lw[t * (t + 1) / 2 + i] * d[t];
        d[i] = s / Lw[i * (i + 1) / 2 + i];
    }
    return true;
}

template <int KP, typename T, bool XLDS>
__global__ void __launch_bounds__(64 * kApeWaves) apeglm_kernel(ApeglmKernelParams kp) {
    constexpr int NA = KP * (KP + 1) / 2, NACC = 2 + KP + NA;
    extern __shared__ double ape_x[];
    __shared__ double s_cur[kApeWaves][NACC], s_try[kApeWaves][NACC], s_best[kApeWaves][NACC];
    __shared__ double s_L[kApeWaves][NA], s_vec[kApeWaves][5][KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = kp.m, p = kp.p;
    const double *xs;
    if constexpr (XLDS) {
        for (int t = threadIdx.x; t < m * p; t += 64 * kApeWaves) ape_x[t] = kp.x[t];      // (m p <= kApeXLdsDoubles here)
        __syncthreads();
        xs = ape_x;
    } else xs = kp.x;
    ApePrior pr;
    pr.ds2 = kp.prior_df * (kp.prior_scale * kp.prior_scale);
    pr.df1 = kp.prior_df + 1.0;
    pr.c = pr.df1 / 2.0;
    pr.ns2 = kp.no_shrink_scale * kp.no_shrink_scale;
    pr.two_ns2 = 2.0 * pr.ns2;
    double *cur = s_cur[wave], *tr = s_try[wave], *best = s_best[wave], *Lw = s_L[wave];
    double *bw = s_vec[wave][0], *bt = s_vec[wave][1], *sw = s_vec[wave][2], *rhs = s_vec[wave][3], *bbest = s_vec[wave][4];
    const T *y = (const T *)kp.y;
    const int nstart = kp.init ? 2 : 1;
    for (int i = blockIdx.x * kApeWaves + wave; i < kp.n; i += gridDim.x * kApeWaves) {
        const long row = (long)i * kp.si;
        const double a = kp.disp[i];
        // ---- the rows that are not fitted, and the weighted mean of the normalized counts for the start
        double sy = 0.0, sws = 0.0;
        int nz = 0;
        for (int j = lane; j < m; j += 64) {
            const long at = row + (long)j * kp.sj;
            const double yj = count_value<T>(y[at], kp.bad);
            const double wj = kp.weights ? kp.weights[at] : 1.0;
            sy = sy + wj * (yj / kp.nf[kp.nf_is_vector ? (long)j : at]);
            sws = sws + wj;
            nz |= yj != 0.0;
        }
        nz = __any(nz);
        if (!(a > 0.0 && a < kInf) || !nz) {
            if (lane == 0) {
                for (int k = 0; k < p; k++) { kp.map[(long)i * p + k] = dnan(); kp.sd[(long)i * p + k] = dnan(); }
                kp.fsr[i] = dnan(); kp.thresh[i] = dnan(); kp.iter[2L * i] = dnan(); kp.iter[2L * i + 1] = dnan();
                kp.conv[i] = dnan(); kp.start[i] = dnan(); kp.objective[i] = dnan();
            }
            continue;
        }
        wave_allreduce_pair(sy, sws, lane);
        const double inva = 1.0 / a;
        double b_conv = 0.0, b_start = 0.0, iters[2] = {0.0, 0.0};
        for (int st = 0; st < nstart; st++) {
            wave_lds_sync();
            if (lane == 0) {
                if (st == 0) {
                    for (int k = 0; k < p; k++) bw[k] = 0.0;
                    if (kp.no_shrink & 1u) {
                        const double q = sws > 0.0 ? sy / sws : 0.0;
                        bw[0] = dlog(q > 0.1 ? q : 0.1);
                    }
                } else {
                    for (int k = 0; k < p; k++) {
                        const double v = kp.init[(long)i * p + k];
                        bw[k] = v < -kApeClip ? -kApeClip : (v > kApeClip ? kApeClip : v);
                    }
                }
            }
            wave_lds_sync();
            ape_eval<KP, T>(kp, pr, xs, row, a, inva, bw, cur, lane);
            int it = 0, conv = 1;
            if (!uniform(dfinite(cur[0]))) {
                conv = 2;
                wave_lds_sync();
                if (lane == 0) cur[0] = dnan();
                wave_lds_sync();
            } else {
                double lam = 0.0;
                while (it < kp.maxit) {
                    it++;
                    bool accepted = false;
                    double smax = 0.0;
                    for (;;) {
                        wave_lds_sync();
                        for (int k = lane; k < p; k += 64) rhs[k] = -cur[1 + k];
                        wave_lds_sync();
                        if (uniform(ape_solve(cur + 1 + KP, rhs, p, lam, Lw, sw))) {
                            wave_lds_sync();
                            double gs = cur[1] * sw[0];
                            smax = __builtin_fabs(sw[0]);
                            for (int k = 1; k < p; k++) {
                                gs = gs + cur[1 + k] * sw[k];
                                const double ak = __builtin_fabs(sw[k]);
                                smax = ak > smax ? ak : (ak != ak ? ak : smax);
                            }
                            for (int k = lane; k < p; k += 64) bt[k] = bw[k] + sw[k];
                            wave_lds_sync();
                            ape_eval<KP, T>(kp, pr, xs, row, a, inva, bt, tr, lane);
                            const double pred = -gs, F = cur[0], Ft = tr[0];
                            const double Fm = cur[1 + KP + NA];
                            const double res = kApeResolution * (Fm > 1.0 ? Fm : 1.0);
                            const bool ok = dfinite(Ft) && (pred > res ? Ft <= F - kApeArmijo * pred : Ft <= F + res);
                            if (uniform(ok)) { accepted = true; break; }
                        }
                        lam = lam < kApeLamFirst ? kApeLamFirst : lam * kApeLamUp;
                        if (lam > kApeLamMax) break;
                    }
                    if (!accepted) { conv = 2; break; }
                    wave_lds_sync();
                    for (int t = lane; t < NACC; t += 64) cur[t] = tr[t];
                    for (int k = lane; k < p; k += 64) bw[k] = bt[k];
                    wave_lds_sync();
                    if (lam == 0.0 && smax < kp.tol) { conv = 0; break; }
                    lam = lam * kApeLamDown;
                    if (lam < kApeLamZero) lam = 0.0;
                }
            }
            iters[st] = (double)it;
            if (st == 0 || uniform(cur[0] < best[0])) {
                wave_lds_sync();
                for (int t = lane; t < NACC; t += 64) best[t] = cur[t];
                for (int k = lane; k < p; k += 64) bbest[k] = bw[k];
                wave_lds_sync();
                b_conv = (double)conv;
                b_start = (double)st;
            }
        }
        // ---- the Laplace approximation at the point kept: sd_k = sqrt((H^-1)_kk), one solve per coordinate
        double sdc = dnan();
        bool pd = true;
        for (int k = 0; k < p && pd; k++) {
            wave_lds_sync();
            for (int t = lane; t < p; t += 64) rhs[t] = t == k ? 1.0 : 0.0;
            wave_lds_sync();
            pd = uniform(ape_solve(best + 1 + KP, rhs, p, 0.0, Lw, sw));
            if (pd) {
                wave_lds_sync();
                const double sd = __builtin_sqrt(sw[k]);
                if (k == kp.coef) sdc = sd;
                if (lane == 0) kp.sd[(long)i * p + k] = sd;
            }
        }
        if (!pd) {
            sdc = dnan();
            b_conv = b_conv + 4.0;
            if (lane == 0) for (int k = 0; k < p; k++) kp.sd[(long)i * p + k] = dnan();
        }
        const double mc = bbest[kp.coef];
        const double fsr = dpnorm_lower(-(__builtin_fabs(mc) / sdc));
        double th = dnan();
        if (kp.has_threshold) {
            double l1, u1, l2, u2;
            dpnorm_both((kp.threshold - mc) / sdc, l1, u1);
            dpnorm_both((-kp.threshold - mc) / sdc, l2, u2);
            th = mc >= 0.0 ? l1 - l2 : u2 - u1;
        }
        if (lane == 0) {
            for (int k = 0; k < p; k++) kp.map[(long)i * p + k] = bbest[k];
            kp.fsr[i] = fsr; kp.thresh[i] = th;
            kp.iter[2L * i] = iters[0]; kp.iter[2L * i + 1] = nstart > 1 ? iters[1] : 0.0;
            kp.conv[i] = b_conv; kp.start[i] = b_start; kp.objective[i] = best[0];
        }
    }
}

template <int KP, typename T>
static void launch_ape_x(const ApeglmKernelParams &kp, int blocks, hipStream_t st) {
    const long xd = (long)kp.m * kp.p;
    if (xd <= kApeXLdsDoubles)
        hipLaunchKernelGGL((apeglm_kernel<KP, T, true>), dim3(blocks), dim3(64 * kApeWaves), (size_t)xd * sizeof(double), st, kp);
    else hipLaunchKernelGGL((apeglm_kernel<KP, T, false>), dim3(blocks), dim3(64 * kApeWaves), 0, st, kp);
}

template <typename T>
static void launch_ape_p(const ApeglmKernelParams &kp, int blocks, hipStream_t st) {
    if (kp.p <= 4) launch_ape_x<4, T>(kp, blocks, st);
    else if (kp.p <= 8) launch_ape_x<8, T>(kp, blocks, st);
    else launch_ape_x<16, T>(kp, blocks, st);
}

hipError_t launch_apeglm(const ApeglmKernelParams &kp, int y_f64, hipStream_t st) {
    int blocks = (kp.n + kApeWaves - 1) / kApeWaves;
    const int most = 8 * device_cu_count();
    if (blocks > most) blocks = most;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] apeglm n=%d m=%d p=%d: design in %s, blocks %d, threads %d\n", kp.n, kp.m, kp.p,
                (long)kp.m * kp.p <= kApeXLdsDoubles ? "LDS" : "L2", blocks, 64 * kApeWaves);
    if (y_f64) launch_ape_p<double>(kp, blocks, st);
    else launch_ape_p<int32_t>(kp, blocks, st);
    return hipGetLastError();
}

}  // namespace dsq
