// rlog.hip -- the regularized-logarithm fit on the device.
//
// rlogData (R/rlog.R:172-272) hands fitNbinomGLMs a design with one coefficient per sample and a ridge on each of them:
// [1 | I_m] (form A, no intercept given) or I_m (form B, the caller's intercept folded into the factors).  The normal
// equations of an IRLS step of such a design are an arrow matrix (form A) or a diagonal one (form B), so the step of
// src/DESeq2.cpp:334-383 is two sums over the samples plus elementwise work -- O(m) per step for ANY m, where the dense
// kernels stop at 64 columns:
//     w = mu / (1 + alpha mu)   z = log(mu / nf) + (y - mu) / mu   u = w / (w + lambda)   h = lambda u
//     A:  beta0 = sum h z / (lambda0 + sum h),  beta_j = u_j (z_j - beta0)        B:  beta_j = u_j z_j
// One wavefront per gene, lane l on samples l, l + 64, ...; the sums are lane-serial partials and the xor butterfly of
// dsq_wave.hpp (the order tests/rlog_spec.py states).  The per-sample state is ONE double, beta_j: mu_j is a function
// of it and of the wave-uniform beta0 (one exp) and is recomputed where it is needed, so the coefficients of the step
// that ends the loop are still there when it ends.  Where it lives:
//     m <= 64 kRegs            registers (kRegs per lane)
//     m <= kLdsDoubles         LDS, m doubles per wave (a workgroup asks for 4 m doubles: nothing beyond 64 KiB)
//     beyond                   the gene's own output row -- exactly m doubles, overwritten by the result at the end
// A lane only ever reads back what it wrote itself, in all three: no barrier, no fence.
// Two sweeps per iteration: the first gives sum h and sum h z, the second beta_j, the new mu_j and the deviance term.
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kRlogRegs = 4;                  // registers regime up to m = 256
constexpr int kRlogLdsDoubles = 2048;         // LDS regime up to m = 2048 (4 waves x 2048 x 8 bytes = 64 KiB)
constexpr double kRlogLn2 = 6.93147180559945286227e-01;      // the double nearest to ln 2: R's log(2)
constexpr double kRlogLarge = 30.0;

enum { RLOG_REG = 0, RLOG_LDS = 1, RLOG_ROW = 2 };

// the per-sample coefficients of one gene
template <int MODE>
struct RlogState {
    double r[MODE == RLOG_REG ? kRlogRegs : 1];
    double *p;
    long stride;
    DSQ_DEV double get(int k, int j) const { if constexpr (MODE == RLOG_REG) return r[k]; else return p[(long)j * stride]; }
    DSQ_DEV void set(int k, int j, double v) { if constexpr (MODE == RLOG_REG) r[k] = v; else p[(long)j * stride] = v; }
};

// the samples of a lane: k-th sample is j = lane + 64 k (registers regime: a compile-time trip count, unrolled, so that
// r[k] stays in registers)
#define RLOG_FOR_SAMPLES(k, j)                                                            \
    _Pragma("unroll MODE == RLOG_REG ? kRlogRegs : 1")                                    \
    for (int k = 0; k < (MODE == RLOG_REG ? kRlogRegs : nk); k++)                         \
        if (const int j = lane + 64 * k; j < kp.m)

template <int MODE, typename T, int FORM_B>
__global__ void __launch_bounds__(256) rlog_kernel(RlogKernelParams kp) {
    extern __shared__ double rlog_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwave = gridDim.x * 4;
    const int nk = (kp.m + 63) >> 6;
    const T *y = (const T *)kp.y;
    const double lam = kp.lambda, lam0 = kp.lambda0;
    for (int i = blockIdx.x * 4 + wave; i < kp.n; i += nwave) {
        const long row = (long)i * kp.si;
        const double alpha = kp.dispFit[i];
        const double size = 1.0 / alpha;
        double st_size, lg_size;
        dnbinom_size_terms(size, st_size, lg_size);
        RlogState<MODE> st;
        if constexpr (MODE == RLOG_LDS) { st.p = rlog_lds + (long)wave * kp.m; st.stride = 1; }
        if constexpr (MODE == RLOG_ROW) { st.p = kp.out + row; st.stride = kp.sj; }
        // ---- the start (R/fitNbinomGLMs.R:144-151) and the all-zero rows (R/rlog.R:223,227)
        double c = 0.0, fscale = 1.0, beta0 = 0.0;
        bool zero_row;
        if constexpr (FORM_B) {
            c = kp.intercept[i];
            zero_row = !dfinite(c);
            fscale = dexp((zero_row ? -10.0 : c) * kRlogLn2);
            RLOG_FOR_SAMPLES(k, j) {
                const long at = row + (long)j * kp.sj;
                const double yj = count_value<T>(y[at], kp.bad);
                const double nfj = kp.nf[kp.nf_is_vector ? (long)j : at] * fscale;
                st.set(k, j, dlog(yj / nfj + 0.1));
            }
        } else {
            double s = 0.0;
            int nz = 0;
            RLOG_FOR_SAMPLES(k, j) {
                const long at = row + (long)j * kp.sj;
                const double yj = count_value<T>(y[at], kp.bad);
                s += yj / kp.nf[kp.nf_is_vector ? (long)j : at];
                nz |= yj != 0.0;
                st.set(k, j, 0.0);
            }
            zero_row = !__any(nz);
            beta0 = dlog(wave_allreduce(s) / (double)kp.m);
        }
        if (zero_row) {
            RLOG_FOR_SAMPLES(k, j) kp.out[row + (long)j * kp.sj] = 0.0;
            if (lane == 0) {
                if (kp.intercept_out) kp.intercept_out[i] = -kInf;
                kp.iter[i] = 0.0;
                kp.flag[i] = 1;
            }
            continue;
        }
        // ---- the IRLS loop (src/DESeq2.cpp:334-383, the QR branch)
        double it = 0.0, dev_old = 0.0;
        for (int t = 0; t < kp.maxit; t++) {
            it += 1.0;
            if constexpr (!FORM_B) {
                double s1 = 0.0, s2 = 0.0;
                RLOG_FOR_SAMPLES(k, j) {
                    const long at = row + (long)j * kp.sj;
                    const double yj = (double)y[at];
                    const double nfj = kp.nf[kp.nf_is_vector ? (long)j : at];
                    const double mu = __builtin_fmax(nfj * dexp(beta0 + st.get(k, j)), kp.minmu);
                    const double w = mu / (1.0 + alpha * mu);
                    const double z = dlog(mu / nfj) + (yj - mu) / mu;
                    const double h = lam * (w / (w + lam));
                    s1 += h;
                    s2 += h * z;
                }
                wave_allreduce_pair(s1, s2, lane);
                // (the old beta0 is still needed by the second sweep: it recomputes mu, w, z of this step)
                const double beta0_new = s2 / (lam0 + s1);
                int large = __builtin_fabs(beta0_new) > kRlogLarge;
                RLOG_FOR_SAMPLES(k, j) {
                    const long at = row + (long)j * kp.sj;
                    const double yj = (double)y[at];
                    const double nfj = kp.nf[kp.nf_is_vector ? (long)j : at];
                    const double mu = __builtin_fmax(nfj * dexp(beta0 + st.get(k, j)), kp.minmu);
                    const double w = mu / (1.0 + alpha * mu);
                    const double z = dlog(mu / nfj) + (yj - mu) / mu;
                    const double b = (w / (w + lam)) * (z - beta0_new);
                    large |= __builtin_fabs(b) > kRlogLarge;
                    st.set(k, j, b);
                }
                beta0 = beta0_new;
                if (__any(large)) { it = (double)kp.maxit; break; }
            } else {
                int large = 0;
                RLOG_FOR_SAMPLES(k, j) {
                    const long at = row + (long)j * kp.sj;
                    const double yj = (double)y[at];
                    const double nfj = kp.nf[kp.nf_is_vector ? (long)j : at] * fscale;
                    const double mu = __builtin_fmax(nfj * dexp(st.get(k, j)), kp.minmu);
                    const double w = mu / (1.0 + alpha * mu);
                    const double z = dlog(mu / nfj) + (yj - mu) / mu;
                    const double b = (w / (w + lam)) * z;
                    large |= __builtin_fabs(b) > kRlogLarge;
                    st.set(k, j, b);
                }
                if (__any(large)) { it = (double)kp.maxit; break; }
            }
            double d = 0.0;
            RLOG_FOR_SAMPLES(k, j) {
                const long at = row + (long)j * kp.sj;
                const double yj = (double)y[at];
                double nfj = kp.nf[kp.nf_is_vector ? (long)j : at];
                if constexpr (FORM_B) nfj = nfj * fscale;
                const double eta = FORM_B ? st.get(k, j) : beta0 + st.get(k, j);
                const double mu = __builtin_fmax(nfj * dexp(eta), kp.minmu);
                d += dnbinom_mu_log(yj, size, mu, st_size, lg_size);
            }
            const double dev = -2.0 * wave_allreduce(d);
            const double conv = __builtin_fabs(dev - dev_old) / (__builtin_fabs(dev) + 0.1);
            if (conv != conv) { it = (double)kp.maxit; break; }
            if (t > 0 && conv < kp.tol) break;
            dev_old = dev;
        }
        // ---- the result (R/fitNbinomGLMs.R:194, R/rlog.R:254-269); a non-finite coefficient: the row R would hand to optim
        int nonfinite = !dfinite(beta0);
        RLOG_FOR_SAMPLES(k, j) nonfinite |= !dfinite(st.get(k, j));
        nonfinite = __any(nonfinite);
        const double b0l = beta0 * kInvLn2;
        RLOG_FOR_SAMPLES(k, j) {
            const double b = st.get(k, j);
            double v = FORM_B ? b * kInvLn2 + c : b0l + b * kInvLn2;
            if (nonfinite) v = dnan();
            kp.out[row + (long)j * kp.sj] = v;
        }
        if (lane == 0) {
            if (kp.intercept_out) kp.intercept_out[i] = nonfinite ? dnan() : b0l;
            kp.iter[i] = it;
            kp.flag[i] = nonfinite ? 2 : 0;
        }
    }
}

template <int MODE, typename T>
static void launch_rlog_form(const RlogKernelParams &kp, int blocks, size_t lds, hipStream_t st) {
    if (kp.intercept) hipLaunchKernelGGL((rlog_kernel<MODE, T, 1>), dim3(blocks), dim3(256), lds, st, kp);
    else hipLaunchKernelGGL((rlog_kernel<MODE, T, 0>), dim3(blocks), dim3(256), lds, st, kp);
}

template <typename T>
static void launch_rlog_t(const RlogKernelParams &kp, int blocks, hipStream_t st) {
    if (kp.m <= 64 * kRlogRegs) launch_rlog_form<RLOG_REG, T>(kp, blocks, 0, st);
    else if (kp.m <= kRlogLdsDoubles) launch_rlog_form<RLOG_LDS, T>(kp, blocks, (size_t)4 * kp.m * sizeof(double), st);
    else launch_rlog_form<RLOG_ROW, T>(kp, blocks, 0, st);
}

hipError_t launch_rlog(const RlogKernelParams &kp, int y_f64, hipStream_t st) {
    int blocks = (kp.n + 3) / 4;
    const int most = 8 * device_cu_count();
    if (blocks > most) blocks = most;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] rlog n=%d m=%d form %c: mode %d, blocks %d, threads 256\n", kp.n, kp.m, kp.intercept ? 'B' : 'A',
                kp.m <= 64 * kRlogRegs ? RLOG_REG : kp.m <= kRlogLdsDoubles ? RLOG_LDS : RLOG_ROW, blocks);
    if (y_f64) launch_rlog_t<double>(kp, blocks, st);
    else launch_rlog_t<int32_t>(kp, blocks, st);
    return hipGetLastError();
}

}  // namespace dsq
