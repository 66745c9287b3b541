// sf_iterate.hip -- the solve of estimateSizeFactors(type = "iterate") on the device (R/core.R:2589-2622; DESIGN.md
// section 18).
//
// One outer round of estimateSizeFactorsIterate fixes the counts k, q = t(t(mu) / sf) and the dispersions a over the rows
// with a positive row sum, and maximises over the centred log size factors s
//     F(s) = sum of L_i over { i : L_i > quantile(L, Q) },   L_i = sum_j log NB(k_ij; mu = q_ij exp(s_j), size = 1 / a_i).
// R hands F to optim(method = "L-BFGS-B") without a gradient: 2 m further n x m passes per gradient.  On a fixed kept
// set F separates in the samples, coupled only by the gauge sum s = 0, so Newton's step under the constraint is closed:
//     g_j = sum_kept (k - mu) / (1 + a mu)      h_j = sum_kept mu (1 + a k) / (1 + a mu)^2
//     lambda = sum_j (g_j / h_j) / sum_j (1 / h_j)      d_j = (g_j - lambda) / h_j
// The kept set moves with s, so the step is safeguarded by an Armijo test on the true F, the cut re-evaluated at every
// trial point.  The iteration is stated once in tests/sf_iterate_spec.py and equalled bit for bit here.
//
// Kernels.  sfi_row_kernel: one wave per gene over its gene-major row, L_i = K'_i + the wave-order sum of nb_split_var,
// exactly loglike_kernel's sums (aux.hip) at mu = (mu_ij / sf_j) exp(s_j); the division is redone in every sweep (it is
// rounded once either way; an n x m workspace and its traffic are saved), K'_i is computed in the first sweep and kept.
// sfi_cut_kernel: one workgroup; one sweep counts the rows n' and the NaN among their L_i, the two order statistics around
// (n' - 1) Q come from the library's selection (dsq_select.hpp: radix_select for the lower one, next_order_stat for the
// upper one), then the type-7 cut, and F = the kept L_i added by thread t of T = 1024 over the rows t, t + T, ..., the 64
// lanes of a wave by the butterfly, the 16 waves in order.  sfi_col_kernel, only at an accepted point: lanes along the
// samples, one wave per (slice of kSfIterSliceGenes consecutive genes, tile of 64 samples), the genes of a slice in
// order, a row that is not kept a wave-uniform skip; the partial sums go to the workspace.  sfi_colsum_kernel adds them in
// slice order, sfi_step_kernel forms lambda, d and g.d; sfi_trial_kernel the centred trial point and its exponentials.  No
// floating-point atomics anywhere.  The host loop reads one 40-byte record back per evaluation and decides the next step.
#include "capi.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_select.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kSfiCutThreads = 1024;
constexpr int kSfiCutWaves = kSfiCutThreads / 64;
constexpr int kSfiVecThreads = 256;
constexpr int kSfiMaxTrials = 30;
constexpr double kSfiArmijo = 1e-4, kSfiRelTol = 1e-10;

struct SfiRecord {
    double F, cut, gd;
    int32_t nrows, nkept, nbad, pad;
};

// the solve's state, carved from the caller's workspace
struct SfiState {
    double *kconst;      // n: K'_i
    double *L[2];        // n each: the row log likelihoods at the current and at the trial point
    double *part;        // slices x 2 x m: the partial column sums of g and h
    double *s[2], *e[2]; // m each: the point and its exponentials, current and trial
    double *d, *g, *h;   // m each
    SfiRecord *rec;
};

// the sum of f(0), f(1), ..., f(m - 1) in index order from 0.0, the same value in every thread of the workgroup: the values
// are staged 256 at a time in LDS (one coalesced sweep), thread 0 adds them in order.  m is the same in every thread.
template <class F>
DSQ_DEV double sfi_serial_sum(int m, double *stage, F f) {
    double acc = 0.0;
    for (int j0 = 0; j0 < m; j0 += kSfiVecThreads) {
        const int j = j0 + (int)threadIdx.x;
        __syncthreads();
        stage[threadIdx.x] = j < m ? f(j) : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int c = m - j0 < kSfiVecThreads ? m - j0 : kSfiVecThreads;
            for (int t = 0; t < c; t++) acc = acc + stage[t];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) stage[kSfiVecThreads] = acc;
    __syncthreads();
    return stage[kSfiVecThreads];
}

// ---- the start: s = log(sf) - mean(log(sf)), the mean a serial sum in sample order; e = exp(s)
__global__ void __launch_bounds__(kSfiVecThreads) sfi_prep_kernel(SfIterateKernelParams kp, double *s, double *e) {
    __shared__ double stage[kSfiVecThreads + 1];
    for (int j = threadIdx.x; j < kp.m; j += kSfiVecThreads) s[j] = sf_log(kp.sf[j]);
    const double mean = sfi_serial_sum(kp.m, stage, [&](int j) { return s[j]; }) / (double)kp.m;
    for (int j = threadIdx.x; j < kp.m; j += kSfiVecThreads) {
        const double v = s[j] - mean;
        s[j] = v;
        e[j] = sf_exp(v);
    }
}

// the centred trial point u - mean(u), u = s + t d, and its exponentials
__global__ void __launch_bounds__(kSfiVecThreads) sfi_trial_kernel(int m, const double *s, const double *d, double t, double *st,
                                                                   double *et) {
    __shared__ double stage[kSfiVecThreads + 1];
    for (int j = threadIdx.x; j < m; j += kSfiVecThreads) st[j] = s[j] + t * d[j];
    const double mean = sfi_serial_sum(m, stage, [&](int j) { return st[j]; }) / (double)m;
    for (int j = threadIdx.x; j < m; j += kSfiVecThreads) {
        const double v = st[j] - mean;
        st[j] = v;
        et[j] = sf_exp(v);
    }
}

// ---- the row pass: L_i at the point whose exponentials are e; K' is loglike_constants (dsq_wave.hpp), without weights
template <bool CONSTS>
__global__ void __launch_bounds__(256) sfi_row_kernel(SfIterateKernelParams kp, double *kconst, const double *e, double *L) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = kp.m;
    for (int g = blockIdx.x * 4 + wave; g < kp.n; g += gridDim.x * 4) {
        if (kp.rows[g] == 0) continue;                 // (its dispersion is not read)
        const int32_t *yg = kp.y + (size_t)g * kp.ld;
        const double *mug = kp.mu + (size_t)g * kp.ld;
        const double alpha = kp.disp[g];
        const double size = 1.0 / alpha;
        const bool fast = nb_split_fast(alpha, size);
        double Kp;
        if constexpr (CONSTS) {
            Kp = loglike_constants<false>(yg, nullptr, m, lane, alpha, size, fast);
            if (lane == 0) kconst[g] = Kp;
        } else Kp = kconst[g];
        double acc = 0.0;
        for (int j = lane; j < m; j += 64) {
            const double mu = (mug[j] / kp.sf[j]) * e[j];
            acc += nb_split_var((double)yg[j], size, alpha, mu, fast);
        }
        acc = wave_allreduce(acc);
        if (lane == 0) L[g] = Kp + acc;
    }
}

// ---- the cut and F: one workgroup
// a sweep over the flagged rows: thread t visits the rows t, t + T, t + 2 T, ... in that order; the loads of eight of them
// are issued together (one workgroup owns the whole vector: the sweeps are bound by the latency of its loads)
template <class Fn>
DSQ_DEV void sfi_sweep(const SfIterateKernelParams &kp, const double *L, Fn fn) {
    constexpr int U = 8;
    for (int base = threadIdx.x; base < kp.n; base += U * kSfiCutThreads) {
        int r[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = base + u * kSfiCutThreads;
            r[u] = i < kp.n ? kp.rows[i] : 0;
            v[u] = i < kp.n ? L[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (r[u] != 0) fn(v[u]);
    }
}

__global__ void __launch_bounds__(kSfiCutThreads) sfi_cut_kernel(SfIterateKernelParams kp, const double *L, SfiRecord *rec) {
    __shared__ __attribute__((aligned(16))) unsigned hist[2048];
    __shared__ unsigned long long bc[3];
    __shared__ unsigned int s_cnt[3];                  // the rows n' | the NaN among their L_i | the rows kept
    __shared__ double s_wave[kSfiCutWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 3) s_cnt[tid] = 0u;
    __syncthreads();
    // the rows n' and the NaN among their L_i, before any key is formed (order_key must not see a NaN)
    unsigned int nr = 0u, nb = 0u;
    sfi_sweep(kp, L, [&](double v) {
        nr++;
        if (v != v) nb++;
    });
    if (nr) atomicAdd(&s_cnt[0], nr);
    if (nb) atomicAdd(&s_cnt[1], nb);
    __syncthreads();
    const unsigned int nrows = s_cnt[0], nbad = s_cnt[1];
    if (nrows == 0u || nbad != 0u) {                   // a NaN among the L_i: F is not finite
        if (tid == 0) {
            rec->F = nbad ? dnan() : 0.0;
            rec->cut = dnan();
            rec->nrows = (int32_t)nrows; rec->nkept = 0; rec->nbad = (int32_t)nbad;
        }
        return;
    }
    // quantile(L, Q), type 7: h = (n' - 1) Q between the order statistics lo = floor(h) and lo + 1.  Both by the shared
    // selection over all n entries, a row that does not take part entering as +inf (as in trend_mean_kernel): the n - n'
    // sentinels sort last, lo <= n' - 1 is never one of them, and gq != 0 means h < n' - 1, so lo + 1 <= n' - 1 is not either.
    const double hq = (double)(nrows - 1u) * kp.Q;
    const unsigned int lo = (unsigned int)__builtin_floor(hq);
    const double gq = hq - (double)lo;
    const double inf = __builtin_inf();
    const auto val = [&](int i) { return kp.rows[i] != 0 ? L[i] : inf; };
    SelState sel = {hist, bc, nullptr, 0};
    const double slo = radix_select<1>(kp.n, (long)lo, val, sel, 0);
    double cut = slo;
    if (gq != 0.0) {
        const double shi = next_order_stat<1>(kp.n, slo, (long)lo, val, sel, 0);
        if (!(shi == slo)) cut = (1.0 - gq) * slo + gq * shi;
    }
    // F: the kept rows, thread t over the rows t, t + T, ..., then the butterfly, then the waves in order
    double acc = 0.0;
    unsigned int nk = 0u;
    sfi_sweep(kp, L, [&](double v) {
        if (v > cut) { acc = acc + v; nk++; }
    });
    acc = wave_allreduce(acc);
    if (lane == 0) s_wave[wave] = acc;
    if (nk) atomicAdd(&s_cnt[2], nk);
    __syncthreads();
    if (tid == 0) {
        double F = s_wave[0];
        for (int w = 1; w < kSfiCutWaves; w++) F = F + s_wave[w];
        rec->F = F;
        rec->cut = cut;
        rec->nrows = (int32_t)nrows; rec->nkept = (int32_t)s_cnt[2]; rec->nbad = 0;
    }
}

// ---- the column pass at an accepted point: partial sums of g and h over the kept genes of a slice
// A slice is as long as a wave is wide: lane l looks at gene i0 + l once (its flag, its L against the cut, its dispersion if
// it is kept), the ballot of the kept lanes drives the loop over the genes -- a wave-uniform skip --, and the loads of four
// genes are issued before the first of them is used.  The sums themselves run in gene order.
static_assert(kSfIterSliceGenes == 64, "sfi_col_kernel: one lane per gene of a slice");
__global__ void __launch_bounds__(256) sfi_col_kernel(SfIterateKernelParams kp, const double *L, const double *e, const SfiRecord *rec,
                                                      double *part) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = kp.m;
    const long tiles = ((long)m + 63) / 64, slices = ((long)kp.n + kSfIterSliceGenes - 1) / kSfIterSliceGenes;
    const double cut = rec->cut;
    for (long item = (long)blockIdx.x * 4 + wave; item < tiles * slices; item += (long)gridDim.x * 4) {
        const long slice = item / tiles;
        const int j = (int)(item % tiles) * 64 + lane;
        const bool valid = j < m;
        const double sfj = valid ? kp.sf[j] : 1.0, ej = valid ? e[j] : 1.0;
        const int i0 = (int)(slice * kSfIterSliceGenes);
        const int il = i0 + lane;
        bool keep = false;
        double al = 0.0;
        if (il < kp.n && kp.rows[il] != 0 && L[il] > cut) {
            keep = true;
            al = kp.disp[il];                          // (the dispersion of a row that is not kept is not read)
        }
        const unsigned long long mask = __ballot(keep);
        double g = 0.0, h = 0.0;
        for (int k0 = 0; k0 < 64; k0 += 4) {
            const unsigned int bits = (unsigned int)(mask >> k0) & 15u;         // (wave-uniform)
            if (!bits) continue;
            double kv[4], mv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                kv[u] = mv[u] = 0.0;
                if (((bits >> u) & 1u) && valid) {
                    const size_t at = (size_t)(i0 + k0 + u) * kp.ld + j;
                    kv[u] = (double)kp.y[at];
                    mv[u] = kp.mu[at];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (!((bits >> u) & 1u)) continue;
                const double a = lane_read(al, k0 + u);
                const double k = kv[u];
                const double mu = (mv[u] / sfj) * ej;
                const double opm = 1.0 + a * mu;
                g = g + (k - mu) / opm;
                h = h + (mu * (1.0 + a * k)) / (opm * opm);
            }
        }
        if (valid) {
            part[(slice * 2 + 0) * m + j] = g;
            part[(slice * 2 + 1) * m + j] = h;
        }
    }
}

// ---- g_j and h_j: the slices' partial sums in slice order from 0.0.  One workgroup per tile of 64 samples, its first wave on
// g, its second on h; sixteen loads are in flight before the first is added.
__global__ void __launch_bounds__(128) sfi_colsum_kernel(SfIterateKernelParams kp, const double *part, double *g, double *h) {
    const int c = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int m = kp.m;
    if (j >= m) return;
    const long slices = ((long)kp.n + kSfIterSliceGenes - 1) / kSfIterSliceGenes;
    const size_t stride = (size_t)2 * m;
    const double *p = part + (size_t)c * m + j;
    double acc = 0.0;
    long b = 0;
    for (; b + 16 <= slices; b += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = p[(size_t)(b + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; u++) acc = acc + v[u];
    }
    for (; b < slices; b++) acc = acc + p[(size_t)b * stride];
    (c ? h : g)[j] = acc;
}

// ---- lambda, d and g.d (serial sums in sample order)
__global__ void __launch_bounds__(kSfiVecThreads) sfi_step_kernel(SfIterateKernelParams kp, SfiState w) {
    __shared__ double stage[kSfiVecThreads + 1];
    const int m = kp.m;
    const double a = sfi_serial_sum(m, stage, [&](int j) { return w.g[j] / w.h[j]; });
    const double b = sfi_serial_sum(m, stage, [&](int j) { return 1.0 / w.h[j]; });
    const double lambda = a / b;
    for (int j = threadIdx.x; j < m; j += kSfiVecThreads) w.d[j] = (w.g[j] - lambda) / w.h[j];
    const double gd = sfi_serial_sum(m, stage, [&](int j) { return w.g[j] * w.d[j]; });
    if (threadIdx.x == 0) w.rec->gd = gd;
}

__global__ void __launch_bounds__(kSfiVecThreads) sfi_finish_kernel(SfIterateKernelParams kp, const double *s, const double *e, double F,
                                                                    int iter, int evals, int flag) {
    for (int j = threadIdx.x; j < kp.m; j += kSfiVecThreads) { kp.s_out[j] = s[j]; kp.sf_out[j] = e[j]; }
    if (threadIdx.x == 0) { *kp.F_out = F; *kp.iter_out = iter; *kp.evals_out = evals; *kp.flag_out = flag; }
}

static size_t sfi_slices(long n) { return (size_t)((n + kSfIterSliceGenes - 1) / kSfIterSliceGenes); }

size_t sf_iterate_workspace_bytes(long n, long m) {
    // K' (n) | L, twice (2 n) | partial column sums (slices x 2 x m) | s, e twice and d, g, h (7 m) | the record
    return ((size_t)n * 3 + sfi_slices(n) * 2 * (size_t)m + (size_t)m * 7) * sizeof(double) + 64;
}

#define SFI_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t launch_sf_iterate(const SfIterateKernelParams &kp, void *workspace, hipStream_t st) {
    const size_t n = kp.n, m = kp.m;
    SfiState w;
    double *p = (double *)workspace;
    w.kconst = p;   p += n;
    w.L[0] = p;     p += n;
    w.L[1] = p;     p += n;
    w.part = p;     p += sfi_slices(kp.n) * 2 * m;
    w.s[0] = p;     p += m;
    w.s[1] = p;     p += m;
    w.e[0] = p;     p += m;
    w.e[1] = p;     p += m;
    w.d = p;        p += m;
    w.g = p;        p += m;
    w.h = p;        p += m;
    w.rec = (SfiRecord *)p;
    const int cus = device_cu_count();
    int rblocks = (kp.n + 3) / 4;
    if (rblocks > 4 * cus) rblocks = 4 * cus;
    const long items = (long)sfi_slices(kp.n) * (((long)kp.m + 63) / 64);
    int cblocks = (int)((items + 3) / 4 < 8L * cus ? (items + 3) / 4 : 8L * cus);
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] sf_iterate n=%d m=%d: row blocks %d, column blocks %d, slice %d genes\n", kp.n, kp.m, rblocks, cblocks,
                kSfIterSliceGenes);
    SfiRecord hr;
    // L and the record at point `which`; the one synchronisation of an evaluation
    const auto eval = [&](int which, bool consts) -> hipError_t {
        if (consts) hipLaunchKernelGGL(sfi_row_kernel<true>, dim3(rblocks), dim3(256), 0, st, kp, w.kconst, w.e[which], w.L[which]);
        else hipLaunchKernelGGL(sfi_row_kernel<false>, dim3(rblocks), dim3(256), 0, st, kp, w.kconst, w.e[which], w.L[which]);
        hipLaunchKernelGGL(sfi_cut_kernel, dim3(1), dim3(kSfiCutThreads), 0, st, kp, w.L[which], w.rec);
        SFI_TRY(hipGetLastError());
        SFI_TRY(hipMemcpyAsync(&hr, w.rec, sizeof hr, hipMemcpyDeviceToHost, st));
        return hipStreamSynchronize(st);
    };
    hipLaunchKernelGGL(sfi_prep_kernel, dim3(1), dim3(kSfiVecThreads), 0, st, kp, w.s[0], w.e[0]);
    SFI_TRY(eval(0, true));
    int cur = 0, iter = 0, evals = 1, flag;
    double F = hr.F;
    if (!std::isfinite(F)) flag = 2;
    else if (hr.nkept == 0) flag = 0;
    else
        for (;;) {
            if (iter >= kp.maxit) { flag = 1; break; }
            iter++;
            hipLaunchKernelGGL(sfi_col_kernel, dim3(cblocks), dim3(256), 0, st, kp, w.L[cur], w.e[cur], w.rec, w.part);
            hipLaunchKernelGGL(sfi_colsum_kernel, dim3((kp.m + 63) / 64), dim3(128), 0, st, kp, w.part, w.g, w.h);
            hipLaunchKernelGGL(sfi_step_kernel, dim3(1), dim3(kSfiVecThreads), 0, st, kp, w);
            bool accepted = false;
            double t = 1.0, Ft = F, gd = 0.0;
            for (int trial = 0; trial < kSfiMaxTrials; trial++, t = 0.5 * t) {
                hipLaunchKernelGGL(sfi_trial_kernel, dim3(1), dim3(kSfiVecThreads), 0, st, kp.m, w.s[cur], w.d, t, w.s[1 - cur],
                                   w.e[1 - cur]);
                SFI_TRY(eval(1 - cur, false));
                evals++;
                gd = hr.gd;
                Ft = hr.F;
                const double slope = (kSfiArmijo * t) * gd;
                if (Ft >= F + slope) { accepted = true; break; }
            }
            if (!accepted) { flag = gd <= kSfiRelTol * std::fabs(F) ? 0 : 1; break; }
            const double gain = Ft - F;
            F = Ft;
            cur = 1 - cur;
            if (gain <= kSfiRelTol * std::fabs(F)) { flag = 0; break; }
        }
    hipLaunchKernelGGL(sfi_finish_kernel, dim3(1), dim3(kSfiVecThreads), 0, st, kp, w.s[cur], w.e[cur], F, iter, evals, flag);
    SFI_TRY(hipGetLastError());
    return hipStreamSynchronize(st);
}

}  // namespace dsq
