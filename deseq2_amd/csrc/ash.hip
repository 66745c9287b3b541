// ash.hip -- adaptive shrinkage on the device: ashr::ash(mixcompdist = "normal", method = "shrink") as lfcShrink(type = "ashr")
// calls it (R/lfcShrink.R:442-486), for C independent columns of (betahat, sebetahat).
//
// Per column: a scale mixture of zero-mean normals sum_k pi_k N(0, sigma_k^2) on ashr's sqrt(2) grid is fitted to the kept
// rows (b finite, s finite and positive) by maximum likelihood.  With l_ik = -log(2 pi (s_i^2 + sigma_k^2)) / 2
// - b_i^2 / (2 (s_i^2 + sigma_k^2)), lnorm_i = max_k l_ik and L_ik = exp(l_ik - lnorm_i), the weights minimise
//     phi(x) = -(1/n) sum_i log (L x)_i + sum_k x_k        over x >= 0
// (its minimiser sums to 1) by a sequential quadratic programme: at x one pass gives phi, g_k = 1 - (1/n) sum_i L_ik / u_i and
// H = (1/n) L' diag(1 / u^2) L + 1e-8 I; the host solves min d'Hd / 2 + g'd under x + d >= 0 by an active-set method on the
// K x K system and backtracks on the true phi (0.01, 0.75), all 32 step sizes of a search evaluated in one pass; it stops at
// min_k g_k >= -1e-8.  The iteration is stated once more in numpy (deseq2_amd/ash_host.py, tests/ash_spec.py) and equalled bit
// for bit here.  The ashr package's numbers, its optimiser and its treatment of excluded rows are unpinned.
//
// Kernels.  ash_range_kernel: one workgroup per column, the kept count and the two extrema the grid is made of (min s,
// max b^2 - s^2; exact whatever the order).  ash_like_kernel: one thread per row, the n x K block L and lnorm into the
// workspace, built once.  ash_eval_kernel: one workgroup per (slice of kAshSliceRows consecutive rows, column): u_i and
// z_i = L_i / u_i staged in LDS, then 4 x 4 register tiles of the upper triangle of z'z (with g on the diagonal tiles and
// sum log u on the first), one thread per (tile, group of kAshGroupRows rows); a group adds its rows in order from 0.0, the
// eight groups of a slice are added in order across eight neighbouring lanes.  ash_reduce_kernel adds the slices in order.
// ash_trial_kernel: phi's row sum at the 32 points max(x + 0.75^j d, 0) from one read of L.  ash_post_kernel: the posterior
// quantities of a row at the final weights, and loglik's partial sums.  f64 throughout, no floating-point atomics, no matrix
// cores (a matrix-core Gram would not keep the stated order).  A finished column's workgroups leave at once.
#include "capi.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dsq_math.hpp"

namespace dsq {

constexpr int kAshGroups = kAshSliceRows / kAshGroupRows;
constexpr int kAshRecPad = 2152;          // (K + 1)(K + 2) / 2 = 2145 doubles at K = 64, rounded up to a multiple of 8
constexpr double kAshStop = 1e-8, kAshRidge = 1e-8, kAshMultTol = 1e-12, kAshSuff = 0.01, kAshStepFactor = 0.75;
constexpr double kAshTwoPi = 0x1.921fb54442d18p+2;
constexpr double kAshSqrtHalf = 0x1.6a09e667f3bcdp-1;     // the double nearest sqrt(1/2), which lies above it
static_assert(kAshGroups == 8 && kAshSliceRows == 128 && kAshMaxK == 64 && kAshTrials == 32, "the kernels' index arithmetic");

// what the host tells the kernels about a column, uploaded in front of every launch that needs it
struct AshCol {
    double x[kAshMaxK];          // the point (the final weights for ash_post_kernel)
    double d[kAshMaxK];          // the direction of the line search
    double sg2[kAshMaxK];        // sigma_k^2
    double sigma[kAshMaxK];
    int32_t K, active, iter, flag;
};

// the call's state, carved from the caller's workspace: three record regions in front, then per column (stride colw doubles)
// L (n x K, K contiguous per row) | lnorm (n) | the slices' partial records | their partial trial sums | their partial loglik
struct AshWork {
    double *rec, *trec, *range;
    double *cols;
    size_t colw, o_lnorm, o_part, o_tpart, o_lpart;
    long recstride;
    int nsl;
};

static size_t ash_slices(long n) { return (size_t)((n + kAshSliceRows - 1) / kAshSliceRows); }
static size_t ash_colw(long n) { return (size_t)n * (kAshMaxK + 1) + ash_slices(n) * (kAshRecPad + kAshTrials + 1); }
size_t ash_workspace_bytes(long n, long C) {
    return ((size_t)C * (kAshRecPad + kAshTrials + 4) + (size_t)C * ash_colw(n)) * sizeof(double) + 64;
}

DSQ_DEV bool ash_kept(double b, double s) { return dfinite(b) && dfinite(s) && s > 0.0; }
DSQ_DEV int ash_rec_doubles(int K) { return (K + 1) * (K + 2) / 2; }

// ---- the kept count and the two extrema of a column
__global__ void __launch_bounds__(1024) ash_range_kernel(AshKernelParams kp, AshWork w) {
    __shared__ double s_mn[16], s_mx[16];
    __shared__ unsigned s_cnt[16];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double *b = kp.b + (size_t)c * kp.ld, *s = kp.s + (size_t)c * kp.ld;
    unsigned cnt = 0u;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (int i = tid; i < kp.n; i += 1024) {
        const double bi = b[i], si = s[i];
        if (!ash_kept(bi, si)) continue;
        cnt++;
        const double dd = bi * bi - si * si;
        mn = si < mn ? si : mn;
        mx = dd > mx ? dd : mx;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned oc = __shfl_xor(cnt, off);
        const double on = __shfl_xor(mn, off), ox = __shfl_xor(mx, off);
        cnt += oc;
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if ((tid & 63) == 0) { s_cnt[tid >> 6] = cnt; s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < 16; v++) {
            cnt += s_cnt[v];
            mn = s_mn[v] < mn ? s_mn[v] : mn;
            mx = s_mx[v] > mx ? s_mx[v] : mx;
        }
        w.range[c * 4 + 0] = (double)cnt;
        w.range[c * 4 + 1] = mn;
        w.range[c * 4 + 2] = mx;
    }
}

// ---- L and lnorm, once
__global__ void __launch_bounds__(256) ash_like_kernel(AshKernelParams kp, AshWork w, const AshCol *__restrict__ tab) {
    const int c = blockIdx.y;
    const AshCol &col = tab[c];
    const int K = col.K;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kp.n) return;
    double *base = w.cols + (size_t)c * w.colw;
    double *Lrow = base + (size_t)i * K;
    const double bi = kp.b[(size_t)c * kp.ld + i], si = kp.s[(size_t)c * kp.ld + i];
    if (!ash_kept(bi, si)) {
        for (int k = 0; k < K; k++) Lrow[k] = 0.0;
        base[w.o_lnorm + i] = 0.0;
        return;
    }
    const double s2 = si * si, bb = bi * bi;
    double m = 0.0;
    for (int k = 0; k < K; k++) {
        const double v = s2 + col.sg2[k];
        const double l = (-0.5 * sf_log(kAshTwoPi * v)) - (0.5 * ddiv_n(bb, v));
        m = k == 0 ? l : (l > m ? l : m);
    }
    for (int k = 0; k < K; k++) {
        const double v = s2 + col.sg2[k];
        const double l = (-0.5 * sf_log(kAshTwoPi * v)) - (0.5 * ddiv_n(bb, v));
        Lrow[k] = sf_exp(l - m);
    }
    base[w.o_lnorm + i] = m;
}

// ---- phi's row sum, g's and the upper triangle of H's, one slice
__global__ void __launch_bounds__(256) ash_eval_kernel(AshKernelParams kp, AshWork w, const AshCol *__restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) double ash_lds[];
    const int c = blockIdx.y;
    const AshCol &col = tab[c];
    if (!col.active) return;
    const int K = col.K, nt = (K + 3) >> 2, Kp = nt * 4;
    const int tid = threadIdx.x;
    double *z = ash_lds, *lu = ash_lds + (size_t)kAshSliceRows * Kp;
    const double *base = w.cols + (size_t)c * w.colw;
    const long r0 = (long)blockIdx.x * kAshSliceRows;
    if (tid < kAshSliceRows) {
        const long i = r0 + tid;
        double *zr = z + (size_t)tid * Kp;
        bool kept = false;
        if (i < kp.n) kept = ash_kept(kp.b[(size_t)c * kp.ld + i], kp.s[(size_t)c * kp.ld + i]);
        if (kept) {
            const double *Lrow = base + (size_t)i * K;
            double u = 0.0;
            for (int k = 0; k < K; k++) u = u + col.x[k] * Lrow[k];
            lu[tid] = sf_log(u);
            for (int k = 0; k < K; k++) zr[k] = Lrow[k] / u;
            for (int k = K; k < Kp; k++) zr[k] = 0.0;
        } else {
            lu[tid] = 0.0;
            for (int k = 0; k < Kp; k++) zr[k] = 0.0;
        }
    }
    __syncthreads();
    const int E = ash_rec_doubles(K);
    double *out = w.cols + (size_t)c * w.colw + w.o_part + (size_t)blockIdx.x * E;
    const int nitems = (nt * (nt + 1) / 2) * kAshGroups;
    for (int start = 0; start < nitems; start += 256) {
        const int item = start + tid;
        const bool valid = item < nitems;              // (nitems is a multiple of 8: eight neighbouring lanes agree)
        const int tile = item >> 3, grp = item & 7;
        int bk = 0, rest = tile;
        if (valid) while (rest >= nt - bk) { rest -= nt - bk; bk++; }
        const int bl = bk + rest;
        double h[16], gs[4], ph = 0.0;
#pragma unroll
        for (int q = 0; q < 16; q++) h[q] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) gs[q] = 0.0;
        if (valid) {
            for (int ii = 0; ii < kAshGroupRows; ii++) {
                const int row = grp * kAshGroupRows + ii;
                const double *zr = z + (size_t)row * Kp;
                double zk[4], zl[4];
#pragma unroll
                for (int q = 0; q < 4; q++) { zk[q] = zr[bk * 4 + q]; zl[q] = zr[bl * 4 + q]; }
#pragma unroll
                for (int a = 0; a < 4; a++)
#pragma unroll
                    for (int b = 0; b < 4; b++) h[a * 4 + b] = h[a * 4 + b] + zk[a] * zl[b];
                if (bk == bl) {
#pragma unroll
                    for (int q = 0; q < 4; q++) gs[q] = gs[q] + zk[q];
                }
                if (tile == 0) ph = ph + lu[row];
            }
        }
        // the eight groups of a slice, in order: lane 8 t takes its own partial sum, then those of lanes 8 t + 1 .. 8 t + 7
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const double own = h[q];
            double acc = own;
            for (int r = 1; r < kAshGroups; r++) acc = acc + __shfl_down(own, r, 8);
            h[q] = acc;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const double own = gs[q];
            double acc = own;
            for (int r = 1; r < kAshGroups; r++) acc = acc + __shfl_down(own, r, 8);
            gs[q] = acc;
        }
        {
            const double own = ph;
            double acc = own;
            for (int r = 1; r < kAshGroups; r++) acc = acc + __shfl_down(own, r, 8);
            ph = acc;
        }
        if (valid && grp == 0) {
            if (tile == 0) out[0] = ph;
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const int k = bk * 4 + a;
                if (k >= K) continue;
                if (bk == bl) out[1 + k] = gs[a];
                const int rowbase = 1 + K + k * K - k * (k - 1) / 2;      // the entry (k, k)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int l = bl * 4 + b;
                    if (l < K && l >= k) out[rowbase + (l - k)] = h[a * 4 + b];
                }
            }
        }
    }
}

// ---- the slices in order from 0.0.  what: 0 the evaluation's record, 1 the trial sums, 2 loglik
__global__ void __launch_bounds__(256) ash_reduce_kernel(AshKernelParams kp, AshWork w, const AshCol *__restrict__ tab, int what) {
    const int c = blockIdx.y;
    const AshCol &col = tab[c];
    if (!col.active) return;
    const int E = what == 0 ? ash_rec_doubles(col.K) : what == 1 ? kAshTrials : 1;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const double *base = w.cols + (size_t)c * w.colw;
    const double *src = base + (what == 0 ? w.o_part : what == 1 ? w.o_tpart : w.o_lpart) + e;
    double *dst = what == 0 ? w.rec + (size_t)c * w.recstride : what == 1 ? w.trec + (size_t)c * kAshTrials : kp.loglik + c;
    double acc = 0.0;
    int b = 0;
    for (; b + 8 <= w.nsl; b += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = src[(size_t)(b + q) * E];
#pragma unroll
        for (int q = 0; q < 8; q++) acc = acc + v[q];
    }
    for (; b < w.nsl; b++) acc = acc + src[(size_t)b * E];
    dst[e] = acc;
}

// ---- sum_i log (L x_j)_i at the 32 trial points x_j = max(x + 0.75^j d, 0), one slice
__global__ void __launch_bounds__(256) ash_trial_kernel(AshKernelParams kp, AshWork w, const AshCol *__restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) double ash_lds[];
    const int c = blockIdx.y;
    const AshCol &col = tab[c];
    if (!col.active) return;
    const int K = col.K, tid = threadIdx.x;
    double *xt = ash_lds;                                     // kAshTrials x kAshMaxK, later the groups' sums
    double *lus = ash_lds + kAshTrials * kAshMaxK;            // kAshTrials x kAshSliceRows
    for (int idx = tid; idx < kAshTrials * K; idx += 256) {
        const int j = idx / K, k = idx - j * K;
        double t = 1.0;
        for (int q = 0; q < j; q++) t = t * kAshStepFactor;
        const double v = col.x[k] + t * col.d[k];
        xt[j * kAshMaxK + k] = v > 0.0 ? v : 0.0;
    }
    __syncthreads();
    const int row = tid & (kAshSliceRows - 1), half = tid >> 7;
    const long i = (long)blockIdx.x * kAshSliceRows + row;
    bool kept = false;
    if (i < kp.n) kept = ash_kept(kp.b[(size_t)c * kp.ld + i], kp.s[(size_t)c * kp.ld + i]);
    double u[16];
#pragma unroll
    for (int q = 0; q < 16; q++) u[q] = 0.0;
    if (kept) {
        const double *Lrow = w.cols + (size_t)c * w.colw + (size_t)i * K;
        const double *xh = xt + (size_t)half * 16 * kAshMaxK;
        for (int k = 0; k < K; k++) {
            const double Lk = Lrow[k];
#pragma unroll
            for (int q = 0; q < 16; q++) u[q] = u[q] + xh[q * kAshMaxK + k] * Lk;
        }
    }
#pragma unroll
    for (int q = 0; q < 16; q++) lus[(half * 16 + q) * kAshSliceRows + row] = kept ? sf_log(u[q]) : 0.0;
    __syncthreads();
    {
        const int j = tid >> 3, g = tid & 7;
        double acc = 0.0;
        for (int ii = 0; ii < kAshGroupRows; ii++) acc = acc + lus[j * kAshSliceRows + g * kAshGroupRows + ii];
        xt[j * kAshGroups + g] = acc;
    }
    __syncthreads();
    if (tid < kAshTrials) {
        double acc = xt[tid * kAshGroups];
        for (int g = 1; g < kAshGroups; g++) acc = acc + xt[tid * kAshGroups + g];
        w.cols[(size_t)c * w.colw + w.o_tpart + (size_t)blockIdx.x * kAshTrials + tid] = acc;
    }
}

// ---- the posterior of a row at the final weights (col.x), and loglik's partial sum of the slice
__global__ void __launch_bounds__(kAshSliceRows) ash_post_kernel(AshKernelParams kp, AshWork w, const AshCol *__restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) double ash_lds[];
    const int c = blockIdx.y;
    const AshCol &col = tab[c];
    const int K = col.K, tid = threadIdx.x;
    const long i = (long)blockIdx.x * kAshSliceRows + tid;
    const double *base = w.cols + (size_t)c * w.colw;
    double ll = 0.0;
    if (i < kp.n) {
        const size_t at = (size_t)c * kp.ld + i;
        const double bi = kp.b[at], si = kp.s[at];
        double pm = dnan(), psd = pm, neg = pm, pos = pm, lf = pm, le = pm, gt = pm;
        if (ash_kept(bi, si)) {
            const double *Lrow = base + (size_t)i * K;
            double u = 0.0;
            for (int k = 0; k < K; k++) u = u + col.x[k] * Lrow[k];
            ll = sf_log(u) + base[w.o_lnorm + i];
            const double s2 = si * si;
            pm = 0.0;
            for (int k = 0; k < K; k++) {
                const double den = col.sg2[k] + s2;
                const double wk = (col.x[k] * Lrow[k]) / u;
                const double mk = ddiv_n(bi * col.sg2[k], den);
                pm = pm + wk * mk;
            }
            double var = 0.0;
            neg = 0.0; pos = 0.0;
            double les = 0.0, gts = 0.0;
            for (int k = 0; k < K; k++) {
                const double den = col.sg2[k] + s2;
                const double wk = (col.x[k] * Lrow[k]) / u;
                const double mk = ddiv_n(bi * col.sg2[k], den);
                const double vk = ddiv_n(col.sg2[k] * s2, den);
                const double dk = mk - pm;
                var = var + wk * (vk + dk * dk);
                const double sd = __builtin_sqrt(vk);
                double lo, up;
                dpnorm_both((-mk) / sd, lo, up);
                neg = neg + wk * lo;
                pos = pos + wk * up;
                if (kp.has_threshold) {
                    dpnorm_both((kp.threshold - mk) / sd, lo, up);
                    les = les + wk * lo;
                    dpnorm_both(((-kp.threshold) - mk) / sd, lo, up);
                    gts = gts + wk * up;
                }
            }
            psd = __builtin_sqrt(var);
            lf = neg < pos ? neg : pos;
            if (kp.has_threshold) { le = les; gt = gts; }
        }
        kp.pm[at] = pm; kp.psd[at] = psd; kp.neg[at] = neg; kp.pos[at] = pos; kp.lfsr[at] = lf; kp.le_t[at] = le; kp.gt_mt[at] = gt;
    }
    ash_lds[tid] = ll;
    __syncthreads();
    if (tid < kAshGroups) {
        double acc = 0.0;
        for (int ii = 0; ii < kAshGroupRows; ii++) acc = acc + ash_lds[tid * kAshGroupRows + ii];
        ash_lds[kAshSliceRows + tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = ash_lds[kAshSliceRows];
        for (int g = 1; g < kAshGroups; g++) acc = acc + ash_lds[kAshSliceRows + g];
        w.cols[(size_t)c * w.colw + w.o_lpart + blockIdx.x] = acc;
    }
}

__global__ void __launch_bounds__(64) ash_finish_kernel(AshKernelParams kp, const AshCol *__restrict__ tab) {
    const int c = blockIdx.x, t = threadIdx.x;
    const AshCol &col = tab[c];
    kp.pi[c * kAshMaxK + t] = t < col.K ? col.x[t] : 0.0;
    kp.sd[c * kAshMaxK + t] = t < col.K ? col.sigma[t] : 0.0;
    if (t == 0) { kp.K[c] = col.K; kp.iter[c] = col.iter; kp.flag[c] = col.flag; }
}

// ------------------------------------------------------------------------------------------------ the host's part
// ceil(2 log2 r) of a positive finite r, exactly: r = f 2^e, f in [0.5, 1)
static int ash_ceil_2log2(double r) {
    int e;
    const double f = std::frexp(r, &e);
    if (f == 0.5) return 2 * e - 2;
    return f < kAshSqrtHalf ? 2 * e - 1 : 2 * e;
}

// (A + ridge I) p = rhs by Cholesky, A F x F symmetric (row-major, stride F), overwritten; false when a pivot is not positive
// and finite.  Every element loses its products in ascending order of the column; forward substitution in ascending, backward
// in descending order.
static bool ash_cholesky_solve(std::vector<double> &A, std::vector<double> &y, int F, double ridge, std::vector<double> &Lf) {
    for (int t = 0; t < F; t++) A[(size_t)t * F + t] = A[(size_t)t * F + t] + ridge;
    Lf.assign((size_t)F * F, 0.0);
    for (int t = 0; t < F; t++) {
        const double piv = A[(size_t)t * F + t];
        if (!(piv > 0.0 && piv < INFINITY)) return false;
        const double r = std::sqrt(piv);
        Lf[(size_t)t * F + t] = r;
        for (int i = t + 1; i < F; i++) Lf[(size_t)i * F + t] = A[(size_t)i * F + t] / r;
        for (int i = t + 1; i < F; i++) {
            const double ci = Lf[(size_t)i * F + t];
            for (int j = t + 1; j <= i; j++) A[(size_t)i * F + j] = A[(size_t)i * F + j] - ci * Lf[(size_t)j * F + t];
        }
    }
    for (int t = 0; t < F; t++) {
        y[t] = y[t] / Lf[(size_t)t * F + t];
        for (int i = t + 1; i < F; i++) y[i] = y[i] - Lf[(size_t)i * F + t] * y[t];
    }
    for (int t = F - 1; t >= 0; t--) {
        y[t] = y[t] / Lf[(size_t)t * F + t];
        for (int i = 0; i < t; i++) y[i] = y[i] - Lf[(size_t)t * F + i] * y[t];
    }
    return true;
}

// d minimising d'Hd / 2 + g'd under x + d >= 0: the active-set method of DESIGN.md section 23 (ash_host.qp, line by line)
static void ash_qp(const double *H, const double *g, const double *x, int K, double *d) {
    static const double p10[13] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12};
    std::vector<double> y(x, x + K), q(K), A, rhs, Lf, A0;
    std::vector<char> work(K);
    std::vector<int> fr;
    for (int k = 0; k < K; k++) work[k] = !(x[k] > 0.0);
    double hmax = H[0];
    for (int k = 1; k < K; k++) hmax = H[(size_t)k * K + k] > hmax ? H[(size_t)k * K + k] : hmax;
    const auto gradient = [&]() {
        for (int k = 0; k < K; k++) q[k] = g[k];
        for (int l = 0; l < K; l++) {
            const double dl = y[l] - x[l];
            for (int k = 0; k < K; k++) q[k] = q[k] + H[(size_t)k * K + l] * dl;
        }
    };
    for (int round = 0; round < 4 * K + 8; round++) {
        gradient();
        fr.clear();
        for (int k = 0; k < K; k++) if (!work[k]) fr.push_back(k);
        const int F = (int)fr.size();
        bool blocked = false;
        if (F) {
            A0.resize((size_t)F * F);
            for (int a = 0; a < F; a++)
                for (int b = 0; b < F; b++) A0[(size_t)a * F + b] = H[(size_t)fr[a] * K + fr[b]];
            bool ok = false;
            for (int j = -1; j <= 12 && !ok; j++) {
                A = A0;
                rhs.resize(F);
                for (int a = 0; a < F; a++) rhs[a] = -q[fr[a]];
                ok = ash_cholesky_solve(A, rhs, F, j < 0 ? 0.0 : (kAshRidge * hmax) * p10[j], Lf);
            }
            if (!ok) break;
            double alpha = 1.0, amin = INFINITY;
            int blk = -1, at = -1;
            for (int a = 0; a < F; a++)
                if (rhs[a] < 0.0) {
                    const double ratio = y[fr[a]] / (-rhs[a]);
                    if (ratio < amin) { amin = ratio; at = a; }
                }
            if (at >= 0 && amin <= 1.0) { alpha = amin; blk = fr[at]; }
            for (int a = 0; a < F; a++) {
                const double yn = y[fr[a]] + alpha * rhs[a];
                y[fr[a]] = yn > 0.0 ? yn : 0.0;
            }
            if (blk >= 0) { y[blk] = 0.0; work[blk] = 1; blocked = true; }
        }
        if (blocked) continue;
        gradient();
        int kmin = -1;
        for (int k = 0; k < K; k++)
            if (work[k] && (kmin < 0 || q[k] < q[kmin])) kmin = k;
        if (kmin < 0 || !(q[kmin] < -kAshMultTol)) break;
        work[kmin] = 0;
    }
    for (int k = 0; k < K; k++) d[k] = y[k] - x[k];
}

struct AshHostCol {
    int K = 0, iter = 0, flag = 0;
    bool active = true;
    double nk = 0.0, phi = 0.0;
    std::vector<double> g, H, d;
};

#define ASH_HIP(expr) DSQ_HIP(expr)

int launch_ash(const AshKernelParams &kp, void *workspace, hipStream_t st) {
    const int C = kp.C;
    const size_t n = kp.n;
    AshWork w;
    double *p = (double *)workspace;
    w.rec = p;    p += (size_t)C * kAshRecPad;
    w.trec = p;   p += (size_t)C * kAshTrials;
    w.range = p;  p += (size_t)C * 4;
    w.cols = p;
    w.colw = ash_colw(kp.n);
    w.nsl = (int)ash_slices(kp.n);
    w.o_lnorm = n * kAshMaxK;
    w.o_part = w.o_lnorm + n;
    w.o_tpart = w.o_part + (size_t)w.nsl * kAshRecPad;
    w.o_lpart = w.o_tpart + (size_t)w.nsl * kAshTrials;
    w.recstride = kAshRecPad;

    // the range pass and the grids
    hipLaunchKernelGGL(ash_range_kernel, dim3(C), dim3(1024), 0, st, kp, w);
    ASH_HIP(hipGetLastError());
    std::vector<double> range((size_t)C * 4);
    ASH_HIP(hipMemcpyAsync(range.data(), w.range, range.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    ASH_HIP(hipStreamSynchronize(st));
    std::vector<AshCol> tab(C);
    std::vector<AshHostCol> hc(C);
    memset(tab.data(), 0, tab.size() * sizeof(AshCol));
    int Kmax = 0;
    for (int c = 0; c < C; c++) {
        const double nk = range[c * 4], smin_raw = range[c * 4 + 1], dmax = range[c * 4 + 2];
        if (!(nk >= 1.0))
            return capi_fail(DSQ_ERR_VALUE, "column %d: no row with a finite estimate and a finite, positive standard error", c);
        const double smin = smin_raw / 10.0;
        const double smax = dmax > 0.0 ? 2.0 * std::sqrt(dmax) : 8.0 * smin;
        const double r = smax / smin;
        if (!(r > 0.0 && r < INFINITY)) return capi_fail(DSQ_ERR_UNSUPPORTED, "column %d: the grid from %g to %g cannot be formed", c, smin, smax);
        int npoint = ash_ceil_2log2(r);
        if (npoint < 1) npoint = 1;
        if (npoint + 1 > kAshMaxK)
            return capi_fail(DSQ_ERR_UNSUPPORTED, "column %d: the grid needs %d components: at most %d", c, npoint + 1, kAshMaxK);
        const int K = npoint + 1;
        AshCol &t = tab[c];
        t.K = K; t.active = 1;
        for (int k = 0; k < K; k++) {
            const int back = npoint - k;
            t.sigma[k] = std::ldexp((back & 1) ? smax * kAshSqrtHalf : smax, -(back >> 1));
            t.sg2[k] = t.sigma[k] * t.sigma[k];
            t.x[k] = 1.0 / (double)K;
        }
        hc[c].K = K; hc[c].nk = nk;
        hc[c].g.resize(K); hc[c].H.resize((size_t)K * K); hc[c].d.assign(K, 0.0);
        Kmax = K > Kmax ? K : Kmax;
    }
    const int Emax = (Kmax + 1) * (Kmax + 2) / 2;
    w.recstride = Emax;
    const size_t eval_lds = ((size_t)kAshSliceRows * (((Kmax + 3) >> 2) * 4) + kAshSliceRows) * sizeof(double);
    const size_t trial_lds = ((size_t)kAshTrials * kAshMaxK + (size_t)kAshTrials * kAshSliceRows) * sizeof(double);
    if (eval_lds > 64 * 1024)
        ASH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ash_eval_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)eval_lds));
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] ash n=%d C=%d: %d slices of %d rows, K up to %d, evaluation LDS %zu bytes\n", kp.n, C, w.nsl, kAshSliceRows, Kmax,
                eval_lds);
    const AshCol *dtab = nullptr;
    const auto upload = [&]() -> int {
        void *v;
        if (int rc = capi_upload_table(WS_ASH_TABLE, tab.data(), tab.size() * sizeof(AshCol), st, &v)) return rc;
        dtab = (const AshCol *)v;
        return DSQ_OK;
    };
    std::vector<double> rec((size_t)C * Emax), trec((size_t)C * kAshTrials);
    // the record at the points tab[c].x of the active columns; one synchronisation
    const auto evaluate = [&]() -> int {
        if (int rc = upload()) return rc;
        hipLaunchKernelGGL(ash_eval_kernel, dim3(w.nsl, C), dim3(256), eval_lds, st, kp, w, dtab);
        hipLaunchKernelGGL(ash_reduce_kernel, dim3((Emax + 255) / 256, C), dim3(256), 0, st, kp, w, dtab, 0);
        ASH_HIP(hipGetLastError());
        ASH_HIP(hipMemcpyAsync(rec.data(), w.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        ASH_HIP(hipStreamSynchronize(st));
        for (int c = 0; c < C; c++) {
            AshHostCol &h = hc[c];
            if (!h.active) continue;
            const int K = h.K;
            const double *r = rec.data() + (size_t)c * Emax;
            double sx = 0.0;
            for (int k = 0; k < K; k++) sx = sx + tab[c].x[k];
            h.phi = (-(r[0] / h.nk)) + sx;
            for (int k = 0; k < K; k++) h.g[k] = 1.0 - r[1 + k] / h.nk;
            const double *tri = r + 1 + K;
            for (int k = 0; k < K; k++)
                for (int l = k; l < K; l++, tri++) h.H[(size_t)k * K + l] = h.H[(size_t)l * K + k] = *tri / h.nk;
            for (int k = 0; k < K; k++) h.H[(size_t)k * K + k] = h.H[(size_t)k * K + k] + kAshRidge;
        }
        return DSQ_OK;
    };
    if (int rc = upload()) return rc;
    hipLaunchKernelGGL(ash_like_kernel, dim3((kp.n + 255) / 256, C), dim3(256), 0, st, kp, w, dtab);
    if (int rc = evaluate()) return rc;
    double ts[kAshTrials];
    ts[0] = 1.0;
    for (int j = 1; j < kAshTrials; j++) ts[j] = ts[j - 1] * kAshStepFactor;
    for (;;) {
        // where each active column stands: converged, out of iterations, or one more quadratic programme
        int nactive = 0;
        for (int c = 0; c < C; c++) {
            AshHostCol &h = hc[c];
            if (!h.active) continue;
            double gmin = h.g[0];
            for (int k = 1; k < h.K; k++) gmin = h.g[k] < gmin ? h.g[k] : gmin;
            if (gmin >= -kAshStop) { h.flag = 0; h.active = false; }
            else if (h.iter >= kp.maxit) { h.flag = 1; h.active = false; }
            else {
                h.iter++;
                ash_qp(h.H.data(), h.g.data(), tab[c].x, h.K, h.d.data());
                for (int k = 0; k < h.K; k++) tab[c].d[k] = h.d[k];
                nactive++;
            }
            tab[c].active = h.active ? 1 : 0;
        }
        if (!nactive) break;
        // the line searches: phi at every step size from one pass; one synchronisation
        if (int rc = upload()) return rc;
        hipLaunchKernelGGL(ash_trial_kernel, dim3(w.nsl, C), dim3(256), trial_lds, st, kp, w, dtab);
        hipLaunchKernelGGL(ash_reduce_kernel, dim3(1, C), dim3(256), 0, st, kp, w, dtab, 1);
        ASH_HIP(hipGetLastError());
        ASH_HIP(hipMemcpyAsync(trec.data(), w.trec, trec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        ASH_HIP(hipStreamSynchronize(st));
        nactive = 0;
        for (int c = 0; c < C; c++) {
            AshHostCol &h = hc[c];
            if (!h.active) continue;
            const int K = h.K;
            double gd = 0.0, dmaxabs = 0.0;
            for (int k = 0; k < K; k++) {
                gd = gd + h.g[k] * h.d[k];
                dmaxabs = std::fabs(h.d[k]) > dmaxabs ? std::fabs(h.d[k]) : dmaxabs;
            }
            int take = -1;
            double xt[kAshMaxK];
            for (int j = 0; j < kAshTrials && take < 0 && dmaxabs > 0.0; j++) {
                double sx = 0.0;
                for (int k = 0; k < K; k++) {
                    const double v = tab[c].x[k] + ts[j] * h.d[k];
                    xt[k] = v > 0.0 ? v : 0.0;
                    sx = sx + xt[k];
                }
                const double cand = (-(trec[(size_t)c * kAshTrials + j] / h.nk)) + sx;
                if (cand <= h.phi + (kAshSuff * ts[j]) * gd) take = j;
            }
            if (take < 0) { h.flag = 2; h.active = false; tab[c].active = 0; continue; }
            for (int k = 0; k < K; k++) tab[c].x[k] = xt[k];
            nactive++;
        }
        if (!nactive) break;
        if (int rc = evaluate()) return rc;
    }
    // the posterior at pi = x / sum x, every column
    for (int c = 0; c < C; c++) {
        AshCol &t = tab[c];
        double sx = 0.0;
        for (int k = 0; k < t.K; k++) sx = sx + t.x[k];
        for (int k = 0; k < t.K; k++) t.x[k] = t.x[k] / sx;
        t.active = 1; t.iter = hc[c].iter; t.flag = hc[c].flag;
    }
    if (int rc = upload()) return rc;
    hipLaunchKernelGGL(ash_post_kernel, dim3(w.nsl, C), dim3(kAshSliceRows), (kAshSliceRows + kAshGroups) * sizeof(double), st, kp, w, dtab);
    hipLaunchKernelGGL(ash_reduce_kernel, dim3(1, C), dim3(256), 0, st, kp, w, dtab, 2);
    hipLaunchKernelGGL(ash_finish_kernel, dim3(C), dim3(64), 0, st, kp, dtab);
    ASH_HIP(hipGetLastError());
    ASH_HIP(hipStreamSynchronize(st));
    return DSQ_OK;
}

}  // namespace dsq
