// contrasts.hip -- K contrasts of the fitted coefficients from ONE covariance pass per gene.
//
// getContrast (R/results.R:760-827) re-enters fitBeta with maxit = 0 once per contrast: every call rebuilds the fitted
// means, X'WX, its ridge inverse and Sigma = Gi G Gi (src/DESeq2.cpp:430-455) for ONE pair (c' beta, sqrt(c' Sigma c)).
// Here Sigma is built once per gene and every contrast is evaluated against it.
//
// ONE ROLLED KERNEL: p and K are run-time values, the p x p matrices of a gene live in LDS (G, then Sigma in its place; the
// LU factors, then T = Gi G in their place; Gi).  A workgroup is four waves; a gene is worked on by wpg = 1, 2 or 4 of
// them (launch: by the design width and by what fits the LDS), so a workgroup holds 4, 2 or 1 genes.  The waves of a gene
// split what is independent -- the samples of the elementwise pass, the Gram sums, the rows of an elimination step and of
// the two products, the contrasts -- and meet at workgroup barriers (every wave of the workgroup walks the same loops: p, K
// and the number of genes per workgroup are uniform).  Contrasts: a wave takes 64 / p of them at a time, a lane per
// (contrast, column of Sigma), and loops over the rest: K has no cap.
//
// THE ARITHMETIC IS THAT OF THE POST-LOOP BLOCK OF fitBeta AT maxit = 0 (src/DESeq2.cpp:430-455 as the kernels of
// fit_beta.hip / fit_beta_wide.hip evaluate it, DESIGN.md sections 2 and 4.2), operation by operation:
//   cell path     (design cells given, at most DSQ_CMAX of them, p <= DSQ_SPEC_BETA_CELL_MAXP -- the designs dsq_fit_beta_dev
//                 fits on cells): mu_j = max(nf_j exp(eta_c), minmu), w_j = mu_j ([wts_j] / (1 + alpha mu_j)), S_c = the
//                 wave-order sum of w over the positions of the cell-sorted sample sequence, G_ab = sum_c (x_ca x_cb) S_c
//                 serially from 0;
//   general path  mu_j = max(nf_j exp(x_j beta), minmu), w_j = ([wts_j] mu_j) / (1 + alpha mu_j), G_ab = the wave-order sum
//                 of x_ja (x_jb w_j);
//   both          LU with partial pivoting (first maximum wins, reciprocal pivots, fma(-l, u, a)), the inverse by p solves,
//                 T = Gi G and Sigma = T Gi with acc = fma(a_ik, b_kj, acc), k ascending, num = the chain fma(c_a, beta_a, .),
//                 den = sqrt of the chain fma(r_b, c_b, .) over r_b = the chain fma(c_a, Sigma_ab, .).
// A wave-order sum is taken by ONE wave (64 per-lane partials over the trips in order, then the xor butterfly of
// dsq_wave.hpp); which wave takes it does not enter the result.  The Gram loops and the LU live inside the kernels of
// fit_beta.hip / fit_beta_wide.hip and cannot be called from here; what IS shared are the butterflies, the lane exchanges
// and the math library.  The call's checks and its device-pointer body are in capi.hip, the host entry in capi_host.hip.
#include "dsq_internal.hpp"
#include <cstdio>
#include <cstdlib>
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

constexpr int kCtWaves = 4;                  // waves per workgroup
constexpr int kCtThreads = 64 * kCtWaves;
constexpr int kCtChunk = 8;                  // Gram sums reduced together (wave_allreduce_many: the bits of one butterfly each)
constexpr size_t kCtCuLds = 160 * 1024;

// LDS of a workgroup (doubles): lambda (p) and, on the cell path, the design rows of the cells (ncell x p) once; per gene
// G, LU / T, Gi (p x p each), beta, rdiag (p each), a row of 64 per wave of the gene, the cell sums (DSQ_CMAX) or the m
// weights, the pivots (p ints)
__host__ __device__ static inline size_t ct_shared_doubles(int p, int ncell) { return (size_t)p + (size_t)ncell * p; }
__host__ __device__ static inline size_t ct_gene_doubles(int p, int m, bool cell, int wpg) {
    return (size_t)3 * p * p + 2 * (size_t)p + (size_t)64 * wpg + (cell ? (size_t)DSQ_CMAX : (size_t)m) + (size_t)(p + 1) / 2;
}

// every count of the gene under the mask is 0 (wave-uniform; contrastAllZero*, R/results.R:1237-1270)
DSQ_DEV bool ct_all_zero(const int32_t *yg, const int32_t *mask, int m, int lane) {
    bool nz = false;
    for (int j = lane; j < m; j += 64) nz |= (mask[j] != 0) && (yg[j] != 0);
    return !__any(nz);
}

// G[a][b0 .. b0 + R - 1] = wave-order sums of x_ja (x_jb w_j), mirrored                                     [one wave]
template <int R>
DSQ_DEV void ct_gram_chunk(const double *xs, const double *w_s, double *G, int m, int P, int a, int b0, int lane) {
    double acc[R];
    _Pragma("unroll")
    for (int u = 0; u < R; u++) acc[u] = 0.0;
    const double *xa_p = xs + (size_t)a * m, *xb_p = xs + (size_t)b0 * m;
    for (int j = lane; j < m; j += 64) {
        const double wv = w_s[j], xa = xa_p[j];
        _Pragma("unroll")
        for (int u = 0; u < R; u++) acc[u] += xa * (xb_p[(size_t)u * m + j] * wv);
    }
    wave_allreduce_many(acc, lane);
    if (lane == 0) {
        _Pragma("unroll")
        for (int u = 0; u < R; u++) { G[(size_t)a * P + b0 + u] = acc[u]; G[(size_t)(b0 + u) * P + a] = acc[u]; }
    }
}

template <bool USE_W, bool CELL>
__global__ void __launch_bounds__(kCtThreads) contrasts_kernel(ContrastsKernelParams kp, int wpg, int gene_doubles) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = kp.p, m = kp.m, K = kp.K, C = CELL ? kp.ncell : 0;
    const int gpw = kCtWaves / wpg;                       // genes per workgroup
    const int slot = wave / wpg, sw = wave - slot * wpg;  // the gene of this wave, and the wave's place among the gene's waves
    const int GT = 64 * wpg, gt = sw * 64 + lane;         // threads of a gene
    double *lambda = smem, *xc = smem + P;
    double *mine = smem + ct_shared_doubles(P, C) + (size_t)slot * gene_doubles;
    double *G = mine, *A = mine + (size_t)P * P, *Gi = mine + 2 * (size_t)P * P;
    double *Sg = G, *Tm = A;                              // (G is dead once T = Gi G exists, the LU factors once Gi does)
    double *beta = mine + 3 * (size_t)P * P, *rdiag = beta + P, *rr = rdiag + P + 64 * sw, *samp = rdiag + P + 64 * wpg;
    int *piv = reinterpret_cast<int *>(samp + (CELL ? DSQ_CMAX : m));
    const double *xs = kp.x;
    const double log2e = 1.4426950408889634;             // log2(exp(1)), R/results.R:809-810

    for (int c = tid; c < P; c += kCtThreads) lambda[c] = kp.lambda[c];
    if constexpr (CELL) {
        for (int e = tid; e < C * P; e += kCtThreads) {
            const int c = e / P, a = e - c * P;
            xc[e] = xs[(size_t)a * m + kp.cell_perm[kp.cell_start[c]]];
        }
    }
    __syncthreads();

    for (long base = (long)blockIdx.x * gpw; base < kp.n; base += (long)gridDim.x * gpw) {
        const bool active = base + slot < kp.n;
        const int g = active ? (int)(base + slot) : kp.n - 1;
        const bool live = active && !(kp.allZero && kp.allZero[g] != 0);
        const double *nfg = kp.nf_is_vector ? kp.nf : kp.nf + (size_t)g * kp.ld;
        const double *wg = USE_W ? kp.weights + (size_t)g * kp.ld : nullptr;
        const int32_t *yg = kp.counts ? kp.counts + (size_t)g * kp.ld : nullptr;
        const double alpha = kp.alpha_hat[g];

        if (live) for (int c = gt; c < P; c += GT) beta[c] = kp.beta[(size_t)g + (size_t)kp.n * c];
        __syncthreads();

        // ---- weights and G = X'WX ----
        if constexpr (CELL) {
            if (live) {
                for (int c = sw; c < C; c += wpg) {
                    double eta = xc[c * P] * beta[0];
                    for (int k = 1; k < P; k++) eta = __builtin_fma(xc[c * P + k], beta[k], eta);
                    const double ex = dexp(eta);
                    const int s0 = kp.cell_start[c], s1 = kp.cell_start[c + 1];
                    double acc = 0.0;
                    for (int k = s0 + ((lane - s0) & 63); k < s1; k += 64) {     // (partial l: the positions k = l mod 64)
                        const int j = kp.cell_perm[k];
                        const double mu = __builtin_fmax(nfg[j] * ex, kp.minmu);
                        const double rcp = 1.0 / (1.0 + alpha * mu);
                        double rw = rcp;
                        if constexpr (USE_W) rw = wg[j] * rcp;
                        acc += mu * rw;
                    }
                    acc = wave_allreduce(acc);
                    if (lane == 0) samp[c] = acc;
                }
            }
            __syncthreads();
            if (live) {
                for (int e = gt; e < P * P; e += GT) {
                    const int a = e / P, b = e - a * P;
                    if (b < a) continue;
                    double v = 0.0;
                    for (int c = 0; c < C; c++) v += (xc[c * P + a] * xc[c * P + b]) * samp[c];
                    G[a * P + b] = v; G[b * P + a] = v;
                }
            }
        } else {
            if (live) {
                for (int j = gt; j < m; j += GT) {
                    double eta = xs[j] * beta[0];
                    for (int c = 1; c < P; c++) eta = __builtin_fma(xs[(size_t)c * m + j], beta[c], eta);
                    const double mu = __builtin_fmax(nfg[j] * dexp(eta), kp.minmu);
                    double wv;
                    if constexpr (USE_W) wv = (wg[j] * mu) / (1.0 + alpha * mu);
                    else wv = mu / (1.0 + alpha * mu);
                    samp[j] = wv;
                }
            }
            __syncthreads();
            if (live) {
                int task = 0;
                for (int a = 0; a < P; a++) {
                    for (int b0 = a; b0 < P; b0 += kCtChunk) {
                        if (task++ % wpg != sw) continue;
                        const int r = P - b0;
                        if (r >= 8) ct_gram_chunk<8>(xs, samp, G, m, P, a, b0, lane);
                        else switch (r) {
                            case 1: ct_gram_chunk<1>(xs, samp, G, m, P, a, b0, lane); break;
                            case 2: ct_gram_chunk<2>(xs, samp, G, m, P, a, b0, lane); break;
                            case 3: ct_gram_chunk<3>(xs, samp, G, m, P, a, b0, lane); break;
                            case 4: ct_gram_chunk<4>(xs, samp, G, m, P, a, b0, lane); break;
                            case 5: ct_gram_chunk<5>(xs, samp, G, m, P, a, b0, lane); break;
                            case 6: ct_gram_chunk<6>(xs, samp, G, m, P, a, b0, lane); break;
                            default: ct_gram_chunk<7>(xs, samp, G, m, P, a, b0, lane); break;
                        }
                    }
                }
            }
        }
        __syncthreads();

        // ---- A = G + diag(lambda), LU with partial pivoting (lane j owns column j) ----
        if (live) {
            for (int e = gt; e < P * P; e += GT) {
                const int i = e / P, j = e - i * P;
                double v = G[e];
                if (i == j) v = v + lambda[i];
                A[e] = v;
            }
        }
        __syncthreads();
        for (int k = 0; k < P; k++) {
            if (live && sw == 0) {
                // "best = |a_kk|; a later row wins when its |a_ik| > best" with a row per lane: a NaN never wins from a later row
                // (key -1) and is never beaten in row k (key +inf); the first of equal maxima is the lowest set bit of the ballot
                double key = -2.0;
                if (lane >= k && lane < P) {
                    const double v = __builtin_fabs(A[(size_t)lane * P + k]);
                    key = (v != v) ? (lane == k ? __builtin_inf() : -1.0) : v;
                }
                double mx = key, xa, xb;
                mx = __builtin_fmax(mx, lane_xor1(mx));
                mx = __builtin_fmax(mx, lane_xor2(mx));
                mx = __builtin_fmax(mx, lane_xor4(mx));
                mx = __builtin_fmax(mx, lane_xor8(mx));
                lane_pair16(mx, xa, xb); mx = __builtin_fmax(xa, xb);
                lane_pair32(mx, xa, xb); mx = __builtin_fmax(xa, xb);
                const int pr = (int)__builtin_ctzll(__ballot(key == mx));
                if (lane == 0) piv[k] = pr;
                if (pr != k && lane < P) {
                    const double t = A[(size_t)k * P + lane];
                    A[(size_t)k * P + lane] = A[(size_t)pr * P + lane];
                    A[(size_t)pr * P + lane] = t;
                }
            }
            __syncthreads();
            if (live) {
                const double rinv = 1.0 / A[(size_t)k * P + k];
                if (gt == 0) rdiag[k] = rinv;
                const int lc = lane < P ? lane : P - 1;
                const double akj = A[(size_t)k * P + lc];
                for (int i = k + 1 + sw; i < P; i += wpg) {
                    const double lraw = A[(size_t)i * P + k], aij = A[(size_t)i * P + lc];    // (read before lane k's store)
                    const double l = lraw * rinv;
                    if (lane == k) A[(size_t)i * P + k] = l;
                    else if (lane > k && lane < P) A[(size_t)i * P + lane] = __builtin_fma(-l, akj, aij);
                }
            }
            __syncthreads();
        }

        // ---- Gi = the inverse, lane c owns right-hand side e_c (p solves) ----
        if (live && sw == 0 && lane < P) {
            const int c = lane;
            int pos = c;                                 // e_c under the row swaps: where its 1 ends
            for (int k = 0; k < P; k++) {
                const int pr = piv[k];
                pos = (pos == k) ? pr : ((pos == pr) ? k : pos);
            }
            for (int i = 0; i < P; i++) {
                double t = (i == pos) ? 1.0 : 0.0;
                for (int j = 0; j < i; j++) t = __builtin_fma(-A[(size_t)i * P + j], Gi[(size_t)j * P + c], t);
                Gi[(size_t)i * P + c] = t;
            }
            for (int i = P - 1; i >= 0; i--) {
                double t = Gi[(size_t)i * P + c];
                for (int j = i + 1; j < P; j++) t = __builtin_fma(-A[(size_t)i * P + j], Gi[(size_t)j * P + c], t);
                Gi[(size_t)i * P + c] = t * rdiag[i];
            }
        }
        __syncthreads();

        // ---- T = Gi G, Sigma = T Gi (lane j owns column j, the rows go round the gene's waves) ----
        if (live && lane < P) {
            for (int i = sw; i < P; i += wpg) {
                double acc = 0.0;
                for (int k = 0; k < P; k++) acc = __builtin_fma(Gi[(size_t)i * P + k], G[(size_t)k * P + lane], acc);
                Tm[(size_t)i * P + lane] = acc;
            }
        }
        __syncthreads();
        if (live && lane < P) {
            for (int i = sw; i < P; i += wpg) {
                double acc = 0.0;
                for (int k = 0; k < P; k++) acc = __builtin_fma(Tm[(size_t)i * P + k], Gi[(size_t)k * P + lane], acc);
                Sg[(size_t)i * P + lane] = acc;
            }
        }
        __syncthreads();

        // ---- the contrasts: 64 / p of them per wave and trip, lane (q, b) takes column b of Sigma for contrast q ----
        if (live) {
            const int cpw = 64 / P;
            const int q = lane / P, b = lane - q * P;
            for (int k0 = sw * cpw; k0 < K; k0 += wpg * cpw) {
                const int k = k0 + q;
                const bool has = q < cpw && k < K;
                const double *ck = kp.contrasts + (size_t)(has ? k : 0) * P;
                double r = 0.0;
                if (has) for (int a = 0; a < P; a++) r = __builtin_fma(ck[a], Sg[(size_t)a * P + b], r);
                rr[lane] = r;
                int zero = 0;                            // the all-zero rule, one wave-wide pass per contrast of the trip
                if (kp.sample_mask) {
                    for (int qq = 0; qq < cpw && k0 + qq < K; qq++) {
                        if (!kp.rule_applies[k0 + qq]) continue;
                        const bool z = ct_all_zero(yg, kp.sample_mask + (size_t)(k0 + qq) * m, m, lane);
                        if (qq == q && z) zero = 1;
                    }
                }
                wave_lds_sync();
                if (has && b == 0) {
                    double cd = 0.0, cn = 0.0;
                    for (int bb = 0; bb < P; bb++) cd = __builtin_fma(rr[q * P + bb], ck[bb], cd);
                    for (int c = 0; c < P; c++) cn = __builtin_fma(ck[c], beta[c], cn);
                    double lfc = log2e * cn;
                    const double se = log2e * __builtin_sqrt(cd);
                    double stat = lfc / se;
                    double pv = dpnorm_upper2(stat);
                    if (zero) { lfc = 0.0; stat = 0.0; pv = 1.0; }        // R/results.R:1021-1028: lfcSE keeps its value
                    const size_t o = (size_t)g + (size_t)kp.n * k;
                    kp.lfc[o] = lfc; kp.se[o] = se; kp.stat[o] = stat; kp.pvalue[o] = pv;
                    if (kp.flags) kp.flags[o] = zero;
                }
                wave_lds_sync();
            }
        } else if (active) {
            for (int k = gt; k < K; k += GT) {                            // buildDataFrameWithNARows (R/results.R:823-824)
                const size_t o = (size_t)g + (size_t)kp.n * k;
                kp.lfc[o] = dnan(); kp.se[o] = dnan(); kp.stat[o] = dnan(); kp.pvalue[o] = dnan();
                if (kp.flags) kp.flags[o] = 0;
            }
        }
        __syncthreads();
    }
}

// contrasts == nullptr: the flags alone, a wave per gene
__global__ void __launch_bounds__(kCtThreads) contrast_flags_kernel(ContrastsKernelParams kp) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * kCtWaves + (threadIdx.x >> 6);
    if (g >= kp.n) return;
    const bool live = !(kp.allZero && kp.allZero[g] != 0);
    const int32_t *yg = kp.counts + (size_t)g * kp.ld;
    for (int k = 0; k < kp.K; k++) {
        int zero = 0;
        if (live && kp.rule_applies[k]) zero = ct_all_zero(yg, kp.sample_mask + (size_t)k * kp.m, kp.m, lane) ? 1 : 0;
        if (lane == 0) kp.flags[(size_t)g + (size_t)kp.n * k] = zero;
    }
}

// ---- launch ---------------------------------------------------------------------------------------------------------
// waves per gene: one up to 16 columns, two up to 32, four beyond -- more when fewer genes' matrices fit the CU's LDS
static int ct_waves_per_gene(int p, int m, bool cell, int ncell) {
    int wpg = p <= 16 ? 1 : p <= 32 ? 2 : 4;
    for (; wpg <= kCtWaves; wpg *= 2) {
        const size_t b = (ct_shared_doubles(p, cell ? ncell : 0) + (kCtWaves / wpg) * ct_gene_doubles(p, m, cell, wpg)) * sizeof(double);
        if (b <= kCtCuLds) return wpg;
    }
    return 0;
}

int contrasts_max_m(int p) {
    if (p < 1 || p > DSQ_P_WIDE) return 0;
    const size_t fixed = (ct_shared_doubles(p, 0) + ct_gene_doubles(p, 0, false, kCtWaves)) * sizeof(double);
    return (int)((kCtCuLds - fixed) / sizeof(double));
}

hipError_t launch_contrasts(const ContrastsKernelParams &kp, hipStream_t st, bool *ok) {
    *ok = true;
    if (!kp.contrasts) {
        hipLaunchKernelGGL(contrast_flags_kernel, dim3((kp.n + kCtWaves - 1) / kCtWaves), dim3(kCtThreads), 0, st, kp);
        return hipGetLastError();
    }
    const bool cell = kp.ncell > 0;
    const int wpg = ct_waves_per_gene(kp.p, kp.m, cell, kp.ncell);
    if (wpg == 0) { *ok = false; return hipSuccess; }
    const int gpw = kCtWaves / wpg;
    const size_t gene_d = ct_gene_doubles(kp.p, kp.m, cell, wpg);
    const size_t lds = (ct_shared_doubles(kp.p, cell ? kp.ncell : 0) + gpw * gene_d) * sizeof(double);
    const void *fn = kp.useWeights ? (cell ? (const void *)contrasts_kernel<true, true> : (const void *)contrasts_kernel<true, false>)
                                   : (cell ? (const void *)contrasts_kernel<false, true> : (const void *)contrasts_kernel<false, false>);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCtCuLds);
        if (e != hipSuccess) return e;
    }
    int bpc = (int)(kCtCuLds / lds);                     // workgroups per CU: by the LDS, at most eight (32 waves)
    bpc = bpc < 1 ? 1 : (bpc > 8 ? 8 : bpc);
    const long need = ((long)kp.n + gpw - 1) / gpw, cap = (long)device_cu_count() * bpc;
    int grid = (int)(need < cap ? need : cap);
    if (grid < 1) grid = 1;
    if (getenv("DSQ_VERBOSE"))
        fprintf(stderr, "[dsq] contrasts p=%d m=%d K=%d: %s path, %d waves per gene, lds=%zu, grid %d\n", kp.p, kp.m, kp.K,
                cell ? "cell" : "per-sample", wpg, lds, grid);
    ContrastsKernelParams q = kp;
    int wpg_a = wpg, gene_a = (int)gene_d;
    void *args[] = {&q, &wpg_a, &gene_a};
    return hipLaunchKernel(fn, dim3(grid), dim3(kCtThreads), args, lds, st);
}

}  // namespace dsq
