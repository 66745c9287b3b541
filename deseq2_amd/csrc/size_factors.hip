// size_factors.hip -- estimateSizeFactors on the device.
//
// estimateSizeFactorsForMatrix (R/core.R:535-578): sf_j = exp(median over {i : loggeomeans_i finite, k_ij > 0} of
// (log k_ij - loggeomeans_i)).  Two shapes of work:
//   - per GENE (loggeomeans, the normalization-factor rows): one wavefront per gene over its coalesced row, the
//     row sum of logs in wave order (64 partials + butterfly) like every other sum over samples;
//   - per SAMPLE, across the gene-major layout: the median is an exact order statistic, found by radix selection
//     over order-preserving 64-bit keys of d_ij = log k_ij - loggeomeans_i, 8 passes of 8 bits, no sort.  A pass:
//     a workgroup owns a slab of genes and a tile of 64 samples, lane = sample (row reads stay coalesced), and counts
//     the digit of every key that still carries the sample's prefix into hist[digit][lane] in LDS (64 KiB; a lane
//     only ever touches its own column, so the bank is the lane: no conflicts inside a wave; the four waves of the
//     workgroup share the table through LDS integer adds); the slab's histogram is added to the
//     256 x m global table with integer atomics (any order of integer adds gives the same table), and a small
//     per-sample kernel picks the digit that holds the wanted rank.
// The median of an even count needs ranks c/2 - 1 and c/2.  Both follow ONE prefix as long as they share a digit; the
// pass in which they part, the upper one is by construction the SMALLEST key of the next non-empty digit: the
// following pass takes that minimum beside its histogram (a register per lane, one 64-bit atomicMin per lane and
// workgroup), so the second rank costs neither a second table nor a second sweep.
// d_ij is recomputed in every pass (4 n m bytes of counts per pass) rather than stored as keys (8 n m written once,
// 8 n m read per pass, and an n x m workspace).
#include "dsq_internal.hpp"
#include "dsq_math.hpp"
#include "dsq_wave.hpp"

namespace dsq {

template <typename T>
DSQ_DEV double sf_count(const SizeFactorKernelParams &kp, long i, long j) {
    return (double)((const T *)kp.y)[i * kp.y_si + j * kp.y_sj];
}
// the matrix whose size factors are wanted: counts, or counts / normMatrix (R/core.R:2160)
template <typename T>
DSQ_DEV double sf_value(const SizeFactorKernelParams &kp, long i, long j) {
    double v = sf_count<T>(kp, i, j);
    if (kp.nm) v = v / kp.nm[i * kp.nm_si + j * kp.nm_sj];
    return v;
}

// ---- 1. loggeomeans: one wave per gene --------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) sf_loggeomeans_kernel(SizeFactorKernelParams kp) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwave = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + wave; i < kp.n; i += nwave) {
        double lgm;
        if (kp.type == 1) {
            // poscounts (R/methods.R:377-382, on the counts themselves): exp(sum(log(x[x > 0])) / length(x)), 0 for an all-zero row
            double s = 0.0, pos = 0.0;
            for (int j = lane; j < kp.m; j += 64) {
                const double k = sf_count<T>(kp, i, j);
                if (k > 0.0) { s += sf_log(k); pos = 1.0; }
            }
            s = wave_allreduce(s);
            pos = wave_allreduce(pos);
            lgm = pos > 0.0 ? sf_log(sf_exp(s / (double)kp.m)) : -kInf;
        } else if (kp.geoMeans) {
            lgm = sf_log(kp.geoMeans[i]);
        } else {
            double s = 0.0;
            for (int j = lane; j < kp.m; j += 64) s += sf_log(sf_value<T>(kp, i, j));
            s = wave_allreduce(s);
            lgm = s / (double)kp.m;
        }
        if (lane == 0) {
            kp.lgm[i] = lgm;
            if (kp.lgm_out) kp.lgm_out[i] = lgm;
            if (!(__builtin_fabs(lgm) == kInf)) atomicOr(kp.any_not_inf, 1);      // all(is.infinite(loggeomeans)), R/core.R:557
        }
    }
}

// ---- 2. one pass of the radix selection ---------------------------------------------------------------------------
// grid (sample tiles, gene slabs); pass 0 .. 7 looks at bits [56 - 8 pass, 64 - 8 pass) of the keys
template <typename T>
__global__ void __launch_bounds__(256) sf_hist_kernel(SizeFactorKernelParams kp, int pass) {
    __shared__ unsigned int hist[256 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int b = threadIdx.x; b < 256 * 64; b += 256) hist[b] = 0u;
    __syncthreads();
    const long j = (long)blockIdx.x * 64 + lane;
    const bool valid = j < kp.m;
    const int shift = 56 - 8 * pass;
    unsigned long long prefix = 0ull, hiprefix = 0ull, himin = ~0ull;
    int hishift = 0;
    bool live = valid, hi_pending = false;
    if (valid && pass > 0) {
        live = kp.cnt[j] != 0u;
        prefix = kp.prefix[j];
        hi_pending = kp.histate[j] == 1u;
        hiprefix = kp.hiprefix[j];
        hishift = (int)kp.hishift[j];
    }
    const long per = (kp.n + gridDim.y - 1) / gridDim.y;
    const long lo = (long)blockIdx.y * per;
    const long hi = lo + per < kp.n ? lo + per : kp.n;
    for (long i = lo + wave; i < hi; i += 4) {
        const double lgm = kp.lgm[i];
        if (!dfinite(lgm) || (kp.control && kp.control[i] == 0)) continue;      // (wave-uniform)
        if (!live) continue;
        const double v = sf_value<T>(kp, i, j);
        if (!(v > 0.0)) continue;
        const unsigned long long key = order_key(sf_log(v) - lgm);
        if (pass == 0 || ((key ^ prefix) >> (shift + 8)) == 0ull)
            atomicAdd(&hist[(unsigned)((key >> shift) & 255ull) * 64u + lane], 1u);
        if (hi_pending && ((key ^ hiprefix) >> hishift) == 0ull && key < himin) himin = key;
    }
    __syncthreads();
    // (thread t reads hist[t + 256 r]: lane t & 63 of digit (t >> 6) + 4 r, so a wave adds to 64 consecutive table entries)
    const long jf = (long)blockIdx.x * 64 + lane;
    for (int b = threadIdx.x; b < 256 * 64; b += 256) {
        const unsigned int c = hist[b];
        if (c != 0u && jf < kp.m) atomicAdd(&kp.hist[(long)(b >> 6) * kp.m + jf], c);
    }
    if (hi_pending && himin != ~0ull) atomicMin(&kp.hikey[j], himin);
}

// ---- 3. per sample: the digit that holds the wanted rank ----------------------------------------------------------
__global__ void __launch_bounds__(256) sf_select_kernel(SizeFactorKernelParams kp, int pass) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= kp.m) return;
    const int shift = 56 - 8 * pass;
    unsigned int c, rank;
    if (pass == 0) {
        c = 0u;
        for (int d = 0; d < 256; d++) c += kp.hist[(long)d * kp.m + j];
        kp.cnt[j] = c;
        rank = c ? (c - 1u) / 2u : 0u;
    } else {
        c = kp.cnt[j];
        rank = kp.rank[j];
    }
    if (c == 0u) {
        for (int d = 0; d < 256; d++) kp.hist[(long)d * kp.m + j] = 0u;
        return;
    }
    unsigned int hs = kp.histate[j];
    if (hs == 1u) hs = 2u;          // the pass that just ran took the minimum of the upper rank's digit: hikey is final
    unsigned int cum = 0u, fcum = 0u, fh = 0u;
    int found = -1, next = -1;
    for (int d = 0; d < 256; d++) {
        const unsigned int h = kp.hist[(long)d * kp.m + j];
        kp.hist[(long)d * kp.m + j] = 0u;                   // (the table of the next pass)
        if (found < 0) {
            if (rank < cum + h) { found = d; fcum = cum; fh = h; }
            else cum += h;
        } else if (next < 0 && h > 0u) next = d;
    }
    const unsigned long long old = pass == 0 ? 0ull : kp.prefix[j];
    kp.prefix[j] = old | ((unsigned long long)(unsigned)found << shift);
    rank -= fcum;
    kp.rank[j] = rank;
    if (hs == 0u && (c & 1u) == 0u && rank + 1u >= fh) {
        // the two middle ranks part here: the upper one is the smallest key of digit `next` under the old prefix
        const unsigned long long hp = old | ((unsigned long long)(unsigned)next << shift);
        if (shift == 0) { kp.hikey[j] = hp; hs = 2u; }
        else { kp.hiprefix[j] = hp; kp.hishift[j] = (unsigned)shift; kp.hikey[j] = ~0ull; hs = 1u; }
    }
    kp.histate[j] = hs;
}

// ---- 4. keys -> size factors --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) sf_finish_kernel(SizeFactorKernelParams kp) {
    __shared__ double gshared;
    for (int j = threadIdx.x; j < kp.m; j += blockDim.x) {
        const unsigned int c = kp.cnt[j];
        double sf;
        if (c == 0u) sf = dnan();                                          // median(numeric(0)) is NA
        else {
            const double a = order_unkey(kp.prefix[j]);
            double med = a;
            if ((c & 1u) == 0u) {
                const double b = kp.histate[j] == 2u ? order_unkey(kp.hikey[j]) : a;
                med = (a + b) * 0.5;
            }
            sf = sf_exp(med);
        }
        kp.sf[j] = sf;
        if (kp.stabilize) kp.logsf[j] = sf_log(sf);
    }
    if (threadIdx.x == 0) *kp.status = *kp.any_not_inf ? 0 : 1;
    if (!kp.stabilize) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;                                                    // mean(log(sf)): a serial sum in sample order
        for (int j = 0; j < kp.m; j++) s += kp.logsf[j];
        gshared = sf_exp(s / (double)kp.m);
    }
    __syncthreads();
    const double g = gshared;
    for (int j = threadIdx.x; j < kp.m; j += blockDim.x) kp.sf[j] = kp.sf[j] / g;      // R/core.R:575
}

// ---- 5. estimateNormFactors (R/core.R:2161-2162): one wave per gene -------------------------------------------------
__global__ void __launch_bounds__(256) sf_norm_factors_kernel(SizeFactorKernelParams kp) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwave = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + wave; i < kp.n; i += nwave) {
        double s = 0.0;
        for (int j = lane; j < kp.m; j += 64) s += sf_log(kp.nm[(long)i * kp.nm_si + j * kp.nm_sj] * kp.sf[j]);
        s = wave_allreduce(s);
        const double g = sf_exp(s / (double)kp.m);
        for (int j = lane; j < kp.m; j += 64)
            kp.nf_out[(long)i * kp.nm_si + j * kp.nm_sj] = (kp.nm[(long)i * kp.nm_si + j * kp.nm_sj] * kp.sf[j]) / g;
    }
}

size_t size_factors_workspace_bytes(long n, long m) {
    // loggeomeans (n f64) | log sf (m f64) | prefix, hikey, hiprefix (m u64 each) | histogram (256 m u32) |
    // cnt, rank, histate, hishift (m u32 each) | flag
    return (size_t)n * 8 + (size_t)m * (8 + 24 + 1024 + 16) + 64;
}

template <typename T>
static hipError_t launch_size_factors_t(SizeFactorKernelParams kp, hipStream_t st) {
    const int cu = device_cu_count();
    int gblocks = (kp.n + 3) / 4;
    if (gblocks > 8 * cu) gblocks = 8 * cu;
    hipLaunchKernelGGL(sf_loggeomeans_kernel<T>, dim3(gblocks), dim3(256), 0, st, kp);
    const int tiles = (kp.m + 63) / 64;
    // two workgroups of 64 KiB LDS fit a CU: about one round of them, and at least 64 genes each (a workgroup zeroes and
    // flushes 16 Ki histogram entries whatever its slab)
    int slabs = (2 * cu + tiles - 1) / tiles;
    const int most = (kp.n + 63) / 64;
    if (slabs > most) slabs = most;
    if (slabs < 1) slabs = 1;
    if (slabs > 65535) slabs = 65535;
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(sf_hist_kernel<T>, dim3(tiles, slabs), dim3(256), 0, st, kp, pass);
        hipLaunchKernelGGL(sf_select_kernel, dim3((kp.m + 255) / 256), dim3(256), 0, st, kp, pass);
    }
    hipLaunchKernelGGL(sf_finish_kernel, dim3(1), dim3(1024), 0, st, kp);
    if (kp.nf_out) hipLaunchKernelGGL(sf_norm_factors_kernel, dim3(gblocks), dim3(256), 0, st, kp);
    return hipGetLastError();
}

// carves the caller's workspace (size_factors_workspace_bytes), zeroes the selection state and enqueues the chain
hipError_t launch_size_factors(SizeFactorKernelParams kp, int y_f64, void *workspace, hipStream_t st) {
    const size_t n = kp.n, m = kp.m;
    char *w = (char *)workspace;
    kp.lgm = (double *)w;                    w += n * 8;
    kp.logsf = (double *)w;                  w += m * 8;
    char *state = w;
    kp.prefix = (unsigned long long *)w;     w += m * 8;
    kp.hikey = (unsigned long long *)w;      w += m * 8;
    kp.hiprefix = (unsigned long long *)w;   w += m * 8;
    kp.hist = (unsigned int *)w;             w += m * 1024;
    kp.cnt = (unsigned int *)w;              w += m * 4;
    kp.rank = (unsigned int *)w;             w += m * 4;
    kp.histate = (unsigned int *)w;          w += m * 4;
    kp.hishift = (unsigned int *)w;          w += m * 4;
    kp.any_not_inf = (int *)w;               w += 8;
    hipError_t e = hipMemsetAsync(state, 0, (size_t)(w - state), st);
    if (e != hipSuccess) return e;
    return y_f64 ? launch_size_factors_t<double>(kp, st) : launch_size_factors_t<int32_t>(kp, st);
}

}  // namespace dsq
