// dsq_select.hpp -- exact order statistics of n doubles by radix selection over their order_key images (dsq_math.hpp), by
// the 1024 threads of one workgroup or by several cooperating workgroups of one launch, and the grid barrier those meet at.
// Users: prior_var_kernel (one or sixteen workgroups) and trend_mean_kernel of trend.hip, sfi_cut_kernel of sf_iterate.hip.
#pragma once
#include "dsq_math.hpp"

namespace dsq {

// ---- the grid barrier ------------------------------------------------------------------------------------------------
// The sixteen-workgroup kernels of trend.hip meet at a hand-rolled spin barrier: the last workgroup to arrive resets the
// count and advances the generation the others poll.  It relies on three things, stated here once:
//   * the workgroups of the launch are CO-RESIDENT -- a plain launch checks nothing, a workgroup that waits for one that
//     has not started waits for ever: kTrendBlocks x 1024 threads, 16 workgroups on a 256-CU device, each kernel within
//     the registers and LDS of one workgroup per CU;
//   * the words are ZERO when the kernel starts: the workspace (all of TrendWs / SelWs) is zeroed by the call's init fill
//     (launch_init_fills; launch_trend_fit and launch_trend_fit_dev: by their own memset), and a barrier leaves count = 0;
//   * EVERY workgroup of the launch comes to every barrier: the decisions in front of one are taken from values all
//     workgroups read alike (the block sums, the merged histogram, the merged counts).
struct GridSync {
    unsigned int count, gen;
    unsigned int pad[14];
};

DSQ_DEV void grid_barrier(GridSync *s, unsigned nblocks) {
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned g = __hip_atomic_load(&s->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        unsigned arrived = atomicAdd(&s->count, 1u);
        if (arrived == nblocks - 1u) {
            atomicExch(&s->count, 0u);
            __threadfence();
            atomicAdd(&s->gen, 1u);
        } else {
            while (__hip_atomic_load(&s->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g) __builtin_amdgcn_s_sleep(2);
        }
        __threadfence();
    }
    __syncthreads();
}

// ---- exact order statistics by radix selection ------------------------------------------------------------------------
// on the order-preserving 64-bit image of the doubles (order_key, dsq_math.hpp), by BLOCKS cooperating workgroups of one
// launch: 1, or kTrendBlocks.  With several, each workgroup histograms its slice, the histograms meet in a global table
// (one per pass, zero at the launch), a grid barrier, and every workgroup scans the table itself -- so all of them take
// the same decisions.  A selected order statistic is exact, so the medians equal numpy's whatever BLOCKS is.
static constexpr int kSelDirect = 1024;       // = hist[2048] reinterpreted as 64-bit keys

struct SelWs {                           // of a launch with BLOCKS > 1: all zero at its start
    GridSync sync;
    unsigned long long cnt[8];           // [slot]: the values <= a median's lower middle; [7]: the residuals kept
    unsigned long long inv_min[8];       // ~key of the smallest value above a median's lower middle (atomicMax; zero = none)
    unsigned int ghist[16][2048];        // one table per radix pass of the launch (two medians of at most six passes)
    // (r6) the early exit of a selection: the candidates left after a pass, gathered by all workgroups (one list and one fill
    // counter per selection: a launch makes two)
    unsigned long long gfill[2];
    unsigned long long glist[2][1024];
};

struct SelState {                        // what the selections of one kernel share
    unsigned *hist;                      // LDS, 2048 words
    unsigned long long *bc;              // LDS, 3 broadcast words
    SelWs *ws;                           // BLOCKS > 1 only ...
    int pass;                            // ... the radix passes made so far: each takes the next table of ws->ghist
};

// the bin of hist[0 .. nb) that holds rank `rank` (0-based; the last bin if the counts end before it): one wave scans the
// bins, 64 at a time.  -> the bin; `rank` becomes the rank inside it, `left` the bin's count
DSQ_DEV unsigned digit_scan(const unsigned *hist, unsigned nb, long &rank, unsigned &left, unsigned long long *bc) {
    if (threadIdx.x < 64) {
        long r = rank;
        int found = -1;
        unsigned inbin = 0;
        for (unsigned b0 = 0; b0 < nb && found < 0; b0 += 64) {
            const unsigned h = hist[b0 + threadIdx.x];
            unsigned incl = h;                              // inclusive prefix over the 64 lanes
            for (int o = 1; o < 64; o <<= 1) {
                unsigned v = __shfl_up(incl, o, 64);
                if ((int)threadIdx.x >= o) incl += v;
            }
            const unsigned tot = __shfl(incl, 63, 64);
            if (r < (long)tot) {
                const unsigned long long m = __ballot((long)incl > r);
                const int l = __ffsll((long long)m) - 1;
                const unsigned before = __shfl(incl, l, 64) - __shfl(h, l, 64);
                found = (int)b0 + l;
                inbin = __shfl(h, l, 64);
                r -= (long)before;
            } else {
                r -= (long)tot;
            }
        }
        if (threadIdx.x == 0) { bc[0] = (unsigned long long)(found < 0 ? (int)nb - 1 : found); bc[1] = (unsigned long long)r; bc[2] = found < 0 ? 0ull : inbin; }
    }
    __syncthreads();
    const unsigned digit = (unsigned)bc[0];
    rank = (long)bc[1];
    left = (unsigned)bc[2];
    __syncthreads();
    return digit;
}

// the rank-th smallest (0-based) of the <= kSelDirect keys in `keys` (LDS), by counting: thread t takes key t and counts the
// keys that sort before it (smaller, or equal with a smaller index); exactly one thread finds `rank` and publishes its key
DSQ_DEV uint64_t rank_direct(const unsigned long long *keys, int cnt, long rank, unsigned long long *bc) {
    for (int t = threadIdx.x; t < cnt; t += blockDim.x) {
        const uint64_t mine = keys[t];
        int before = 0;
        for (int j = 0; j < cnt; j++) {
            const uint64_t o = keys[j];
            before += (o < mine || (o == mine && j < t)) ? 1 : 0;
        }
        if (before == (int)rank) bc[0] = mine;
    }
    __syncthreads();
    const uint64_t r = bc[0];
    __syncthreads();
    return r;
}

template <int BLOCKS, class F>
DSQ_DEV double radix_select(int n, long rank, F &&value, SelState &S, int slot) {
    // the rank-th smallest (0-based) of value(i), i < n; every thread returns it.  Digits of 11, 11, 11, 11, 11, 9 bits.
    // (r6) Once the candidates left (the keys that share the digits chosen so far) fit the histogram's LDS -- after two
    // passes, usually: the first 22 bits of a double leave a handful of 50 000 residuals -- they are gathered there and the
    // order statistic is taken by direct counting: three passes over the values instead of six, the same (exact) result.
    unsigned *hist = S.hist;
    unsigned long long *bc = S.bc;
    uint64_t prefix = 0, mask = 0;
    int shift = 64;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)blockDim.x * BLOCKS;
    while (shift > 0) {
        const int bits = shift >= 11 + 9 ? 11 : shift;         // 64 = 5 x 11 + 9
        shift -= bits;
        const unsigned nb = 1u << bits;
        for (unsigned b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = 0;
        __syncthreads();
        // (round 4 measured two variants of this pass -- the atomics of lanes that hit the same bin merged by ballot, the
        //  leading digits of log residuals being few; eight loads in flight per thread -- at 0.41 and 0.25 ms for the
        //  kernel against 0.24: neither the LDS atomics nor the L2 round trips are what one workgroup spends its time on)
        for (long i = first; i < n; i += stride) {
            const uint64_t k = order_key(value((int)i));
            if ((k & mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & (nb - 1u)], 1u);
        }
        __syncthreads();
        if constexpr (BLOCKS > 1) {                            // the workgroups' histograms, merged: every one reads the sum
            unsigned *gh = S.ws->ghist[S.pass++];
            for (unsigned b = threadIdx.x; b < nb; b += blockDim.x) { const unsigned h = hist[b]; if (h) atomicAdd(&gh[b], h); }
            grid_barrier(&S.ws->sync, BLOCKS);
            for (unsigned b = threadIdx.x; b < nb; b += blockDim.x) hist[b] = __hip_atomic_load(&gh[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
        }
        unsigned left;
        prefix |= (uint64_t)digit_scan(hist, nb, rank, left, bc) << shift;
        mask |= (uint64_t)(nb - 1u) << shift;
        if (shift > 0 && left > 0 && left <= (unsigned)kSelDirect) {
            // the candidates go to one list: in LDS, or -- every workgroup appending its own, a grid barrier, then each workgroup
            // taking the whole list -- in the launch's workspace (the same decision in every workgroup: `left` comes from the
            // merged histogram)
            unsigned long long *keys = reinterpret_cast<unsigned long long *>(hist);
            unsigned long long *fill = &bc[2], *list = keys;
            if constexpr (BLOCKS > 1) {
                fill = &S.ws->gfill[slot]; list = S.ws->glist[slot];
            } else {
                if (threadIdx.x == 0) bc[2] = 0ull;
                __syncthreads();
            }
            for (long i = first; i < n; i += stride) {
                const uint64_t k = order_key(value((int)i));
                if ((k & mask) == prefix) list[atomicAdd(fill, 1ull)] = k;
            }
            if constexpr (BLOCKS > 1) {
                grid_barrier(&S.ws->sync, BLOCKS);
                for (unsigned t = threadIdx.x; t < left; t += blockDim.x)
                    keys[t] = __hip_atomic_load(&list[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            return order_unkey(rank_direct(keys, (int)left, rank, bc));
        }
    }
    return order_unkey(prefix);
}

// the order statistic of 0-based rank r + 1, given the one of rank r, `a`: a itself when at least r + 2 values are <= a (a
// tie), else the smallest value above a; every thread returns it.  (Values that take no part are +inf: they sort last.)
template <int BLOCKS, class F>
DSQ_DEV double next_order_stat(int n, double a, long r, F &&value, SelState &S, int slot) {
    // the values <= a are counted and the smallest one above a kept (as the largest ~key: zero = none) where all threads
    // meet: in LDS, or in the launch's zeroed workspace
    unsigned long long *cnt = &S.bc[0], *imin = &S.bc[1];
    if constexpr (BLOCKS > 1) {
        cnt = &S.ws->cnt[slot]; imin = &S.ws->inv_min[slot];
    } else {
        if (threadIdx.x == 0) { *cnt = 0ull; *imin = 0ull; }
        __syncthreads();
    }
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)blockDim.x * BLOCKS;
    unsigned long long le = 0, inv = 0;
    for (long i = first; i < n; i += stride) {
        const double v = value((int)i);
        if (v <= a) le++;
        else { const unsigned long long kv = ~order_key(v); if (kv > inv) inv = kv; }
    }
    if (le) atomicAdd(cnt, le);
    if (inv) atomicMax(imin, inv);
    if constexpr (BLOCKS > 1) grid_barrier(&S.ws->sync, BLOCKS);
    else __syncthreads();
    const unsigned long long tot = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long iv = __hip_atomic_load(imin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return ((long)tot > r + 1) ? a : order_unkey(~iv);
}

template <int BLOCKS, class F>
DSQ_DEV double median(int n, long k, F &&value, SelState &S, int slot) {
    // numpy.median of the k finite values (invalid entries are +inf and sort last): the lower middle order statistic
    // by selection; for an even count the next one is either the same value (a tie) or the smallest value above it
    const double a = radix_select<BLOCKS>(n, (k - 1) / 2, value, S, slot);
    if (k & 1) return a;
    const double b = next_order_stat<BLOCKS>(n, a, (k - 1) / 2, value, S, slot);
    return (a + b) * 0.5;
}

}  // namespace dsq
