"""The specification of the local-regression dispersion trend (fitType = "local"), in numpy, one
evaluation point at a time.  csrc/local_fit.hip and deseq2_amd/local_fit_host.py equal it bit for bit.

What it states is the estimator behind locfit(logDisps ~ logMeans, weights = means) with locfit's documented defaults --
nearest-neighbour fraction 0.7, local quadratic, tricube kernel, Gaussian family, prior weights multiplying the kernel
weights -- evaluated directly at every requested mean (locfit's ev = dat()).  locfit itself evaluates on the vertices of an
adaptive tree and interpolates: agreement with its interpolated values is not claimed.

`fns.unary("log" / "exp", v)` is the library's pinned arithmetic (csrc/dsq_math.hpp; the CPU checker restates it).  Every
other operation is one IEEE double operation, in the order written.

  fit set      rows with 10 minDisp <= disps < Inf and 0 < means < Inf (R: disps >= 10 minDisp; a mean or a dispersion that
               has no finite logarithm is left out, where locfit would stop), N of them; x = log(means), y = log(disps),
               w = means, sorted by x, stable (ties by row).  N = 0: the trend is the constant minDisp (R returns the
               vector rep(minDisp, length(disps)) there, which cannot be called: the constant function is the deviation).
  bandwidth    k = floor(7 N / 10) (0.7 N in integers); k < 3 raises.
  window       z = log(q); l = the smallest start in [0, N - k] at which x[l + k] - z < z - x[l] no longer holds (bisection:
               the condition falls from true to false along l); h = max(z - x[l], x[l + k - 1] - z), the k-th smallest
               |x_j - z|.
  weights      t_j = (x_j - z) / h, a = |t_j|; for a < 1: W_j = w_j * (u * u * u), u = 1 - (a * a) * a.  A point with
               a >= 1 (the window edge, a NaN t when h = 0) adds nothing.
  terms        c0 = W, c1 = c0 * t, c2 = c1 * t, c3 = c2 * t, c4 = c3 * t; g0 = c0 * y, g1 = c1 * y, g2 = c2 * y.
  sums         S_r = sum c_r, T_r = sum g_r over j = l .. l + k - 1 in THE order: LANES = 64 partial sums, partial
               (j mod LANES) takes its points in ascending j from +0.0, then the partials are added pairwise -- partial i
               with partial i xor 1, then xor 2, 4, 8, 16, 32 (a butterfly: dsq_wave.hpp wave_allreduce).  The order is a
               function of (l, k) and LANES alone; dsq_local_fit_lanes() exports LANES.
  solve        the intercept of the 3 x 3 normal equations by elimination without pivoting, pivots S0, then the two Schur
               complements (solve3 below, in the order written).
  singular     fewer than three distinct x among the points with W > 0, or a pivot that is not > 0: NaN.
  value        exp(a0).  q that is NaN, <= 0 or Inf gives NaN.
"""
import numpy as np

LANES = 64
TOO_FEW = "local dispersion fit: fewer than 3 points in a window"


def bandwidth(N):
    return (7 * int(N)) // 10


def fit_set(fns, means, disps, minDisp):
    """(x, y, w) of the fit set in sorted order, and the rows they came from"""
    means, disps = np.asarray(means, np.float64), np.asarray(disps, np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.flatnonzero((disps >= 10 * minDisp) & (disps < np.inf) & (means > 0) & (means < np.inf))
    x = fns.unary("log", means[keep])
    o = np.argsort(x, kind="stable")
    rows = keep[o]
    return x[o], fns.unary("log", disps[rows]), means[rows].copy(), rows


def window_start(x, k, z):
    lo, hi = 0, x.size - k
    while lo < hi:
        mid = (lo + hi) // 2
        if x[mid + k] - z < z - x[mid]:
            lo = mid + 1
        else:
            hi = mid
    return lo


def bandwidth_h(x, k, z, l):
    return max(z - x[l], x[l + k - 1] - z)


def butterfly(part):
    """the pairwise sum of LANES partials (last axis), every lane's view of it: entry 0 is the total"""
    lanes = np.arange(LANES)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[..., lanes ^ off]
    return part[..., 0]


def moments(x, y, w, k, z):
    """(S0..S4, T0..T2), the number of distinct x with positive weight, (l, h)"""
    l = window_start(x, k, z)
    h = bandwidth_h(x, k, z, l)
    part = np.zeros((8, LANES))
    distinct = 0
    with np.errstate(all="ignore"):
        for j in range(l, l + k):
            t = (x[j] - z) / h
            a = abs(t)
            if not a < 1:
                continue
            u = 1 - (a * a) * a
            c0 = w[j] * ((u * u) * u)
            c1 = c0 * t
            c2 = c1 * t
            c3 = c2 * t
            c4 = c3 * t
            lane = j % LANES
            for r, v in enumerate((c0, c1, c2, c3, c4, c0 * y[j], c1 * y[j], c2 * y[j])):
                part[r, lane] = part[r, lane] + v
            if c0 > 0 and (j == l or x[j] != x[j - 1]):
                distinct += 1
        return butterfly(part), distinct, (l, h)


def solve3(S, T):
    """the intercept a0, or NaN when a pivot is not > 0"""
    S0, S1, S2, S3, S4 = (np.float64(v) for v in S)
    T0, T1, T2 = (np.float64(v) for v in T)
    with np.errstate(all="ignore"):
        if not S0 > 0:
            return np.nan
        m1 = S1 / S0
        m2 = S2 / S0
        A11 = S2 - m1 * S1
        A12 = S3 - m1 * S2
        A22 = S4 - m2 * S2
        b1 = T1 - m1 * T0
        b2 = T2 - m2 * T0
        if not A11 > 0:
            return np.nan
        m3 = A12 / A11
        p2 = A22 - m3 * A12
        c2 = b2 - m3 * b1
        if not p2 > 0:
            return np.nan
        a2 = c2 / p2
        a1 = (b1 - A12 * a2) / A11
        return ((T0 - S1 * a1) - S2 * a2) / S0


def _exp(fns, v):
    """sf_exp of csrc/dsq_math.hpp: NaN and +Inf stay, exp(-Inf) = 0"""
    if np.isnan(v) or v == np.inf:
        return v
    if v == -np.inf:
        return 0.0
    return float(fns.unary("exp", np.array([v]))[0])


def evaluate(fns, fit, q):
    """dispFit at the means q, and the number of singular points (a q with a logarithm whose value is NaN)"""
    x, y, w, k, minDisp = fit
    q = np.atleast_1d(np.asarray(q, np.float64))
    if x.size == 0:
        return np.full(q.shape, minDisp), 0
    out = np.full(q.shape, np.nan)
    with np.errstate(invalid="ignore"):
        ok = np.flatnonzero((q > 0) & (q < np.inf))
    zs = fns.unary("log", q[ok])
    for i, z in zip(ok, zs):
        m, distinct, _ = moments(x, y, w, k, z)
        a0 = solve3(m[:5], m[5:]) if distinct >= 3 else np.nan
        out[i] = _exp(fns, a0)
    return out, int(np.isnan(out[ok]).sum())


def local_fit(fns, means, disps, minDisp=1e-8):
    """the fit: (x, y, w, k, minDisp), for evaluate(); raises when a window would hold fewer than 3 points"""
    x, y, w, _ = fit_set(fns, means, disps, minDisp)
    k = bandwidth(x.size)
    if x.size and k < 3:
        raise RuntimeError(TOO_FEW)
    return x, y, w, k, float(minDisp)
