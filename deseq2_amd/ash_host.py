"""Adaptive shrinkage (ashr::ash(mixcompdist = "normal", method = "shrink")) on the host: the operations of csrc/ash.hip and of
its host loop in numpy over an engine's exp / log, the same operations in the same order, so that
HostEngine.ash_fit and dsq_ash_dev agree to the bit -- grid, active-set solver and iteration counts included.

`un(name, v)` is the engine's unary arithmetic (exp, log).  +, -, *, / and sqrt are IEEE, every operation rounded once.
Every sum over the rows: the rows are taken in slices of SLICE_ROWS consecutive rows, a slice in GROUPS groups of GROUP_ROWS
consecutive rows; a group adds its rows in order from 0.0, a slice adds its groups in order starting from the first, the
slices are added in order from 0.0.  A row that is not kept enters every sum as 0.0."""
import numpy as np

from .results_host import pnorm_both

MAX_K = 64                         # DSQ_ASH_MAX_K
SLICE_ROWS, GROUP_ROWS = 128, 16   # dsq_ash_slice_rows()
GROUPS = SLICE_ROWS // GROUP_ROWS
TRIALS = 32                        # the step sizes 0.75^j, j = 0 .. 31, of one line search
SUFF_DECREASE, STEP_FACTOR = 0.01, 0.75
STOP = 1e-8                        # min_k g_k >= -STOP ends the iteration
RIDGE = 1e-8
MULT_TOL = 1e-12                   # a bound leaves the working set when its multiplier is below -MULT_TOL
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")       # the double nearest sqrt(1/2), which lies above it
FLAG_CONVERGED, FLAG_MAXIT, FLAG_NO_STEP = 0, 1, 2


class Unsupported(NotImplementedError):
    pass


def _log(un, v):
    """log with the edges spelled out (sf_log of csrc/dsq_math.hpp)"""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, np.nan)
    ok = (v > 0) & (v < np.inf)
    if ok.any():
        out[ok] = un("log", np.ascontiguousarray(v[ok]))
    out[v == 0] = -np.inf
    out[v == np.inf] = np.inf
    return out


def _exp(un, v):
    """exp with the edges spelled out (sf_exp of csrc/dsq_math.hpp)"""
    v = np.asarray(v, np.float64)
    out = np.array(v, dtype=np.float64, copy=True)
    ok = np.isfinite(v)
    if ok.any():
        out[ok] = un("exp", np.ascontiguousarray(v[ok]))
    out[v == -np.inf] = 0.0
    return out


def kept_rows(b, s):
    with np.errstate(invalid="ignore"):
        return np.isfinite(b) & np.isfinite(s) & (s > 0)


def row_range(b, s):
    """(kept count, min s, max (b b - s s)) over the kept rows; the extrema are exact whatever the order"""
    k = kept_rows(b, s)
    if not k.any():
        return 0, np.inf, -np.inf
    bk, sk = b[k], s[k]
    return int(k.sum()), float(sk.min()), float((bk * bk - sk * sk).max())


def ceil_2log2(r):
    """ceil(2 log2 r) of a positive finite r, exactly: r = f 2^e with f in [0.5, 1); 2 log2 f is -2 at f = 0.5, in (-2, -1] up
    to sqrt(1/2), in (-1, 0) beyond"""
    f, e = np.frexp(r)
    e = int(e)
    if f == 0.5:
        return 2 * e - 2
    return 2 * e - 1 if f < SQRT_HALF else 2 * e


def grid(smin_raw, dmax):
    """ashr's gridmult = sqrt(2) rule from the two extrema: the K = npoint + 1 standard deviations, ascending"""
    smin = smin_raw / 10.0
    smax = 2.0 * np.sqrt(dmax) if dmax > 0.0 else 8.0 * smin
    r = smax / smin
    if not (r > 0.0 and r < np.inf):
        raise Unsupported("ash: the grid from min(s) / 10 = %r to %r cannot be formed" % (smin, smax))
    npoint = max(ceil_2log2(r), 1)
    if npoint + 1 > MAX_K:
        raise Unsupported("ash: the grid needs %d components (at most %d are served)" % (npoint + 1, MAX_K))
    sigma = np.empty(npoint + 1)
    for k in range(npoint + 1):
        t = npoint - k
        sigma[k] = np.ldexp(smax * SQRT_HALF if t & 1 else smax, -(t >> 1))
    return sigma


def likelihood(un, b, s, sigma):
    """(L n x K, lnorm n, kept): rows that are not kept hold 0"""
    kept = kept_rows(b, s)
    n, K = b.size, sigma.size
    L, lnorm = np.zeros((n, K)), np.zeros(n)
    if kept.any():
        bk, sk = b[kept], s[kept]
        s2, bb = sk * sk, bk * bk
        sg2 = sigma * sigma
        v = s2[:, None] + sg2[None, :]
        l = (-0.5 * _log(un, TWO_PI * v)) - (0.5 * (bb[:, None] / v))
        m = l[:, 0].copy()
        for k in range(1, K):
            m = np.where(l[:, k] > m, l[:, k], m)
        L[kept] = _exp(un, l - m[:, None])
        lnorm[kept] = m
    return L, lnorm, kept


def slice_sum(T):
    """the sum down the rows of an (n, E) array in the order of the module docstring"""
    n, E = T.shape
    S = -(-n // SLICE_ROWS)
    pad = np.zeros((S * SLICE_ROWS, E))
    pad[:n] = T
    pad = pad.reshape(S, GROUPS, GROUP_ROWS, E)
    part = np.zeros((S, GROUPS, E))
    for j in range(GROUP_ROWS):
        part = part + pad[:, :, j, :]
    sl = part[:, 0, :]
    for g in range(1, GROUPS):
        sl = sl + part[:, g, :]
    total = np.zeros(E)
    for i in range(S):
        total = total + sl[i]
    return total


def mix(L, x):
    """u = L x, the components in order from 0.0"""
    u = np.zeros(L.shape[0])
    for k in range(L.shape[1]):
        u = u + x[k] * L[:, k]
    return u


def evaluate(un, L, kept, x, nk):
    """phi, g and H (full symmetric K x K) at x"""
    K = L.shape[1]
    with np.errstate(all="ignore"):
        u = mix(L, x)
        lu = np.where(kept, _log(un, np.where(kept, u, 1.0)), 0.0)
        z = np.where(kept[:, None], L / np.where(kept, u, 1.0)[:, None], 0.0)
        iu = np.triu_indices(K)
        sums = slice_sum(np.concatenate([lu[:, None], z, z[:, iu[0]] * z[:, iu[1]]], axis=1))
        sx = np.float64(0.0)
        for k in range(K):
            sx = sx + x[k]
        phi = (-(sums[0] / nk)) + sx
        g = 1.0 - sums[1:1 + K] / nk
        H = np.zeros((K, K))
        H[iu] = sums[1 + K:] / nk
        H = H + np.triu(H, 1).T
        H[np.arange(K), np.arange(K)] = H[np.arange(K), np.arange(K)] + RIDGE
    return phi, g, H


def step_sizes():
    t, out = np.float64(1.0), []
    for _ in range(TRIALS):
        out.append(t)
        t = t * STEP_FACTOR
    return np.array(out)


def trial_point(x, d, t):
    v = x + t * d
    return np.where(v > 0.0, v, 0.0)


def trial(un, L, kept, x, d, nk):
    """phi at the TRIALS points max(x + t_j d, 0)"""
    out = np.empty(TRIALS)
    cols = []
    sxs = []
    with np.errstate(all="ignore"):
        for t in step_sizes():
            xt = trial_point(x, d, t)
            u = mix(L, xt)
            cols.append(np.where(kept, _log(un, np.where(kept, u, 1.0)), 0.0))
            sx = np.float64(0.0)
            for k in range(x.size):
                sx = sx + xt[k]
            sxs.append(sx)
        sums = slice_sum(np.stack(cols, axis=1))
        for j in range(TRIALS):
            out[j] = (-(sums[j] / nk)) + sxs[j]
    return out


def cholesky_solve(A, rhs, ridge):
    """p with (A + ridge I) p = rhs by Cholesky; None when a pivot is not positive and finite.  Factor: column t, then the
    trailing columns lose the outer product of column t (so every element loses its products in ascending t).  Forward
    substitution in ascending, backward in descending order of the columns."""
    F = rhs.size
    A = A.copy()
    A[np.arange(F), np.arange(F)] = A[np.arange(F), np.arange(F)] + ridge
    Lf = np.zeros((F, F))
    with np.errstate(all="ignore"):
        for t in range(F):
            piv = A[t, t]
            if not (piv > 0.0 and piv < np.inf):
                return None
            r = np.sqrt(piv)
            Lf[t, t] = r
            col = A[t + 1:, t] / r
            Lf[t + 1:, t] = col
            A[t + 1:, t + 1:] = A[t + 1:, t + 1:] - col[:, None] * col[None, :]
        y = rhs.copy()
        for t in range(F):
            y[t] = y[t] / Lf[t, t]
            y[t + 1:] = y[t + 1:] - Lf[t + 1:, t] * y[t]
        for t in reversed(range(F)):
            y[t] = y[t] / Lf[t, t]
            y[:t] = y[:t] - Lf[t, :t] * y[t]
    return y


def qp(H, g, x):
    """d minimising d'Hd / 2 + g'd under x + d >= 0, by a primal active-set method on y = x + d:
    the working set starts as { k : x_k = 0 }; on the free set the Newton step of the quadratic (Cholesky; when a pivot
    fails, with a further ridge 1e-8 max_k H_kk 10^j, j = 0 .. 12); the longest feasible part of it is taken, the blocking
    bound (the lowest index among equals) joins the working set; after a full step the bound with the most negative
    multiplier (the lowest index among equals) below -MULT_TOL leaves it, and none such ends the solve.  At most 4 K + 8 rounds."""
    K = x.size
    y = x.copy()
    work = ~(x > 0.0)
    hmax = H[np.arange(K), np.arange(K)].max()
    with np.errstate(all="ignore"):
        for _ in range(4 * K + 8):
            dy = y - x
            q = g.copy()
            for l in range(K):
                q = q + H[:, l] * dy[l]
            free = np.flatnonzero(~work)
            blocked = False
            if free.size:
                A = H[np.ix_(free, free)]
                p = cholesky_solve(A, -q[free], 0.0)
                j = 0
                while p is None and j <= 12:
                    p = cholesky_solve(A, -q[free], (RIDGE * hmax) * 10.0 ** j)
                    j += 1
                if p is None:
                    break
                neg = p < 0.0
                alpha, blk = np.float64(1.0), -1
                if neg.any():
                    ratio = np.where(neg, y[free] / np.where(neg, -p, 1.0), np.inf)
                    a = ratio.min()
                    if a <= 1.0:
                        alpha, blk = a, int(free[int(np.argmin(ratio))])
                yn = y[free] + alpha * p
                y[free] = np.where(yn > 0.0, yn, 0.0)
                if blk >= 0:
                    y[blk] = 0.0
                    work[blk] = True
                    blocked = True
            if blocked:
                continue
            dy = y - x
            q = g.copy()
            for l in range(K):
                q = q + H[:, l] * dy[l]
            w = np.flatnonzero(work)
            if w.size == 0:
                break
            kmin = int(w[int(np.argmin(q[w]))])
            if not (q[kmin] < -MULT_TOL):
                break
            work[kmin] = False
    return y - x


def dot(a, b):
    s = np.float64(0.0)
    for k in range(a.size):
        s = s + a[k] * b[k]
    return s


def posterior(un, b, s, L, lnorm, kept, sigma, pi, threshold=None):
    """the per-row posterior quantities at the weights pi, and loglik"""
    n, K = L.shape
    vexp = lambda v: un("exp", v)
    names = ("PosteriorMean", "PosteriorSD", "NegativeProb", "PositiveProb", "lfsr", "le_T", "gt_mT")
    out = {k: np.full(n, np.nan) for k in names}
    with np.errstate(all="ignore"):
        u = mix(L, pi)
        ll = np.where(kept, _log(un, np.where(kept, u, 1.0)) + lnorm, 0.0)
        loglik = slice_sum(ll[:, None])[0]
        if kept.any():
            bk, sk, Lk, uk = b[kept], s[kept], L[kept], u[kept]
            s2 = sk * sk
            sg2 = sigma * sigma
            w, m, v = [], [], []
            for k in range(K):
                den = sg2[k] + s2
                w.append((pi[k] * Lk[:, k]) / uk)
                m.append((bk * sg2[k]) / den)
                v.append((sg2[k] * s2) / den)
            pm = np.zeros(bk.size)
            for k in range(K):
                pm = pm + w[k] * m[k]
            var, neg, pos, le, gt = (np.zeros(bk.size) for _ in range(5))
            for k in range(K):
                dk = m[k] - pm
                var = var + w[k] * (v[k] + dk * dk)
                sd = np.sqrt(v[k])
                lo, up = pnorm_both(vexp, (-m[k]) / sd)
                neg, pos = neg + w[k] * lo, pos + w[k] * up
                if threshold is not None:
                    le = le + w[k] * pnorm_both(vexp, (threshold - m[k]) / sd)[0]
                    gt = gt + w[k] * pnorm_both(vexp, ((-threshold) - m[k]) / sd)[1]
            out["PosteriorMean"][kept], out["PosteriorSD"][kept] = pm, np.sqrt(var)
            out["NegativeProb"][kept], out["PositiveProb"][kept] = neg, pos
            out["lfsr"][kept] = np.where(neg < pos, neg, pos)
            if threshold is not None:
                out["le_T"][kept], out["gt_mT"][kept] = le, gt
    return out, loglik


def fit_column(un, b, s, threshold=None, maxit=100):
    b, s = np.ascontiguousarray(b, np.float64), np.ascontiguousarray(s, np.float64)
    nk, smin_raw, dmax = row_range(b, s)
    if nk == 0:
        raise ValueError("ash: no row with a finite estimate and a finite, positive standard error")
    sigma = grid(smin_raw, dmax)
    K = sigma.size
    L, lnorm, kept = likelihood(un, b, s, sigma)
    nkf = np.float64(nk)
    x = np.full(K, 1.0 / K)
    ts = step_sizes()
    it = 0
    phi, g, H = evaluate(un, L, kept, x, nkf)
    while True:
        if g.min() >= -STOP:
            flag = FLAG_CONVERGED
            break
        if it >= maxit:
            flag = FLAG_MAXIT
            break
        it += 1
        d = qp(H, g, x)
        gd = dot(g, d)
        cand = trial(un, L, kept, x, d, nkf)
        moved = np.abs(d).max() > 0.0
        j = next((j for j in range(TRIALS) if moved and cand[j] <= phi + (SUFF_DECREASE * ts[j]) * gd), None)
        if j is None:
            flag = FLAG_NO_STEP
            break
        x = trial_point(x, d, ts[j])
        phi, g, H = evaluate(un, L, kept, x, nkf)
    sx = np.float64(0.0)
    for k in range(K):
        sx = sx + x[k]
    pi = x / sx
    post, loglik = posterior(un, b, s, L, lnorm, kept, sigma, pi, threshold)
    post.update(pi=pi, sd=sigma, K=K, iter=it, flag=flag, loglik=loglik, nkept=nk)
    return post


ROW_KEYS = ("PosteriorMean", "PosteriorSD", "NegativeProb", "PositiveProb", "lfsr", "le_T", "gt_mT")


def fit(un, b, s, threshold=None, maxit=100):
    """b, s: n or n x C.  Returns dict: the ROW_KEYS n x C (NaN on the rows that are not kept; le_T / gt_mT NaN without a
    threshold), pi and sd C x MAX_K (zero beyond K), K, iter, flag (int32, C), loglik (C)"""
    b, s = np.asarray(b, np.float64), np.asarray(s, np.float64)
    if b.shape != s.shape or b.ndim not in (1, 2):
        raise ValueError("betahat and sebetahat are two vectors of one length, or two n x C matrices")
    B, S = (b[:, None], s[:, None]) if b.ndim == 1 else (b, s)
    n, C = B.shape
    cols = [fit_column(un, B[:, c], S[:, c], threshold, maxit) for c in range(C)]
    out = {k: np.stack([f[k] for f in cols], axis=1) for k in ROW_KEYS}
    out["pi"], out["sd"] = np.zeros((C, MAX_K)), np.zeros((C, MAX_K))
    for c, f in enumerate(cols):
        out["pi"][c, :f["K"]], out["sd"][c, :f["K"]] = f["pi"], f["sd"]
    for k in ("K", "iter", "flag"):
        out[k] = np.array([f[k] for f in cols], np.int32)
    out["loglik"] = np.array([f["loglik"] for f in cols], np.float64)
    return out
