"""The arithmetic specification of adaptive shrinkage stated in numpy: the reference for the ash tests.
Not a test itself.  exp / log are the oracle's (oracle.unary, bit-equal to the device's dexp / dlog), sqrt is IEEE; +, -, *, /
are IEEE, every operation rounded once, in the order written here.  Shares no code with the product (deseq2_amd/csrc/ash.hip,
deseq2_amd/ash_host.py, core.ash).

THE ESTIMATOR.  ashr::ash(b, s, mixcompdist = "normal", method = "shrink") (Stephens 2017): beta_i ~ sum_k pi_k N(0, sigma_k^2),
b_i | beta_i ~ N(beta_i, s_i^2); no point mass, uniform prior on pi, mode 0.  A row is KEPT when b is finite and s finite and
positive; the others take no part and come back NaN.  No kept row: ValueError.

GRID (ashr's gridmult = sqrt(2) rule).  smin = min s / 10; smax = 2 sqrt(max (b b - s s)) when that maximum is positive, else
8 smin; npoint = max(ceil(2 log2(smax / smin)), 1), formed exactly from the binary exponent and mantissa of the quotient;
sigma_k = sqrt(2)^(k - npoint) smax: smax, or smax * 0x1.6a09e667f3bcdp-1 for an odd power, scaled by a power of two.
K = npoint + 1 > 64: Unsupported.

LIKELIHOOD.  v = s s + sigma_k sigma_k; l_ik = (-0.5 log(2 pi v)) - (0.5 (b b / v)); lnorm_i = max_k; L_ik = exp(l_ik - lnorm_i).

SUMS OVER THE ROWS: slices of 128 consecutive rows, each in 8 groups of 16; a group adds its rows in order from 0.0, a slice
its groups in order starting from the first, the slices are added in order from 0.0.  A row that is not kept enters as 0.0.
Sums over the components run in order from 0.0.

WEIGHTS.  Minimise phi(x) = -(1/n) sum_i log u_i + sum_k x_k, u = L x, over x >= 0 (n the kept count) from x = 1/K:
    g_k = 1 - (sum_i L_ik / u_i) / n,   H_kl = (sum_i (L_ik / u_i)(L_il / u_i)) / n + 1e-8 [k = l]
    min_k g_k >= -1e-8: flag 0.  Else, after maxit iterations: flag 1.  Else the quadratic programme
        min d'Hd / 2 + g'd  subject to  x + d >= 0
    by the ACTIVE-SET method below, then the first t = 0.75^j, j = 0 .. 31, with
        phi(max(x + t d, 0)) <= phi(x) + (0.01 t) g'd        (d = 0, or no such j: flag 2)
ACTIVE SET, on y = x + d from y = x.  Working set W = { k : not x_k > 0 }.  Up to 4 K + 8 rounds:
    q = g + H (y - x) (column by column, in order); on the free set F solve H_FF p = -q_F by Cholesky (each element loses its
    products in ascending order of the column; forward substitution ascending, backward descending); a pivot that is not
    positive and finite: retry with the ridge (1e-8 max_k H_kk) 10^j, j = 0 .. 12, then give up (d = y - x as it stands).
    ratio_k = y_k / -p_k over the p_k < 0; a = min: a <= 1 -> y = max(y + a p, 0), the first k at the minimum gets y_k = 0 and joins
    W, next round.  Otherwise y = max(y + p, 0), q again; the k in W with the smallest q_k (the first among equals) leaves W when
    q_k < -1e-12; none: done.
pi = x / sum x.

POSTERIOR at pi, per kept row: u = sum_k pi_k L_k; w_k = (pi_k L_k) / u; den = sigma_k^2 + s^2; m_k = (b sigma_k^2) / den;
v_k = (sigma_k^2 s^2) / den; PosteriorMean = sum w m; PosteriorSD = sqrt(sum w (v + (m - PM)^2));
NegativeProb = sum w pnorm(-m / sqrt v), PositiveProb = sum w pnorm(-m / sqrt v, lower = FALSE); lfsr the smaller;
with T: le_T = sum w pnorm((T - m) / sqrt v), gt_mT = sum w pnorm((-T - m) / sqrt v, lower = FALSE).
loglik = sum_i (log u_i + lnorm_i)."""
import numpy as np

from tests.results_spec import pnorm_both
from tests.sf_spec import _exp, _log

MAX_K, SLICE, GROUP, TRIALS = 64, 128, 16, 32
ROWS = ("PosteriorMean", "PosteriorSD", "NegativeProb", "PositiveProb", "lfsr", "le_T", "gt_mT")
KEYS = ROWS + ("pi", "sd", "K", "iter", "flag", "loglik")


class Unsupported(NotImplementedError):
    pass


def kept(b, s):
    with np.errstate(invalid="ignore"):
        return np.isfinite(b) & np.isfinite(s) & (s > 0)


def grid(b, s):
    k = kept(b, s)
    if not k.any():
        raise ValueError("no kept row")
    smin = s[k].min() / 10.0
    dmax = (b[k] * b[k] - s[k] * s[k]).max()
    smax = 2.0 * np.sqrt(dmax) if dmax > 0.0 else 8.0 * smin
    r = smax / smin
    if not (0.0 < r < np.inf):
        raise Unsupported("grid")
    f, e = np.frexp(r)
    c = 2 * int(e) - (2 if f == 0.5 else 1 if f < float.fromhex("0x1.6a09e667f3bcdp-1") else 0)
    npoint = max(c, 1)
    if npoint + 1 > MAX_K:
        raise Unsupported("K = %d" % (npoint + 1))
    out = []
    for j in range(npoint + 1):
        back = npoint - j
        base = smax * float.fromhex("0x1.6a09e667f3bcdp-1") if back % 2 else smax
        out.append(np.ldexp(base, -(back // 2)))
    return np.array(out)


def row_sum(T, keep):
    """the sum down the rows of T (n x E): slices, groups, rows, as the docstring orders them"""
    n = T.shape[0]
    total = np.zeros(T.shape[1])
    for r0 in range(0, n, SLICE):
        sl = None
        for g0 in range(r0, r0 + SLICE, GROUP):
            acc = np.zeros(T.shape[1])
            for i in range(g0, min(g0 + GROUP, n)):
                acc = acc + (T[i] if keep[i] else 0.0)
            sl = acc if sl is None else sl + acc
        total = total + sl
    return total


def block(O, b, s, sigma):
    keep = kept(b, s)
    n, K = b.size, sigma.size
    L, lnorm = np.zeros((n, K)), np.zeros(n)
    for i in np.flatnonzero(keep):
        v = s[i] * s[i] + sigma * sigma
        l = (-0.5 * _log(O, 6.283185307179586 * v)) - (0.5 * ((b[i] * b[i]) / v))
        lnorm[i] = l.max()
        L[i] = _exp(O, l - lnorm[i])
    return L, lnorm, keep


def mixture(L, x):
    u = np.zeros(L.shape[0])
    for k in range(x.size):
        u = u + x[k] * L[:, k]
    return u


def ordered(v):
    acc = np.float64(0.0)
    for e in v:
        acc = acc + e
    return acc


def evaluate(O, L, keep, x, nk):
    K = x.size
    with np.errstate(all="ignore"):
        u = np.where(keep, mixture(L, x), 1.0)
        z = L / u[:, None]
        pairs = [(k, l) for k in range(K) for l in range(k, K)]
        T = np.column_stack([_log(O, u), z] + [z[:, k] * z[:, l] for k, l in pairs])
        S = row_sum(T, keep)
        phi = (-(S[0] / nk)) + ordered(x)
        g = 1.0 - S[1:1 + K] / nk
        H = np.zeros((K, K))
        for (k, l), v in zip(pairs, S[1 + K:] / nk):
            H[k, l] = H[l, k] = v
        for k in range(K):
            H[k, k] = H[k, k] + 1e-8
    return phi, g, H


def solve(A, rhs, ridge):
    """Cholesky solve, left-looking: column j loses the earlier columns' products in ascending order"""
    F = rhs.size
    A = A + ridge * np.eye(F)
    C = np.zeros((F, F))
    with np.errstate(all="ignore"):
        for j in range(F):
            col = A[j:, j].copy()
            for t in range(j):
                col = col - C[j:, t] * C[j, t]
            if not (0.0 < col[0] < np.inf):
                return None
            C[j, j] = np.sqrt(col[0])
            C[j + 1:, j] = col[1:] / C[j, j]
        y = rhs.astype(np.float64).copy()
        for i in range(F):
            acc = y[i]
            for t in range(i):
                acc = acc - C[i, t] * y[t]
            y[i] = acc / C[i, i]
        for i in reversed(range(F)):
            acc = y[i]
            for t in reversed(range(i + 1, F)):
                acc = acc - C[t, i] * y[t]
            y[i] = acc / C[i, i]
    return y


def quadratic_programme(H, g, x):
    K = x.size
    y = x.copy()
    W = [not (x[k] > 0.0) for k in range(K)]
    hmax = max(H[k, k] for k in range(K))

    def gradient():
        q = g.copy()
        for l in range(K):
            q = q + H[:, l] * (y[l] - x[l])
        return q
    with np.errstate(all="ignore"):
        for _ in range(4 * K + 8):
            q = gradient()
            F = [k for k in range(K) if not W[k]]
            if F:
                A = H[np.ix_(F, F)]
                p = solve(A, -q[F], 0.0)
                for j in range(13):
                    if p is not None:
                        break
                    p = solve(A, -q[F], (1e-8 * hmax) * 10.0 ** j)
                if p is None:
                    break
                best, at = np.inf, -1
                for a, k in enumerate(F):
                    if p[a] < 0.0 and y[k] / (-p[a]) < best:
                        best, at = y[k] / (-p[a]), a
                step = best if (at >= 0 and best <= 1.0) else 1.0
                for a, k in enumerate(F):
                    v = y[k] + step * p[a]
                    y[k] = v if v > 0.0 else 0.0
                if at >= 0 and best <= 1.0:
                    y[F[at]] = 0.0
                    W[F[at]] = True
                    continue
            q = gradient()
            inW = [k for k in range(K) if W[k]]
            if not inW:
                break
            kmin = inW[0]
            for k in inW[1:]:
                if q[k] < q[kmin]:
                    kmin = k
            if not (q[kmin] < -1e-12):
                break
            W[kmin] = False
    return y - x


def steps():
    out = [np.float64(1.0)]
    while len(out) < TRIALS:
        out.append(out[-1] * 0.75)
    return out


def fit_column(O, b, s, threshold=None, maxit=100):
    b, s = np.asarray(b, np.float64), np.asarray(s, np.float64)
    sigma = grid(b, s)
    K = sigma.size
    L, lnorm, keep = block(O, b, s, sigma)
    nk = np.float64(keep.sum())
    x = np.full(K, 1.0 / K)
    it, ts = 0, steps()
    phi, g, H = evaluate(O, L, keep, x, nk)
    while True:
        if g.min() >= -1e-8:
            flag = 0
            break
        if it >= maxit:
            flag = 1
            break
        it += 1
        d = quadratic_programme(H, g, x)
        gd = ordered(g * d)
        flag = 2
        if np.abs(d).max() > 0.0:
            with np.errstate(all="ignore"):
                xs = [np.where(x + t * d > 0.0, x + t * d, 0.0) for t in ts]
                T = np.column_stack([_log(O, np.where(keep, mixture(L, xt), 1.0)) for xt in xs])
                S = row_sum(T, keep)
            for j, t in enumerate(ts):
                if (-(S[j] / nk)) + ordered(xs[j]) <= phi + (0.01 * t) * gd:
                    x, flag = xs[j], 0
                    break
        if flag == 2:
            break
        phi, g, H = evaluate(O, L, keep, x, nk)
    pi = x / ordered(x)
    out = {k: np.full(b.size, np.nan) for k in ROWS}
    with np.errstate(all="ignore"):
        u = mixture(L, pi)
        ll = _log(O, np.where(keep, u, 1.0)) + lnorm
        loglik = row_sum(ll[:, None], keep)[0]
        for i in np.flatnonzero(keep):
            den = sigma * sigma + s[i] * s[i]
            w = (pi * L[i]) / u[i]
            m = (b[i] * (sigma * sigma)) / den
            v = ((sigma * sigma) * (s[i] * s[i])) / den
            pm = ordered(w * m)
            sd = np.sqrt(v)
            lo, up = pnorm_both(O,(-m) / sd)
            out["PosteriorMean"][i] = pm
            out["PosteriorSD"][i] = np.sqrt(ordered(w * (v + (m - pm) * (m - pm))))
            out["NegativeProb"][i], out["PositiveProb"][i] = ordered(w * lo), ordered(w * up)
            out["lfsr"][i] = min(out["NegativeProb"][i], out["PositiveProb"][i])
            if threshold is not None:
                out["le_T"][i] = ordered(w * pnorm_both(O,(threshold - m) / sd)[0])
                out["gt_mT"][i] = ordered(w * pnorm_both(O,((-threshold) - m) / sd)[1])
    out.update(pi=pi, sd=sigma, K=K, iter=it, flag=flag, loglik=loglik)
    return out


def fit(O, b, s, threshold=None, maxit=100):
    """b, s: n x C.  The per-row outputs (C, n); pi, sd (C, 64) zero beyond K; K, iter, flag int32 (C,); loglik (C,)"""
    b, s = np.asarray(b, np.float64), np.asarray(s, np.float64)
    b, s = (b[:, None], s[:, None]) if b.ndim == 1 else (b, s)
    cols = [fit_column(O, b[:, c], s[:, c], threshold, maxit) for c in range(b.shape[1])]
    out = {k: np.stack([f[k] for f in cols]) for k in ROWS}
    out["pi"], out["sd"] = np.zeros((len(cols), MAX_K)), np.zeros((len(cols), MAX_K))
    for c, f in enumerate(cols):
        out["pi"][c, :f["K"]], out["sd"][c, :f["K"]] = f["pi"], f["sd"]
    for k in ("K", "iter", "flag"):
        out[k] = np.array([f[k] for f in cols], np.int32)
    out["loglik"] = np.array([f["loglik"] for f in cols])
    return out
