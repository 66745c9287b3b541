"""The arithmetic specification of the apeglm posterior stated in numpy: the reference for the
apeglm tests.  Not a test itself.  exp / log / log1p are the oracle's (oracle.unary, bit-equal to the device's dexp / dlog /
dlog1p, tests/test_gpu_math.py), sqrt is IEEE; +, -, *, / are IEEE, every operation rounded once, in the order written here.
Shares no code with the product (deseq2_amd/csrc/apeglm.hip, deseq2_amd/apeglm_host.py, core.apeglm).

THE ESTIMATOR.  Gene i: counts y_j, design x (m x p), offsets o_j = log nf_j, weights w_j >= 0, dispersion a.  Coefficients on
the natural-log scale.  The columns in no_shrink get Normal(0, NS^2) (NS = 15), every other column a Student t prior with df
degrees of freedom (1: Cauchy), mean 0 and scale S.  The negative log posterior, constants dropped:

    F(b) = - sum_j w_j [ y_j eta_j - (y_j + 1/a) log1p(a mu_j) ]
           + sum_{k in no_shrink} b_k^2 / (2 NS^2) + sum_{k not in no_shrink} ((df + 1) / 2) log1p(b_k^2 / (df S^2))
    eta = x b + o,  mu = exp(eta)
    dF/db_k    = - sum_j w_j x_jk (y_j - mu_j) / (1 + a mu_j)       + b_k / NS^2  |  (df + 1) b_k / (df S^2 + b_k^2)
    d2F/db_k l =   sum_j w_j x_jk x_jl mu_j (1 + a y_j) / (1 + a mu_j)^2
                                                + [k = l] ( 1 / NS^2  |  (df + 1) (df S^2 - b_k^2) / (df S^2 + b_k^2)^2 )

(the log1p(a mu) form: log(mu + 1/a) loses eight digits of F at a = 1e-8).  The prior curvature is negative beyond
|b_k| = sqrt(df) S: the posterior can have two modes.

THE SEARCH is the library's own: damped Newton (Levenberg-Marquardt).  At b with (F, g, H), damping lam (0 at the start):
    solve (H + lam diag|H_kk|) s = -g by Cholesky (rows in order, inner products subtracted term by term, ascending)
    the trial b + s is ACCEPTED when F(b + s) is finite and, with pred = -g.s and res = 2^-44 max(M, 1), M the sum of the
    magnitudes F is made of (sum_j w_j (|y_j eta_j| + (y_j + 1/a) log1p(a mu_j)) plus the prior's terms: F itself can cancel
    to nothing while its rounding stays that of M),
        pred > res:   F(b + s) <= F - 1e-4 pred         (Armijo on the true objective)
        otherwise:    F(b + s) <= F + res               (the predicted decrease is below what F resolves: near the optimum
                                                         g.s ~ 1e-13 at F ~ 770, and a pure Armijo test would reject the
                                                         exact Newton step for ever)
    a failed factorisation, a non-finite trial or a rejected one raise lam (1e-4 first, then x 10; beyond 1e12: conv = 2)
    an accepted step with lam = 0 and max |s| < tol ends the search with conv = 0; otherwise lam <- lam / 10, 0 below 1e-7
    maxit iterations: conv = 1 (maxit = 0 returns the start); F not finite at the start: conv = 2, objective NaN
Two starts: (a) shrunken coefficients 0, column 0 -- when it is unshrunken -- at log(max(sum w y/nf / sum w, 0.1)), other
unshrunken columns 0; (b) the caller's init clipped to +-30, when given.  The lower F is kept; a tie (or an F that is not
finite at (b)) goes to (a).

Every sum over the samples: lane l of 64 adds the samples l, l + 64, ... in order from 0.0, then the xor butterfly of
sf_spec.wave_sum.

OUTPUTS.  map; sd_k = sqrt((H(map)^-1)_kk) (one Cholesky solve per unit vector; no factor: sd NaN and conv + 4);
for the coefficient c: fsr = pnorm(-|map_c| / sd_c); with a threshold T: thresh = P(|b_c| < T) under N(map_c, sd_c^2),
formed from the lower tails when map_c >= 0 and from the upper tails otherwise (the side where neither is near one).
A row whose counts are all zero or whose dispersion is NaN, infinite or not positive: NaN everywhere."""
import math

import numpy as np

from tests.results_spec import pnorm_both
from tests.sf_spec import _exp, _log, wave_sum

MAX_P = 16
ARMIJO = 1e-4
RES = 2.0 ** -44
LAM_FIRST, LAM_UP, LAM_DOWN, LAM_ZERO, LAM_MAX = 1e-4, 10.0, 0.1, 1e-7, 1e12
CLIP = 30.0
NOT_PD = 4
QNORM_975 = 1.959963984540054           # qnorm(0.975)


def _log1p(O, v):
    return O.unary("log1p", np.ascontiguousarray(v, dtype=np.float64))


class Posterior:
    """F, gradient and Hessian of one gene"""

    def __init__(self, O, y, x, nf, w, a, no_shrink, S, df=1.0, NS=15.0):
        self.O = O
        self.y, self.x, self.w = np.asarray(y, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64)
        self.o = _log(O, np.asarray(nf, np.float64))
        self.a = np.float64(a)
        self.no_shrink = np.asarray(no_shrink, bool)
        self.S, self.df, self.NS = np.float64(S), np.float64(df), np.float64(NS)

    def __call__(self, b):
        y, x, w, a = self.y, self.x, self.w, self.a
        m, p = x.shape
        with np.errstate(all="ignore"):
            eta = x[:, 0] * b[0]
            for k in range(1, p):
                eta = eta + x[:, k] * b[k]
            eta = eta + self.o
            mu = _exp(self.O, eta)
            am = a * mu
            inva = 1.0 / a
            one = 1.0 + am
            r = w * ((y - mu) / one)
            h = w * ((mu * (1.0 + a * y)) / (one * one))
            # every sum is its own wave-order sum; they are taken in one call, one row of `terms` each
            t1, t2 = y * eta, (y + inva) * _log1p(self.O, am)
            terms = [w * (t1 - t2)]
            terms += [r * x[:, k] for k in range(p)]
            terms += [(h * x[:, k]) * x[:, l] for k in range(p) for l in range(k + 1)]
            terms += [w * (np.abs(t1) + t2)]                        # the magnitudes F is summed from
            sums = wave_sum(np.stack(terms))
            F, Fmag = -sums[0], sums[-1]
            g = -sums[1:1 + p]
            H = np.zeros((p, p))
            at = 1 + p
            for k in range(p):
                for l in range(k + 1):
                    H[k, l] = H[l, k] = sums[at]
                    at += 1
            ds2 = self.df * (self.S * self.S)
            df1 = self.df + 1.0
            ns2 = self.NS * self.NS
            for k in range(p):
                if self.no_shrink[k]:
                    t = (b[k] * b[k]) / (2.0 * ns2)
                    F, Fmag = F + t, Fmag + t
                    g[k] = g[k] + b[k] / ns2
                    H[k, k] = H[k, k] + 1.0 / ns2
                else:
                    bb = b[k] * b[k]
                    den = ds2 + bb
                    t = (df1 / 2.0) * _log1p(self.O, np.array([bb / ds2]))[0]
                    F, Fmag = F + t, Fmag + t
                    g[k] = g[k] + (df1 * b[k]) / den
                    H[k, k] = H[k, k] + (df1 * (ds2 - bb)) / (den * den)
        self.magnitude = Fmag
        return F, g, H


def solve(H, rhs, lam):
    """(H + lam diag|H_kk|) s = rhs by Cholesky, or None when a pivot is not positive and finite"""
    p = rhs.size
    Lo = np.zeros((p, p))
    s = np.zeros(p)
    with np.errstate(all="ignore"):
        for i in range(p):
            for j in range(i + 1):
                v = np.float64(H[i, j])
                if i == j:
                    v = v + np.float64(lam) * abs(v)
                for t in range(j):
                    v = v - Lo[i, t] * Lo[j, t]
                if i == j:
                    if not (v > 0.0 and v < np.inf):
                        return None
                    Lo[i, i] = np.sqrt(v)
                else:
                    Lo[i, j] = v / Lo[j, j]
        for i in range(p):
            v = np.float64(rhs[i])
            for t in range(i):
                v = v - Lo[i, t] * s[t]
            s[i] = v / Lo[i, i]
        for i in range(p - 1, -1, -1):
            v = s[i]
            for t in range(i + 1, p):
                v = v - Lo[t, i] * s[t]
            s[i] = v / Lo[i, i]
    return s


def search(post, b, tol=1e-8, maxit=100, resolution_clause=True):
    """(b, F, H, iter, conv) from the start b.  resolution_clause = False: the pure Armijo rule (the tests' mutant)"""
    b = np.array(b, np.float64)
    F, g, H = post(b)
    Fmag = post.magnitude
    if not np.isfinite(F):
        return b, np.nan, H, 0, 2
    lam = 0.0
    for it in range(1, maxit + 1):
        while True:
            s = solve(H, -g, lam)
            if s is not None:
                with np.errstate(all="ignore"):
                    gs = g[0] * s[0]
                    for k in range(1, b.size):
                        gs = gs + g[k] * s[k]
                    pred = -gs
                    bt = b + s
                    Ft, gt, Ht = post(bt)
                    res = RES * max(Fmag, 1.0)
                    if pred > res or not resolution_clause:
                        ok = Ft <= F - ARMIJO * pred
                    else:
                        ok = Ft <= F + res
                if np.isfinite(Ft) and ok:
                    break
            lam = LAM_FIRST if lam < LAM_FIRST else lam * LAM_UP
            if lam > LAM_MAX:
                return b, F, H, it, 2
        b, F, g, H, Fmag = bt, Ft, gt, Ht, post.magnitude
        if lam == 0.0 and np.abs(s).max() < tol:
            return b, F, H, it, 0
        lam = lam * LAM_DOWN
        if lam < LAM_ZERO:
            lam = 0.0
    return b, F, H, maxit, 1


def start_a(O, y, nf, w, p, no_shrink):
    b = np.zeros(p)
    if no_shrink[0]:
        with np.errstate(all="ignore"):
            sy, sw = wave_sum(w * (y / nf)), wave_sum(w)
            q = sy / sw if sw > 0.0 else 0.0
        b[0] = _log(O, np.array([q if q > 0.1 else 0.1]))[0]
    return b


def clip(v):
    v = np.array(v, np.float64)
    v[v < -CLIP] = -CLIP
    v[v > CLIP] = CLIP
    return v


def fit_gene(O, y, x, nf, w, a, coef, no_shrink, S, df=1.0, NS=15.0, init=None, threshold=None, tol=1e-8, maxit=100, **kw):
    """dict of one gene's outputs, or None for a row that is not fitted"""
    y = np.asarray(y, np.float64)
    p = x.shape[1]
    if not (a > 0.0 and a < np.inf) or not (y != 0).any():
        return None
    post = Posterior(O, y, x, nf, w, a, no_shrink, S, df, NS)
    runs = [search(post, start_a(O, y, np.asarray(nf, np.float64), np.asarray(w, np.float64), p, no_shrink), tol, maxit, **kw)]
    if init is not None:
        runs.append(search(post, clip(init), tol, maxit, **kw))
    start = 1 if len(runs) == 2 and runs[1][1] < runs[0][1] else 0
    b, F, H, _, conv = runs[start]
    sd = np.full(p, np.nan)
    cols = [solve(H, np.eye(p)[k], 0.0) for k in range(p)]
    if cols[0] is None:
        conv += NOT_PD
    else:
        with np.errstate(all="ignore"):
            sd = np.sqrt(np.array([cols[k][k] for k in range(p)]))
    with np.errstate(all="ignore"):
        fsr = pnorm_both(O, np.array([-(abs(b[coef]) / sd[coef])]))[0][0]
        thresh = np.nan
        if threshold is not None:
            lo, up = pnorm_both(O, np.array([(threshold - b[coef]) / sd[coef], (-threshold - b[coef]) / sd[coef]]))
            thresh = lo[0] - lo[1] if b[coef] >= 0.0 else up[1] - up[0]
    return {"map": b, "sd": sd, "fsr": fsr, "thresh": thresh, "iter": [runs[0][3], runs[1][3] if len(runs) == 2 else 0],
            "conv": conv, "start": start, "objective": F}


def fit(O, Y, x, nf, disp, coef, no_shrink, S, df=1.0, NS=15.0, weights=None, init=None, threshold=None, tol=1e-8, maxit=100, **kw):
    """dict(map n x p, sd n x p, fsr, thresh, iter n x 2, conv, start, objective), NaN on the rows that are not fitted.
    nf: m size factors or an n x m matrix; no_shrink: boolean mask of p"""
    Y = np.asarray(Y, np.float64)
    x = np.asarray(x, np.float64)
    n, m = Y.shape
    p = x.shape[1]
    assert 1 <= p <= MAX_P and 0 <= coef < p and not no_shrink[coef]
    nf = np.broadcast_to(np.asarray(nf, np.float64), (n, m))
    out = {"map": np.full((n, p), np.nan), "sd": np.full((n, p), np.nan), "fsr": np.full(n, np.nan), "thresh": np.full(n, np.nan),
           "iter": np.full((n, 2), np.nan), "conv": np.full(n, np.nan), "start": np.full(n, np.nan), "objective": np.full(n, np.nan)}
    for i in range(n):
        r = fit_gene(O, Y[i], x, nf[i], np.ones(m) if weights is None else weights[i], disp[i], coef, np.asarray(no_shrink, bool), S,
                     df, NS, None if init is None else init[i], threshold, tol, maxit, **kw)
        if r is not None:
            for k in out:
                out[k][i] = r[k]
    return out


def interval(mapc, sdc):
    """map_c -+ qnorm(0.975) sd_c, n x 2"""
    return np.stack([mapc - QNORM_975 * sdc, mapc + QNORM_975 * sdc], axis=1)


def svalue(lfsr):
    """R/lfcShrink.R:523-528 as written"""
    lfsr = np.asarray(lfsr, np.float64)
    n = lfsr.size
    nan = np.isnan(lfsr)
    order = sorted(range(n), key=lambda i: (nan[i], lfsr[i] if not nan[i] else 0.0, i))   # sort / rank, ties "first", NA last
    lfsr_sorted = lfsr[order]                                    # :524
    cumsum_idx = np.arange(1, n + 1)                             # :525
    cumsum_lfsr = np.cumsum(lfsr_sorted)                         # :526 (sequential, as R's cumsum)
    rank = np.empty(n, int)
    rank[order] = np.arange(n)
    return (cumsum_lfsr / cumsum_idx)[rank]                      # :527


def prior_scale_equation(A, D, S):
    """sum_i (D_i^2 - S_i^2 - A) / (S_i^2 + A)^2, the score of the marginal likelihood D_i ~ N(0, A + S_i^2), by fsum"""
    return math.fsum((d * d - s * s - A) / ((s * s + A) ** 2) for d, s in zip(D, S))
