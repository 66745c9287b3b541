"""The apeglm posterior on the host: the iteration of csrc/apeglm.hip in numpy over an engine's
exp / log / log1p, the same operations in the same order, so that HostEngine.apeglm_fit and dsq_apeglm_dev agree to the bit.

Per gene: minimise the negative log posterior F(b) of a negative binomial GLM under a Student t prior (Cauchy at
prior_df = 1) on the shrunken coefficients and Normal(0, no_shrink_scale^2) on the others, by a damped Newton
(Levenberg-Marquardt) iteration from two starts.  `un(name, v)` is the engine's unary arithmetic.  Every sum over the
samples: lane l of 64 adds the samples l, l + 64, ... in order from 0.0, then the xor butterfly (1, 2, 4, 8, 16, 32)."""
import numpy as np

from .results_host import pnorm_both

MAX_P = 16                         # DSQ_APEGLM_MAX_P
ARMIJO = 1e-4
RESOLUTION = 2.0 ** -44            # a predicted decrease below RESOLUTION max(magnitude of F's terms, 1) is below what F resolves
LAMBDA_FIRST, LAMBDA_UP, LAMBDA_DOWN, LAMBDA_ZERO, LAMBDA_MAX = 1e-4, 10.0, 0.1, 1e-7, 1e12
CLIP = 30.0
CONV_NOT_PD = 4                    # added to conv when the Hessian at the returned point has no Cholesky factor
_LANES = np.arange(64)


def _lane_sums(cols):
    """wave-order sums down the samples of an (m, C) array"""
    part = np.zeros((64, cols.shape[1]))
    for j0 in range(0, cols.shape[0], 64):
        blk = cols[j0:j0 + 64]
        part[:blk.shape[0]] += blk
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[_LANES ^ off]
    return part[0]


class _Gene:
    """the data of one gene and its posterior at a point: (F, g, packed lower triangle of H, the magnitude F is summed from)"""

    def __init__(self, un, y, x, off, w, a, shrink, S, df, ns):
        self.un, self.y, self.x, self.off, self.w, self.a = un, y, x, off, w, np.float64(a)
        self.inva = np.float64(1.0) / self.a
        self.shrink = shrink
        self.p = x.shape[1]
        self.tri = np.tril_indices(self.p)
        S, df, ns = np.float64(S), np.float64(df), np.float64(ns)
        self.ds2, self.df1 = df * (S * S), df + 1.0
        self.c = self.df1 / 2.0
        self.ns2 = ns * ns
        self.two_ns2 = 2.0 * self.ns2

    def at(self, b):
        p, x, y = self.p, self.x, self.y
        with np.errstate(all="ignore"):
            e = x[:, 0] * b[0]
            for k in range(1, p):
                e = e + x[:, k] * b[k]
            eta = e + self.off
            mu = self.un("exp", eta)
            am = self.a * mu
            L = self.un("log1p", am)
            t1, t2 = y * eta, (y + self.inva) * L
            d1 = 1.0 + am
            wr = self.w * ((y - mu) / d1)
            wh = self.w * ((mu * (1.0 + self.a * y)) / (d1 * d1))
            whx = wh[:, None] * x
            s = _lane_sums(np.concatenate([(self.w * (t1 - t2))[:, None], wr[:, None] * x, whx[:, self.tri[0]] * x[:, self.tri[1]],
                                           (self.w * (np.abs(t1) + t2))[:, None]], axis=1))
            F, g, H, Fm = -s[0], -s[1:1 + p], s[1 + p:-1].copy(), s[-1]
            for k in range(p):
                kk = k * (k + 1) // 2 + k
                if self.shrink[k]:
                    bb = b[k] * b[k]
                    den = self.ds2 + bb
                    t = self.c * self.un("log1p", np.array([bb / self.ds2]))[0]
                    F, Fm = F + t, Fm + t
                    g[k] = g[k] + (self.df1 * b[k]) / den
                    H[kk] = H[kk] + (self.df1 * (self.ds2 - bb)) / (den * den)
                else:
                    t = (b[k] * b[k]) / self.two_ns2
                    F, Fm = F + t, Fm + t
                    g[k] = g[k] + b[k] / self.ns2
                    H[kk] = H[kk] + 1.0 / self.ns2
        return F, g, H, Fm


def cholesky_solve(H, rhs, lam):
    """d with (H + lam diag|H_kk|) d = rhs for the packed lower triangle H; None when a pivot is not positive"""
    p = rhs.size
    at = lambda i, j: i * (i + 1) // 2 + j
    Lf = np.zeros(p * (p + 1) // 2)
    d = np.zeros(p)
    with np.errstate(all="ignore"):
        for i in range(p):
            for j in range(i + 1):
                s = H[at(i, j)]
                if i == j:
                    s = s + lam * np.abs(s)
                for t in range(j):
                    s = s - Lf[at(i, t)] * Lf[at(j, t)]
                if i == j:
                    if not (s > 0.0 and s < np.inf):
                        return None
                    Lf[at(i, i)] = np.sqrt(s)
                else:
                    Lf[at(i, j)] = s / Lf[at(j, j)]
        for i in range(p):
            s = rhs[i]
            for t in range(i):
                s = s - Lf[at(i, t)] * d[t]
            d[i] = s / Lf[at(i, i)]
        for i in reversed(range(p)):
            s = d[i]
            for t in range(i + 1, p):
                s = s - Lf[at(t, i)] * d[t]
            d[i] = s / Lf[at(i, i)]
    return d


def search(gene, b, tol, maxit):
    """the damped Newton iteration from b: (b, F, H, iter, conv)"""
    F, g, H, Fm = gene.at(b)
    if not np.isfinite(F):
        return b, np.float64(np.nan), H, 0, 2
    lam, it = np.float64(0.0), 0
    while it < maxit:
        it += 1
        trial = None
        while True:
            s = cholesky_solve(H, -g, lam)
            if s is not None:
                with np.errstate(all="ignore"):
                    bt = b + s
                    gs = g[0] * s[0]
                    for k in range(1, b.size):
                        gs = gs + g[k] * s[k]
                    pred = -gs
                    cand = gene.at(bt)
                    res = RESOLUTION * (Fm if Fm > 1.0 else 1.0)
                    if np.isfinite(cand[0]) and (cand[0] <= F - ARMIJO * pred if pred > res else cand[0] <= F + res):
                        trial = cand
                        break
            lam = np.float64(LAMBDA_FIRST) if lam < LAMBDA_FIRST else lam * LAMBDA_UP
            if lam > LAMBDA_MAX:
                break
        if trial is None:
            return b, F, H, it, 2
        b, (F, g, H, Fm) = bt, trial
        if lam == 0.0 and np.abs(s).max() < tol:
            return b, F, H, it, 0
        lam = lam * LAMBDA_DOWN
        if lam < LAMBDA_ZERO:
            lam = np.float64(0.0)
    return b, F, H, it, 1


def clip(v):
    v = np.asarray(v, np.float64)
    return np.where(v < -CLIP, -CLIP, np.where(v > CLIP, CLIP, v))


def fit(un, y, x, nf, disp, coef, no_shrink, prior_scale, prior_df=1.0, no_shrink_scale=15.0, weights=None, init=None,
        threshold=None, tol=1e-8, maxit=100):
    """y: n x m counts, nf: m or n x m, x: m x p; no_shrink: boolean mask of p.  Returns dict(map n x p, sd n x p, fsr n,
    thresh n (NaN without a threshold), iter n x 2, conv n, start n, objective n), NaN on the rows that are not fitted"""
    y = np.asarray(y, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    n, m = y.shape
    p = x.shape[1]
    nf = np.broadcast_to(np.asarray(nf, np.float64), (n, m))
    shrink = ~np.asarray(no_shrink, bool)
    vexp = lambda v: un("exp", v)
    out = {"map": np.full((n, p), np.nan), "sd": np.full((n, p), np.nan), "fsr": np.full(n, np.nan),
           "thresh": np.full(n, np.nan), "iter": np.full((n, 2), np.nan), "conv": np.full(n, np.nan),
           "start": np.full(n, np.nan), "objective": np.full(n, np.nan)}
    for i in range(n):
        a = disp[i]
        if not (a > 0.0 and a < np.inf) or not (y[i] != 0.0).any():
            continue
        w = np.ones(m) if weights is None else np.asarray(weights[i], np.float64)
        gene = _Gene(un, y[i], x, un("log", np.ascontiguousarray(nf[i])), w, a, shrink, prior_scale, prior_df, no_shrink_scale)
        b0 = np.zeros(p)
        if not shrink[0]:
            with np.errstate(all="ignore"):
                sy, sw = _lane_sums(np.stack([w * (y[i] / nf[i]), w], axis=1))
                q = sy / sw if sw > 0.0 else 0.0
            b0[0] = un("log", np.array([q if q > 0.1 else 0.1]))[0]
        best = search(gene, b0, tol, maxit)
        iters, start = [best[3], 0], 0
        if init is not None:
            other = search(gene, clip(init[i]), tol, maxit)
            iters[1] = other[3]
            if other[1] < best[1]:
                best, start = other, 1
        b, F, H, _, conv = best
        e = np.eye(p)
        var = [cholesky_solve(H, e[k], np.float64(0.0)) for k in range(p)]
        if var[0] is None:
            conv += CONV_NOT_PD
        else:
            with np.errstate(all="ignore"):
                out["sd"][i] = np.sqrt(np.array([var[k][k] for k in range(p)]))
        out["map"][i], out["iter"][i], out["conv"][i], out["start"][i], out["objective"][i] = b, iters, conv, start, F
        mc, sc = b[coef], out["sd"][i, coef]
        with np.errstate(all="ignore"):
            out["fsr"][i] = pnorm_both(vexp, np.array([-(np.abs(mc) / sc)]))[0][0]
            if threshold is not None:
                u = np.array([(threshold - mc) / sc, (-threshold - mc) / sc])
                lo, up = pnorm_both(vexp, u)
                out["thresh"][i] = lo[0] - lo[1] if mc >= 0.0 else up[1] - up[0]
    return out


def svalue(fsr):
    """apeglm::svalue as R/lfcShrink.R:523-528 restates it: the cumulative mean of the sorted false sign rates, NA last"""
    fsr = np.asarray(fsr, np.float64)
    order = np.argsort(fsr, kind="stable")                       # sort(lfsr, na.last = TRUE): NaN sorts last in numpy too
    cm = np.cumsum(fsr[order]) / np.arange(1, fsr.size + 1)      # cumsum(lfsr.sorted) / seq_along(lfsr)
    rank = np.empty(fsr.size, np.int64)                          # rank(lfsr, ties.method = "first", na.last = TRUE)
    rank[order] = np.arange(fsr.size)
    return cm[rank]


def prior_scale(D, S, floor=1e-6, tol=1e-12, maxit=1000):
    """The adaptive scale of the prior from maximum-likelihood estimates D with standard errors S (natural log scale):
    the marginal-likelihood estimate of A under D_i ~ N(0, A + S_i^2) (Efron and Morris) by the fixed point
    A <- sum w_i (D_i^2 - S_i^2) / sum w_i, w_i = 1 / (S_i^2 + A)^2, every sum by math.fsum; returns
    min(max(sqrt(A), floor), 1)"""
    import math
    D, S = np.asarray(D, np.float64), np.asarray(S, np.float64)
    keep = np.isfinite(D) & np.isfinite(S)
    d2, s2 = D[keep] * D[keep], S[keep] * S[keep]
    if d2.size == 0:
        raise ValueError("no row with a finite estimate and standard error: the prior scale cannot be estimated")
    excess = d2 - s2
    A = max(math.fsum(excess.tolist()) / d2.size, 0.0)                           # the moment estimate
    A = A if A > 0.0 else floor * floor
    for _ in range(maxit):
        # (elementwise IEEE operations, each rounded once; only the two sums are exact)
        w = 1.0 / ((s2 + A) * (s2 + A))
        new = math.fsum((w * excess).tolist()) / math.fsum(w.tolist())
        if not new > 0.0:
            A = 0.0
            break
        done = abs(new - A) <= tol * new
        A = new
        if done:
            break
    return min(max(math.sqrt(A), floor), 1.0)
