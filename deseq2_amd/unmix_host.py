"""unmix() on the host: the iteration of csrc/unmix.hip in numpy over an engine's log, the same
operations in the same order, so that HostEngine.unmix_fit and dsq_unmix_dev agree to the bit.

Per sample: minimise L(p) = sum_g |v(x_g) - v(sum_j pure_gj p_j)|^power over [lo, 100]^k from p = 1 by a projected
Levenberg-Marquardt iteration on the reweighted Gauss-Newton system; every sum over the genes in the order of the kernel
(thread t of THREADS adds genes t, t + THREADS, ...; xor butterfly over the 64 lanes; waves in order)."""
import numpy as np

THREADS = 256                      # kUnmixThreads of csrc/capi.hpp
MAX_K = 16                         # DSQ_UNMIX_MAX_K
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LN4 = float.fromhex("0x1.62e42fefa39efp+0")
UPPER = 100.0
_LANES = np.arange(64)


class Transform:
    """v and v' of one call: alpha (the negative binomial form, lower bound 1e-6) or shift (the shifted log, lower bound 0)"""

    def __init__(self, vlog, alpha=None, shift=None):
        self.vlog = vlog
        self.alpha, self.shift = alpha, shift
        self.lo = 1e-6 if alpha is not None else 0.0
        self.la = float(self.log(np.array([alpha]))[0]) if alpha is not None else 0.0

    def log(self, v):
        v = np.asarray(v, np.float64)
        out = np.full(v.shape, np.nan)
        ok = (v > 0) & (v < np.inf)
        if ok.any():
            out[ok] = self.vlog(np.ascontiguousarray(v[ok]))
        out[v == 0] = -np.inf
        out[v == np.inf] = np.inf
        return out

    def __call__(self, q, slope=False):
        q = np.asarray(q, np.float64)
        with np.errstate(all="ignore"):
            if self.alpha is not None:
                z = np.sqrt(self.alpha * q)
                s = np.sqrt(z * z + 1.0)
                v = ((2.0 * self.log(z + s) - self.la) - LN4) / LN2
                return (v, self.alpha / ((z * s) * LN2)) if slope else v
            t = q + self.shift
            return (self.log(t), 1.0 / t) if slope else self.log(t)


def _gene_sums(cols):
    """kernel-order sums down the rows of an (n, C) array"""
    n, C = cols.shape
    part = np.zeros((THREADS, C))
    for g0 in range(0, n, THREADS):
        blk = cols[g0:g0 + THREADS]
        part[:blk.shape[0]] += blk
    part = part.reshape(THREADS // 64, 64, C)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[:, _LANES ^ off]
    total = part[0, 0]
    for w in range(1, THREADS // 64):
        total = total + part[w, 0]
    return total


def _system(tr, target, pure, p, power):
    """loss, packed lower triangle of A = J'WJ (row by row) and b = J'Wr at p"""
    k = pure.shape[1]
    with np.errstate(all="ignore"):
        f = pure[:, 0] * p[0]
        for j in range(1, k):
            f = f + pure[:, j] * p[j]
        vf, slope = tr(f, slope=True)
        r = target - vf
        absr = np.abs(r)
        J = slope[:, None] * pure
        wJ = J if power == 2 else (1.0 / np.fmax(absr, 1e-8))[:, None] * J
        tri_i, tri_j = np.tril_indices(k)                       # (0,0), (1,0), (1,1), ...: the packed order
        cols = np.concatenate([wJ[:, tri_i] * J[:, tri_j], wJ * r[:, None]], axis=1)
        cols[~np.isfinite(slope)] = 0.0
        sums = _gene_sums(np.concatenate([cols, (absr if power == 1 else r * r)[:, None]], axis=1))
    na = k * (k + 1) // 2
    return float(sums[-1]), sums[:na], sums[na:na + k]


def _cholesky_step(A, b, lam, fixed):
    """d with (A_FF + lam diag(A_FF)) d_F = b_F and d = 0 on `fixed` (identity rows); None when a pivot is not positive"""
    k = b.size
    at = lambda i, j: i * (i + 1) // 2 + j
    Lf = np.zeros(k * (k + 1) // 2)
    d = np.zeros(k)
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i + 1):
                if (fixed >> i) & 1 or (fixed >> j) & 1:
                    s = np.float64(i == j)
                else:
                    s = A[at(i, j)]
                    if i == j:
                        s = s + lam * s
                for t in range(j):
                    s = s - Lf[at(i, t)] * Lf[at(j, t)]
                if i == j:
                    if not s > 0.0:
                        return None
                    Lf[at(i, i)] = np.sqrt(s)
                else:
                    Lf[at(i, j)] = s / Lf[at(j, j)]
        for i in range(k):
            s = np.float64(0.0) if (fixed >> i) & 1 else b[i]
            for t in range(i):
                s = s - Lf[at(i, t)] * d[t]
            d[i] = s / Lf[at(i, i)]
        for i in reversed(range(k)):
            s = d[i]
            for t in range(i + 1, k):
                s = s - Lf[at(t, i)] * d[t]
            d[i] = s / Lf[at(i, i)]
    return d


def _free_set_step(A, b, lam, p, lo):
    k = p.size
    fixed = 0
    for j in range(k):
        if not A[j * (j + 1) // 2 + j] > 0.0:
            fixed |= 1 << j
    d = None
    for _ in range(k + 1):
        d = _cholesky_step(A, b, np.float64(lam), fixed)
        if d is None:
            return None
        more = 0
        for j in range(k):
            if not (fixed >> j) & 1 and ((p[j] <= lo and d[j] < 0.0) or (p[j] >= UPPER and d[j] > 0.0)):
                more |= 1 << j
        if not more:
            break
        fixed |= more
    return d


def fit_one(tr, target, pure, power, maxit):
    """(p, loss, iter, flag) of one sample; target = v(x) of the sample"""
    k = pure.shape[1]
    p = np.ones(k)
    loss, A, b = _system(tr, target, pure, p, power)
    if not np.isfinite(loss):
        return np.full(k, np.nan), np.nan, 0, 2
    lam, it = 1e-3, 0
    while it < maxit:
        it += 1
        trial = None
        for _ in range(30):
            d = _free_set_step(A, b, lam, p, tr.lo)
            if d is not None:
                with np.errstate(all="ignore"):
                    q = np.minimum(np.maximum(p + d, tr.lo), UPPER)          # (a NaN stays: the trial is then rejected)
                if np.array_equal(q, p):
                    break
                cand = _system(tr, target, pure, q, power)
                if cand[0] < loss:
                    trial = (q,) + cand
                    lam = max(lam * 0.25, 1e-9)
                    break
            lam = 4.0 * lam
        if trial is None:
            return p, loss, it, 0
        rel = (loss - trial[1]) / loss
        p, loss, A, b = trial
        if rel < 1e-10:
            return p, loss, it, 0
    return p, loss, it, 1


def unmix_fit(vlog, x, pure, alpha=None, shift=None, power=1, maxit=200):
    x = np.asarray(x, np.float64)
    pure = np.ascontiguousarray(pure, np.float64)
    m, k = x.shape[1], pure.shape[1]
    tr = Transform(vlog, alpha, shift)
    target = tr(x)
    out = {"p": np.empty((m, k)), "loss": np.empty(m), "iter": np.empty(m, np.int32), "flag": np.empty(m, np.int32)}
    for i in range(m):
        out["p"][i], out["loss"][i], out["iter"][i], out["flag"][i] = fit_one(
            tr, np.ascontiguousarray(target[:, i]), pure, int(power), int(maxit))
    return out


def mix_from_p(p):
    """mix <- mix / rowSums(mix) (R/helper.R:116), the row sum taken in column order"""
    p = np.asarray(p, np.float64)
    s = p[:, 0].copy()
    for j in range(1, p.shape[1]):
        s = s + p[:, j]
    with np.errstate(all="ignore"):
        return p / s[:, None]
