"""The arithmetic specification of unmix() stated in numpy: the reference for the unmix tests.  Not a
test itself.  log is the oracle's (bit-equal to the device's dlog, tests/test_gpu_math.py), sqrt is IEEE,
asinh(z) = log(z + sqrt(z z + 1)); +, -, *, / are IEEE, every operation rounded once, in the order written here.  Shares no
code with the product (deseq2_amd/csrc/unmix.hip, deseq2_amd.engine.HostEngine.unmix_fit, core.unmix).

The objective is R's (R/helper.R:93-95, :106-108) on R's box (:98, :111) from R's start; the optimiser is the library's own.

Every sum over the genes: thread t of T adds the genes t, t + T, ... in order from 0.0; the 64 lanes of a wave combine by the
butterfly of sf_spec.wave_sum; the T / 64 wave results add in wave order."""
import numpy as np

from tests.sf_spec import _log

T = 256                                              # kUnmixThreads of csrc/capi.hpp (dsq_unmix_block_threads)
LN2 = float.fromhex("0x1.62e42fefa39efp-1")          # R's log(2)
LN4 = float.fromhex("0x1.62e42fefa39efp+0")          # R's log(4)
HI = 100.0
LAMBDA0, LAMBDA_MIN = 1e-3, 1e-9
REL_TOL = 1e-10
ABS_FLOOR = 1e-8
MAX_REJECT = 30
MAX_K = 16


def lower_bound(alpha):
    return 1e-6 if alpha is not None else 0.0


def block_sum(terms):
    """the sum over axis 0 (genes) of an (n, C) array in the order of the kernel; returns C values"""
    terms = np.asarray(terms, np.float64)
    n, C = terms.shape
    rows = -(-n // T)
    pad = np.zeros((rows * T, C))
    pad[:n] = terms
    pad = pad.reshape(rows, T, C)
    part = np.zeros((T, C))
    for r in range(rows):                            # (a partial never holds -0.0: adding the +0.0 of the padding changes nothing)
        part = part + pad[r]
    part = part.reshape(T // 64, 64, C)
    idx = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[:, idx ^ off, :]
    tot = part[0, 0]
    for w in range(1, T // 64):
        tot = tot + part[w, 0]
    return tot


def v_and_slope(O, q, alpha, shift):
    """v(q) and v'(q), elementwise"""
    q = np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        if alpha is not None:
            la = float(_log(O, np.array([alpha]))[0])
            z = np.sqrt(alpha * q)
            s = np.sqrt(z * z + 1.0)
            v = ((2.0 * _log(O, z + s) - la) - LN4) / LN2
            d = alpha / ((z * s) * LN2)
        else:
            t = q + shift
            v = _log(O, t)
            d = 1.0 / t
    return v, d


def system(O, vx, pure, p, alpha, shift, power):
    """(L, A (k x k, lower triangle filled), b) at p for one sample whose transformed target is vx"""
    n, k = pure.shape
    with np.errstate(all="ignore"):
        f = pure[:, 0] * p[0]
        for j in range(1, k):
            f = f + pure[:, j] * p[j]
        vf, d = v_and_slope(O, f, alpha, shift)
        r = vx - vf
        ar = np.abs(r)
        cols = [ar if power == 1 else r * r]
        live = np.isfinite(d)
        w = 1.0 / np.fmax(ar, ABS_FLOOR) if power == 1 else np.ones(n)
        J = d[:, None] * pure
        wJ = w[:, None] * J
        for i in range(k):
            cols.append(np.where(live, wJ[:, i] * r, 0.0))
        for i in range(k):
            for j in range(i + 1):
                cols.append(np.where(live, wJ[:, i] * J[:, j], 0.0))
        tot = block_sum(np.stack(cols, axis=1))
    A = np.zeros((k, k))
    c = 1 + k
    for i in range(k):
        for j in range(i + 1):
            A[i, j] = tot[c]
            c += 1
    return float(tot[0]), A, tot[1:1 + k].copy()


def solve(A, b, lam, fixed):
    """(A_FF + lam diag(A_FF)) d_F = b_F, d = 0 on the fixed coordinates: Cholesky row by row, every inner product
    subtracted term by term in ascending order.  None: a pivot that is not positive."""
    k = b.size
    Lo = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i + 1):
                if fixed[i] or fixed[j]:
                    s = np.float64(1.0 if i == j else 0.0)
                else:
                    s = np.float64(A[i, j])
                    if i == j:
                        s = s + np.float64(lam) * s
                for t in range(j):
                    s = s - Lo[i, t] * Lo[j, t]
                if i == j:
                    if not s > 0.0:
                        return None
                    Lo[i, i] = np.sqrt(s)
                else:
                    Lo[i, j] = s / Lo[j, j]
        d = np.zeros(k)
        for i in range(k):
            s = np.float64(0.0 if fixed[i] else b[i])
            for t in range(i):
                s = s - Lo[i, t] * d[t]
            d[i] = s / Lo[i, i]
        for i in range(k - 1, -1, -1):
            s = d[i]
            for t in range(i + 1, k):
                s = s - Lo[t, i] * d[t]
            d[i] = s / Lo[i, i]
    return d


def step(A, b, lam, p, lo, active_set=True):
    """the step on the free set: a coordinate on a bound whose step points outward is fixed and the system solved again"""
    k = p.size
    fixed = [not A[j, j] > 0.0 for j in range(k)]
    d = None
    for _ in range(k + 1):
        d = solve(A, b, lam, fixed)
        if d is None or not active_set:
            return d
        more = [not fixed[j] and ((p[j] <= lo and d[j] < 0.0) or (p[j] >= HI and d[j] > 0.0)) for j in range(k)]
        if not any(more):
            break
        fixed = [a or c for a, c in zip(fixed, more)]
    return d


def fit_sample(O, vx, pure, alpha, shift, power, maxit=200, lo=None, active_set=True, loss_power=None):
    """one sample.  Returns (p, loss, iter, flag).  lo / active_set / loss_power: switches for the mutants of the tests only."""
    k = pure.shape[1]
    lo = lower_bound(alpha) if lo is None else lo
    lp = power if loss_power is None else loss_power
    p = np.ones(k)
    L, A, b = system(O, vx, pure, p, alpha, shift, lp)
    if not np.isfinite(L):
        return np.full(k, np.nan), np.nan, 0, 2
    lam = LAMBDA0
    it, flag = 0, 1
    while it < maxit:
        it += 1
        rej = 0
        accepted = False
        while True:
            d = step(A, b, lam, p, lo, active_set)
            if d is not None:
                with np.errstate(all="ignore"):
                    pt = p + d
                pt = np.where(pt < lo, lo, pt)
                pt = np.where(pt > HI, HI, pt)
                if (pt == p).all():
                    break
                Lt, At, bt = system(O, vx, pure, pt, alpha, shift, lp)
                if Lt < L:
                    accepted = True
                    lam = max(lam * 0.25, LAMBDA_MIN)
                    break
            lam = 4.0 * lam
            rej += 1
            if rej >= MAX_REJECT:
                break
        if not accepted:
            flag = 0
            break
        rel = (L - Lt) / L
        p, L, A, b = pt, Lt, At, bt
        if rel < REL_TOL:
            flag = 0
            break
    return p, L, it, flag


def unmix_fit(O, x, pure, alpha=None, shift=None, power=1, maxit=200, **mutant):
    """dict(p m x k, loss m, iter m int32, flag m int32) for the n x m samples x and the n x k components pure"""
    x = np.asarray(x, np.float64)
    pure = np.ascontiguousarray(pure, np.float64)
    n, m = x.shape
    k = pure.shape[1]
    assert (alpha is None) != (shift is None) and power in (1, 2) and 2 <= k <= MAX_K
    vx, _ = v_and_slope(O, x, alpha, shift)
    out = {"p": np.zeros((m, k)), "loss": np.zeros(m), "iter": np.zeros(m, np.int32), "flag": np.zeros(m, np.int32)}
    for i in range(m):
        out["p"][i], out["loss"][i], out["iter"][i], out["flag"][i] = fit_sample(
            O, np.ascontiguousarray(vx[:, i]), pure, alpha, shift, power, maxit, **mutant)
    return out


def mix_of(p):
    """p / sum(p), the sum taken in coordinate order"""
    p = np.asarray(p, np.float64)
    s = p[:, 0].copy()
    for j in range(1, p.shape[1]):
        s = s + p[:, j]
    with np.errstate(all="ignore"):
        return p / s[:, None]


def loss_at(O, x_col, pure, p, alpha, shift, power):
    """L at p in plain numpy sums: for the checks that owe nothing to the summation order"""
    vx, _ = v_and_slope(O, x_col, alpha, shift)
    vf, _ = v_and_slope(O, pure @ p, alpha, shift)
    return float((np.abs(vx - vf) ** power).sum())
