"""The solve of estimateSizeFactors(type = "iterate") (R/core.R:2600-2611) on the host: the iteration of csrc/sf_iterate.hip
 in numpy, the same operations in the same order, so that HostEngine.sf_iterate_solve and
dsq_sf_iterate_dev agree to the bit.  The row log likelihoods are the engine's nbinomLogLike (K' + the wave-order sum of
the mu-dependent part), exp / log the engine's; everything else is IEEE arithmetic in the order written here."""
import numpy as np

SLICE_GENES = 64            # dsq_sf_iterate_slice_genes(): the consecutive genes of one partial column sum
CUT_THREADS = 1024        # the workgroup that adds F: thread t takes the rows t, t + 1024, ...
MAX_TRIALS = 30
ARMIJO = 1e-4
RELTOL = 1e-10


def _serial(v):
    """the sum of v in index order, from 0.0"""
    return float(np.cumsum(np.r_[0.0, np.asarray(v, np.float64)])[-1])


def _exp(vexp, v):
    """exp with the edges spelled out (sf_exp of csrc/dsq_math.hpp): NaN and +Inf stay, exp(-Inf) = 0"""
    v = np.asarray(v, np.float64)
    out = np.array(v, copy=True)
    ok = np.isfinite(v)
    if ok.any():
        out[ok] = vexp(np.ascontiguousarray(v[ok]))
    out[v == -np.inf] = 0.0
    return out


def _log(vlog, v):
    """log with the edges spelled out (sf_log): log(0) = -Inf, log(Inf) = Inf, log(< 0) = log(NaN) = NaN"""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, np.nan)
    ok = (v > 0) & (v < np.inf)
    if ok.any():
        out[ok] = vlog(np.ascontiguousarray(v[ok]))
    out[v == 0] = -np.inf
    out[v == np.inf] = np.inf
    return out


def _wave64(part):
    """the butterfly over the last axis of 64 partial sums"""
    idx = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[..., idx ^ off]
    return part[..., 0]


def cut_and_sum(L, rows, Q):
    """(cut, F, nkept) of the row log likelihoods L over the flagged rows: quantile(L[rows], Q) of type 7, the rows strictly
    above it, and their sum in the order of sfi_cut_kernel.  A NaN among them: F is NaN."""
    v = L[rows]
    if v.size == 0:
        return np.nan, 0.0, 0
    if np.isnan(v).any():
        return np.nan, np.nan, 0
    s = np.sort(v)
    h = (v.size - 1) * Q
    lo = int(np.floor(h))
    g = h - lo
    cut = s[lo]
    with np.errstate(all="ignore"):
        if g != 0.0 and s[lo + 1] != s[lo]:
            cut = (1.0 - g) * s[lo] + g * s[lo + 1]
        kept = rows & (L > cut)
        n = L.size
        pad = (-n) % CUT_THREADS
        c = np.r_[np.where(kept, L, 0.0), np.zeros(pad)].reshape(-1, CUT_THREADS)
        part = np.zeros(CUT_THREADS)
        for blk in c:
            part = part + blk
        w = _wave64(part.reshape(-1, 64))
        F = w[0]
        for x in w[1:]:
            F = F + x
    return float(cut), float(F), int(kept.sum())


def solve(loglike, vexp, vlog, counts, mu, sf, disp, rows, Q, maxit, slice_genes):
    """loglike(K, mu, disp) -> the row sums of the log density; counts / mu n x m, sf m, disp n, rows n flags.
    Returns dict(s, sf, F, iter, evals, flag)."""
    K = np.asarray(counts, np.float64)
    n, m = K.shape
    rows = np.asarray(rows) != 0
    sf = np.asarray(sf, np.float64)
    a = np.where(rows, np.asarray(disp, np.float64), 0.0)
    G = int(slice_genes)
    with np.errstate(all="ignore"):
        q = np.asarray(mu, np.float64) / sf[None, :]
        Kr, qr, ar = np.ascontiguousarray(K[rows]), q[rows], np.ascontiguousarray(a[rows])

        def evaluate(e):
            L = np.full(n, np.nan)
            if Kr.shape[0]:
                L[rows] = np.asarray(loglike(Kr, qr * e[None, :], ar)).reshape(-1)
            return (L,) + cut_and_sum(L, rows, Q)

        def direction(L, cut, e):
            kept = rows & (L > cut)
            g, h = np.zeros(m), np.zeros(m)
            for b in range(0, n, G):
                pg, ph = np.zeros(m), np.zeros(m)
                for i in b + np.nonzero(kept[b:b + G])[0]:
                    mui = q[i] * e
                    opm = 1.0 + a[i] * mui
                    pg = pg + (K[i] - mui) / opm
                    ph = ph + (mui * (1.0 + a[i] * K[i])) / (opm * opm)
                g, h = g + pg, h + ph
            lam = _serial(g / h) / _serial(1.0 / h)
            d = (g - lam) / h
            return d, _serial(g * d)

        ls = _log(vlog, sf)
        s = ls - _serial(ls) / m
        e = _exp(vexp, s)
        L, cut, F, nkept = evaluate(e)
        it, evals = 0, 1
        if not np.isfinite(F):
            flag = 2
        elif nkept == 0:
            flag = 0
        else:
            while True:
                if it >= maxit:
                    flag = 1
                    break
                it += 1
                d, gd = direction(L, cut, e)
                t, accepted = 1.0, False
                for _ in range(MAX_TRIALS):
                    u = s + t * d
                    st = u - _serial(u) / m
                    et = _exp(vexp, st)
                    Lt, cutt, Ft, _ = evaluate(et)
                    evals += 1
                    if Ft >= F + (ARMIJO * t) * gd:
                        accepted = True
                        break
                    t = 0.5 * t
                if not accepted:
                    flag = 0 if gd <= RELTOL * abs(F) else 1
                    break
                gain = Ft - F
                s, e, L, cut, F = st, et, Lt, cutt, Ft
                if gain <= RELTOL * abs(F):
                    flag = 0
                    break
    return {"s": s, "sf": e, "F": float(F), "iter": it, "evals": evals, "flag": flag}
