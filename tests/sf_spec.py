"""The arithmetic specification of estimateSizeFactors stated in numpy: the reference for the
size-factor tests.  Not a test itself.  log / exp are the oracle's (oracle.unary, bit-equal to the device's dlog / dexp,
tests/test_gpu_math.py), the row sums are explicit wave-order sums, the median is np.sort and the two middle values.
Shares no code with the product (deseq2_amd.engine.HostEngine.size_factors)."""
import numpy as np


def wave_sum(T):
    """wave-order sum along the last axis: partial l adds items l, l + 64, ... in order from 0.0, then the butterfly
    v[l] += v[l ^ off] for off = 1, 2, 4, 8, 16, 32"""
    T = np.asarray(T, np.float64)
    m = T.shape[-1]
    part = np.zeros(T.shape[:-1] + (64,))
    for j0 in range(0, m, 64):
        blk = T[..., j0:j0 + 64]
        part[..., : blk.shape[-1]] = part[..., : blk.shape[-1]] + blk
    idx = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[..., idx ^ off]
    return part[..., 0]


def _log(O, v):
    """log with the edges spelled out: log(0) = -Inf, log(Inf) = Inf, log(< 0) = log(NaN) = NaN"""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, np.nan)
    ok = (v > 0) & (v < np.inf)
    if ok.any():
        out[ok] = O.unary("log", np.ascontiguousarray(v[ok]))
    out[v == 0] = -np.inf
    out[v == np.inf] = np.inf
    return out


def _exp(O, v):
    v = np.asarray(v, np.float64)
    out = np.array(v, dtype=np.float64, copy=True)        # NaN and +Inf stay
    ok = np.isfinite(v)
    if ok.any():
        out[ok] = O.unary("exp", np.ascontiguousarray(v[ok]))
    out[v == -np.inf] = 0.0
    return out


def size_factors(O, counts, type="ratio", geoMeans=None, control=None, normMatrix=None):
    """returns dict(sizeFactors, loggeomeans, counts_selected (per sample), status[, normalizationFactors]).
    control: boolean mask over the genes or None."""
    K = np.asarray(counts, np.float64)
    n, m = K.shape
    with np.errstate(all="ignore"):
        V = K if normMatrix is None else K / np.asarray(normMatrix, np.float64)
        if type == "poscounts":
            pos = K > 0
            s = wave_sum(np.where(pos, _log(O, np.where(pos, K, 1.0)), 0.0))
            lgm = np.where(pos.any(axis=1), _log(O, _exp(O, s / m)), -np.inf)
            stabilize = True
        elif geoMeans is not None:
            lgm = _log(O, np.asarray(geoMeans, np.float64))
            stabilize = True
        else:
            lgm = wave_sum(_log(O, V)) / m
            stabilize = False
        status = 1 if np.isinf(lgm).all() else 0
        use = np.isfinite(lgm)
        if control is not None:
            use = use & np.asarray(control, bool)
        sf = np.full(m, np.nan)
        cnt = np.zeros(m, dtype=np.int64)
        for j in range(m):
            sel = use & (V[:, j] > 0)
            c = cnt[j] = int(sel.sum())
            if c == 0:
                continue
            d = np.sort(_log(O, V[sel, j]) - lgm[sel])
            med = d[c // 2] if c % 2 else (d[c // 2 - 1] + d[c // 2]) * 0.5
            sf[j] = _exp(O, np.array([med]))[0]
        if stabilize:
            ls = _log(O, sf)
            s = 0.0
            for j in range(m):                   # mean(log(sf)): serial, in sample order
                s = s + ls[j]
            sf = sf / _exp(O, np.array([s / m]))[0]
        out = {"sizeFactors": sf, "loggeomeans": lgm, "counts_selected": cnt, "status": status}
        if normMatrix is not None:
            nf = np.asarray(normMatrix, np.float64) * sf[None, :]
            g = _exp(O, wave_sum(_log(O, nf)) / m)
            out["normalizationFactors"] = nf / g[:, None]
    return out
