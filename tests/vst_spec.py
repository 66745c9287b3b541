"""The arithmetic specification of the variance stabilizing transformation stated in numpy: the
reference for the VST tests.  Not a test itself.  log / log1p are the oracle's (oracle.unary, bit-equal to the device's
dlog / dlog1p, tests/test_gpu_math.py); sqrt, +, -, *, / are IEEE, every operation rounded once, in the order R evaluates
the expressions of R/vst.R.  Shares no code with the product (deseq2_amd.engine.HostEngine.vst_transform, core.vst)."""
import numpy as np

from tests.sf_spec import wave_sum

LN2 = float.fromhex("0x1.62e42fefa39efp-1")          # the double nearest to ln 2: R's log(2)
KINDS = ("parametric", "mean", "spline", "log2", "normalized")


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


def _log1p(O, v):
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, np.nan)
    ok = (v > -1) & (v < np.inf)
    if ok.any():
        out[ok] = O.unary("log1p", np.ascontiguousarray(v[ok]))
    out[v == np.inf] = np.inf
    return out


def asinh(O, x):
    """asinh for x >= 0 (NaN stays NaN) from log / log1p / sqrt, four ranges:
         x < 2^-28          x
         x <= 2             log1p(x + x^2 / (1 + sqrt(x^2 + 1)))
         x <= 2^28          log(2 x + 1 / (sqrt(x^2 + 1) + x))
         beyond             log(x) + ln2"""
    x = np.asarray(x, np.float64)
    out = np.array(x, copy=True)
    with np.errstate(all="ignore"):
        t = x * x
        r = np.sqrt(t + 1.0)
        mid = (x >= 2.0 ** -28) & (x <= 2.0)
        big = (x > 2.0) & (x <= 2.0 ** 28)
        huge = x > 2.0 ** 28
        if mid.any():
            out[mid] = _log1p(O, (x + t / (1.0 + r))[mid])
        if big.any():
            out[big] = _log(O, (2.0 * x + 1.0 / (r + x))[big])
        if huge.any():
            out[huge] = _log(O, x[huge]) + LN2
    return out


def spline_eval(table, u):
    """S(u) of the table x | y | b | c | d (5 x K), as R's spline_eval walks it: i = 0, j = K; while j > i + 1: k = (i + j) / 2,
    u < x_k ? j = k : i = k -- the largest i with x_i <= u, 0 left of the first knot, K - 1 for a NaN; then Horner
    y + dx (b + dx (c + dx d)) with dx = u - x_i"""
    x, y, b, c, d = np.asarray(table, np.float64).reshape(5, -1)
    u = np.asarray(u, np.float64)
    lo = np.zeros(u.shape, dtype=np.int64)
    hi = np.full(u.shape, x.size, dtype=np.int64)
    with np.errstate(all="ignore"):
        while (hi > lo + 1).any():
            live = hi > lo + 1
            mid = (lo + hi) // 2
            left = live & (u < x[np.minimum(mid, x.size - 1)])
            hi = np.where(left, mid, hi)
            lo = np.where(live & ~left, mid, lo)
        dx = u - x[lo]
        return y[lo] + dx * (b[lo] + dx * (c[lo] + dx * d[lo]))


def normalized(counts, nf):
    """q_ij = k_ij / nf_ij, one division; nf: m size factors or an n x m matrix"""
    K = np.asarray(counts, np.float64)
    nf = np.asarray(nf, np.float64)
    with np.errstate(all="ignore"):
        return K / (nf[None, :] if nf.ndim == 1 else nf)


def transform(O, counts, nf, kind, asymptDisp=None, extraPois=None, alpha=None, pc=1.0, table=None, eta=None, xi=None):
    q = normalized(counts, nf)
    with np.errstate(all="ignore"):
        if kind == "parametric":
            a, e = float(asymptDisp), float(extraPois)
            ope = 1.0 + e
            aq = a * q
            s1 = ope + (2.0 * a) * q
            v = aq * (ope + aq)
            return _log(O, (s1 + 2.0 * np.sqrt(v)) / (4.0 * a)) / LN2
        if kind == "mean":
            al = float(alpha)
            la, l4 = _log(O, np.array([al]))[0], _log(O, np.array([4.0]))[0]
            return ((2.0 * asinh(O, np.sqrt(al * q)) - la) - l4) / LN2
        if kind == "spline":
            return float(eta) * spline_eval(table, asinh(O, q)) + float(xi)
        if kind == "log2":
            return _log(O, q + float(pc)) / LN2
        if kind == "normalized":
            return q
    raise ValueError(kind)


def row_stats(counts, nf):
    """rowMeans and row maxima of q: the mean is the wave-order sum over the samples divided by m, the maximum exact, NaN
    if the row holds one"""
    q = normalized(counts, nf)
    with np.errstate(all="ignore"):
        mean = wave_sum(q) / q.shape[1]
        mx = np.where(np.isnan(q).any(axis=1), np.nan, np.nanmax(np.where(np.isnan(q), -np.inf, q), axis=1))
    return mean, mx


def vst_subset(baseMean, nsub):
    """the rows vst() fits the trend on (R/vst.R:239-250), 0-based indices into the full object, in the order R visits them:
    rows with mean > 5, order() = ascending with ties by index, positions round(seq(1, L, length = nsub)) with Python's
    round() (half to even, as R's)"""
    bm = [float(v) for v in np.asarray(baseMean, np.float64)]
    if len(bm) < nsub:
        raise ValueError("less than 'nsub' rows")
    keep = [i for i, v in enumerate(bm) if v > 5]
    if len(keep) < nsub:
        raise ValueError("less than 'nsub' rows with mean normalized count > 5")
    ordered = sorted(keep, key=lambda i: (bm[i], i))
    L = len(ordered)
    out = []
    for t in range(nsub):
        pos = 1.0 if t == 0 else (float(L) if t == nsub - 1 else 1.0 + t * ((L - 1) / (nsub - 1)))
        out.append(ordered[round(pos) - 1])
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------- derived error bounds
U = 2.0 ** -52
ASINH_ULPS = 8.0          # asserted against mpmath by tests/test_vst_cpu.py::test_asinh_definition_against_mpmath


def spec_bound(kind, res, A=None, la=0.0):
    """Distance of the specification (and of the host statement: libm's log / log2 / asinh are within an ulp like the
    oracle's log / log1p) from the exact value of the expression at the same q, from the count of roundings.
    parametric: the argument of the logarithm is a sum of positive terms (e > -1) built by 8 operations, relative error
      <= 8 * 2^-53 = 2^-50, which the logarithm turns into an absolute one; the logarithm adds an ulp (2^-52 |log|), the
      division by the double nearest ln 2 scales absolute errors by 1.4427 < 1.5 and adds half an ulp of the result and the
      2^-54 of the constant: 1.5 * 2^-50 + |result| * 2^-51.  log2(q + pc): two operations in the argument, same form.
    mean: asinh within ASINH_ULPS ulps (asserted below), one more from the rounded sqrt(alpha q); doubling is exact; log(alpha)
      and log(4) within an ulp; the two subtractions round at the size of their results:
      2^-52 (18 |A| + 2 |log alpha| + 2.1) before the division, A = asinh: 1.5 * 2^-52 (20 |A| + 4 |log alpha| + 4) + |result| 2^-51."""
    res = np.abs(np.asarray(res, np.float64))
    if kind == "mean":
        return 1.5 * U * (20 * np.abs(A) + 4 * abs(la) + 4) + res * 2.0 ** -51
    return 1.5 * 2.0 ** -50 + res * 2.0 ** -51


def spline_bound(table, eta, xi, u, res):
    """The spline formula eta S(u) + xi at u = asinh(q): u carries up to ASINH_ULPS + 1 ulps between any two of {libm, the
    asinh of the specification, the exact value}; S passes that on with its slope, bounded by 1.25 times the largest |S'|
    at nine points of every piece that holds a u (S' is a parabola on a piece); Horner's six operations round at the size
    of the partial sums T = |y| + |dx| (|b| + |dx| (|c| + |dx| |d|)); the final multiply-add rounds at |eta S| + |result|."""
    x, y, b, c, d = np.asarray(table, np.float64).reshape(5, -1)
    u = np.asarray(u, np.float64)
    i = np.clip(np.searchsorted(x, u, side="right") - 1, 0, x.size - 1)
    dx = np.abs(u - x[i])
    T = np.abs(y[i]) + dx * (np.abs(b[i]) + dx * (np.abs(c[i]) + dx * np.abs(d[i])))
    lo = np.minimum(u.min(), x[0])
    hi = np.maximum(u.max(), x[-1])
    edges = np.concatenate([[lo], x[1:], [hi]])
    slope = 0.0
    for f in np.linspace(0, 1, 9):
        pt = edges[:-1] + f * (edges[1:] - edges[:-1])
        h = pt - x
        slope = max(slope, float(np.abs(b + h * (2 * c + 3 * d * h)).max()))
    return abs(eta) * (1.25 * slope * (ASINH_ULPS + 1) * U * np.abs(u) + 4 * U * T) + U * (abs(eta) * T + np.abs(res) + abs(xi))
