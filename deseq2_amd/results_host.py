"""results() in plain numpy: the host statement of what csrc/results.hip computes, used by
HostEngine.  `vexp` is the engine's exp (the pinned arithmetic of csrc/dsq_math.hpp), every other operation is IEEE and
written in the order the kernels run it, so the two engines give the same bits."""
import numpy as np

ALT = ("greaterAbs", "lessAbs", "greater", "less", "greaterAbs2014")
COLUMNS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue")


def _horner(lead, x, num, den, n):
    xnum, xden = lead * x, x
    for i in range(n):
        xnum = (xnum + num[i]) * x
        xden = (xden + den[i]) * x
    return xnum, xden


_A = (2.2352520354606839287, 161.02823106855587881, 1067.6894854603709582, 18154.981253343561249)
_B = (47.20258190468824187, 976.09855173777669322, 10260.932208618978205, 45507.789335026729956)
_C = (0.39894151208813466764, 8.8831497943883759412, 93.506656132177855979, 597.27027639480026226, 2494.5375852903726711,
      6848.1904505362823326, 11602.651437647350124, 9842.7148383839780218)
_D = (22.266688044328115691, 235.38790178262499861, 1519.377599407554805, 6485.558298266760755, 18615.571640885098091,
      34900.952721145977266, 38912.003286093271411, 19685.429676859990727)
_P = (0.21589853405795699, 0.1274011611602473639, 0.022235277870649807, 0.001421619193227893466, 2.9112874951168792e-5)
_Q = (1.28426009614491121, 0.468238212480865118, 0.0659881378689285515, 0.00378239633202758244, 7.29751555083966205e-5)


def pnorm_both(vexp, z):
    """(pnorm(z), pnorm(z, lower.tail = FALSE)): Cody's algorithm as R's pnorm_both runs it, one pass for both tails"""
    z = np.asarray(z, np.float64)
    shape = z.shape
    z = z.ravel()
    lower, upper = np.full(z.shape, np.nan), np.full(z.shape, np.nan)
    ex = lambda v: vexp(np.ascontiguousarray(v)) if v.size else v
    with np.errstate(all="ignore"):
        y = np.abs(z)
        c = y <= 0.67448975
        if c.any():
            zc = z[c]
            xnum, xden = _horner(0.065682337918207449113, zc * zc, _A, _B, 3)
            tiny = np.abs(zc) <= 5.5511151231257827e-17
            xnum[tiny], xden[tiny] = 0.0, 0.0
            temp = zc * (xnum + _A[3]) / (xden + _B[3])
            lower[c], upper[c] = 0.5 + temp, 0.5 - temp
        tail = np.zeros(z.shape)
        m = (y > 0.67448975) & (y <= 5.656854249492380195206754896838)
        f = (y > 5.656854249492380195206754896838) & (y < 38.5)
        for sel, far in ((m, False), (f, True)):
            if not sel.any():
                continue
            ys = y[sel]
            if far:
                xsq = 1.0 / (ys * ys)
                xnum, xden = _horner(0.02307344176494017303, xsq, _P, _Q, 4)
                temp = xsq * (xnum + _P[4]) / (xden + _Q[4])
                temp = (0.398942280401432677939946059934 - temp) / ys
            else:
                xnum, xden = _horner(1.0765576773720192317e-8, ys, _C, _D, 7)
                temp = (xnum + _C[7]) / (xden + _D[7])
            t = np.trunc(ys * 16.0) / 16.0
            dl = (ys - t) * (ys + t)
            tail[sel] = ex(-t * t * 0.5) * ex(-dl * 0.5) * temp
        rest = 1.0 - tail
        pos, neg = (y > 0.67448975) & (z > 0), (y > 0.67448975) & ~(z > 0)
        lower[pos], upper[pos] = rest[pos], tail[pos]
        lower[neg], upper[neg] = tail[neg], rest[neg]
    return lower.reshape(shape), upper.reshape(shape)


def _pnorm_sd(vexp, x, se):
    """pnorm(x, sd = se) with the rules of R's pnorm5 around the quotient"""
    q = x / se
    out = pnorm_both(vexp, np.where(np.isfinite(q), q, 0.0))[0]
    out = np.where((se == 0) | ~np.isfinite(q), np.where(x < 0, 0.0, 1.0), out)
    return np.where(np.isnan(x) | np.isnan(se) | (se < 0), np.nan, out)


def _pmax(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, b))


def _pmin(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, b))


def threshold_tests(vexp, LFC, SE, T, altHypothesis, pt=None):
    """newStat, newPvalue of R/results.R:484-515 (normal distribution).  pt = (lower, upper), two functions of q: the same
    tests under Student's t with the rows' degrees of freedom bound into them (:477-515 with useT; plain quotients, gene i
    with its own df -- DESIGN.md section 15)"""
    up = (lambda q: pnorm_both(vexp, q)[1]) if pt is None else pt[1]
    with np.errstate(all="ignore"):
        if altHypothesis == "greaterAbs" and pt is not None:
            return LFC / SE, pt[0]((-np.abs(LFC) + T) / SE) + pt[0]((-np.abs(LFC) - T) / SE)
        if altHypothesis == "greaterAbs":
            return LFC / SE, _pnorm_sd(vexp, -np.abs(LFC) + T, SE) + _pnorm_sd(vexp, -np.abs(LFC) - T, SE)
        if altHypothesis == "greaterAbs2014":
            q = (np.abs(LFC) - T) / SE
            sign = np.where(np.isnan(LFC), np.nan, np.where(LFC > 0, 1.0, np.where(LFC < 0, -1.0, 0.0)))
            return sign * _pmax(q, 0.0), _pmin(1.0, 2.0 * up(q))
        if altHypothesis == "lessAbs":
            qa, qb = (T - LFC) / SE, (LFC + T) / SE
            return _pmin(_pmax(qa, 0.0), _pmax(qb, 0.0)), _pmax(up(qa), up(qb))
        if altHypothesis == "greater":
            q = (LFC - T) / SE
            return _pmax(q, 0.0), up(q)
        if altHypothesis == "less":
            return _pmin((LFC + T) / SE, 0.0), up((-T - LFC) / SE)
    raise ValueError("altHypothesis should be one of %s" % ", ".join(ALT))


def results_table(vexp, lfc, se, stat, pvalue, baseMean, replace, na_mask, lfcThreshold, altHypothesis, pt=None):
    """the five columns of R/results.R:443-575 from the coefficient's columns (pt: see threshold_tests)"""
    lfc, se = np.array(lfc, np.float64), np.array(se, np.float64)
    stat, pvalue = np.array(stat, np.float64), np.array(pvalue, np.float64)
    bm = np.array(baseMean, np.float64)
    if not (lfcThreshold == 0 and altHypothesis == "greaterAbs"):
        stat, pvalue = (np.array(v) for v in threshold_tests(vexp, lfc, se, float(lfcThreshold), altHypothesis, pt))
    if na_mask is not None:
        pvalue[np.asarray(na_mask) == 1] = np.nan
    if replace is not None:
        with np.errstate(invalid="ignore"):
            z = (np.asarray(replace) == 1) & (bm == 0)
        lfc[z], se[z], stat[z], pvalue[z] = 0.0, 0.0, 0.0, 1.0
    return dict(zip(COLUMNS, (bm, lfc, se, stat, pvalue)))


def quantile7(filter, theta):
    s = np.sort(np.asarray(filter, np.float64))
    out = np.empty(len(theta))
    for k, t in enumerate(np.asarray(theta, np.float64)):
        h = (s.size - 1) * t
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        g = h - lo
        with np.errstate(all="ignore"):
            out[k] = s[lo] if (g == 0 or s[hi] == s[lo]) else (1.0 - g) * s[lo] + g * s[hi]
    return out


def filtered_p(filter, p, theta, alpha):
    """filtered_p (R/results.R:721-740) with p.adjust(., "BH"), all cutoffs from one sort of the p-values (the
    formulation of csrc/results.hip).  theta None: one column, every non-NA p-value adjusted.
    Returns filtPadj (n x K), numRej, cutoffs."""
    p = np.asarray(p, np.float64)
    n = p.size
    if theta is None:
        cutoffs = np.array([-np.inf])
    else:
        filter = np.asarray(filter, np.float64)
        if np.isnan(filter).any():
            raise ValueError("filter holds NA")
        cutoffs = quantile7(filter, theta)
    rows = np.where(~np.isnan(p))[0]
    rows = rows[np.argsort(p[rows], kind="stable")]
    ps = p[rows]
    out = np.full((n, len(cutoffs)), np.nan, order="F")
    for k, c in enumerate(cutoffs):
        use = np.ones(rows.size, bool) if theta is None else filter[rows] >= c
        r = np.cumsum(use)
        if r.size == 0 or r[-1] == 0:
            continue
        with np.errstate(all="ignore"):
            v = np.where(use, (float(r[-1]) / np.maximum(r, 1)) * ps, np.inf)
        suf = np.minimum.accumulate(v[::-1])[::-1]
        out[rows[use], k] = np.minimum(1.0, suf)[use]
    with np.errstate(invalid="ignore"):
        numRej = (out < alpha).sum(axis=0).astype(np.int32)
    return out, numRej, cutoffs
