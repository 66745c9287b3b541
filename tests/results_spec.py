"""The arithmetic specification of results() stated in numpy: the reference for the results
tests.  Not a test itself.  exp is the oracle's (oracle.unary, bit-equal to the device's dexp, tests/test_gpu_math.py);
+, -, *, / are IEEE, every operation rounded once, in the order written here.  Shares no code with the product
(deseq2_amd.engine.HostEngine.results_table / filtered_p, core.results)."""
import numpy as np

ALT = ("greaterAbs", "lessAbs", "greater", "less", "greaterAbs2014")


def _exp(O, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return O.unary("exp", v) if v.size else v


# ---- pnorm: R's pnorm_both (W. J. Cody, Algorithm 715) for one tail -----------------------------------------------------
_A = (2.2352520354606839287, 161.02823106855587881, 1067.6894854603709582, 18154.981253343561249, 0.065682337918207449113)
_B = (47.20258190468824187, 976.09855173777669322, 10260.932208618978205, 45507.789335026729956)
_C = (0.39894151208813466764, 8.8831497943883759412, 93.506656132177855979, 597.27027639480026226, 2494.5375852903726711,
      6848.1904505362823326, 11602.651437647350124, 9842.7148383839780218, 1.0765576773720192317e-8)
_D = (22.266688044328115691, 235.38790178262499861, 1519.377599407554805, 6485.558298266760755, 18615.571640885098091,
      34900.952721145977266, 38912.003286093271411, 19685.429676859990727)
_P = (0.21589853405795699, 0.1274011611602473639, 0.022235277870649807, 0.001421619193227893466, 2.9112874951168792e-5,
      0.02307344176494017303)
_Q = (1.28426009614491121, 0.468238212480865118, 0.0659881378689285515, 0.00378239633202758244, 7.29751555083966205e-5)
_SQRT32 = 5.656854249492380195206754896838
_M_1_SQRT_2PI = 0.398942280401432677939946059934


def pnorm_both(O, z):
    """(lower, upper) tail of the standard normal at z.  Three ranges of y = |z|:
         y <= 0.67448975    temp = z R(z^2): lower = 0.5 + temp, upper = 0.5 - temp   (R(.) is 1 at y <= eps / 4)
         y <= sqrt(32)      tail = exp(-t^2 / 2) exp(-(y - t)(y + t) / 2) R(y), t = trunc(16 y) / 16
         y <  38.5          the same split exponential times (1 / sqrt(2 pi) - R(1 / y^2) / y^2) / y
         beyond             tail = 0
       and outside the central range (lower, upper) = (1 - tail, tail) for z > 0, (tail, 1 - tail) otherwise.  NaN stays."""
    z = np.asarray(z, np.float64)
    shape = z.shape
    z = z.ravel()
    lower, upper = np.full(z.shape, np.nan), np.full(z.shape, np.nan)
    with np.errstate(all="ignore"):
        y = np.abs(z)
        c = y <= 0.67448975
        if c.any():
            zc = z[c]
            xsq = zc * zc
            xnum = _A[4] * xsq
            xden = xsq
            for i in range(3):
                xnum = (xnum + _A[i]) * xsq
                xden = (xden + _B[i]) * xsq
            tiny = np.abs(zc) <= 5.5511151231257827e-17
            xnum[tiny] = 0.0
            xden[tiny] = 0.0
            temp = zc * (xnum + _A[3]) / (xden + _B[3])
            lower[c] = 0.5 + temp
            upper[c] = 0.5 - temp
        tail = np.zeros(z.shape)
        m = (y > 0.67448975) & (y <= _SQRT32)
        if m.any():
            ym = y[m]
            xnum = _C[8] * ym
            xden = ym
            for i in range(7):
                xnum = (xnum + _C[i]) * ym
                xden = (xden + _D[i]) * ym
            temp = (xnum + _C[7]) / (xden + _D[7])
            t = np.trunc(ym * 16.0) / 16.0
            dl = (ym - t) * (ym + t)
            tail[m] = _exp(O, -t * t * 0.5) * _exp(O, -dl * 0.5) * temp
        f = (y > _SQRT32) & (y < 38.5)
        if f.any():
            yf = y[f]
            xsq = 1.0 / (yf * yf)
            xnum = _P[5] * xsq
            xden = xsq
            for i in range(4):
                xnum = (xnum + _P[i]) * xsq
                xden = (xden + _Q[i]) * xsq
            temp = xsq * (xnum + _P[4]) / (xden + _Q[4])
            temp = (_M_1_SQRT_2PI - temp) / yf
            t = np.trunc(yf * 16.0) / 16.0
            dl = (yf - t) * (yf + t)
            tail[f] = _exp(O, -t * t * 0.5) * _exp(O, -dl * 0.5) * temp
        o = (y > 0.67448975)                      # (NaN: neither)
        rest = 1.0 - tail
        pos = o & (z > 0)
        neg = o & ~(z > 0)
        lower[pos], upper[pos] = rest[pos], tail[pos]
        lower[neg], upper[neg] = tail[neg], rest[neg]
    return lower.reshape(shape), upper.reshape(shape)


def pnorm_lower(O, z):
    return pnorm_both(O, z)[0]


def pnorm_upper(O, z):
    return pnorm_both(O, z)[1]


def pnorm_sd(O, x, se):
    """pnorm(x, mean = 0, sd = se) with pnorm5's rules: NaN in -> NaN; se < 0 -> NaN; se == 0 or a non-finite x / se ->
    0 for x < 0, else 1; otherwise pnorm_lower(x / se)"""
    x, se = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(se, np.float64))
    with np.errstate(all="ignore"):
        q = x / se
        out = pnorm_lower(O, np.where(np.isfinite(q), q, 0.0))
        step = np.where(x < 0, 0.0, 1.0)
        out = np.where((se == 0) | ~np.isfinite(q), step, out)
        out = np.where(np.isnan(x) | np.isnan(se) | (se < 0), np.nan, out)
    return out


def _pmax(a, b):
    """R's pmax / pmin on doubles (na.rm = FALSE): NA if either is, else the second unless the first is larger / smaller"""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, b))


def _pmin(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, b))


def _sign(v):
    return np.where(np.isnan(v), np.nan, np.where(v > 0, 1.0, np.where(v < 0, -1.0, 0.0)))


def threshold_tests(O, LFC, SE, T, altHypothesis):
    """(stat, pvalue) of R/results.R:484-515 under the normal distribution, in that operation order"""
    LFC, SE = np.asarray(LFC, np.float64), np.asarray(SE, np.float64)
    T = float(T)
    up = lambda q: pnorm_upper(O, q)              # pnorm(q, lower.tail = FALSE): +-Inf give 0 / 1 through the ranges
    with np.errstate(all="ignore"):
        if altHypothesis == "greaterAbs":
            stat = LFC / SE
            pval = pnorm_sd(O, -np.abs(LFC) + T, SE) + pnorm_sd(O, -np.abs(LFC) - T, SE)
        elif altHypothesis == "greaterAbs2014":
            q = (np.abs(LFC) - T) / SE
            stat = _sign(LFC) * _pmax(q, 0.0)
            pval = _pmin(1.0, 2.0 * up(q))
        elif altHypothesis == "lessAbs":
            qa, qb = (T - LFC) / SE, (LFC + T) / SE
            stat = _pmin(_pmax(qa, 0.0), _pmax(qb, 0.0))
            pval = _pmax(up(qa), up(qb))
        elif altHypothesis == "greater":
            q = (LFC - T) / SE
            stat = _pmax(q, 0.0)
            pval = up(q)
        elif altHypothesis == "less":
            stat = _pmin((LFC + T) / SE, 0.0)
            pval = up((-T - LFC) / SE)
        else:
            raise ValueError(altHypothesis)
    return stat, pval


def results_table(O, beta, betaSE, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
                  altHypothesis="greaterAbs"):
    """the five columns before the adjustment: the coefficient's columns as given, threshold_tests when asked
    (R/results.R:464-518), pvalue NA where na_mask (:564), then the nowZero fill (:567-575)"""
    lfc, se = np.array(beta, np.float64), np.array(betaSE, np.float64)
    st, pv = np.array(stat, np.float64), np.array(pvalue, np.float64)
    bm = np.asarray(baseMean, np.float64)
    if not (lfcThreshold == 0 and altHypothesis == "greaterAbs"):
        st, pv = threshold_tests(O, lfc, se, lfcThreshold, altHypothesis)
        st, pv = np.array(st), np.array(pv)
    if na_mask is not None:
        pv[np.asarray(na_mask, bool)] = np.nan
    if replace is not None:
        z = np.asarray(replace, bool) & (bm == 0)
        lfc[z], se[z], st[z], pv[z] = 0.0, 0.0, 0.0, 1.0
    return {"baseMean": bm.copy(), "log2FoldChange": lfc, "lfcSE": se, "stat": st, "pvalue": pv}


# ---- p.adjust(p, "BH") and filtered_p, line by line ---------------------------------------------------------------------
def p_adjust_bh(p):
    """stats::p.adjust(p, "BH"): p0 <- p; p <- p[!is.na(p)]; n <- length(p); i <- n:1; o <- order(p, decreasing = TRUE);
    ro <- order(o); p0[!is.na(p0)] <- pmin(1, cummin(n / i * p[o]))[ro]"""
    p0 = np.array(p, np.float64)
    nna = ~np.isnan(p0)
    pp = p0[nna]
    n = pp.size
    if n == 0:
        return p0
    i = np.arange(n, 0, -1).astype(np.float64)
    o = np.argsort(-pp, kind="stable")
    ro = np.argsort(o, kind="stable")
    with np.errstate(all="ignore"):
        p0[nna] = np.minimum(1.0, np.minimum.accumulate((n / i) * pp[o]))[ro]
    return p0


def quantile7(filter, theta):
    """quantile(filter, theta), type 7: h = (n - 1) theta, g = h - floor(h), (1 - g) s[lo] + g s[hi] with both products
    rounded; s[lo] itself when g == 0 or s[hi] == s[lo]"""
    s = np.sort(np.asarray(filter, np.float64))
    out = np.empty(len(theta))
    for k, t in enumerate(np.asarray(theta, np.float64)):
        h = (s.size - 1) * t
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        g = h - lo
        with np.errstate(all="ignore"):
            out[k] = s[lo] if (g == 0 or s[hi] == s[lo]) else (1.0 - g) * s[lo] + g * s[hi]
    return out


def filtered_p(filter, p, cutoffs, alpha):
    """genefilter's filtered_p (R/results.R:721-740): one p.adjust per cutoff over the rows with filter >= cutoff.
    Returns (filtPadj n x K, numRej = colSums(filtPadj < alpha, na.rm = TRUE))"""
    filter, p = np.asarray(filter, np.float64), np.asarray(p, np.float64)
    out = np.full((filter.size, len(cutoffs)), np.nan)
    for k, c in enumerate(cutoffs):
        use = filter >= c
        if use.any():
            out[use, k] = p_adjust_bh(p[use])
    with np.errstate(invalid="ignore"):
        numRej = (out < alpha).sum(axis=0).astype(np.int32)
    return out, numRej


def filtered_p_one_sort(filter, p, cutoffs, alpha):
    """the same, the way the kernel computes it: ONE ascending sort of the non-NA p (any order among ties); per cutoff the
    inclusive prefix count r of the used rows, mS = r[-1], v = (mS / r) p on the used rows, a suffix minimum, pmin(1, .)"""
    filter, p = np.asarray(filter, np.float64), np.asarray(p, np.float64)
    n = p.size
    rows = np.where(~np.isnan(p))[0]
    rows = rows[np.argsort(p[rows], kind="stable")]
    ps = p[rows]
    out = np.full((n, len(cutoffs)), np.nan)
    for k, c in enumerate(cutoffs):
        use = filter[rows] >= c
        r = np.cumsum(use)
        if r.size == 0 or r[-1] == 0:
            continue
        mS = float(r[-1])
        with np.errstate(all="ignore"):
            v = np.where(use, (mS / np.maximum(r, 1)) * ps, np.inf)
        suf = np.minimum.accumulate(v[::-1])[::-1]
        out[rows[use], k] = np.minimum(1.0, suf)[use]
    with np.errstate(invalid="ignore"):
        numRej = (out < alpha).sum(axis=0).astype(np.int32)
    return out, numRej


def results(O, beta, betaSE, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
            altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1):
    """what dsq_results computes: the table, then filtPadj / numRej / cutoffs over theta (theta None: independentFiltering =
    FALSE, one column with a cutoff of -Inf)"""
    tab = results_table(O, beta, betaSE, stat, pvalue, baseMean, replace, na_mask, lfcThreshold, altHypothesis)
    f = tab["baseMean"] if filter is None else np.asarray(filter, np.float64)
    if theta is None:
        cutoffs = np.array([-np.inf])
        fp = p_adjust_bh(tab["pvalue"])[:, None]
        with np.errstate(invalid="ignore"):
            nr = (fp < alpha).sum(axis=0).astype(np.int32)
    else:
        cutoffs = quantile7(f, theta)
        fp, nr = filtered_p(f, tab["pvalue"], cutoffs, alpha)
    tab.update(filtPadj=fp, numRej=nr, cutoffs=cutoffs)
    return tab
