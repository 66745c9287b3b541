"""CPU: the numerical specification of results() (tests/results_spec.py) against independent
statements -- the line-by-line p.adjust loop, scipy's BH, mpmath at 50 digits --, core.lowess, and core.results over
HostEngine (R/results.R:298-740, tests/testthat/test_results.R)."""
import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import results_spec as S
from tests.helpers import assert_same, make_case


# ---- 1. one sort for all cutoffs == one p.adjust per cutoff, bit for bit ------------------------------------------------
def _bh_inputs(n, kind, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(size=n) ** 3
    f = np.exp(rng.normal(3, 2, n))
    if kind == "na":
        p[rng.uniform(size=n) < 0.2] = np.nan
    elif kind == "ties":
        p = np.round(p, 2)
    elif kind == "zero_one":
        p[::3] = 0.0
        p[1::5] = 1.0
    elif kind == "zero_filter":
        f[rng.uniform(size=n) < 0.3] = 0.0
        p[rng.uniform(size=n) < 0.1] = np.nan
    elif kind == "equal_filter":
        f[:] = 7.5
    elif kind == "subset_all_na":
        p[f >= np.median(f)] = np.nan          # the subsets of the upper cutoffs hold no non-NA p-value
    return f, p


@pytest.mark.parametrize("kind", ["plain", "na", "ties", "zero_one", "zero_filter", "equal_filter", "subset_all_na"])
@pytest.mark.parametrize("n", [1, 2, 37, 1000])
def test_one_sort_equals_filtered_p(n, kind):
    f, p = _bh_inputs(n, kind, seed=n + len(kind))
    theta = np.linspace(np.mean(f == 0), 0.95, 50)
    cut = S.quantile7(f, theta)
    a, ra = S.filtered_p(f, p, cut, 0.1)
    b, rb = S.filtered_p_one_sort(f, p, cut, 0.1)
    assert_same(b, a, "filtPadj %s n=%d" % (kind, n))
    assert_same(rb, ra, "numRej")
    if kind == "subset_all_na" and n > 2:
        assert np.isnan(a[:, -1]).all()


def test_quantile7_is_numpys_linear_quantile():
    rng = np.random.default_rng(3)
    for n in (1, 2, 37, 1000):
        f = rng.normal(size=n)
        th = np.linspace(0, 1, 23)
        np.testing.assert_allclose(S.quantile7(f, th), np.quantile(f, th), rtol=1e-14, atol=1e-15)
        assert_same(S.quantile7(f, th), np.array([core.quantile7(f, t) for t in th]), "core.quantile7")


# ---- 2. p.adjust(., "BH") against scipy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 37, 1000])
def test_p_adjust_bh_vs_scipy(n):
    from scipy.stats import false_discovery_control
    p = np.random.default_rng(n).uniform(size=n) ** 2
    want = false_discovery_control(p, method="bh")
    assert np.max(np.abs(S.p_adjust_bh(p) - want)) <= 1e-15
    assert np.max(np.abs(core.p_adjust(p) - want)) <= 1e-15
    pn = p.copy()
    pn[::4] = np.nan
    assert_same(core.p_adjust(pn), S.p_adjust_bh(pn), "core.p_adjust with NA")
    assert_same(core.p_adjust(pn, "none"), pn, "none")


# ---- 3. / 4. pnorm and the threshold tests against mpmath at 50 digits ----------------------------------------------------
# the budget of the two-sided check of tests/test_oracle_math.py: 5.0 spacings of the exact value (+ 0.5 for the rounding of
# the reference to double); where the exact value is subnormal, one denormal step
MAX_ULP = 5.0 + 0.5


def _mp_tail(z, upper):
    import mpmath as mp
    mp.mp.dps = 50
    out = np.empty(len(z))
    for i, v in enumerate(z):
        if np.isinf(v):
            out[i] = 0.0 if (v > 0) == upper else 1.0
            continue
        t = mp.mpf(float(v)) / mp.sqrt(2)
        out[i] = float(mp.erfc(t if upper else -t) / 2)
    return out


def _within_budget(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    sub = np.abs(want) < 2.0 ** -1022
    if sub.any():
        assert np.max(np.abs(got[sub] - want[sub])) <= 2.0 ** -1074, what + " (subnormal)"
    g, w = got[~sub], want[~sub]
    err = np.abs(g - w) / np.spacing(np.abs(w))
    print("%s: max error %.2f spacings" % (what, err.max()))
    assert err.max() <= MAX_ULP, "%s: %.2f spacings at %r" % (what, err.max(), g[np.argmax(err)])


def _z_grid():
    rng = np.random.default_rng(715)
    edges = np.array([0.67448975, np.sqrt(32.0)])
    z = np.concatenate([np.linspace(0, 38, 1521), edges, np.nextafter(edges, 0), np.nextafter(edges, 40), rng.uniform(0, 38, 1500),
                        [1e-17, 1e-300, 5.5e-17, 37.5, 38.0]])
    return np.concatenate([z, -z])


def test_pnorm_one_tail_vs_mpmath(oracle):
    z = _z_grid()
    lo, up = S.pnorm_both(oracle, z)
    _within_budget(lo, _mp_tail(z, False), "pnorm_lower")
    _within_budget(up, _mp_tail(z, True), "pnorm_upper")
    # the one-tail statement and the engine's two-sided one are the same algorithm: 2 * upper(|z|) bit for bit
    assert_same(2.0 * S.pnorm_upper(oracle, np.abs(z)), oracle.unary("pnorm_upper2", z), "2 upper(|z|)")
    sp = S.pnorm_both(oracle, np.array([np.nan, np.inf, -np.inf, 38.5, -38.5, 0.0]))
    assert np.isnan(sp[0][0]) and sp[0][1:].tolist() == [1.0, 0.0, 1.0, 0.0, 0.5] and sp[1][1:].tolist() == [0.0, 1.0, 0.0, 1.0, 0.5]


def _mp_threshold(LFC, SE, T, alt):
    """R/results.R:484-515 with the distribution function at 50 digits.  The ARGUMENTS of pnorm are the doubles R itself
    forms (x / se inside pnorm(x, sd = se), (LFC - T) / SE ...): a line's own roundings are part of the line."""
    with np.errstate(all="ignore"):
        a = np.abs(LFC)
        if alt == "greaterAbs":
            return LFC / SE, _mp_sum(_mp_exact((-a + T) / SE, False), _mp_exact((-a - T) / SE, False))
        if alt == "greaterAbs2014":
            q = (a - T) / SE
            return np.sign(LFC) * np.maximum(q, 0), np.minimum(1.0, [float(2 * v) for v in _mp_exact(q, True)])
        if alt == "lessAbs":
            qa, qb = (T - LFC) / SE, (LFC + T) / SE
            pa, pb = _mp_exact(qa, True), _mp_exact(qb, True)
            return np.minimum(np.maximum(qa, 0), np.maximum(qb, 0)), np.array([float(max(u, v)) for u, v in zip(pa, pb)])
        if alt == "greater":
            q = (LFC - T) / SE
            return np.maximum(q, 0), np.array([float(v) for v in _mp_exact(q, True)])
        q = (LFC + T) / SE
        return np.minimum(q, 0), np.array([float(v) for v in _mp_exact((-T - LFC) / SE, True)])


def _mp_exact(z, upper):
    import mpmath as mp
    mp.mp.dps = 50
    return [mp.erfc((mp.mpf(float(v)) if upper else -mp.mpf(float(v))) / mp.sqrt(2)) / 2 for v in z]


def _mp_sum(a, b):
    return np.array([float(u + v) for u, v in zip(a, b)])


def _threshold_case():
    rng = np.random.default_rng(484)
    n = 600
    LFC = rng.normal(0, 2, n)
    SE = np.exp(rng.normal(-1, 0.7, n))
    LFC[:40] = rng.normal(0, 0.05, 40)          # statistics in the central range of pnorm
    return LFC, SE


def _check_threshold(fn, oracle, alt):
    LFC, SE = _threshold_case()
    stat, pv = fn(oracle, LFC, SE, 0.5, alt)
    wstat, wpv = _mp_threshold(LFC, SE, 0.5, alt)
    assert_same(stat, wstat, alt + " stat")
    _within_budget(pv, wpv, alt + " pvalue")


@pytest.mark.parametrize("alt", S.ALT)
def test_threshold_tests_vs_mpmath(oracle, alt):
    _check_threshold(S.threshold_tests, oracle, alt)


def test_threshold_mutants_fail(oracle):
    def one_term(O, LFC, SE, T, alt):
        return LFC / SE, S.pnorm_sd(O, -np.abs(LFC) + T, SE)

    def wrong_sign(O, LFC, SE, T, alt):
        return S._pmin((LFC + T) / SE, 0.0), S.pnorm_upper(O, (T + LFC) / SE)
    with pytest.raises(AssertionError):
        _check_threshold(one_term, oracle, "greaterAbs")
    with pytest.raises(AssertionError):
        _check_threshold(wrong_sign, oracle, "less")


def test_threshold_edge_values(oracle):
    """SE = 0, SE NA, |LFC / SE| beyond 38: R's rules (pnorm5 around the quotient, pmax / pmin propagate NA)"""
    LFC = np.array([1.0, -1.0, 0.2, 0.0, 3.0, 500.0, -500.0, np.nan])
    SE = np.array([0.0, 0.0, 0.0, 0.0, np.nan, 1.0, 1.0, 1.0])
    st, pv = S.threshold_tests(oracle, LFC, SE, 0.5, "greaterAbs")
    assert pv[:4].tolist() == [0.0, 0.0, 1.0, 1.0] and np.isnan(pv[4]) and pv[5] == 0.0 and pv[6] == 0.0 and np.isnan(pv[7])
    st, pv = S.threshold_tests(oracle, LFC, SE, 0.5, "greater")
    assert pv[:4].tolist() == [0.0, 1.0, 1.0, 1.0] and np.isnan(pv[4]) and pv[5] == 0.0 and pv[6] == 1.0
    assert st[:4].tolist() == [np.inf, 0.0, 0.0, 0.0] and np.isnan(st[4])


# ---- 5. core.lowess -------------------------------------------------------------------------------------------------------
def test_lowess_reproduces_a_line():
    x = np.sort(np.random.default_rng(5).uniform(0, 1, 50))
    y = 3.0 - 2.0 * x
    for f in (0.2, 2.0 / 3.0):
        fit = core.lowess(x, y, f=f)
        assert np.max(np.abs(fit["y"] - y)) < 1e-12
        assert_same(fit["x"], x, "x")


def test_lowess_is_the_local_tricube_line():
    rng = np.random.default_rng(50)
    x = np.sort(rng.uniform(0, 10, 50))
    y = np.sin(x) + rng.normal(0, 0.3, 50)
    f = 1.0 / 5.0
    ns = max(2, min(50, int(f * 50 + 1e-7)))
    fit = core.lowess(x, y, f=f, iter=0, delta=0.0)
    for i in range(50):
        d = np.abs(x - x[i])
        h = np.sort(d)[ns - 1]
        r = d / h
        assert not ((r > 0.999) & (r < 1.0)).any() and not ((r > 0) & (r <= 0.001)).any()      # (the algorithm's two cut bands are empty)
        w = np.where(r < 1.0, (1.0 - r ** 3) ** 3, 0.0)
        sw = np.sqrt(w)
        coef, *_ = np.linalg.lstsq(np.column_stack([sw, sw * x]), sw * y, rcond=None)
        assert abs(fit["y"][i] - (coef[0] + coef[1] * x[i])) < 1e-10, i


# ---- 6. core.results over HostEngine ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def analysis(oracle):
    """a two-group analysis with outliers: replaced rows (one of them all zero afterwards) and Cook's-flagged rows"""
    d = make_case(300, 14, "two_group", seed=21)
    k = d["counts"].copy()
    k[3] = [90000] + [12] * 13                 # replaced (7 replicates per group)
    k[5] = [70000] + [0] * 13                  # replaced and all zero afterwards: the nowZero fill
    E = HostEngine(oracle)
    dds = core.DESeq(core.DESeqDataSet(k, d["x"], engine=E))
    # the same counts without replacement: Cook's outliers keep their flags
    dds0 = core.DESeq(core.DESeqDataSet(k, d["x"], engine=E), minReplicatesForReplace=np.inf)
    return dds, dds0


def test_results_errors(oracle, analysis):
    dds, _ = analysis
    d = make_case(50, 8, "two_group", seed=2)
    with pytest.raises(RuntimeError, match="first run DESeq"):
        core.results(core.DESeqDataSet(d["counts"], d["x"], engine=HostEngine(oracle)))       # test_results.R:14
    with pytest.raises(ValueError, match="LRT requires"):
        core.results(dds, test="LRT")                                                         # :24
    with pytest.raises(ValueError, match="lessAbs"):
        core.results(dds, altHypothesis="lessAbs")                                            # :25
    with pytest.raises(ValueError, match="name"):
        core.results(dds, name=["Intercept", "group1"])                                       # :26
    with pytest.raises(ValueError):
        core.results(dds, test="foo")                                                         # :29
    with pytest.raises(ValueError):
        core.results(dds, alpha=1.5)
    with pytest.raises(ValueError):
        core.results(dds, lfcThreshold=-1)
    for kw in ({"contrast": [0, 1]}, {"addMLE": True}, {"format": "GRanges"}, {"parallel": True}, {"pAdjustMethod": "holm"}):
        with pytest.raises(NotImplementedError):
            core.results(dds, **kw)
    dl = core.DESeq(core.DESeqDataSet(d["counts"], d["x"], engine=HostEngine(oracle)), test="LRT", reduced=np.ones((8, 1)))
    with pytest.raises(ValueError, match="Wald tests"):
        core.results(dl, lfcThreshold=1)                                                      # :114
    dp = core.DESeq(core.DESeqDataSet(d["counts"], d["x"], engine=HostEngine(oracle)), betaPrior=True)
    with pytest.raises(ValueError, match="betaPrior=FALSE"):
        core.results(dp, lfcThreshold=1, altHypothesis="lessAbs")                             # :62-67
    # test = "Wald" on the LRT object: makeWaldTest's columns
    rw = core.results(dl, test="Wald")
    with np.errstate(all="ignore"):
        assert_same(rw["stat"], dl.mcols["beta"][:, 1] / dl.mcols["betaSE"][:, 1], "makeWaldTest stat")


def test_results_table_and_padj(oracle, analysis):
    dds, dds0 = analysis
    assert core.resultsNames(dds) == ["Intercept", "coef1"]
    res = core.results(dds)
    rep = np.asarray(dds.mcols["replace"]) == 1
    now_zero = rep & (dds.mcols["baseMean"] == 0)
    assert now_zero[5] and rep[3] and not now_zero[3]
    for c, v in (("log2FoldChange", 0.0), ("lfcSE", 0.0), ("stat", 0.0), ("pvalue", 1.0)):
        assert (res[c][now_zero] == v).all(), c                                               # R/results.R:567-575
    keep = ~now_zero
    assert_same(res["log2FoldChange"][keep], dds.mcols["beta"][keep, 1], "lfc")
    assert_same(res["stat"][keep], dds.mcols["WaldStatistic"][keep, 1], "stat")
    # sum(padj < alpha) is the count of the chosen threshold; the metadata of R/results.R:695-704
    md = res.metadata
    j = int(np.where(md["filterNumRej"]["theta"] == md["filterTheta"])[0][0])
    with np.errstate(invalid="ignore"):
        assert int((res["padj"] < 0.1).sum()) == int(md["filterNumRej"]["numRej"][j])
    assert md["alpha"] == 0.1 and md["lfcThreshold"] == 0 and len(md["lo.fit"]["y"]) == 50
    assert md["filterThreshold"] == S.quantile7(res["baseMean"], [md["filterTheta"]])[0]
    # the whole independent filtering against the specification
    theta = md["filterNumRej"]["theta"]
    fp, nr = S.filtered_p(res["baseMean"], res["pvalue"], S.quantile7(res["baseMean"], theta), 0.1)
    assert_same(md["filterNumRej"]["numRej"], nr, "numRej")
    assert_same(res["padj"], fp[:, j], "padj")
    # independentFiltering = FALSE: p.adjust of the table's p-values
    r0 = core.results(dds, independentFiltering=False)
    assert_same(r0["padj"], core.p_adjust(r0["pvalue"]), "padj without filtering")
    assert_same(r0["padj"], S.p_adjust_bh(res["pvalue"]), "padj without filtering (spec)")
    assert "filterThreshold" not in r0.metadata
    # Cook's-flagged rows carry NA in pvalue and padj; cooksCutoff = FALSE switches the filter off
    flags = core.cooksOutlier(dds0)
    assert flags.any()
    rc = core.results(dds0)
    assert np.isnan(rc["pvalue"][flags]).all() and np.isnan(rc["padj"][flags]).all()
    rn = core.results(dds0, cooksCutoff=False)
    assert_same(rn["pvalue"], dds0.mcols["WaldPvalue"][:, 1], "no Cook's filter")
    assert np.isfinite(rn["pvalue"][flags]).all()
    # a threshold test goes through the specification's branch
    rt = core.results(dds, lfcThreshold=0.5, altHypothesis="greater", cooksCutoff=False)
    st, pv = S.threshold_tests(oracle, dds.mcols["beta"][:, 1], dds.mcols["betaSE"][:, 1], 0.5, "greater")
    assert_same(rt["stat"][keep], st[keep], "greater stat")
    assert_same(rt["pvalue"][keep], pv[keep], "greater pvalue")
    assert core.results(dds, tidy=True).columns[0] == "row"


def test_filter_fun_receives_the_table(analysis):
    """test_results.R:151-175: a custom filterFun gets the results table, the filter, alpha and the method"""
    dds, _ = analysis
    seen = {}

    def fun(res, filter, alpha, pAdjustMethod):
        seen.update(filter=filter, alpha=alpha, method=pAdjustMethod, n=len(res["pvalue"]))
        res["padj"] = core.p_adjust(res["pvalue"], pAdjustMethod)
        return res
    res = core.results(dds, filterFun=fun, alpha=0.05)
    assert seen == {"filter": None, "alpha": 0.05, "method": "BH", "n": dds.n}
    assert_same(res["padj"], core.p_adjust(res["pvalue"]), "filterFun padj")
    assert res.metadata["lfcThreshold"] == 0


def test_results_workspace_bytes_of_empty_and_bad_sizes():
    """(the layout of DsqResultsArgs / DsqResultsOut: test_capi_cpu.test_struct_layout_matches_header)"""
    from deseq2_amd import _lib
    assert _lib.lib().dsq_results_workspace_bytes(0, 0) >= 0 and _lib.lib().dsq_results_workspace_bytes(-1, 2) == 0
