"""CPU: Student's t in the engine's arithmetic.  deseq2_amd/student_t.py on the oracle's exp / log /
log1p / stirlerr against 50-digit values (tests/golden/pt_golden.json, written by make_golden_pt.py with mpmath, which shares
no arithmetic with it); then what rides on it through HostEngine(oracle): mcols tDegreesFreedom, the five threshold tests of
results() and resultsContrasts on a useT analysis, each against the formulas of R/results.R:477-515 and :812-815 written out
here with mpmath's incomplete beta function.

Measured on the golden grid (2374 normal-valued records): largest relative error 1.4e-13 (q = 37, df = 1e6, a tail of 9e-300:
|log p| eps alone is 1.5e-13); the bound below is 1e-12, the bar tests/test_chain_audit_cpu.py holds the useT p-values to."""
from collections import OrderedDict

import json
import os

import mpmath as mp
import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd import student_t as S
from deseq2_amd.engine import HostEngine
from tests import results_spec as RS
from tests.helpers import assert_same

mp.mp.dps = 50
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pt_golden.json")))
ALT = ("greaterAbs", "lessAbs", "greater", "less", "greaterAbs2014")


def _records(kind, tail):
    r = [e for e in GOLD[kind] if e[0] == tail]
    return np.array([float(e[1]) for e in r]), np.array([float(e[2]) for e in r]), [e[3] for e in r]


# ---- the primitive ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", ["upper", "lower"])
def test_golden_grid(oracle, tail):
    """relative error <= 1e-12 wherever the exact value is a normal number -- q = 1e300 at df = 0.05, 0.3, 0.5, 1 included,
    where q^2 overflows and the tail is still 1e-15 .. 3e-301; where it is below the smallest normal number, a result in
    [0, 2.3e-308]"""
    fn = S.pt_upper if tail == "upper" else S.pt_lower
    q, df, want = _records("normal", tail)
    assert q.size > 1000
    got, steps = S.pt_upper_steps(oracle, q if tail == "upper" else -q, df)
    assert_same(got, fn(oracle, q, df), "pt_%s" % tail)
    worst = 0.0
    for g, w, a, b in zip(got, want, q, df):
        w = mp.mpf(w)
        err = abs(mp.mpf(float(g)) - w) / w
        worst = max(worst, float(err))
        assert err <= 1e-12, (tail, a, b, g, w)
    print("pt_%s: %d points, largest relative error %.3g, steps %s" % (tail, q.size, worst, steps))
    assert 40 < max(steps.values()) < S.CAP // 2
    for point in ((1e300, 0.05), (1e300, 0.3), (1e300, 0.5), (1e300, 1.0)):
        s = 1.0 if tail == "upper" else -1.0
        assert ((q == s * point[0]) & (df == point[1])).any(), point
    q, df, want = _records("tiny", tail)
    assert q.size > 50
    got = fn(oracle, q, df)
    assert ((got >= 0) & (got <= 2.3e-308)).all()


def test_special_values_and_symmetry(oracle):
    nan, inf = np.nan, np.inf
    up = lambda q, df: S.pt_upper(oracle, np.array([q], float), np.array([df], float))[0]
    lo = lambda q, df: S.pt_lower(oracle, np.array([q], float), np.array([df], float))[0]
    for q, df in ((nan, 3.0), (1.0, nan), (nan, nan), (1.0, 0.0), (1.0, -2.0), (inf, -1.0), (0.0, -inf)):
        assert np.isnan(up(q, df)) and np.isnan(lo(q, df)), (q, df)
    for df in (0.05, 1.0, 47.25, 1e8, inf):
        assert lo(-inf, df) == 0.0 and lo(inf, df) == 1.0 and up(inf, df) == 0.0 and up(-inf, df) == 1.0
        assert up(0.0, df) == 0.5 and up(-0.0, df) == 0.5 and lo(0.0, df) == 0.5
    rng = np.random.Generator(np.random.PCG64(3))
    q = 10.0 ** rng.uniform(-10, 4, 3000) * rng.choice([-1.0, 1.0], 3000)
    df = 10.0 ** rng.uniform(np.log10(0.05), 8, 3000)
    assert_same(S.pt_lower(oracle, q, df), S.pt_upper(oracle, -q, df), "lower(q) vs upper(-q)")
    # df = Inf: the normal tails of the results() statement, bit for bit
    z = np.concatenate([q[:500], [0.0, -0.0, 0.3, -0.67448975, 5.0, -6.0, 37.0, 39.0, -40.0]])
    l, u = RS.pnorm_both(oracle, z)
    assert_same(S.pt_lower(oracle, z, np.full(z.size, inf)), l, "df = Inf, lower")
    assert_same(S.pt_upper(oracle, z, np.full(z.size, inf)), u, "df = Inf, upper")
    assert_same(S.pt_two_sided(oracle, z, np.full(z.size, 7.5)), 2.0 * S.pt_upper(oracle, np.abs(z), np.full(z.size, 7.5)), "two-sided")


def test_tails_add_up_and_fall(oracle):
    """lower + upper within 2 ulp of 1 on |q| <= 6; the upper tail never rises along a fine sweep of q (the sweep crosses
    every range switch of the method: t = q^2 / df = 1 and |q| = 2)"""
    rng = np.random.Generator(np.random.PCG64(4))
    q = rng.uniform(-6, 6, 4000)
    df = 10.0 ** rng.uniform(np.log10(0.05), 8, 4000)
    s = S.pt_lower(oracle, q, df) + S.pt_upper(oracle, q, df)
    assert np.abs(s - 1.0).max() <= 2 * 2.220446049250313e-16
    sweep = np.concatenate([np.linspace(-50.0, 50.0, 20001), [1.9999, 2.0, 2.0001]])
    sweep.sort()
    for d in (0.7, 5.5, 1e4):
        u = S.pt_upper(oracle, sweep, np.full(sweep.size, d))
        assert (np.diff(u) <= 0).all(), d
        assert u[0] > 0.5 > u[-1] >= 0


def test_core_pt_on_the_host_engine(oracle):
    E = HostEngine(oracle)
    rng = np.random.Generator(np.random.PCG64(5))
    q = rng.normal(0, 4, (40, 3))
    df = rng.uniform(0.5, 30, 40)
    df[7], df[9] = np.nan, np.inf
    assert_same(core.pt(q, df, engine=E), S.pt_lower(oracle, q, df[:, None]), "core.pt matrix")
    assert_same(core.pt(q[:, 0], 4.5, lower_tail=False, engine=E), S.pt_upper(oracle, q[:, 0], 4.5), "core.pt vector, one df")
    keep = rng.uniform(size=q.shape) < 0.2
    got = E.pt(q, df, "two_sided", keep=keep)
    assert_same(got[keep], q[keep], "kept entries")
    assert_same(got[~keep], S.pt_two_sided(oracle, q, df[:, None])[~keep], "written entries")
    import deseq2_amd
    assert deseq2_amd.pt is core.pt


# ---- the tables --------------------------------------------------------------------------------------------------------------
def mp_upper(q, df):
    """pt(q, df, lower.tail = FALSE) at 50 digits; None for NA"""
    if np.isnan(q) or np.isnan(df):
        return None
    if np.isinf(q):
        return mp.mpf(0 if q > 0 else 1)
    q, df = mp.mpf(float(q)), mp.mpf(float(df))
    half = mp.betainc(df / 2, mp.mpf(1) / 2, 0, df / (df + q * q), regularized=True) / 2
    return half if q >= 0 else 1 - half


def mp_lower(q, df):
    return mp_upper(-q, df)


def mp_normal_upper(q, df):
    return None if np.isnan(q) or np.isnan(df) else mp.ncdf(-mp.mpf(float(q)))


def formulas(alt, lfc, se, T, df, upper=mp_upper):
    """R/results.R:477-515 for one gene; None for NA"""
    lower = lambda q, d: upper(-q, d)
    with np.errstate(all="ignore"):
        if alt == "greaterAbs":
            a, b = lower((-abs(lfc) + T) / se, df), lower((-abs(lfc) - T) / se, df)
            return None if a is None or b is None else a + b
        if alt == "greaterAbs2014":
            u = upper((abs(lfc) - T) / se, df)
            return None if u is None else min(mp.mpf(1), 2 * u)
        if alt == "lessAbs":
            a, b = upper((T - lfc) / se, df), upper((lfc + T) / se, df)
            return None if a is None or b is None else max(a, b)
        if alt == "greater":
            return upper((lfc - T) / se, df)
        return upper((-T - lfc) / se, df)


def worst_error(res, alt, T, df, skip, upper=mp_upper):
    """largest relative error of res$pvalue against the formulas at the returned lfc, se (NA must sit where the formula has it)"""
    worst = 0.0
    for i in range(res.n):
        if skip[i]:
            continue
        want = formulas(alt, np.float64(res["log2FoldChange"][i]), np.float64(res["lfcSE"][i]), T, df[i], upper)
        got = res["pvalue"][i]
        if want is None:
            if not np.isnan(got):
                return np.inf
            continue
        if np.isnan(got):
            return np.inf
        worst = max(worst, float(abs(mp.mpf(float(got)) - want) / want) if want != 0 else float(got != 0))
    return worst


@pytest.fixture(scope="module")
def analysis(oracle):
    """~ condition (three levels, six samples each) with observation weights on 90 genes: fractional degrees of freedom, row 3
    with sum(w) - p <= 0, rows 9 and 40 all zero, row 5 with an outlier count that is replaced, rows 7 and 8 with zeros in levels 1 and 2
    (row 8 is also given df <= 0), row 6 with zeros in levels 0 and 1"""
    from deseq2_amd import simulate
    f = OrderedDict(condition=np.repeat([0, 1, 2], 6))
    x, _ = core.standard_model_matrix(f)
    k = simulate.make_counts(90, x, seed=11, drop_all_zero=False)["counts"]
    rng = np.random.Generator(np.random.PCG64(12))
    w = rng.uniform(0.3, 1.0, k.shape)
    w[3] = 0.1
    w[3, 0] = 1.0                                                    # 1 + 17 * 0.1 - 3 < 0
    k[9] = 0
    k[40] = 0
    k[5] = np.maximum(k[5], 20)
    k[5, 2] = 200000
    k[7, f["condition"] != 0] = 0
    k[7, f["condition"] == 0] = [30, 41, 28, 35, 33, 29]
    k[8, f["condition"] != 0] = 0
    k[8, f["condition"] == 0] = [50, 61, 48, 55, 47, 52]
    k[6, f["condition"] != 2] = 0
    k[6, f["condition"] == 2] = [44, 39, 51, 40, 46, 38]
    w[8] = 0.1
    w[8, 13] = 1.0
    dds = core.DESeq(core.DESeqDataSet(k, x, weights=w, engine=HostEngine(oracle)), factors=f, useT=True,
                     minReplicatesForReplace=6)
    return dds, k, w, f


def test_degrees_of_freedom_column(analysis):
    dds, k, w, f = analysis
    wn = w / w.max(axis=1, keepdims=True)
    want = wn.sum(axis=1) - 3
    want[want <= 0] = np.nan
    want[[9, 40]] = np.nan
    got = dds.mcols["tDegreesFreedom"]
    assert np.isnan(got[[3, 8, 9, 40]]).all() and np.isfinite(got).sum() == 86
    np.testing.assert_allclose(got, want, rtol=1e-14, equal_nan=True)
    assert (got[np.isfinite(got)] % 1 != 0).all()                   # fractional
    assert np.asarray(dds.mcols["replace"])[5] == 1
    assert dds.attrs["useT"]


@pytest.mark.parametrize("T", [0.5, 1.0])
@pytest.mark.parametrize("alt", ALT)
def test_threshold_tests_under_t(analysis, alt, T):
    dds, k, w, f = analysis
    res = core.results(dds, lfcThreshold=T, altHypothesis=alt, cooksCutoff=False, independentFiltering=False)
    df = np.asarray(dds.mcols["tDegreesFreedom"])
    skip = np.asarray(dds.mcols["allZero"], bool)
    err = worst_error(res, alt, T, df, skip)
    print("%s, T = %g: largest relative error %.3g" % (alt, T, err))
    assert err <= 1e-12
    assert np.isnan(res["pvalue"][[3, 8, 9, 40]]).all() and np.isfinite(res["pvalue"]).sum() == 86
    assert_same(res["padj"], RS.p_adjust_bh(res["pvalue"]), "padj")
    with np.errstate(all="ignore"):
        if alt == "greaterAbs":
            assert_same(res["stat"], res["log2FoldChange"] / res["lfcSE"], "stat")
    # mutants: the normal distribution, and the degrees of freedom of the row above
    assert worst_error(res, alt, T, df, skip, mp_normal_upper) > 1e-6
    shifted = np.roll(df, 1)
    ok = skip | np.isnan(df) | np.isnan(shifted)
    assert worst_error(res, alt, T, shifted, ok) > 1e-6


def test_filtering_runs_on_the_t_p_values(analysis):
    dds, k, w, f = analysis
    res = core.results(dds, lfcThreshold=0.5, altHypothesis="greaterAbs")
    plain = core.results(dds, lfcThreshold=0.5, altHypothesis="greaterAbs", cooksCutoff=False, independentFiltering=False)
    theta = res.metadata["filterNumRej"]["theta"]
    na = np.isnan(res["pvalue"]) & ~np.isnan(plain["pvalue"])        # (the Cook's mask)
    fp, nr = RS.filtered_p(res["baseMean"], res["pvalue"], RS.quantile7(res["baseMean"], theta), 0.1)
    assert_same(res.metadata["filterNumRej"]["numRej"], nr, "numRej")
    j = int(np.where(theta == res.metadata["filterTheta"])[0][0])
    assert_same(res["padj"], fp[:, j], "padj")
    assert_same(res["pvalue"][~na], plain["pvalue"][~na], "pvalue")


def test_contrasts_under_t(analysis):
    """numeric, character and list forms on the three-level factor; ("condition", 1, 0) is served by the pull of the stored
    columns (the chain's own useT p-values), the others by the covariance pass: pvalue = 2 ptU(|stat|, df), and 1 where the
    contrast's samples are all zero, on the df <= 0 row 8 too"""
    dds, k, w, f = analysis
    dds.attrs["coefNames"] = ["Intercept", "condition_1_vs_0", "condition_2_vs_0"]
    try:
        forms = [("condition", 1, 0), ("condition", 2, 1), [["condition_2_vs_0"], ["condition_1_vs_0"]], [0, -1, 1], [0, 1, 0.5]]
        res = core.resultsContrasts(dds, forms, cooksCutoff=False, independentFiltering=False)
    finally:
        dds.attrs.pop("coefNames")
    df = np.asarray(dds.mcols["tDegreesFreedom"])
    allZero = np.asarray(dds.mcols["allZero"], bool)
    cond = f["condition"]
    refitted = np.asarray(dds.mcols["replace"]) == 1
    assert refitted[5]
    masks = [np.isin(cond, [0, 1]), np.isin(cond, [1, 2]), np.isin(cond, [1, 2]), np.isin(cond, [1, 2]), None]
    for r, mask, form in zip(res, masks, forms):
        zero = np.zeros(dds.n, bool) if mask is None else (~allZero & ~(k[:, mask] != 0).any(axis=1))
        checked = 0
        for i in range(dds.n):
            got = r["pvalue"][i]
            if allZero[i]:
                assert np.isnan(got)
            elif zero[i]:
                assert got == 1.0 and r["log2FoldChange"][i] == 0.0 and r["stat"][i] == 0.0, (form, i)
            elif np.isnan(df[i]):
                assert np.isnan(got), (form, i)
            else:
                want = 2 * mp_upper(abs(float(r["stat"][i])), df[i])
                if r is res[0] and refitted[i]:
                    # the pull takes the chain's stored p-value, and refitWithoutOutliers tests its rows without useT
                    # (R/core.R:2524-2527): the normal distribution on that row, as in R
                    want = 2 * mp.ncdf(-abs(mp.mpf(float(r["stat"][i]))))
                assert abs(mp.mpf(float(got)) - want) <= 1e-12 * want, (form, i, got, want)
                checked += 1
        assert checked >= 80
        assert_same(r["padj"], RS.p_adjust_bh(r["pvalue"]), "padj of %r" % (form,))
    assert res[1]["pvalue"][8] == 1.0 and res[3]["pvalue"][7] == 1.0 and res[0]["pvalue"][6] == 1.0
    assert np.isnan(res[4]["pvalue"][8]) and np.isnan(df[8])
    assert_same(res[1]["pvalue"], res[2]["pvalue"], "character vs list")
    assert_same(res[2]["pvalue"], res[3]["pvalue"], "list vs numeric")
    # the normal distribution would be off by far more than the bound
    i = int(np.nanargmin(np.where(np.isfinite(df), res[3]["pvalue"], np.nan)))
    assert abs(2 * mp.ncdf(-abs(float(res[3]["stat"][i]))) / mp.mpf(float(res[3]["pvalue"][i])) - 1) > 1e-3
    # a threshold test on a contrast: the tail of results() takes the same degrees of freedom
    thr = core.resultsContrasts(dds, [[0, -1, 1]], lfcThreshold=0.5, altHypothesis="greater", cooksCutoff=False,
                                independentFiltering=False)[0]
    assert worst_error(thr, "greater", 0.5, df, allZero | (~allZero & ~(k[:, masks[3]] != 0).any(axis=1))) <= 1e-12


def test_an_object_without_the_column(analysis, oracle):
    """attrs["useT"] without mcols tDegreesFreedom -- an object from before the column was stored, or a hand-made one: both
    entry points say what is missing"""
    dds, k, w, f = analysis
    saved = dds.mcols.pop("tDegreesFreedom")
    try:
        with pytest.raises(NotImplementedError, match="tDegreesFreedom.*Student-t"):
            core.results(dds, lfcThreshold=1, altHypothesis="greater")
        with pytest.raises(NotImplementedError, match="tDegreesFreedom.*Student-t"):
            core.resultsContrasts(dds, [[0, -1, 1]])
        core.results(dds)                                             # (the stored columns need no distribution)
    finally:
        dds.mcols["tDegreesFreedom"] = saved


def test_pt_entry_checks_its_arguments():
    """dsq_pt / dsq_pt_dev decide their argument errors (1 = DSQ_ERR_ARG) before a device is asked for; an empty call is
    nothing to do only where there is a device to do nothing on"""
    import ctypes
    from deseq2_amd import _lib
    L = _lib.lib()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    q, df, out = np.zeros(6), np.ones(3), np.zeros(6)
    for fn, tail_args in ((L.dsq_pt, ()), (L.dsq_pt_dev, (None,))):
        assert fn(None, P(df), 3, 2, 0, None, P(out), *tail_args) == 1
        assert fn(P(q), None, 3, 2, 0, None, P(out), *tail_args) == 1
        assert fn(P(q), P(df), 3, 2, 0, None, None, *tail_args) == 1
        assert fn(P(q), P(df), -1, 2, 0, None, P(out), *tail_args) == 1
        assert fn(P(q), P(df), 3, 2, 3, None, P(out), *tail_args) == 1
        assert b"tail" in L.dsq_last_error()
    assert set(_lib.DSQ_PT) == {"lower", "upper", "two_sided"}
