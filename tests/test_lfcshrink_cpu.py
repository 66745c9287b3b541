"""CPU: core.lfcShrink(type = "normal") over HostEngine(oracle) (R/lfcShrink.R:145-326, 496-505): the
reference's expectations (tests/testthat/test_lfcShrink.R:7-23, 47-48, 86-97) restated, every argument check once, the pin
against the betaPrior = TRUE chain (itself held to the oracle, the LAPACK restatement and the 50-digit audit), the lean route
against the full one, the replaced rows, and the rewritten contrast columns of estimateBetaPriorVar."""
from collections import OrderedDict

import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests.helpers import assert_same
from tests.lfcshrink_cases import counts as _counts, spiked as _spiked

COLS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj")


def _f2():
    return OrderedDict(condition=np.repeat([0, 1], 6))


def _f3():
    return OrderedDict(condition=np.repeat([0, 1, 2], 4))


def _dataset(f, oracle, seed=5, **kw):
    x, _ = core.standard_model_matrix(f)
    k = _counts(300, x, seed)
    return core.DESeqDataSet(k, x, engine=HostEngine(oracle), **kw), k, x


@pytest.fixture(scope="module")
def two(oracle):
    """two groups, n = 300, m = 12, no replaced rows"""
    f = _f2()
    d, k, x = _dataset(f, oracle)
    return core.DESeq(d, factors=f, minReplicatesForReplace=np.inf), k, x, f


@pytest.fixture(scope="module")
def three(oracle):
    """a three-level factor, n = 300, m = 12, no replaced rows"""
    f = _f3()
    d, k, x = _dataset(f, oracle, seed=7)
    return core.DESeq(d, factors=f, minReplicatesForReplace=np.inf), k, x, f


def _snapshot(dds):
    return ({k: np.array(v, copy=True) for k, v in dds.mcols.items()}, sorted(dds.attrs), sorted(dds.assays))


def _unchanged(dds, snap):
    mc, attrs, assays = snap
    assert list(dds.mcols) == list(mc) and sorted(dds.attrs) == attrs and sorted(dds.assays) == assays
    for k, v in mc.items():
        assert_same(np.asarray(dds.mcols[k], v.dtype), v, "the caller's mcols$" + k)


# ---- test_lfcShrink.R restated ---------------------------------------------------------------------------------------------------
def test_first_run_deseq(oracle):
    d, _, _ = _dataset(_f2(), oracle)
    with pytest.raises(RuntimeError, match="first run DESeq\\(\\) before running lfcShrink\\(\\)"):       # test_lfcShrink.R:7
        core.lfcShrink(d, coef=1)


def test_reference_expectations(two):
    dds, k, x, f = two
    snap = _snapshot(dds)
    res = core.results(dds, name=1)
    half = core.results(core.DESeq(core.DESeqDataSet(k[:150], x, engine=dds.engine), minReplicatesForReplace=np.inf), name=1)
    with pytest.raises(ValueError, match="rownames"):                             # :13
        core.lfcShrink(dds, coef=1, res=half, quiet=True)
    with pytest.raises(ValueError):                                               # :17: no such factor
        core.lfcShrink(dds, contrast=("treatment", 1, 0), res=res, quiet=True)
    with pytest.raises(ValueError):                                               # :18: no such level
        core.lfcShrink(dds, contrast=("condition", 2, 0), res=res, quiet=True)
    dds.attrs["coefNames"] = ["Intercept", "condition_B_vs_A"]
    try:
        by_name = core.lfcShrink(dds, coef="condition_B_vs_A", res=res, quiet=True)   # :21
        by_index = core.lfcShrink(dds, coef=1, res=res, quiet=True)               # :22
        no_res = core.lfcShrink(dds, coef=1, quiet=True)                          # :23
    finally:
        del dds.attrs["coefNames"]
    for c in COLS:
        assert_same(by_name[c], by_index[c], "coef by name / by index: " + c)
        assert_same(no_res[c], by_index[c], "res given / made: " + c)
    # shrunken: the fold changes move towards 0, and only they and their standard errors change (:318-325)
    live = ~np.isnan(res["log2FoldChange"])
    assert np.abs(by_index["log2FoldChange"][live]).sum() < np.abs(res["log2FoldChange"][live]).sum()
    assert not np.array_equal(by_index["log2FoldChange"][live], res["log2FoldChange"][live])
    for c in ("baseMean", "stat", "pvalue", "padj"):
        assert_same(by_index[c], res[c], "lfcThreshold = 0 leaves " + c)
    assert by_index.metadata["lfcThreshold"] == 0
    assert by_index.priorInfo["type"] == "normal" and by_index.priorInfo["betaPriorVar"].shape == (2,)
    assert by_index.priorInfo["betaPriorVar"][0] == 1e6 and by_index.priorInfo["betaPriorVar"][1] > 0
    assert res.priorInfo["type"] == "none" and "lfcThreshold" in res.metadata     # the argument `res` is untouched
    assert_same(res["log2FoldChange"], core.results(dds, name=1)["log2FoldChange"], "the caller's res")
    # :47-48: lfcThreshold = 1 also replaces stat, pvalue, padj -- by those of results(refit, lfcThreshold = 1)
    thr = core.lfcShrink(dds, coef=1, lfcThreshold=1, quiet=True)
    assert thr.metadata["lfcThreshold"] == 1
    assert_same(thr["baseMean"], res["baseMean"], "baseMean")
    assert not np.array_equal(thr["pvalue"][live], res["pvalue"][live])
    with np.errstate(all="ignore"):
        small = np.abs(thr["log2FoldChange"]) < 1
    assert (thr["pvalue"][small & live & ~np.isnan(thr["pvalue"])] > 0.5).all()   # greaterAbs: inside the threshold
    _unchanged(dds, snap)


def test_user_supplied_matrix_and_lrt_upstream(oracle):
    f = _f2()
    x, _ = core.standard_model_matrix(f)
    k = _counts(120, x, 3)
    E = HostEngine(oracle)
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=E), minReplicatesForReplace=np.inf)          # :86-90: no factors
    r = core.lfcShrink(dds, coef=1, res=core.results(dds), quiet=True)
    with pytest.raises(ValueError, match="user-supplied design matrix supports shrinkage only with 'coef'"):
        core.lfcShrink(dds, contrast=("condition", 1, 0), res=core.results(dds), quiet=True)
    with_f = core.DESeq(core.DESeqDataSet(k, x, engine=E), factors=f, minReplicatesForReplace=np.inf)
    for c in COLS:
        assert_same(r[c], core.lfcShrink(with_f, coef=1, quiet=True)[c], "matrix / factors: " + c)
    with_f.attrs["factors"] = OrderedDict(condition=np.repeat([0, 1, 2], 4))      # not the matrix of the analysis
    with pytest.raises(ValueError, match="only with 'coef'"):
        core.lfcShrink(with_f, contrast=("condition", 1, 0), res=core.results(with_f), quiet=True)
    # :92-97: only the LRT ran upstream -- the prior variance still comes from the stored MLE coefficients
    lrt = core.DESeq(core.DESeqDataSet(k, x, engine=E), test="LRT", reduced=np.ones((12, 1)), minReplicatesForReplace=np.inf)
    rl = core.lfcShrink(lrt, coef=1, quiet=True)
    assert_same(rl["log2FoldChange"], r["log2FoldChange"], "LRT upstream: log2FoldChange")
    assert_same(rl["lfcSE"], r["lfcSE"], "LRT upstream: lfcSE")
    assert_same(rl["pvalue"], core.results(lrt, name=1)["pvalue"], "LRT upstream: the p-values stay the LRT's")


def test_every_other_check(two, three):
    dds, k, x, f = two
    res = core.results(dds, name=1)
    L = lambda **kw: core.lfcShrink(dds, quiet=True, **kw)
    prior = core.DESeq(core.DESeqDataSet(k[:60], x, engine=dds.engine), betaPrior=True, factors=f, minReplicatesForReplace=np.inf)
    with pytest.raises(ValueError, match="downstream of DESeq\\(\\) with betaPrior=FALSE"):
        core.lfcShrink(prior, coef=1, quiet=True)
    for bad in (-1, [0, 1], np.nan):
        with pytest.raises(ValueError, match="lfcThreshold"):
            L(coef=1, lfcThreshold=bad)
    for bad in ("nope", 2, -1, 1.5):
        with pytest.raises(ValueError, match="resultsNamesDDS"):
            L(coef=bad)
    with pytest.raises(ValueError, match="missing\\(coef\\) \\| missing\\(contrast\\)"):
        L(coef=1, contrast=("condition", 1, 0))
    with pytest.raises(ValueError, match="one of coef or contrast required if 'res' is missing"):
        L()
    with pytest.raises(ValueError, match="requires either 'coef' or 'contrast'"):
        L(res=res)
    with pytest.raises(ValueError, match="numeric contrast, user must provide 'res' object"):
        L(contrast=[0.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="res should be a DESeqResults object"):
        L(coef=1, res={"lfcSE": np.zeros(dds.n)})
    nose = core.results(dds, name=1)
    nose["lfcSE"] = np.full(dds.n, np.nan)
    with pytest.raises(ValueError, match="lfcShrink requires standard errors"):
        L(coef=1, res=nose)
    nodisp = core._shallow(dds)
    nodisp.mcols = {k_: v for k_, v in dds.mcols.items() if k_ != "dispersion"}
    nodisp.attrs = dict(dds.attrs)
    with pytest.raises(RuntimeError, match="require dispersion estimates, first call estimateDispersions\\(\\)"):
        core.lfcShrink(nodisp, coef=1, res=res, quiet=True)
    # the character pre-checks of :277-281, then checkContrast over the expanded names (:286)
    with pytest.raises(ValueError, match="length\\(contrast\\) == 3"):
        L(contrast=("condition", 1), res=res)
    with pytest.raises(ValueError, match="names\\(colData\\(dds\\)\\)"):
        L(contrast=("batch", 1, 0), res=res)
    with pytest.raises(ValueError, match="levels\\(colData"):
        L(contrast=("condition", 1, 5), res=res)
    with pytest.raises(ValueError, match="should be different level names"):
        L(contrast=("condition", 1, 1), res=res)
    with pytest.raises(ValueError, match="one element for every element of 'resultsNames\\(object\\)'"):
        L(contrast=[0.0, 1.0], res=res)                        # (the expanded matrix has three columns)
    with pytest.raises(ValueError, match="should be elements of 'resultsNames\\(object\\)'"):
        L(contrast=[["condition1"], ["coef1"]], res=res)
    # type, and what is not served
    for t in ("apeglm", "ashr"):
        with pytest.raises(NotImplementedError, match=t):
            L(coef=1, type=t)
    with pytest.raises(ValueError, match="should be one of"):
        L(coef=1, type="ridge")
    for kw in (dict(svalue=True), dict(returnList=True), dict(format="GRanges"), dict(saveCols=[0]), dict(parallel=True),
               dict(apeAdapt=False, apeMethod="nbinomC")):
        with pytest.raises(NotImplementedError):
            L(coef=1, **kw)
    with pytest.raises(TypeError):
        L(coef=1, shrink=True)
    L(coef=1, svalue=False, returnList=False, format="DataFrame", saveCols=None, parallel=False, apeAdapt=True, apeMethod="nbinomCR")
    assert "apeglm" in core.lfcShrink.__doc__ and core.lfcShrink.__defaults__[3] == "normal"


# ---- the pin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3])
def test_pin_against_the_beta_prior_chain(oracle, two, three, levels):
    """without replaced rows the dispersions do not depend on betaPrior, so lfcShrink on the betaPrior = FALSE analysis must
    give the coefficients DESeq(betaPrior = TRUE) fits on the same data, bit for bit: by `coef` the standard matrix, by
    `contrast` the expanded one"""
    dds, k, x, f = two if levels == 2 else three
    snap = _snapshot(dds)
    E = HostEngine(oracle)
    std = core.DESeq(core.DESeqDataSet(k, x, engine=E), betaPrior=True, modelMatrixType="standard", factors=f,
                     minReplicatesForReplace=np.inf)
    assert_same(std.mcols["dispersion"], dds.mcols["dispersion"], "the dispersions do not depend on betaPrior")
    for c in range(1, levels):
        r = core.lfcShrink(dds, coef=c, quiet=True)
        assert_same(r["log2FoldChange"], std.mcols["beta"][:, c], "coef %d: log2FoldChange" % c)
        assert_same(r["lfcSE"], std.mcols["betaSE"][:, c], "coef %d: lfcSE" % c)
        assert_same(r.priorInfo["betaPriorVar"], std.attrs["betaPriorVar"], "coef %d: betaPriorVar" % c)
        assert np.isnan(r["log2FoldChange"][9])                # the all-zero row
    exp = core.DESeq(core.DESeqDataSet(k, x, engine=E), betaPrior=True, factors=f, minReplicatesForReplace=np.inf)
    assert exp.attrs["modelMatrixType"] == "expanded"
    pairs = [(1, 0)] if levels == 2 else [(1, 0), (2, 0), (2, 1), (0, 2)]
    ref = core.resultsContrasts(exp, [("condition", a, b) for a, b in pairs])
    for (a, b), want in zip(pairs, ref):
        r = core.lfcShrink(dds, contrast=("condition", a, b), quiet=True)
        assert_same(r["log2FoldChange"], want["log2FoldChange"], "condition %d vs %d: log2FoldChange" % (a, b))
        assert_same(r["lfcSE"], want["lfcSE"], "condition %d vs %d: lfcSE" % (a, b))
        assert_same(r.priorInfo["betaPriorVar"], exp.attrs["betaPriorVar"], "condition %d vs %d: betaPriorVar" % (a, b))
        full = core.lfcShrink(dds, contrast=("condition", a, b), lfcThreshold=1, quiet=True)
        for c in COLS:
            assert_same(full[c], core.resultsContrasts(exp, [("condition", a, b)], lfcThreshold=1)[0][c],
                        "condition %d vs %d, lfcThreshold = 1: %s" % (a, b, c))
    _unchanged(dds, snap)


def test_numeric_and_list_contrasts(three):
    """the three forms of one contrast over the names of the expanded matrix give one table"""
    dds, k, x, f = three
    res = core.results(dds, name=2)
    ch = core.lfcShrink(dds, contrast=("condition", 2, 1), res=res, quiet=True)
    num = core.lfcShrink(dds, contrast=[0.0, 0.0, -1.0, 1.0], res=res, quiet=True)
    lst = core.lfcShrink(dds, contrast=[["condition2"], ["condition1"]], res=res, quiet=True)
    live = np.asarray(dds.mcols["baseMean"]) > 0
    for c in ("log2FoldChange", "lfcSE"):
        assert_same(num[c], lst[c], "numeric / list: " + c)
        assert_same(num[c][live], ch[c][live], "numeric / character: " + c)


# ---- the two routes -----------------------------------------------------------------------------------------------------------
def test_lean_route_equals_full_route(two, three):
    for dds, calls in ((two[0], [dict(coef=1), dict(contrast=("condition", 1, 0))]),
                       (three[0], [dict(coef=1), dict(coef=2), dict(contrast=("condition", 2, 1))])):
        for call in calls:
            lean = core.lfcShrink(dds, quiet=True, **call)
            full = core.lfcShrink(dds, lfcThreshold=1, quiet=True, **call)
            for c in ("log2FoldChange", "lfcSE"):
                assert_same(lean[c], full[c], "%r: %s" % (call, c))


def test_lean_route_skips_the_mle_pass(two, monkeypatch):
    """lfcThreshold = 0 runs ONE fit (the ridge pass); lfcThreshold > 0 runs nbinomWaldTest: two"""
    dds = two[0]
    calls = []
    real = core.fitNbinomGLMs
    monkeypatch.setattr(core, "fitNbinomGLMs", lambda *a, **kw: calls.append(kw.get("lam")) or real(*a, **kw))
    core.lfcShrink(dds, coef=1, res=core.results(dds, name=1), quiet=True)
    assert len(calls) == 1 and calls[0] is not None
    del calls[:]
    core.lfcShrink(dds, coef=1, res=core.results(dds, name=1), lfcThreshold=1, quiet=True)
    assert len(calls) == 2 and calls[0] is None and calls[1] is not None


# ---- replaced rows ------------------------------------------------------------------------------------------------------------
def test_replaced_rows_are_refitted_on_the_original_counts(oracle):
    """R's dds.shr is nbinomWaldTest(dds, betaPrior = TRUE, ...): counts(dds) are the ORIGINAL counts also where DESeq()
    refitted on the replaced ones, and the rows left out are those of the allZero column as refitWithoutOutliers left it"""
    f, x, k = _spiked()
    E = HostEngine(oracle)
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=E), factors=f)
    replace = np.asarray(dds.mcols["replace"], np.float64) == 1
    allZero = np.asarray(dds.mcols["allZero"], bool)
    assert replace.sum() >= 5 and allZero[5] and replace[5] and allZero[9] and not replace[9]
    snap = _snapshot(dds)
    got = core.lfcShrink(dds, coef=1, quiet=True)
    thr = core.lfcShrink(dds, coef=1, lfcThreshold=1, quiet=True)
    # the literal sequence: the prior variance from the stored coefficients, then the ridge fit of the rows that are not all
    # zero NOW on dds.y
    view = type("V", (), {"mcols": {"baseMean": dds.mcols["baseMean"][~allZero], "dispFit": dds.mcols["dispFit"][~allZero]}})()
    bpv, _ = core.estimateBetaPriorVar(view, np.asarray(dds.mcols["beta"])[~allZero], ["Intercept", "condition1"])
    assert_same(got.priorInfo["betaPriorVar"], bpv, "betaPriorVar")
    rows = np.where(~allZero)[0]
    sub = core.DESeqDataSet(k[rows], x, engine=E)
    sub.mcols["dispersion"] = np.asarray(dds.mcols["dispersion"])[rows]
    fit = core.fitNbinomGLMs(sub, lam=1.0 / bpv)
    lfc, se = np.full(dds.n, np.nan), np.full(dds.n, np.nan)
    lfc[rows], se[rows] = fit["betaMatrix"][:, 1], fit["betaSE"][:, 1]
    lfc[5] = se[5] = 0.0                                       # nowZero (R/results.R:567-575): replaced, baseMean now 0
    assert_same(got["log2FoldChange"], lfc, "log2FoldChange")
    assert_same(got["lfcSE"], se, "lfcSE")
    assert np.isnan(got["log2FoldChange"][9])
    assert_same(thr["log2FoldChange"], lfc, "log2FoldChange, full route")
    assert_same(thr["lfcSE"], se, "lfcSE, full route")
    assert thr["pvalue"][5] == 1 and thr["stat"][5] == 0
    # ... and NOT on the replaced counts: a spiked row's fit differs between the two
    rc = E.to_numpy(dds.assays["replaceCounts"])
    nz = dds.attrs.get("nz_rows", np.arange(dds.n))
    assert rc.shape[0] == nz.size
    sub_r = core.DESeqDataSet(rc[np.isin(nz, rows)].astype(np.int64), x, engine=E)
    sub_r.mcols["dispersion"] = sub.mcols["dispersion"]
    fit_r = core.fitNbinomGLMs(sub_r, lam=1.0 / bpv)
    spiked_live = replace[rows]
    assert not np.array_equal(fit_r["betaMatrix"][spiked_live, 1], fit["betaMatrix"][spiked_live, 1])
    _unchanged(dds, snap)


# ---- the contrast columns of estimateBetaPriorVar --------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [2, 3, 6])
def test_contrast_columns_in_one_allocation(levels, monkeypatch):
    """addAllContrasts (R/expanded.R:76-98) built at once gives the bits of one column_stack per pair"""
    rng = np.random.default_rng(levels)
    factors = OrderedDict(batch=np.arange(12) % 2, condition=np.arange(12) % levels)
    x, names = core.standard_model_matrix(factors)
    n = 500
    mle = rng.normal(0, 2.0, (n, len(names)))
    view = type("V", (), {"mcols": {"baseMean": np.exp(rng.normal(3, 2, n)), "dispFit": rng.uniform(0.01, 1.0, n)}})()
    beta = mle
    for f in factors:                                          # the loop as it was
        idx = [i for i, nm in enumerate(names) if nm.startswith(f) and nm != "Intercept"]
        for j in range(len(idx) - 1):
            for i in range(j + 1, len(idx)):
                beta = np.column_stack([beta, beta[:, idx[i]] - beta[:, idx[j]]])
    seen = []
    real = core.matchWeightedUpperQuantileForVariance
    monkeypatch.setattr(core, "matchWeightedUpperQuantileForVariance",
                        lambda xc, w, *a, **kw: seen.append(np.array(xc, copy=True)) or real(xc, w, *a, **kw))
    got, enames = core.estimateBetaPriorVar(view, mle, names, modelMatrixType="expanded", factors=factors)
    assert len(seen) == beta.shape[1] and beta.shape[1] == len(names) + (levels - 1) * (levels - 2) // 2
    for c, xc in enumerate(seen):
        col = beta[:, c]
        assert_same(xc, col[np.abs(col) < 10], "column %d" % c)
    # ... and the variances are those of the columns taken one at a time
    w = 1.0 / (1.0 / view.mcols["baseMean"] + view.mcols["dispFit"])
    pv = [1e6] + [real(beta[:, c][np.abs(beta[:, c]) < 10], w[np.abs(beta[:, c]) < 10]) for c in range(1, beta.shape[1])]
    assert got[0] == 1e6 and got[1] == pv[1]                   # batch has two levels: one level column, no contrast ... but
    # averagePriorsOverLevels hands every level column of a factor the mean over its level and contrast columns
    cond = [c for c, nm in enumerate(names) if nm.startswith("condition")] + list(range(len(names), beta.shape[1]))
    mean = float(np.cumsum([pv[c] for c in cond])[-1] / len(cond))
    assert (got[[i for i, nm in enumerate(enames) if nm.startswith("condition")]] == mean).all()
