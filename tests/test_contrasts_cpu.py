"""CPU: core.resultsContrasts over HostEngine(oracle) (R/results.R:375-438, 760-1040, 1146-1270) against
the reference's known answers (tests/testthat/test_results.R:43-56), against the numpy statement tests/contrast_spec.py bit
for bit, and against the independent LAPACK restatement of fitBeta."""
from collections import OrderedDict

import json
import os

import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import contrast_spec as CS
from tests.helpers import assert_same

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "nmath_golden.json")))
COLS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj")


def _factors12():
    return OrderedDict(group=np.tile([0, 1], 6), condition=np.repeat([0, 1, 2], 4))


def _counts(n, x, seed):
    from deseq2_amd import simulate
    return simulate.make_counts(n, x, seed=seed, drop_all_zero=False)["counts"]


@pytest.fixture(scope="module")
def kat(oracle):
    """test_results.R:5-20: ~ group + condition on 12 samples, gene 0 the perfect-fit gene; gene 7 has zeros in condition
    levels 1 and 2, gene 8 in levels 0 and 1, gene 9 everywhere"""
    f = _factors12()
    x, _ = core.standard_model_matrix(f)
    k = _counts(200, x, 5)
    k[0] = GOLD["kat"]["test_results_R_9_43_50"]["counts"]
    k[7, f["condition"] != 0] = 0
    k[7, f["condition"] == 0] = [30, 41, 28, 35]
    k[8, f["condition"] != 2] = 0
    k[8, f["condition"] == 2] = [50, 61, 48, 55]
    k[9] = 0
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f)
    return dds, k, f


def _spec_inputs(dds):
    n = dds.n
    nf = np.broadcast_to(dds.sizeFactors[None, :], (n, dds.m)) if dds.sizeFactors is not None else np.asarray(dds.nf)
    bpv = dds.attrs.get("betaPriorVar", np.full(np.shape(dds.mcols["beta"])[1], 1e6))
    return dict(nf=nf, dispersion=dds.mcols["dispersion"], beta_log2=dds.mcols["beta"], betaPriorVar=bpv,
                allZero=dds.mcols["allZero"])


def _same_tables(a, b, what, cols=COLS):
    for c in cols:
        assert_same(a[c], b[c], "%s$%s" % (what, c))


def _against_spec(oracle, res, cols, dds, mask, counts, what, lrt=None, **kw):
    """the DESeqResults `res` against contrast_spec.contrast_table on the four columns `cols`"""
    rep = dds.mcols.get("replace")
    rep = None if rep is None else np.asarray(rep) == 1
    theta = res.metadata["filterNumRej"]["theta"]
    t = CS.contrast_table(oracle, cols, dds.mcols["baseMean"], mask, counts, dds.mcols["allZero"], lrt=lrt, replace=rep,
                          theta=theta, **kw)
    for c in COLS[:5]:
        assert_same(res[c], t[c], "%s$%s" % (what, c))
    assert_same(res.metadata["filterNumRej"]["numRej"], t["numRej"], what + " numRej")
    j = int(np.where(theta == res.metadata["filterTheta"])[0][0])
    assert_same(res["padj"], t["filtPadj"][:, j], what + "$padj")


def test_known_answers_and_three_forms(oracle, kat):
    """test_results.R:43-50: condition 1 vs 3 = -3, 1 vs 2 = -1, 2 vs 3 = -2 on the perfect-fit gene, as character, list and
    numeric contrast; the three forms of one contrast give the same table bit for bit"""
    dds, k, f = kat
    names = core.resultsNames(dds)
    assert names == ["Intercept", "coef1", "coef2", "coef3"]
    dds.attrs["coefNames"] = ["Intercept", "group_1_vs_0", "condition_1_vs_0", "condition_2_vs_0"]
    try:
        forms = {
            -3.0: [("condition", 0, 2), [[], ["condition_2_vs_0"]], [0, 0, 0, -1]],
            -1.0: [("condition", 0, 1), [[], ["condition_1_vs_0"]], [0, 0, -1, 0]],
            -2.0: [("condition", 1, 2), [["condition_1_vs_0"], ["condition_2_vs_0"]], [0, 0, 1, -1]],
        }
        for want, three in forms.items():
            res = core.resultsContrasts(dds, three, cooksCutoff=False)
            for r in res:
                assert r["log2FoldChange"][0] == pytest.approx(want, abs=1e-6)
            _same_tables(res[1], res[2], "list vs numeric %g" % want)
            if want == -2.0:       # (against the reference level the character form pulls stored columns: see the next test)
                _same_tables(res[0], res[1], "character vs list")
        r = core.resultsContrasts(dds, [[["condition_2_vs_0"], ["condition_1_vs_0"]]])[0]        # test_results.R:53-55
        assert r["log2FoldChange"][0] == pytest.approx(2.0, abs=1e-6)
        assert r.metadata["contrast"] == "condition_2_vs_0 vs condition_1_vs_0"
        assert core.resultsContrasts(dds, [[0, 0, 1, -1]])[0].metadata["contrast"] == "0,0,+1,-1"
        assert core.resultsContrasts(dds, [("condition", 1, 2)])[0].metadata["contrast"] == "condition 1 vs 2"
    finally:
        dds.attrs.pop("coefNames")


def test_pull_and_swap(oracle, kat):
    """:876-932: a character contrast against the reference level IS the stored coefficient; with the levels swapped the fold
    change and the Wald statistic change sign, nothing else changes"""
    dds, k, f = kat
    a, b = core.resultsContrasts(dds, [("condition", 1, 0), ("condition", 0, 1)])
    # (gene 8 has zeros in both levels: cleanContrast's zero rule applies to the pulled columns and not to results(name = ))
    z = CS.all_zero(k, CS.mask_character(f["condition"], 1, 0), dds.mcols["allZero"])
    assert z[8] and not z[7] and not z[9]
    ref = core.results(dds, name=2)
    keep = ~z
    for c in COLS[:5]:
        assert_same(a[c][keep], ref[c][keep], "pulled$" + c)
    assert (a["log2FoldChange"][z] == 0).all() and (a["stat"][z] == 0).all() and (a["pvalue"][z] == 1).all()
    assert_same(a["lfcSE"][z], ref["lfcSE"][z], "lfcSE keeps its value")
    assert_same(b["log2FoldChange"], -a["log2FoldChange"], "swapped lfc")
    assert_same(b["stat"], -a["stat"], "swapped stat")
    for c in ("baseMean", "lfcSE", "pvalue", "padj"):
        assert_same(b[c], a[c], "swapped$" + c)
    # ... and on a gene-for-gene basis equal to results(name = ) when no row is flagged
    a1 = core.resultsContrasts(dds, [("group", 1, 0)])[0]
    assert not CS.all_zero(k, CS.mask_character(f["group"], 1, 0), dds.mcols["allZero"]).any()
    _same_tables(a1, core.results(dds, name=1), "group 1 vs 0")
    stored = {"log2FoldChange": dds.mcols["beta"][:, 2], "lfcSE": dds.mcols["betaSE"][:, 2], "stat": dds.mcols["WaldStatistic"][:, 2],
              "pvalue": dds.mcols["WaldPvalue"][:, 2]}
    _against_spec(oracle, a, stored, dds, CS.mask_character(f["condition"], 1, 0), k, "pulled vs spec",
                  na_mask=core._cooks_flags(dds, None) if "maxCooks" in dds.mcols else None)


def test_error_messages(oracle, kat):
    dds, k, f = kat
    rc = lambda c, **kw: core.resultsContrasts(dds, [c], **kw)
    for bad in (False, "condition", {"a": 1}):                                    # test_results.R:30; :1147-1151
        with pytest.raises(ValueError, match="should be either a character vector of length 3"):
            rc(bad)
    with pytest.raises(ValueError, match="as a character vector of length 3, should have the form"):
        rc(("a", "b", "c", "d"))                                                  # test_results.R:31
    with pytest.raises(ValueError, match="1 and 1 should be different level names"):
        rc(("condition", 1, 1))                                                   # test_results.R:32
    with pytest.raises(ValueError, match="foo should be the name of a factor"):
        rc(("foo", 1, 0))                                                         # test_results.R:27,42
    with pytest.raises(ValueError, match="as 0 is the reference level, was expecting condition_3_vs_0"):
        rc(("condition", 3, 0))                                                   # test_results.R:28
    with pytest.raises(ValueError, match="as 0 is the reference level, was expecting condition_3_vs_0"):
        rc(("condition", 0, 3))
    with pytest.raises(ValueError, match="1 and 5 should be levels of condition such that condition_1_vs_0 and condition_5_vs_0"):
        rc(("condition", 1, 5))
    with pytest.raises(ValueError, match="as a list, should have length 2"):
        rc([["coef2"], ["coef3"], ["coef3"]])                                     # test_results.R:35
    with pytest.raises(ValueError, match="should have character vectors as elements"):
        rc([["coef2"], [1]])                                                      # test_results.R:36
    with pytest.raises(ValueError, match="should be elements of 'resultsNames"):
        rc([["coef2"], ["foo"]])                                                  # test_results.R:37
    with pytest.raises(ValueError, match="but not both"):
        rc([["coef2"], ["coef2"]])                                                # test_results.R:38
    with pytest.raises(ValueError, match="non-zero length"):
        rc([[], []])                                                              # test_results.R:39
    with pytest.raises(ValueError, match="one element for every element"):
        rc([0, 1, 0])
    with pytest.raises(ValueError, match="cannot have all elements equal to 0"):
        rc([0, 0, 0, 0])                                                          # test_results.R:40
    with pytest.raises(ValueError, match="listValues"):
        rc([0, 0, 1, -1], listValues=(1, 1))
    with pytest.raises(ValueError, match="sequence of contrasts"):
        core.resultsContrasts(dds, "condition")
    for kw in ({"addMLE": True}, {"parallel": True}):
        with pytest.raises(NotImplementedError):
            rc([0, 0, 1, -1], **kw)
    with pytest.raises(TypeError):
        rc([0, 0, 1, -1], name="coef1")
    # a character contrast needs the factors, and the matrix they generate
    saved = dds.attrs["factors"]
    try:
        dds.attrs["factors"] = None
        with pytest.raises(ValueError, match="numeric"):
            rc(("condition", 1, 2))
        dds.attrs["factors"] = OrderedDict(condition=saved["condition"])
        with pytest.raises(ValueError, match="numeric"):
            rc(("condition", 1, 2))
        dds.attrs["useT"] = True
        with pytest.raises(NotImplementedError, match="Student-t"):
            rc([0, 0, 1, -1])
    finally:
        dds.attrs["factors"] = saved
        dds.attrs["useT"] = False
    d2 = core.DESeqDataSet(k, dds.x, engine=HostEngine(oracle))
    with pytest.raises(RuntimeError, match="first run DESeq"):
        core.resultsContrasts(d2, [[0, 0, 1, -1]])


def test_results_contrast_still_not_implemented(kat):
    with pytest.raises(NotImplementedError, match="resultsContrasts"):
        core.results(kat[0], contrast=[0, 0, 1, -1])


def test_list_values_and_spec(oracle, kat):
    """listValues = (0.5, -0.5) (test_results.R:56-61): the numeric contrast it builds, its name, the table against the spec"""
    dds, k, f = kat
    c = np.array([0, 0, -0.5, 0.5])
    rl, rn, r1, r2 = core.resultsContrasts(dds, [[["coef3"], ["coef2"]], c, [["coef3"]], [[], ["coef2"]]], listValues=(0.5, -0.5),
                                           cooksCutoff=False)
    _same_tables(rl, rn, "listValues")
    assert rl.metadata["contrast"] == "0.5 coef3 vs 0.5 coef2" and rn.metadata["contrast"] == "0,0,-0.5,+0.5"
    assert r1.metadata["contrast"] == "0.5 coef3 effect" and r2.metadata["contrast"] == "-0.5 coef2 effect"
    x = dds.x
    sp = _spec_inputs(dds)
    _against_spec(oracle, rl, CS.get_contrast(oracle, x, c=c, **sp), dds, CS.mask_numeric(x, c), k, "listValues vs spec")
    c1 = np.array([0, 0, 0, 0.5])
    assert CS.mask_numeric(x, c1) is None
    _against_spec(oracle, r1, CS.get_contrast(oracle, x, c=c1, **sp), dds, None, k, "one-sided list vs spec")


def test_all_zero_rule(oracle, kat):
    """:1021-1028, :1245-1270: zeros in both contrasted groups -> 0 / kept SE / 0 / 1; a one-sign numeric contrast is not
    zeroed; an all-zero gene is NA"""
    dds, k, f = kat
    c = np.array([0.0, 0.0, 1.0, -1.0])
    one_sign = np.array([0.0, 0.0, 1.0, 1.0])
    a, b = core.resultsContrasts(dds, [c, one_sign], cooksCutoff=False)
    sp = _spec_inputs(dds)
    raw = CS.get_contrast(oracle, dds.x, c=c, **sp)
    assert a["log2FoldChange"][7] == 0 and a["stat"][7] == 0 and a["pvalue"][7] == 1
    assert a["lfcSE"][7] == raw["lfcSE"][7] and np.isfinite(raw["lfcSE"][7]) and raw["log2FoldChange"][7] != 0
    assert b["log2FoldChange"][7] != 0 and b["pvalue"][7] != 1
    for r in (a, b):
        for col in COLS[1:]:
            assert np.isnan(r[col][9]), col
    assert dds.mcols["allZero"][9] and a["baseMean"][9] == 0
    _against_spec(oracle, a, raw, dds, CS.mask_numeric(dds.x, c), k, "zero rule vs spec")
    _against_spec(oracle, b, CS.get_contrast(oracle, dds.x, c=one_sign, **sp), dds, None, k, "one sign vs spec")
    # ... with the default Cook's filter too
    a2 = core.resultsContrasts(dds, [c])[0]
    _against_spec(oracle, a2, raw, dds, CS.mask_numeric(dds.x, c), k, "with Cook's mask",
                  na_mask=core._cooks_flags(dds, None) if "maxCooks" in dds.mcols else None)
    # ... and a threshold test runs on the contrast's columns
    a3 = core.resultsContrasts(dds, [c], lfcThreshold=0.5, altHypothesis="greater", cooksCutoff=False)[0]
    _against_spec(oracle, a3, raw, dds, CS.mask_numeric(dds.x, c), k, "threshold", lfcThreshold=0.5, altHypothesis="greater")


def test_independent_lapack(oracle, kat):
    """num and den against the LAPACK restatement of fitBeta(maxit = 0), at the tolerances tests/test_oracle_vs_lapack.py
    applies to contrast_num / contrast_denom (rtol 1e-7, atol 1e-12)"""
    from oracle import lapack_oracle as F
    dds, k, f = kat
    nz = ~dds.mcols["allZero"]
    sp = _spec_inputs(dds)
    for c in ([0, 0, 1, -1], [0, 1, -0.5, -0.5], [1, 0, 0, 1]):
        got = CS.get_contrast(oracle, dds.x, c=np.asarray(c, float), **sp)
        ref = F.fitBeta(k[nz].astype(float), dds.x, sp["nf"][nz], sp["dispersion"][nz], np.asarray(c, float),
                        CS.LN2 * sp["beta_log2"][nz], 1.0 / (CS.LN2 ** 2 * sp["betaPriorVar"]), np.ones((int(nz.sum()), dds.m)), False,
                        1e-8, 0, False, 0.5)
        np.testing.assert_allclose(got["log2FoldChange"][nz] / CS.LOG2E, np.reshape(ref["contrast_num"], -1), rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(got["lfcSE"][nz] / CS.LOG2E, np.reshape(ref["contrast_denom"], -1), rtol=1e-7, atol=1e-12)
        res = core.resultsContrasts(dds, [c], cooksCutoff=False)[0]
        z = CS.all_zero(k, CS.mask_numeric(dds.x, c), dds.mcols["allZero"])
        assert_same(res["lfcSE"], got["lfcSE"], "engine lfcSE")
        assert_same(res["log2FoldChange"][~z], got["log2FoldChange"][~z], "engine lfc")


def test_lrt_object(oracle, kat):
    """:1030-1037: on an LRT analysis the fold change and its error come from the contrast, stat and pvalue are the LRT's"""
    _, k, f = kat
    x, _ = core.standard_model_matrix(f)
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), test="LRT", reduced=x[:, :2])
    dds.attrs["factors"] = f
    c = np.array([0.0, 0.0, 1.0, -1.0])
    rn, rc, rp = core.resultsContrasts(dds, [c, ("condition", 1, 2), ("condition", 0, 1)], cooksCutoff=False)
    _same_tables(rn, rc, "LRT numeric vs character")
    sp = _spec_inputs(dds)
    lrt = (dds.mcols["LRTStatistic"], dds.mcols["LRTPvalue"])
    _against_spec(oracle, rn, CS.get_contrast(oracle, x, c=c, **sp), dds, CS.mask_numeric(x, c), k, "LRT vs spec", lrt=lrt)
    assert_same(rn["stat"], dds.mcols["LRTStatistic"], "stat is the LRT's")
    assert rn["log2FoldChange"][7] == 0 and rn["pvalue"][7] == dds.mcols["LRTPvalue"][7]
    # the swap negates the fold change only (:917)
    assert_same(rp["log2FoldChange"], np.where(CS.all_zero(k, CS.mask_character(f["condition"], 0, 1), dds.mcols["allZero"]), 0.0,
                                               -dds.mcols["beta"][:, 2]), "LRT swapped lfc")
    assert_same(rp["stat"], dds.mcols["LRTStatistic"], "LRT swapped stat")


def test_beta_prior_expanded(oracle, kat):
    """betaPrior = TRUE with factors: the coefficients live on the expanded model matrix (:946-954), a level-vs-level
    contrast goes through its columns with lambda = 1 / (log(2)^2 betaPriorVar)"""
    _, k, f = kat
    x, _ = core.standard_model_matrix(f)
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), betaPrior=True, factors=f)
    assert dds.attrs["modelMatrixType"] == "expanded" and np.shape(dds.mcols["beta"])[1] == 6
    xe, _ = core.makeExpandedModelMatrix(f)
    ra, rb = core.resultsContrasts(dds, [("condition", 2, 0), [0, 0, 0, -1, 0, 1]], cooksCutoff=False)
    _same_tables(ra, rb, "expanded character vs numeric")
    c = np.array([0, 0, 0, -1, 0, 1.0])
    sp = _spec_inputs(dds)
    assert (np.asarray(sp["betaPriorVar"]) != 1e6).any()
    _against_spec(oracle, ra, CS.get_contrast(oracle, xe, c=c, **sp), dds, CS.mask_numeric(xe, c), k, "expanded vs spec")
    assert ra.priorInfo["type"] == "normal"
    with pytest.raises(ValueError, match="condition3 and condition0 are expected to be in resultsNames"):
        core.resultsContrasts(dds, [("condition", 3, 0)])


def test_weights(oracle, kat):
    """observation weights enter normalised by the row maximum (:787-795)"""
    _, k, f = kat
    x, _ = core.standard_model_matrix(f)
    rng = np.random.default_rng(8)
    w = rng.uniform(0.3, 1.0, k.shape)
    c = np.array([0.0, 0.0, 1.0, -1.0])
    dw = core.DESeq(core.DESeqDataSet(k, x, weights=w, engine=HostEngine(oracle)), factors=f)
    rw = core.resultsContrasts(dw, [c], cooksCutoff=False)[0]
    _against_spec(oracle, rw, CS.get_contrast(oracle, x, c=c, weights=w, **_spec_inputs(dw)), dw, CS.mask_numeric(x, c), k, "weighted")
    unweighted = CS.get_contrast(oracle, x, c=c, **_spec_inputs(dw))
    assert not np.array_equal(unweighted["lfcSE"][:7], rw["lfcSE"][:7])


def test_replaced_outliers_are_judged_on_the_original_counts(oracle):
    """:1239, :1268: contrastAllZero* read counts(object), not replaceCounts"""
    f = OrderedDict(condition=np.repeat([0, 1, 2], 7))
    x, _ = core.standard_model_matrix(f)
    k = _counts(150, x, 9)
    k[4, f["condition"] == 0] = [30, 25, 28, 0, 0, 0, 0]
    k[4, f["condition"] != 0] = 0
    k[4, 8] = 60000                                   # the one non-zero count of levels 1 and 2: replaced by the trimmed mean, 0
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f)
    E = dds.engine
    assert np.asarray(dds.mcols["replace"])[4] == 1
    nz = dds.attrs.get("nz_rows")
    row = 4 if nz is None else int(np.where(nz == 4)[0][0])
    assert (np.asarray(E.to_numpy(dds.assays["replaceCounts"]))[row, f["condition"] != 0] == 0).all()
    c = np.array([0.0, 1.0, -1.0])
    r = core.resultsContrasts(dds, [c], cooksCutoff=False)[0]
    assert r["log2FoldChange"][4] != 0 and r["pvalue"][4] != 1
    _against_spec(oracle, r, CS.get_contrast(oracle, x, c=c, **_spec_inputs(dds)), dds, CS.mask_numeric(x, c), k, "replaced")
    k2 = k.copy()
    k2[4, 8] = 0                                      # the same gene without the outlier IS zeroed
    assert CS.all_zero(k2, CS.mask_numeric(x, c), np.zeros(150, bool))[4]
