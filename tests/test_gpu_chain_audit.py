"""-m gpu: tests/hp_reference.py: chain_audit on the device -- every derived column of native.DESeq() (dsq_deseq) and of
fused.DESeq() (the resident dsq_deseq_dev chain) recomputed at 50 digits from the upstream columns the same call returned, on
the cases of tests/chain_cases.py: the smallest shapes at which the glue kernels of csrc/pipeline.hip, csrc/outlier.hip and
csrc/beta_prior.hip still take each of their paths.  The budgets are hp_reference.BUDGETS, measured on the CPU against the
oracle chain (tests/test_chain_audit_cpu.py), never against the device.  The worst ratios are printed (run with -s)."""
import numpy as np
import pytest

from deseq2_amd import core, native
from tests import chain_cases as CC
from tests import hp_reference as H

pytestmark = pytest.mark.gpu

CASES = CC.cases()
_RUNS = {}


def _native(name):
    if name not in _RUNS:
        c = CASES[name]
        _RUNS[name] = native.DESeq(c["counts"], c["x"], c["sizeFactors"], assays=("mu", "H", "cooks", "replaceCounts"),
                                   **CC.native_kwargs(c))
    return _RUNS[name]


def _fits():
    return {"exact": native.parametricDispersionFit, "restated": (core.parametricDispersionFit, 1e-9)}


def _check(name, c, res, trend_fits):
    refit = bool(np.nansum(res["replace"]) > 0)
    R = H.chain_audit(c, res, scalars=not refit, trend_fits=trend_fits)
    print("%s %s ties %s" % (name, R.summary(), R.ties))
    assert not R.failures, R.failures[:10]
    for k, v in R.ratios.items():
        K = H.BUDGETS[H._BUDGET_OF.get(k, k)]
        assert v <= K, "%s %s: ratio %.3g over K = %g (row %s)" % (name, k, v, K, R.where[k])
    live = np.nan_to_num(res["allZero"], nan=1.0) == 0
    assert R.ties.get("dispOutlier", 0) <= 0.01 * live.sum()
    lrt = c.get("test") == "LRT"
    for fam in ("baseMean", "dispMAP", "dispersion", "mu", "betaSE", "cooks", "maxCooks", "dispPriorVar") + (
            () if lrt else ("stat", "pvalue")) + (() if refit else ("varLogDispEsts",) + (("trend",) if trend_fits else ())):
        assert R.counts.get(fam, 0) > 0, fam
    assert R.counts.get("logLikeReduced", 0) + R.counts.get("LRTStatistic", 0) > 0 or not lrt
    return R


def _same_scalars(a, b):
    assert np.nansum(a["replace"]) > 0 and not np.nansum(b["replace"]) > 0
    fa, fb = a["dispersionFunction"], b["dispersionFunction"]
    assert np.array_equal(np.asarray(fa["coefficients"]), np.asarray(fb["coefficients"]))
    assert fa["varLogDispEsts"] == fb["varLogDispEsts"] and fa["dispPriorVar"] == fb["dispPriorVar"]
    if "betaPriorVar" in a:
        assert np.array_equal(a["betaPriorVar"], b["betaPriorVar"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_audit_holds_for_the_host_entry(name):
    _check(name, CASES[name], _native(name), _fits())


@pytest.mark.parametrize("refit,plain", CC.REFIT_PAIRS)
def test_a_refit_reuses_the_all_gene_scalars(refit, plain):
    """R/core.R:2512-2527: the scalars audited on the run without a refit are bit-identical on the run with it"""
    _same_scalars(_native(refit), _native(plain))


_RESIDENT = {}


def _resident(name):
    if name not in _RESIDENT:
        from deseq2_amd import fused
        from deseq2_amd.engine import DeviceEngine
        c = CASES[name]
        dds = core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], engine=DeviceEngine("cuda:0"))
        assert fused.supported(dds, **CC.chain_kwargs(c))
        fused.DESeq(dds, **CC.chain_kwargs(c))
        assert dds.attrs.get("fused")
        _RESIDENT[name] = CC.result_of(dds)
    return _RESIDENT[name]


@pytest.mark.parametrize("name", ["bc_outliers", "bc_no_refit", "bc_lrt"])
def test_the_audit_holds_for_the_resident_chain(name):
    """fused.DESeq() (dsq_deseq_dev): the second case with minReplicatesForReplace 7 and +Inf -- the all-gene scalars are audited
    on the latter -- and under LRT, where 2 (logLike - logLikeReduced) is held at the full model's logLike"""
    _check(name + " (resident)", CASES[name], _resident(name), _fits())


@pytest.mark.parametrize("refit", ["bc_outliers", "bc_lrt"])
def test_a_resident_refit_reuses_the_all_gene_scalars(refit):
    _same_scalars(_resident(refit), _resident("bc_no_refit"))
