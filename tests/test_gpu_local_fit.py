"""-m gpu: fitType = "local" on the device (csrc/local_fit.hip).  dsq_local_fit_dev and dsq_local_fit
equal the numpy specification of tests/local_fit_spec.py BIT FOR BIT on every case of tests/local_fit_cases.py; a fit
handle evaluated later gives the bits of a fresh call; fused.DESeq(fitType = "local") equals core.DESeq(fitType = "local")
column for column with and without the outlier refit, and brings no n-vector to the host between its phases; vst and rlog
with the local trend agree between the device and the host engine."""
import numpy as np
import pytest

from tests import local_fit_cases as CS
from tests import local_fit_spec as S
from tests.helpers import assert_bits, assert_same

from deseq2_amd import core, fused, native, simulate
from deseq2_amd.engine import DeviceEngine, HostEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    return DeviceEngine("cuda:0")


def _dev(E, a):
    return E.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=E.device)


# ---------------------------------------------------------------------------------------------- bitwise: device == spec
@pytest.mark.parametrize("fit_name,which", CS.PAIRS)
def test_device_equals_the_specification(E, oracle, fit_name, which):
    t = E.torch
    ref, nsing, fit = CS.reference(oracle, fit_name, which)
    means, disps = CS.FIT_SETS[fit_name]
    q = CS.eval_list(fit_name, which)
    # the resident entry, its outputs prefilled with garbage
    out = t.full((q.size,), -7.25, dtype=t.float64, device=E.device)
    r = native.local_fit_dev(_dev(E, means), _dev(E, disps), CS.MIN_DISP, eval_means=_dev(E, q), out=out)
    st = r["status"].cpu().numpy()
    assert_bits(out.cpu().numpy(), ref, "dsq_local_fit_dev: %s / %s" % (fit_name, which))
    assert tuple(st) == (fit[0].size, fit[3], nsing, int(fit[0].size == 0))
    N = fit[0].size
    if N:       # the handle: the header's N, k and x | y | w of the fit set in sorted order
        blk = r["fit"].cpu().numpy()
        n = means.size
        assert tuple(blk[:2].view(np.int32)) == (N, fit[3], 0, n) and blk[2] == CS.MIN_DISP
        for j, name in enumerate("xyw"):
            assert_bits(blk[4 + j * n: 4 + j * n + N], fit[j], "fit handle: " + name)
    # the host entry
    h = native.local_fit(means, disps, CS.MIN_DISP, eval_means=q)
    assert_bits(h["dispFit"], ref, "dsq_local_fit: %s / %s" % (fit_name, which))
    assert (h["N"], h["k"], h["nSingular"], h["allBelowFloor"]) == tuple(st)


def test_evaluating_at_the_fit_means_themselves(E, oracle):
    means, disps = CS.FIT_SETS["mixed"]
    fit = S.local_fit(oracle, means, disps, CS.MIN_DISP)
    ref, nsing = S.evaluate(oracle, fit, means)
    r = native.local_fit_dev(_dev(E, means), _dev(E, disps), CS.MIN_DISP)
    assert_bits(r["dispFit"].cpu().numpy(), ref, "dsq_local_fit_dev at means")
    h = native.local_fit(means, disps, CS.MIN_DISP)
    assert_bits(h["dispFit"], ref, "dsq_local_fit at means")
    assert h["nSingular"] == nsing == int(r["status"][2])


@pytest.mark.parametrize("fit_name", ["n129", "ties", "all_below"])
def test_a_fit_built_once_evaluates_like_fresh_calls(E, oracle, fit_name):
    means, disps = CS.FIT_SETS[fit_name]
    qa, qb = CS.eval_list(fit_name, "n65"), CS.eval_list(fit_name, "special")
    built = native.local_fit_dev(_dev(E, means), _dev(E, disps), CS.MIN_DISP, evaluate=False)
    assert built["dispFit"] is None
    for q in (qa, qb):
        fresh = native.local_fit_dev(_dev(E, means), _dev(E, disps), CS.MIN_DISP, eval_means=_dev(E, q))
        later = native.local_fit_dev(fit=built["fit"], eval_means=_dev(E, q), minDisp=CS.MIN_DISP)
        assert_bits(later["dispFit"].cpu().numpy(), fresh["dispFit"].cpu().numpy(), "later against fresh")
        assert (later["status"] == fresh["status"]).all()
    # ... and through the host entry, the block travelling through host memory
    hb = native.local_fit(means, disps, CS.MIN_DISP, evaluate=False)
    for q, which in ((qa, "n65"), (qb, "special")):
        again = native.local_fit(fit=hb["fit"], eval_means=q, minDisp=CS.MIN_DISP)
        assert_bits(again["dispFit"], CS.reference(oracle, fit_name, which)[0], "host block, " + which)
    # the engine's object: host means in, host values out; resident means in, resident values out
    f = E.local_fit(means, disps, CS.MIN_DISP)
    assert_bits(f(qa), CS.reference(oracle, fit_name, "n65")[0], "DeviceEngine.local_fit")
    assert_bits(f(_dev(E, qb)).cpu().numpy(), CS.reference(oracle, fit_name, "special")[0], "DeviceEngine.local_fit, resident")
    assert f(qa.reshape(5, 13)).shape == (5, 13) and f.nSingular == CS.reference(oracle, fit_name, "n65")[1]


@pytest.mark.parametrize("name", sorted(CS.TOO_FEW))
def test_fewer_than_three_points_in_a_window_raises(E, name):
    means, disps = CS.TOO_FEW[name]
    with pytest.raises(RuntimeError, match="fewer than 3 points in a window"):
        native.local_fit(means, disps, CS.MIN_DISP)
    with pytest.raises(RuntimeError, match="fewer than 3 points in a window"):
        E.local_fit(means, disps, CS.MIN_DISP)
    r = native.local_fit_dev(_dev(E, means), _dev(E, disps), CS.MIN_DISP)          # the resident entry reports: N, k, all NaN
    assert tuple(r["status"].cpu().numpy()[:2]) == (means.size, S.bandwidth(means.size))
    assert np.isnan(r["dispFit"].cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------- the chain
def _outlier_case():
    x = simulate.design_two_group(14)                       # two groups of seven: replaceOutliers + refit
    d = simulate.make_counts(300, x, seed=21)
    counts = d["counts"].copy()
    rng = np.random.default_rng(4)
    for r in rng.choice(counts.shape[0], 6, replace=False):
        counts[r, rng.integers(14)] = int(counts[r].max() * 40 + 1000)
    return counts, x, d["size_factors"]


def _compare(a, b, what):
    E = a.engine
    keys = [k for k in a.mcols if k != "rowsForOptim"]
    assert set(keys) <= set(b.mcols) | {"rowsForOptim"}, (sorted(keys), sorted(b.mcols))
    for k in keys:
        assert_same(np.asarray(a.mcols[k]).astype(np.float64), np.asarray(b.mcols[k]).astype(np.float64), "%s: mcols$%s" % (what, k))
    assert_bits(a.mcols["dispFit"], b.mcols["dispFit"], what + ": dispFit")
    fa, fb = a.dispersionFunction, b.dispersionFunction
    assert fa["fitType"] == fb["fitType"] == "local"
    assert fa["varLogDispEsts"] == fb["varLogDispEsts"] and fa["dispPriorVar"] == fb["dispPriorVar"], what
    probe = np.exp(np.linspace(0.0, 8.0, 33))
    assert_bits(fa["coefficients"](probe), fb["coefficients"](probe), what + ": the stored function")
    for k in ("mu", "H", "cooks"):
        assert_same(E.to_numpy(a.assays[k]), E.to_numpy(b.assays[k]), "%s: assays$%s" % (what, k))


@pytest.mark.parametrize("replace", [True, False])
def test_fused_chain_equals_the_call_by_call_chain(E, replace):
    counts, x, sf = _outlier_case()
    kw = {} if replace else {"minReplicatesForReplace": np.inf}
    a = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
    core.DESeq(a, fitType="local", **kw)
    b = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
    assert fused.supported(b, fitType="local")
    # every copy the engine brings to the host while the chain is enqueued: the fit's status words, nothing of length n
    copied, host = [], E._host
    E._host = lambda v: copied.append(int(v.numel())) or host(v)
    try:
        fused.DESeq(b, fitType="local", **kw)
    finally:
        E._host = host
    assert b.attrs.get("fused")
    assert copied and max(copied) <= 4, copied
    if replace:
        assert b.attrs["status"]["N_REPLACE"] >= 3 and b.attrs["status"]["N_REFIT"] >= 3       # the refit at new means ran
        assert a.mcols["replace"].sum() == b.attrs["status"]["N_REPLACE"]
    else:
        assert "replace" not in b.mcols
    _compare(a, b, "fused, replace = %s" % replace)


def test_vst_and_rlog_with_the_local_trend_agree_across_engines(E, oracle):
    """Given size factors, so that both engines fit the trend to the same bits: the local trend itself -- the spline table of
    vst, the dispFit of rlog -- is then equal bit for bit.  The transforms differ as they do for every trend, by libm's log /
    asinh / log2 on the host engine against the device's pinned ones: vst within twice tests/vst_spec.py's derived distance
    to the exact value (tests/test_gpu_vst.py), rlog within tests/rlog_cases.py's tolerance (tests/test_gpu_rlog.py)."""
    from tests import rlog_cases, vst_spec
    H = HostEngine(oracle)
    x = simulate.design_two_group(6)
    d = simulate.make_counts(1300, x, seed=8)
    objs = [core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=eng) for eng in (E, H)]
    a, b = (core.vst(o, fitType="local") for o in objs)
    assert a.dds.dispersionFunction["fitType"] == b.dds.dispersionFunction["fitType"] == "local"
    sa, sb = a.dds.attrs["vst_spline"], b.dds.attrs["vst_spline"]
    assert_bits(sa["table"], sb["table"], "vst: spline table")
    A, B = a.assay(), b.assay()
    q = np.asarray(H.to_numpy(core.normalized_counts(b.dds).handle))
    bound = 2 * vst_spec.spline_bound(sb["table"], sb["eta"], sb["xi"], np.arcsinh(q), B)
    assert np.isfinite(A).all() and (np.abs(A - B) <= bound).all()
    small = [core.DESeqDataSet(d["counts"][:150], x, sizeFactors=d["size_factors"], engine=eng) for eng in (E, H)]
    ra, rb = (core.rlog(o, fitType="local") for o in small)
    assert ra.dds.dispersionFunction["fitType"] == "local"
    assert_bits(ra.dds.mcols["dispFit"], rb.dds.mcols["dispFit"], "rlog: dispFit")
    assert abs(ra.attrs["betaPriorVar"] - rb.attrs["betaPriorVar"]) <= 1e-12 * rb.attrs["betaPriorVar"]
    rlog_cases.compare(ra.assay(), rb.assay(), "rlog, local trend", ra.dds.mcols["rlogIter"], rb.dds.mcols["rlogIter"])
