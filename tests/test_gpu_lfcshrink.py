"""lfcShrink(type = "normal") on the device.
1. dsq_beta_prior_var_dev (csrc/beta_prior.hip: keys, the batched radix sort of results.hip, one wave per column for the
   order-sensitive sums) == dsq_beta_prior_var (host threads) == core.estimateBetaPriorVar (the line-cited mirror), BIT FOR
   BIT, NaN included: all three follow one definition, sum for sum.
2. core.lfcShrink over the DeviceEngine == over HostEngine(oracle), every returned column and betaPriorVar bit for bit."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from tests.helpers import assert_same
from tests.lfcshrink_cases import counts as _counts, spiked as _spiked

pytestmark = pytest.mark.gpu

COLS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj")


@pytest.fixture(scope="module")
def engine():
    from deseq2_amd.engine import DeviceEngine
    return DeviceEngine("cuda:0")


# ---- 1. the prior variance ---------------------------------------------------------------------------------------------------
# columns: (levels of the one factor, expanded): 2 columns; 3 columns; 3 + 3; 12 + 55 (more than one batch of 64 columns)
SHAPES = {"two_groups": (2, False), "factor3": (3, False), "factor3_expanded": (3, True), "factor12_expanded": (12, True)}


def _prior_case(n, shape, seed, planted):
    """MLE coefficients, baseMean, dispFit, all-zero flags.  planted (n >= 63): ties in |x| (exact duplicates, +- pairs; at
    n > 2048 a run of one value longer than a sort tile), |x| at and beyond 10, NaN coefficients, NaN dispFit, a baseMean so
    small that the weight underflows to 0, all-zero rows; standard matrices only (the expanded one refuses a variance that
    is not > 0): a column with no row under 10 (1e6) and one whose rows under 10 all carry a NaN weight (NaN)"""
    levels, expanded = SHAPES[shape]
    rng = np.random.Generator(np.random.PCG64(seed))
    factors = OrderedDict(condition=np.arange(2 * levels) % levels)
    p = levels
    mle = rng.normal(0, 1.5, (n, p)) * rng.choice([1.0, 1.0, 1.0, 8.0], (n, 1))
    mle[:, 0] = rng.normal(5, 2, n)
    bm = np.exp(rng.normal(3, 2, n))
    dfit = 0.05 + 3.0 / bm
    az = np.zeros(n, bool)
    if planted and n >= 63:
        mle[::7, 1] = 0.25
        mle[1::7, 1] = -0.25
        mle[2::7, 1] = 0.25
        if n > 2048:
            mle[100:2300, p - 1] = -0.5                        # one run of 2200 equal values
        mle[3, 1:] = 10.0                                      # at 10: not < 10
        mle[4, 1:] = -10.0
        mle[5, 1:] = 12.5
        mle[10, 1] = np.nan
        mle[11, :] = np.nan
        dfit[12] = np.nan
        dfit[20::17] = np.nan
        bm[13] = 1e-320                                        # 1 / baseMean = Inf: the weight is 0
        bm[14] = 0.0
        az[15::13] = True
        mle[15::13] = np.nan
        if not expanded and p == 3:
            mle[:, 1] = np.where(np.arange(n) % 2 == 0, 11.0, -13.0)       # no row under 10: 1e6
            small = np.zeros(n, bool)
            small[20::17] = True                               # the rows of the NaN dispFit
            mle[:, 2] = np.where(small, 0.5, 10.0 + np.abs(mle[:, 2]))     # the rows under 10 all carry a NaN weight: NaN
    if n == 2 and planted:
        az[1] = True                                           # one live row: the one-gene rule
        mle[1] = np.nan
    return factors, mle, bm, dfit, az, expanded


def _three_ways(engine, factors, mle, bm, dfit, az, expanded):
    import torch
    from deseq2_amd import core, native
    x, names = core.standard_model_matrix(factors)
    view = type("V", (), {"mcols": {"baseMean": bm[~az], "dispFit": dfit[~az]}})()
    with np.errstate(all="ignore"):
        ref, _ = core.estimateBetaPriorVar(view, mle[~az], names, modelMatrixType="expanded" if expanded else "standard",
                                           factors=factors)
    cf = native.coef_factor_codes(factors)
    pcf = native.coef_factor_codes(factors, expanded=True) if expanded else None
    host = native.estimateBetaPriorVarHost(mle, bm, dfit, az, cf, prior_coef_factor=pcf)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    dev = native.estimateBetaPriorVar_dev(t(mle.T), t(bm), t(dfit), t(az.astype(np.int32), torch.int32), cf, prior_coef_factor=pcf)
    via_engine = engine.beta_prior_var(mle, bm, dfit, az, cf, prior_coef_factor=pcf)
    return np.asarray(ref), host, dev, via_engine


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2049, 4097])
def test_prior_var_dev_equals_host_equals_mirror(engine, n, shape):
    """wave edges, the 2048-key sort tile, the one-row rule; every planted value of _prior_case"""
    case = _prior_case(n, shape, 1000 + n, planted=True)
    ref, host, dev, via_engine = _three_ways(engine, *case)
    what = "n=%d %s" % (n, shape)
    assert_same(host, ref, what + ": dsq_beta_prior_var against the mirror")
    assert_same(dev, host, what + ": dsq_beta_prior_var_dev against dsq_beta_prior_var")
    assert_same(via_engine, host, what + ": DeviceEngine.beta_prior_var")
    if n >= 63 and shape == "factor3":
        assert dev[1] == 1e6 and np.isnan(dev[2])
    if n <= 2 and not case[5]:
        assert dev[1] == case[1][0, 1] ** 2                    # a one-gene object: the squared coefficient


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("N", [21, 41, 2001])
def test_prior_var_dev_where_the_floor_hangs_on_the_last_bit(engine, N, shape):
    """N kept rows with (N - 1) 0.95 an integer: order = 1 + (sum of the normalised weights - 1) 0.95 sits at an integer up to
    the rounding of the running total, so floor(order) -- which value the quantile is -- needs every add in its place"""
    for seed in range(4):
        case = _prior_case(N, shape, 7000 + 10 * N + seed, planted=False)
        case[1][:] = np.clip(case[1], -9.5, 9.5)               # every row is kept
        ref, host, dev, via_engine = _three_ways(engine, *case)
        what = "N=%d %s seed %d" % (N, shape, seed)
        assert_same(host, ref, what + ": dsq_beta_prior_var against the mirror")
        assert_same(dev, host, what + ": dsq_beta_prior_var_dev against dsq_beta_prior_var")


def test_prior_var_dev_refuses_a_short_workspace():
    import torch
    from deseq2_amd import _lib as L, native
    factors, mle, bm, dfit, az, _ = _prior_case(65, "factor3_expanded", 5, planted=False)
    cf, pcf = native.coef_factor_codes(factors), native.coef_factor_codes(factors, expanded=True)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    d = [t(mle.T), t(bm), t(dfit), t(az.astype(np.int32), torch.int32)]
    out = np.zeros(pcf.size)
    a = L.DsqBetaPriorArgs(n=65, p=3, mle_beta=d[0].data_ptr(), baseMean=d[1].data_ptr(), dispFit=d[2].data_ptr(),
                           allZero=d[3].data_ptr(), coef_factor=cf.ctypes.data, expanded=1, p_prior=int(pcf.size),
                           prior_coef_factor=pcf.ctypes.data, prior_coef_src=None, upperQuantile=0.05)
    columns = L.lib().dsq_beta_prior_var_columns(C.byref(a))
    assert columns == 3 + 1                                    # the design columns and the pair of the two level columns
    need = int(L.lib().dsq_beta_prior_var_workspace_bytes(65, columns))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().dsq_beta_prior_var_dev(C.byref(a), out.ctypes.data_as(C.c_void_p), C.c_void_p(ws.data_ptr()), need - 1, st)
    assert rc == 1 and "workspace" in L.lib().dsq_last_error().decode()
    L.check(L.lib().dsq_beta_prior_var_dev(C.byref(a), out.ctypes.data_as(C.c_void_p), C.c_void_p(ws.data_ptr()), need, st))
    assert_same(out, native.estimateBetaPriorVarHost(mle, bm, dfit, az, cf, prior_coef_factor=pcf), "the exact workspace")


# ---- 2. core.lfcShrink: the device engine against the host engine --------------------------------------------------------------
def _analysis(which):
    from deseq2_amd import core, simulate
    kw, calls = {}, []
    rng = np.random.default_rng(3)
    if which == "two_groups":                                  # p = 2: the cell kernel
        f = OrderedDict(condition=np.repeat([0, 1], 4))
        x, _ = core.standard_model_matrix(f)
        k = _counts(400, x, 11)
        calls = [dict(coef=1), dict(contrast=("condition", 1, 0))]
    elif which in ("factor3", "weights", "normfactors"):       # a three-level factor: the expanded matrix
        f = OrderedDict(condition=np.repeat([0, 1, 2], 4))
        x, _ = core.standard_model_matrix(f)
        k = _counts(300, x, 17)
        k[7, f["condition"] != 0] = 0                          # zeros in the contrasted groups
        k[7, f["condition"] == 0] = [30, 41, 28, 35]
        num = np.array([0.0, 0.0, -1.0, 1.0])                  # over Intercept, condition0, condition1, condition2
        calls = [dict(coef=2), dict(coef=1, lfcThreshold=1), dict(contrast=("condition", 2, 1)),
                 dict(contrast=("condition", 2, 1), lfcThreshold=1), dict(contrast=num, res="coef2"),
                 dict(contrast=[["condition2"], ["condition0", "condition1"]], res="coef2")]
        if which == "weights":
            w = rng.uniform(0.2, 1.0, k.shape)
            w[rng.uniform(size=k.shape) < 0.1] = 0.05
            kw["weights"] = w
            calls = calls[:4]
        if which == "normfactors":
            nf = np.exp(rng.normal(0, 0.3, k.shape))
            kw["normalizationFactors"] = nf / np.exp(np.mean(np.log(nf), axis=1, keepdims=True))
            calls = calls[:3]
    elif which == "continuous":                                # one continuous covariate, p = 3: the general kernel
        f = None
        m = 10
        x = np.column_stack([np.ones(m), np.repeat([0.0, 1.0], 5), rng.normal(0, 0.5, m)])
        k = _counts(200, x, 29)
        calls = [dict(coef=1), dict(coef=2, lfcThreshold=1)]
    elif which == "paired12":                                  # ~ patient + treatment, p = 12, m = 22: the rolled kernel
        f = OrderedDict(patient=np.tile(np.arange(11), 2), treatment=np.repeat([0, 1], 11))
        x, _ = core.standard_model_matrix(f)
        k = _counts(120, x, 31)
        calls = [dict(coef=11), dict(contrast=("treatment", 1, 0))]
    else:
        assert which == "spiked"
        f, x, k = _spiked()
        calls = [dict(coef=1), dict(coef=1, lfcThreshold=1), dict(contrast=("condition", 1, 0))]
    return f, x, k, kw, calls


def _shrink_both(dev, host, calls, what):
    import torch
    from deseq2_amd import core
    for call in calls:
        call = dict(call)
        rd = rh = None
        if call.get("res") == "coef2":
            call.pop("res")
            rd, rh = core.results(dev, name=2), core.results(host, name=2)
        a = core.lfcShrink(dev, res=rd, quiet=True, **call)
        b = core.lfcShrink(host, res=rh, quiet=True, **call)
        for c in COLS:
            assert_same(a[c], b[c], "%s %r %s" % (what, call, c))
        assert_same(a.priorInfo["betaPriorVar"], b.priorInfo["betaPriorVar"], "%s %r betaPriorVar" % (what, call))
        assert a.metadata["lfcThreshold"] == b.metadata["lfcThreshold"] == call.get("lfcThreshold", 0)
        if "contrast" in call and not call.get("lfcThreshold"):
            # the lean route against the full one, on the device as well
            full = core.lfcShrink(dev, res=rd, quiet=True, **dict(call, lfcThreshold=1))
            for c in ("log2FoldChange", "lfcSE"):
                assert_same(a[c], full[c], "%s %r lean against full %s" % (what, call, c))


@pytest.mark.parametrize("which", ["two_groups", "factor3", "continuous", "paired12", "weights", "normfactors", "spiked"])
def test_lfcshrink_device_equals_host(oracle, engine, which):
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    f, x, k, kw, calls = _analysis(which)
    dkw = {} if f is None else dict(factors=f)
    host = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle), **kw), **dkw)
    dev = core.DESeq(core.DESeqDataSet(k, x, engine=engine, **kw), **dkw)
    keys = sorted(dev.mcols)
    _shrink_both(dev, host, calls, which)
    assert sorted(dev.mcols) == keys
    if which == "spiked":
        assert np.nansum(np.asarray(host.mcols["replace"], np.float64)) > 0 and host.mcols["allZero"][5]
        r = core.lfcShrink(dev, coef=1, quiet=True)
        assert r["log2FoldChange"][5] == 0 and r["lfcSE"][5] == 0           # the nowZero fill


def test_lfcshrink_on_a_fused_analysis(oracle, engine):
    """an analysis made by fused.DESeq (resident, one launch chain) against the call-by-call one on the host"""
    from deseq2_amd import core, fused
    from deseq2_amd.engine import HostEngine
    f, x, k, kw, calls = _analysis("factor3")
    host = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f)
    dev = fused.DESeq(core.DESeqDataSet(k, x, engine=engine))
    if dev.attrs.get("factors") is None:
        dev.attrs["factors"] = f                 # (the fused chain records the factors of a beta-prior analysis only)
    _shrink_both(dev, host, calls[:4], "fused")
