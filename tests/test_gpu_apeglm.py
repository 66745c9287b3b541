"""apeglm shrinkage on the device (csrc/apeglm.hip) against the numpy specification of tests/apeglm_spec.py, BIT FOR BIT (map,
sd, fsr, thresh, iter, conv, start, objective): dexp / dlog / dlog1p equal the oracle's, sqrt and the four operations are
IEEE, every sum over the samples has the order the specification states.  dsq_apeglm_dev through ctypes on the smallest
shapes at which the kernel can go wrong (tests/apeglm_cases.py), then the host entry (native.apeglm), and
core.lfcShrinkApeglm / core.apeglm on a DeviceEngine against the same call on HostEngine(oracle)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from tests import apeglm_cases as AC
from tests import apeglm_spec as S
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in AC.gpu_cases()}
GUARD = 16
_WANT = {}


def _want(oracle, c):
    """the specification's outputs of a case, computed once"""
    if c["name"] not in _WANT:
        _WANT[c["name"]] = S.fit(oracle, c["Y"], c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], weights=c["weights"],
                                 init=c["init"], threshold=c["threshold"], maxit=c["maxit"])
    return _WANT[c["name"]]


def _gene_major(a, ld, fill, dtype):
    buf = np.full((a.shape[0], ld), fill, dtype=dtype)
    buf[:, :a.shape[1]] = a
    return buf


def _dev(c, p_claim=None, check=True):
    """dsq_apeglm_dev through ctypes: matrices gene-major with ld = round8(m) + pad, the padding filled with NaN (counts that
    are int32: with a negative number), or in R layout; every output prefilled with garbage and followed by a guard"""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    reps = 1 if c["tile"] is None else -(-c["tile"] // c["Y"].shape[0])
    tile = lambda a: None if a is None else (np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:c["tile"]] if reps > 1 else a)
    Y, disp, w, init = tile(c["Y"]), tile(c["disp"]), tile(c["weights"]), tile(c["init"])
    n, m = Y.shape
    p = c["x"].shape[1]
    nf = np.asarray(c["nf"], np.float64)
    vec = nf.ndim == 1
    nf = nf if vec else tile(nf)
    ld = ((m + 7) & ~7) + c["pad"]
    ydt = np.float64 if c["y_f64"] else np.int32
    if c["layout_r"]:
        up = lambda a, fill, dt: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt).T), device=dev)
    else:
        up = lambda a, fill, dt: torch.as_tensor(_gene_major(np.asarray(a, dt), ld, fill, dt), device=dev)
    yt = up(Y, np.nan if c["y_f64"] else -7, ydt)
    nft = torch.as_tensor(nf, device=dev) if vec else up(nf, np.nan, np.float64)
    wt = None if w is None else up(w, np.nan, np.float64)
    xt = torch.as_tensor(np.ascontiguousarray(c["x"].T), device=dev)
    dt = torch.as_tensor(np.ascontiguousarray(disp, np.float64), device=dev)
    it = None if init is None else torch.as_tensor(np.ascontiguousarray(init, np.float64), device=dev)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    sizes = {"map": n * p, "sd": n * p, "fsr": n, "thresh": n, "iter": 2 * n, "conv": n, "start": n, "objective": n}
    outs = {k: torch.full((v + GUARD,), -777.25, dtype=torch.float64, device=dev) for k, v in sizes.items()}
    mask = sum(int(b) << k for k, b in enumerate(c["no_shrink"]))
    ptr = lambda t: None if t is None else t.data_ptr()
    a = L.DsqApeglmArgs(n=n, m=m, p=p if p_claim is None else p_claim, layout=L.DSQ_LAYOUT_R if c["layout_r"] else L.DSQ_LAYOUT_GENE_MAJOR,
                        ld=ld, y=ptr(yt), y_type=L.DSQ_Y_FLOAT64 if c["y_f64"] else L.DSQ_Y_INT32, nf=ptr(nft), nf_is_vector=int(vec),
                        x=ptr(xt), weights=ptr(wt), disp=ptr(dt), init=ptr(it), coef=c["coef"], no_shrink=mask, prior_scale=c["S"],
                        prior_df=1.0, no_shrink_scale=15.0, has_threshold=int(c["threshold"] is not None),
                        threshold=0.0 if c["threshold"] is None else c["threshold"], tol=1e-8, maxit=c["maxit"])
    o = L.DsqApeglmOut(bad=ptr(bad), **{k: ptr(v) for k, v in outs.items()})
    st = torch.cuda.Stream() if c["stream"] else torch.cuda.current_stream()
    torch.cuda.synchronize()
    rc = L.lib().dsq_apeglm_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream))
    st.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    if not check:
        return rc, host
    L.check(rc)
    assert int(bad.cpu()[0]) == 0
    for k, v in sizes.items():
        assert (host[k][v:] == -777.25).all(), "written beyond " + k
    if not c["layout_r"]:
        after = yt.cpu().numpy()
        assert (np.isnan(after[:, m:]).all() if c["y_f64"] else (after[:, m:] == -7).all())          # the padding is as it was
    shape = {"map": (n, p), "sd": (n, p), "iter": (n, 2)}
    return {k: host[k][:v].reshape(shape.get(k, (n,))) for k, v in sizes.items()}, reps


def _same(got, want, what, reps=1):
    for key in AC.SPEC_KEYS:
        w = want[key]
        if reps > 1:
            w = np.tile(w, (reps,) + (1,) * (w.ndim - 1))[:got[key].shape[0]]
        assert_same(got[key], w, "%s: %s" % (what, key))


@pytest.mark.parametrize("name", list(CASES))
def test_device_entry_equals_the_specification(oracle, name):
    c = CASES[name]
    if c["tile"] is not None:
        import torch
        c = dict(c, tile=8 * torch.cuda.get_device_properties(0).multi_processor_count * AC.WAVES + 5)      # past one grid round
    got, reps = _dev(c)
    _same(got, _want(oracle, c), name, reps)


def test_the_cases_hold_what_they_are_for(oracle):
    """rows won by either start, rows that are not fitted, the design on both sides of its LDS bound"""
    from deseq2_amd import _lib as L
    assert int(L.lib().dsq_apeglm_lds_doubles()) == AC.LDS_DOUBLES
    starts = np.concatenate([_want(oracle, CASES[k])["start"] for k in ("p2", "p5", "small_scale")])
    assert (starts == 0).sum() > 0 and (starts == 1).sum() > 0
    w = _want(oracle, CASES["p4"])
    assert np.isnan(w["conv"][[0, 1, 6, 7]]).all() and np.isnan(w["map"][[0, 1, 6, 7]]).all() and (w["conv"][2:6] == 0).all()


def test_p17_is_refused_before_any_launch():
    from deseq2_amd import _lib as L
    rc, host = _dev(CASES["p16"], p_claim=17, check=False)
    assert rc == L.DSQ_ERR_UNSUPPORTED
    assert all((v == -777.25).all() for v in host.values())


def test_host_entry_equals_the_specification(oracle):
    from deseq2_amd import native
    for name in ("m65", "p9", "f64_counts", "no_init", "no_shrink_01"):
        c = CASES[name]
        Y = c["Y"].astype(np.float64) if c["y_f64"] else c["Y"]
        got = native.apeglm(Y, c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], weights=c["weights"], init=c["init"],
                            threshold=c["threshold"], maxit=c["maxit"])
        _same(got, _want(oracle, c), "native.apeglm " + name)


def test_host_entry_refuses_a_bad_count_matrix():
    from deseq2_amd import native, _lib as L
    c = CASES["n5"]
    Y = c["Y"].astype(np.float64)
    Y[1, 2] = 2.5
    with pytest.raises(L.DsqError) as e:
        native.apeglm(Y, c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"])
    assert e.value.code == L.DSQ_ERR_VALUE


def _analysis(engine, weights=None, from_device=False):
    from deseq2_amd import core
    from tests.lfcshrink_cases import counts
    f = OrderedDict(condition=np.repeat([0, 1], 6))
    x, _ = core.standard_model_matrix(f)
    k = counts(200, x, 5)
    sf = np.exp(np.random.default_rng(3).normal(0.0, 0.2, 12))
    if from_device:
        import torch
        dev = engine.device
        dds = core.DESeqDataSet.from_device(engine, torch.as_tensor(np.ascontiguousarray(k.T.astype(np.int32)), device=dev),
                                            torch.as_tensor(np.ascontiguousarray(np.broadcast_to(sf, k.shape).T), device=dev), x,
                                            sizeFactors=sf)
    else:
        dds = core.DESeqDataSet(k, x, sizeFactors=sf, weights=weights, engine=engine)
    return core.DESeq(dds, factors=f, minReplicatesForReplace=np.inf)


@pytest.mark.parametrize("how", ["plain", "weights", "from_device"])
def test_lfcShrinkApeglm_on_the_device_engine_equals_the_host_engine(oracle, how):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    w = np.round(np.random.default_rng(4).uniform(0.3, 1.0, (200, 12)), 2) if how == "weights" else None
    dev = _analysis(DeviceEngine(), w, from_device=how == "from_device")
    host = _analysis(HostEngine(oracle), w)
    for kw in (dict(), dict(lfcThreshold=1.0), dict(svalue=True, apeAdapt=False)):
        (rd, fd), (rh, fh) = (core.lfcShrinkApeglm(d, coef=1, returnList=True, quiet=True, **kw) for d in (dev, host))
        assert rd.columns == rh.columns and rd.priorInfo == rh.priorInfo
        for col in rd.columns:
            assert_same(np.asarray(rd[col], np.float64), np.asarray(rh[col], np.float64), "%s %s: %s" % (how, kw, col))
        for key in ("map", "sd", "fsr", "svalue", "interval"):
            assert_same(fd[key], fh[key], "%s %s: fit$%s" % (how, kw, key))
        for key in ("iter", "conv", "start", "objective"):
            assert_same(fd["diag"][key], fh["diag"][key], "%s %s: fit$diag$%s" % (how, kw, key))


def test_core_apeglm_on_the_device_engine_equals_the_specification(oracle):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine
    c = CASES["p3"]
    nf = np.asarray(c["nf"], np.float64)
    want = _want(oracle, c)
    got = core.apeglm(c["Y"], c["x"], c["disp"], c["coef"], threshold=c["threshold"], weights=c["weights"], init=c["init"],
                      offset=S._log(oracle, nf), prior_control={"prior_scale": c["S"]}, engine=DeviceEngine())
    # (exp(log(nf)) is not nf to the bit: the offsets of this call are the rounded logarithms, so hold the fields that do not
    # depend on that to the specification run on exp(offset))
    from tests.sf_spec import _exp
    want = S.fit(oracle, c["Y"], c["x"], _exp(oracle, S._log(oracle, nf)), c["disp"], c["coef"], c["no_shrink"], c["S"],
                 weights=c["weights"], init=c["init"], threshold=c["threshold"])
    for key in ("map", "sd", "fsr", "thresh"):
        assert_same(got[key], want[key], "core.apeglm: " + key)
    assert_same(got["svalue"], S.svalue(want["fsr"]), "core.apeglm: svalue")
    assert_same(got["interval"], S.interval(want["map"][:, c["coef"]], want["sd"][:, c["coef"]]), "core.apeglm: interval")
