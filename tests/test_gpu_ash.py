"""Adaptive shrinkage on the device (csrc/ash.hip) against the numpy specification of tests/ash_spec.py, BIT FOR BIT on every
output -- the seven per-row columns, pi, sd, K, iteration counts, flags, loglik: dexp / dlog equal the oracle's, sqrt and the
four operations are IEEE, every sum has the order the specification states, and the host loop (grid, active-set solver, line
search) runs the same operations in C++.  dsq_ash_dev through ctypes on the smallest shapes at which the kernels can go wrong
(tests/ash_cases.py), every buffer carved from a poisoned arena (tests/poison.py); then the host entry (native.ash), the
device engine and core.lfcShrinkAshr on an analysis made by from_device against the same call on HostEngine(oracle)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from tests import ash_cases as AC
from tests import ash_spec as S
from tests import poison as P
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

CASES = AC.gpu_cases()
PAD = 3                          # rows n .. ld-1 of every column
_WANT = {}


def _want(oracle, name):
    if name not in _WANT:
        c = CASES[name]
        _WANT[name] = S.fit(oracle, c["b"], c["s"], c["threshold"])
    return _WANT[name]


def _call(arena, b, s, threshold, prefill, short=0, check=True, reuse=None):
    """dsq_ash_dev through ctypes on buffers carved from `arena`: inputs (C, n + PAD) with the padding rows holding kept-looking
    values, outputs and the workspace -- exactly its _workspace_bytes -- prefilled with the byte `prefill`, or, with `reuse`,
    the output and workspace buffers of an earlier call as that call left them"""
    import torch
    from deseq2_amd import _lib as L
    n, cols = b.shape
    ld = n + PAD
    pad = lambda a: np.concatenate([np.ascontiguousarray(a.T), np.full((cols, PAD), 0.75)], axis=1)
    bt, st_ = arena.put(pad(b), "betahat"), arena.put(pad(s), "sebetahat")
    need = int(L.lib().dsq_ash_workspace_bytes(n, cols))
    if reuse is None:
        byte = P.BYTE[prefill]
        outs = OrderedDict((k, arena.empty((cols, ld), torch.float64, byte, k)) for k in S.ROWS)
        outs["pi"] = arena.empty((cols, L.DSQ_ASH_MAX_K), torch.float64, byte, "pi")
        outs["sd"] = arena.empty((cols, L.DSQ_ASH_MAX_K), torch.float64, byte, "sd")
        for k in ("K", "iter", "flag"):
            outs[k] = arena.empty((cols,), torch.int32, byte, k)
        outs["loglik"] = arena.empty((cols,), torch.float64, byte, "loglik")
        ws = arena.carve(need, byte, "workspace")
        for k in S.ROWS:
            arena.holds(outs[k][:, n:], byte, "padding rows of " + k)
    else:
        outs, ws = reuse
    a = L.DsqAshArgs(n=n, C=cols, ld=ld, betahat=bt.data_ptr(), sebetahat=st_.data_ptr(), has_threshold=int(threshold is not None),
                     threshold=0.0 if threshold is None else threshold, maxit=100)
    o = L.DsqAshOut(**{k: v.data_ptr() for k, v in outs.items()})
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()
    rc = L.lib().dsq_ash_dev(C.byref(a), C.byref(o), C.c_void_p(ws.data_ptr()), need - short, C.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    if check:
        L.check(rc)
        arena.check()
    return rc, {k: (v[:, :n] if k in S.ROWS else v) for k, v in host.items()}, host, (outs, ws)


def _arena(n, cols):
    from deseq2_amd import _lib as L
    need = int(L.lib().dsq_ash_workspace_bytes(n, cols))
    return P.Arena.on_device(2 * (need + 24 * (n + PAD) * cols * 8) + 40 * (P.MARGIN + P.ALIGN) + (1 << 20))


@pytest.mark.parametrize("name", list(CASES))
def test_device_entry_equals_the_specification(oracle, name):
    c = CASES[name]
    prefill = (P.FF, P.ZERO, P.LEFT)[list(CASES).index(name) % 3]
    n, cols = c["b"].shape
    arena = _arena(n, cols)
    if prefill == P.LEFT:          # the buffers as another fit of the same shape on other data left them
        r = np.random.default_rng(1)
        ob, os_ = np.column_stack([AC.column(n, 900 + j)[0] for j in range(cols)]), r.uniform(0.1, 1.0, (n, cols))
        left = _call(arena, ob, os_, c["threshold"], P.ZERO)[3]
        got = _call(arena, c["b"], c["s"], c["threshold"], P.ZERO, reuse=left)[1]
    else:
        got = _call(arena, c["b"], c["s"], c["threshold"], prefill)[1]
    want = _want(oracle, name)
    for k in S.KEYS:
        assert_same(got[k], want[k], "%s (%s): %s" % (name, prefill, k))


def test_the_cases_hold_what_they_are_for(oracle):
    from deseq2_amd import _lib as L
    assert int(L.lib().dsq_ash_slice_rows()) == AC.SLICE == S.SLICE
    assert _want(oracle, "K7")["K"][0] == 7 and _want(oracle, "K64")["K"][0] == 64 and _want(oracle, "n64")["K"][0] == 17
    w = _want(oracle, "C3")
    assert len(set(w["K"])) > 1 and w["iter"].max() - w["iter"].min() >= 3 and (w["flag"] == 0).all()
    e = _want(oracle, "excluded")
    bad = [0, 63, 64, AC.SLICE - 1, AC.SLICE, 2 * AC.SLICE - 1, 2 * AC.SLICE, 2 * AC.SLICE + 8]
    assert np.isnan(e["PosteriorMean"][0, bad]).all() and np.isnan(e["PosteriorMean"][0]).sum() == len(bad)
    assert np.isnan(_want(oracle, "n63")["le_T"]).all() and not np.isnan(_want(oracle, "n64")["le_T"]).any()


def test_refusals_leave_the_outputs_alone():
    from deseq2_amd import _lib as L
    b, s = AC.wide_column(70, 7, top=170.0)                       # K = 65
    rc, _, host, _ = _call(_arena(70, 1), b[:, None], s[:, None], None, P.FF, check=False)
    assert rc == L.DSQ_ERR_UNSUPPORTED
    assert all((v.view(np.uint8) == 0xFF).all() for v in host.values())
    b, s = AC.column(40, 1)
    rc, _, host, _ = _call(_arena(40, 1), b[:, None], np.full((40, 1), np.nan), None, P.FF, check=False)      # no kept row
    assert rc == L.DSQ_ERR_VALUE and all((v.view(np.uint8) == 0xFF).all() for v in host.values())
    rc, _, host, _ = _call(_arena(40, 1), b[:, None], s[:, None], None, P.FF, short=8, check=False)           # a short workspace
    assert rc == L.DSQ_ERR_ARG and all((v.view(np.uint8) == 0xFF).all() for v in host.values())


def test_host_entry_equals_the_specification(oracle):
    from deseq2_amd import native
    for name in ("n65", "K7", "C3_T", "excluded"):
        c = CASES[name]
        got, want = native.ash(c["b"], c["s"], threshold=c["threshold"]), _want(oracle, name)
        for k in S.KEYS:
            assert_same(got[k].T if k in S.ROWS else got[k], want[k], "native.ash %s: %s" % (name, k))


def test_device_engine_equals_the_specification(oracle):
    from deseq2_amd.engine import DeviceEngine
    c, want = CASES["C3_T"], _want(oracle, "C3_T")
    got = DeviceEngine().ash_fit(c["b"], c["s"], threshold=c["threshold"])
    for k in S.KEYS:
        v = got[k].cpu().numpy() if k in S.ROWS else got[k]
        assert_same(v, want[k], "DeviceEngine.ash_fit: " + k)


def _analysis(engine, from_device):
    from deseq2_amd import core
    from tests.lfcshrink_cases import counts
    f = OrderedDict(condition=np.repeat([0, 1, 2], 4))
    x, _ = core.standard_model_matrix(f)
    k = counts(200, x, 5)
    k[[3, 77]] = 0                                               # all-zero genes: NA rows
    sf = np.exp(np.random.default_rng(3).normal(0.0, 0.2, 12))
    if from_device:
        import torch
        dev = engine.device
        dds = core.DESeqDataSet.from_device(engine, torch.as_tensor(np.ascontiguousarray(k.T.astype(np.int32)), device=dev),
                                            torch.as_tensor(np.ascontiguousarray(np.broadcast_to(sf, k.shape).T), device=dev), x,
                                            sizeFactors=sf)
    else:
        dds = core.DESeqDataSet(k, x, sizeFactors=sf, engine=engine)
    return core.DESeq(dds, factors=f, minReplicatesForReplace=np.inf)


def test_lfcShrinkAshr_on_the_device_engine_equals_the_host_engine(oracle):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    dev, host = _analysis(DeviceEngine(), True), _analysis(HostEngine(oracle), False)
    calls = (dict(coef=1), dict(coef=2, lfcThreshold=1.0), dict(contrast=("condition", 2, 1), svalue=True),
             dict(contrast=[("condition", 2, 1), ("condition", 1, 0), [0.0, 1.0, 1.0]]))
    for kw in calls:
        rd, rh = (core.lfcShrinkAshr(d, returnList=True, quiet=True, **kw) for d in (dev, host))
        if not isinstance(rd, list):
            rd, rh = [rd], [rh]
        assert len(rd) == len(rh)
        for (d, fd), (h, fh) in zip(rd, rh):
            assert d.columns == h.columns
            if "lfcSE" not in d._set:
                import torch
                assert torch.is_tensor(d.tab.resident["lfcSE"])                  # (a handle until it is asked for)
            for col in d.columns:
                assert_same(np.asarray(d[col], np.float64), np.asarray(h[col], np.float64), "%s: %s" % (kw, col))
            assert np.isnan(np.asarray(d["log2FoldChange"])[[3, 77]]).all()
            for key in fd["result"]:
                assert_same(fd["result"][key], fh["result"][key], "%s: fit$result$%s" % (kw, key))
            for key in ("pi", "sd"):
                assert_same(fd["fitted_g"][key], fh["fitted_g"][key], "%s: fitted_g$%s" % (kw, key))
            assert (fd["loglik"], fd["iter"], fd["flag"]) == (fh["loglik"], fh["iter"], fh["flag"])
