"""unmix() on the device (csrc/unmix.hip) against the numpy specification of tests/unmix_spec.py, BIT FOR BIT (p, loss, iter,
flag): dlog equals the oracle's log, sqrt and the four operations are IEEE, every sum over the genes has the order the
specification states.  dsq_unmix_dev on the smallest shapes at which the kernels can go wrong, then the host entry
(native.unmix), and core.unmix on a DeviceEngine against the same call on HostEngine(oracle)."""
import ctypes as C

import numpy as np
import pytest

from tests import unmix_cases as CS
from tests import unmix_spec as S
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

T = S.T
FORM_POWER = [(f, p) for f in CS.FORMS for p in (1, 2)]


def _inputs(n, k, m, seed):
    """mixtures of k components over n genes with noise, a fifth of pure zero"""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.round(400.0 * rng.uniform(size=(n, k)) ** 2)
    base[rng.uniform(size=(n, k)) < 0.2] = 0.0
    w = rng.dirichlet(np.ones(k), m)
    x = rng.poisson(base @ w.T * 1.5).astype(np.float64)
    return x, base


def _dev(x, pure, pad=0, stream=None, short=0, maxit=200, power=1, **form):
    """dsq_unmix_dev through ctypes: x gene-major with ld = round8(m) + pad, the padding filled with NaN; outputs prefilled
    with garbage.  Returns the host results and the x buffer as it is afterwards."""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    n, m = x.shape
    k = pure.shape[1]
    ld = ((m + 7) & ~7) + pad
    buf = np.full((n, ld), np.nan)
    buf[:, :m] = x
    xt = torch.as_tensor(buf, device=dev)
    pt = torch.as_tensor(np.ascontiguousarray(pure, np.float64), device=dev)
    p = torch.full((m, k), -777.0, dtype=torch.float64, device=dev)
    loss = torch.full((m,), -777.0, dtype=torch.float64, device=dev)
    it = torch.full((m,), -5, dtype=torch.int32, device=dev)
    flag = torch.full((m,), -5, dtype=torch.int32, device=dev)
    need = int(L.lib().dsq_unmix_workspace_bytes(n, m, k))
    assert need == n * m * 8
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    ws[need:] = 171
    a = L.DsqUnmixArgs(n=n, m=m, k=k, ld=ld, x=xt.data_ptr(), pure=pt.data_ptr(), has_alpha=int("alpha" in form),
                       has_shift=int("shift" in form), alpha=form.get("alpha", 0.0), shift=form.get("shift", 0.0), power=power,
                       maxit=maxit)
    o = L.DsqUnmixOut(p=p.data_ptr(), loss=loss.data_ptr(), iter=it.data_ptr(), flag=flag.data_ptr())
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    rc = L.lib().dsq_unmix_dev(C.byref(a), C.byref(o), C.c_void_p(ws.data_ptr()), need - short, C.c_void_p(st.cuda_stream))
    st.synchronize()
    if short:
        return rc
    L.check(rc)
    assert (ws[need:].cpu().numpy() == 171).all()                       # nothing written past the workspace
    return {"p": p.cpu().numpy(), "loss": loss.cpu().numpy(), "iter": it.cpu().numpy(), "flag": flag.cpu().numpy(),
            "x_after": xt.cpu().numpy()}


def _same(got, want, what):
    for key in ("p", "loss", "iter", "flag"):
        assert_same(got[key], want[key], "%s: %s" % (what, key))


@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3])
def test_gene_counts_around_the_block(oracle, n):
    x, pure = _inputs(n, 3, 3, seed=n)
    for form, power in FORM_POWER:
        want = S.unmix_fit(oracle, x, pure, power=power, **CS.FORMS[form])
        _same(_dev(x, pure, power=power, **CS.FORMS[form]), want, "n = %d, %s, power %d" % (n, form, power))


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 9, 16])
def test_component_counts(oracle, k):
    """4 | 5 and 8 | 9: the padded accumulator widths 4, 8, 16; 9 and 16 take the two-sweep layout"""
    x, pure = _inputs(131, k, 3, seed=100 + k)
    for form, power in (("alpha", 2), ("shift", 1)):
        want = S.unmix_fit(oracle, x, pure, power=power, **CS.FORMS[form])
        _same(_dev(x, pure, power=power, **CS.FORMS[form]), want, "k = %d, %s, power %d" % (k, form, power))


def test_one_sample_and_more_samples_than_one_grid_round(oracle):
    import torch
    x, pure = _inputs(70, 3, 1, seed=5)
    _same(_dev(x, pure, power=1, alpha=0.01), S.unmix_fit(oracle, x, pure, power=1, alpha=0.01), "m = 1")
    m = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 37      # the fit grid is capped at two workgroups per CU
    x, pure = _inputs(70, 3, m, seed=6)
    got = _dev(x, pure, power=2, alpha=0.01)
    _same(got, S.unmix_fit(oracle, x, pure, power=2, alpha=0.01), "m = %d" % m)


def test_leading_dimension_and_padding(oracle):
    x, pure = _inputs(97, 4, 5, seed=7)
    want = S.unmix_fit(oracle, x, pure, power=2, shift=0.5)
    got = _dev(x, pure, pad=16, power=2, shift=0.5)
    _same(got, want, "ld = m + padding")
    assert got["x_after"].shape == (97, 24) and np.isnan(got["x_after"][:, 5:]).all()
    assert_same(got["x_after"][:, :5], x, "x is not written")


@pytest.mark.parametrize("name", ["vertices", "zeros", "markers"])
def test_bounds_and_zeros(oracle, name):
    """a sample equal to a pure column (the others end on lo), 150 x a pure column (the upper bound), all-zero rows of pure,
    zero entries of x, an all-zero sample: the device entry, the host entry and native.unmix"""
    from deseq2_amd import native
    x, pure, _ = CS.cases()[name]
    wants = {}
    for form, power in FORM_POWER:
        want = wants[form, power] = S.unmix_fit(oracle, x, pure, power=power, **CS.FORMS[form])
        _same(_dev(x, pure, power=power, **CS.FORMS[form]), want, "%s, %s, power %d: dsq_unmix_dev" % (name, form, power))
        _same(native.unmix(x, pure, power=power, **CS.FORMS[form]), want, "%s, %s, power %d: dsq_unmix" % (name, form, power))
    if name == "vertices":
        assert (wants["shift", 1]["p"][0, 1:] == 0.0).all() and (wants["alpha", 2]["p"][0, 1:] == 1e-6).all()
        assert wants["alpha", 2]["p"][2, 1] == 100.0 and wants["shift", 1]["p"][2, 1] == 100.0


def test_a_sample_with_a_nan(oracle):
    x, pure = _inputs(200, 3, 4, seed=8)
    x[17, 2] = np.nan
    for form, power in FORM_POWER:
        got = _dev(x, pure, power=power, **CS.FORMS[form])
        want = S.unmix_fit(oracle, x, pure, power=power, **CS.FORMS[form])
        _same(got, want, "NaN sample, %s, power %d" % (form, power))
        assert got["flag"][2] == 2 and np.isnan(got["p"][2]).all() and np.isnan(got["loss"][2]) and got["iter"][2] == 0
        assert (got["flag"][[0, 1, 3]] != 2).all() and np.isfinite(got["p"][[0, 1, 3]]).all()


def test_a_second_stream_and_maxit(oracle):
    import torch
    x, pure = _inputs(150, 5, 6, seed=9)
    want = S.unmix_fit(oracle, x, pure, power=1, alpha=0.01)
    _same(_dev(x, pure, power=1, alpha=0.01, stream=torch.cuda.Stream()), want, "side stream")
    for maxit in (0, 3):
        _same(_dev(x, pure, power=1, alpha=0.01, maxit=maxit), S.unmix_fit(oracle, x, pure, power=1, alpha=0.01, maxit=maxit),
              "maxit = %d" % maxit)


def test_a_workspace_one_byte_short_is_refused():
    from deseq2_amd import _lib as L
    x, pure = _inputs(65, 3, 2, seed=10)
    assert _dev(x, pure, short=1, alpha=0.01) == 1 and "workspace" in L.lib().dsq_last_error().decode()


def test_host_entry_refuses_bad_values():
    from deseq2_amd import native
    x, pure = _inputs(65, 3, 2, seed=11)
    x[3, 1] = -1.0
    with pytest.raises(Exception, match="x holds"):
        native.unmix(x, pure, alpha=0.01)


def test_core_unmix_on_the_device_engine(oracle):
    """the resident normalized counts of a small analysis go into core.unmix as the handle normalized_counts() returns"""
    from deseq2_amd import core, simulate
    from deseq2_amd.engine import DeviceEngine, HostEngine
    x = simulate.design_two_group(12)
    k = simulate.make_counts(300, x, seed=21)["counts"]
    rng = np.random.Generator(np.random.PCG64(22))
    res = {}
    for label, E in (("host", HostEngine(oracle)), ("device", DeviceEngine())):
        dds = core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=E))
        nc = core.normalized_counts(dds)
        if label == "host":
            q = nc.assay()
            pure = core._named(np.column_stack([q[:, :6].mean(axis=1), q[:, 6:].mean(axis=1), rng.gamma(2.0, 40.0, q.shape[0])]),
                               None, ["A", "B", "other"])
        res[label] = (core.unmix(nc, pure, alpha=0.05, power=2), core.unmix(nc, pure, shift=1.0, format="list"))
    for a, b in zip(res["host"], res["device"]):
        ma, mb = (a["mix"], b["mix"]) if isinstance(a, dict) else (a, b)
        assert ma.shape == (12, 3) and mb.colnames == ["A", "B", "other"]
        # (the two engines' size factors agree to rounding, not to the bit: so do the normalized counts that go in)
        np.testing.assert_allclose(np.asarray(mb), np.asarray(ma), rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["device"][1]["cor"], res["host"][1]["cor"], atol=1e-8)
    # on the SAME matrix the two engines agree to the bit
    xm = np.asarray(core.normalized_counts(core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=HostEngine(oracle)))).assay())
    for kw in (dict(alpha=0.05, power=1), dict(shift=1.0, power=2)):
        assert_same(np.asarray(core.unmix(xm, pure, engine=DeviceEngine(), **kw)),
                    np.asarray(core.unmix(xm, pure, engine=HostEngine(oracle), **kw)), "core.unmix, %r" % (kw,))
