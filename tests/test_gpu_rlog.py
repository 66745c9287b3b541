"""The rlog fit on the device (csrc/rlog.hip) against the numpy specification of tests/rlog_spec.py, BIT FOR BIT: dexp / dlog
/ dnbinom_mu_log equal the oracle's, the four operations and max are IEEE, the sums are wave-order sums.  Then the host
entry against the device entry, core.rlog on the DeviceEngine against the same call on HostEngine(oracle), and sample
counts the dense fit cannot take."""
import ctypes as C

import numpy as np
import pytest

from tests import rlog_spec
from tests.helpers import assert_same
from tests.rlog_cases import inputs, compare

pytestmark = pytest.mark.gpu


def _dev(k, nf, disp, bpv, intercept=None, layout="gm", pad=0, f64=False, stream=None, tol=1e-4, maxit=100, minmu=0.5):
    """dsq_rlog_dev through ctypes on tensors laid out as asked: gene-major with ld = round8(m) + pad (padding filled with
    garbage, in the output too) or R layout; int32 or float64 counts; nf the m size factors or a matrix.  Returns the
    host results, the whole output buffer and the bad-count word."""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    k = np.asarray(k)
    n, m = k.shape

    def place(a, dtype, garbage):
        if layout == "r":
            return torch.as_tensor(np.ascontiguousarray(a.T.astype(dtype)).reshape(-1), device=dev), 0
        ld = ((m + 7) & ~7) + pad
        buf = np.full((n, ld), garbage, dtype=dtype)
        buf[:, :m] = a
        return torch.as_tensor(buf.reshape(-1), device=dev), ld
    yt, ld = place(k, np.float64 if f64 else np.int32, 12345)
    vec = np.ndim(nf) == 1
    nft = torch.as_tensor(np.asarray(nf, np.float64), device=dev) if vec else place(np.asarray(nf, np.float64), np.float64, np.nan)[0]
    out = torch.full((n * (ld if layout != "r" else m),), -777.0, dtype=torch.float64, device=dev)
    dt = torch.as_tensor(np.asarray(disp, np.float64), device=dev)
    it = None if intercept is None else torch.as_tensor(np.asarray(intercept, np.float64), device=dev)
    oi = torch.full((n,), -5.0, dtype=torch.float64, device=dev)
    oit = torch.full((n,), -5.0, dtype=torch.float64, device=dev)
    flag = torch.full((n,), -5, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    a = L.DsqRlogArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R if layout == "r" else L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=yt.data_ptr(),
                      y_type=L.DSQ_Y_FLOAT64 if f64 else L.DSQ_Y_INT32, nf=nft.data_ptr(), nf_is_vector=int(vec),
                      dispFit=dt.data_ptr(), betaPriorVar=float(bpv), intercept=None if it is None else it.data_ptr(),
                      tol=tol, minmu=minmu, maxit=maxit)
    o = L.DsqRlogOut(rlog=out.data_ptr(), intercept=oi.data_ptr() if it is None else None, iter=oit.data_ptr(),
                     flag=flag.data_ptr(), bad=bad.data_ptr())
    if stream is None:
        L.check(L.lib().dsq_rlog_dev(C.byref(a), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    else:
        torch.cuda.synchronize()
        L.check(L.lib().dsq_rlog_dev(C.byref(a), C.byref(o), C.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    full = out.cpu().numpy()
    res = full.reshape(m, n).T if layout == "r" else full.reshape(n, ld)[:, :m]
    return {"rlog": res, "intercept": oi.cpu().numpy(), "iter": oit.cpu().numpy(), "flag": flag.cpu().numpy(),
            "full": full.reshape(n, ld) if layout != "r" else None, "bad": int(bad.cpu()[0])}


def _same(got, want, what, formA):
    assert_same(got["rlog"], want["rlog"], what + " rlog")
    assert_same(got["iter"], want["iter"], what + " iter")
    assert_same(got["flag"], want["flag"], what + " flag")
    if formA:
        assert_same(got["intercept"], want["intercept"], what + " intercept")


_SPEC_A = {}


def _case(O, n, m, seed, nf_matrix, special=True):
    """inputs with the rows the issue names, and their form A specification (computed once per shape)"""
    key = (n, m, seed, nf_matrix, special)
    if key not in _SPEC_A:
        d = inputs(n, m, seed, nf_matrix=nf_matrix)
        if special and nf_matrix and n > 12:
            d["nf"] = np.array(d["nf"])
            d["nf"][9] = 1e-5                                  # log of the mean beyond 30: leaves by |beta| > 30
            d["counts"][9] = 10 ** 9 - np.arange(m) % 7
            d["nf"][12, m // 2] = np.nan                       # a non-finite coefficient: flag 2
        _SPEC_A[key] = (d, rlog_spec.rlog_fit(O, d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"]))
    return _SPEC_A[key]


# every row length at which the kernel takes another path: up to 64 kRlogRegs = 256 samples the coefficients sit in
# registers (one, two, ... kRlogRegs per lane: 64 / 65, 129), up to kRlogLdsDoubles = 2048 in LDS, beyond in the output row
SHAPES = [(37, 1), (37, 2), (37, 3), (37, 63), (37, 64), (37, 65), (37, 129), (37, 255), (37, 256), (37, 257),
          (64, 2047), (64, 2048), (64, 2049)]


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_bit_identity(oracle, idx):
    n, m = SHAPES[idx]
    nf_matrix, f64, layout = bool(idx & 1), bool(idx & 2), ("gm", "r")[(idx >> 2) & 1 if m < 2000 else 0]
    d, sa = _case(oracle, n, m, 0, nf_matrix)
    k, nf, disp, bpv = d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"]
    ga = _dev(k, nf, disp, bpv, layout=layout, pad=8 * (idx % 3), f64=f64)
    _same(ga, sa, "A %dx%d" % (n, m), True)
    assert ga["bad"] == 0 and ga["flag"][3] == 1 and ga["intercept"][3] == -np.inf
    if ga["full"] is not None:
        assert (ga["full"][:, m:] == -777.0).all(), "padding written"
    if nf_matrix:
        assert ga["iter"][9] == 100 and ga["flag"][9] == 0 and ga["flag"][12] == 2 and np.isnan(ga["rlog"][12]).all()
    # form B on the other layout / count type: the fitted intercept frozen, a non-finite entry, a finite one on zero counts
    c = np.array(sa["intercept"])
    c[5] = np.inf
    if nf_matrix:
        c[[9, 12]] = 3.0
    k2 = k.copy()
    k2[7] = 0
    sb = rlog_spec.rlog_fit(oracle, k2, nf, disp, bpv, intercept=c)
    gb = _dev(k2, nf, disp, bpv, intercept=c, layout="r" if layout == "gm" and m < 2000 else "gm", pad=8, f64=not f64)
    _same(gb, sb, "B %dx%d" % (n, m), False)
    assert (gb["flag"][[3, 5]] == 1).all() and gb["flag"][7] == 0


@pytest.mark.parametrize("maxit", [0, 2])
def test_maxit(oracle, maxit):
    """maxit = 0: the post-loop block alone (the start values); maxit = 2: genes that end at maxit"""
    d, _ = _case(oracle, 37, 65, 0, True)
    for icpt in (None, np.linspace(-2.0, 9.0, 37)):
        s = rlog_spec.rlog_fit(oracle, d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"], intercept=icpt, maxit=maxit)
        g = _dev(d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"], intercept=icpt, maxit=maxit)
        _same(g, s, "maxit %d" % maxit, icpt is None)
        assert (g["iter"][g["flag"] != 1] == maxit).any()


def test_stream_and_bad_counts(oracle):
    import torch
    d, sa = _case(oracle, 37, 129, 0, False)
    st = torch.cuda.Stream()
    g = _dev(d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"], stream=st)
    _same(g, sa, "side stream", True)
    k = d["counts"].astype(np.float64)
    assert _dev(k, d["nf"], d["dispFit"], d["betaPriorVar"], f64=True)["bad"] == 0
    k[6, 100] += 0.5
    assert _dev(k, d["nf"], d["dispFit"], d["betaPriorVar"], f64=True)["bad"] == 1
    k[6, 100] = -1.0
    assert _dev(k, d["nf"], d["dispFit"], d["betaPriorVar"], f64=True, layout="r")["bad"] == 1


def test_host_entry(oracle):
    from deseq2_amd import native, _lib as L
    for nf_matrix in (False, True):
        d, _ = _case(oracle, 300, 12, 1, nf_matrix, special=False)
        k, nf, disp, bpv = d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"]
        g = _dev(k, nf, disp, bpv)
        h = native.rlog(k, nf, disp, bpv)
        _same(h, g, "dsq_rlog", True)
        c = np.array(g["intercept"])
        hb = native.rlog(k.astype(np.float64), nf, disp, bpv, intercept=c)
        _same(hb, _dev(k, nf, disp, bpv, intercept=c), "dsq_rlog B", False)
        assert hb["intercept"] is None
    kf = k.astype(np.float64)
    kf[10, 2] = 0.25
    with pytest.raises(L.DsqError) as e:
        native.rlog(kf, nf, disp, bpv)
    assert e.value.code == L.DSQ_ERR_VALUE
    for v in (np.nan, 0.0, -1.0):
        bad = disp.copy()
        bad[10] = v
        with pytest.raises(L.DsqError) as e:
            native.rlog(k, nf, bad, bpv)
        assert e.value.code == L.DSQ_ERR_ARG
    bad = disp.copy()
    bad[3] = np.nan                                            # an all-zero row: its dispFit is never read
    _same(native.rlog(k, nf, bad, bpv), g, "NaN dispFit on a zero row", True)
    with pytest.raises(L.DsqError) as e:
        native.rlog(k, nf, disp, -1.0)
    assert e.value.code == L.DSQ_ERR_ARG


@pytest.mark.parametrize("m", [8, 33])
def test_core_rlog_device_against_host(oracle, m):
    """betaPriorVar: equal to a tolerance, not to the bit -- log2(q + 0.5) is dlog / ln2 on the device and libm's log2 on the
    host engine (an ulp apart at most), so the quantile that is matched may differ in its last bits: 32 * 2^-52 on a log
    fold change of order one, twice that on its square."""
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    k = inputs(400, m, seed=5)["counts"]
    dh = core.rlog(k, engine=HostEngine(oracle))
    dd = core.rlog(k, engine=DeviceEngine())
    assert dd.kind == "rlog"
    bh, bd = dh.attrs["betaPriorVar"], dd.attrs["betaPriorVar"]
    print("betaPriorVar host %.17g device %.17g" % (bh, bd))
    assert abs(bh - bd) <= 1e-12 * bh
    compare(dd.assay(), dh.assay(), "core.rlog %d" % m, dd.dds.mcols["rlogIter"], dh.dds.mcols["rlogIter"])
    zero = ~(k != 0).any(axis=1)
    assert (dd.assay()[zero] == 0).all() and (dd.mcols["rlogIntercept"][zero] == -np.inf).all()
    compare(dd.mcols["rlogIntercept"][~zero][:, None], dh.mcols["rlogIntercept"][~zero][:, None], "rlogIntercept %d" % m)
    # the frozen rlog on the device against the specification
    d2 = core.rlog(k, intercept=dd.mcols["rlogIntercept"], betaPriorVar=bd, engine=DeviceEngine())
    disp = np.where(np.isnan(d2.dds.mcols["dispFit"]), 1.0, d2.dds.mcols["dispFit"])
    s = rlog_spec.rlog_fit(oracle, k, d2.dds.sizeFactors, disp, bd, intercept=dd.mcols["rlogIntercept"])
    assert_same(d2.assay(), s["rlog"], "frozen rlog")


@pytest.mark.parametrize("n,m", [(200, 200), (64, 2000)])
def test_beyond_the_dense_limit(oracle, n, m):
    d, sa = _case(oracle, n, m, 2, False, special=False)
    g = _dev(d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"])
    _same(g, sa, "%dx%d" % (n, m), True)
    assert (g["flag"] == 0).sum() >= n - 2 and (g["iter"][g["flag"] == 0] < 100).any()
