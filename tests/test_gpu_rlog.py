"""The rlog fit on the device (csrc/rlog.hip) against the numpy specification of tests/rlog_spec.py, BIT FOR BIT: dexp / dlog
/ dnbinom_mu_log equal the oracle's, the four operations and max are IEEE, the sums are wave-order sums.  Then the host
entry against the device entry, core.rlog on the DeviceEngine against the same call on HostEngine(oracle), and sample
counts the dense fit cannot take."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import rlog_spec
from tests.helpers import assert_same
from tests.rlog_cases import inputs, compare, lapack_case, mutants, TIE_CAP

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


# ---- past one grid round ----------------------------------------------------------------------------------------------------
LAUNCH_LINE = re.compile(r"\[dsq\] rlog n=(\d+) m=(\d+) form ([AB]): mode (\d), blocks (\d+), threads 256")
BASE = 19             # distinct ordinary rows of the tiled inputs (no divisor of a round: a slot's second row is another one)


def _dev_line(monkeypatch, capfd, *a, **kw):
    """_dev under DSQ_VERBOSE: the result and what launch_rlog (csrc/rlog.hip) printed: form, mode, genes of one grid round"""
    monkeypatch.setenv("DSQ_VERBOSE", "1")
    capfd.readouterr()
    got = _dev(*a, **kw)
    err = capfd.readouterr().err
    monkeypatch.delenv("DSQ_VERBOSE")
    lines = LAUNCH_LINE.findall(err)
    assert len(lines) == 1, "no launch line in %r" % err
    print(err.strip())
    n, m, form, mode, blocks = lines[0]
    return got, dict(n=int(n), m=int(m), form=form, mode=int(mode), round=4 * int(blocks))


def _expand(spec, rep_of):
    return {key: v[rep_of] for key, v in spec.items()}


@pytest.mark.parametrize("m,mode", [(5, 0), (257, 1), (2049, 2)], ids=["m5-registers", "m257-lds", "m2049-output-row"])
def test_gene_loop_past_one_round(oracle, monkeypatch, capfd, m, mode):
    """The persistent loop of rlog_kernel, `i += gridDim.x * 4`, in each storage mode (RLOG_REG / RLOG_LDS / RLOG_ROW), form A
    and then form B on the intercepts form A returned: n = round + 5 rows, launch_rlog's round being 8 workgroups of four
    waves per CU (worked out from the CU count, confirmed by the launch line).  Rows 0 .. 4 and round .. round + 4 share their
    waves.  First trip: rows 0 and 3 all-zero (`continue`), row 1 leaves by |beta| > 30 (`break`), row 2 has a NaN factor (the
    NaN exit), row 4 is ordinary.  Second trip: three ordinary rows behind rows 0, 1, 2, then the |beta| > 30 row behind the
    all-zero row 3 and the NaN row behind row 4.  Form B turns the -Inf / NaN intercepts of these rows into `continue` in both
    trips and adds a planted +Inf at round + 1.  The ordinary rows repeat BASE distinct ones, so the specification
    is evaluated on the ten rows named, the special rows and BASE more, and EVERY row of both trips is compared bit for bit.
    m > 600 has no reference but the specification: a dense QR at m = 2 049 costs about a minute per gene."""
    import torch
    rnd = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 4             # launch_rlog, csrc/rlog.hip
    n = rnd + 5
    assert rnd % BASE != 0
    b = inputs(BASE, m, seed=3, nf_matrix=True, zero_row=False)
    src = np.arange(n) % BASE
    k, nf, disp, bpv = b["counts"][src], np.array(b["nf"][src]), b["dispFit"][src], b["betaPriorVar"]
    zero, large, nan = [0, 3], [1, rnd + 3], [2, rnd + 4]
    k[zero] = 0
    nf[large] = 1e-5                                           # log of the mean beyond 30: leaves by |beta| > 30
    k[large] = 10 ** 9 - np.arange(m) % 7
    nf[nan, m // 2] = np.nan                                   # a non-finite coefficient: flag 2
    reps = np.r_[np.arange(5), rnd + np.arange(5), 5 + np.arange(BASE)]              # (5 .. 5 + BASE - 1: every ordinary row once)
    rep_of = 10 + (src - 5) % BASE
    rep_of[reps[:10]] = np.arange(10)
    assert (src[reps[rep_of]] == src).all()

    sa = _expand(rlog_spec.rlog_fit(oracle, k[reps], nf[reps], disp[reps], bpv), rep_of)
    ga, line = _dev_line(monkeypatch, capfd, k, nf, disp, bpv, pad=8)
    assert (line["form"], line["mode"], line["round"]) == ("A", mode, rnd) and line["round"] < n
    _same(ga, sa, "A %dx%d" % (n, m), True)
    assert (ga["flag"][zero] == 1).all() and (ga["iter"][large] == 100).all() and (ga["flag"][large] == 0).all()
    assert (ga["flag"][nan] == 2).all() and (ga["flag"][rnd:rnd + 3] == 0).all() and ga["flag"][4] == 0
    assert (ga["full"][:, m:] == -777.0).all(), "padding written"

    c = np.array(ga["intercept"])                              # -Inf on the zero rows, NaN on the flag 2 rows
    c[rnd + 1] = np.inf
    c[large] = 3.0
    sb = _expand(rlog_spec.rlog_fit(oracle, k[reps], nf[reps], disp[reps], bpv, intercept=c[reps]), rep_of)
    gb, line = _dev_line(monkeypatch, capfd, k, nf, disp, bpv, intercept=c, f64=True)
    assert (line["form"], line["mode"], line["round"]) == ("B", mode, rnd) and line["round"] < n
    _same(gb, sb, "B %dx%d" % (n, m), False)
    assert (gb["flag"][zero + nan + [rnd + 1]] == 1).all() and (gb["flag"][[rnd, rnd + 2]] == 0).all()


# ---- m >= 64 against the LAPACK restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(65, 100), (257, 24)])
def test_device_against_dense_lapack(oracle, m, n):
    """Beyond 63 samples the dense C oracle has no design wide enough; oracle/lapack_oracle.py's fitBeta on [1 | I_m] / I_m has
    no width limit.  The device against it, forms A and B, with the project's RTOL and TIE_CAP unchanged (the specification
    alone stays at zero ties and under 2e-14 on these inputs: profiles/rlog.md).  m > 600 stays with the bit identity to the
    specification: a dense QR at m = 2 049 costs about a minute per gene."""
    c = lapack_case(oracle, n, m)
    d = c["d"]
    nf, disp, bpv = d["nf"], d["dispFit"], d["betaPriorVar"]
    ga = _dev(d["counts"], nf, disp, bpv)
    rows, v, it = c["lapackA"]
    compare(ga["rlog"][rows], v, "device / LAPACK form A m=%d" % m, ga["iter"][rows], it)
    assert_same(ga["intercept"], c["specA"]["intercept"], "intercept")             # (form B below is on the same intercepts)
    gb = _dev(c["k2"], nf, disp, bpv, intercept=c["c"])
    rows, v, it = c["lapackB"]
    compare(gb["rlog"][rows], v, "device / LAPACK form B m=%d" % m, gb["iter"][rows], it)
    assert (gb["flag"][[3, 5]] == 1).all() and gb["flag"][7] == 0
    if m == 65:
        # the same comparison refuses a device result with one value moved by 3e-11 relative, one iteration count off by one
        rows, v, it = c["lapackA"]
        assert TIE_CAP * rows.size < 1
        for name, (mv, mi) in zip(("value", "iteration count"), mutants(ga["rlog"], ga["iter"], rows)):
            with pytest.raises(AssertionError):
                compare(mv[rows], v, "mutant: " + name, mi[rows], it)
