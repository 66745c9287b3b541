"""The variance stabilizing transformation on the device (csrc/vst.hip) against the numpy specification of
tests/vst_spec.py, BIT FOR BIT: dlog / dlog1p equal the oracle's log / log1p, sqrt and the four operations are IEEE, the
row sums are wave-order sums, the maximum is exact.  Then core.vst / varianceStabilizingTransformation on the DeviceEngine
against the same calls on HostEngine(oracle)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import vst_spec
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu


def _counts(n, m, seed, zeros=0.1, hi=6.0):
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.normal(hi, 2.5, (n, 1)) * np.exp(rng.normal(0, 0.4, m))[None, :]
    k = rng.poisson(mu).astype(np.int64)
    k[rng.uniform(size=k.shape) < zeros] = 0
    if n > 3:
        k[3] = 0                                      # a row of zeros
    return np.minimum(k, 2 ** 31 - 1).astype(np.int32)


def _sf(m, seed):
    return np.exp(np.random.default_rng(seed + 7).normal(0, 0.3, m))


def _trend_a(mu):
    return 0.05 + 2.0 / mu


def _trend_b(mu):
    return 0.3 + 0.5 / np.sqrt(mu) + 4.0 / mu


def _product_table(trend, k, nf):
    """a spline table built by the product's own host code (core.vst_spline_table + the affine rescaling of R/vst.R:175-178)"""
    from deseq2_amd import core
    from deseq2_amd.engine import spline_eval
    q = vst_spec.normalized(k, nf)
    fin = np.where(np.isfinite(q), q, 0.0)
    sfa = nf if np.ndim(nf) == 1 else np.exp(np.log(nf).mean(axis=0))
    table = core.vst_spline_table(trend, float(fin.max()), float(np.mean(1.0 / sfa[np.isfinite(sfa)])))
    rm = fin.mean(axis=1)
    h1, h2 = core.quantile7(rm, .95), core.quantile7(rm, .999)
    s1, s2 = (float(spline_eval(table, np.arcsinh(h))) for h in (h1, h2))
    eta = (np.log2(h2) - np.log2(h1)) / (s2 - s1)
    return table, float(eta), float(np.log2(h1) - eta * s1)


def _hand_table():
    """irregular knots, arbitrary (finite) coefficients: the device evaluates the table it is given"""
    rng = np.random.default_rng(5)
    x = np.cumsum(rng.uniform(0.01, 0.3, 37)) + 0.4      # last knot near 6: asinh(q) passes it from q = 200 on
    return np.vstack([x, rng.normal(0, 3, 37), rng.normal(0, 1, 37), rng.normal(0, .5, 37), rng.normal(0, .2, 37)])


def _kind_params(kind, k, nf, variant=0):
    if kind == "parametric":
        return [dict(asymptDisp=a, extraPois=e) for a, e in ((1e-4, 1e-2), (1e-2, 1e3), (0.1, 1.0), (10.0, 30.0))][variant % 4]
    if kind == "mean":
        return dict(alpha=(1e-4, 0.07, 10.0)[variant % 3])
    if kind == "log2":
        return dict(pc=(1.0, 0.5)[variant % 2])
    if kind == "spline":
        if variant % 3 == 2:
            return dict(table=_hand_table(), eta=1.7, xi=-0.3)
        t, eta, xi = _product_table((_trend_a, _trend_b)[variant % 3], k, nf)
        return dict(table=t, eta=eta, xi=xi)
    return {}


def _dev(k, nf, kind, params, layout="gm", pad=0, f64=False, stats=False, stream=None, misalign=False):
    """dsq_vst_dev / dsq_vst_rowstats_dev through ctypes on tensors laid out as asked: gene-major with
    ld = round8(m) + pad (padding filled with garbage, in the output too) or R layout; int32 or float64 counts; nf the m
    size factors or a matrix.  Returns the host result (n x m), the whole output buffer, and the bad-count flag."""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    k = np.asarray(k)
    n, m = k.shape
    kt = np.float64 if f64 else np.int32
    off = 1 if misalign else 0                     # start the buffers one element into an allocation

    def place(a, dtype, garbage):
        if layout == "r":
            flat = np.concatenate([np.full(off, garbage, dtype), np.ascontiguousarray(a.T.astype(dtype)).reshape(-1)])
            t = torch.as_tensor(flat, device=dev)
            return t, t[off:], 0
        ld = ((m + 7) & ~7) + pad
        buf = np.full((n, ld), garbage, dtype=dtype)
        buf[:, :m] = a
        flat = np.concatenate([np.full(off, garbage, dtype), buf.reshape(-1)])
        t = torch.as_tensor(flat, device=dev)
        return t, t[off:], ld
    _, yt, ld = place(k, kt, 12345)
    vec = np.ndim(nf) == 1
    if vec:
        nft = torch.as_tensor(np.concatenate([np.zeros(off), np.asarray(nf, np.float64)]), device=dev)[off:]
    else:
        _, nft, _ = place(np.asarray(nf, np.float64), np.float64, np.nan)
    nout = n * (ld if layout != "r" else m)
    outall = torch.full((nout + off,), -777.0, dtype=torch.float64, device=dev)
    out = outall[off:]
    rs = torch.full((2, n), -5.0, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = dict(kind=L.DSQ_VST[kind], asymptDisp=0.0, extraPois=0.0, alpha=0.0, pc=0.0, spline=None, nknots=0, eta=0.0, xi=0.0)
    tab = None
    for key, v in params.items():
        if key == "table":
            tab = np.ascontiguousarray(v, dtype=np.float64)
            kw["spline"], kw["nknots"] = tab.ctypes.data_as(C.c_void_p), tab.shape[1]
        else:
            kw[key] = float(v)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = L.DsqVstArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R if layout == "r" else L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=p(yt),
                     y_type=L.DSQ_Y_FLOAT64 if f64 else L.DSQ_Y_INT32, nf=p(nft), nf_is_vector=int(vec), **kw)
    o = L.DsqVstOut(out=p(out), rowMean=p(rs[0]), rowMax=p(rs[1]), bad=p(bad))
    s = torch.cuda.current_stream() if stream is None else stream
    fn = L.lib().dsq_vst_rowstats_dev if stats else L.lib().dsq_vst_dev
    with torch.cuda.stream(s):
        rc = fn(C.byref(a), C.byref(o), C.c_void_p(s.cuda_stream))
    torch.cuda.synchronize()
    if rc != 0:
        return rc, outall.cpu().numpy(), None
    if stats:
        h = rs.cpu().numpy()
        return (h[0], h[1]), None, int(bad.cpu()[0])
    full = out.cpu().numpy()
    if layout == "r":
        return full.reshape(m, n).T, full, int(bad.cpu()[0])
    full = full.reshape(n, ld)
    return full[:, :m], full, int(bad.cpu()[0])


def _check(O, k, nf, kind, params, what, **kw):
    ref = vst_spec.transform(O, k, nf, kind, **params)
    got, full, bad = _dev(k, nf, kind, params, **kw)
    assert not isinstance(got, int), "%s: error code %r" % (what, got)
    assert_same(got, ref, what)
    if kw.get("layout", "gm") == "gm":
        assert (full[:, k.shape[1]:] == -777.0).all(), what + ": padding columns were written"
    assert bad == 0
    return ref


SHAPES = [(40, 1), (500, 3), (300, 63), (300, 64), (300, 65), (2000, 500), (150, 2051)]


@pytest.mark.parametrize("kind", vst_spec.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_kind_equals_the_specification(oracle, kind, shape):
    n, m = shape
    k = _counts(n, m, seed=n + 3 * m)
    sf = _sf(m, m)
    for variant in range(2 if m > 100 else 4):
        params = _kind_params(kind, k, sf, variant)
        ref = _check(oracle, k, sf, kind, params, "%s %dx%d variant %d" % (kind, n, m, variant), pad=8 * (variant % 2))
        if kind == "spline":
            u = vst_spec.asinh(oracle, vst_spec.normalized(k, sf))
            x = np.asarray(params["table"])[0]
            assert (u < x[0]).any(), "no value left of the first knot"
            if variant % 3 == 2:
                assert (u > x[-1]).any(), "no value right of the last knot"
        assert np.isfinite(ref).all()


@pytest.mark.parametrize("kind", vst_spec.KINDS)
@pytest.mark.parametrize("variant", ["r_layout", "float64_gm", "float64_r", "norm_matrix", "norm_matrix_r", "odd_ld_scalar",
                                     "misaligned"])
def test_layouts_count_types_and_normalization_matrix(oracle, kind, variant):
    n, m = 700, 67
    k = _counts(n, m, seed=11)
    nf = _sf(m, 3)
    kw = {}
    if variant in ("r_layout", "float64_r", "norm_matrix_r"):
        kw["layout"] = "r"
    if variant.startswith("float64"):
        kw["f64"] = True
    if variant.startswith("norm_matrix"):
        nf = np.exp(np.random.default_rng(2).normal(0, 0.3, (n, m)))
    if variant == "odd_ld_scalar":
        kw["pad"] = 3                               # ld = 75: rows do not start on 16-byte boundaries
    if variant == "misaligned":
        kw["misalign"] = True
    for v in range(3):
        _check(oracle, k, nf, kind, _kind_params(kind, k, nf, v), "%s %s variant %d" % (kind, variant, v), **kw)


@pytest.mark.parametrize("kind", vst_spec.KINDS)
def test_large_counts_nan_size_factor_and_right_of_last_knot(oracle, kind):
    n, m = 400, 70
    k = _counts(n, m, seed=23).astype(np.int64)
    rng = np.random.default_rng(4)
    big = rng.uniform(size=k.shape) < 0.2
    k[big] = rng.integers(2 ** 30, 2 ** 31, size=int(big.sum()))
    k[0, :] = 2 ** 31 - 1
    k[3] = 0
    k = k.astype(np.int32)
    assert k.max() == 2 ** 31 - 1 and (k[3] == 0).all()
    sf = _sf(m, 9)
    for v in range(4):
        params = _kind_params(kind, k, sf, v)
        if kind == "spline" and v % 3 != 2:
            # a table built for a smaller maximum: the large counts lie right of its last knot
            t, eta, xi = _product_table((_trend_a, _trend_b)[v % 3], np.minimum(k, 50000), sf)
            params = dict(table=t, eta=eta, xi=xi)
            u = vst_spec.asinh(oracle, vst_spec.normalized(k, sf))
            assert (u > t[0, -1]).any() and (u < t[0, 0]).any()
        _check(oracle, k, sf, kind, params, "%s big counts variant %d" % (kind, v))
    sf_nan = sf.copy()
    sf_nan[5] = np.nan
    params = _kind_params(kind, k, sf, 0)
    ref = vst_spec.transform(oracle, k, sf_nan, kind, **params)
    got, _, _ = _dev(k, sf_nan, kind, params)
    assert np.isnan(ref[:, 5]).all() and np.isfinite(np.delete(ref, 5, axis=1)).all()
    assert_same(got, ref, kind + " NaN size factor")


@pytest.mark.parametrize("variant", ["gm", "r", "float64", "norm_matrix", "nan_sf"])
@pytest.mark.parametrize("shape", [(40, 1), (300, 63), (300, 65), (1000, 500), (150, 2051)])
def test_row_statistics(oracle, variant, shape):
    n, m = shape
    k = _counts(n, m, seed=n + m)
    nf = _sf(m, 1)
    kw = {}
    if variant == "r":
        kw["layout"] = "r"
    if variant == "float64":
        kw["f64"] = True
    if variant == "norm_matrix":
        nf = np.exp(np.random.default_rng(2).normal(0, 0.3, (n, m)))
    if variant == "nan_sf":
        nf[0] = np.nan
    (mean, mx), _, _ = _dev(k, nf, "normalized", {}, stats=True, pad=8, **kw)
    rmean, rmx = vst_spec.row_stats(k, nf)
    assert_same(mean, rmean, "rowMeans")
    assert_same(mx, rmx, "row maxima")
    if variant == "nan_sf":
        assert np.isnan(mx).all() and np.isnan(mean).all()


# ---- past one grid round ----------------------------------------------------------------------------------------------------
STATS_LINE = re.compile(r"\[dsq\] vst_rowstats n=(\d+) m=(\d+): blocks (\d+), threads 256")
KIND_LINE = re.compile(r"\[dsq\] vst kind=(\d) n=(\d+) m=(\d+): mode (paired|gene-major|r-layout), items (\d+), blocks (\d+), threads (\d+)")


def _dev_line(monkeypatch, capfd, pattern, *a, **kw):
    """_dev under DSQ_VERBOSE: the result and the fields of the one line the launch printed (csrc/vst.hip)"""
    monkeypatch.setenv("DSQ_VERBOSE", "1")
    capfd.readouterr()
    got = _dev(*a, **kw)
    err = capfd.readouterr().err
    monkeypatch.delenv("DSQ_VERBOSE")
    lines = pattern.findall(err)
    assert len(lines) == 1, "no launch line in %r" % err
    print(err.strip())
    return got, lines[0]


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("variant", ["gm", "nan_sf"])
@pytest.mark.parametrize("m", [3, 65])
def test_row_statistics_past_one_round(oracle, monkeypatch, capfd, variant, m):
    """the persistent loop of vst_rowstats_kernel, `i += gridDim.x * 4`: n = round + 5 rows, launch_vst_rowstats' round being
    8 workgroups of four waves per CU (from the CU count, confirmed by the launch line); every row of both trips compared"""
    rnd = 8 * _cus() * 4                                                                # launch_vst_rowstats, csrc/vst.hip
    n = rnd + 5
    k = _counts(n, m, seed=n + m)
    nf = _sf(m, 1)
    if variant == "nan_sf":
        nf[0] = np.nan
    ((mean, mx), _, _), line = _dev_line(monkeypatch, capfd, STATS_LINE, k, nf, "normalized", {}, stats=True, pad=8)
    assert (int(line[0]), int(line[1])) == (n, m) and 4 * int(line[2]) == rnd < n
    rmean, rmx = vst_spec.row_stats(k, nf)
    assert_same(mean, rmean, "rowMeans")
    assert_same(mx, rmx, "row maxima")
    if variant == "nan_sf":
        assert np.isnan(mx).all() and np.isnan(mean).all()
    else:
        assert (mx[rnd:] > 0).any() and mx[3] == 0


@pytest.mark.parametrize("kind", ["parametric", "spline"])
@pytest.mark.parametrize("form", ["paired", "gene-major", "r-layout"])
def test_transform_past_one_round(oracle, monkeypatch, capfd, form, kind):
    """the grid-stride loop of vst_transform_kernel, `t += gridDim.x * blockDim.x`, on each launch form: pairs of samples
    (gene-major, even ld), single samples gene-major (odd ld) and R layout, a closed form (workgroups of 256, eight per CU)
    and the spline (workgroups of 512, four per CU).  The shape is the smallest number of rows that makes more items than
    launch_vst_kind's round holds, by the CU count; the launch line must show items > blocks x threads.  Every element is
    compared.  The 64-bit index branch (`total > 0xffffffff`) needs more than 34 GB of counts and output and stays untested."""
    threads, per_cu = (512, 4) if kind == "spline" else (256, 8)                         # launch_vst_kind, csrc/vst.hip
    rnd = _cus() * per_cu * threads
    m = 500 if form == "paired" else 67
    inner = (m + 1) // 2 if form == "paired" else m                                       # items of a row
    n = rnd // inner + 3
    k = _counts(n, m, seed=n + 3 * m)
    sf = _sf(m, m)
    params = _kind_params(kind, k, sf, 0)
    kw = dict(layout="r") if form == "r-layout" else dict(pad=3) if form == "gene-major" else dict(pad=8)
    ref = vst_spec.transform(oracle, k, sf, kind, **params)
    (got, full, bad), line = _dev_line(monkeypatch, capfd, KIND_LINE, k, sf, kind, params, **kw)
    _, ln, lm, mode, items, blocks, lthreads = line
    assert (int(ln), int(lm), mode, int(lthreads)) == (n, m, form, threads)
    assert int(items) == n * inner and int(blocks) * threads == rnd < int(items) < 2 * rnd
    assert_same(got, ref, "%s %s %dx%d" % (kind, form, n, m))
    if form != "r-layout":
        assert (full[:, m:] == -777.0).all(), "padding columns were written"
    assert bad == 0 and np.isfinite(ref).all()


@pytest.mark.parametrize("kind", vst_spec.KINDS)
def test_host_entry_equals_device_entry(oracle, kind):
    from deseq2_amd import native
    n, m = 997, 70
    k = _counts(n, m, seed=53)
    for nf in (_sf(m, 5), np.exp(np.random.default_rng(2).normal(0, 0.3, (n, m)))):
        params = _kind_params(kind, k, nf, 1)
        got, _, _ = _dev(k, nf, kind, params)
        (mean, mx), _, _ = _dev(k, nf, kind, params, stats=True)
        h, hmean, hmax = native.vst(k, nf, kind, want_stats=True, **params)
        assert_same(h, got, "dsq_vst " + kind)
        assert_same(hmean, mean, "dsq_vst rowMean")
        assert_same(hmax, mx, "dsq_vst rowMax")
        assert_same(native.vst(k.astype(np.float64), nf, kind, **params), got, "dsq_vst, REALSXP counts " + kind)


def test_non_default_stream_gives_the_same_bits(oracle):
    import torch
    k = _counts(3000, 130, seed=61)
    sf = _sf(130, 2)
    s = torch.cuda.Stream()
    for kind in vst_spec.KINDS:
        params = _kind_params(kind, k, sf, 0)
        a, _, _ = _dev(k, sf, kind, params)
        b, _, _ = _dev(k, sf, kind, params, stream=s)
        assert a.tobytes() == b.tobytes(), kind
    a, _, _ = _dev(k, sf, "normalized", {}, stats=True)
    b, _, _ = _dev(k, sf, "normalized", {}, stats=True, stream=s)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_argument_errors_return_their_codes_and_launch_nothing():
    from deseq2_amd import _lib as L, native
    k = _counts(50, 9, seed=1)
    sf = _sf(9, 1)
    tab = _hand_table()
    uns = tab.copy()
    uns[0, 5] = uns[0, 4]
    cases = [("parametric", dict(asymptDisp=0.0, extraPois=1.0), L.DSQ_ERR_ARG),
             ("parametric", dict(asymptDisp=-1.0, extraPois=1.0), L.DSQ_ERR_ARG),
             ("parametric", dict(asymptDisp=np.nan, extraPois=1.0), L.DSQ_ERR_ARG),
             ("mean", dict(alpha=0.0), L.DSQ_ERR_ARG),
             ("spline", dict(table=tab[:, :1], eta=1.0, xi=0.0), L.DSQ_ERR_ARG),
             ("spline", dict(table=uns, eta=1.0, xi=0.0), L.DSQ_ERR_ARG),
             ("spline", dict(eta=1.0, xi=0.0), L.DSQ_ERR_ARG),
             ("spline", dict(table=np.vstack([np.arange(2000.0)] * 5), eta=1.0, xi=0.0), L.DSQ_ERR_UNSUPPORTED)]
    for kind, params, code in cases:
        rc, outall, _ = _dev(k, sf, kind, params)
        assert rc == code, (kind, params, rc)
        assert (outall == -777.0).all(), "an output was written after an argument error"
    kbad = k.astype(np.float64)
    kbad[7, 3] = 2.5
    _, _, bad = _dev(kbad, sf, "log2", dict(pc=1.0), f64=True)
    assert bad == 1
    for v in (2.5, -1.0):
        kbad[7, 3] = v
        with pytest.raises(L.DsqError) as ei:
            native.vst(kbad, sf, "normalized")
        assert ei.value.code == L.DSQ_ERR_VALUE


# ---------------------------------------------------------------------------------------------------------------- end to end
def _e2e_bound(ref, fn, q, spline=None):
    """DeviceEngine against HostEngine(oracle): the dispersion function is bitwise the same (asserted), so both sides
    evaluate the same expression of the same q and differ in libm's log / asinh / log2 against dlog and the asinh built
    from it.  tests/vst_spec.py derives the distance of either side to the exact value, per element and for the formula that
    was fitted (spec_bound: the closed forms with their own coefficients; spline_bound: the spline formula, whose argument
    asinh(q) carries up to 9 ulps that the slope of eta S passes on); the two sides are at most twice that apart."""
    if fn["fitType"] == "custom":
        return 2 * vst_spec.spline_bound(spline["table"], spline["eta"], spline["xi"], np.arcsinh(q), ref)
    if fn["fitType"] == "mean":
        al = float(fn["coefficients"])
        return 2 * vst_spec.spec_bound("mean", ref, A=np.arcsinh(np.sqrt(al * q)), la=np.log(al))
    return 2 * vst_spec.spec_bound("parametric", ref)


def _oracle_engine():
    """HostEngine(oracle) with the one step HostEngine states in libm taken from the oracle's arithmetic as well:
    HostEngine.size_factors is "equal to rounding, not to the bit" by design, and a size factor that
    differs in its last bit moves every bit downstream, so the bitwise comparison of the dispersion function asked of this
    test needs the size-factor step of the host side in the specified arithmetic: tests/sf_spec.py, the statement the
    device is held to bit for bit by tests/test_gpu_size_factors.py.  The calls on the two engines stay the same.  Used
    only where the call estimates the factors; with given factors the host side is the plain HostEngine(oracle)."""
    from deseq2_amd.engine import HostEngine, SF_ALL_ZERO
    from oracle import oracle as O
    from tests import sf_spec

    class OracleEngine(HostEngine):
        def size_factors(self, y, type="ratio", geoMeans=None, control=None, normMatrix=None):
            r = sf_spec.size_factors(O, np.asarray(y), type=type, geoMeans=geoMeans,
                                     control=None if control is None else np.asarray(control) != 0, normMatrix=normMatrix)
            if r["status"] == 1:
                raise ValueError(SF_ALL_ZERO)
            return r
    return OracleEngine(O)


def _pair(d, sf, **kw):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    from oracle import oracle as O
    out = []
    for E in (DeviceEngine(), HostEngine(O) if sf is not None else _oracle_engine()):
        out.append(core.DESeqDataSet(d["counts"], d["x"], sizeFactors=sf, engine=E, **kw))
    return out


def _same_transform(a, b, what):
    fa, fb = a.dds.dispersionFunction, b.dds.dispersionFunction
    assert fa["fitType"] == fb["fitType"], what
    if fa["fitType"] != "custom":
        assert_same(np.asarray(fa["coefficients"], float), np.asarray(fb["coefficients"], float), what + " dispersion function")
    else:
        assert_same(a.dds.attrs["vst_spline"]["table"], b.dds.attrs["vst_spline"]["table"], what + " spline table")
    A, B = a.assay(), b.assay()
    fin = np.isfinite(B)
    assert (np.isfinite(A) == fin).all()
    err = np.abs(A - B)[fin]
    q = np.asarray(b.dds.engine.to_numpy(core_normalized(b.dds)))
    bound = _e2e_bound(B[fin], fa, q[fin], a.dds.attrs.get("vst_spline"))
    print("%s: max |device - host| = %.3g (smallest bound %.3g)" % (what, err.max(), bound.min()))
    assert (err <= bound).all(), what


def core_normalized(dds):
    from deseq2_amd import core
    return core.normalized_counts(dds).handle


def _custom_fit(means, disps):
    c = float(np.median(disps))
    return lambda mu: c + 1.5 / np.asarray(mu, float)


@pytest.mark.parametrize("fitType", ["parametric", "mean", "custom"])
@pytest.mark.parametrize("blind", [True, False])
def test_vst_end_to_end(fitType, blind):
    from deseq2_amd import core
    from tests.helpers import make_case
    d = make_case(3000, 12, "two_group", seed=5, sf_random=True, drop_all_zero=False)
    ft = _custom_fit if fitType == "custom" else fitType
    for sf in (d["size_factors"], None):                 # given factors, and factors estimated by vst() itself
        dev, host = _pair(d, sf)
        a = core.vst(dev, blind=blind, nsub=500, fitType=ft)
        b = core.vst(host, blind=blind, nsub=500, fitType=ft)
        assert_same(a.dds.attrs["vst_rows"], b.dds.attrs["vst_rows"], "subset rows")
        if sf is None:
            assert not np.all(a.dds.sizeFactors == 1.0)
            assert_same(a.dds.sizeFactors, b.dds.sizeFactors, "estimated size factors")
        _same_transform(a, b, "vst %s blind=%s" % (fitType, blind))
        assert a.handle.t.is_cuda                         # the result is a resident handle


@pytest.mark.parametrize("fitType", ["parametric", "mean", "custom"])
def test_variance_stabilizing_transformation_end_to_end(fitType):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine
    from tests.helpers import make_case
    d = make_case(1200, 10, "two_group", seed=7, sf_random=True, drop_all_zero=False)
    assert (d["counts"].sum(axis=1) == 0).any()
    ft = _custom_fit if fitType == "custom" else fitType
    for blind in (True, False):
        dev, host = _pair(d, d["size_factors"])
        a = core.varianceStabilizingTransformation(dev, blind=blind, fitType=ft)
        b = core.varianceStabilizingTransformation(host, blind=blind, fitType=ft)
        _same_transform(a, b, "VST object %s blind=%s" % (fitType, blind))
    # matrix input: the `~ 1` object, size factors estimated
    a = core.varianceStabilizingTransformation(d["counts"], fitType=ft, engine=DeviceEngine(), sfType="poscounts")
    b = core.varianceStabilizingTransformation(d["counts"], fitType=ft, engine=_oracle_engine(), sfType="poscounts")
    assert_same(a.dds.sizeFactors, b.dds.sizeFactors, "matrix input: size factors")
    _same_transform(a, b, "VST matrix " + fitType)


def test_frozen_vst_fits_nothing(oracle):
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine
    from tests.helpers import make_case
    d = make_case(800, 8, "two_group", seed=9, sf_random=True)
    E = DeviceEngine()
    dds = core.DESeqDataSet(d["counts"], d["x"], sizeFactors=d["size_factors"], engine=E)
    dds.dispersionFunction = {"fitType": "parametric", "coefficients": np.array([0.04, 3.0]), "varLogDispEsts": None}
    E.record = []
    t = core.varianceStabilizingTransformation(dds, blind=False)
    names = [r[0] for r in E.record]
    E.record = None
    assert names == ["vst_transform"], names
    ref = vst_spec.transform(oracle, d["counts"], d["size_factors"], "parametric", asymptDisp=0.04, extraPois=3.0)
    assert_same(t.assay(), ref, "frozen VST")
    assert_same(core.normTransform(dds, pc=1).assay(), vst_spec.transform(oracle, d["counts"], d["size_factors"], "log2", pc=1.0),
                "normTransform")
    assert_same(core.normalized_counts(dds).assay(), vst_spec.normalized(d["counts"], d["size_factors"]), "normalized counts")
