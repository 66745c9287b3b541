"""estimateSizeFactors on the device (csrc/size_factors.hip) against the numpy specification of tests/sf_spec.py, BIT FOR
BIT: dlog / dexp equal the oracle's log / exp, the row sums are the wave-order sums, the median is an exact order statistic."""
import ctypes as C

import numpy as np
import pytest

from tests import sf_spec
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu


def _counts(n, m, seed, zeros=0.01, hi=6.0):
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.normal(hi, 2, (n, 1)) * np.exp(rng.normal(0, 0.4, m))[None, :]
    k = rng.poisson(mu).astype(np.int64) + (0 if zeros else 1)      # zeros = 0: no zero at all
    if zeros:
        k[rng.uniform(size=k.shape) < zeros] = 0
    return k.astype(np.int32)


def _dev(k, type="ratio", geoMeans=None, control=None, normMatrix=None, layout="gm", pad=0, f64=False):
    """dsq_size_factors_dev through ctypes on tensors laid out as asked: gene-major with ld = round8(m) + pad (padding
    filled with garbage) or R layout; int32 or float64 counts.  Returns host (sf, loggeomeans, nf or None, status)."""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    k = np.asarray(k)
    n, m = k.shape
    kt = np.float64 if f64 else np.int32

    def place(a, dtype, garbage):
        if layout == "r":
            return torch.as_tensor(np.ascontiguousarray(a.T.astype(dtype)), device=dev), 0
        ld = ((m + 7) & ~7) + pad
        buf = np.full((n, ld), garbage, dtype=dtype)
        buf[:, :m] = a
        return torch.as_tensor(buf, device=dev), ld
    yt, ld = place(k, kt, 12345)
    nmt = None if normMatrix is None else place(np.asarray(normMatrix, np.float64), np.float64, np.nan)[0]
    sf = torch.full((m,), -7.0, dtype=torch.float64, device=dev)
    lgm = torch.empty(n, dtype=torch.float64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    nf = None if nmt is None else torch.full_like(nmt, -3.0)
    gmt = None if geoMeans is None else torch.as_tensor(np.asarray(geoMeans, np.float64), device=dev)
    ct = None if control is None else torch.as_tensor(np.asarray(control).astype(np.int32), device=dev)
    wsb = int(L.lib().dsq_size_factors_workspace_bytes(n, m))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = L.DsqSizeFactorArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R if layout == "r" else L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=p(yt),
                            y_type=L.DSQ_Y_FLOAT64 if f64 else L.DSQ_Y_INT32, type=L.DSQ_SF[type], geoMeans=p(gmt),
                            control=p(ct), normMatrix=p(nmt), workspace=p(ws), workspace_bytes=wsb)
    o = L.DsqSizeFactorOut(sizeFactors=p(sf), loggeomeans=p(lgm), normalizationFactors=p(nf), status=p(st))
    L.check(L.lib().dsq_size_factors_dev(C.byref(a), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    nfh = None
    if nf is not None:
        nfh = nf.cpu().numpy()
        nfh = nfh.T if layout == "r" else nfh[:, :m]
    return sf.cpu().numpy(), lgm.cpu().numpy(), nfh, int(st.cpu()[0])


def _check(O, k, what, mask=None, **kw):
    ref = sf_spec.size_factors(O, k, type=kw.get("type", "ratio"), geoMeans=kw.get("geoMeans"), control=mask,
                               normMatrix=kw.get("normMatrix"))
    sf, lgm, nf, st = _dev(k, control=mask, **kw)
    assert st == ref["status"], what
    assert_same(lgm, ref["loggeomeans"], what + " loggeomeans")
    assert_same(sf, ref["sizeFactors"], what + " sizeFactors")
    if "normMatrix" in kw:
        assert_same(nf, ref["normalizationFactors"], what + " normalizationFactors")
    return ref, sf


MODES = ["ratio", "poscounts", "geoMeans", "control_index", "control_logical", "normMatrix", "normMatrix_poscounts"]


def _mode_args(mode, k, seed):
    rng = np.random.default_rng(seed + 99)
    n, m = k.shape
    kw, mask = {}, None
    if mode in ("poscounts", "normMatrix_poscounts"):
        kw["type"] = "poscounts"
    if mode == "geoMeans":
        kw["geoMeans"] = np.exp(rng.normal(4, 1, n))
        kw["geoMeans"][5::11] = 0.0
    if mode == "control_index":
        from deseq2_amd.engine import control_flags
        mask = control_flags(rng.choice(n, max(1, n // 3), replace=False), n).astype(bool)
    if mode == "control_logical":
        mask = rng.uniform(size=n) < 0.5
        mask[0] = True
    if mode.startswith("normMatrix"):
        kw["normMatrix"] = np.exp(rng.normal(0, 0.3, (n, m)))
    return kw, mask


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 6), (1000, 6), (997, 48), (3000, 70)])
def test_every_mode_equals_the_specification(oracle, mode, shape):
    n, m = shape
    k = _counts(n, m, seed=n * 3 + m, zeros=0.0 if n == 1 else 0.05 if "poscounts" in mode or mode == "geoMeans" else 0.005)
    kw, mask = _mode_args(mode, k, n)
    ref, _ = _check(oracle, k, "%s %dx%d" % (mode, n, m), mask=mask, **kw)
    assert ref["status"] == 0 and np.isfinite(ref["sizeFactors"]).all()


@pytest.mark.parametrize("shape,mode", [((50000, 500), "ratio"), ((50000, 500), "poscounts"), ((4000, 2000), "ratio"),
                                        ((4000, 2000), "normMatrix")])
def test_large_shapes(oracle, shape, mode):
    """more than one sample tile, many gene slabs"""
    n, m = shape
    k = _counts(n, m, seed=n + m, zeros=0.02 if mode == "poscounts" else 0.0002)
    kw, mask = _mode_args(mode, k, n)
    ref, _ = _check(oracle, k, "%s %dx%d" % (mode, n, m), mask=mask, **kw)
    assert ref["status"] == 0 and np.isfinite(ref["sizeFactors"]).all()


def test_normalization_factors_past_one_round(oracle):
    """sf_norm_factors_kernel's gene loop (`i += nwave`, a wave per gene; launch_size_factors: eight workgroups of four waves
    per CU, the grid sf_loggeomeans_kernel has too) on five rows more than that round: the normalization-factor matrix, the
    log geometric means and the factors against the specification.  (test_large_shapes takes sf_loggeomeans_kernel to 50 000
    rows; its normMatrix shape has 4 000.)"""
    import torch
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 4 + 5        # launch_size_factors, csrc/size_factors.hip
    k = _counts(n, 3, seed=n, zeros=0.0002)
    nm = np.exp(np.random.default_rng(7).normal(0, 0.3, k.shape))
    ref, _ = _check(oracle, k, "normMatrix %dx3" % n, normMatrix=nm)
    assert ref["status"] == 0 and np.isfinite(ref["normalizationFactors"]).all()


@pytest.mark.parametrize("variant", ["padded_ld", "r_layout", "float64_gm", "float64_r", "r_layout_normMatrix"])
def test_layouts_and_count_types(oracle, variant):
    k = _counts(997, 70, seed=17)
    kw = {}
    if variant == "padded_ld":
        kw.update(pad=24)
    if variant.startswith("r_layout") or variant == "float64_r":
        kw.update(layout="r")
    if variant.startswith("float64"):
        kw.update(f64=True)
    if variant.endswith("normMatrix"):
        kw.update(normMatrix=np.exp(np.random.default_rng(3).normal(0, 0.3, k.shape)))
    _check(oracle, k, variant, **kw)
    _check(oracle, k, variant + " poscounts", type="poscounts", **kw)


def test_counts_up_to_int32_max(oracle):
    k = _counts(500, 70, seed=23).astype(np.int64)
    rng = np.random.default_rng(4)
    big = rng.uniform(size=k.shape) < 0.2
    k[big] = rng.integers(2 ** 30, 2 ** 31, size=int(big.sum()))
    k[0, :] = 2 ** 31 - 1
    k = k.astype(np.int32)
    assert k.max() == 2 ** 31 - 1 and k.min() >= 0
    _check(oracle, k, "int32 max")
    _check(oracle, k, "int32 max poscounts", type="poscounts")


def test_odd_and_even_selection_counts(oracle):
    """both branches of the median: the middle value, and (a + b) * 0.5 of the two middle values"""
    k = _counts(2001, 70, seed=31, zeros=0.0)
    k[np.arange(35), np.arange(35)] = 0              # samples 0 .. 34 lose one gene each
    gm = np.exp(np.log(np.maximum(k, 1)).mean(axis=1))
    ref, _ = _check(oracle, k, "odd/even", geoMeans=gm)
    par = ref["counts_selected"] % 2
    assert (par == 0).any() and (par == 1).any()
    ref, _ = _check(oracle, k, "odd/even poscounts", type="poscounts")
    par = ref["counts_selected"] % 2
    assert (par == 0).any() and (par == 1).any()


def test_heavy_ties(oracle):
    """counts in 0 .. 3: a handful of distinct logs, so the two middle ranks sit in long runs of equal keys"""
    rng = np.random.default_rng(8)
    k = rng.integers(0, 4, size=(3000, 70)).astype(np.int32)
    _check(oracle, k, "ties poscounts", type="poscounts")
    _check(oracle, k, "ties geoMeans", geoMeans=np.full(3000, 1.5))
    k1 = np.maximum(k, 1)
    _check(oracle, k1, "ties ratio")
    k2 = rng.integers(1, 3, size=(1000, 6)).astype(np.int32)          # even selections split between two values
    _check(oracle, k2, "ties two values", geoMeans=np.ones(1000))


def test_all_zero_sample_is_nan(oracle):
    """a sample that selects nothing gets NaN.  "ratio" cannot meet one (every gene then has a zero: status 1); on the
    geoMeans / poscounts path the reference's closing division by exp(mean(log(sf))) makes every factor NA with it
    (R/core.R:575).  Before that division the other samples are what they are without the empty one: shown through
    loggeomeans and the "ratio" run on the remaining samples."""
    k = _counts(1000, 12, seed=41, zeros=0.0)
    gm = np.exp(np.log(k.astype(float)).mean(axis=1))
    k0 = k.copy()
    k0[:, 5] = 0
    ref, sf = _check(oracle, k0, "all-zero sample geoMeans", geoMeans=gm)
    assert ref["counts_selected"][5] == 0 and np.isnan(sf).all()
    ref, sf = _check(oracle, k0, "all-zero sample poscounts", type="poscounts")
    assert np.isnan(sf).all()
    sf0, _, _, st = _dev(k0)
    assert st == 1 and np.isnan(sf0).all()


def test_every_gene_with_a_zero(oracle):
    from deseq2_amd import native, _lib
    k = _counts(400, 9, seed=43, zeros=0.0)
    k[np.arange(400), np.arange(400) % 9] = 0
    _, _, _, st = _dev(k)
    assert st == 1
    with pytest.raises(_lib.DsqError) as ei:
        native.estimateSizeFactorsForMatrix(k)
    assert ei.value.code == _lib.DSQ_ERR_FIT
    ref, sf = _check(oracle, k, "poscounts on the same matrix", type="poscounts")
    assert ref["status"] == 0 and np.isfinite(sf).all()
    assert_same(native.estimateSizeFactorsForMatrix(k, type="poscounts"), sf, "host entry poscounts")


def test_control_genes_single_row(oracle):
    k = _counts(500, 70, seed=47)
    k[123] = np.maximum(k[123], 1)
    mask = np.zeros(500, bool)
    mask[123] = True
    ref, _ = _check(oracle, k, "single control row", mask=mask)
    assert (ref["counts_selected"] == 1).all()


@pytest.mark.parametrize("mode", MODES)
def test_host_entry_equals_device_entry(oracle, mode):
    from deseq2_amd import native
    k = _counts(997, 70, seed=53, zeros=0.05 if "poscounts" in mode or mode == "geoMeans" else 0.005)
    kw, mask = _mode_args(mode, k, 7)
    sf, lgm, nf, st = _dev(k, control=mask, **kw)
    assert st == 0
    got, glgm = native.estimateSizeFactorsForMatrix(k, controlGenes=mask, want_loggeomeans=True, **kw)
    assert_same(glgm, lgm, "host loggeomeans")
    assert_same(got, nf if "normMatrix" in kw else sf, "host entry " + mode)
    got64 = native.estimateSizeFactorsForMatrix(k.astype(np.float64), controlGenes=mask, **kw)
    assert_same(got64, got, "host entry, REALSXP counts " + mode)


def test_two_runs_give_identical_bits():
    k = _counts(20000, 200, seed=59)
    a = _dev(k, type="poscounts")
    b = _dev(k, type="poscounts")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    nm = np.exp(np.random.default_rng(1).normal(0, 0.3, k.shape))
    a, b = _dev(k, normMatrix=nm), _dev(k, normMatrix=nm)
    assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_engine_and_from_device(oracle):
    """core.estimateSizeFactors on a DeviceEngine data set and on one built by from_device (no host counts)"""
    import torch
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine
    k = _counts(1500, 24, seed=61)
    x = np.column_stack([np.ones(24), np.repeat([0.0, 1.0], 12)])
    ref = sf_spec.size_factors(oracle, k)
    E = DeviceEngine()
    dds = core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=E))
    assert_same(dds.sizeFactors, ref["sizeFactors"], "DeviceEngine sizeFactors")
    assert_same(E.to_numpy(dds.nf), np.broadcast_to(ref["sizeFactors"][None, :], k.shape), "nf handle")
    kr = torch.as_tensor(np.ascontiguousarray(k.T), device=E.device)
    d2 = core.DESeqDataSet.from_device(E, kr, torch.ones((24, 1500), dtype=torch.float64, device=E.device), x)
    assert d2.counts_host is None
    core.estimateSizeFactors(d2, type="poscounts")
    assert_same(d2.sizeFactors, sf_spec.size_factors(oracle, k, type="poscounts")["sizeFactors"], "from_device poscounts")
    nm = np.exp(np.random.default_rng(2).normal(0, 0.3, k.shape))
    d3 = core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=E), normMatrix=nm)
    assert d3.sizeFactors is None
    assert_same(E.to_numpy(d3.nf), sf_spec.size_factors(oracle, k, normMatrix=nm)["normalizationFactors"], "nf matrix")


def _same_analysis(a, b, E):
    assert set(a.mcols) == set(b.mcols)
    for key in b.mcols:
        assert_same(np.asarray(a.mcols[key], float), np.asarray(b.mcols[key], float), "mcols$" + key)
    assert_same(E.to_numpy(a.assays["mu"]), E.to_numpy(b.assays["mu"]), "mu")


@pytest.mark.parametrize("sfType", ["ratio", "poscounts"])
def test_fused_chain_with_sftype(sfType):
    from deseq2_amd import core, fused
    from deseq2_amd.engine import DeviceEngine
    from tests.helpers import make_case
    d = make_case(2000, 16, "two_group", seed=5, sf_random=True)
    E = DeviceEngine()
    a = fused.DESeq(core.DESeqDataSet(d["counts"], d["x"], engine=E), sfType=sfType)
    assert a.attrs.get("fused") and a.sizeFactors is not None and not np.all(a.sizeFactors == 1.0)
    b = fused.DESeq(core.DESeqDataSet(d["counts"], d["x"], sizeFactors=a.sizeFactors, engine=E))
    assert b.attrs.get("fused")
    _same_analysis(a, b, E)


def test_fused_chain_with_norm_matrix():
    from deseq2_amd import core, fused
    from deseq2_amd.engine import DeviceEngine
    from tests.helpers import make_case
    d = make_case(2000, 16, "two_group", seed=6, sf_random=True)
    nm = np.exp(np.random.default_rng(9).normal(0, 0.2, d["counts"].shape))
    E = DeviceEngine()
    a = core.estimateSizeFactors(core.DESeqDataSet(d["counts"], d["x"], engine=E), normMatrix=nm)
    nf = E.to_numpy(a.nf).copy()
    fused.DESeq(a)
    b = fused.DESeq(core.DESeqDataSet(d["counts"], d["x"], normalizationFactors=nf, engine=E))
    assert a.attrs.get("fused") and b.attrs.get("fused")
    _same_analysis(a, b, E)
