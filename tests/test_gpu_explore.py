"""Sample PCA and sample distances on the device (csrc/explore.hip) against the numpy specification of
tests/explore_spec.py, BIT FOR BIT (rowMean, rowVar, select, G, dist2, dist, and through the same LAPACK call sdev / x /
percentVar): dsq_top_var_dev / dsq_sample_pairs_dev on the smallest shapes at which the kernels can go wrong, the host
entries, core.pca / plotPCA / sampleDists / rowVars on a DeviceEngine against the same calls on HostEngine, and once the
device's outputs against the statements that share nothing with the specification (tests/explore_cases.py)."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import explore_cases as CS
from tests import explore_spec as S
from tests.helpers import assert_bits, assert_same

pytestmark = pytest.mark.gpu

PAD = 3                                   # ld = m + 3, the padding filled with NaN: a read past m shows in every sum


def _resident(A, pad=PAD):
    import torch
    n, m = A.shape
    buf = np.full((n, m + pad), np.nan)
    buf[:, :m] = A
    return torch.as_tensor(buf, device="cuda:0"), m + pad


def _top_var_dev(A, ntop, pad=PAD):
    """dsq_top_var_dev through ctypes; outputs prefilled with garbage, one spare entry behind select"""
    import torch
    from deseq2_amd import _lib as L
    n, m = A.shape
    xt, ld = _resident(A, pad)
    k = max(0, min(ntop, n))
    pack = torch.full((2, n), -777.0, dtype=torch.float64, device="cuda:0")
    sel = torch.full((k + 1,), -5, dtype=torch.int32, device="cuda:0")
    a = L.sized(L.DsqTopVarArgs, n=n, m=m, ld=ld, x=xt.data_ptr(), ntop=ntop)
    o = L.sized(L.DsqTopVarOut, rowMean=pack[0].data_ptr(), rowVar=pack[1].data_ptr(), select=sel.data_ptr())
    st = torch.cuda.current_stream()
    L.check(L.lib().dsq_top_var_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    h, s = pack.cpu().numpy(), sel.cpu().numpy()
    assert s[k] == -5                                                   # nothing written past the selection
    assert_bits(xt.cpu().numpy()[:, :m], A, "the input is left alone")
    return h[0], h[1], s[:k].astype(np.int64)


def _pairs_dev(A, kind, rows=None, centre=None, pad=PAD):
    import torch
    from deseq2_amd import _lib as L
    n, m = A.shape
    xt, ld = _resident(A, pad)
    rt = None if rows is None else torch.as_tensor(np.ascontiguousarray(rows, np.int32), device="cuda:0")
    ct = None if centre is None else torch.as_tensor(np.ascontiguousarray(centre, np.float64), device="cuda:0")
    out = torch.full((m * m + 1,), -777.0, dtype=torch.float64, device="cuda:0")
    a = L.sized(L.DsqSamplePairsArgs, n=n, m=m, ld=ld, x=xt.data_ptr(), kind=L.DSQ_PAIRS[kind], nrows=0 if rows is None else len(rows),
                rows=None if rt is None else rt.data_ptr(), centre=None if ct is None else ct.data_ptr())
    o = L.sized(L.DsqSamplePairsOut, out=out.data_ptr())
    st = torch.cuda.current_stream()
    L.check(L.lib().dsq_sample_pairs_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    h = out.cpu().numpy()
    assert h[m * m] == -777.0                                           # nothing written past the matrix
    return h[:m * m].reshape(m, m)


def _all_outputs(A, what, rows=None):
    """every output of the two entry points on A against the specification"""
    mean, var, _ = _top_var_dev(A, 0)
    smean, svar = S.row_vars(A)
    assert_bits(mean, smean, what + ": rowMean")
    assert_bits(var, svar, what + ": rowVar")
    centre = smean if rows is None else smean[rows]
    d2 = _pairs_dev(A, "dist2", rows=rows)
    want = S.pair_sums(A, "dist2", rows=rows)
    assert_bits(d2, want, what + ": dist2")
    assert_bits(d2, d2.T, what + ": dist2 symmetric")
    with np.errstate(all="ignore"):
        assert_bits(_pairs_dev(A, "dist", rows=rows), np.sqrt(want), what + ": dist")
    G = _pairs_dev(A, "gram", rows=rows, centre=centre)
    assert_bits(G, S.pair_sums(A, "gram", rows=rows, centre=centre), what + ": gram")
    assert_bits(G, G.T, what + ": gram symmetric")


@pytest.mark.parametrize("m", CS.M_LIST)
def test_sample_counts_around_the_tile(m):
    """one tile, a tile edge, several tiles with a ragged last one: diagonal and off-diagonal tiles and the mirror"""
    _all_outputs(CS.matrix(CS.L + 5, m, seed=100 + m), "m = %d" % m)


@pytest.mark.parametrize("R", CS.ROWS_SUMMED)
def test_rows_summed_around_the_slice(R):
    assert S.slice_length(R, 65) == CS.L
    _all_outputs(CS.matrix(R, 65, seed=R), "%d rows" % R)


def test_several_tiles_and_several_slices():
    """m = 129: six tiles; 3 L + 7 rows: four slices, the last one short"""
    _all_outputs(CS.matrix(3 * CS.L + 7, 129, seed=12), "6 tiles x 4 slices")


def test_a_slice_longer_than_the_shortest():
    """m = 130: six tiles, at most 341 slices; one row more than 341 slices of 64 rows hold makes the slices 65 rows long"""
    from deseq2_amd import _lib as L
    R = 341 * CS.L + 1
    assert S.slice_length(R, 130) == CS.L + 1 == L.lib().dsq_sample_pairs_slice_rows(R, 130)
    A = CS.matrix(R, 130, seed=13)
    assert_bits(_pairs_dev(A, "dist2"), S.pair_sums(A, "dist2"), "dist2 at L = 65")


@pytest.mark.parametrize("which", ["single", "all", "permutation", "repeated"])
def test_row_lists(which):
    A = CS.matrix(90, 7, seed=3)
    _all_outputs(A, "rows: " + which, rows=CS.row_lists(90, seed=4)[which])


def test_a_listed_row_outside_the_matrix_is_not_read():
    """dsq_sample_pairs_dev cannot look at a resident list before the launch: the kernel does not read such a row, its sums
    are NaN (the host entry refuses the list: tests/test_explore_cpu.py)"""
    A = CS.matrix(10, 4, seed=2)
    d2 = _pairs_dev(A, "dist2", rows=[0, 10, 3, -1])
    off = ~np.eye(4, dtype=bool)
    assert np.isnan(d2[off]).all() and (np.diag(d2) == 0).all()


def test_a_nan_spreads_over_the_pairs_of_its_sample():
    A = CS.matrix(70, 5, seed=8)
    A[11, 3] = np.nan
    d = _pairs_dev(A, "dist")
    assert_bits(d, S.sample_dists(A), "dist with a NaN")
    assert np.isnan(d[3, [0, 1, 2, 4]]).all() and np.isfinite(np.delete(np.delete(d, 3, 0), 3, 1)).all() and d[3, 3] == 0


ROWVARS_LINE = re.compile(r"\[dsq\] row_vars n=(\d+) m=(\d+): blocks (\d+), threads 256, (one read|two sweeps)")


def _with_line(monkeypatch, capfd, pattern, fn):
    monkeypatch.setenv("DSQ_VERBOSE", "1")
    capfd.readouterr()
    got = fn()
    err = capfd.readouterr().err
    monkeypatch.delenv("DSQ_VERBOSE")
    lines = pattern.findall(err)
    assert len(lines) == 1, "no launch line in %r" % err
    return got, lines[0]


@pytest.mark.parametrize("m", [3, 65])
def test_row_variances_past_one_round(monkeypatch, capfd, m):
    """the persistent loop of row_vars_kernel, `i += gridDim.x * 4`: n = round + 5 rows, the round being 8 workgroups of four
    waves per CU (from the CU count, confirmed by the launch line); every row of both trips compared"""
    import torch
    rnd = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    n = rnd + 5
    A = CS.matrix(n, m, seed=n + m)
    (mean, var, _), line = _with_line(monkeypatch, capfd, ROWVARS_LINE, lambda: _top_var_dev(A, 0))
    assert (int(line[0]), int(line[1])) == (n, m) and 4 * int(line[2]) == rnd < n and line[3] == "one read"
    smean, svar = S.row_vars(A)
    assert_bits(mean, smean, "rowMean")
    assert_bits(var, svar, "rowVar")


@pytest.mark.parametrize("m", [511, 512, 513, 600])
def test_rows_around_the_register_resident_width(monkeypatch, capfd, m):
    from deseq2_amd import _lib as L
    W = L.lib().dsq_row_vars_register_width()
    assert W == 512
    A = CS.matrix(9, m, seed=m)
    A[4] = 3.0
    A[6, m - 1] = np.nan
    (mean, var, _), line = _with_line(monkeypatch, capfd, ROWVARS_LINE, lambda: _top_var_dev(A, 0))
    assert line[3] == ("one read" if m <= W else "two sweeps")
    smean, svar = S.row_vars(A)
    assert_bits(mean, smean, "rowMean")
    assert_bits(var, svar, "rowVar")
    assert var[4] == 0 and np.isnan(var[6])


def test_the_order_of_the_selection():
    A = CS.selection_matrix()
    n = A.shape[0]
    _, rv = S.row_vars(A)
    want = CS.lexsort_order(rv)
    for ntop in (1, n - 1, n, n + 10):
        mean, var, sel = _top_var_dev(A, ntop)
        assert_bits(var, rv, "rowVar")
        assert_same(sel, want[:min(ntop, n)], "order, ntop = %d" % ntop)
        assert_same(sel, S.top_var(rv, ntop), "order against the specification, ntop = %d" % ntop)


def test_the_order_over_several_sort_tiles():
    """5000 rows (three tiles of the radix sort), a third of them duplicates of others, constant rows and NaN rows among them"""
    rng = np.random.Generator(np.random.PCG64(77))
    A = CS.matrix(5000, 4, seed=9)
    dup = rng.choice(5000, size=1600, replace=False)
    A[dup] = A[rng.integers(0, 5000, size=1600)]
    A[rng.choice(5000, size=40, replace=False)] = 5.0
    A[rng.choice(5000, size=30, replace=False), 1] = np.nan
    _, rv = S.row_vars(A)
    want = CS.lexsort_order(rv)
    assert np.isnan(rv).sum() >= 30 and (np.diff(np.sort(rv[~np.isnan(rv)])) == 0).sum() > 100
    _, var, sel = _top_var_dev(A, 5000)
    assert_bits(var, rv, "rowVar")
    assert_same(sel, want, "order of 5000 rows")
    assert_same(_top_var_dev(A, 500)[2], want[:500], "the first 500")


# ---------------------------------------------------------------------------------------------- the engine and core
@pytest.fixture(scope="module")
def engines():
    from deseq2_amd.engine import DeviceEngine, HostEngine
    return DeviceEngine("cuda:0"), HostEngine()


class _Obj:
    def __init__(self, engine, factors=None):
        self.engine, self.attrs = engine, ({"factors": factors} if factors else {})


def _transform(E, A, factors=None):
    from deseq2_amd import core
    return core.DESeqTransform(_Obj(E, factors), E.matrix(A), "vst")


@pytest.mark.parametrize("which", ["planted", "example"])
def test_pca_on_the_device_engine(engines, which):
    """core.pca: device == host engine == specification on every output, and the device's result against prcomp restated
    over LAPACK's SVD within the tolerance tests/explore_cases.py records"""
    from deseq2_amd import core
    from tests.test_explore_cpu import pca_deviation
    D, H = engines
    A, factors = CS.pca_input(which)
    got, host, spec = core.pca(_transform(D, A), ntop=500), core.pca(_transform(H, A), ntop=500), S.pca(A, 500)
    for key in ("select", "sdev", "x", "percentVar"):
        assert_bits(got[key], spec[key], "%s: device vs spec: %s" % (which, key))
        assert_bits(got[key], host[key], "%s: device vs host engine: %s" % (which, key))
    ref = CS.prcomp_svd(A, got["select"])
    keep = CS.comparable(ref["d"])
    assert 0 in keep and 1 in keep and len(keep) == CS.PCA_COMPARED[which]
    assert pca_deviation(got, ref, keep) <= CS.PCA_TOL[which]


def test_pca_stops_on_a_selected_nan_row_only(engines):
    from deseq2_amd import core
    D, _ = engines
    A = CS.selection_matrix()
    n = A.shape[0]
    t = _transform(D, A)
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        core.pca(t, ntop=n - 2)
    got, want = core.pca(t, ntop=n - 3), S.pca(A, n - 3)
    for key in ("select", "sdev", "x", "percentVar"):
        assert_bits(got[key], want[key], "pca short of the NaN rows: " + key)


def test_plotpca_distances_and_variances_of_a_resident_transform(engines):
    """the public calls on what normTransform / normalized_counts leave resident, against the same calls on the host engine
    over the same values (the transform itself is held to its own specification by tests/test_gpu_vst.py)"""
    from deseq2_amd import core, simulate
    D, H = engines
    m = 12
    x = simulate.design_factor(m, 3)
    d = simulate.make_counts(700, x, seed=5, beta_sd=np.array([2.0, 2.0]))
    factors = {"condition": (np.arange(m) * 3) // m, "batch": np.arange(m) % 2}
    dds = core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=D)
    dds.attrs["factors"] = factors
    for t in (core.normTransform(dds), core.normalized_counts(dds)):
        A = t.assay()
        th = _transform(H, A, factors)
        pd, ph = (core.plotPCA(o, intgroup=["condition", "batch"], pcsToUse=(2, 3)) for o in (t, th))
        assert list(pd) == list(ph) == ["PC2", "PC3", "group", "condition", "batch", "name"]
        for key in ("PC2", "PC3"):
            assert_bits(pd[key], ph[key], key)
        assert list(pd["group"]) == list(ph["group"]) and pd["name"] == ph["name"]
        assert_bits(pd.attrs["percentVar"], ph.attrs["percentVar"], "percentVar")
        assert_bits(core.sampleDists(t), core.sampleDists(th), "sampleDists")
        assert_bits(core.sampleDists(t), S.sample_dists(A), "sampleDists against the specification")
        assert_bits(core.rowVars(t), S.row_vars(A)[1], "rowVars")
    with pytest.raises(ValueError, match="the argument 'intgroup' should specify columns"):
        core.plotPCA(core.normTransform(core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=D)))


def test_host_entries():
    """dsq_top_var / dsq_sample_pairs: host pointers in R layout, staged through the library's own buffers"""
    from deseq2_amd import native
    A = CS.matrix(150, 67, seed=21)
    A[40] = A[41]
    smean, svar = S.row_vars(A)
    r = native.top_var(A, ntop=20)
    assert_bits(r["rowMean"], smean, "rowMean")
    assert_bits(r["rowVar"], svar, "rowVar")
    assert_same(r["select"], S.top_var(svar, 20), "select")
    rows = r["select"]
    assert_bits(native.sample_pairs(A, "gram", rows=rows, centre=smean[rows]), S.pair_sums(A, "gram", rows=rows, centre=smean[rows]), "gram")
    assert_bits(native.sample_pairs(A, "dist"), S.sample_dists(A), "dist")
    assert_bits(native.sample_pairs(A, "dist2"), S.pair_sums(A, "dist2"), "dist2")


# ---------------------------------------------------------------------------------------------- independent statements
def test_device_outputs_against_the_independent_statements():
    """once on the GPU's own outputs: numpy.var in longdouble, scipy's pdist and the longdouble sums, the longdouble Gram"""
    from tests.test_explore_cpu import _check_dist, _check_gram, _check_var, _var_rows
    A = _var_rows(65)
    _check_var(_top_var_dev(A, 0)[1], A, "device")
    B = CS.matrix(1000, 66, seed=1066)
    _check_dist(_pairs_dev(B, "dist"), B, "device")
    G = CS.matrix(600, 10, seed=70)
    mean, var, rows = _top_var_dev(G, 70)
    _check_gram(_pairs_dev(G, "gram", rows=rows, centre=mean[rows]), G, rows, mean, "device")
