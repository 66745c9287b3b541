"""Sample PCA and sample distances on the CPU: HostEngine's row_vars / top_var / pair_sums equal the
numpy specification of tests/explore_spec.py BIT FOR BIT; the specification and the host engine are held to statements that
share nothing with them (numpy.var and sums in longdouble, scipy's pdist, prcomp restated over LAPACK's SVD) within bounds
that are derived, not measured; four mutations of the specification are refused by those same comparisons; plotPCA's
return value and checks; the C ABI's refusals (decided before a device is asked for)."""
import ctypes as C

import numpy as np
import pytest

from tests import explore_cases as CS
from tests import explore_spec as S
from tests.helpers import assert_bits, assert_same

from deseq2_amd import core, explore_host
from deseq2_amd.engine import HostEngine


@pytest.fixture(scope="module")
def E():
    return HostEngine()


class _Obj:
    """the object a transform came from, as far as the exploration functions look at it"""

    def __init__(self, engine, factors=None):
        self.engine, self.attrs = engine, ({"factors": factors} if factors else {})


def _transform(E, A, factors=None):
    return core.DESeqTransform(_Obj(E, factors), E.matrix(A), "vst")


# ---------------------------------------------------------------------------------------------- bitwise: host engine == spec
@pytest.mark.parametrize("m", CS.M_LIST + (513, 600))
def test_row_vars_equal_the_specification(E, m):
    A = CS.matrix(37, m, seed=m)
    A[5] = 2.5
    A[9, m // 2] = np.nan
    mean, var = E.row_vars(E.matrix(A))
    smean, svar = S.row_vars(A)
    assert_bits(mean, smean, "rowMean")
    assert_bits(var, svar, "rowVar")
    assert var[5] == 0.0 and np.isnan(var[9])


@pytest.mark.parametrize("m", CS.M_LIST)
@pytest.mark.parametrize("kind", ["dist2", "gram"])
def test_pair_sums_equal_the_specification_over_m(E, m, kind):
    A = CS.matrix(CS.L + 5, m, seed=100 + m)
    centre = S.row_vars(A)[0] if kind == "gram" else None
    got = E.pair_sums(E.matrix(A), kind, centre=centre)
    assert_bits(got, S.pair_sums(A, kind, centre=centre), "%s, m = %d" % (kind, m))
    assert_bits(got, got.T, "symmetric")


@pytest.mark.parametrize("R", CS.ROWS_SUMMED)
def test_pair_sums_equal_the_specification_over_the_rows_summed(E, R):
    A = CS.matrix(R, 65, seed=R)
    assert S.slice_length(R, 65) == CS.L == explore_host.slice_rows(R, 65)
    mean = S.row_vars(A)[0]
    assert_bits(E.pair_sums(E.matrix(A), "dist2"), S.pair_sums(A, "dist2"), "dist2, %d rows" % R)
    assert_bits(E.pair_sums(E.matrix(A), "dist"), S.sample_dists(A), "dist, %d rows" % R)
    assert_bits(E.pair_sums(E.matrix(A), "gram", centre=mean), S.pair_sums(A, "gram", centre=mean), "gram, %d rows" % R)


@pytest.mark.parametrize("which", ["single", "all", "permutation", "repeated"])
def test_pair_sums_over_a_row_list(E, which):
    A = CS.matrix(90, 7, seed=3)
    rows = CS.row_lists(90, seed=4)[which]
    centre = S.row_vars(A)[0][rows]
    for kind, c in (("dist2", None), ("gram", centre)):
        assert_bits(E.pair_sums(E.matrix(A), kind, rows=rows, centre=c), S.pair_sums(A, kind, rows=rows, centre=c),
                    "%s over %s" % (kind, which))


def test_the_slice_rule():
    """a function of (rows summed, m) alone: one tile of pairs is cut into up to WORK slices of at least LMIN rows; at
    m = 2000 (528 tiles) three slices, i.e. 1584 tiles of partial sums (52 MB)"""
    for R, m, want in ((1, 2, 64), (20000, 48, 64), (60000, 48, 64), (200000, 48, 98), (500, 500, 64), (60000, 2000, 20000),
                       (60000, 129, 176), (60000, 9000, 60000)):
        assert S.slice_length(R, m) == explore_host.slice_rows(R, m) == want, (R, m)


def test_a_nan_spreads_over_the_pairs_of_its_sample(E):
    A = CS.matrix(70, 5, seed=8)
    A[11, 3] = np.nan
    d = E.pair_sums(E.matrix(A), "dist")
    assert_bits(d, S.sample_dists(A), "dist with a NaN")
    off = ~np.eye(5, dtype=bool)
    assert np.isnan(d[3][off[3]]).all() and np.isnan(d[:, 3][off[3]]).all() and np.isfinite(np.delete(np.delete(d, 3, 0), 3, 1)).all()
    assert (np.diag(d) == 0).all() and not np.signbit(np.diag(d)).any()


# ---------------------------------------------------------------------------------------------- the selection
def test_the_order_of_the_selection(E):
    A = CS.selection_matrix()
    n = A.shape[0]
    _, rv = S.row_vars(A)
    assert rv[3] == rv[7] == rv[21] and rv[10] == rv[11] == 0 and np.isnan(rv[[15, 16, n - 1]]).all()
    want = CS.lexsort_order(rv)
    assert list(want[-3:]) == [15, 16, n - 1] and list(want[-5:-3]) == [10, 11]
    for ntop in (1, n - 1, n, n + 10):
        k = min(ntop, n)
        assert_same(S.top_var(rv, ntop), want[:k], "spec order, ntop = %d" % ntop)
        tv = E.top_var(E.matrix(A), ntop)
        assert_same(tv["select"], want[:k], "host engine order, ntop = %d" % ntop)
        assert_bits(tv["selVar"], rv[want[:k]], "variances of the selection")
    t = _transform(E, A)
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        core.pca(t, ntop=n - 2)
    with pytest.raises(ValueError, match="infinite or missing values in 'x'"):
        S.pca(A, n - 2)
    got, want = core.pca(t, ntop=n - 3), S.pca(A, n - 3)
    for key in ("select", "sdev", "x", "percentVar"):
        assert_bits(got[key], want[key], "pca short of the NaN rows: " + key)


# ---------------------------------------------------------------------------------------------- independent statements
def _var_rows(m):
    """rows of one sign with a coefficient of variation above 1e-3, and two constant rows"""
    A = CS.matrix(300, m, seed=50 + m)
    A[17] = 6.25
    A[18] = 1e-3
    return A


def _check_var(var, A, what):
    m = A.shape[1]
    exact = CS.var_longdouble(A)
    const = np.array([17, 18])
    assert (var[const] == 0).all(), what
    rest = np.setdiff1d(np.arange(A.shape[0]), const)
    rel = np.abs((var[rest].astype(np.longdouble) - exact[rest]) / exact[rest]).astype(np.float64)
    print("%s: m = %d, max relative error %.3g (bound %.3g)" % (what, m, rel.max(), CS.var_bound(m)))
    assert rel.max() <= CS.var_bound(m), what


@pytest.mark.parametrize("m", [2, 3, 12, 65, 200])
def test_row_variances_against_longdouble(E, m):
    A = _var_rows(m)
    _check_var(S.row_vars(A)[1], A, "spec")
    _check_var(E.row_vars(E.matrix(A))[1], A, "host engine")


def _check_dist(d, A, what):
    from scipy.spatial.distance import pdist, squareform
    R = A.shape[0]
    exact = CS.dist_longdouble(A)
    off = ~np.eye(A.shape[1], dtype=bool)
    rel = np.abs((d.astype(np.longdouble) - exact)[off] / exact[off]).astype(np.float64)
    print("%s: %d rows, max relative error against longdouble %.3g (bound %.3g)" % (what, R, rel.max(), CS.dist_bound(R)))
    assert rel.max() <= CS.dist_bound(R), what
    sp = squareform(pdist(A.T))
    rel = np.abs(d - sp)[off] / sp[off]
    assert rel.max() <= CS.dist_bound(R), what + " against scipy"
    assert (np.diag(d) == 0).all()


@pytest.mark.parametrize("n,m", [(1, 3), (200, 9), (1000, 66)])
def test_distances_against_scipy_and_longdouble(E, n, m):
    A = CS.matrix(n, m, seed=n + m)
    _check_dist(S.sample_dists(A), A, "spec")
    _check_dist(E.pair_sums(E.matrix(A), "dist"), A, "host engine")


def _check_gram(G, A, rows, mean, what):
    C_ = A[rows] - mean[rows][:, None]
    exact, scale = CS.gram_longdouble(C_)
    err = np.abs(G.astype(np.longdouble) - exact).astype(np.float64)
    bound = CS.gram_bound(len(rows)) * scale.astype(np.float64)
    print("%s: k = %d, max error / bound %.3g" % (what, len(rows), (err / bound).max()))
    assert (err <= bound).all(), what


@pytest.mark.parametrize("k", [1, 70, 500])
def test_gram_against_longdouble(E, k):
    A = CS.matrix(600, 10, seed=k)
    mean, var = S.row_vars(A)
    rows = S.top_var(var, k)
    _check_gram(S.pair_sums(A, "gram", rows=rows, centre=mean[rows]), A, rows, mean, "spec")
    _check_gram(E.pair_sums(E.matrix(A), "gram", rows=rows, centre=mean[rows]), A, rows, mean, "host engine")


def pca_deviation(got, ref, keep):
    """the largest relative deviation over the comparable components: sdev and percentVar per component, the scores of a
    component against the largest score of that component"""
    keep = np.asarray(keep)
    dev = [np.abs(got["sdev"][keep] - ref["sdev"][keep]) / ref["sdev"][keep],
           np.abs(got["percentVar"][keep] - ref["percentVar"][keep]) / ref["percentVar"][keep],
           np.abs(got["x"][:, keep] - ref["x"][:, keep]).max(axis=0) / np.abs(ref["x"][:, keep]).max(axis=0)]
    return float(np.max(np.concatenate(dev)))


@pytest.mark.parametrize("which", ["planted", "example"])
def test_pca_against_prcomp_over_the_svd(E, which):
    A, factors = CS.pca_input(which)
    got = core.pca(_transform(E, A), ntop=500)
    spec = S.pca(A, 500)
    for key in ("select", "sdev", "x", "percentVar"):
        assert_bits(got[key], spec[key], "%s: host engine vs spec: %s" % (which, key))
    ref = CS.prcomp_svd(A, got["select"])
    keep = CS.comparable(ref["d"])
    dev = pca_deviation(got, ref, keep)
    print("%s: %d of %d components compared %s, deviation %.3g (recorded %.3g, tolerance %.3g)"
          % (which, len(keep), ref["d"].size, keep, dev, CS.PCA_MEASURED[which], CS.PCA_TOL[which]))
    assert 0 in keep and 1 in keep, "pcsToUse = (1, 2) must be among the components compared"
    assert len(keep) == CS.PCA_COMPARED[which]
    assert dev <= CS.PCA_TOL[which]
    assert abs(got["percentVar"].sum() - 1) < 1e-12 and (np.diff(got["sdev"]) <= 0).all()
    top = np.argmax(np.abs(got["x"]), axis=0)
    lead = got["x"][top, np.arange(got["x"].shape[1])]
    assert (lead[keep] > 0).all() and (lead >= 0).all()            # (a clipped eigenvalue leaves a column of zeros)


# ---------------------------------------------------------------------------------------------- mutations
def test_mutations_are_refused(E):
    """what the comparisons above must not let pass"""
    # a variance divided by m
    A = _var_rows(12)
    with pytest.raises(AssertionError):
        _check_var(S.row_vars(A)[1] * (11.0 / 12.0), A, "variance / m")
    # a selection with ties broken by descending index
    B = CS.selection_matrix()
    rv = S.row_vars(B)[1]
    idx = np.arange(rv.size)
    nan = np.isnan(rv)
    mutant = np.lexsort((-idx, np.where(nan, np.inf, -rv), nan))
    with pytest.raises(AssertionError):
        assert_same(mutant, CS.lexsort_order(rv), "ties by descending index")
    # a Gram without the centring
    G = CS.matrix(600, 10, seed=70)
    mean, var = S.row_vars(G)
    rows = S.top_var(var, 70)
    with pytest.raises(AssertionError):
        _check_gram(S.pair_sums(G, "gram", rows=rows), G, rows, mean, "no centring")
    # a dist2 that skips the last slice
    D = CS.matrix(200, 9, seed=209)
    with pytest.raises(AssertionError):
        _check_dist(np.sqrt(S.pair_sums(D, "dist2", _skip_last_slice=True)), D, "last slice skipped")
    with pytest.raises(AssertionError):
        assert_bits(S.pair_sums(D, "dist2", _skip_last_slice=True), E.pair_sums(E.matrix(D), "dist2"), "last slice skipped")


# ---------------------------------------------------------------------------------------------- plotPCA
def test_plotpca_returns_the_data_frame_of_r(E, capfd):
    A, factors = CS.pca_input("planted")
    t = _transform(E, A, factors)
    p = core.pca(t, ntop=500)
    capfd.readouterr()
    d = core.plotPCA(t)
    assert "using ntop=500 top features by variance" in capfd.readouterr().err
    assert list(d) == ["PC1", "PC2", "group", "condition", "name"]
    assert_bits(d["PC1"], p["x"][:, 0], "PC1")
    assert_bits(d["PC2"], p["x"][:, 1], "PC2")
    assert_bits(d.attrs["percentVar"], p["percentVar"][:2], "percentVar")
    assert_same(d["group"], factors["condition"], "group")
    assert_same(d["condition"], factors["condition"], "condition")
    assert d["name"] == ["sample%d" % (j + 1) for j in range(A.shape[1])]
    # the three planted groups separate on the first two components
    g = np.asarray(factors["condition"])
    centres = np.array([[d["PC1"][g == c].mean(), d["PC2"][g == c].mean()] for c in range(3)])
    spread = max(np.hypot(d["PC1"][g == c] - centres[c, 0], d["PC2"][g == c] - centres[c, 1]).max() for c in range(3))
    assert min(np.hypot(*(centres[a] - centres[b])) for a, b in ((0, 1), (0, 2), (1, 2))) > 2 * spread
    two = core.plotPCA(t, intgroup=["condition", "batch"], pcsToUse=(2, 3))
    assert list(two) == ["PC2", "PC3", "group", "condition", "batch", "name"]
    assert list(two["group"]) == ["%d:%d" % (a, b) for a, b in zip(factors["condition"], factors["batch"])]
    assert_bits(two["PC3"], p["x"][:, 2], "PC3")
    assert_bits(two.attrs["percentVar"], p["percentVar"][1:3], "percentVar of (2, 3)")
    with pytest.raises(ValueError, match="the argument 'intgroup' should specify columns of colData\\(dds\\)"):
        core.plotPCA(t, intgroup="foo")
    with pytest.raises(ValueError, match="pcsToUse"):
        core.plotPCA(t, pcsToUse=(1, 13))
    with pytest.raises(ValueError, match="pcsToUse"):
        core.plotPCA(t, pcsToUse=(1, 2, 3))
    with pytest.raises(NotImplementedError):
        core.plotPCA(t, returnData=False)
    with pytest.raises(ValueError, match="ntop"):
        core.pca(t, ntop=0)
    assert_bits(core.rowVars(t), S.row_vars(A)[1], "rowVars")
    assert_bits(core.sampleDists(t), S.sample_dists(A), "sampleDists")
    import deseq2_amd
    for name in ("rowVars", "sampleDists", "pca", "plotPCA"):
        assert getattr(deseq2_amd, name) is getattr(core, name)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_the_entry_points_check_their_arguments():
    """dsq_top_var[_dev] / dsq_sample_pairs[_dev] decide their argument errors before a device is asked for (1 = DSQ_ERR_ARG)
    and launch nothing"""
    from deseq2_amd import _lib as L
    lib = L.lib()
    n, m = 5, 3
    x = np.asfortranarray(CS.matrix(n, m, seed=1))
    mean, var, sel, out = np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros((m, m))
    rows = np.array([0, 4, 2], np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def targs(**kw):
        d = dict(n=n, m=m, ld=8, x=P(x), ntop=2)
        d.update(kw)
        return L.sized(L.DsqTopVarArgs, **d)

    def pargs(**kw):
        d = dict(n=n, m=m, ld=8, x=P(x), kind=0, nrows=3, rows=P(rows), centre=None)
        d.update(kw)
        return L.sized(L.DsqSamplePairsArgs, **d)

    tout = L.sized(L.DsqTopVarOut, rowMean=P(mean), rowVar=P(var), select=P(sel))
    pout = L.sized(L.DsqSamplePairsOut, out=P(out))
    tops = (lambda a, o=tout: lib.dsq_top_var(C.byref(a), C.byref(o)), lambda a, o=tout: lib.dsq_top_var_dev(C.byref(a), C.byref(o), None))
    pairs = (lambda a, o=pout: lib.dsq_sample_pairs(C.byref(a), C.byref(o)),
             lambda a, o=pout: lib.dsq_sample_pairs_dev(C.byref(a), C.byref(o), None))
    for call in tops:
        assert call(targs(m=1)) == 1 and b"at least two" in lib.dsq_last_error()
        assert call(targs(n=0)) == 1 and call(targs(x=None)) == 1 and call(targs(ntop=-1)) == 1
        assert call(targs(), L.sized(L.DsqTopVarOut, rowMean=None, rowVar=P(var), select=P(sel))) == 1 and b"NULL output" in lib.dsq_last_error()
        assert call(targs(), L.sized(L.DsqTopVarOut, rowMean=P(mean), rowVar=P(var), select=None)) == 1
        bad = targs()
        bad.struct_size -= 4
        assert call(bad) == 1 and b"struct_size" in lib.dsq_last_error()
    for call in pairs:
        assert call(pargs(m=1)) == 1 and b"at least two" in lib.dsq_last_error()
        assert call(pargs(n=0)) == 1 and call(pargs(x=None)) == 1 and call(pargs(kind=3)) == 1
        assert call(pargs(nrows=0)) == 1 and call(pargs(rows=None, nrows=2)) == 1 and b"nrows" in lib.dsq_last_error()
        assert call(pargs(), L.sized(L.DsqSamplePairsOut, out=None)) == 1 and b"NULL output" in lib.dsq_last_error()
        bad = pargs()
        bad.struct_size += 8
        assert call(bad) == 1 and b"struct_size" in lib.dsq_last_error()
    assert tops[1](targs(ld=2)) == 1 and b"ld" in lib.dsq_last_error()
    assert pairs[1](pargs(ld=2)) == 1 and b"ld" in lib.dsq_last_error()
    for r in (n, -1):
        rows[1] = r
        assert pairs[0](pargs()) == 1 and b"outside" in lib.dsq_last_error()
    assert (out == 0).all() and (mean == 0).all() and (sel == 0).all()          # nothing was written
    assert lib.dsq_sample_pairs_slice_rows(60000, 2000) == 20000 and lib.dsq_sample_pairs_slice_rows(1, 2) == 64
    assert lib.dsq_sample_pairs_slice_rows(0, 5) == 0 and lib.dsq_row_vars_register_width() == 512
