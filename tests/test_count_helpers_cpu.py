"""collapseReplicates, colSums, fpm, fpkm, counts and plotCounts on the CPU: the numpy specification
of tests/counts_spec.py is held to statements that share nothing with it (Python-int sums; fractions.Fraction arithmetic
rounded once per operation -- float(Fraction) is correctly rounded --, bit for bit); HostEngine equals the specification
bit for bit; the reference's own expectations (tests/testthat/test_collapse.R, test_fpkm.R, the two roxygen examples of
R/helper.R) are re-run; the object semantics of collapseReplicates, its errors and the overflow rule; counts() and
plotCounts()."""
import math
import warnings
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import counts_spec as S
from tests.helpers import assert_bits

from deseq2_amd import core
from deseq2_amd.engine import HostEngine

I32MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def E():
    return HostEngine(O)


def _counts(n, m, seed, hi=100000):
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, hi, size=(n, m), dtype=np.int32)
    y[rng.random((n, m)) < 0.2] = 0
    return y


def _csr(codes):
    codes = np.asarray(codes)
    g = int(codes.max()) + 1
    return np.argsort(codes, kind="stable"), np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=g))])


# ---------------------------------------------------------------------------------------------- the specification, independently
def test_integer_sums_against_python_ints(E):
    y = _counts(23, 9, seed=1, hi=I32MAX // 5)
    y[3, :] = I32MAX // 5
    members, offsets = _csr([2, 0, 1, 0, 2, 2, 1, 2, 2])
    got, status = S.collapse(y, members, offsets)
    rows = y.tolist()
    for i in range(23):
        for c in range(3):
            assert int(got[i, c]) == sum(rows[i][j] for j in members[offsets[c]:offsets[c + 1]])
    assert status == 0
    big = np.full((1000, 3), I32MAX, dtype=np.int32)
    assert [int(v) for v in S.col_sums(big)] == [1000 * I32MAX] * 3
    assert [int(v) for v in S.col_sums(y)] == [sum(r[j] for r in rows) for j in range(9)]
    h, hs = E.collapse_columns(E.counts(y), members, offsets)
    assert hs == 0 and np.array_equal(np.asarray(h), got) and np.asarray(h).dtype == np.int32
    assert np.array_equal(E.col_sums(E.counts(y)), S.col_sums(y))


def _fpm_fraction(k, lib, kind, length):
    """the three formulas in exact rational arithmetic, rounded once per operation"""
    def op(fr):
        return Fraction(float(fr))
    f = op(Fraction(10 ** 6) * op(Fraction(int(k)) / Fraction(lib)))
    if kind == "fpm":
        return float(f)
    if kind == "fpkm_basepairs":
        return float(op(Fraction(1000) * op(f / Fraction(length))))
    return float(op(op(Fraction(1000) * f) / Fraction(length)))


@pytest.mark.parametrize("kind", ["fpm", "fpkm_basepairs", "fpkm_txlen"])
def test_fpm_kinds_against_rational_arithmetic(E, kind):
    rng = np.random.Generator(np.random.PCG64(2))
    n, m = 31, 5
    y = _counts(n, m, seed=3)
    y[0, 0], y[1, 1] = I32MAX, 1
    lib = rng.uniform(1e4, 3e7, size=m)
    bp = rng.integers(1, 30000, size=n).astype(np.float64)
    tl = rng.uniform(30.0, 8000.0, size=(n, m))
    kw = {"fpm": {}, "fpkm_basepairs": {"basepairs": bp}, "fpkm_txlen": {"txlen": tl}}[kind]
    got = S.fpm(y, lib, kind, **kw)
    want = np.empty((n, m))
    for i in range(n):
        for j in range(m):
            want[i, j] = _fpm_fraction(y[i, j], lib[j], kind, bp[i] if kind == "fpkm_basepairs" else tl[i, j])
    assert_bits(got, want, kind + ": specification against Fraction arithmetic")
    assert_bits(np.asarray(E.fpm_transform(E.counts(y), lib, kind, **{k: (E.matrix(v) if k == "txlen" else v) for k, v in kw.items()})),
                got, kind + ": host engine against the specification")


def test_fpm_edge_values(E):
    y = np.array([[0, 7, 3], [5, 0, I32MAX]], dtype=np.int32)
    lib = np.array([0.0, np.nan, 2.0])
    with np.errstate(all="ignore"):
        f = S.fpm(y, lib, "fpm")
    assert np.isnan(f[0, 0]) and np.isposinf(f[1, 0]) and np.isnan(f[:, 1]).all() and f[0, 2] == 1.5e6
    assert_bits(np.asarray(E.fpm_transform(E.counts(y), lib, "fpm")), f, "edges")
    with np.errstate(all="ignore"):
        k = S.fpm(y, np.array([1.0, 1.0, 1.0]), "fpkm_basepairs", basepairs=np.array([0.0, 2.0]))
    assert np.isnan(k[0, 0]) and np.isposinf(k[0, 1]) and k[1, 0] == 2.5e9


def test_library_sizes(E):
    """sizeFactors * exp(mean(log(colSums))): the specification against libm within a few ulps, core against the
    specification bit for bit; the column sums as double are ONE rounding of the exact sums"""
    sums = np.array([2 ** 53 + 1, 123456789, 987654321012], dtype=np.int64)
    cs = S.as_double(sums)
    assert cs[0] == float(Fraction(2 ** 53 + 1)) == 2.0 ** 53
    sf = np.array([0.5, 1.0, 2.0])
    lib = S.library_sizes(O, sf, sums)
    want = sf * math.exp(sum(math.log(float(v)) for v in cs) / 3)
    np.testing.assert_allclose(lib, want, rtol=1e-14)
    y = _counts(40, 3, seed=4)
    dds = core.DESeqDataSet(y, np.ones((3, 1)), sizeFactors=sf, engine=E)
    assert_bits(core._library_sizes(dds, True), S.library_sizes(O, sf, S.col_sums(y)), "library sizes, robust")
    assert_bits(core._library_sizes(dds, False), S.as_double(S.col_sums(y)), "library sizes, column sums")


# ---------------------------------------------------------------------------------------------- the reference's expectations
def _dds(E, counts, **kw):
    counts = np.asarray(counts)
    return core.DESeqDataSet(counts, np.ones((counts.shape[1], 1)), engine=E, **kw)


def test_testthat_collapse(E):
    """tests/testthat/test_collapse.R"""
    counts = _counts(10, 8, seed=5, hi=500)
    dds = _dds(E, counts)
    dds2 = core.collapseReplicates(dds, np.repeat([1, 2, 3, 4], 2), run=range(1, 9))
    assert np.array_equal(np.asarray(dds2.y)[:, 0], counts[:, 0:2].sum(axis=1))
    assert dds2.attrs["runsCollapsed"][0] == "1,2"
    dds.assays["foobar"] = E.matrix(np.random.Generator(np.random.PCG64(6)).random((10, 8)))
    with pytest.warns(UserWarning, match="only sums"):
        dds3 = core.collapseReplicates(dds, np.repeat([1, 2, 3, 4], 2))
    assert dds3.assays == {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        core.collapseReplicates(_dds(E, counts), np.repeat([1, 2, 3, 4], 2))
    for kw in ({"weights": np.ones((10, 8))}, {"normalizationFactors": np.ones((10, 8))}):
        with pytest.warns(UserWarning, match="only sums"):
            out = core.collapseReplicates(_dds(E, counts, **kw), np.repeat([1, 2, 3, 4], 2))
        assert not out.has_weights and out.sizeFactors is not None and not out._sf_given


def test_testthat_fpkm(E):
    """tests/testthat/test_fpkm.R: matrix(c(1:4, 2 * 1:4), ncol = 2), four rows of 10 bp"""
    dds = _dds(E, np.column_stack([np.arange(1, 5), 2 * np.arange(1, 5)]))
    dds.mcols["basepairs"] = np.full(4, 10.0)
    assert core.fpm(dds, robust=False).assay()[0, 0] == 1e5
    assert abs(core.fpm(dds).assay()[0, 0] - 1e5) / 1e5 < 0.1
    assert abs(core.fpkm(dds).assay()[0, 0] - 1e5 * 100) / 1e7 < 0.1
    assert not dds._sf_given and np.array_equal(dds.sizeFactors, np.ones(2))      # estimated on a copy (:381-383)


def test_roxygen_example_collapse(E):
    """R/helper.R:169-184: twelve samples, nine levels given in scrambled order"""
    counts = _counts(60, 12, seed=7, hi=3000)
    sample = np.array(["sample%d" % v for v in np.repeat(np.arange(1, 10), [2, 1, 1, 2, 1, 1, 2, 1, 1])])
    sample = sample[np.random.Generator(np.random.PCG64(8)).permutation(12)]
    run = ["run%d" % (j + 1) for j in range(12)]
    dds = _dds(E, counts)
    coll = core.collapseReplicates(dds, sample, run)
    assert coll.attrs["colnames"] == sorted(set(sample)) and coll.m == 9
    first = sample == coll.attrs["colnames"][0]
    assert np.array_equal(counts[:, first].sum(axis=1), np.asarray(coll.y)[:, 0])
    assert coll.attrs["runsCollapsed"][0] == ",".join(r for r, f in zip(run, first) if f)


def test_roxygen_example_fpm_fpkm(E):
    """R/helper.R:262-282: 1e6 * rep(c(.125, .25, .25, .5), each = 4), lengths 1, 1, 2 and 0.5 kb"""
    m = (1e6 * np.repeat([.125, .25, .25, .5], 4)).reshape(4, 4, order="F").astype(np.int64)
    dds = _dds(E, m)
    dds.mcols["basepairs"] = np.array([1000.0, 1000.0, 2000.0, 500.0])
    f = core.fpm(dds, robust=False).assay()
    assert np.array_equal(f, np.full((4, 4), 250000.0))               # every column sums to 1e6
    k = core.fpkm(dds, robust=False).assay()
    assert np.array_equal(k, np.repeat([[250000.0], [250000.0], [125000.0], [500000.0]], 4, axis=1))
    # robust: the median-ratio factors of these columns are 0.5, 1, 1, 2 up to rounding, so every entry is the same again
    fr = core.fpm(dds).assay()
    np.testing.assert_allclose(fr, np.full((4, 4), fr[0, 0]), rtol=1e-12)
    assert core.fpm(dds).kind == "fpm" and core.fpkm(dds).kind == "fpkm"


# ---------------------------------------------------------------------------------------------- collapseReplicates: the object
def test_collapse_object_semantics(E):
    counts = _counts(30, 7, seed=9, hi=1000)
    x = np.column_stack([np.ones(7), np.arange(7) % 2])
    sf = np.array([0.5, 0.7, 0.9, 1.1, 1.3, 1.5, 1.7])
    dds = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
    dds.attrs["factors"] = OrderedDict(condition=np.arange(7) % 2, batch=np.arange(7) % 3)
    dds.attrs["colnames"] = list("ABCDEFG")
    dds.mcols["basepairs"] = np.arange(30.0)
    dds.dispersionFunction = {"fitType": "mean", "mean": 0.1}
    groupby = ["k", "b", "k", 10, "b", 9, "k"]              # unsorted, interleaved, numbers among strings
    out = core.collapseReplicates(dds, groupby)
    # as.character() of every label, strings sorted by code point: "10" < "9" < "b" < "k"
    assert out.attrs["colnames"] == ["10", "9", "b", "k"]
    keep = [3, 5, 1, 0]
    want = np.column_stack([counts[:, [3]].sum(1), counts[:, [5]].sum(1), counts[:, [1, 4]].sum(1), counts[:, [0, 2, 6]].sum(1)])
    assert np.array_equal(np.asarray(out.y), want) and (out.n, out.m) == (30, 4)
    assert np.array_equal(out.x, x[keep]) and np.array_equal(out.sizeFactors, sf[keep]) and out._sf_given
    assert_bits(np.asarray(out.nf), np.broadcast_to(sf[keep], (30, 4)), "the normalization factors R builds from them")
    assert list(out.attrs["factors"]) == ["condition", "batch"]
    assert np.array_equal(out.attrs["factors"]["batch"], (np.arange(7) % 3)[keep])
    assert out.mcols["basepairs"] is dds.mcols["basepairs"] and out.dispersionFunction == dds.dispersionFunction
    assert "runsCollapsed" not in out.attrs
    assert core.collapseReplicates(dds, groupby, renameCols=False).attrs["colnames"] == ["D", "F", "B", "A"]
    # numeric labels sort as numbers
    assert core.collapseReplicates(dds, [10, 9, 10, 2.5, 9, 9, 2.5]).attrs["colnames"] == ["2.5", "9", "10"]
    # a factor with levels in its own order, one of them without a sample: droplevels removes it
    out = core.collapseReplicates(dds, ["z", "a", "z", "a", "z", "a", "z"], levels=["z", "unused", "a"])
    assert out.attrs["colnames"] == ["z", "a"] and np.array_equal(np.asarray(out.y)[:, 0], counts[:, [0, 2, 4, 6]].sum(1))
    # no real size factors: none on the result either
    plain = core.collapseReplicates(_dds(E, counts), groupby)
    assert not plain._sf_given and np.array_equal(plain.sizeFactors, np.ones(4))
    # the collapsed object goes on through the workflow
    core.estimateSizeFactors(plain)
    assert plain._sf_given and np.isfinite(plain.sizeFactors).all()


def test_collapse_errors(E):
    counts = _counts(5, 4, seed=10, hi=100)
    dds = _dds(E, counts)
    with pytest.raises(ValueError, match=r"length\(groupby\) == ncol\(object\) is not TRUE"):
        core.collapseReplicates(dds, [1, 2, 3])
    # the length check comes first: a refused call does not also warn about the assays it would have dropped
    extra = _dds(E, counts)
    extra.assays["foobar"] = E.matrix(np.ones((5, 4)))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match=r"length\(groupby\) == ncol\(object\) is not TRUE"):
            core.collapseReplicates(extra, [1, 2, 3])
    with pytest.raises(ValueError, match=r"length\(groupby\) == length\(run\) is not TRUE"):
        core.collapseReplicates(dds, [1, 1, 2, 2], run=[1, 2, 3])
    with pytest.raises(ValueError, match="not among its levels"):
        core.collapseReplicates(dds, ["a", "b", "a", "c"], levels=["a", "b"])


def test_collapse_overflow(E):
    """a group summing to exactly 2^31 - 1 passes, 2^31 raises naming the level"""
    counts = np.full((6, 4), 3, dtype=np.int64)
    counts[4, 0], counts[4, 2] = I32MAX - 9, 9
    out = core.collapseReplicates(_dds(E, counts), ["p", "q", "p", "q"])
    assert int(np.asarray(out.y)[4, 0]) == I32MAX
    counts[4, 2] = 10
    with pytest.raises(ValueError, match="level 'p' exceeds the largest integer"):
        core.collapseReplicates(_dds(E, counts), ["p", "q", "p", "q"])
    y = E.counts(counts)
    members, offsets = _csr([0, 1, 0, 1])
    assert S.collapse(counts, members, offsets)[1] == 1 and E.collapse_columns(y, members, offsets)[1] == 1
    assert E.collapse_overflow_group(y, members, offsets) == 0


def test_collapse_closing_check_guards_the_sums(E, monkeypatch):
    """the closing stopifnot of R/helper.R:214 is made for real: an engine whose group sums lose a count is refused"""
    counts = _counts(8, 4, seed=11, hi=100) + 1
    honest = E.collapse_columns

    def lossy(y, members, offsets):
        h, s = honest(y, members, offsets)
        h = np.array(h, copy=True, order="F")
        h[3, 1] -= 1
        return h, s
    monkeypatch.setattr(E, "collapse_columns", lossy)
    with pytest.raises(ValueError, match=r"sum\(as.numeric\(assay\(object\)\)\) == sum\(as.numeric\(assay\(collapsed\)\)\) is not TRUE"):
        core.collapseReplicates(_dds(E, counts), [1, 1, 2, 2])


# ---------------------------------------------------------------------------------------------- fpkm, counts, plotCounts
def test_fpkm_lengths(E):
    counts = _counts(50, 6, seed=12) + 1
    dds = _dds(E, counts, sizeFactors=np.linspace(0.6, 1.6, 6))
    with pytest.raises(ValueError, match=r'mcols\["basepairs"\]'):
        core.fpkm(dds)
    rng = np.random.Generator(np.random.PCG64(13))
    bp, tl = rng.integers(100, 5000, size=50).astype(float), rng.uniform(100.0, 4000.0, size=(50, 6))
    dds.mcols["basepairs"] = bp
    lib = S.library_sizes(O, dds.sizeFactors, S.col_sums(counts))
    assert_bits(core.fpkm(dds).assay(), S.fpm(counts, lib, "fpkm_basepairs", basepairs=bp), "fpkm, basepairs, robust")
    assert_bits(core.fpm(dds).assay(), S.fpm(counts, lib, "fpm"), "fpm, robust")
    dds.assays["avgTxLength"] = E.matrix(tl)                          # takes precedence; the library sizes are the column sums
    cs = S.as_double(S.col_sums(counts))
    assert_bits(core.fpm(dds).assay(), S.fpm(counts, cs, "fpm"), "fpm with avgTxLength: not robust")
    assert_bits(core.fpkm(dds, robust=False).assay(), S.fpm(counts, cs, "fpkm_txlen", txlen=tl), "fpkm, avgTxLength")
    want, _ = S.fpkm_txlen_robust(O, counts, tl)
    np.testing.assert_allclose(core.fpkm(dds).assay(), want, rtol=1e-12)        # (HostEngine.size_factors: libm, equal to rounding)


def test_counts_accessor(E):
    counts = _counts(20, 5, seed=14)
    sf = np.array([0.5, 1.0, 2.0, 4.0, 0.25])
    dds = _dds(E, counts, sizeFactors=sf)
    assert np.array_equal(core.counts(dds).assay(), counts)
    assert_bits(core.counts(dds, normalized=True).assay(), counts / sf[None, :], "normalized")
    with pytest.warns(UserWarning, match="there are no assays named 'replaceCounts', using original.\ncalling DESeq\\(\\) will replace"):
        assert np.array_equal(core.counts(dds, replaced=True).assay(), counts)
    rep = counts.copy()
    rep[2, 3] = 77
    dds.assays["replaceCounts"] = E.counts(rep)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.array_equal(core.counts(dds, replaced=True).assay(), rep)
        assert_bits(core.counts(dds, normalized=True, replaced=True).assay(), rep / sf[None, :], "normalized, replaced")
    assert np.array_equal(core.counts(dds).assay(), counts)
    with pytest.raises(ValueError, match="first calculate size factors, add normalizationFactors, or set normalized=FALSE"):
        core.counts(_dds(E, counts), normalized=True)
    with pytest.raises(ValueError, match="first calculate size factors"):
        core.counts(_dds(E, counts, sizeFactors=np.array([1.0, np.nan, 1.0, 1.0, 1.0])), normalized=True)
    nf = np.random.Generator(np.random.PCG64(15)).uniform(0.5, 2.0, size=(20, 5))
    assert_bits(core.counts(_dds(E, counts, normalizationFactors=nf), normalized=True).assay(), counts / nf, "normalization factors")


def test_plot_counts(E):
    counts = _counts(20, 6, seed=16) + 1
    sf = np.array([0.5, 1.0, 2.0, 4.0, 0.25, 1.5])
    dds = _dds(E, counts, sizeFactors=sf)
    dds.attrs["factors"] = OrderedDict(condition=np.arange(6) % 2, batch=np.arange(6) % 3)
    d = core.plotCounts(dds, 7)
    assert list(d) == ["count", "condition"]
    assert_bits(d["count"], core.counts(dds, normalized=True).assay()[7] + 0.5, "count")
    d = core.plotCounts(dds, 19, intgroup=["batch", "condition"], normalized=False, transform=False)
    assert list(d) == ["count", "batch", "condition"] and np.array_equal(d["count"], counts[19].astype(float))
    assert_bits(core.plotCounts(dds, 0, pc=3)["count"], counts[0] / sf + 3, "pc given")
    for gene in (-1, 20, "gene1", 1.5):
        with pytest.raises(ValueError, match="gene >= 1 & gene <= nrow"):
            core.plotCounts(dds, gene)
    with pytest.raises(ValueError, match="all variables in 'intgroup' must be columns of colData"):
        core.plotCounts(dds, 0, intgroup="genotype")
    with pytest.raises(NotImplementedError):
        core.plotCounts(dds, 0, returnData=False)
    # without size factors they are estimated on a copy (R/plots.R:385-387)
    plain = _dds(E, counts)
    plain.attrs["factors"] = dds.attrs["factors"]
    est = core.estimateSizeFactors(_dds(E, counts)).sizeFactors
    assert_bits(core.plotCounts(plain, 4)["count"], counts[4] / est + 0.5, "estimated size factors")
    assert not plain._sf_given
    rep = counts.copy()
    rep[4, 1] = 999
    dds.assays["replaceCounts"] = E.counts(rep)
    assert_bits(core.plotCounts(dds, 4, replaced=True)["count"], rep[4] / sf + 0.5, "replaced")


# ---------------------------------------------------------------------------------------------- the C ABI's refusals
def test_capi_refusals_before_a_device_is_asked_for():
    import ctypes as C
    from deseq2_amd import _lib as L
    lib = L.lib()
    y = np.zeros((4, 3), dtype=np.int32, order="F")
    mem, off = np.arange(3, dtype=np.int32), np.array([0, 1, 3], dtype=np.int32)
    out = np.zeros((4, 3), dtype=np.int32, order="F")
    f64 = np.zeros((4, 3), order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)       # noqa: E731

    def collapse(**kw):
        d = dict(n=4, m=3, g=2, ld=0, y=p(y), members=p(mem), offsets=p(off))
        d.update(kw)
        return lib.dsq_collapse(C.byref(L.sized(L.DsqCollapseArgs, **d)), C.byref(L.sized(L.DsqCollapseOut, ld=0, out=p(out), status=None)))
    for kw in ({"n": 0}, {"m": 0}, {"g": 0}, {"g": 4}, {"y": None}, {"members": None}, {"offsets": None}):
        assert collapse(**kw) == L.DSQ_ERR_ARG, kw
    a = L.DsqCollapseArgs(struct_size=4, n=4, m=3, g=2, y=p(y), members=p(mem), offsets=p(off))
    assert lib.dsq_collapse(C.byref(a), C.byref(L.sized(L.DsqCollapseOut, out=p(out)))) == L.DSQ_ERR_ARG
    sums = np.zeros(3, dtype=np.int64)
    for kw in ({"n": 0}, {"y": None}):
        d = dict(n=4, m=3, ld=0, y=p(y))
        d.update(kw)
        assert lib.dsq_col_sums(C.byref(L.sized(L.DsqColSumsArgs, **d)), C.byref(L.sized(L.DsqColSumsOut, sums=p(sums)))) == L.DSQ_ERR_ARG
    assert lib.dsq_col_sums(C.byref(L.sized(L.DsqColSumsArgs, n=4, m=3, ld=0, y=p(y))), C.byref(L.sized(L.DsqColSumsOut, sums=None))) == L.DSQ_ERR_ARG
    libsz = np.ones(3)
    for kw in ({"kind": 3}, {"kind": 1}, {"kind": 2}, {"lib": None}, {"m": 0}):
        d = dict(n=4, m=3, ld=0, y=p(y), kind=0, lib=p(libsz), basepairs=None, txlen=None)
        d.update(kw)
        assert lib.dsq_fpm(C.byref(L.sized(L.DsqFpmArgs, **d)), C.byref(L.sized(L.DsqFpmOut, out=p(f64)))) == L.DSQ_ERR_ARG, kw
    st = C.c_void_p(None)
    a = L.sized(L.DsqFpmArgs, n=4, m=3, ld=2, y=p(y), kind=0, lib=p(libsz))
    assert lib.dsq_fpm_dev(C.byref(a), C.byref(L.sized(L.DsqFpmOut, out=p(f64))), st) == L.DSQ_ERR_ARG          # ld < m
    a = L.sized(L.DsqCollapseArgs, n=4, m=3, g=2, ld=3, y=p(y), members=p(mem), offsets=p(off))
    assert lib.dsq_collapse_dev(C.byref(a), C.byref(L.sized(L.DsqCollapseOut, ld=1, out=p(out), status=p(out))), st) == L.DSQ_ERR_ARG
    assert lib.dsq_collapse_dev(C.byref(a), C.byref(L.sized(L.DsqCollapseOut, ld=2, out=p(out), status=None)), st) == L.DSQ_ERR_ARG
