"""estimateSizeFactors without a GPU: the host statement (HostEngine.size_factors, core.estimateSizeFactors) against the
numpy specification of tests/sf_spec.py, tests/testthat/test_size_factor.R restated, and DESeq(sfType=...) on the oracle engine."""

import numpy as np
import pytest

from tests import sf_spec


def _counts(n, m, seed, zeros=0.1):
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.normal(6, 2, (n, 1)) * np.exp(rng.normal(0, 0.4, m))[None, :]
    k = rng.poisson(mu).astype(np.int64)
    k[rng.uniform(size=k.shape) < zeros] = 0
    return np.minimum(k, 2 ** 31 - 1).astype(np.int32)


def _tol(m, counts):
    """HostEngine.size_factors and the specification differ in libm's log / exp against the oracle's (an ulp each) and in the
    order of the m-term row sum; a difference d_ij carries at most (m + 2) roundings of magnitude |log k| <= log(max count),
    the median is 1-Lipschitz in the sup norm, exp turns the absolute error of the median into a relative one of the
    factor, and the stabilisation adds a handful more: relative (m + 8) * 2^-52 * max(1, log(max count))."""
    return (m + 8) * 2.0 ** -52 * max(1.0, float(np.log(np.max(counts))))


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
        idx = rng.choice(n, n // 3, replace=False)
        kw["controlGenes"] = idx
        mask = np.zeros(n, bool); mask[idx] = True
    if mode == "control_logical":
        mask = rng.uniform(size=n) < 0.5
        kw["controlGenes"] = mask
    if mode.startswith("normMatrix"):
        kw["normMatrix"] = np.exp(rng.normal(0, 0.3, (n, m)))
    return kw, mask


def _spec(O, k, kw, mask):
    return sf_spec.size_factors(O, k, type=kw.get("type", "ratio"), geoMeans=kw.get("geoMeans"), control=mask,
                                normMatrix=kw.get("normMatrix"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(300, 6), (500, 70)])
def test_host_engine_and_core_match_the_specification(oracle, mode, shape):
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine, control_flags
    n, m = shape
    k = _counts(n, m, seed=n + m, zeros=0.1 if mode in ("poscounts", "geoMeans", "normMatrix_poscounts") else 0.01)   # ("ratio" needs genes without a zero)
    kw, mask = _mode_args(mode, k, n)
    ref = _spec(oracle, k, kw, mask)
    assert ref["status"] == 0 and np.isfinite(ref["sizeFactors"]).all()
    tol = _tol(m, k)
    E = HostEngine(oracle)
    got = E.size_factors(E.counts(k), type=kw.get("type", "ratio"), geoMeans=kw.get("geoMeans"),
                         control=control_flags(kw.get("controlGenes"), n), normMatrix=kw.get("normMatrix"))
    np.testing.assert_allclose(got["sizeFactors"], ref["sizeFactors"], rtol=tol, atol=0)
    x = np.ones((m, 1))
    dds = core.DESeqDataSet(k, x, engine=E)
    core.estimateSizeFactors(dds, **kw)
    if "normMatrix" in kw:
        assert dds.sizeFactors is None
        np.testing.assert_allclose(np.asarray(dds.nf), ref["normalizationFactors"], rtol=2 * tol, atol=0)
        np.testing.assert_allclose(got["normalizationFactors"], ref["normalizationFactors"], rtol=2 * tol, atol=0)
    else:
        np.testing.assert_allclose(dds.sizeFactors, ref["sizeFactors"], rtol=tol, atol=0)
        np.testing.assert_array_equal(np.asarray(dds.nf), np.broadcast_to(dds.sizeFactors[None, :], k.shape))
        sf2 = core.estimateSizeFactorsForMatrix(E, E.counts(k), **kw)
        np.testing.assert_array_equal(sf2, dds.sizeFactors)


def test_empty_selection_is_nan_and_both_median_branches_occur(oracle):
    """A sample without a positive count selects nothing: its median is NA.  In the reference that sample can only be
    seen on the geoMeans / poscounts path ("ratio" stops: every gene then has a zero), where the closing division by
    exp(mean(log(sf))) spreads the NA over every sample (R/core.R:575) -- so the whole vector is NaN, as in R."""
    from deseq2_amd.engine import HostEngine
    E = HostEngine(oracle)
    k = _counts(201, 8, seed=5, zeros=0.0)
    k[0, 5] = 0                     # one sample selects 200 differences, the others 201
    gm = np.exp(np.log(np.maximum(k, 1)).mean(axis=1))
    ref = sf_spec.size_factors(oracle, k, geoMeans=gm)
    assert set(ref["counts_selected"] % 2) == {0, 1}
    np.testing.assert_allclose(E.size_factors(k, geoMeans=gm)["sizeFactors"], ref["sizeFactors"], rtol=_tol(8, k), atol=0)
    k[:, 3] = 0
    for kw in (dict(geoMeans=gm), dict(type="poscounts")):
        ref = sf_spec.size_factors(oracle, k, **kw)
        assert ref["counts_selected"][3] == 0 and np.isnan(ref["sizeFactors"]).all()
        assert np.isnan(E.size_factors(k, **kw)["sizeFactors"]).all()
    assert sf_spec.size_factors(oracle, k)["status"] == 1
    with pytest.raises(ValueError, match="every gene contains at least one zero"):
        E.size_factors(k)


def test_testthat_size_factor_errors_and_calls(oracle):
    """tests/testthat/test_size_factor.R:5-10 on matrix(1:16, ncol = 4)"""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    E = HostEngine(oracle)
    mat = np.arange(1, 17).reshape(4, 4, order="F")
    y = E.counts(mat)
    with pytest.raises(ValueError, match="geoMeans should be as long"):
        core.estimateSizeFactorsForMatrix(E, y, geoMeans=np.arange(1, 6))
    with pytest.raises(ValueError, match="every gene contains at least one zero"):
        core.estimateSizeFactorsForMatrix(E, y, geoMeans=np.zeros(4))
    with pytest.raises(ValueError, match="numeric or logical"):
        core.estimateSizeFactorsForMatrix(E, y, controlGenes="foo")
    assert np.isfinite(core.estimateSizeFactorsForMatrix(E, y, geoMeans=np.arange(1, 5))).all()
    assert np.isfinite(core.estimateSizeFactorsForMatrix(E, y, controlGenes=[0, 1])).all()
    with pytest.raises(NotImplementedError, match="f4"):
        core.estimateSizeFactorsForMatrix(E, y, type="iterate")
    dds = core.DESeqDataSet(mat, np.ones((4, 1)), engine=E)
    with pytest.raises(NotImplementedError, match="f4"):
        core.estimateSizeFactors(dds, type="iterate")


def test_testthat_norm_matrix(oracle):
    """test_size_factor.R:12-18: (normalizationFactors / nm)[1, ] == true.sf at expect_equal's tolerance"""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    mat = np.arange(1, 17).reshape(4, 4, order="F").astype(float)
    nm = mat / np.exp(np.log(mat).mean(axis=1))[:, None]
    true_sf = np.array([2, 1, 1, .5])
    counts = (2 * mat * true_sf[None, :]).astype(np.int64)
    dds = core.DESeqDataSet(counts, np.ones((4, 1)), engine=HostEngine(oracle))
    core.estimateSizeFactors(dds, normMatrix=nm)
    got = (np.asarray(dds.nf) / nm)[0]
    print("normMatrix case: max |nf / nm - true.sf| =", np.abs(got - true_sf).max())
    np.testing.assert_allclose(got, true_sf, rtol=1.5e-8, atol=0)
    ref = sf_spec.size_factors(oracle, counts, normMatrix=nm)["normalizationFactors"]
    np.testing.assert_allclose((ref / nm)[0], true_sf, rtol=1.5e-8, atol=0)


def _poscounts_case(seed=1):
    rng = np.random.default_rng(seed)
    true_sf = 2.0 ** np.repeat([-2, -1, 0, 0, 1, 2], 2)
    n, m = 100, 12
    mean = 2.0 ** rng.normal(4, 2, (n, 1)) * true_sf[None, :]
    disp = 0.01
    cts = rng.negative_binomial(1.0 / disp, 1.0 / (1.0 + mean * disp)).astype(np.int64)
    cts[np.arange(n), rng.integers(0, m, n)] = 0
    cts[0, 0] = 1000000
    return cts, true_sf


def test_testthat_poscounts_recovers_the_size_factors(oracle):
    """test_size_factor.R:20-37: 100 genes x 12 samples, true factors 2^(-2,-2,-1,-1,0,0,0,0,1,1,2,2), one random zero per
    gene and a 1e6 outlier; intercept and slope - 1 of lm(sf ~ true.sf) both below 0.1 (the reference's own bound)"""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    cts, true_sf = _poscounts_case(1)
    dds = core.DESeqDataSet(cts, np.ones((12, 1)), engine=HostEngine(oracle))
    core.estimateSizeFactors(dds, type="poscounts")
    slope, icpt = np.polyfit(true_sf, dds.sizeFactors, 1)
    print("poscounts recovery: intercept %.4f, slope - 1 %.4f" % (icpt, slope - 1))
    assert abs(icpt) < 0.1 and abs(slope - 1) < 0.1
    ref = sf_spec.size_factors(oracle, cts, type="poscounts")["sizeFactors"]
    slope, icpt = np.polyfit(true_sf, ref, 1)
    assert abs(icpt) < 0.1 and abs(slope - 1) < 0.1


def test_control_genes_argument_forms():
    from deseq2_amd.engine import control_flags
    assert control_flags(None, 5) is None
    np.testing.assert_array_equal(control_flags([0, 3], 5), [1, 0, 0, 1, 0])
    np.testing.assert_array_equal(control_flags(np.array([True, False, True]), 3), [1, 0, 1])
    with pytest.raises(ValueError, match="numeric or logical"):
        control_flags("foo", 5)
    with pytest.raises(IndexError):
        control_flags([5], 5)
    with pytest.raises(ValueError, match="twice"):
        control_flags([1, 1], 5)


def test_size_factor_entries_are_exported():
    """(the layout of DsqSizeFactorArgs / DsqSizeFactorOut: test_capi_cpu.test_struct_layout_matches_header)"""
    from deseq2_amd import _lib
    for s in ("dsq_size_factors", "dsq_size_factors_dev", "dsq_size_factors_workspace_bytes"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), s)
    assert _lib.lib().dsq_size_factors_workspace_bytes(1000, 70) >= 1000 * 8 + 70 * 1024


@pytest.mark.parametrize("sfType", ["ratio", "poscounts"])
def test_deseq_with_sftype_equals_deseq_on_the_estimated_factors(oracle, sfType):
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    from tests.helpers import make_case, assert_same
    d = make_case(120, 8, "two_group", seed=3, sf_random=True)
    E = HostEngine(oracle)
    a = core.DESeq(core.DESeqDataSet(d["counts"], d["x"], engine=E), sfType=sfType)
    sf = a.sizeFactors
    assert sf is not None and np.isfinite(sf).all() and not np.all(sf == 1.0)
    b = core.DESeq(core.DESeqDataSet(d["counts"], d["x"], sizeFactors=sf, engine=E))
    assert set(a.mcols) == set(b.mcols)
    for k in b.mcols:
        assert_same(np.asarray(a.mcols[k], float), np.asarray(b.mcols[k], float), "mcols$" + k)
    c = core.DESeq(core.DESeqDataSet(d["counts"], d["x"], engine=E))             # sfType = None: factors of one, as before
    assert np.all(c.sizeFactors == 1.0)
