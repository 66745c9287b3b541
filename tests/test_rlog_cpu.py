"""rlog without a GPU: the numpy specification of the structured fit (tests/rlog_spec.py: the arrow-matrix step, wave-order
sums) against the dense fit of the oracle on the model matrix the reference builds ([1 | I_m] / I_m, useQR = TRUE, the
general per-sample path); core.rlog on HostEngine(oracle) -- the literal route of R/rlog.R -- against the specification;
errors and warnings; the names the feature adds."""
import warnings

import numpy as np
import pytest

from tests import rlog_spec
from tests.rlog_cases import inputs, compare, dense_design, dense_values, lapack_case, mutants, RTOL, TIE_CAP


def _dense(O, k, nf, disp, bpv, intercept=None):
    """the reference's route on the rows that are fitted: returns (rows, rlog values, iter)"""
    rows, x, args = dense_design(k, nf, disp, bpv, intercept)
    r = O.fitBeta(*args, cell_mode=0)
    return rows, dense_values(x, r, rows, intercept), r["iter"]


@pytest.mark.parametrize("nf_matrix", [False, True])
@pytest.mark.parametrize("m", [1, 2, 3, 6, 12, 33, 63])
def test_spec_against_dense_oracle(oracle, m, nf_matrix):
    """Maxima seen on the seeded inputs (profiles/rlog.md): no row with another iteration count in any case; the largest
    relative difference is recorded there per form."""
    d = inputs(240, m, seed=int(nf_matrix), nf_matrix=nf_matrix)
    k, nf, disp, bpv = d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"]
    sa = rlog_spec.rlog_fit(oracle, k, nf, disp, bpv)
    assert sa["flag"][3] == 1 and (sa["rlog"][3] == 0).all() and sa["intercept"][3] == -np.inf
    rows, v, it = _dense(oracle, k, nf, disp, bpv)
    assert (sa["flag"][rows] == 0).all()
    compare(sa["rlog"][rows], v, "form A m=%d" % m, sa["iter"][rows], it)
    # form B: the intercept fitted above, frozen; the all-zero row comes back with -Inf (not fitted), one more non-finite
    # entry, and one finite intercept on all-zero counts (fitted)
    c = np.array(sa["intercept"])
    c[5] = np.nan
    k2 = k.copy()
    k2[7] = 0
    sb = rlog_spec.rlog_fit(oracle, k2, nf, disp, bpv, intercept=c)
    assert (sb["flag"][[3, 5]] == 1).all() and (sb["rlog"][[3, 5]] == 0).all() and sb["flag"][7] == 0
    rows, v, it = _dense(oracle, k2, nf, disp, bpv, intercept=c)
    compare(sb["rlog"][rows], v, "form B m=%d" % m, sb["iter"][rows], it)


# m >= 64: the dense C oracle stops at 64 columns ([1 | I_63]); the LAPACK restatement has no width limit
LAPACK_SHAPES = [(63, 100), (64, 100), (65, 100), (129, 60), (257, 24)]


@pytest.mark.parametrize("m,n", LAPACK_SHAPES)
def test_spec_against_dense_lapack(oracle, m, n):
    """The specification against oracle/lapack_oracle.py's fitBeta on the dense [1 | I_m] / I_m design, forms A and B, at
    the project's RTOL and TIE_CAP.  m = 63 is held to the C oracle too, so this line overlaps the one above.  Measured
    maxima: profiles/rlog.md.  m > 600 stays with the bit identity of the device to the specification alone: a dense QR
    at m = 2 049 costs about a minute per gene."""
    c = lapack_case(oracle, n, m)
    d = c["d"]
    for form, spec, ref, k, icpt in (("A", c["specA"], c["lapackA"], d["counts"], None), ("B", c["specB"], c["lapackB"], c["k2"], c["c"])):
        rows, v, it = ref
        assert rows.size >= n - 2 and (spec["flag"][rows] == 0).all()
        compare(spec["rlog"][rows], v, "spec / LAPACK form %s m=%d" % (form, m), spec["iter"][rows], it)
        if m == 63:
            orows, ov, oit = _dense(oracle, k, d["nf"], d["dispFit"], d["betaPriorVar"], intercept=icpt)
            assert (orows == rows).all()
            compare(ov, v, "oracle / LAPACK form %s m=%d" % (form, m), oit, it)
            compare(spec["rlog"][rows], ov, "spec / oracle form %s m=%d" % (form, m), spec["iter"][rows], oit)
    assert (c["specB"]["flag"][[3, 5]] == 1).all() and c["specB"]["flag"][7] == 0


def test_lapack_comparison_has_teeth(oracle):
    """the comparison of test_spec_against_dense_lapack refuses one value moved by 3e-11 relative and one iteration count
    off by one (one row of 99 is above TIE_CAP), and passes the unchanged result"""
    c = lapack_case(oracle, 100, 65)
    rows, v, it = c["lapackA"]
    spec = c["specA"]
    compare(spec["rlog"][rows], v, "unchanged", spec["iter"][rows], it)
    assert TIE_CAP * rows.size < 1
    for name, (mv, mi) in zip(("value", "iteration count"), mutants(spec["rlog"], spec["iter"], rows)):
        with pytest.raises(AssertionError):
            compare(mv[rows], v, "mutant: " + name, mi[rows], it)


def _spec_of(O, dt, counts, intercept=None):
    dds = dt.dds
    nf = dds.sizeFactors if dds.sizeFactors is not None else np.asarray(dds.engine.to_numpy(dds.nf))
    disp = np.where(np.isnan(dds.mcols["dispFit"]), 1.0, dds.mcols["dispFit"])      # (all-zero rows: never read by a fit)
    return rlog_spec.rlog_fit(O, counts, nf, disp, dt.attrs["betaPriorVar"], intercept=intercept)


@pytest.fixture(scope="module")
def host_case(oracle):
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    d = inputs(200, 6, seed=3)
    k = d["counts"]
    k[11] = 0
    E = HostEngine(oracle)
    return core, E, k


def _check_transform(O, dt, k, intercept=None):
    s = _spec_of(O, dt, k, intercept)
    compare(dt.assay(), s["rlog"], "core.rlog", dt.dds.mcols["rlogIter"], s["iter"])
    if intercept is None:
        zero = ~(k != 0).any(axis=1)
        assert (dt.assay()[zero] == 0).all() and (dt.mcols["rlogIntercept"][zero] == -np.inf).all()
        compare(dt.mcols["rlogIntercept"][~zero][:, None], s["intercept"][~zero][:, None], "rlogIntercept")
    else:
        assert "rlogIntercept" not in dt.mcols
    return s


def test_core_rlog_matrix_and_round_trip(oracle, host_case):
    core, E, k = host_case
    before = k.copy()
    dt = core.rlog(k, engine=E)
    assert dt.kind == "rlog" and dt.attrs["betaPriorVar"] > 0 and (k == before).all()
    _check_transform(oracle, dt, k)
    # the frozen rlog: the data set's own intercept passed back, same prior variance
    icpt = dt.mcols["rlogIntercept"]
    dt2 = core.rlogTransformation(k, intercept=icpt, betaPriorVar=dt.attrs["betaPriorVar"], engine=E)
    assert dt2.attrs["betaPriorVar"] == dt.attrs["betaPriorVar"]
    _check_transform(oracle, dt2, k, icpt)
    assert (dt2.assay()[[3, 11]] == 0).all()
    # a given prior variance is used as given and changes the result
    dt3 = core.rlog(k, betaPriorVar=0.25, engine=E)
    assert dt3.attrs["betaPriorVar"] == 0.25
    _check_transform(oracle, dt3, k)
    assert np.abs(dt3.assay() - dt.assay()).max() > 1e-3


@pytest.mark.parametrize("blind", [True, False])
def test_core_rlog_dataset(oracle, host_case, blind):
    core, E, k = host_case
    x = np.c_[np.ones(6), np.r_[np.zeros(3), np.ones(3)]]
    sf = np.exp(np.random.default_rng(2).normal(0, 0.3, 6))
    dds = core.DESeqDataSet(k, x, sizeFactors=sf, engine=E)
    dt = core.rlog(dds, blind=blind)
    assert dds.mcols == {} and dds.dispersionFunction is None          # the argument is left as it was
    assert (dt.dds.sizeFactors == sf).all()
    _check_transform(oracle, dt, k)
    if not blind:
        # the trend was fitted under the object's design: it differs from the blind one
        blind_fit = core.rlog(dds, blind=True).dds.mcols["dispFit"]
        assert not np.array_equal(blind_fit, dt.dds.mcols["dispFit"], equal_nan=True)
        # an object that carries dispFit is not fitted again
        dds2 = core.DESeqDataSet(k, x, sizeFactors=sf, engine=E)
        dds2.mcols["dispFit"] = np.where(np.isnan(dt.dds.mcols["dispFit"]), 1.0, dt.dds.mcols["dispFit"]) * 2.0
        dt2 = core.rlog(dds2, blind=False)
        assert (dt2.dds.mcols["dispFit"] == dds2.mcols["dispFit"]).all()
        _check_transform(oracle, dt2, k)


def test_errors_and_warnings(oracle, host_case):
    core, E, k = host_case
    x = np.ones((6, 1))
    with pytest.raises(NotImplementedError, match="weights"):
        core.rlog(core.DESeqDataSet(k, x, weights=np.ones(k.shape), engine=E))
    with pytest.raises(ValueError, match="intercept should be as long"):
        core.rlog(k, intercept=np.zeros(5), engine=E)
    dds = core.DESeqDataSet(k, x, sizeFactors=np.ones(6), engine=E)
    dds.mcols["dispFit"] = np.full(k.shape[0], 0.1)
    dds.mcols["dispFit"][20] = np.nan
    with pytest.raises(ValueError, match="dispFit"):
        core.rlog(dds, blind=False)
    # sparsity: every gene above a row sum of 100 has one sample that holds more than 90 % of it
    sparse = np.zeros((50, 6), dtype=np.int32)
    sparse[np.arange(50), np.arange(50) % 6] = 1000
    sparse[:10] += 1
    with pytest.warns(UserWarning, match="close to a negative binomial"):
        core.sparseTest(core.DESeqDataSet(sparse, x, sizeFactors=np.ones(6), engine=E))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        core.sparseTest(core.DESeqDataSet(k, x, sizeFactors=np.ones(6), engine=E))
        core.sparseTest(core.DESeqDataSet(np.ones((5, 6), dtype=np.int32), x, sizeFactors=np.ones(6), engine=E))


def test_names_exist():
    from deseq2_amd import core, native, engine, _lib
    assert callable(core.rlog) and core.rlogTransformation is core.rlog and callable(core.rlogData)
    assert callable(native.rlog) and callable(native.rlog_dev)
    assert hasattr(engine.DeviceEngine, "rlog_fit") and hasattr(engine.HostEngine, "rlog_fit")
    assert "dsq_rlog_dev" in _lib.EXPORTED_SYMBOLS and "dsq_rlog" in _lib.EXPORTED_SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "dsq_rlog_dev") and hasattr(L, "dsq_rlog")
    assert _lib.DsqRlogArgs and _lib.DsqRlogOut
    assert RTOL == 1e-11
