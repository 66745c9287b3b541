"""rlog without a GPU: the numpy specification of the structured fit (tests/rlog_spec.py: the arrow-matrix step, wave-order
sums) against the dense fit of the oracle on the model matrix the reference builds ([1 | I_m] / I_m, useQR = TRUE, the
general per-sample path); core.rlog on HostEngine(oracle) -- the literal route of R/rlog.R -- against the specification;
errors and warnings; the names the feature adds."""
import warnings

import numpy as np
import pytest

from tests import rlog_spec
from tests.rlog_cases import inputs, compare, RTOL

LN2 = np.log(2.0)


def _dense(O, k, nf, disp, bpv, intercept=None):
    """the reference's route on the rows that are fitted: returns (rows, rlog values, iter)"""
    k = np.asarray(k, np.float64)
    n, m = k.shape
    NF = np.broadcast_to(nf[None, :], (n, m)) if np.ndim(nf) == 1 else np.asarray(nf, np.float64)
    if intercept is None:
        rows = np.where((k != 0).any(axis=1))[0]
        x = np.hstack([np.ones((m, 1)), np.eye(m)])
        lam = np.r_[1e-6, np.full(m, 1.0 / bpv)]
        NFs = NF[rows]
        b0 = np.zeros((rows.size, m + 1))
        b0[:, 0] = np.log((k[rows] / NFs).mean(axis=1))
    else:
        rows = np.where(np.isfinite(intercept))[0]
        x = np.eye(m)
        lam = np.full(m, 1.0 / bpv)
        NFs = NF[rows] * (2.0 ** intercept[rows])[:, None]
        b0 = np.log(k[rows] / NFs + 0.1)
    p = x.shape[1]
    r = O.fitBeta(k[rows], x, NFs, disp[rows], np.r_[1.0, np.zeros(p - 1)], b0, lam / LN2 ** 2, np.ones((rows.size, m)), False,
                  1e-4, 100, True, 0.5, cell_mode=0)
    v = (np.log2(np.e) * r["beta_mat"]) @ x.T
    if intercept is not None:
        v = v + intercept[rows][:, None]
    return rows, v, r["iter"]


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
