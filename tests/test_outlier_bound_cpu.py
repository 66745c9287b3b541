"""The candidate bound of the outlier phase (csrc/fit_beta.hip: cooks_can_exceed; csrc/pipeline.hip: phase_outlier_first),
restated in numpy in the kernel's operation order (tests/outlier_first_cases.py) and held against the oracle chain's own
Cook's distances: every finite distance is at most its bound, every non-finite one is flagged, every replaced row is a
candidate -- and the flag does not say "always": at most 5 % of the rows are candidates without being replaced.
Runs without a GPU."""
import numpy as np
import pytest
from scipy.stats import f as fdist

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from oracle import oracle as O
from tests import outlier_first_cases as OC


@pytest.fixture(scope="module")
def chains():
    out = {}
    for name, c in OC.chain_inputs().items():
        dds = core.DESeq(core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], engine=HostEngine(O)))
        E = dds.engine
        nz = dds.attrs.get("nz_rows")
        y = np.asarray(c["counts"], np.float64)
        if nz is not None:
            y = y[nz]
        m, p = c["x"].shape
        assays = {k: np.asarray(E.to_numpy(dds.assays[k]), np.float64) for k in ("mu", "H", "cooks")}
        assert assays["mu"].shape == y.shape, (assays["mu"].shape, y.shape)
        rep = np.asarray(dds.mcols["replace"], np.float64)
        rep = np.nan_to_num(rep if nz is None else rep[nz]).astype(bool)
        out[name] = dict(y=y, p=p, cutoff=float(fdist.ppf(.99, p, m - p)), replace=rep, **assays)
    return out


@pytest.mark.parametrize("name", ["two_group_28", "batch_condition_48"])
def test_bound_holds_on_the_oracle_chain(chains, name):
    c = chains[name]
    with np.errstate(all="ignore"):
        bound = OC.cooks_expr(c["y"], c["mu"], c["H"], c["p"], OC.ALPHA_FLOOR)
    flag = OC.sample_flag(c["y"], c["mu"], c["H"], c["p"], c["cutoff"])
    fin = np.isfinite(c["cooks"])
    assert (c["cooks"][fin] <= bound[fin]).all(), "a Cook's distance above its bound"
    assert flag[~fin].all(), "a non-finite distance that is not flagged"
    over = fin & (c["cooks"] > c["cutoff"])
    assert flag[over].all()
    cand = flag.any(axis=1)
    assert c["replace"].sum() >= 4, "the planted outliers are gone"
    assert (over.any(axis=1) == c["replace"]).all()          # (replaceOutliers flags the rows with ANY distance over the cutoff)
    assert cand[c["replace"]].all(), "a replaced row that is no candidate"
    share = (cand & ~c["replace"]).mean()
    print("%s: %d rows, %d candidates, %d replaced, share flagged without replacement %.4f" %
          (name, len(cand), cand.sum(), c["replace"].sum(), share))
    assert share <= 0.05
    assert (~cand).sum() >= 0.9 * len(cand)


def test_bound_entrywise_fuzz():
    rng = np.random.default_rng(5)
    N = 400000
    m = 500
    mu = np.exp(rng.uniform(np.log(0.5), np.log(1e9), N))
    y = np.floor(np.where(rng.uniform(size=N) < 0.5, rng.poisson(np.minimum(mu, 1e6)), np.exp(rng.uniform(0, np.log(2e9), N))))
    y[rng.uniform(size=N) < 0.05] = 0.0
    h = np.where(rng.uniform(size=N) < 0.5, rng.uniform(0, 1, N), 1.0 - np.exp(rng.uniform(np.log(1e-12), 0, N)))
    h[:100] = 0.0
    h[100:200] = 1.0 - 1e-12
    alpha = np.exp(rng.uniform(np.log(OC.ALPHA_FLOOR), np.log(float(m)), N))
    alpha[::7] = OC.ALPHA_FLOOR
    for p in (2, 4, 7):
        with np.errstate(all="ignore"):
            ck = OC.cooks_expr(y, mu, h, p, alpha)
            bound = OC.cooks_expr(y, mu, h, p, OC.ALPHA_FLOOR)
        assert np.isfinite(ck).all()
        assert (ck <= bound).all()
        for cutoff in (0.0, 1.0, float(fdist.ppf(.99, p, m - p)), 1e6):
            assert OC.sample_flag(y, mu, h, p, cutoff)[ck > cutoff].all()
            assert OC.sample_flag_divfree(y, mu, h, p, cutoff)[bound > cutoff].all()      # (the alt build's form: no narrower)


def test_non_finite_entries_are_flagged():
    vals_mu = np.array([0.0, 1e-200, 0.5, 10.0, 1e160, 1e308, np.inf, np.nan])
    vals_h = np.array([-0.5, 0.0, 0.3, 1.0, 1.5, np.inf, np.nan])
    vals_y = np.array([0.0, 1.0, 1e9])
    y, mu, h = (a.ravel() for a in np.meshgrid(vals_y, vals_mu, vals_h, indexing="ij"))
    for alpha in (OC.ALPHA_FLOOR, 1.0, 500.0):
        with np.errstate(all="ignore"):
            ck = OC.cooks_expr(y, mu, h, 4, alpha)
        for cutoff in (0.0, 3.3, 1e6):
            flag = OC.sample_flag(y, mu, h, 4, cutoff)
            assert flag[~np.isfinite(ck)].all()
            assert flag[h < 0].all()
            assert OC.sample_flag_divfree(y, mu, h, 4, cutoff)[flag].all()
            with np.errstate(invalid="ignore"):
                assert flag[ck > cutoff].all()
