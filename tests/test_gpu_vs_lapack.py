"""-m gpu: the HIP path against the independently written LAPACK restatement (oracle/lapack_oracle.py) -- the same
comparison and budgets the C oracle is held to in tests/test_oracle_vs_lapack.py, through the host-pointer C ABI.  The
bit-for-bit comparisons with the C oracle are tests/test_gpu_parity.py and its neighbours; this file shows the HIP results
next to an implementation that shares no arithmetic with them (LAPACK, cephes, numpy's summation order)."""
import numpy as np
import pytest

from deseq2_amd import native
from oracle import lapack_oracle
from tests import wide_cases
from tests.helpers import assert_same
from tests.test_oracle_vs_lapack import (SHAPE_NAMES, _case, _fit_beta_compare, compare, golden_cases, run_all,
                                         shape_case)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(golden_cases()))
def test_hip_vs_lapack_small(name):
    d = golden_cases()[name]
    compare(run_all(native, d), run_all(lapack_oracle, d), d, name)


@pytest.mark.parametrize("n,m,design,kw", [
    (1500, 50, "batch_condition", {}),
    (400, 120, ("factor", 8), {}),
    (600, 30, "two_group", {"weights": True}),
    (300, 64, "batch_condition", {"weights": True, "zero_w": True, "useQR": False}),
])
def test_hip_vs_lapack(n, m, design, kw):
    d = _case(n, m, design, seed=n + m, **kw)
    compare(run_all(native, d), run_all(lapack_oracle, d), d, "%dx%d" % (n, m))


def test_hip_vs_lapack_beyond_the_resident_waves():
    """9 000 genes x 100 samples, ~ batch + condition: three times the 3 072 wave slots the persistent fit kernels keep
    resident, so every wave fits several genes in a row: fitBeta$iter equal on every gene, fitDisp
    iterations equal outside <= 1 % ulp-level ties, values within 1e-7 / 1e-8 (about a minute of numpy)."""
    d = _case(9000, 100, "batch_condition", seed=9100)
    st = compare(run_all(native, d), run_all(lapack_oracle, d), d, "9000x100")
    assert st["fitBeta"]["iter_mismatch"] == 0 and st["fitDispGrid"]["same"] >= 0.99


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_hip_vs_lapack_at_baseline_shapes(name):
    """BASELINE.json configs C2..C5 at full shape (C3: 1000 x 500 p=4; C4: 200 x 2000, 10-level factor, QR; C5:
    1000 x 200, weights with zeros + the betaPrior pass on the expanded p=3 design; C2: 1000 x 100): iteration counts
    equal (ties <= 1 %), well-conditioned share >= 0.95, grid agreement >= 0.95, values within 1e-7 / 1e-8."""
    d = shape_case(name)
    compare(run_all(native, d), run_all(lapack_oracle, d), d, name, min_well=0.95)


@pytest.mark.parametrize("seed", (5, 6, 7))
def test_hip_floor_regime_vs_lapack(seed):
    """the dispersion-floor regime (Poisson / NB mixture, > 25 % of the genes start at alpha_0 = 1e-8): everything R's
    callers see -- fitBeta$iter, clamped dispGeneEst, dispGeneEstConv / refitDisp, MAP dispConv and dispMAP
    (tests/floor_regime.py)"""
    from tests.floor_regime import assert_visible_parity, floor_case, visible_chain
    d = floor_case(seed)
    assert_visible_parity(visible_chain(native, d), visible_chain(lapack_oracle, d), "hip seed %d" % seed)


# ---- designs of 11 to 64 columns (tests/wide_cases.py): the rolled kernels of fit_beta_wide.hip / fit_disp_wide.hip, the
# cell kernels at their widest, the per-width kernels on long rows -- searches run to convergence

_LAPACK = {}


def _wide(name):
    """the case and its LAPACK results, computed once for the tests of this module"""
    if name not in _LAPACK:
        d = wide_cases.expanded_case(name) if name in wide_cases.EXPANDED else wide_cases.wide_case(name)
        _LAPACK[name] = (d, run_all(lapack_oracle, d))
    return _LAPACK[name]


@pytest.mark.parametrize("name", sorted(wide_cases.WIDE))
def test_hip_vs_lapack_wide(name):
    """every case of wide_cases.WIDE in the geometry the launch picks by itself: fitBeta$iter equal on every gene, fitDisp
    iterations equal outside ulp-level ties (<= max(1, 1 %)), grid agreement >= 0.95, values at scale 1"""
    d, ref = _wide(name)
    compare(run_all(native, d), ref, d, name, min_well=wide_cases.MIN_WELL)


@pytest.mark.parametrize("name", wide_cases.EXPANDED)
def test_hip_vs_lapack_expanded_prior_wide(name):
    """betaPrior pass 2 on the expanded design of a wide factor (p = 13, 21, 48, 64; rank deficient), QR and normal
    equations, values at scale 1"""
    d, ref = _wide(name)
    got = run_all(native, d)
    compare(got, ref, d, name, min_well=wide_cases.MIN_WELL)
    _fit_beta_compare(got["fitBetaPrior"], ref["fitBetaPrior"], name, "fitBetaPrior", 1.0)


@pytest.mark.parametrize("name", sorted(wide_cases.FLOOR))
def test_hip_floor_regime_vs_lapack_wide(name):
    """the dispersion-floor regime on a paired design (p = 21) and on a 16-level factor"""
    from tests.floor_regime import assert_visible_parity, visible_chain
    d = wide_cases.floor_wide_case(name)
    assert_visible_parity(visible_chain(native, d), visible_chain(lapack_oracle, d), "hip " + name)


@pytest.mark.parametrize("geometry", [{"DSQ_WIDE_NW": "1"}, {"DSQ_WIDE_NW": "8"}, {"DSQ_WIDE_LDS": "0"}],
                         ids=lambda g: "-".join("%s=%s" % kv for kv in g.items()))
@pytest.mark.parametrize("name", ["paired30_qr", "cont_p31_m124"])
def test_hip_vs_lapack_wide_forced_geometry(monkeypatch, name, geometry):
    """the rolled kernels with one and with eight waves per gene, and fitBeta with the gene's slab in global memory, against
    the same LAPACK results as the default geometry"""
    for k, v in geometry.items():
        monkeypatch.setenv(k, v)
    d, ref = _wide(name)
    compare(run_all(native, d), ref, d, "%s %r" % (name, geometry), min_well=wide_cases.MIN_WELL)


BEYOND_N, BEYOND_EVERY = 1400, 9


def test_hip_vs_lapack_wide_beyond_the_resident_genes(oracle):
    """`~ patient + treatment`, 30 patients (p = 31, m = 60), on more genes than the rolled launches keep resident: on the
    MI355X (256 CUs) fitBeta runs 2 waves per gene with 4 genes/CU = 1 024 gene slots, fitDisp 2 waves per gene with
    5 genes/CU = 1 280 (4 genes/CU = 1 024 for the second-derivative pass) -- the DSQ_VERBOSE=1 lines of this test -- so with
    1 400 genes every workgroup of the two searches fits a second gene after its first.  HIP == oracle bit for bit on every
    gene; every 9th gene (156 of them) against LAPACK with the budgets of compare().  A fit depends on its own row alone, so
    the LAPACK results of the row subset are held against the subset of the full run's rows: the test shows once, on the
    oracle, that the two are the same."""
    d = wide_cases.case(BEYOND_N, wide_cases.paired(30))
    n = d["counts"].shape[0]
    assert n > 1280
    got, orc = run_all(native, d), run_all(oracle, d)
    for fn in ("fitBeta", "fitDispMLE", "fitDispMAP", "fitDispGrid"):
        for k, v in orc[fn].items():
            if v is not None:
                assert_same(got[fn][k], v, "%s$%s, %d genes" % (fn, k, n))
    rows = np.arange(0, n, BEYOND_EVERY)
    ds = wide_cases.take_rows(d, rows)
    sub = {fn: {k: (v[rows] if v is not None else None) for k, v in got[fn].items()} for fn in got}
    osub = run_all(oracle, ds)
    for fn in ("fitBeta", "fitDispMLE", "fitDispMAP", "fitDispGrid"):
        for k, v in osub[fn].items():
            if v is not None:
                assert_same(orc[fn][k][rows], v, "row subset of the inputs, %s$%s" % (fn, k))
    compare(sub, run_all(lapack_oracle, ds), ds, "paired30 x %d, every %dth gene" % (n, BEYOND_EVERY),
            min_well=wide_cases.MIN_WELL)
