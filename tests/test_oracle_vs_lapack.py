"""CPU: the C oracle against its independently written counterpart (oracle/lapack_oracle.py).

The reference (src/DESeq2.cpp) cannot be built AS R BUILDS IT in this image -- it needs R, Rcpp, RcppArmadillo and
Armadillo, none of which exist here.  Its source does compile against stand-in headers (oracle/shim/, oracle/Makefile `ref`):
that build is the reference's control flow over stand-in linear algebra and binary128 special functions -- not R's nmath, not
Armadillo's LAPACK -- and tests/test_oracle_vs_reference.py holds the oracle and the restatement below to it, the half a
second reading of the same text cannot check.  The reference's OWN tests pin the oracle too: tests/test_oracle_properties.py
restates their known answers and properties.  This file is the other half: a numpy restatement of the same three routines
with real LAPACK (dgeqrf / dgesv / dgetrf / dgetri through numpy.linalg -- what Armadillo itself calls), scipy's special
functions and numpy's summation order, written from the reference's text matrix expression by matrix expression.  Two
restatements that share no linear algebra, no lgamma / digamma and no summation order must agree on: iteration counts
and accept counts EQUAL (bar last-bit ties of the final Armijo test, bounded below), values within 1e-7 / 1e-8 relative
(north_star asks 1e-6).

Conditioning.  At alpha ~ 1e-8 (the minDisp clamp) the reference's dlog_posterior multiplies a sum of
digamma differences by alpha^-2 = 1e16 (src/DESeq2.cpp:90-96): its value there is rounding noise of
whichever lgamma/digamma implementation is underneath, and so is the number of line-search steps.  The
strict comparison therefore covers the genes whose start AND final dispersion are above 1e-6; for the
others the test asserts what is implementation-independent: both end at the same floor."""
import os

import numpy as np
import pytest

from tests.helpers import make_case

FLAGS = ("iter", "iter_accept")


def _case(n, m, design, seed, weights=False, useQR=True, useCR=True, lam=1e-6, zero_w=False):
    d = make_case(n, m, design, seed=seed, weights=weights, sf_random=True)
    if zero_w:
        d["weights"][:, ::5] = 0.0          # whole samples dropped: exercises x.rows(find(w > thr)) :41
    p = d["x"].shape[1]
    d.update(useWeights=weights, useQR=useQR, useCR=useCR, lam=np.full(p, lam) / np.log(2) ** 2)
    return d


def golden_cases():
    return {
        "c1_two_group_m6": _case(120, 6, "two_group", 11),
        "bc_m12": _case(100, 12, "batch_condition", 12),
        "bc_m24_weights": _case(80, 24, "batch_condition", 13, weights=True),
        "two_m10_normal_eq": _case(80, 10, "two_group", 14, useQR=False),
        "factor5_m20_ridge": _case(60, 20, ("factor", 5), 15, lam=0.5),
        "two_m16_zero_weights_noCR": _case(60, 16, "two_group", 16, weights=True, zero_w=True, useCR=False),
    }


def live_cases():
    c = dict(golden_cases())
    c.update({
        "bc_m60": _case(300, 60, "batch_condition", 21),
        "factor10_m100": _case(400, 100, ("factor", 10), 22),   # 400 genes: the 1 % tie budget needs a sample that can resolve it
        "two_m200_weights": _case(60, 200, "two_group", 23, weights=True),
        "bc_m36_zero_weights": _case(120, 36, "batch_condition", 24, weights=True, zero_w=True),
        "two_m8_ridge_ne": _case(200, 8, "two_group", 25, useQR=False, lam=2.0),
        # designs with a continuous covariate (general mode).  From p = 7 the Cox-Reid Gram sums of fitDisp are taken
        # serially (rows of <= 256 samples; <= 1024 from p = 10) -- round 3's re-specified order, held to the same budgets
        "cont_p5_m40": _case(150, 40, ("factor_cont", 4), 26),
        "cont_p8_m60_serial": _case(150, 60, ("factor_cont", 7), 27),
        "cont_p10_m120_serial_weights": _case(120, 120, ("factor_cont", 9), 28, weights=True),
        "cont_p9_m300_waveorder": _case(100, 300, ("factor_cont", 8), 29),
        "cont_p12_m90_serial_ne": _case(100, 90, ("factor_cont", 11), 30, useQR=False),
    })
    return c


SHAPE_NAMES = ("C2_two_group_m100", "C3_batch_condition_m500", "C4_factor10_m2000", "C5_weights_prior_m200")


def shape_case(name):
    """BASELINE.json configs C2..C5 at their full SHAPE (samples, design, options), a gene count the numpy restatement
    finishes in seconds.  C5 adds the betaPrior pass 2: the expanded design
    (Intercept, condA, condB; R/expanded.R:1-18) with lambda = (1e-6, 1/sigma^2, 1/sigma^2), sigma^2 = 1
    (R/fitNbinomGLMs.R:311,319-325), start values of the rank-deficient branch (:146-155)."""
    if name == "C2_two_group_m100":
        return _case(1000, 100, "two_group", 34)
    if name == "C3_batch_condition_m500":
        return _case(1000, 500, "batch_condition", 31)
    if name == "C4_factor10_m2000":
        return _case(200, 2000, ("factor", 10), 32)
    if name == "C5_weights_prior_m200":
        d = _case(1000, 200, "two_group", 33, weights=True, zero_w=True)
        cond = d["x"][:, 1]
        d["x_expanded"] = np.column_stack([np.ones_like(cond), 1.0 - cond, cond])
        d["lam_expanded"] = np.array([1e-6, 1.0, 1.0]) / np.log(2) ** 2
        return d
    raise KeyError(name)


def shape_cases():
    return {k: shape_case(k) for k in SHAPE_NAMES}


def run_all(F, d):
    """fitBeta -> fitDisp (MLE) -> fitDisp (MAP) -> fitDispGrid, the reference's call sequence"""
    y, x, nf, w = d["counts"].astype(float), d["x"], d["nf"], d["weights"]
    p = x.shape[1]
    uw = d["useWeights"]
    beta = F.fitBeta(y, x, nf, d["alpha_init"], np.r_[1.0, np.zeros(p - 1)], d["beta_init"], d["lam"], w, uw, 1e-8,
                     100, d["useQR"], 0.5)
    mu = np.maximum(nf * np.exp(beta["beta_mat"] @ x.T), 0.5)           # R/fitNbinomGLMs.R:180, core.R:763
    la0 = np.log(d["alpha_init"])
    wd = np.maximum(w, 1e-6) if uw else w
    mle = F.fitDisp(y, x, mu, la0, la0, 1.0, np.log(1e-8 / 10), 1.0, 1e-6, 100, False, wd, uw, 1e-2, d["useCR"])
    mp = F.fitDisp(y, x, mu, la0 + 0.3, la0 - 0.2, 0.7, np.log(1e-8 / 10), 1.0, 1e-6, 100, True, wd, uw, 1e-2,
                   d["useCR"])
    grid = np.linspace(np.log(1e-8), np.log(max(10, y.shape[1])), 20)
    gr = F.fitDispGrid(y, x, mu, grid, la0, 1.0, True, wd, uw, 1e-2, d["useCR"])
    res = {"fitBeta": beta, "fitDispMLE": mle, "fitDispMAP": mp, "fitDispGrid": gr, "aux": {"mu": mu}}
    if "x_expanded" in d:        # fitGLMsWithPrior pass 2 (R/fitNbinomGLMs.R:319-325) at the MAP dispersions
        xe = d["x_expanded"]
        b0 = np.zeros((y.shape[0], xe.shape[1]))
        b0[:, 0] = np.log((y / nf).mean(axis=1))                         # :148-151
        alpha = np.minimum(np.maximum(np.exp(mp["log_alpha"]), 1e-8), max(10, y.shape[1]))
        contrast = d.get("contrast_expanded", np.r_[0.0, -1.0, 1.0])     # C5: condB against condA
        res["fitBetaPrior"] = F.fitBeta(y, xe, nf, alpha, contrast, b0, d["lam_expanded"], w, uw, 1e-8,
                                        100, d["useQR"], 0.5)
    return res


def _close(a, b, what, rtol=1e-8, atol=0.0):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what, equal_nan=True)


# budgets the comparisons are held to (measured: profiles/r02_parity.md).  `well` = share of genes whose start and
# final dispersions are above 1e-6 (the rest sit at the minDisp floor, see "Conditioning" above): >= 0.95 and grid
# agreement >= 0.95 everywhere except the m <= 12 cases (measured 0.84 / 0.87 at m = 6, 0.93 / 0.97 at m = 12, where
# the estimate of a sixth of the synthetic genes collapses to the floor): 0.8 / 0.85 there.  Ties <= 1 %.
MAX_TIE_FRAC = 0.01
MIN_GRID_SAME = 0.95


def _fit_beta_compare(gb, rb, name, fn, scale=1.0):
    np.testing.assert_array_equal(gb["iter"], rb["iter"], err_msg="%s %s$iter" % (name, fn))
    conv = rb["iter"] < 100
    assert conv.mean() > 0.8
    for k in ("beta_mat", "beta_var_mat", "contrast_num", "contrast_denom"):
        _close(gb[k][conv], rb[k][conv], "%s %s$%s" % (name, fn, k), rtol=1e-7 * scale, atol=1e-12)
    _close(gb["hat_diagonals"][conv], rb["hat_diagonals"][conv], "%s %s$hat_diagonals" % (name, fn), rtol=1e-8 * scale,
           atol=1e-14)
    _close(gb["deviance"][conv], rb["deviance"][conv], "%s %s$deviance" % (name, fn), rtol=1e-8 * scale)
    return {"n": int(conv.size), "iter_mismatch": 0, "converged": float(conv.mean())}


def compare(got, ref, d, name, min_well=None, min_grid=None, scale=1.0):
    """asserts the budgets and returns the measured rates (tools/parity_report.py prints them).  scale: multiplier of
    the VALUE tolerances; the iteration counts are held equal either way"""
    alpha0 = d["alpha_init"]
    tiny = d["counts"].shape[1] <= 12          # m <= 12: up to a sixth of the synthetic genes sit at the floor
    if min_well is None:
        min_well = 0.8 if tiny else 0.95
    if min_grid is None:
        min_grid = 0.85 if tiny else MIN_GRID_SAME
    stats = {"fitBeta": _fit_beta_compare(got["fitBeta"], ref["fitBeta"], name, "fitBeta", scale)}
    if "fitBetaPrior" in ref:
        # the expanded design (Intercept, condA, condB) is rank deficient: X'WX + diag(1e-6, 1, 1) / ln(2)^2 has a
        # condition number of ~1e6 x that of a full-rank design, and LU with different pivoting orders (LAPACK's dgetrf
        # against the oracle's) moves the last digits of its inverse accordingly -- 1e-6, north_star's bar, there
        stats["fitBetaPrior"] = _fit_beta_compare(got["fitBetaPrior"], ref["fitBetaPrior"], name, "fitBetaPrior",
                                                  10 * scale)
    # ---- fitDisp: strict on the well-conditioned genes
    for fn in ("fitDispMLE", "fitDispMAP"):
        g, r = got[fn], ref[fn]
        well = (alpha0 > 1e-6) & (np.exp(r["log_alpha"]) > 1e-6) & (np.exp(g["log_alpha"]) > 1e-6)
        # a Cox-Reid matrix made singular by the weight subsetting (e.g. the reference level of a factor loses all
        # its samples: intercept = sum of the dummies) has det = +-rounding noise: lp is NaN in both, the rest noise
        np.testing.assert_array_equal(np.isfinite(g["initial_lp"]), np.isfinite(r["initial_lp"]),
                                      err_msg="%s %s: non-finite log posterior in different genes" % (name, fn))
        well &= np.isfinite(r["initial_lp"])
        assert well.mean() >= min_well, "%s %s: only %.3f of the genes are well conditioned" % (name, fn, well.mean())
        # a final proposal whose gain is a few ulp of lp (|lp| ~ 1e4 -> 2e-12) passes or fails the Armijo test
        # (:229) on the last bit: such a gene may take one step more or less.  Everything else: equal.
        tie = well & (np.minimum(np.abs(g["last_change"]), np.abs(r["last_change"])) < 64 * np.spacing(np.abs(r["last_lp"])))
        tie &= (g["iter"] != r["iter"]) | (g["iter_accept"] != r["iter_accept"])
        assert tie.sum() <= max(1, MAX_TIE_FRAC * well.sum()), "%s %s: %d ulp-level ties" % (name, fn, tie.sum())
        # (a rejected last-bit proposal halves kappa until a step small enough passes, so the COUNT of a tie gene
        # can differ by tens of iterations -- C3 shape: 14 vs 34 -- while its optimum agrees to 1e-7, checked below)
        well_strict = well & ~tie
        for k in FLAGS:
            np.testing.assert_array_equal(g[k][well_strict], r[k][well_strict], err_msg="%s %s$%s" % (name, fn, k))
        for k in ("log_alpha", "initial_lp", "last_lp"):
            _close(g[k][well_strict], r[k][well_strict], "%s %s$%s" % (name, fn, k),
                   rtol=(1e-7 if k == "log_alpha" else 1e-8) * scale, atol=1e-9)
            # a tie gene stops one (tiny) step earlier or later: its optimum agrees to the search's own tolerance
            _close(g[k][tie], r[k][tie], "%s %s$%s (ties)" % (name, fn, k), rtol=1e-6, atol=1e-9)
        _close(g["initial_dlp"][well], r["initial_dlp"][well], "%s %s$initial_dlp" % (name, fn), rtol=1e-6, atol=1e-5)
        for k in ("last_dlp", "last_d2lp"):
            if k in g and g[k] is not None:
                _close(g[k][well_strict], r[k][well_strict], "%s %s$%s" % (name, fn, k), rtol=1e-6, atol=1e-5)
        floor = ~well
        if floor.any():        # both end (far) below any dispersion the callers keep (minDisp clamp 1e-8 .. 1e-6)
            assert (np.exp(g["log_alpha"][floor]) < 1e-5).all() and (np.exp(r["log_alpha"][floor]) < 1e-5).all()
        with np.errstate(all="ignore"):
            rel = np.abs(g["log_alpha"][well] - r["log_alpha"][well]) / np.maximum(np.abs(r["log_alpha"][well]), 1e-300)
        stats[fn] = {"n": int(well.size), "well": float(well.mean()), "ties": int(tie.sum()),
                     "iter_mismatch_outside_ties": 0, "max_rel_log_alpha": float(rel.max()) if rel.size else 0.0}
    # ---- grid: argmax over a fixed grid; ties in the noise region can pick a neighbour
    gg, rg = got["fitDispGrid"]["log_alpha"], ref["fitDispGrid"]["log_alpha"]
    same = gg == rg
    assert same.mean() >= min_grid, "%s fitDispGrid: only %.3f identical" % (name, same.mean())
    assert (np.exp(rg[~same]) < 1e-5).all() and (np.exp(gg[~same]) < 1e-5).all()
    stats["fitDispGrid"] = {"n": int(same.size), "same": float(same.mean())}
    return stats


@pytest.fixture(scope="module")
def lapack():
    from oracle import lapack_oracle
    return lapack_oracle


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_oracle_vs_lapack_at_baseline_shapes(oracle, lapack, name):
    """C2..C5 shapes of BASELINE.json"""
    d = shape_case(name)
    compare(run_all(oracle, d), run_all(lapack, d), d, name, min_well=0.95)


@pytest.mark.parametrize("name", sorted(live_cases()))
def test_oracle_vs_lapack(oracle, lapack, name):
    d = live_cases()[name]
    compare(run_all(oracle, d), run_all(lapack, d), d, name)


def weight_edge_inputs():
    """src/DESeq2.cpp:39-43: rows with weight <= threshold are dropped from the Cox-Reid matrix, then the
    design columns that are left all-zero.  Every observation weighted out (a 0 x 0 matrix, det = 1), a single
    observation left, a design column that loses all its samples."""
    from deseq2_amd import simulate
    from tests.helpers import beta_init_qr
    m, n, p = 16, 30, 4
    x = simulate.design_batch_condition(m)
    rng = np.random.default_rng(6)
    y = rng.negative_binomial(2.0, 0.05, size=(n, m)).astype(float)
    w = rng.uniform(0.0, 1.0, (n, m))
    w[0] = 0.0
    w[1, 1:] = 0.0
    w[2, x[:, 1] == 1] = 0.0
    w[3] = 1.0
    alpha = rng.uniform(0.05, 1.0, n)
    nf = np.ones((n, m))
    bargs = (y, x, nf, alpha, np.r_[1.0, 0, 0, 0], beta_init_qr(y, nf, x), np.full(p, 1e-6) / np.log(2) ** 2, w, True,
             1e-8, 100, True, 0.5)
    return y, x, nf, w, alpha, bargs


def check_weight_subsetting_edge_cases(oracle, other):
    """the oracle against `other` (the LAPACK restatement here, the reference build in tests/test_oracle_vs_reference.py) on
    weight_edge_inputs()"""
    y, x, nf, w, alpha, bargs = weight_edge_inputs()
    n = y.shape[0]
    ob, rb = oracle.fitBeta(*bargs), other.fitBeta(*bargs)
    np.testing.assert_array_equal(ob["iter"], rb["iter"])
    ok = rb["iter"] < 100
    np.testing.assert_allclose(ob["beta_mat"][ok], rb["beta_mat"][ok], rtol=1e-7, atol=1e-10)
    mu = np.where(np.isfinite(oracle.fittedMu(x, nf, ob["beta_mat"], 0.5)), oracle.fittedMu(x, nf, ob["beta_mat"], 0.5), 0.5)
    la = np.log(alpha)
    for prior in (False, True):
        dargs = (y, x, mu, la, la - 0.1, 0.8, np.log(1e-9), 1.0, 1e-6, 100, prior, np.maximum(w, 1e-6), True, 1e-2, True)
        od, rd = oracle.fitDisp(*dargs), other.fitDisp(*dargs)
        # gene 2: the Cox-Reid matrix is singular after the subsetting (det = rounding noise in both)
        ok = np.isfinite(rd["initial_lp"]) & np.isfinite(od["initial_lp"]) & (np.arange(n) != 2)
        for k in FLAGS:
            np.testing.assert_array_equal(od[k][ok], rd[k][ok], err_msg="fitDisp$" + k)
        for k in ("log_alpha", "initial_lp", "initial_dlp", "last_lp", "last_d2lp"):
            np.testing.assert_allclose(od[k][ok], rd[k][ok], rtol=1e-7, atol=1e-9, err_msg="fitDisp$" + k)


def test_weight_subsetting_edge_cases(oracle, lapack):
    check_weight_subsetting_edge_cases(oracle, lapack)


def sweep_case(seed):
    """random shapes / designs / weights / ridge / QR / CR settings"""
    rng = np.random.default_rng(9000 + seed)
    designs = ["two_group", "batch_condition", ("factor", 3), ("factor", 5), ("factor", 7), ("factor", 10)]
    dz = designs[rng.integers(len(designs))]
    pmin = {"two_group": 2, "batch_condition": 4}.get(dz, dz[1] if isinstance(dz, tuple) else 2)
    m = int(rng.integers(max(pmin + 2, 6), 120))
    n = int(rng.integers(30, 80))
    kw = dict(weights=bool(rng.uniform() < 0.5), useQR=bool(rng.uniform() < 0.6), useCR=bool(rng.uniform() < 0.8),
              lam=float(10 ** rng.uniform(-6, 0)))
    if kw["weights"] and rng.uniform() < 0.5:
        kw["zero_w"] = True
    return _case(n, m, dz, seed=int(rng.integers(1e6)), **kw)


@pytest.mark.parametrize("seed", range(12))
def test_seeded_sweep(oracle, lapack, seed):
    """random shapes / designs / weights / ridge / QR / CR settings"""
    d = sweep_case(seed)
    compare(run_all(oracle, d), run_all(lapack, d), d, "sweep%d" % seed)


# ---- designs of 11 to 64 columns (tests/wide_cases.py) -----------------------------------------------------------------
from tests import wide_cases   # noqa: E402


@pytest.fixture(scope="module")
def wide_runs(oracle, lapack):
    """(case, oracle results, LAPACK results) of a wide case, computed once for the tests of this module that need it"""
    done = {}

    def get(name):
        if name not in done:
            d = wide_cases.expanded_case(name) if name in wide_cases.EXPANDED else wide_cases.wide_case(name)
            done[name] = (d, run_all(oracle, d), run_all(lapack, d))
        return done[name]
    return get


@pytest.mark.parametrize("name", sorted(wide_cases.WIDE))
def test_oracle_vs_lapack_wide(wide_runs, name):
    """11 <= p <= 64: factors either side of the last cell-collapsed width, paired designs, a factor with a continuous
    covariate at the summation-order boundaries of include/dsq_arith_spec.h -- the budgets of compare() as they stand (value
    tolerances at scale 1, fitBeta$iter equal on every gene, ties <= max(1, 1 %), grid agreement >= 0.95); the share of
    well-conditioned genes, a property of the inputs, is at least wide_cases.MIN_WELL (measured: profiles/wide_parity.md)"""
    d, got, ref = wide_runs(name)
    assert 11 <= d["x"].shape[1] <= 64
    compare(got, ref, d, name, min_well=wide_cases.MIN_WELL)


@pytest.mark.parametrize("name", wide_cases.EXPANDED)
def test_oracle_vs_lapack_expanded_prior_wide(wide_runs, name):
    """betaPrior pass 2 on the expanded design of a factor of 12 / 20 / 47 / 63 levels (p = 13, 21, 48, 64; rank
    deficient), QR and normal equations: iterations equal on every gene and values at scale 1 -- not the 10 x compare()
    grants the three-column expanded design of C5"""
    d, got, ref = wide_runs(name)
    assert d["x_expanded"].shape[1] == d["x"].shape[1] + 1 and np.linalg.matrix_rank(d["x_expanded"]) == d["x"].shape[1]
    compare(got, ref, d, name, min_well=wide_cases.MIN_WELL)
    _fit_beta_compare(got["fitBetaPrior"], ref["fitBetaPrior"], name, "fitBetaPrior", 1.0)


def _copy(res):
    return {fn: {k: (np.array(v, copy=True) if v is not None else None) for k, v in r.items()} for fn, r in res.items()}


def _steady_gene(d, got, ref):
    """a gene on which every strict check of compare() applies: fitBeta converged, well conditioned in both searches, the
    last accepted step far from an ulp-level tie, a dispersion away from 1 and from the floor, the grid results equal"""
    ok = (ref["fitBeta"]["iter"] < 100) & (d["alpha_init"] > 1e-6)
    for fn in ("fitDispMLE", "fitDispMAP"):
        for r in (got[fn], ref[fn]):
            ok &= (np.exp(r["log_alpha"]) > 1e-5) & np.isfinite(r["initial_lp"]) & (np.abs(r["log_alpha"]) > 0.1)
            ok &= np.abs(r["last_change"]) > 1e4 * np.spacing(np.abs(ref[fn]["last_lp"]))
        ok &= (got[fn]["iter"] == ref[fn]["iter"]) & (ref[fn]["iter"] < 99)
    gg, rg = got["fitDispGrid"]["log_alpha"], ref["fitDispGrid"]["log_alpha"]
    ok &= (gg == rg) & (np.exp(rg) > 1e-5)
    assert ok.sum() >= 5, "the case has no gene to mutate"
    return int(np.flatnonzero(ok)[2])


@pytest.mark.parametrize("name", ["paired30_qr", "cont_p31_m124"])
def test_wide_comparison_has_teeth(wide_runs, name):
    """the oracle's own output on a paired and on a factor-plus-covariate case, one entry changed at a time by a few times
    the tolerance it is held to (or one count by one): compare() must refuse each, and pass the unchanged output"""
    d, got, ref = wide_runs(name)
    compare(got, ref, d, name, min_well=wide_cases.MIN_WELL)
    g = _steady_gene(d, got, ref)
    grid = np.linspace(np.log(1e-8), np.log(max(10, d["counts"].shape[1])), 20)      # run_all's grid
    fine_step = 2 * (grid[1] - grid[0]) / (grid.size - 1)      # the second pass: 20 points over +- one step of the first

    def bump_iter(r): r["fitBeta"]["iter"][g] += 1
    def beta_row(r): r["fitBeta"]["beta_mat"][g] *= 1 + 3e-7
    def var_column(r): r["fitBeta"]["beta_var_mat"][:, -1] *= 1 + 3e-7
    def hat_row(r): r["fitBeta"]["hat_diagonals"][g] *= 1 + 3e-8
    def deviance(r): r["fitBeta"]["deviance"][g] *= 1 + 3e-8
    def map_iter(r): r["fitDispMAP"]["iter"][g] += 1
    def mle_log_alpha(r): r["fitDispMLE"]["log_alpha"][g] += 3e-7 * abs(r["fitDispMLE"]["log_alpha"][g])
    def last_lp(r): r["fitDispMLE"]["last_lp"][g] *= 1 + 3e-8
    def grid_neighbour(r): r["fitDispGrid"]["log_alpha"][g] += fine_step

    for mutate in (bump_iter, beta_row, var_column, hat_row, deviance, map_iter, mle_log_alpha, last_lp, grid_neighbour):
        m = _copy(got)
        mutate(m)
        try:
            compare(m, ref, d, "%s with %s" % (name, mutate.__name__), min_well=wide_cases.MIN_WELL)
        except AssertionError:
            continue
        pytest.fail("compare() accepted the mutation %s of gene %d" % (mutate.__name__, g))
