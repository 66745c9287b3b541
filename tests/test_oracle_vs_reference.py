"""CPU: the C oracle and the LAPACK restatement against the reference's own compiled source.

oracle/deseq2_oracle.c (which the HIP kernels equal bit for bit) and oracle/lapack_oracle.py are two restatements of the
reference's src/DESeq2.cpp by readers of the same text: a reading error both share -- a convergence test, a detail of the
Armijo rule, a Cox-Reid term, which rows `weights > threshold` keeps -- leaves them in agreement with each other.  This file
holds both to outputs of src/DESeq2.cpp ITSELF, compiled where it lies against the stand-in headers of oracle/shim/
(oracle/Makefile, target `ref`).  That build is the reference's control flow -- the IRLS loop, the line search, the posterior
and its derivatives, the weight subsetting, the grid search -- over stand-in dense linear algebra and binary128 special
functions; it is not R's nmath and not Armadillo's LAPACK, which is the half tests/test_oracle_vs_lapack.py covers.

  golden layer   tests/golden/reference/<case>.npz (tests/reference_cases.py, written by tests/golden/make_reference_golden.py):
                 always runs, needs no reference tree and no library.
  live layer     when oracle/_ref/libdeseq2_ref.so is there and loads: the recorded files are regenerated bit for bit, and the
                 cases of tests/test_oracle_vs_lapack.py that are too many or too large to record run against the library.

Budgets: those of compare() and assert_visible_parity() as they stand (iteration and accept counts equal, ties <= 1 %, grid
agreement >= 0.95, values within 1e-7 / 1e-8, the well-conditioned share at least wide_cases.MIN_WELL = 0.9 on the wide cases,
0.95 on the narrow ones, 0.8 at m <= 12); measured rates: profiles/reference_parity.md."""
import numpy as np
import pytest

from oracle import reference
from tests import reference_cases as RC
from tests import test_oracle_vs_lapack as T
from tests import wide_cases

NAMES = list(RC.kinds())
live = pytest.mark.skipif(not reference.available(), reason=reference.why_not() or "-")


@pytest.fixture(scope="module")
def lapack():
    from oracle import lapack_oracle
    return lapack_oracle


@pytest.fixture(scope="module")
def recorded():
    """(case, recorded reference result) by name, read once"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = (RC.build(name), RC.load(name))
        return done[name]
    return get


@pytest.fixture(scope="module")
def oracle_runs(oracle, recorded):
    """the C oracle's result of a recorded case, computed once for the tests of this module that need it"""
    done = {}

    def get(name):
        if name not in done:
            done[name] = RC.run(oracle, name, recorded(name)[0])
        return done[name]
    return get


# ---- golden layer --------------------------------------------------------------------------------------------------------

def test_every_case_is_recorded():
    """the six narrow golden cases, every name of wide_cases.WIDE / EXPANDED / FLOOR and the floor seeds 5, 6, 7 each have
    their file, no file is larger than the largest fixture there was before them, and the matrices hold G_HEAD >= 16 genes"""
    import os
    kinds = RC.kinds()
    assert set(T.golden_cases()) | set(wide_cases.WIDE) | set(wide_cases.EXPANDED) | set(wide_cases.FLOOR) | {
        "floor_seed5", "floor_seed6", "floor_seed7"} == set(kinds)
    assert RC.G_HEAD >= 16
    for name in kinds:
        assert os.path.exists(RC.path(name)), "%s is not recorded: python tests/golden/make_reference_golden.py" % name
        assert os.path.getsize(RC.path(name)) <= RC.MAX_FILE_BYTES, name
    assert sorted(os.listdir(RC.DIR)) == sorted(n + ".npz" for n in kinds)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_recorded_reference(recorded, oracle_runs, name):
    d, ref = recorded(name)
    RC.check(oracle_runs(name), ref, name, d, "oracle " + name)


@pytest.mark.parametrize("name", NAMES)
def test_lapack_reproduces_recorded_reference(lapack, recorded, name):
    d, ref = recorded(name)
    RC.check(RC.run(lapack, name, d), ref, name, d, "lapack " + name, lapack=True)


def _swap(res, g, h):
    for dd in res.values():
        for v in dd.values():
            if v is not None and np.ndim(v) >= 1 and np.shape(v)[0] > max(g, h):
                v[[g, h]] = v[[h, g]]


@pytest.mark.parametrize("name", ["bc_m24_weights", "cont_p31_m124"])
def test_comparison_with_recorded_reference_has_teeth(recorded, oracle_runs, name):
    """the oracle's own output on a narrow and on a wide case, against the RECORDED reference: one count off by one on a steady
    gene, beta_mat / log_alpha / deviance of that gene nudged by 1e-6 relative, two genes swapped -- each must be refused,
    the unchanged output accepted.  The gene is one whose matrix rows are recorded (g < G_HEAD)."""
    d, ref = recorded(name)
    got = {fn: dd for fn, dd in oracle_runs(name).items() if fn != "aux"}
    RC.check(got, ref, name, d, name)
    full = RC.complete(ref, got)
    g = T._steady_gene(d, got, full)
    assert g < RC.G_HEAD, "the steady gene %d has no recorded matrix rows" % g
    h = g + 1 + int(np.flatnonzero(got["fitBeta"]["iter"][g + 1:] != got["fitBeta"]["iter"][g])[0])

    def beta_iter(r): r["fitBeta"]["iter"][g] += 1
    def mle_iter(r): r["fitDispMLE"]["iter"][g] += 1
    def map_iter(r): r["fitDispMAP"]["iter"][g] -= 1
    def map_accept(r): r["fitDispMAP"]["iter_accept"][g] += 1
    def beta_row(r): r["fitBeta"]["beta_mat"][g] *= 1 + 1e-6
    def mle_log_alpha(r): r["fitDispMLE"]["log_alpha"][g] *= 1 + 1e-6
    def map_log_alpha(r): r["fitDispMAP"]["log_alpha"][g] *= 1 + 1e-6
    def deviance(r): r["fitBeta"]["deviance"][g] *= 1 + 1e-6
    def swap_genes(r): _swap(r, g, h)

    for mutate in (beta_iter, mle_iter, map_iter, map_accept, beta_row, mle_log_alpha, map_log_alpha, deviance, swap_genes):
        m = T._copy(got)
        mutate(m)
        try:
            RC.check(m, ref, name, d, "%s with %s" % (name, mutate.__name__))
        except AssertionError:
            continue
        pytest.fail("the comparison accepted the mutation %s of gene %d" % (mutate.__name__, g))


# ---- the fixtures cannot rot ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def regenerated(recorded):
    """what the library writes today for every recorded case, computed once on a few threads (the library's routines keep no
    state between calls and ctypes releases the interpreter lock while they run)"""
    import os
    from concurrent.futures import ThreadPoolExecutor
    workers = max(1, min(8, len(os.sched_getaffinity(0))))
    by_cost = sorted(NAMES, key=lambda n: -recorded(n)[0]["counts"].size * recorded(n)[0]["x"].shape[1])
    with ThreadPoolExecutor(workers) as pool:
        packs = list(pool.map(lambda n: RC.pack(n, RC.run(reference, n, recorded(n)[0])), by_cost))
    return dict(zip(by_cost, packs))


@live
@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_current(regenerated, name):
    """the library regenerates the recorded file bit for bit: same keys, shapes, types and bytes"""
    now = regenerated[name]
    with np.load(RC.path(name)) as z:
        then = {k: z[k] for k in z.files}
    hint = "%s is not what the reference build writes today: rerun python tests/golden/make_reference_golden.py" % name
    assert sorted(now) == sorted(then), hint
    for k, v in now.items():
        assert v.dtype == then[k].dtype and v.shape == then[k].shape, "%s (%s)" % (hint, k)
        assert v.tobytes() == then[k].tobytes(), "%s (%s)" % (hint, k)


# ---- live layer ----------------------------------------------------------------------------------------------------------

@live
@pytest.mark.parametrize("name", sorted(set(T.live_cases()) - set(RC.NARROW)))
def test_oracle_vs_reference_live(oracle, name):
    """the cases of test_oracle_vs_lapack.live_cases() that are not recorded"""
    d = T.live_cases()[name]
    T.compare(T.run_all(oracle, d), T.run_all(reference, d), d, name)


@live
@pytest.mark.parametrize("seed", range(12))
def test_seeded_sweep_vs_reference(oracle, seed):
    """the inputs of test_oracle_vs_lapack.test_seeded_sweep: random shapes / designs / weights / ridge / QR / CR settings"""
    d = T.sweep_case(seed)
    T.compare(T.run_all(oracle, d), T.run_all(reference, d), d, "sweep%d" % seed)


@live
def test_weight_subsetting_edge_cases_vs_reference(oracle):
    """the inputs and assertions of test_oracle_vs_lapack.test_weight_subsetting_edge_cases (src/DESeq2.cpp:39-43: every
    observation weighted out, a single observation left, a design column that loses all its samples)"""
    T.check_weight_subsetting_edge_cases(oracle, reference)


def _scalars_run(F, d, tol_beta, maxit_beta, minmu, kappa_0, tol_disp, maxit_disp, min_log_alpha, sigmasq, thr):
    """run_all's call sequence with every scalar argument of the three routines passed in"""
    y, x, nf, w = d["counts"].astype(float), d["x"], d["nf"], d["weights"]
    p = x.shape[1]
    beta = F.fitBeta(y, x, nf, d["alpha_init"], np.r_[0.0, 1.0], d["beta_init"], d["lam"], w, True, tol_beta, maxit_beta,
                     True, minmu)
    mu = np.maximum(nf * np.exp(beta["beta_mat"] @ x.T), minmu)
    la0 = np.log(d["alpha_init"])
    wd = np.maximum(w, 1e-6)
    mle = F.fitDisp(y, x, mu, la0, la0, sigmasq, min_log_alpha, kappa_0, tol_disp, maxit_disp, False, wd, True, thr, True)
    mp = F.fitDisp(y, x, mu, la0 + 0.3, la0 - 0.2, sigmasq, min_log_alpha, kappa_0, tol_disp, maxit_disp, True, wd, True,
                   thr, True)
    grid = np.linspace(np.log(1e-8), np.log(10.0), 15)
    gr = F.fitDispGrid(y, x, mu, grid, la0 - 0.2, sigmasq, True, wd, True, thr, True)
    assert p == 2
    return {"fitBeta": beta, "fitDispMLE": mle, "fitDispMAP": mp, "fitDispGrid": gr}


@live
def test_every_scalar_argument_vs_reference(oracle):
    """an input the recorded files cannot hold (their call sequence fixes the scalars): two groups at m = 6 with weights,
    minmu = 2 (a floor the fitted means of the low genes reach), tol, maxit and kappa_0 of both routines, the prior variance,
    the floor of log alpha and the weight threshold all away from their defaults, the contrast on the second coefficient.
    The oracle follows the reference under compare(); and each setting is seen to matter: the same inputs at the default
    scalars give other iteration counts."""
    d = T._case(300, 6, "two_group", 4106, weights=True)
    away = dict(tol_beta=1e-5, maxit_beta=5, minmu=2.0, kappa_0=0.3, tol_disp=1e-4, maxit_disp=40,
                min_log_alpha=np.log(1e-7), sigmasq=2.5, thr=0.3)
    default = dict(tol_beta=1e-8, maxit_beta=100, minmu=0.5, kappa_0=1.0, tol_disp=1e-6, maxit_disp=100,
                   min_log_alpha=np.log(1e-9), sigmasq=1.0, thr=1e-2)
    got, ref = _scalars_run(oracle, d, **away), _scalars_run(reference, d, **away)
    T.compare(got, ref, d, "scalars away from their defaults")
    base = _scalars_run(reference, d, **default)
    assert (base["fitBeta"]["iter"] != ref["fitBeta"]["iter"]).any()
    assert (base["fitDispMLE"]["iter"] != ref["fitDispMLE"]["iter"]).mean() > 0.2
    for k, v in away.items():          # one scalar at a time back at its default: the reference's own result moves
        one = _scalars_run(reference, d, **dict(away, **{k: default[k]}))
        same = all(np.array_equal(np.asarray(one[fn][q]), np.asarray(ref[fn][q]), equal_nan=True)
                   for fn in one for q in one[fn])
        assert not same, "the reference's result does not depend on %s at these inputs" % k
