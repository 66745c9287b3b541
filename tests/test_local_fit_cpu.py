"""fitType = "local" on the CPU: HostEngine.local_fit equals the numpy specification of
tests/local_fit_spec.py BIT FOR BIT on every case of tests/local_fit_cases.py; the specification is held to a 50-digit
mpmath weighted least squares of the same estimator that shares no arithmetic with it, within a bound derived from each
point's measured condition number; data on an exact quadratic is reproduced to that bound inside and outside the range; the
window bisection equals the sort-based k-th distance; the C ABI decides its argument errors before a device is asked for;
and the Python surface: estimateDispersions(fitType = "local") through the MAP step (the reference's
test_dispersions.R:117), the opt-in substitution for a parametric trend that does not fit, vst's spline path.

The bound.  With u = 2^-53, kappa the 2-norm condition number of the 3 x 3 normal matrix in t and |a| the largest
coefficient in that basis, the intercept is held to
    (ceil(k / LANES) + 6 + 30) u kappa max(1, |a|)  +  2 u (1 + |a0|):
ceil(k / LANES) + 6 is the depth of the specification's summation (a lane's sequential additions, then six butterfly
steps), i.e. the constant of the forward error of every moment relative to the sum of its terms' magnitudes; 30 covers the
roundings of t, of the tricube weight and its powers (about a dozen per term) and of the 17 operations of the elimination,
which is backward stable on a positive definite matrix without pivoting; kappa carries a relative perturbation of the
matrix and the right-hand side to the solution.  The last term is the rounding of the pinned exponential and of its
argument.  Nothing in it comes from the values the code gives.  It is a worst-case bound; measured on these cases
(profiles/local_fit.md): kappa up to 3.7e4, the observed error at most 0.0047 of the bound (a margin of 210)."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

from tests import local_fit_cases as CS
from tests import local_fit_spec as S
from tests.helpers import assert_bits

from deseq2_amd import core, local_fit_host, simulate
from deseq2_amd.engine import HostEngine

U = 2.0 ** -53


@pytest.fixture(scope="module")
def E(oracle):
    return HostEngine(oracle)


# ---------------------------------------------------------------------------------------------- bitwise: host engine == spec
@pytest.mark.parametrize("fit_name,which", CS.PAIRS)
def test_host_engine_equals_the_specification(E, oracle, fit_name, which):
    ref, nsing, fit = CS.reference(oracle, fit_name, which)
    f = E.local_fit(*CS.FIT_SETS[fit_name], CS.MIN_DISP)
    assert (f.N, f.k) == (fit[0].size, fit[3]) and f.allBelowFloor == (fit[0].size == 0)
    assert_bits(f(CS.eval_list(fit_name, which)), ref, "%s / %s" % (fit_name, which))
    assert f.nSingular == nsing


def test_what_the_cases_are_meant_to_hit(oracle):
    assert S.LANES == local_fit_host.LANES == CS.LANES
    n = {k: S.fit_set(oracle, *v, CS.MIN_DISP)[0].size for k, v in CS.FIT_SETS.items()}
    assert (n["n5"], n["n63"], n["n65"], n["mixed"], n["all_below"]) == (5, CS.LANES - 1, CS.LANES + 1, 58, 0)
    assert S.bandwidth(5) == 3 and S.bandwidth(4) == 2 and S.bandwidth(10) == 7 and S.bandwidth(60000) == 42000
    # rows below the floor, the NaN and the zero mean are not in the fit set; the row exactly at the floor is
    rows = S.fit_set(oracle, *CS.FIT_SETS["mixed"], CS.MIN_DISP)[3]
    assert 7 in rows and not set(rows) & ({4, 10} | set(range(0, 90, 3)))
    # k = 3: the third nearest point sits at distance h and has weight 0, so every point is singular -- and counted
    ref, nsing, _ = CS.reference(oracle, "n5", "n65")
    assert np.isnan(ref).all() and nsing == 65
    ref, nsing, _ = CS.reference(oracle, "all_equal", "n65")
    assert np.isnan(ref).all() and nsing == 65
    # all below the floor: the constant, also where the mean has no logarithm
    ref, nsing, _ = CS.reference(oracle, "all_below", "special")
    assert (ref == CS.MIN_DISP).all() and nsing == 0
    # NaN, 0, negative and infinite means give NaN and are not counted as singular
    ref, nsing, _ = CS.reference(oracle, "n300", "special")
    # (the quadratic extrapolated to 1e-300 and 1e300 overflows the exponential: Inf, not NaN)
    assert np.isnan(ref[-5:]).all() and np.isfinite(ref[:7]).all() and not np.isnan(ref[7:9]).any() and nsing == 0
    # the tie case: some window edge cuts a run of equal x
    x, _, _, k, _ = CS.reference(oracle, "ties", "n65")[2]
    zs = oracle.unary("log", CS.eval_list("ties", "n65"))
    ls = [S.window_start(x, k, z) for z in zs]
    assert any(l + k < x.size and x[l + k] == x[l + k - 1] for l in ls)


@pytest.mark.parametrize("name", sorted(CS.TOO_FEW))
def test_fewer_than_three_points_in_a_window_raises(E, oracle, name):
    means, disps = CS.TOO_FEW[name]
    with pytest.raises(RuntimeError, match="fewer than 3 points in a window"):
        S.local_fit(oracle, means, disps, CS.MIN_DISP)
    with pytest.raises(RuntimeError, match="fewer than 3 points in a window"):
        E.local_fit(means, disps, CS.MIN_DISP)


# ---------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("fit_name", [f for f in CS.FIT_SETS if f != "all_below"])
def test_window_bisection_equals_the_sorted_kth_distance(oracle, fit_name):
    x, _, _, k, _ = CS.reference(oracle, fit_name, "special")[2]
    for which in ("n65", "special"):
        q = CS.eval_list(fit_name, which)
        with np.errstate(invalid="ignore"):
            q = q[(q > 0) & (q < np.inf)]
        for z in oracle.unary("log", q):
            l = S.window_start(x, k, z)
            assert 0 <= l <= x.size - k
            assert S.bandwidth_h(x, k, z, l) == np.sort(np.abs(x - z))[k - 1], (fit_name, which, z)


# ---------------------------------------------------------------------------------------------- the independent statement
def _mp_intercept(mp, x, y, w, k, z):
    """the local quadratic fit at z in 50 digits: the k-th smallest distance over ALL points, tricube weights, least squares
    on 1, (x - z), (x - z)^2 by LU; None where it does not exist"""
    X, Y, Wt, Z = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in y], [mp.mpf(float(v)) for v in w], mp.mpf(float(z))
    h = sorted(abs(v - Z) for v in X)[k - 1]
    if h == 0:
        return None
    A, b = mp.zeros(3, 3), mp.zeros(3, 1)
    seen = set()
    for xv, yv, wv in zip(X, Y, Wt):
        t = abs(xv - Z) / h
        if t >= 1:
            continue
        W = wv * (1 - t ** 3) ** 3
        seen.add(xv)
        d = xv - Z
        for r in range(3):
            b[r] += W * d ** r * yv
            for c in range(3):
                A[r, c] += W * d ** (r + c)
    if len(seen) < 3:
        return None
    return mp.lu_solve(A, b)[0]


def _bound(x, y, w, k, z, a0):
    m, _, _ = S.moments(x, y, w, k, z)
    G = np.array([[m[0], m[1], m[2]], [m[1], m[2], m[3]], [m[2], m[3], m[4]]])
    kappa = np.linalg.cond(G)
    a = np.abs(np.linalg.solve(G, m[5:])).max()
    return (math.ceil(k / S.LANES) + 36) * U * kappa * max(1.0, a) + 2 * U * (1 + abs(a0)), kappa


def _hold_to_mpmath(oracle, fit, q, what, expect=None):
    """every finite value of the specification against the 50-digit statement (or `expect`, a function of z); returns
    (largest kappa, largest error / bound)"""
    mp.mp.dps = 50
    x, y, w, k, _ = fit
    out, _ = S.evaluate(oracle, fit, q)
    worst, kmax = 0.0, 0.0
    for v, z in zip(out, oracle.unary("log", q)):
        ref = _mp_intercept(mp, x, y, w, k, z) if expect is None else expect(mp, z)
        if ref is None:
            assert np.isnan(v), (what, z)
            continue
        assert np.isfinite(v), (what, z)
        err = float(abs(mp.log(mp.mpf(float(v))) - ref))
        bound, kappa = _bound(x, y, w, k, z, float(ref))
        worst, kmax = max(worst, err / bound), max(kmax, kappa)
        assert err <= bound, "%s at z = %r: error %.3g over the bound %.3g (kappa %.3g)" % (what, z, err, bound, kappa)
    print("%s: kappa up to %.3g, error / bound at most %.3g" % (what, kmax, worst))
    return kmax, worst


@pytest.mark.parametrize("fit_name", ["n20", "n63", "n64", "n65", "n129", "n300", "n1000", "ties", "mixed", "weights", "all_equal", "n5"])
def test_the_specification_against_50_digit_least_squares(oracle, fit_name):
    fit = CS.reference(oracle, fit_name, "special")[2]
    q = np.concatenate([CS.eval_list(fit_name, "n65")[:10], CS.eval_list(fit_name, "special")[:7]])
    _hold_to_mpmath(oracle, fit, q, fit_name)


def test_a_mutated_weight_is_refused(oracle):
    """what the comparison must not let pass: a tricube with the wrong outer power"""
    mp.mp.dps = 50
    x, y, w, k, _ = CS.reference(oracle, "n129", "n65")[2]
    z = float(oracle.unary("log", CS.eval_list("n129", "n65")[:1])[0])
    good = _mp_intercept(mp, x, y, w, k, z)
    h = np.sort(np.abs(x - z))[k - 1]
    t = np.abs(x - z) / h
    W = np.where(t < 1, w * (1 - t ** 3) ** 2, 0.0)
    mutant = np.polynomial.polynomial.polyfit(x - z, y, 2, w=np.sqrt(W))[0]
    assert abs(mutant - float(good)) > 1e3 * _bound(x, y, w, k, z, float(good))[0]


@pytest.mark.parametrize("N,seed", [(40, 1), (129, 2), (500, 3)])
def test_an_exact_quadratic_is_reproduced(oracle, N, seed):
    """y = c0 + c1 x + c2 x^2 exactly (rounded once): the local quadratic fit returns it at every z, inside the range and
    outside, where the window is one-sided and kappa grows -- the bound grows with it"""
    mp.mp.dps = 50
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.sort(rng.uniform(0.0, 9.0, N))
    c = (-1.25, -0.75, 0.0625)
    quad = lambda mp_, z: c[0] + c[1] * mp_.mpf(float(z)) + c[2] * mp_.mpf(float(z)) ** 2
    y = np.array([float(quad(mp, v)) for v in x])
    fit = (x, y, np.exp(rng.uniform(0.0, 9.0, N)), S.bandwidth(N), CS.MIN_DISP)
    q = np.exp(np.concatenate([rng.uniform(0.0, 9.0, 12), [x[0], x[-1], -0.5, -2.0, 9.5, 11.0]]))
    _hold_to_mpmath(oracle, fit, q, "quadratic, N = %d" % N, expect=quad)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_the_entry_points_check_their_arguments():
    """dsq_local_fit[_dev] decide their argument errors before a device is asked for (1 = DSQ_ERR_ARG) and launch nothing"""
    from deseq2_amd import _lib as L
    lib = L.lib()
    n = 6
    means, disps, ev = np.ones(n), np.ones(n), np.ones(3)
    block, out, st = np.zeros(4 + 3 * n), np.zeros(n), np.zeros(4, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def args(**kw):
        d = dict(n=n, means=P(means), disps=P(disps), minDisp=1e-8, fit_in=None, n_eval=0, eval_means=None)
        d.update(kw)
        return L.sized(L.DsqLocalFitArgs, **d)

    def outs(**kw):
        d = dict(fit=P(block), dispFit=P(out), status=P(st))
        d.update(kw)
        return L.sized(L.DsqLocalFitOut, **d)

    for call in (lambda a, o: lib.dsq_local_fit(C.byref(a), C.byref(o)), lambda a, o: lib.dsq_local_fit_dev(C.byref(a), C.byref(o), None)):
        assert call(args(n=0), outs()) == 1 and call(args(means=None), outs()) == 1 and call(args(disps=None), outs()) == 1
        assert call(args(), outs(status=None)) == 1 and b"status" in lib.dsq_last_error()
        assert call(args(minDisp=0.0), outs()) == 1 and call(args(minDisp=float("nan")), outs()) == 1
        assert call(args(n_eval=3), outs()) == 1 and call(args(eval_means=P(ev), n_eval=0), outs()) == 1 and b"n_eval" in lib.dsq_last_error()
        assert call(args(n_eval=-1), outs()) == 1
        assert call(args(eval_means=P(ev), n_eval=3), outs(dispFit=None)) == 1
        assert call(args(fit_in=P(block), means=None, disps=None), outs()) == 1 and b"fit_in" in lib.dsq_last_error()
        bad = args()
        bad.struct_size += 8
        assert call(bad, outs()) == 1 and b"struct_size" in lib.dsq_last_error()
        bad = outs()
        bad.struct_size -= 4
        assert call(args(), bad) == 1
    assert (block == 0).all() and (out == 0).all() and (st == 0).all()          # nothing was written
    assert lib.dsq_local_fit_lanes() == S.LANES
    assert lib.dsq_local_fit_block_doubles(n) == 4 + 3 * n and lib.dsq_local_fit_block_doubles(0) == 0


# ---------------------------------------------------------------------------------------------- the Python surface
@pytest.fixture(scope="module")
def example(oracle):
    x = simulate.design_two_group(6)
    d = simulate.make_counts(400, x, seed=3)
    return d, x


def test_estimate_dispersions_local_runs_through_map(example, oracle):
    """the reference's test_dispersions.R:117: estimateDispersions(dds, fitType = "local")"""
    d, x = example
    dds = core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=HostEngine(oracle))
    core.getBaseMeansAndVariances(dds)
    core.estimateDispersions(dds, fitType="local")
    fn = dds.dispersionFunction
    assert fn["fitType"] == "local" and callable(fn["coefficients"]) and fn["varLogDispEsts"] > 0
    mc = dds.mcols
    assert np.isfinite(mc["dispFit"]).all() and (mc["dispFit"] > 0).all()
    assert np.isfinite(mc["dispMAP"]).all() and np.isfinite(mc["dispersion"]).all()
    # the stored function is the fit: it gives dispFit back, bit for bit, and equals the specification on the same genes
    assert_bits(fn["coefficients"](mc["baseMean"]), mc["dispFit"], "dispFit")
    use = mc["dispGeneEst"] > 100 * 1e-8
    ref = S.evaluate(oracle, S.local_fit(oracle, mc["baseMean"][use], mc["dispGeneEst"][use], 1e-8), mc["baseMean"])[0]
    assert_bits(mc["dispFit"], ref, "dispFit against the specification")
    f2 = core.localDispersionFit(dds, mc["baseMean"][use], mc["dispGeneEst"][use], 1e-8)
    assert_bits(f2(mc["baseMean"][:50]), mc["dispFit"][:50], "localDispersionFit")
    # the true trend is 0.1 + 4 / mean (simulate.make_counts): the local fit follows it where the data are dense
    lo, hi = np.quantile(mc["baseMean"], [.25, .75])
    mid = (mc["baseMean"] > lo) & (mc["baseMean"] < hi)
    truth = 0.1 + 4.0 / mc["baseMean"][mid]
    assert np.median(np.abs(np.log(mc["dispFit"][mid] / truth))) < 0.5


def test_deseq_local_and_the_strings_every_entry_accepts(example, oracle):
    d, x = example
    dds = core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=HostEngine(oracle))
    core.DESeq(dds, fitType="local")
    assert dds.dispersionFunction["fitType"] == "local" and np.isfinite(dds.mcols["WaldPvalue"][:, 1]).all()
    with pytest.raises(ValueError, match="fitType"):
        core.estimateDispersionsFit(dds, fitType="glmGamPoi")
    with pytest.raises(ValueError, match="parametricFallback"):
        core.estimateDispersionsFit(dds, parametricFallback="parametric")
    rl = core.rlog(d["counts"][:60], fitType="local", engine=HostEngine(oracle))
    assert rl.dds.dispersionFunction["fitType"] == "local" and np.isfinite(np.asarray(rl.assay())).all()


def test_parametric_fallback_local_is_opt_in(oracle, capsys):
    """a parametric trend that does not fit: "mean" by default (unchanged), the reference's substitution and its message with
    parametricFallback = "local"; the fitted trend rises with the mean as the simulated truth does"""
    x = simulate.design_two_group(12)
    counts = simulate.make_counts_trend_fails(500, x, seed=5)
    E = HostEngine(oracle)
    dds = core.DESeqDataSet(counts, x, sizeFactors=np.ones(12), engine=E)
    core.getBaseMeansAndVariances(dds)
    core.estimateDispersionsGeneEst(dds)
    core.estimateDispersionsFit(dds)
    assert dds.dispersionFunction["fitType"] == "mean" and capsys.readouterr().err == ""
    core.estimateDispersionsFit(dds, parametricFallback="local")
    assert dds.dispersionFunction["fitType"] == "local"
    assert "a local regression fit was automatically substituted" in capsys.readouterr().err
    lo, hi = np.quantile(dds.mcols["baseMean"], [.05, .95])
    grid = np.exp(np.linspace(np.log(lo), np.log(hi), 40))
    vals = dds.dispersionFunction["coefficients"](grid)
    assert (np.diff(vals) > 0).all(), vals
    # core.DESeq hands the choice through
    dds2 = core.DESeqDataSet(counts, x, sizeFactors=np.ones(12), engine=E)
    core.DESeq(dds2, parametricFallback="local")
    assert dds2.dispersionFunction["fitType"] == "local"
    assert_bits(dds2.mcols["dispFit"], dds.mcols["dispFit"], "dispFit through DESeq")


def test_vst_local_equals_the_spline_path_of_the_same_function(oracle):
    E = HostEngine(oracle)
    x = simulate.design_two_group(6)
    counts = simulate.make_counts(1300, x, seed=8, drop_all_zero=True)["counts"]
    a = core.vst(counts, fitType="local", engine=E)
    b = core.vst(counts, fitType=lambda means, disps: E.local_fit(means, disps, 1e-8), engine=E)
    assert a.dds.dispersionFunction["fitType"] == "local" and b.dds.dispersionFunction["fitType"] == "custom"
    assert_bits(np.asarray(a.assay()), np.asarray(b.assay()), "vst")
    assert np.isfinite(np.asarray(a.assay())).all()
    c = core.varianceStabilizingTransformation(counts[:300], fitType="local", engine=E)
    assert c.dds.dispersionFunction["fitType"] == "local" and np.isfinite(np.asarray(c.assay())).all()


def test_deseq_parallel_fits_the_local_trend_on_the_gathered_vectors(example, oracle):
    """one process, one shard: the gathered vectors are the shard's own, so every column equals core.DESeq's"""
    from deseq2_amd import parallel
    d, x = example
    a = core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=HostEngine(oracle))
    core.DESeq(a, fitType="local")
    b = core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=HostEngine(oracle))
    parallel.DESeqParallel(b, fitType="local")
    assert b.dispersionFunction["fitType"] == "local"
    for k in ("dispFit", "dispMAP", "dispersion", "beta", "betaSE", "WaldStatistic"):
        assert_bits(b.mcols[k], a.mcols[k], k)
