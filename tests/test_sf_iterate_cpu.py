"""estimateSizeFactors(type = "iterate") without a GPU: the host engine's solve against the numpy specification
(tests/sf_iterate_spec.py) bit for bit, the closed-form gradient against differences of the specification's F, the minima
against R's optim call restated through scipy (tests/sf_iterate_lbfgsb.py), the reference's own expectation
(tests/testthat/test_size_factor.R:39-45) through core.estimateSizeFactors, the callers, and the errors."""
import numpy as np
import pytest

from tests import sf_iterate_cases as CS
from tests import sf_iterate_spec as S
from tests.helpers import assert_same
from tests.sf_spec import _exp

KEYS = ("s", "sf", "F", "iter", "evals", "flag")

SOLVE_CASES = {
    "plain": dict(n_rows=100, m=12, seed=1),
    "one row": dict(n_rows=1, m=5, seed=6),
    "two rows": dict(n_rows=2, m=5, seed=7),
    "excluded rows between": dict(n_rows=21, m=5, seed=2, interleave=True),
    "dispersion edges, m = 65": dict(n_rows=131, m=65, seed=3, disp_edges=True),
    "far start": dict(n_rows=60, m=8, seed=33, far=True),
    "pairs of equal rows": dict(n_rows=42, m=6, seed=5, dup=2),
    "four equal rows at the cut": dict(n_rows=20, m=6, seed=8, dup=4),
    "every row tied": dict(n_rows=4, m=6, seed=8, dup=4),
    "past one slice and one round of F": dict(n_rows=1100, m=5, seed=9, interleave=True),
}


def _same(got, want, what):
    for key in KEYS:
        assert_same(got[key], want[key], "%s: %s" % (what, key))


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
def test_host_engine_equals_the_specification(oracle, name):
    from deseq2_amd.engine import HostEngine
    c = CS.solve_case(**SOLVE_CASES[name])
    want = S.solve(oracle, **c)
    got = HostEngine(oracle).sf_iterate_solve(c["counts"], c["mu"], c["sf"], c["disp"], c["rows"])
    _same(got, want, name)
    print("%s: F = %.6f, iter %d, evals %d, flag %d" % (name, want["F"], want["iter"], want["evals"], want["flag"]))
    if name in ("one row", "every row tied"):
        # an empty kept set: quantile(L, Q) is the one L itself, or every row is tied at it (strict ">")
        assert (want["flag"], want["iter"], want["evals"], want["F"]) == (0, 0, 1, 0.0)
        assert_same(want["s"], S.Problem(oracle, **c).start(), "s unchanged")
    elif name == "far start":
        assert want["flag"] == 0 and want["evals"] > want["iter"] + 1          # the Armijo test rejected at least once
    else:
        assert want["flag"] == 0 and want["iter"] >= 1


def test_ties_straddle_the_cut(oracle):
    """pairs of equal rows: the two order statistics around (n' - 1) Q are one pair, the cut is their value, and the strict
    comparison keeps neither"""
    c = CS.solve_case(**SOLVE_CASES["pairs of equal rows"])
    P = S.Problem(oracle, **c)
    L, cut, kept, F = P.evaluate(_exp(oracle, P.start()))
    s = np.sort(L)
    assert s[2] == s[3] == cut and (L == cut).sum() == 2 and not kept[L == cut].any() and kept.sum() == 42 - 4


def test_constants_agree_with_the_library():
    from deseq2_amd import _lib, sf_iterate_host as H
    L = _lib.lib()
    assert L.dsq_sf_iterate_slice_genes() == S.G == H.SLICE_GENES
    assert (S.T, S.MAX_TRIALS, S.ARMIJO, S.RELTOL) == (H.CUT_THREADS, H.MAX_TRIALS, H.ARMIJO, H.RELTOL)
    for sym in ("dsq_sf_iterate", "dsq_sf_iterate_dev", "dsq_sf_iterate_workspace_bytes", "dsq_sf_iterate_slice_genes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    n, m = 131, 65
    slices = -(-n // S.G)
    assert L.dsq_sf_iterate_workspace_bytes(n, m) == 8 * (3 * n + 2 * slices * m + 7 * m) + 64
    assert L.dsq_sf_iterate_workspace_bytes(0, m) == 0


@pytest.mark.parametrize("name", ["plain", "dispersion edges, m = 65", "excluded rows between"])
def test_gradient_and_gauge(oracle, name):
    """g against central differences of the specification's F (no centring: d F / d s_j on the kept set) at points whose
    kept set is the same at s, s + eps e_j and s - eps e_j; sum_j d_j = 0 to rounding.  Bound: the differences of an F of
    size |F| carry eps(double) |F| / (2 eps) of rounding and eps^2 / 6 |F'''| ~ eps^2 |h_j| of truncation."""
    c = CS.solve_case(**SOLVE_CASES[name])
    P = S.Problem(oracle, **c)
    rng = np.random.Generator(np.random.PCG64(77))
    s = P.start() + rng.normal(0.0, 0.05, P.m)
    L, cut, kept, F = P.evaluate(_exp(oracle, s))
    g, h = P.gradient(kept, _exp(oracle, s))
    d, gd = P.step(g, h)
    assert abs(S.serial_sum(d)) <= 8 * np.finfo(float).eps * np.abs(d).sum() * P.m
    assert gd > 0                                                                     # an ascent direction: h > 0
    assert (h > 0).all()
    eps = 1e-4
    checked = 0
    for j in range(P.m):
        up, dn = s.copy(), s.copy()
        up[j] += eps
        dn[j] -= eps
        Lu, _, ku, Fu = P.evaluate(_exp(oracle, up))
        Ld, _, kd, Fd = P.evaluate(_exp(oracle, dn))
        if not ((ku == kept).all() and (kd == kept).all()):
            continue
        checked += 1
        num = (Fu - Fd) / (2 * eps)
        bound = 4 * (np.finfo(float).eps * abs(F) / (2 * eps) + eps * eps * abs(h[j]))
        assert abs(num - g[j]) <= bound, (j, num, g[j], bound)
    assert checked >= P.m // 2


# R's optim call restated through scipy, on inputs where both converge.  max |s - s_scipy| as measured on these cases
# (profiles/sf_iterate.md): 9.1e-6, 2.6e-5, 5.4e-7, 1.0e-5, 1.3e-6; asserted at twice the largest.
SCIPY_CASES = [dict(n_rows=100, m=12, seed=11), dict(n_rows=300, m=12, seed=12), dict(n_rows=400, m=16, seed=13),
               dict(n_rows=200, m=6, seed=14), dict(n_rows=150, m=8, seed=15, far=True)]
DS_MEASURED = 2.622e-5


@pytest.mark.parametrize("kw", SCIPY_CASES, ids=lambda kw: "%dx%d" % (kw["n_rows"], kw["m"]))
def test_minimum_against_the_scipy_restatement(oracle, kw):
    pytest.importorskip("scipy")
    from tests import sf_iterate_lbfgsb as B
    c = CS.solve_case(**kw)
    w = S.solve(oracle, **c)
    b = B.sf_iterate_lbfgsb(**c)
    assert w["flag"] == 0 and b["convergence"] == 0
    fn = B.fn_of(**c)                       # both points on ONE statement of R's fn (scipy's density)
    Fw, Fb = fn(w["s"]), b["F"]
    ds = np.abs(w["s"] - b["s"]).max()
    print("%r: F %.9f, scipy %.9f, (F - F_scipy) / |F| = %.3e; max |s - s_scipy| = %.3e; %d evaluations against %d" %
          (kw, Fw, Fb, (Fw - Fb) / abs(Fb), ds, w["evals"], b["nfev"]))
    assert abs(Fw - w["F"]) <= 1e-9 * abs(Fw)                     # (the two statements of the density agree)
    assert Fw >= Fb - 2.2e-9 * max(abs(Fb), 1.0)                  # factr * eps: optim's own stopping tolerance
    assert 2 * DS_MEASURED < 1e-2 / np.sqrt(kw["m"])              # the resolution of the outer loop's 1e-4 criterion
    assert ds <= 2 * DS_MEASURED


@pytest.mark.parametrize("n", [5, 100])
def test_testthat_iterate_recovers_the_size_factors(oracle, n):
    """test_size_factor.R:20-29, 39-45 with numpy's generator: intercept and slope - 1 of lm(sf ~ true.sf) both below 0.1.
    n = 100 is the reference's own size (4 outer rounds); n = 5 is the smallest gene count at which the outer loop
    converges within 10 rounds on this generator's data (4 rounds; n = 4 does not converge)."""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    cts, true_sf = CS.testthat_case(n)
    dds = core.DESeqDataSet(cts, np.ones((12, 1)), engine=HostEngine(oracle))
    core.estimateSizeFactors(dds, type="iterate", geoMeans=np.ones(3), controlGenes="ignored")     # (R/methods.R:374-375)
    slope, icpt = np.polyfit(true_sf, dds.sizeFactors, 1)
    print("iterate recovery, n = %d: %d rounds, intercept %.4f, slope - 1 %.4f" % (n, dds.attrs["sfIterateRounds"], icpt, slope - 1))
    assert dds.attrs["sfIterateRounds"] == 4
    assert abs(icpt) < .1 and abs(slope - 1) < .1
    assert_same(np.asarray(dds.nf), np.broadcast_to(dds.sizeFactors[None, :], (n, 12)), "the n x m matrix of the factors")
    assert "prefit" not in dds.attrs
    if n == 5:
        with pytest.raises(ValueError, match="did not converge$"):
            core.estimateSizeFactors(core.DESeqDataSet(CS.testthat_case(4)[0], np.ones((12, 1)), engine=HostEngine(oracle)),
                                     type="iterate")


def test_through_the_callers(oracle):
    """DESeq(sfType = "iterate") and vst(sfType = "iterate") equal the two-step call"""
    from deseq2_amd import core, simulate
    from deseq2_amd.engine import HostEngine
    x = simulate.design_two_group(8)
    k = simulate.make_counts(120, x, seed=41)["counts"]
    E = HostEngine(oracle)
    one = core.DESeq(core.DESeqDataSet(k, x, engine=E), sfType="iterate")
    two = core.DESeq(core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=E), type="iterate"))
    assert_same(one.sizeFactors, two.sizeFactors, "DESeq: sizeFactors")
    assert not np.array_equal(one.sizeFactors, np.ones(8))
    for key in ("dispersion", "log2FoldChange" if "log2FoldChange" in one.mcols else "dispMAP"):
        assert_same(one.mcols[key], two.mcols[key], "DESeq: " + key)
    v1 = core.vst(k, nsub=60, engine=E, sfType="iterate")
    v2 = core.vst(core.estimateSizeFactors(core.DESeqDataSet(k, np.ones((8, 1)), engine=E), type="iterate"), nsub=60)
    assert_same(np.asarray(v1.assay()), np.asarray(v2.assay()), "vst")


def test_errors(oracle):
    from deseq2_amd import core, native
    from deseq2_amd.engine import HostEngine
    E = HostEngine(oracle)
    cts, _ = CS.testthat_case(20)
    with pytest.raises(ValueError, match="did not converge$"):
        core.estimateSizeFactorsIterate(core.DESeqDataSet(cts, np.ones((12, 1)), engine=E), niter=1)
    # a solve cut off before its first iteration, from a start that is not stationary: flag 1 ...
    c = CS.solve_case(**SOLVE_CASES["far start"])
    r = E.sf_iterate_solve(c["counts"], c["mu"], c["sf"], c["disp"], c["rows"], maxit=0)
    _same(r, S.solve(oracle, maxit=0, **c), "maxit = 0")
    assert (r["flag"], r["iter"], r["evals"]) == (1, 0, 1)

    # ... which estimateSizeFactorsIterate reports as R's res$convergence != 0
    class Cut(HostEngine):
        def sf_iterate_solve(self, *a, **kw):
            kw["maxit"] = 0
            return HostEngine.sf_iterate_solve(self, *a, **kw)
    with pytest.raises(ValueError, match="did not converge within an iteration"):
        core.estimateSizeFactors(core.DESeqDataSet(cts, np.ones((12, 1)), engine=Cut(oracle)), type="iterate")
    # four samples: residual df 3 of the intercept design
    with pytest.raises(NotImplementedError, match="f4"):
        core.estimateSizeFactors(core.DESeqDataSet(cts[:, :4], np.ones((4, 1)), engine=E), type="iterate")
    for f in (lambda: core.estimateSizeFactorsForMatrix(E, E.counts(cts), type="iterate"),
              lambda: native.estimateSizeFactorsForMatrix(cts, type="iterate")):
        with pytest.raises(NotImplementedError, match="f4.*no such type"):
            f()
