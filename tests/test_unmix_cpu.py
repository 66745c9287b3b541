"""CPU: unmix().  HostEngine.unmix_fit against the numpy specification bit for bit; the minimum the
iteration reaches against R's optim call restated through scipy (tests/unmix_lbfgsb.py), for both forms of v and both powers;
a local check that owes nothing to that reference; the construction of tests/testthat/test_unmix.R; R's argument checks and
those of the C entry; three mutants that the comparison of the minima must catch.

The bounds of the comparison (profiles/unmix.md).  Measured on the cases of unmix_cases.MINIMUM_SAMPLES, specification against
unmix_lbfgsb: the largest relative excess of our loss over the reference's is <= 0 for both powers (ours is up to 1.2e-2 lower
under power 1, where the reference stops short of the flat minimum); the largest difference of mix is 3.44e-3 (power 1) and
2.26e-4 (power 2).
  DELTA   ten times a non-positive excess is no bound, so it comes from the stopping rules: the reference stops when its
          relative decrease falls below factr * eps = 2.2e-9, ours at 1e-10; neither loss is known better than that:
          10 * 2.2e-9 = 2.2e-8.
  EPS     ten times the measured worst: 2.3e-3 for power 2; for power 1 that would be 3.4e-2, above the 0.02 at which the check
          turns vacuous, so 0.02 (a factor 5.8)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import unmix_cases as CS
from tests import unmix_lbfgsb as RF
from tests import unmix_spec as S
from tests.helpers import assert_same

DELTA = 2.2e-8
EPS = {1: 0.02, 2: 2.3e-3}
CASES = CS.cases()
GRID = [(name, form, power) for name in CASES for form in CS.FORMS for power in (1, 2)]
MIN_GRID = [g for g in GRID if g[0] in CS.MINIMUM_SAMPLES and g[1] in CS.MINIMUM_FORMS.get(g[0], tuple(CS.FORMS))]


@functools.lru_cache(maxsize=None)
def _spec(name, form, power):
    from oracle import oracle as O
    x, pure, _ = CASES[name]
    return S.unmix_fit(O, x, pure, power=power, **CS.FORMS[form])


@functools.lru_cache(maxsize=None)
def _reference(name, form, power):
    x, pure, _ = CASES[name]
    sel = CS.minimum_samples(name, power, x.shape[1])
    return sel, RF.unmix_lbfgsb(x[:, sel], pure, power=power, **CS.FORMS[form])


def _libm_loss(name, form, power, P, sel):
    x, pure, _ = CASES[name]
    return np.array([RF.sum_loss(P[i], x[:, j], pure, power=power, **CS.FORMS[form]) for i, j in enumerate(sel)])


def minimum_misses(name, form, power, fit):
    """check 2 on the samples compared: the list of what misses it"""
    sel, ref = _reference(name, form, power)
    ours = _libm_loss(name, form, power, fit["p"][sel], sel)
    mix = S.mix_of(fit["p"][sel])
    excess = (ours - ref["loss"]) / ref["loss"]
    dmix = np.abs(mix - ref["mix"]).max(axis=1)
    print("%s %s power %d: excess %s, mix difference %s" % (name, form, power, excess, dmix))
    out = []
    for i, j in enumerate(sel):
        if not ours[i] <= ref["loss"][i] * (1 + DELTA):
            out.append(("loss", j, ours[i], ref["loss"][i]))
        if not dmix[i] <= EPS[power]:
            out.append(("mix", j, dmix[i]))
    return out


# ---- 1. bit-equality ------------------------------------------------------------------------------------------------------------
def test_block_constant():
    from deseq2_amd import _lib, unmix_host
    assert S.T == unmix_host.THREADS == _lib.lib().dsq_unmix_block_threads()
    assert S.MAX_K == unmix_host.MAX_K == _lib.DSQ_UNMIX_MAX_K == 16


@pytest.mark.parametrize("name,form,power", GRID)
def test_host_engine_equals_the_specification(oracle, name, form, power):
    x, pure, _ = CASES[name]
    got = HostEngine(oracle).unmix_fit(x, pure, power=power, **CS.FORMS[form])
    want = _spec(name, form, power)
    for k in ("p", "loss", "iter", "flag"):
        assert_same(got[k], want[k], "%s %s power %d: %s" % (name, form, power, k))
    assert got["iter"].dtype == np.int32 and got["flag"].dtype == np.int32
    assert set(want["flag"]) <= {0, 1} and (want["iter"] >= 1).all()


def test_the_paths_are_taken():
    """the cases reach both bounds, the tolerance stop and the cap"""
    p = _spec("vertices", "alpha", 2)["p"]
    assert (p[0, 1:] == 1e-6).all() and p[0, 0] > 0.5                  # a sample equal to a pure column: the others on lo
    assert p[2, 1] == 100.0                                              # 150 x a pure column: the upper bound
    assert (_spec("vertices", "shift", 1)["p"][0, 1:] == 0.0).all()                 # ... on lo = 0 under the shifted log
    flags = np.concatenate([_spec(*g)["flag"] for g in GRID])
    assert (flags == 0).any() and (flags == 1).any()
    z = _spec("zeros", "shift", 1)
    assert z["loss"][2] == 0.0 and (z["p"][2] == 0.0).all()              # the all-zero sample under the shifted log: p = 0


# ---- 2. the minimum against the reference optimiser ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,power", MIN_GRID)
def test_minimum_against_the_reference_optimiser(oracle, name, form, power):
    assert DELTA <= 1e-4 and EPS[power] <= 0.02
    assert minimum_misses(name, form, power, _spec(name, form, power)) == []


# ---- 4. a check that owes nothing to the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,power", GRID)
def test_no_coordinate_move_lowers_the_loss(oracle, name, form, power):
    """at the returned p no clipped move of +-1e-3 along a coordinate lowers L by more than DELTA L"""
    x, pure, _ = CASES[name]
    kw = CS.FORMS[form]
    fit = _spec(name, form, power)
    lo = S.lower_bound(kw.get("alpha"))
    for i in range(x.shape[1]):
        p = fit["p"][i]
        here = S.loss_at(oracle, x[:, i], pure, p, kw.get("alpha"), kw.get("shift"), power)
        for j in range(p.size):
            for step in (-1e-3, 1e-3):
                q = p.copy()
                q[j] = min(max(p[j] + step, lo), S.HI)
                there = S.loss_at(oracle, x[:, i], pure, q, kw.get("alpha"), kw.get("shift"), power)
                assert there >= here - DELTA * here, (name, form, power, i, j, step, here, there)


# ---- 5. the reference's own expectation ------------------------------------------------------------------------------------------
def test_the_construction_of_test_unmix_R(oracle):
    """tests/testthat/test_unmix.R:4-56 with numpy's generator in place of R's stream (set.seed(1) cannot be reproduced here):
    n = 100, three components at 1e4 U(0, 1), dispersion 0.01, the eight mixtures of its coldata; alpha is the dispersion the
    data were drawn with (the reference takes the fitted mean dispersion of the same data)"""
    x, pure, truth = CASES["reference"]
    E = HostEngine(oracle)
    xn = core._named(x, None, ["sample%d" % (i + 1) for i in range(8)])
    pn = core._named(pure, None, ["a", "b", "c"])
    mix = core.unmix(xn, pn, alpha=0.01, quiet=True, engine=E)
    assert mix.shape == (8, 3) and mix.colnames == ["a", "b", "c"] and mix.rownames == xn.colnames
    for c in range(3):
        assert np.abs(truth[:, c] - mix[:, c]).max() < 0.1                                    # :44-46
    assert np.abs(np.asarray(mix).sum(axis=1) - 1.0).max() <= 2.220446049250313e-16
    assert_same(np.asarray(mix), S.mix_of(_spec("reference", "alpha", 1)["p"]), "core.unmix against the specification")
    mix2 = core.unmix(x, pure, shift=0.5, quiet=True, engine=E)                               # :49
    assert mix2.shape == (8, 3) and mix2.colnames is None
    assert_same(np.asarray(mix2), S.mix_of(_spec("reference", "shift", 1)["p"]), "shift")
    mix3 = core.unmix(xn, pn, alpha=0.01, format="list", quiet=True, engine=E)                # :52
    assert sorted(mix3) == ["cor", "fitted", "mix"]
    assert mix3["mix"].shape == (8, 3) and mix3["cor"].shape == (8,) and mix3["fitted"].shape == (100, 8)
    assert_same(np.asarray(mix3["mix"]), np.asarray(mix), "format = list")
    assert (mix3["cor"] > 0.95).all() and mix3["fitted"].colnames == xn.colnames
    np.testing.assert_allclose(np.asarray(mix3["fitted"]), pure @ np.asarray(mix).T, rtol=1e-14)
    rng = np.random.Generator(np.random.PCG64(5))
    pure4 = np.column_stack([pure, pure[:, 2] + rng.poisson(10, 100)])                        # :55
    with pytest.warns(UserWarning, match="highly correlated"):
        core.unmix(x, pure4, alpha=0.01, power=2, quiet=True, engine=E)                       # :56
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        core.unmix(x[:, :2], pure, alpha=0.01, power=2, engine=E)
    import deseq2_amd
    assert deseq2_amd.unmix is core.unmix


# ---- 6. R's checks, and the C entry's -------------------------------------------------------------------------------------------------
def test_the_checks_of_R(oracle):
    x, pure, _ = CASES["zeros"]
    E = HostEngine(oracle)
    with pytest.raises(ValueError, match="should be one of"):
        core.unmix(x, pure, alpha=0.01, format="frame", engine=E)                             # :72
    with pytest.raises(ValueError, match=r"!missing\(shift\) is not TRUE"):
        core.unmix(x, pure, engine=E)                                                         # :73
    with pytest.raises(ValueError, match=r"missing\(shift\) \| missing\(alpha\) is not TRUE"):
        core.unmix(x, pure, alpha=0.01, shift=0.5, engine=E)                                  # :75
    with pytest.raises(ValueError, match="power %in% 1:2"):
        core.unmix(x, pure, alpha=0.01, power=3, engine=E)                                    # :76
    with pytest.raises(ValueError, match=r"nrow\(x\) == nrow\(pure\)"):
        core.unmix(x[:-1], pure, alpha=0.01, engine=E)                                        # :77
    with pytest.raises(ValueError, match=r"ncol\(pure\) > 1"):
        core.unmix(x, pure[:, :1], alpha=0.01, engine=E)                                      # :78
    with pytest.raises(ValueError, match="alpha > 0"):
        core.unmix(x, pure, alpha=0.0, engine=E)                                              # :88
    with pytest.raises(ValueError, match="shift > 0"):
        core.unmix(x, pure, shift=-1.0, engine=E)                                             # :101
    # R's order: the format before the missing arguments, the power before the dimensions
    with pytest.raises(ValueError, match="should be one of"):
        core.unmix(x, pure, format="frame", engine=E)
    with pytest.raises(ValueError, match="power %in% 1:2"):
        core.unmix(x[:-1], pure, alpha=0.01, power=0, engine=E)
    with pytest.raises(NotImplementedError, match="at most 16"):
        core.unmix(x, np.ones((70, 17)) + np.arange(17.0) * np.arange(70.0)[:, None] % 7, alpha=0.01, engine=E)


def test_the_entry_points_check_their_arguments():
    """dsq_unmix / dsq_unmix_dev decide their argument errors before a device is asked for (1 = DSQ_ERR_ARG,
    2 = DSQ_ERR_UNSUPPORTED, 5 = DSQ_ERR_VALUE)"""
    from deseq2_amd import _lib as L
    lib = L.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    n, m = 6, 3
    x = np.asfortranarray(np.arange(1.0, n * m + 1).reshape(n, m))
    pure = np.asfortranarray(np.arange(1.0, n * 17 + 1).reshape(n, 17))
    p, loss = np.zeros((m, 17)), np.zeros(m)
    it, flag = np.zeros(m, np.int32), np.zeros(m, np.int32)
    out = L.DsqUnmixOut(p=P(p), loss=P(loss), iter=P(it), flag=P(flag))

    def args(**kw):
        base = dict(n=n, m=m, k=3, ld=8, x=P(x), pure=P(pure), has_alpha=1, has_shift=0, alpha=0.01, shift=0.0, power=1, maxit=200)
        base.update(kw)
        return L.DsqUnmixArgs(**base)

    ws = np.zeros(n * m)
    calls = (lambda a: lib.dsq_unmix(C.byref(a), C.byref(out)),
             lambda a: lib.dsq_unmix_dev(C.byref(a), C.byref(out), P(ws), ws.nbytes, None))
    for call in calls:
        assert call(args(k=1)) == 1 and b"at least two" in lib.dsq_last_error()
        assert call(args(k=17)) == 2 and b"at most 16" in lib.dsq_last_error()
        assert call(args(has_shift=1, shift=0.5)) == 1 and b"exactly one" in lib.dsq_last_error()
        assert call(args(has_alpha=0)) == 1 and b"exactly one" in lib.dsq_last_error()
        assert call(args(alpha=0.0)) == 1 and b"alpha" in lib.dsq_last_error()
        assert call(args(alpha=np.inf)) == 1
        assert call(args(has_alpha=0, has_shift=1, shift=-0.5)) == 1 and b"shift" in lib.dsq_last_error()
        assert call(args(power=0)) == 1 and call(args(power=3)) == 1 and b"power" in lib.dsq_last_error()
        assert call(args(x=None)) == 1 and call(args(n=0)) == 1 and call(args(maxit=-1)) == 1
    assert lib.dsq_unmix_dev(C.byref(args(ld=2)), C.byref(out), P(ws), ws.nbytes, None) == 1 and b"ld" in lib.dsq_last_error()
    assert lib.dsq_unmix_dev(C.byref(args()), C.byref(out), P(ws), ws.nbytes - 1, None) == 1 and b"workspace" in lib.dsq_last_error()
    assert lib.dsq_unmix_workspace_bytes(n, m, 3) == ws.nbytes and lib.dsq_unmix_workspace_bytes(0, m, 3) == 0
    for bad in (-1.0, np.nan, np.inf):
        xb = x.copy(order="F")
        xb[2, 1] = bad
        assert lib.dsq_unmix(C.byref(args(x=P(xb))), C.byref(out)) == 5 and b"x holds" in lib.dsq_last_error()
        pb = pure.copy(order="F")
        pb[1, 2] = bad
        assert lib.dsq_unmix(C.byref(args(pure=P(pb))), C.byref(out)) == 5 and b"pure holds" in lib.dsq_last_error()


# ---- 7. mutants that must fail check 2 ----------------------------------------------------------------------------------------------
def test_mutant_the_loss_of_power_2_where_power_1_was_asked(oracle):
    x, pure, _ = CASES["reference"]
    fit = S.unmix_fit(oracle, x, pure, power=1, loss_power=2, **CS.FORMS["alpha"])
    assert minimum_misses("reference", "alpha", 1, fit) != []


def test_mutant_a_zero_lower_bound_under_the_alpha_form(oracle):
    """lo = 0 with all-zero rows of pure and marker genes: the first step from p = 1 puts the small component on 0, where
    v'(0) is infinite on every gene that could move it again"""
    x, pure, _ = CASES["markers"]
    assert (pure == 0).all(axis=1).any()
    fit = S.unmix_fit(oracle, x, pure, power=2, lo=0.0, **CS.FORMS["alpha"])
    assert (fit["p"] == 0.0).any()
    assert minimum_misses("markers", "alpha", 2, fit) != []


def test_mutant_no_active_set_on_a_sample_that_is_a_pure_column(oracle):
    x, pure, _ = CASES["vertices"]
    fit = S.unmix_fit(oracle, x, pure, power=2, active_set=False, **CS.FORMS["alpha"])
    assert minimum_misses("vertices", "alpha", 2, fit) != []
