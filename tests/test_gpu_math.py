"""-m gpu: the device math library (csrc/dsq_math.hpp) must reproduce the oracle's scalar
primitives (oracle/orc_nmath.c) BIT FOR BIT -- that is what makes iteration counts of the
kernels identical to the oracle's by construction.

Every entry point the kernels call is evaluated on its own through the hook dsq_test_math (csrc/util.hip), on three kinds of
input (tests/math_cases.py): a random set, the nextafter neighbours of every threshold its branches compare with, and -- for
the routines that branch once per wave -- the same elements in a wave that takes the fast branch and in one that a single
lane sends the slow way.  The comparisons are on the 64 bits (assert_bits: the sign of a zero counts)."""
import numpy as np
import pytest

from tests import math_cases as MC
from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu


def _inputs(rng):
    pos = np.concatenate([np.exp(rng.uniform(-30, 30, 40000)), rng.uniform(0, 20, 40000),
                          np.arange(0, 40, 0.5), [1e-300, 5e-324, 1e300, np.inf, 0.0, np.nan]])
    anyx = np.concatenate([rng.uniform(-750, 720, 40000), rng.uniform(-2, 2, 40000), -pos[:2000],
                           [np.inf, -np.inf, np.nan, 0.0, -0.0, 709.8, -745.2]])
    return pos, anyx


@pytest.mark.parametrize("name,op", [("exp", 0), ("log", 1), ("log1p", 2), ("lgamma", 3), ("digamma", 4),
                                     ("trigamma", 5), ("stirlerr", 6), ("pnorm_upper2", 9)])
def test_unary_bit_exact(oracle, name, op):
    from deseq2_amd import native
    rng = np.random.default_rng(op + 11)
    pos, anyx = _inputs(rng)
    if name == "exp":
        x = anyx
    elif name == "log":
        x = np.concatenate([pos, [-1.0]])
    elif name == "log1p":
        x = np.concatenate([rng.uniform(-1, 3, 50000), np.exp(rng.uniform(-60, 60, 20000)),
                            -np.exp(rng.uniform(-60, 0, 20000)), [-1.0, -2.0, np.inf, np.nan, 0.0]])
    elif name == "pnorm_upper2":            # the Wald p-value: +-40 covers its three ranges and the underflow; the range edges
        edges = [0.67448975, float(np.sqrt(32.0)), 37.5, 38.4, 38.5]
        edges = np.array([t for e in edges for t in (np.nextafter(e, 0.0), e, np.nextafter(e, 100.0))])
        x = np.concatenate([anyx[:40000] * (40.0 / 750.0), anyx[40000:80000] * 20.0, edges, -edges,
                            [0.0, -0.0, np.inf, -np.inf, np.nan]])
    elif name == "stirlerr":
        x = pos[(pos > 0) & np.isfinite(pos)]
    else:
        x = pos
    got = native.test_math(op, x)
    want = oracle.unary(name, x)
    assert_bits(got, want, name)


def test_bd0_and_dnbinom_bit_exact(oracle):
    from deseq2_amd import native
    rng = np.random.default_rng(5)
    n = 200000
    x = rng.integers(0, 5000, n).astype(float)
    x[rng.uniform(size=n) < 0.2] = 0.0
    size = np.exp(rng.uniform(np.log(1e-3), np.log(1e9), n))
    mu = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), n))
    mu[:2000] = x[:2000] * (1 + rng.normal(0, 1e-3, 2000)) + 1e-9   # x ~ np branch of bd0
    got = native.test_math(8, x, size, mu)
    want = oracle.dnbinom_mu_log(x, size, mu)
    assert_bits(got, want, "dnbinom_mu_log")
    xx = np.exp(rng.uniform(-5, 12, n)); npp = xx * np.exp(rng.normal(0, 0.2, n))
    got = native.test_math(7, xx, npp)
    want = _orc_bd0(oracle, xx[:20000], npp[:20000])
    assert_bits(got[:20000], want, "bd0")
    # edge cases: infinite size (Poisson limit), zero mu, huge mu
    xe = np.array([0, 3, 7, 0, 5, 2, 4], float)
    se = np.array([np.inf, np.inf, 1e300, 0.0, 0.5, 10, 10], float)
    me = np.array([2.5, 2.5, 3.0, 1.0, 0.0, np.inf, 1e-300], float)
    assert_bits(native.test_math(8, xe, se, me), oracle.dnbinom_mu_log(xe, se, me), "dnbinom edge")


# ---- the references (none of them the code under test) ---------------------------------------------------------------------
def _orc_bd0(oracle, x, npp):
    L = oracle.lib()
    return np.array([L.orc_bd0(a, b) for a, b in zip(x, npp)])


def _pnorm_ref(which):
    def ref(oracle, z):
        from tests import results_spec
        return (results_spec.pnorm_lower if which == "lower" else results_spec.pnorm_upper)(oracle, z)
    return ref


def _unary_ref(name):
    return lambda oracle, x: oracle.unary(name, x)


_SPECIAL = [np.inf, -np.inf, np.nan, 0.0, -0.0]

# name of the hook's op -> (reference, random set, edges set).  The old ops are here for their edges sets (their random
# sets: test_unary_bit_exact); log_pn takes positive normal finite arguments only, the stirlerr pair positive ones.
_UNARY = {
    "exp": (_unary_ref("exp"), None, MC.exp_edges),
    "log": (_unary_ref("log"), None, lambda: np.concatenate([MC.log_edges(), MC.log_subnormals(np.random.default_rng(1))])),
    "log1p": (_unary_ref("log1p"), None, MC.log1p_edges),
    "lgamma": (_unary_ref("lgamma"), None, MC.gamma_edges),
    "digamma": (_unary_ref("digamma"), None, MC.gamma_edges),
    "trigamma": (_unary_ref("trigamma"), None, MC.gamma_edges),
    "stirlerr": (_unary_ref("stirlerr"), lambda r: MC.stirlerr_random(r), MC.stirlerr_edges),
    "pnorm_upper2": (_unary_ref("pnorm_upper2"), None, MC.pnorm_edges),
    "log_full": (_unary_ref("log"), lambda r: np.concatenate([MC.positive_random(r), _SPECIAL, [-1.0, 5e-324]]),
                 lambda: np.concatenate([MC.log_edges(), MC.log_subnormals(np.random.default_rng(1))])),
    "log_pn": (_unary_ref("log"), lambda r: MC.positive_normal(MC.positive_random(r)), lambda: MC.positive_normal(MC.log_edges())),
    "stirlerr_n": (_unary_ref("stirlerr"), lambda r: MC.stirlerr_random(r), lambda: MC.stirlerr_edges(n_form=True)),
    "lgamma_pair_lg": (_unary_ref("lgamma"), lambda r: np.concatenate([MC.positive_random(r), _SPECIAL, [1e-300, 5e-324, 1e300]]),
                       MC.gamma_edges),
    "lgamma_pair_dg": (_unary_ref("digamma"), lambda r: np.concatenate([MC.positive_random(r), _SPECIAL, [1e-300, 5e-324, 1e300]]),
                       MC.gamma_edges),
    "pnorm_lower": (_pnorm_ref("lower"), lambda r: np.concatenate([MC.pnorm_random(r), _SPECIAL]), MC.pnorm_edges),
    "pnorm_upper": (_pnorm_ref("upper"), lambda r: np.concatenate([MC.pnorm_random(r), _SPECIAL]), MC.pnorm_edges),
    "sf_log": (_unary_ref("log"), lambda r: np.concatenate([MC.positive_random(r), [5e-324, 1e-310]]),
               lambda: np.concatenate([MC.log_edges(), MC.log_subnormals(np.random.default_rng(1), 2000)])),
    "sf_exp": (_unary_ref("exp"), lambda r: np.concatenate([r.uniform(-750, 720, 40000), r.uniform(-2, 2, 40000)]),
               lambda: np.concatenate([MC.exp_edges(), [np.inf, -np.inf]])),
}


@pytest.mark.parametrize("name", sorted(_UNARY))
def test_unary_entry_points_random_and_edges(oracle, name):
    """each one-argument entry point against its reference on its random set and on the nextafter neighbours of its
    thresholds; the edges set once more in waves of its own, so that a wave-uniform branch is decided by those lanes alone"""
    from deseq2_amd import native
    ref, random_set, edge_set = _UNARY[name]
    op = native.MATH_OPS[name]
    if random_set is not None:
        x = random_set(np.random.default_rng(op + 101))
        assert_bits(native.test_math(op, x), ref(oracle, x), name + " random")
    e = edge_set()
    assert_bits(native.test_math(op, e), ref(oracle, e), name + " edges")
    for n in MC.PARTIAL_LENGTHS:                    # a partial last wave: the inactive lanes decide nothing
        assert_bits(native.test_math(op, e[:n]), ref(oracle, e[:n]), "%s edges[:%d]" % (name, n))


def _layout_check(run, ref, pure, poisoned, where, what):
    """both layouts against the reference, and the ordinary elements bit for bit the same in both: a lane's result does not
    depend on its 63 neighbours"""
    gp, gq = run(*pure), run(*poisoned)
    assert_bits(gp, ref(*pure), what + " pure")
    assert_bits(gq, ref(*poisoned), what + " poisoned")
    assert_bits(gq[where], gp, what + " poisoned vs pure at the ordinary elements")


@pytest.mark.parametrize("name", ["log", "log_full", "sf_log"])
def test_log_wave_layouts(oracle, name):
    """dlog takes dlog_pn unless a lane of the wave is special; dlog_pn itself on the pure layout"""
    from deseq2_amd import native
    op = native.MATH_OPS[name]
    pure, pois, where = MC.log_layouts(np.random.default_rng(21))
    ref = lambda x: oracle.unary("log", x)
    _layout_check(lambda x: native.test_math(op, x), ref, (pure,), (pois,), where, name)
    assert_bits(native.test_math(native.MATH_OPS["log_pn"], pure), ref(pure), "log_pn pure")


@pytest.mark.parametrize("name,refname", [("lgamma", "lgamma"), ("digamma", "digamma"), ("trigamma", "trigamma"),
                                          ("lgamma_pair_lg", "lgamma"), ("lgamma_pair_dg", "digamma")])
def test_gamma_wave_layouts(oracle, name, refname):
    """all lanes >= 10 (the early break, fit_disp's common case), one lane at 1e-3 per wave (ten trips), mixed at random"""
    from deseq2_amd import native
    op = native.MATH_OPS[name]
    pure, pois, where, mixed, where_mixed = MC.gamma_layouts(np.random.default_rng(22))
    run = lambda x: native.test_math(op, x)
    ref = lambda x: oracle.unary(refname, x)
    _layout_check(run, ref, (pure,), (pois,), where, name)
    gm = run(mixed)
    assert_bits(gm, ref(mixed), name + " mixed")
    assert_bits(gm[where_mixed], run(pure), name + " mixed vs pure at the ordinary elements")


@pytest.mark.parametrize("name", ["bd0", "bd0_fast"])
def test_bd0_layouts_random_edges(oracle, name):
    """the unrolled series with the multiply-by-reciprocal quotient (every lane ok) against the plain loop (one lane with
    v <= 1e-10), for both division forms; the 0.1 (x + np) switch and the ok window from both sides"""
    from deseq2_amd import native
    op = native.MATH_OPS[name]
    run = lambda x, npp: native.test_math(op, x, npp)
    ref = lambda x, npp: _orc_bd0(oracle, x, npp)
    pure, pois, where = MC.bd0_layouts(np.random.default_rng(23))
    _layout_check(run, ref, pure, pois, where, name)
    x, npp = MC.bd0_random(np.random.default_rng(24))
    assert_bits(run(x, npp), ref(x, npp), name + " random")
    x, npp = MC.bd0_edges(fast=(name == "bd0_fast"))
    assert_bits(run(x, npp), ref(x, npp), name + " edges")
    keep = ~MC.is_bd0_trigger(x, npp)               # without the lanes that fail ok: the lanes just inside take the fast way
    assert_bits(run(x[keep], npp[keep]), ref(x[keep], npp[keep]), name + " edges inside the window")


def test_dnbinom_layouts_and_guard_corners(oracle):
    """the scaling-free regime (every lane inside the guard) against the plain divisions (one lane with mu = 1e-61); every
    regime in random lanes; size and mu at the nextafter neighbours of 1e-60 and 1e60"""
    from deseq2_amd import native
    run = lambda x, size, mu: native.test_math(8, x, size, mu)
    pure, pois, where = MC.dnbinom_layouts(np.random.default_rng(25))
    _layout_check(run, oracle.dnbinom_mu_log, pure, pois, where, "dnbinom_mu_log")
    r = MC.dnbinom_random(np.random.default_rng(26))
    assert_bits(run(*r), oracle.dnbinom_mu_log(*r), "dnbinom_mu_log random, every regime")
    x, size, mu = MC.dnbinom_guard_corners()
    assert_bits(run(x, size, mu), oracle.dnbinom_mu_log(x, size, mu), "dnbinom_mu_log guard corners")
    keep = ~MC.is_dnbinom_trigger(x, size, mu)      # the lanes just inside the guard alone: they take the fast regime
    assert keep.sum() > 100
    assert_bits(run(x[keep], size[keep], mu[keep]), oracle.dnbinom_mu_log(x[keep], size[keep], mu[keep]),
                "dnbinom_mu_log guard corners, inside")
    for n in MC.PARTIAL_LENGTHS:
        assert_bits(run(x[:n], size[:n], mu[:n]), oracle.dnbinom_mu_log(x[:n], size[:n], mu[:n]), "dnbinom_mu_log [:%d]" % n)


def test_div_n_and_rcp_n_are_ieee_division():
    """the scaling-free quotient against IEEE division (numpy: correctly rounded) over |x| in [1e-200, 1e200], quotients in
    [1e-250, 1e250], a = +0, quotients next to rounding boundaries and midpoints, extreme mantissas, both signs"""
    from deseq2_amd import native
    a, x = MC.div_operands(np.random.default_rng(27))
    assert a.size > 100000
    assert_bits(native.test_math(native.MATH_OPS["div_n"], a, x), a / x, "div_n")
    assert_bits(native.test_math(native.MATH_OPS["rcp_n"], x), 1.0 / x, "rcp_n")
    ah, xh = MC.div_hard_cases(np.random.default_rng(30))       # exact quotients a relative 2^-107 .. 2^-97 from a midpoint
    assert ah.size > 10000
    assert_bits(native.test_math(native.MATH_OPS["div_n"], ah, xh), ah / xh, "div_n next to midpoints")
    for n in MC.PARTIAL_LENGTHS:
        assert_bits(native.test_math(native.MATH_OPS["div_n"], a[:n], x[:n]), a[:n] / x[:n], "div_n [:%d]" % n)
    # the limit stated in ddiv_n's comment, pinned: a numerator of -0 (no caller forms one) gives +0 whatever the divisor's
    # sign -- IEEE division gives -0 over a positive divisor; the sign is what v_div_fixup would restore
    az, xz = MC.div_negative_zero(np.random.default_rng(31))
    assert_bits(native.test_math(native.MATH_OPS["div_n"], az, xz), np.zeros(az.size), "div_n(-0, x)")


def test_nb_split_one_sample_loglike(oracle):
    """K' + the sweep's term for one sample, as loglike_constants and loglike_kernel form them, against the oracle's
    nbinomLogLike on rows of length 1: inside the split, outside it (y < 1e-10 size) and with an alpha that is not `fast`"""
    from deseq2_amd import native
    y, alpha, mu = MC.nb_split_inputs(np.random.default_rng(28))
    assert MC.nb_split_outside(y, alpha).sum() > 1000 and (y == 0).sum() > 1000
    got = native.test_math(native.MATH_OPS["nb_split"], y, alpha, mu)
    want = oracle.nbinomLogLike(y[:, None], mu[:, None], alpha, None, False)
    assert_bits(got, want, "nb_split")
    for n in MC.PARTIAL_LENGTHS:
        assert_bits(native.test_math(native.MATH_OPS["nb_split"], y[:n], alpha[:n], mu[:n]), want[:n], "nb_split [:%d]" % n)


def test_sf_edge_tables():
    from deseq2_amd import native
    MC.check_table(lambda v: native.test_math(native.MATH_OPS["sf_log"], v), MC.SF_LOG_TABLE, "sf_log")
    MC.check_table(lambda v: native.test_math(native.MATH_OPS["sf_exp"], v), MC.SF_EXP_TABLE, "sf_exp")


def test_order_key_properties():
    from deseq2_amd import native
    x = MC.order_inputs(np.random.default_rng(29))
    keys = native.test_math(native.MATH_OPS["order_key"], x).view(np.uint64)
    back = native.test_math(native.MATH_OPS["order_roundtrip"], x)
    MC.check_order_properties(x, keys, back)
