"""CPU: the input builders of the device-math tests (tests/math_cases.py) do what they claim -- without this the GPU tests
could test nothing and pass --, the oracle is right where the new inputs put it (against mpmath, at the bounds of
tests/test_oracle_math.py), and the edge tables and order-key properties hold for a numpy restatement."""
import numpy as np
import pytest

from tests import math_cases as MC

EPS = 2.220446049250313e-16


# ---- the builders -------------------------------------------------------------------------------------------------------------
def test_edges_are_the_threshold_and_its_neighbours():
    e = MC.edges([1.0, -745.1332191019412, 0.0], k=3)
    assert e.size == 21
    for t in (1.0, -745.1332191019412, 0.0):
        near = np.sort(e[np.abs(e - t) <= 4 * np.spacing(abs(t))]) if t else np.sort(e[np.abs(e) < 1e-300])
        assert near.size == 7 and near[3] == t
        assert np.all(np.diff(near) > 0)
        assert np.array_equal(near[1:], np.nextafter(near[:-1], np.inf))
    assert set(np.arange(1.0, 11.0)) <= set(MC.gamma_edges())
    assert np.all(MC.stirlerr_edges() > 0) and np.all(MC.stirlerr_edges(n_form=True) < 1e100)
    sub = MC.log_subnormals(np.random.default_rng(1))
    assert sub.size >= 20000 and np.all((sub > 0) & (sub < MC.DBL_MIN))
    assert np.log2(sub).min() < -1070 and MC.DBL_MIN in MC.log_edges()
    assert np.all((MC.positive_normal(MC.log_edges()) >= MC.DBL_MIN) & np.isfinite(MC.positive_normal(MC.log_edges())))


def _check_layout(pure, pois, where, trig_pure, trig_pois):
    """every aligned 64-block of pure without a trigger lane, every block of poisoned with one; the same ordinary elements"""
    assert MC.blocks_with_trigger(trig_pure).max() == 0
    counts = MC.blocks_with_trigger(trig_pois)
    assert counts.min() >= 1 and counts.size == -(-pois[0].size // 64) and counts.size > 100
    for a, b in zip(pure, pois):
        assert np.array_equal(b[where].view(np.uint64), a.view(np.uint64))
    assert pure[0].size % 64 != 0 and pois[0].size % 64 != 0        # both end in a partial wave


def test_log_layouts():
    pure, pois, where = MC.log_layouts(np.random.default_rng(21))
    _check_layout((pure,), (pois,), where, MC.is_log_trigger(pure), MC.is_log_trigger(pois))
    t = pois[MC.is_log_trigger(pois)]
    assert (t == 0).any() and np.isnan(t).any() and (t < 0).any() and np.isinf(t).any() and ((t > 0) & (t < MC.DBL_MIN)).any()


def test_gamma_layouts():
    pure, pois, where, mixed, where_mixed = MC.gamma_layouts(np.random.default_rng(22))
    _check_layout((pure,), (pois,), where, MC.is_gamma_trigger(pure), MC.is_gamma_trigger(pois))
    assert np.all(pois[MC.is_gamma_trigger(pois)] == 1e-3) and (pure == 10.0).any()
    assert np.array_equal(mixed[where_mixed], pure)
    c = MC.blocks_with_trigger(MC.is_gamma_trigger(mixed))
    assert c.min() >= 1 and c.max() < 64                            # every wave mixed


def test_bd0_layouts():
    pure, pois, where = MC.bd0_layouts(np.random.default_rng(23))
    _check_layout(pure, pois, where, MC.is_bd0_trigger(*pure), MC.is_bd0_trigger(*pois))
    series, ok = MC.bd0_state(*pure)
    assert series.all() and ok.all()
    x, npp = pure
    rel = np.abs(x - npp) / (x + npp)
    assert rel.min() >= 1e-4 and rel.max() <= 0.09 and (x > npp).any() and (x < npp).any()
    xt, nt = (v[MC.is_bd0_trigger(*pois)] for v in pois)
    assert np.allclose(np.abs(xt - nt) / (xt + nt), 1e-7, rtol=1e-3)  # in the series branch, v = 1e-14 <= 1e-10
    # the edges set has lanes on both sides of the series switch and of the v window, and the plain form's the |ej| window's
    for fast in (False, True):
        x, npp = MC.bd0_edges(fast)
        series, ok = MC.bd0_state(x, npp)
        with np.errstate(all="ignore"):
            in_branch = np.abs(x - npp) < 0.1 * (x + npp)
        assert in_branch.any() and (~in_branch).any() and (series & ok).any() and (series & ~ok).any() and (x == npp).any()
        if fast:
            assert x.min() >= 1e-40 and x.max() <= 1e40
        else:
            ej = np.abs(2.0 * x * ((x - npp) / (x + npp)))
            assert (series & (ej >= 1e280)).any() and (series & (ej <= 1e-150)).any()
            assert (series & (ej < 1e280) & (ej > 1e279)).any() and (series & (ej > 1e-150) & (ej < 1e-148)).any()


def test_dnbinom_layouts_and_corners():
    pure, pois, where = MC.dnbinom_layouts(np.random.default_rng(25))
    _check_layout(pure, pois, where, MC.is_dnbinom_trigger(*pure), MC.is_dnbinom_trigger(*pois))
    assert MC.dnbinom_general(*pure).all()                           # all lanes in the general regime and inside the guard
    t = MC.is_dnbinom_trigger(*pois)
    assert np.all(pois[2][t] == 1e-61) and np.all((pois[1][t] >= 1e-3) & (pois[1][t] <= 1e9)) and np.all(pois[0][t] >= 1)
    x, size, mu = MC.dnbinom_guard_corners()
    assert np.array_equal(x, np.floor(x))                            # counts stay integer-valued
    t = MC.is_dnbinom_trigger(x, size, mu)
    gen = MC.dnbinom_general(x, size, mu)
    assert t.sum() > 100 and (gen & ~t).sum() > 100
    for v in (size, mu):                                             # each guard constant from both sides, in all four pairings
        for c in (1e-60, 1e60):
            assert (v == c).any() and (v == np.nextafter(c, 0)).any() and (v == np.nextafter(c, np.inf)).any()
    for s_lo in (True, False):
        for m_lo in (True, False):
            assert (((size < 1) == s_lo) & ((mu < 1) == m_lo) & (np.abs(np.log10(mu)) > 59) & (np.abs(np.log10(size)) > 59)).any()
    assert (x < 1e-10 * size).any() and ((x >= 1e-10 * size) & (size > 1e9) & (size < 1e16)).any()
    r = MC.dnbinom_random(np.random.default_rng(26))
    t = MC.is_dnbinom_trigger(*r)
    c = MC.blocks_with_trigger(t)
    assert (c == 0).sum() > 100 and (c > 0).sum() > 100 and (r[0] == 0).any()


def test_div_operands_cover_the_stated_range():
    a, x = MC.div_operands(np.random.default_rng(27))
    with np.errstate(all="ignore"):
        q = np.abs(a / x)
    assert np.abs(x).min() >= 1e-200 and np.abs(x).max() <= 1e200 and np.abs(x).min() < 1e-195 and np.abs(x).max() > 1e195
    nz = a != 0
    assert (~nz).sum() >= 128 and not np.signbit(a[~nz]).any() and (x[~nz] > 0).any() and (x[~nz] < 0).any()
    az, xz = MC.div_negative_zero(np.random.default_rng(31))
    assert np.signbit(az).all() and (az == 0).all() and (xz > 0).any() and (xz < 0).any()
    assert np.abs(a[nz]).min() >= 1e-250 and q[nz].min() >= 1e-250 and q[nz].max() <= 1e250
    assert q[nz].min() < 1e-240 and q[nz].max() > 1e240
    assert (x < 0).any() and (a < 0).any()
    m = np.frexp(np.abs(x))[0]
    assert (m == 0.5).any() and (m == 1.0 - 2.0 ** -53).any() and (m == 0.5 + 2.0 ** -53).any()
    assert np.array_equal(MC.div_in_range(a, x)[0], a)


def test_div_hard_cases_sit_next_to_midpoints():
    from fractions import Fraction
    a, x = MC.div_hard_cases(np.random.default_rng(30), n=300)
    assert a.size > 1000 and (a < 0).any() and (x < 0).any()
    q = a / x
    for ai, xi, qi in zip(a[:400].tolist(), x[:400].tolist(), q[:400].tolist()):
        exact = Fraction(ai) / Fraction(xi)
        off = abs(exact - Fraction(qi)) / Fraction(float(np.spacing(abs(qi))))       # in ulps of the rounded quotient
        assert Fraction(1, 2) - Fraction(1, 2 ** 40) < off <= Fraction(1, 2), (ai, xi, float(off))
        assert off != Fraction(1, 2)


def test_nb_split_inputs_cover_every_class():
    y, alpha, mu = MC.nb_split_inputs(np.random.default_rng(28))
    assert np.array_equal(y, np.floor(y)) and y.min() == 0 and y.max() == 1e9 and (y == 0).sum() > 1000
    assert MC.nb_split_outside(y, alpha).sum() > 1000
    assert (alpha == 0).any() and np.isinf(alpha).any() and np.isnan(alpha).any() and (alpha < 0).any()
    pos = alpha[alpha > 0]
    assert pos.min() == 1e-12 and pos[np.isfinite(pos)].max() == np.exp(10.0)
    assert mu.min() >= 1e-30 and mu.max() <= 1e30 and mu.min() < 1e-29 and mu.max() > 1e29


# ---- the oracle at the edges, against mpmath ----------------------------------------------------------------------------------
def _mp():
    import mpmath as mp
    mp.mp.dps = 120
    return mp


def _errors(mp, got, xs, f, relative):
    """worst error of got against f(x) in mpmath: in ulps of the exact value (relative) or in eps max(1, |v|); where the exact
    value is subnormal the error is held to one denormal step, where it overflows the result has to be infinite"""
    worst = 0.0
    for g, x in zip(got, xs):
        w = f(mp.mpf(float(x)))
        aw = abs(w)
        if aw > mp.mpf(MC.DBL_MAX):
            assert np.isinf(g) and (g > 0) == (w > 0), (x, g)
        elif not relative:
            worst = max(worst, float(abs(mp.mpf(float(g)) - w) / (mp.mpf(EPS) * max(1, aw))))
        elif aw == 0:
            assert g == 0.0, (x, g)
        elif aw < mp.mpf(2) ** -1022:
            assert abs(mp.mpf(float(g)) - w) <= mp.mpf(2) ** -1074, (x, g)
        else:
            worst = max(worst, float(abs(mp.mpf(float(g)) - w) / mp.mpf(float(np.spacing(abs(float(w)))))))
    return worst


@pytest.mark.parametrize("name,max_ulp", [("exp", 1.5), ("log", 1.5), ("log1p", 1.5), ("trigamma", 8.0)])
def test_oracle_relative_accuracy_at_the_edges(oracle, name, max_ulp):
    mp = _mp()
    if name == "exp":
        x, f = MC.exp_edges(), mp.exp
    elif name == "log":
        x = np.concatenate([MC.log_edges(), MC.log_subnormals(np.random.default_rng(1), 300)])
        x, f = x[(x > 0) & np.isfinite(x)], mp.log
    elif name == "log1p":
        x = MC.log1p_edges()
        x, f = x[x > -1.0], mp.log1p
    else:
        x = MC.gamma_edges()
        x, f = x[x > 1e-150], lambda v: mp.psi(1, v)        # below, the value overflows and an ulp is undefined
    err = _errors(mp, oracle.unary(name, x), x, f, relative=True)
    print("%s: %.2f ulp at %d edge arguments" % (name, err, x.size))
    assert err <= max_ulp


def _stirlerr_mp(mp):
    def f(n):
        if n <= mp.mpf(10) ** 15:       # (the difference cancels: ~ 17 + log10(n log n) digits, far inside 120)
            return mp.loggamma(n + 1) - (n + mp.mpf(1) / 2) * mp.log(n) + n - mp.log(2 * mp.pi) / 2
        return 1 / (12 * n) - 1 / (360 * n ** 3) + 1 / (1260 * n ** 5) - 1 / (1680 * n ** 7)
    return f


@pytest.mark.parametrize("name,max_eps", [("lgamma", 50.0), ("digamma", 16.0), ("stirlerr", 80.0)])
def test_oracle_absolute_accuracy_at_the_edges(oracle, name, max_eps):
    mp = _mp()
    if name == "lgamma":
        x = MC.gamma_edges()
        x, f = x[x > 0], mp.loggamma
    elif name == "digamma":
        x = MC.gamma_edges()
        x, f = x[x > 1.0 / MC.DBL_MAX], lambda v: mp.psi(0, v)
    else:
        x, f = MC.stirlerr_edges(n_form=True), _stirlerr_mp(mp)
    err = _errors(mp, oracle.unary(name, x), x, f, relative=False)
    print("%s: %.2f eps max(1, |v|) at %d edge arguments" % (name, err, x.size))
    assert err <= max_eps


# ---- the edge tables and the order-key properties, on a numpy restatement ---------------------------------------------------
def _sf_log_np(v):
    with np.errstate(all="ignore"):
        return np.log(v)


def _sf_exp_np(v):
    with np.errstate(all="ignore"):
        return np.exp(v)


def test_sf_edge_tables_hold_for_libm():
    MC.check_table(_sf_log_np, MC.SF_LOG_TABLE, "log")
    MC.check_table(_sf_exp_np, MC.SF_EXP_TABLE, "exp")
    with pytest.raises(AssertionError):
        MC.check_table(lambda v: np.abs(_sf_log_np(v)), MC.SF_LOG_TABLE, "a wrong log")


def test_order_key_properties_hold_for_the_restatement():
    x = MC.order_inputs(np.random.default_rng(29))
    assert (x == 0).sum() == 2 and np.isinf(x).sum() == 2 and (np.abs(x) == MC.DBL_MAX).sum() == 2
    assert ((np.abs(x) > 0) & (np.abs(x) < MC.DBL_MIN)).sum() > 500 and (np.abs(x) == MC.DBL_MIN).sum() == 2
    keys = MC.order_key_np(x)
    MC.check_order_properties(x, keys, MC.order_unkey_np(keys))
    # and the checks bite: a key that drops the sign handling orders the negatives backwards; one that merges the zeros
    # collides; a round trip that loses the sign of zero is seen
    with pytest.raises(AssertionError):
        MC.check_order_properties(x, x.view(np.uint64) ^ np.uint64(1 << 63), x)
    merged = keys.copy()
    merged[x == 0] = keys[(x == 0) & ~np.signbit(x)][0]
    with pytest.raises(AssertionError):
        MC.check_order_properties(x, merged, x)
    with pytest.raises(AssertionError):
        MC.check_order_properties(x, keys, x + 0.0)
