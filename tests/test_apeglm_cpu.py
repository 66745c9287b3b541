"""CPU: the apeglm posterior.  The numpy specification (tests/apeglm_spec.py) against a 50-digit
statement of the same formulas, its stopping rule against the 50-digit Newton step, its optimum against scipy's L-BFGS-B on
the same objective; the host engine against the specification bit for bit on every case of the GPU list; core.svalue, the
prior scale, and tests/testthat/test_lfcShrink.R re-run through core.lfcShrinkApeglm on HostEngine(oracle).

Measured here (the figures profiles/apeglm.md and the README quote), 381 rows, four designs, seeds 11-14:
    rows on which scipy found a lower mode                       0
    scipy's own stopping error in F (spread across its starts)   3.6e-12
    max |map - scipy| on rows at the same mode                   1.3e-7 (printed as `map distance`)
    worst 50-digit residual Newton step on the conv = 0 rows     1.0e-15 (no row ended with conv = 1 or 2)"""
from collections import OrderedDict

import mpmath as mp
import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import apeglm_cases as AC
from tests import apeglm_spec as S
from tests.helpers import assert_same

EPS = 2.0 ** -53
MAP_DISTANCE = 1.3e-7          # measured max |map - scipy| at the same mode (scipy's stopping tolerance); the test asserts twice this
SCALES = {11: 0.05, 12: 0.2, 13: 0.35, 14: None}        # None: the adaptive scale of the set's own MLE


# ---- the 50-digit statement ---------------------------------------------------------------------------------------------------
def _mp_posterior(y, x, nf, w, a, no_shrink, Sc, b, df=1.0, NS=15.0):
    """(F, g, H) at b in 50 digits, and the first-order bounds on what double arithmetic in the specification's order can
    differ from them by: every elementary operation and exp / log / log1p is taken to err by at most 1 ulp, eta_j carries
    E_j = (p + 2) (sum_k |x_jk b_k| + |o_j|) ulps of absolute error into mu_j, r_j, h_j (|dr/deta| = h, |dh/deta| <= h,
    |dt/deta| = |r|), and a wave-order sum of m terms adds (7 + m / 64) ulps of the sum of their magnitudes"""
    mp.mp.dps = 50
    m, p = x.shape
    M = lambda v: mp.mpf(float(v))
    a_, bb = M(a), [M(v) for v in b]
    F, g, H = mp.mpf(0), [mp.mpf(0)] * p, [[mp.mpf(0)] * p for _ in range(p)]
    tF, tg, tH = mp.mpf(0), [mp.mpf(0)] * p, [[mp.mpf(0)] * p for _ in range(p)]
    add = 8 + m // 64
    for j in range(m):
        o = mp.log(M(nf[j]))
        eta = sum(M(x[j, k]) * bb[k] for k in range(p)) + o
        E = (p + 2) * (sum(abs(M(x[j, k]) * bb[k]) for k in range(p)) + abs(o)) + 2
        mu = mp.exp(eta)
        yj, wj = M(y[j]), M(w[j])
        L = mp.log1p(a_ * mu)
        t = yj * eta - (yj + 1 / a_) * L
        r = (yj - mu) / (1 + a_ * mu)
        h = mu * (1 + a_ * yj) / (1 + a_ * mu) ** 2
        F -= wj * t
        tF += wj * (abs(r) * E + 6 * (abs(yj * eta) + (yj + 1 / a_) * L) + add * abs(t))
        for k in range(p):
            xk = M(x[j, k])
            g[k] -= wj * r * xk
            tg[k] += wj * abs(xk) * (h * E + (8 + add) * abs(r))
            for l in range(p):
                xl = M(x[j, l])
                H[k][l] += wj * h * xk * xl
                tH[k][l] += wj * abs(xk * xl) * h * (E + 10 + add)
    ds2, df1, ns2 = M(df) * M(Sc) ** 2, M(df) + 1, M(NS) ** 2
    for k in range(p):
        if no_shrink[k]:
            terms = (bb[k] ** 2 / (2 * ns2), bb[k] / ns2, 1 / ns2)
        else:
            den = ds2 + bb[k] ** 2
            terms = (df1 / 2 * mp.log1p(bb[k] ** 2 / ds2), df1 * bb[k] / den, df1 * (ds2 - bb[k] ** 2) / den ** 2)
            terms = terms[:2] + (terms[2],)
        F, g[k], H[k][k] = F + terms[0], g[k] + terms[1], H[k][k] + terms[2]
        tF += 8 * abs(terms[0]) + abs(F)
        tg[k] += 8 * abs(terms[1]) + abs(g[k])
        # (ds2 - b^2 cancels: its error is relative to ds2 + b^2)
        tH[k][k] += 8 * (df1 / (ds2 + bb[k] ** 2) if not no_shrink[k] else abs(terms[2])) + abs(H[k][k])
    return F, g, H, tF * EPS, [v * EPS for v in tg], [[v * EPS for v in row] for row in tH]


def _mp_newton_step(y, x, nf, w, a, no_shrink, Sc, b):
    """max |H^-1 g| at b in 50 digits"""
    _, g, H, *_ = _mp_posterior(y, x, nf, w, a, no_shrink, Sc, b)
    s = mp.lu_solve(mp.matrix(H), mp.matrix(g))
    return float(max(abs(v) for v in s))


def _case_rows(c):
    m = c["Y"].shape[1]
    nf = np.broadcast_to(np.asarray(c["nf"], np.float64), c["Y"].shape)
    w = np.ones(c["Y"].shape) if c["weights"] is None else c["weights"]
    return nf, w, m


def test_specification_against_50_digits(oracle):
    """F, gradient, Hessian, sd, fsr and thresh of the specification at its own optimum and at the start, each inside the
    bound its conditioning gives"""
    c = {k["name"]: k for k in AC.gpu_cases()}["f64_counts"]
    nf, w, m = _case_rows(c)
    p = c["x"].shape[1]
    T = c["threshold"]
    fit = S.fit(oracle, c["Y"], c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], weights=c["weights"], init=c["init"],
                threshold=T)
    worst = {}
    checked = 0
    for i in range(c["Y"].shape[0]):
        if np.isnan(fit["conv"][i]):
            continue
        post = S.Posterior(oracle, c["Y"][i], c["x"], nf[i], w[i], c["disp"][i], c["no_shrink"], c["S"])
        for b in (S.clip(c["init"][i]), fit["map"][i]):          # (the optimum last: H50 and tH are used below)
            F, g, H = post(b)
            F50, g50, H50, tF, tg, tH = _mp_posterior(c["Y"][i], c["x"], nf[i], w[i], c["disp"][i], c["no_shrink"], c["S"], b)
            ratios = [abs(mp.mpf(float(F)) - F50) / tF]
            ratios += [abs(mp.mpf(float(g[k])) - g50[k]) / tg[k] for k in range(p)]
            ratios += [abs(mp.mpf(float(H[k, l])) - H50[k][l]) / tH[k][l] for k in range(p) for l in range(p)]
            for nm, r in zip(["F"] + ["g"] * p + ["H"] * p * p, ratios):
                worst[nm] = max(worst.get(nm, 0.0), float(r))
        # sd, fsr, thresh at the optimum: H50 and the bound on H carried through the inverse and the normal tails
        Hm = mp.matrix(H50)
        inv = Hm ** -1
        cond = float(mp.norm(Hm, 2) * mp.norm(inv, 2))
        k = c["coef"]
        tvar = sum(abs(inv[k, r]) * tH[r][s] * abs(inv[s, k]) for r in range(p) for s in range(p)) + 8 * p * p * EPS * cond * inv[k, k]
        sd50 = mp.sqrt(inv[k, k])
        tsd = tvar / (2 * sd50) + 2 * EPS * sd50
        worst["sd"] = max(worst.get("sd", 0.0), float(abs(mp.mpf(float(fit["sd"][i, k])) - sd50) / tsd))
        mc = mp.mpf(float(fit["map"][i, k]))
        z = -abs(mc) / sd50
        tz = abs(z) * (tsd / sd50 + 2 * EPS)
        fsr50 = mp.ncdf(z)
        tfsr = mp.npdf(z) * tz + 16 * EPS * fsr50 + mp.mpf(2) ** -1074
        worst["fsr"] = max(worst.get("fsr", 0.0), float(abs(mp.mpf(float(fit["fsr"][i])) - fsr50) / tfsr))
        u1, u2 = (T - mc) / sd50, (-T - mc) / sd50
        th50 = mp.ncdf(u1) - mp.ncdf(u2)
        side = (lambda u: mp.ncdf(u)) if mc >= 0 else (lambda u: mp.ncdf(-u))
        tth = sum(mp.npdf(u) * abs(u) * (tsd / sd50 + 4 * EPS) + 16 * EPS * side(u) for u in (u1, u2)) + 2 * EPS * th50
        worst["thresh"] = max(worst.get("thresh", 0.0), float(abs(mp.mpf(float(fit["thresh"][i])) - th50) / tth))
        checked += 1
    print("error / bound, worst over %d rows:" % checked, {k: "%.3g" % v for k, v in worst.items()})
    assert checked >= 12
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- the comparison sets: four designs x seeds 11-14 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(oracle):
    """per (design, seed): the rows, the MLE start (the same search under a prior of scale 1e6: flat over the data's range),
    the scale, and the specification's fit"""
    out = []
    for dname, x in AC.prototype_designs().items():
        for seed, Sc in SCALES.items():
            d = AC.scipy_rows(seed, x, n=24)
            m, p = x.shape
            ns = np.zeros(p, bool)
            ns[0] = True
            flat = S.fit(oracle, d["Y"], x, d["nf"], d["disp"], p - 1, ns, 1e6, NS=1e6)
            init = flat["map"]
            if Sc is None:
                Sc = core.apeglm_prior_scale(np.stack([init[:, p - 1], flat["sd"][:, p - 1]], axis=1))
            fit = S.fit(oracle, d["Y"], x, d["nf"], d["disp"], p - 1, ns, Sc, init=init)
            out.append(dict(d, name="%s/%d" % (dname, seed), ns=ns, S=Sc, init=init, fit=fit))
    return out


def test_stopping_rule(oracle, sets):
    """no row whose 50-digit residual Newton step is below tol carries conv = 1 (or 2); and the rows that stopped with
    conv = 0 do sit where the 50-digit Newton step is below tol.  The pure Armijo rule, run on the same rows, fails this."""
    tol = 1e-8
    stuck, n, worst = [], 0, 0.0
    for s in sets:
        m = s["x"].shape[0]
        for i in range(s["Y"].shape[0]):
            conv = s["fit"]["conv"][i]
            step = _mp_newton_step(s["Y"][i], s["x"], s["nf"], np.ones(m), s["disp"][i], s["ns"], s["S"], s["fit"]["map"][i])
            n += 1
            if conv != 0 and step < tol:
                stuck.append((s["name"], i, conv, step))
            if conv == 0:
                worst = max(worst, step)
    print("rows %d, worst 50-digit residual Newton step on conv = 0 rows %.3g" % (n, worst))
    assert not stuck, stuck
    assert worst <= tol
    # rows found at the benchmark's shapes: F cancels to less than 1 while its terms sum to 1e4, so a resolution taken
    # relative to |F| rejected the last Newton steps for ever
    c = AC.on_optimum_rows()
    fit = S.fit(oracle, c["Y"], c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], init=c["init"])
    assert (fit["conv"] == 0).all() and (fit["iter"] < 20).all()
    for i in range(c["Y"].shape[0]):
        assert _mp_newton_step(c["Y"][i], c["x"], c["nf"], np.ones(48), c["disp"][i], c["no_shrink"], c["S"], fit["map"][i]) < tol
    pure = S.fit(oracle, c["Y"], c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], init=c["init"], resolution_clause=False)
    assert (pure["conv"] == 1).all()
    # the mutant: without the clause for a predicted decrease below the resolution of F, rows sit on the optimum and never stop
    mutant = 0
    for s in sets[:4]:
        m = s["x"].shape[0]
        for i in range(s["Y"].shape[0]):
            post = S.Posterior(oracle, s["Y"][i], s["x"], s["nf"], np.ones(m), s["disp"][i], s["ns"], s["S"])
            b, _, _, _, conv = S.search(post, S.start_a(oracle, s["Y"][i].astype(np.float64), s["nf"], np.ones(m), 2, s["ns"]),
                                        resolution_clause=False)
            if conv != 0 and _mp_newton_step(s["Y"][i], s["x"], s["nf"], np.ones(m), s["disp"][i], s["ns"], s["S"], b) < 10 * tol:
                mutant += 1
    assert mutant > 0


def test_specification_against_scipy(oracle, sets):
    """the specification's F is not above the best of scipy's L-BFGS-B from both starts by more than scipy's own stopping
    error, measured as the spread of scipy's F across its two starts where both reach the same point; rows where scipy finds
    a lower mode: at most 1 %"""
    from scipy.optimize import minimize
    rows, same_mode, lower, spread, excess, dist = 0, 0, [], 0.0, [], 0.0
    pending = []
    for s in sets:
        m, p = s["x"].shape
        for i in range(s["Y"].shape[0]):
            post = S.Posterior(oracle, s["Y"][i], s["x"], s["nf"], np.ones(m), s["disp"][i], s["ns"], s["S"])
            starts = (S.start_a(oracle, s["Y"][i].astype(np.float64), s["nf"], np.ones(m), p, s["ns"]), S.clip(s["init"][i]))
            rs = [minimize(lambda b: float(post(b)[0]), b0, jac=lambda b: post(b)[1], method="L-BFGS-B",
                           options=dict(ftol=1e-15, gtol=1e-10, maxiter=2000)) for b0 in starts]
            if np.abs(rs[0].x - rs[1].x).max() < 1e-4:
                spread = max(spread, abs(rs[0].fun - rs[1].fun))
            best = min(rs, key=lambda r: r.fun)
            pending.append((s["name"], i, s["fit"]["objective"][i], best.fun, np.abs(s["fit"]["map"][i] - best.x).max()))
            rows += 1
    for name, i, F, Fs, d in pending:
        if F > Fs + spread:
            (lower if d > 1e-3 else excess).append((name, i, F, Fs, d))
        elif d < 1e-3:
            same_mode += 1
            dist = max(dist, d)
    print("rows %d, scipy's stopping error in F %.3g, lower mode found by scipy on %d rows, same mode on %d rows, map distance %.3g"
          % (rows, spread, len(lower), same_mode, dist))
    assert rows >= 16 * 20                                 # (make_counts drops its all-zero rows)
    # scipy's own stopping error is the tolerance of every row: held to what ftol = 1e-15 can leave at F ~ 1e3-1e5
    assert spread <= 1e-9, spread
    assert not excess, excess
    assert len(lower) <= 0.01 * rows, lower
    assert same_mode >= 0.95 * rows
    assert dist <= 2 * MAP_DISTANCE


# ---- host engine == specification, to the bit ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wants(oracle):
    return {c["name"]: (c, S.fit(oracle, c["Y"], c["x"], c["nf"], c["disp"], c["coef"], c["no_shrink"], c["S"], weights=c["weights"],
                                 init=c["init"], threshold=c["threshold"], maxit=c["maxit"])) for c in AC.gpu_cases()}


def test_host_engine_equals_the_specification(oracle, wants):
    E = HostEngine(oracle)
    for name, (c, want) in wants.items():
        nf = np.asarray(c["nf"], np.float64)
        got = E.apeglm_fit(c["Y"], c["x"], nf if nf.ndim == 2 else None, c["disp"], c["coef"], c["no_shrink"], c["S"],
                           weights=c["weights"], init=c["init"], threshold=c["threshold"], maxit=c["maxit"],
                           sizeFactors=nf if nf.ndim == 1 else None)
        for key in AC.SPEC_KEYS:
            assert_same(got[key], want[key], "%s: %s" % (name, key))


def test_both_starts_win_and_the_listed_rows_are_there(wants):
    starts = np.concatenate([w["start"] for _, w in wants.values()])
    assert (starts == 0).sum() > 0 and (starts == 1).sum() > 0
    small = wants["small_scale"][1]["start"]
    assert (small == 1).sum() >= 3                         # S = 0.05 supplies the rows the second start wins
    c, w = wants["p4"]
    assert np.isnan(w["conv"][[0, 1, 6, 7]]).all() and np.isnan(w["objective"][[0, 1, 6, 7]]).all()     # all-zero, NaN / 0 / Inf dispersion
    assert (w["conv"][2:6] == 0).all()                     # a whole group zero, 2^31 - 1, a = 1e-8, a = 1e2
    assert (wants["maxit0"][1]["iter"] == 0)[~np.isnan(wants["maxit0"][1]["conv"])].all()
    c0, w0 = wants["maxit0"]
    fitted = ~np.isnan(w0["conv"])
    won_b = fitted & (w0["start"] == 1)
    assert_same(w0["map"][won_b], S.clip(c0["init"][won_b]), "maxit = 0 returns the start")
    assert ((w0["conv"][fitted] % 4) == 1).all()


# ---- s-values and the prior scale -----------------------------------------------------------------------------------------------
def test_svalue():
    lf = np.array([0.2, 0.01, np.nan, 0.2, 0.4, 0.01, 0.0, np.nan, 0.3])
    # R/lfcShrink.R:523-528 by hand: sorted 0, .01, .01, .2, .2, .3, .4, NA, NA; ranks with ties "first"
    srt = np.array([0.0, 0.01, 0.01, 0.2, 0.2, 0.3, 0.4, np.nan, np.nan])
    cm = np.cumsum(srt) / np.arange(1, 10)
    rank = np.array([4, 2, 8, 5, 7, 3, 1, 9, 6]) - 1
    assert_same(core.svalue(lf), cm[rank], "svalue by hand")
    rng = np.random.default_rng(1)
    v = np.round(rng.uniform(size=500), 2)
    v[rng.uniform(size=500) < 0.1] = np.nan
    assert_same(core.svalue(v), S.svalue(v), "svalue against the four lines")
    assert np.isnan(core.svalue(v)[np.isnan(v)]).all()


def test_prior_scale_is_the_root_of_its_equation():
    mp.mp.dps = 50
    rng = np.random.default_rng(2)
    for A_true, n in ((0.04, 400), (0.15, 250), (0.5, 300), (3.0, 200)):       # (the last one: the cap at 1)
        Sd = np.exp(rng.normal(-1.0, 0.5, n))
        D = rng.normal(0.0, np.sqrt(A_true + Sd ** 2))
        D[:5], Sd[5:8] = np.nan, np.inf                    # rows that are left out
        got = core.apeglm_prior_scale(np.stack([D, Sd], axis=1))
        keep = np.isfinite(D) & np.isfinite(Sd)
        eq = lambda A: mp.fsum((mp.mpf(d) ** 2 - mp.mpf(s) ** 2 - A) / (mp.mpf(s) ** 2 + A) ** 2 for d, s in zip(D[keep], Sd[keep]))
        root = mp.findroot(eq, mp.mpf(A_true))
        want = min(float(mp.sqrt(root)), 1.0)
        assert (want == 1.0) == (A_true == 3.0)
        # the fixed point stops at a relative change of 1e-12 and converges linearly: within 1e-10 of the root
        assert abs(got - want) <= 1e-10 * want, (got, want)
        assert abs(S.prior_scale_equation(float(root), D[keep], Sd[keep])) < 1e-6
    assert core.apeglm_prior_scale(np.array([[0.001, 1.0], [-0.002, 1.0], [0.0, 2.0]])) == 1e-6          # the floor
    with pytest.raises(ValueError):
        core.apeglm_prior_scale(np.array([[np.nan, 1.0]]))


def test_argument_errors_of_the_c_entries():
    """DSQ_ERR_ARG for coef inside no_shrink or out of range and for a scale or df that is not positive and finite,
    DSQ_ERR_UNSUPPORTED beyond DSQ_APEGLM_MAX_P: decided from the argument block, before a device is asked for"""
    import ctypes as C
    from deseq2_amd import _lib as L
    n, m, p = 3, 5, 17
    buf = {k: np.zeros(n * m * p) for k in ("y", "nf", "x", "disp", "map", "sd", "fsr", "thresh", "iter", "conv", "start", "objective")}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = dict(n=n, m=m, p=2, layout=L.DSQ_LAYOUT_R, ld=0, y=ptr(buf["y"]), y_type=L.DSQ_Y_FLOAT64, nf=ptr(buf["nf"]), nf_is_vector=1,
                x=ptr(buf["x"]), weights=None, disp=ptr(buf["disp"]), init=None, coef=1, no_shrink=1, prior_scale=0.3, prior_df=1.0,
                no_shrink_scale=15.0, has_threshold=0, threshold=0.0, tol=1e-8, maxit=100)
    o = L.DsqApeglmOut(bad=None, **{k: ptr(buf[k]) for k in ("map", "sd", "fsr", "thresh", "iter", "conv", "start", "objective")})
    cases = [(dict(coef=0), L.DSQ_ERR_ARG), (dict(coef=1, no_shrink=3), L.DSQ_ERR_ARG), (dict(coef=2), L.DSQ_ERR_ARG),
             (dict(coef=-1), L.DSQ_ERR_ARG), (dict(prior_scale=0.0), L.DSQ_ERR_ARG), (dict(prior_scale=-1.0), L.DSQ_ERR_ARG),
             (dict(prior_scale=np.inf), L.DSQ_ERR_ARG), (dict(prior_scale=np.nan), L.DSQ_ERR_ARG), (dict(prior_df=0.0), L.DSQ_ERR_ARG),
             (dict(prior_df=np.nan), L.DSQ_ERR_ARG), (dict(no_shrink_scale=0.0), L.DSQ_ERR_ARG), (dict(no_shrink=4), L.DSQ_ERR_ARG),
             (dict(has_threshold=1, threshold=-0.5), L.DSQ_ERR_ARG), (dict(maxit=-1), L.DSQ_ERR_ARG), (dict(tol=np.nan), L.DSQ_ERR_ARG),
             (dict(disp=None), L.DSQ_ERR_ARG), (dict(p=17, coef=16), L.DSQ_ERR_UNSUPPORTED), (dict(p=17, coef=1), L.DSQ_ERR_UNSUPPORTED)]
    lib = L.lib()
    for change, want in cases:
        a = L.DsqApeglmArgs(**dict(good, **change))
        for rc in (lib.dsq_apeglm(C.byref(a), C.byref(o)), lib.dsq_apeglm_dev(C.byref(a), C.byref(o), None)):
            assert rc == want, (change, rc)
            assert lib.dsq_last_error()
    assert all((v == 0).all() for v in buf.values())          # nothing was written


# ---- tests/testthat/test_lfcShrink.R through lfcShrinkApeglm --------------------------------------------------------------------
def _f2():
    return OrderedDict(condition=np.repeat([0, 1], 6))


@pytest.fixture(scope="module")
def two(oracle):
    from tests.lfcshrink_cases import counts
    f = _f2()
    x, _ = core.standard_model_matrix(f)
    k = counts(200, x, 5)
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f, minReplicatesForReplace=np.inf)
    return dds, k, x


def test_reference_expectations(oracle, two, capsys):
    dds, k, x = two
    with pytest.raises(RuntimeError, match="first run DESeq\\(\\) before running lfcShrink\\(\\)"):       # test_lfcShrink.R:7
        core.lfcShrinkApeglm(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), coef=1)
    res = core.results(dds, name=1)
    half = core.results(core.DESeq(core.DESeqDataSet(k[:100], x, engine=dds.engine), minReplicatesForReplace=np.inf), name=1)
    with pytest.raises(ValueError, match="rownames"):                             # :14
        core.lfcShrinkApeglm(dds, coef=1, res=half, quiet=True)
    with pytest.raises(ValueError, match="'coef' should specify same coefficient as in results 'res'"):   # :82-83
        core.lfcShrinkApeglm(dds, coef=1, res=core.results(dds, name=0), quiet=True)
    ape = core.lfcShrinkApeglm(dds, coef=1)                                       # :24
    err = capsys.readouterr().err
    assert "using 'apeglm' for LFC shrinkage" in err and "bty895" in err
    assert ape.columns == ["baseMean", "log2FoldChange", "lfcSE", "pvalue", "padj"]
    assert ape.priorInfo["type"] == "apeglm" and ape.priorInfo["prior_control"]["no_shrink"] == [0]
    assert 0 < ape.priorInfo["prior_control"]["prior_scale"] <= 1 and ape.metadata["lfcThreshold"] == 0
    assert ape.metadata["description"]["log2FoldChange"].startswith("log2 fold change (MAP)")
    assert ape.metadata["description"]["lfcSE"].startswith("posterior SD")
    assert_same(ape["pvalue"], res["pvalue"], "the p-values are the results' own")
    dds.attrs["coefNames"] = ["Intercept", "condition_B_vs_A"]
    try:
        by_name = core.lfcShrinkApeglm(dds, coef="condition_B_vs_A", res=core.results(dds, name=1), quiet=True)
    finally:
        del dds.attrs["coefNames"]
    assert_same(by_name["log2FoldChange"], ape["log2FoldChange"], "coef by name")
    # shrinkage: towards zero on the whole, large effects kept
    mle, shr = np.asarray(res["log2FoldChange"]), np.asarray(ape["log2FoldChange"])
    ok = np.isfinite(mle) & np.isfinite(shr)
    assert np.abs(shr[ok]).sum() < np.abs(mle[ok]).sum() and (np.abs(shr[ok]) <= np.abs(mle[ok]) + 1e-6).mean() > 0.95
    sv = core.lfcShrinkApeglm(dds, coef=1, svalue=True, quiet=True)              # :58-59
    assert sv.columns == ["baseMean", "log2FoldChange", "lfcSE", "svalue"] and "svalue" in sv
    assert sv.metadata["description"]["svalue"] == "s-value: coef1"
    thr = core.lfcShrinkApeglm(dds, coef=1, lfcThreshold=1)                       # :49
    assert "computing FSOS 'false sign or small' s-values (T=1)" in capsys.readouterr().err
    assert "svalue" in thr.columns and thr.metadata["description"]["svalue"] == "FSOS s-value (T=1): coef1"
    assert thr.metadata["lfcThreshold"] == 1
    lst = core.lfcShrinkApeglm(dds, coef=1, returnList=True, lfcThreshold=1, quiet=True)              # :73
    assert isinstance(lst, tuple) and set(lst[1]) == {"map", "sd", "fsr", "svalue", "interval", "diag", "thresh", "prior_control"}
    assert_same(thr["svalue"], core.svalue(lst[1]["thresh"]), "FSOS s-values are the s-values of P(|b| < T)")
    assert_same(np.asarray(lst[0]["log2FoldChange"]), float.fromhex("0x1.71547652b82fep+0") * lst[1]["map"][:, 1], "log2(e) map")


def test_user_supplied_matrix_and_the_route_without_a_wald_test(oracle, two):
    dds, k, x = two
    plain = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), minReplicatesForReplace=np.inf)          # :86-90: no factors
    a = core.lfcShrinkApeglm(plain, coef=1, res=core.results(plain), quiet=True)
    b = core.lfcShrinkApeglm(dds, coef=1, quiet=True)
    assert_same(a["log2FoldChange"], b["log2FoldChange"], "a user-supplied matrix")
    # apeAdapt = FALSE needs dispersions only (R/lfcShrink.R:176-180)
    kz = k[(k != 0).any(axis=1)]                           # (estimateDispersions is served on rows that are not all zero)
    d = core.DESeqDataSet(kz, x, engine=HostEngine(oracle))
    with pytest.raises(RuntimeError, match="require dispersion estimates"):
        core.lfcShrinkApeglm(d, coef=1, apeAdapt=False, quiet=True)
    d = core.estimateDispersions(core.estimateSizeFactors(d))
    assert "beta" not in d.mcols
    r, fit = core.lfcShrinkApeglm(d, coef=1, apeAdapt=False, returnList=True, quiet=True)
    assert fit["prior_control"]["prior_scale"] == 1.0 and (fit["diag"]["start"] == 0).all()
    assert np.isfinite(np.asarray(r["log2FoldChange"])).all() and r.n == kz.shape[0]
    assert r.columns == ["baseMean", "log2FoldChange", "lfcSE", "pvalue", "padj"] and np.isnan(r["pvalue"]).all()


def test_pinned_refusals(two):
    dds, _, _ = two
    with pytest.raises(NotImplementedError, match="lfcShrinkApeglm"):
        core.lfcShrink(dds, coef=1, type="apeglm")
    for kw in (dict(svalue=True), dict(returnList=True), dict(apeAdapt=False, apeMethod="nbinomC")):
        with pytest.raises(NotImplementedError, match="lfcShrinkApeglm"):
            core.lfcShrink(dds, coef=1, **kw)
    assert core.lfcShrink.__defaults__[3] == "normal"
    for kw in (dict(apeMethod="general"), dict(format="GRanges"), dict(saveCols=[0]), dict(parallel=True)):
        with pytest.raises(NotImplementedError):
            core.lfcShrinkApeglm(dds, coef=1, quiet=True, **kw)
    with pytest.raises(TypeError):
        core.lfcShrinkApeglm(dds, coef=1, shrink=True)
    with pytest.raises(ValueError):
        core.lfcShrinkApeglm(dds, coef=0, quiet=True)                             # the intercept is not shrunk
    with pytest.raises(ValueError, match="coef"):
        core.lfcShrinkApeglm(dds, coef=5, quiet=True)
    with pytest.raises(ValueError, match="lfcThreshold"):
        core.lfcShrinkApeglm(dds, coef=1, lfcThreshold=-1, quiet=True)
