"""No GPU: the budgets of tests/hp_reference.py measured, and the proof that they bite.

On every case that tests/test_gpu_hp.py runs, the independent numpy restatement (oracle/lapack_oracle.py) must stay
within K / 4 of the 50-digit values and the C oracle within K (K: hp_reference.BUDGETS; the ratios are printed, run with
-s to see them).  Then mutants of the numpy restatement -- a dropped sample, a sample read from its neighbour, w for
sqrt(w) sqrt(w) in the hat diagonal, no ridge in A, db for d2b, no inner usePrior = false term, >= for > at a weight equal
to the threshold -- must each exceed a budget by 10 x or more at EVERY shape they apply to: a shape that cannot see a
mutant would be a shape (or a magnitude) that checks nothing."""
import numpy as np
import pytest
from scipy import special

from oracle import lapack_oracle as LO
from tests import hp_reference as H

THR = H.WEIGHT_THRESHOLD
DISP_KEYS = (("lp", "initial_lp"), ("dlp", "initial_dlp"), ("d2lp", "last_d2lp"))
POST_KEYS = ("beta_var_mat", "hat_diagonals", "contrast_num", "contrast_denom")


def _disp_args(c, prior, useCR=True, y=None, sl=slice(None)):
    y = c["y"] if y is None else y
    return (y[:, sl], c["x"][sl], c["mu"][:, sl], c["log_alpha"], c["prior_mean"], c["sigmasq"], np.log(1e-9), 1.0, 1e-6, 0,
            prior, c["weights"][:, sl], c["useWeights"], THR, useCR)


def _disp_ratios(c, fro, out, prior):
    return {k: max(H.ratio(out[ko][i], *fro[i][prior][k]) for i in range(c["n"])) for k, ko in DISP_KEYS}


@pytest.mark.parametrize("shape", H.DISP_SHAPES, ids=H.shape_id)
def test_disp_budgets_hold_for_both_oracles(oracle, shape):
    c, fro, grd = H.disp_reference(shape)
    ties = 0
    for prior in (False, True):
        for name, O, div in (("lapack_oracle", LO, 4.0), ("C oracle", oracle, 1.0)):
            r = _disp_ratios(c, fro, O.fitDisp(*_disp_args(c, prior)), prior)
            print("%s %s prior=%d %s" % (H.shape_id(shape), name, prior, {k: round(v, 3) for k, v in r.items()}))
            for k, v in r.items():
                assert v <= H.BUDGETS[k] / div, "%s %s: ratio %.3g over K%s = %g" % (name, k, v, "/4" if div > 1 else "", H.BUDGETS[k] / div)
        g = LO.fitDispGrid(c["y"], c["x"], c["mu"], c["grid"], c["prior_mean"], c["sigmasq"], prior, c["weights"],
                           c["useWeights"], THR, True)["log_alpha"]
        for i in range(c["n"]):
            a_mp, stages = grd[i][prior]
            tie = any(gap < H.BUDGETS["lp"] * H.U * M for gap, M in stages)
            ties += tie
            assert tie or abs(g[i] - a_mp) <= 1e-9 * (c["grid"][1] - c["grid"][0]), (i, g[i], a_mp)
    assert ties <= 0.02 * 2 * c["n"]


@pytest.mark.parametrize("shape", [("factor", 3, 24, True), ("factor", 2, 16, True)], ids=H.shape_id)
def test_disp_budgets_hold_without_cox_reid(oracle, shape):
    c, fro, _ = H.disp_reference(shape, False)
    for prior in (False, True):
        for name, O, div in (("lapack_oracle", LO, 4.0), ("C oracle", oracle, 1.0)):
            r = _disp_ratios(c, fro, O.fitDisp(*_disp_args(c, prior, useCR=False)), prior)
            print("%s useCR=0 %s prior=%d %s" % (H.shape_id(shape), name, prior, {k: round(v, 3) for k, v in r.items()}))
            for k, v in r.items():
                assert v <= H.BUDGETS[k] / div, "%s %s: ratio %.3g over %g" % (name, k, v, H.BUDGETS[k] / div)


# ---- a copy of the numpy restatement's derivative functions, with the mutations ---------------------------------------
def _np_disp(c, prior, mut):
    """lapack_oracle's log_posterior / dlog_posterior / d2log_posterior at maxit = 0, restated with a mutation switch"""
    out = {k: np.zeros(c["n"]) for _, k in DISP_KEYS}
    x = c["x"]
    for i in range(c["n"]):
        la, y, mu, w = c["log_alpha"][i], c["y"][i].astype(float), c["mu"][i], c["weights"][i]
        alpha = np.exp(la)

        def mats(orders):
            base = 1.0 / mu + alpha
            diags = [base ** -1.0, -1.0 * base ** -2.0, 2.0 * base ** -3.0][:orders]
            xx = x
            if c["useWeights"]:
                keep = (w >= THR) if mut == "ge_threshold" else (w > THR)
                xx = x[keep]
                xx = xx[:, np.abs(xx).sum(axis=0) > 0.0]
                diags = [d[keep] for d in diags]
            return [xx.T @ (xx * d[:, None]) for d in diags]

        an1, an2 = 1.0 / alpha, alpha ** -2.0
        ws = w if c["useWeights"] else 1.0
        t0 = special.gammaln(y + an1) - special.gammaln(an1) - y * np.log(mu + an1) - an1 * np.log(1.0 + mu * alpha)
        (b,) = mats(1)
        lp = np.sum(ws * t0) - 0.5 * np.log(np.linalg.det(b))
        t1 = LO._dll_terms(y, mu, alpha)
        b, db = mats(2)
        dlp0 = (an2 * np.sum(ws * t1) - 0.5 * np.trace(np.linalg.inv(b) @ db)) * alpha
        t2 = (-1 * an2 * special.polygamma(1, an1) + mu ** 2 * alpha * (1 + mu * alpha) ** -2.0
              + an2 * special.polygamma(1, y + an1) + an2 * y * (mu + an1) ** -2.0)
        b, db, d2b = mats(3)
        if mut == "db_for_d2b":
            d2b = db
        bi = np.linalg.inv(b)
        tr = np.trace(bi @ db)
        cr = 0.5 * tr ** 2 - 0.5 * (tr ** 2 - np.trace(bi @ db @ bi @ db) + np.trace(bi @ d2b))
        ll = -2 * alpha ** -3.0 * np.sum(ws * t1) + an2 * np.sum(ws * t2)
        d2 = (ll + cr) * alpha ** 2 + (0.0 if mut == "no_inner" else dlp0)
        if prior:
            lp += -0.5 * (la - c["prior_mean"][i]) ** 2 / c["sigmasq"]
            dlp0 = dlp0 + -1.0 * (la - c["prior_mean"][i]) / c["sigmasq"]
            d2 += -1.0 / c["sigmasq"]
        out["initial_lp"][i], out["initial_dlp"][i], out["last_d2lp"][i] = lp, dlp0, d2
    return out


def _excess(ratios):
    return max(v / H.BUDGETS[k] for k, v in ratios.items())


@pytest.mark.parametrize("shape", H.DISP_SHAPES, ids=H.shape_id)
def test_disp_mutants_exceed_the_budget(shape):
    c, fro, _ = H.disp_reference(shape)
    base = _np_disp(c, True, None)
    ref = LO.fitDisp(*_disp_args(c, True))
    for _, ko in DISP_KEYS:                               # the copy is the restatement: same values to a few ulp
        np.testing.assert_allclose(base[ko], ref[ko], rtol=1e-9, atol=1e-9)
    assert _excess(_disp_ratios(c, fro, base, True)) <= 1.0
    shifted = c["y"].copy(); shifted[:, -1] = shifted[:, -2]
    mutants = {"drop_last": LO.fitDisp(*_disp_args(c, True, sl=slice(0, c["m"] - 1))),
               "shift": LO.fitDisp(*_disp_args(c, True, y=shifted)),
               "db_for_d2b": _np_disp(c, True, "db_for_d2b"), "no_inner": _np_disp(c, True, "no_inner")}
    if c["useWeights"]:
        mutants["ge_threshold"] = _np_disp(c, True, "ge_threshold")
    for name, out in mutants.items():
        e = _excess(_disp_ratios(c, fro, out, True))
        print("%s mutant %s: %.3g x the budget" % (H.shape_id(shape), name, e))
        assert e >= 10.0, "mutant %s is invisible at %s: %.3g x the budget" % (name, H.shape_id(shape), e)


# ---- fitBeta ---------------------------------------------------------------------------------------------------------------
def _beta_ratios(c, post, step, o0, o1):
    n, p = c["n"], c["p"]
    r = {}
    for k in POST_KEYS:
        got = np.asarray(o0[k]).reshape(n, -1)
        r[k] = max(H.ratio(got[i, j], post[i][k][0][j], post[i][k][1][j]) for i in range(n) for j in range(got.shape[1]))
    r["beta_step"] = max(H.ratio(o1["beta_mat"][i, k], step[i][0][k], step[i][1]) for i in range(n) for k in range(p))
    devs = [H.ratio(o1["deviance"][i], *step[i][2]) for i in range(n) if step[i][2] is not None]
    assert devs, "no gene of the case keeps its one-step beta inside the box: the deviance is not exercised"
    r["deviance"] = max(devs)
    return r


def _beta_run(O, c, useQR, y=None, sl=slice(None), lam=None):
    y = c["y"] if y is None else y
    lam = c["lam"] if lam is None else lam
    a = (y[:, sl], c["x"][sl], c["nf"][:, sl], np.exp(c["log_alpha"]), c["contrast"])
    b = (lam, c["weights"][:, sl], c["useWeights"], 1e-8)
    return O.fitBeta(*a, c["beta_drawn"], *b, 0, useQR, c["minmu"]), O.fitBeta(*a, c["beta_start"], *b, 1, useQR, c["minmu"])


@pytest.mark.parametrize("shape", H.BETA_SHAPES, ids=H.shape_id)
def test_beta_budgets_hold_and_mutants_exceed_them(oracle, shape):
    c, post, step = H.beta_reference(shape)
    for useQR in (True, False):
        for name, O, div in (("lapack_oracle", LO, 4.0), ("C oracle", oracle, 1.0)):
            o0, o1 = _beta_run(O, c, useQR)
            assert (np.asarray(o0["deviance"]) == 0).all() and (np.asarray(o0["iter"]) == 0).all()
            assert (np.asarray(o1["iter"]) == 1).all()
            for i in range(c["n"]):
                if step[i][2] is None:
                    assert o1["deviance"][i] == 0.0
            r = _beta_ratios(c, post, step, o0, o1)
            print("%s %s useQR=%d %s" % (H.shape_id(shape), name, useQR, {k: float("%.3g" % v) for k, v in r.items()}))
            for k, v in r.items():
                assert v <= H.BUDGETS[k] / div, "%s %s: ratio %.3g over %g" % (name, k, v, H.BUDGETS[k] / div)
    # mutants: through the restatement on mutated inputs, and a copy of its post-fit block (oracle/lapack_oracle.py:227-238)
    shifted = c["y"].copy(); shifted[:, -1] = shifted[:, -2]
    m = c["m"]
    o0, o1 = _beta_run(LO, c, False)

    def pad(o):               # a dropped sample has no hat diagonal: compare the others
        o = dict(o); o["hat_diagonals"] = np.column_stack([o["hat_diagonals"], o0["hat_diagonals"][:, -1]])
        return o
    d0, d1 = _beta_run(LO, c, False, sl=slice(0, m - 1))
    mutants = {"drop_last": (pad(d0), d1), "shift": _beta_run(LO, c, False, y=shifted),
               "no_ridge": _beta_run(LO, c, False, lam=np.zeros(c["p"]))}
    hat_w = dict(o0)
    alpha = np.exp(c["log_alpha"])
    mu = np.maximum(c["nf"] * np.exp(c["beta_drawn"] @ c["x"].T), c["minmu"])
    w = (c["weights"] * mu if c["useWeights"] else mu) / (1.0 + alpha[:, None] * mu)
    hat_w["hat_diagonals"] = o0["hat_diagonals"] * w                 # (x w)' inv (x w) = w * [sqrt(w) x]' inv [sqrt(w) x]
    mutants["w_for_sqrt_w"] = (hat_w, o1)
    for name, (m0, m1) in mutants.items():
        e = _excess(_beta_ratios(c, post, step, m0, m1))
        print("%s mutant %s: %.3g x the budget" % (H.shape_id(shape), name, e))
        assert e >= 10.0, "mutant %s is invisible at %s: %.3g x the budget" % (name, H.shape_id(shape), e)


# ---- the aux routines: a plain numpy restatement of each (written here: lapack_oracle has none), and the C oracle -----------
def _trim_mean(v, trim):
    lo = int(np.floor(len(v) * trim))
    return np.sort(v)[lo:len(v) - lo].mean()


def np_aux(shape, c):
    name, y, nf, w, useW = shape[0], c["y"].astype(float), c["nf"], c["weights"], c["useWeights"]
    yn = y / nf
    if name == "nbinomLogLike":
        size = (1.0 / np.exp(c["log_alpha"]))[:, None]
        mu = c["mu"]
        with np.errstate(all="ignore"):
            t = (special.gammaln(y + size) - special.gammaln(size) - special.gammaln(y + 1) + size * np.log(size / (size + mu))
                 + np.where(y > 0, y * np.log(mu / (size + mu)), 0.0))
        return np.sum(w * t if useW else t, axis=1)
    if name == "linearMu":
        mu = nf * ((yn @ c["q"]) @ c["a"].T)
        return np.maximum(mu, c["mu_floor"]) if c["mu_floor"] > 0 else mu
    if name == "prefitMoments":
        v = w * yn if useW else yn
        mu = np.maximum(1.0, (yn @ c["q"]) @ c["a"].T)
        est = (((yn - mu) ** 2 - mu) / mu ** 2).sum(axis=1) / (c["m"] - c["p"])
        return {"baseMean": v.mean(axis=1), "baseVar": v.var(axis=1, ddof=1), "allZero": y.sum(axis=1) == 0,
                "roughDisp": np.maximum(est, 0.0), "beta_init": np.linalg.solve(c["r"], c["q"].T @ np.log(yn + 0.1).T).T}
    _, cell = np.unique(c["x"], axis=0, return_inverse=True)
    cell = cell.reshape(-1)
    sizes = np.bincount(cell)
    out = {"cooks": np.zeros_like(yn), "maxCooks": np.zeros(c["n"]), "robustDisp": np.zeros(c["n"])}
    tr, sc = [1 / 3, 1 / 4, 1 / 8], [2.04, 1.86, 1.51]
    keep = sizes[cell] >= 3
    for i in range(c["n"]):
        vs = []
        for k in np.flatnonzero(sizes >= 3):
            b = 0 if sizes[k] <= 3.5 else 1 if sizes[k] <= 23.5 else 2
            sub = yn[i, cell == k]
            vs.append(sc[b] * _trim_mean((sub - _trim_mean(sub, tr[b])) ** 2, tr[b]))
        v = max(vs) if vs else 1.51 * _trim_mean((yn[i] - _trim_mean(yn[i], 1 / 8)) ** 2, 1 / 8)
        mean = yn[i].mean()
        alpha = max((v - mean) / mean ** 2, 0.04)
        mu, Hh = c["mu_fit"][i], c["H"][i]
        ck = (y[i] - mu) ** 2 / (mu + alpha * mu ** 2) / c["p"] * Hh / (1 - Hh) ** 2
        out["cooks"][i], out["robustDisp"][i] = ck, alpha
        out["maxCooks"][i] = ck[keep].max() if c["m"] > c["p"] and keep.any() else np.nan
    return out


def c_aux(O, shape, c):
    name = shape[0]
    if name == "nbinomLogLike":
        return O.nbinomLogLike(c["y"], c["mu"], np.exp(c["log_alpha"]), c["weights"], c["useWeights"])
    if name == "linearMu":
        return O.linearMu(c["y"], c["nf"], c["x"], c["mu_floor"])
    if name == "prefitMoments":
        return O.prefitMoments(c["y"], c["nf"], c["x"], c["weights"], c["useWeights"])
    return O.cooksDistance(c["y"], c["nf"], c["mu_fit"], c["H"], c["x"])


@pytest.mark.parametrize("shape", H.AUX_SHAPES, ids=H.aux_id)
def test_aux_budgets_hold_for_numpy_and_c_oracle(oracle, shape):
    c, ref = H.aux_reference(shape)
    for name, got, div in (("numpy", np_aux(shape, c), 4.0), ("C oracle", c_aux(oracle, shape, c), 1.0)):
        worst = {}
        for fam, i, v, rv, M in H.aux_items(shape, c, ref, got):
            worst[fam] = max(worst.get(fam, 0.0), H.ratio(v, rv, M))
        print("%s %s %s" % (H.aux_id(shape), name, {k: float("%.3g" % v) for k, v in worst.items()}))
        for k, v in worst.items():
            assert v <= H.BUDGETS[k] / div, "%s %s: ratio %.3g over %g" % (name, k, v, H.BUDGETS[k] / div)
    # a dropped last sample must show in every output family of the case
    cut = dict(c)
    m1 = c["m"] - 1
    for k in ("y", "nf", "mu", "weights", "mu_fit", "H"):
        if k in c:
            cut[k] = np.column_stack([c[k][:, :m1], np.zeros(c["n"]) if k == "y" else c[k][:, m1]]).astype(c[k].dtype)
    if shape[0] != "cooksDistance":                       # (a count read as zero: Cook's own sample would only move one entry)
        got = np_aux(shape, cut)
        e = max(H.ratio(v, rv, M) / H.BUDGETS[fam] for fam, i, v, rv, M in H.aux_items(shape, c, ref, got))
        print("%s mutant last count dropped: %.3g x the budget" % (H.aux_id(shape), e))
        assert e >= 10.0


def test_nb_density_and_poisson_limit():
    """the direct NB form against the Poisson limit at size 1e12, and against scipy at a moderate size"""
    for y, mu in ((0, 0.5), (3, 2.5), (40, 55.0), (2 ** 20, 1e6)):
        nb = H.mp.fsum(H.nb_logpmf_parts(y, float(mu), H.mp.mpf(10) ** 12))
        po = H.mp.fsum(H.pois_logpmf_parts(y, float(mu)))
        assert abs(nb - po) <= 2.0 * ((y - mu) ** 2 + y + mu + 1.0) / 1e12, (y, mu, nb, po)
        from scipy.stats import nbinom
        ref = nbinom.logpmf(y, 5.0, 5.0 / (5.0 + mu))
        assert abs(float(H.mp.fsum(H.nb_logpmf_parts(y, float(mu), H.mp.mpf(5)))) - ref) <= 1e-9 * abs(ref)
