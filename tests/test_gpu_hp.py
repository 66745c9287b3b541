"""-m gpu: the HIP library, through deseq2_amd.native, against the 50-digit statement of tests/hp_reference.py.

With the iteration frozen (fitDisp and fitBeta at maxit = 0, fitBeta at maxit = 1, fitDispGrid, which has no search
state) every output is a closed-form function of the inputs, and is held to |hip - mp| <= K u M on EVERY gene: K from
hp_reference.BUDGETS (measured on the CPU against the numpy restatement, never against this library), M the magnitude of
the sum or solve being checked.  The flags are exact.  This pins the VALUE of every per-gene function against a reference
that shares no arithmetic with it; the control flow of the searches stays with test_gpu_vs_lapack.py and the bitwise suites.

Shape -> kernel variant (from launch_fit_disp_p / launch_disp_p / fit_disp_rolled_applies in csrc/fit_disp*.hip and
launch_fit_beta_p / beta_geometry / launch_fit_beta_rolled in csrc/fit_beta*.hip; the DSQ_VERBOSE=1 lines of a run name
the variant each launch took):

  fitDisp / fitDispGrid                                      (p, m)
    cell-collapsed, p < 4 / p >= 4                           (2, 6) (3, 64) (3, 65) (10, 130)
    distinct-count histogram on / off (256 <= m <= 2560)     factor-10 at m = 255, 256, 2560, 2561
    unstaged long rows, distinct counts in global memory     (10, 2000) factor; (3, 1500) with weights
    weights: whole samples at zero, a weight == threshold,   (3, 24) (2, 16), also with useCR off
      a dropped column
    general path (a continuous covariate), sweep Gram        (5, 40) (4, 500)
    general path, serial Gram and its limits                 (7, 256) (7, 257) (10, 1024) (10, 1025)
      (include/dsq_arith_spec.h: p >= 7 up to m = 256, p >= 10 up to m = 1024)
    rolled wide kernel, default geometry                     (12, 60) paired (31, 60) 48-level factor (48, 96)
                                                             (64, 130) with weights
    rolled wide kernel, DSQ_WIDE_NW = 1 and 8                (31, 60)

  fitBeta                                                    (p, m)
    cell kernel (launch_beta_cells: cells + p <= 64)         (2, 6) (3, 500) (10, 2000) (3, 37) weights
    general, staged / unstaged                               (4, 100) (4, 1500)
    rows in registers, one trip / two trips and beyond       (7, 249) (7, 250) (10, 502) (10, 503)
    stored rows in LDS (p = 10) / replay beyond its budget   (10, 600) (10, 2000) continuous
    rolled (slab in LDS): 1 wave per gene                    (12, 60)
            2 waves per gene (the default at p = 31)         (31, 60)
            8 waves per gene                                 (48, 96) (64, 130)
            DSQ_WIDE_NW = 1, 4 and 8                         (31, 60)   (no listed shape takes 4 waves by itself)

  aux kernels, host ABI and _dev ABI (gene-major resident inputs)
    nbinomLogLike (7) (1500, weights); linearMu (3, 24) floored, (10, 130), (3, 500); prefitMoments (2, 6),
    (3, 500, weights); cooksDistance (3, 12), (2, 1000) with mu and H from the mp statement of a maxit = 0 fit
"""
import numpy as np
import pytest

from deseq2_amd import native
from tests import hp_reference as H

pytestmark = pytest.mark.gpu

THR = H.WEIGHT_THRESHOLD


def _check(failures, what, gene, m, value, ref, M, K):
    r = H.ratio(value, ref, M) if np.isfinite(value) else float("inf")
    if not r <= K:
        failures.append("%s: gene %d, m = %d: ratio %.3g over the budget K = %g (hip %r, mp %s)"
                        % (what, gene, m, r, K, float(value), H.mp.nstr(ref, 20)))
    return r


def _disp_case(shape, useCR=True):
    c, fro, grd = H.disp_reference(shape, useCR)
    fails, worst, ties = [], {}, 0
    for prior in (False, True):
        o = native.fitDisp(c["y"], c["x"], c["mu"], c["log_alpha"], c["prior_mean"], c["sigmasq"], np.log(1e-9), 1.0, 1e-6,
                           0, prior, c["weights"], c["useWeights"], THR, useCR)
        assert (o["iter"] == 0).all() and (o["iter_accept"] == 0).all() and (o["last_change"] == -1.0).all()
        assert (o["log_alpha"] == c["log_alpha"]).all()
        assert (o["initial_lp"] == o["last_lp"]).all() and (o["initial_dlp"] == o["last_dlp"]).all()
        for k, ko in (("lp", "initial_lp"), ("dlp", "initial_dlp"), ("d2lp", "last_d2lp")):
            for i in range(c["n"]):
                v, M = fro[i][prior][k]
                r = _check(fails, "fitDisp$%s (prior %s)" % (ko, prior), i, c["m"], o[ko][i], v, M, H.BUDGETS[k])
                worst[k] = max(worst.get(k, 0.0), r)
        g = native.fitDispGrid(c["y"], c["x"], c["mu"], c["grid"], c["prior_mean"], c["sigmasq"], prior, c["weights"],
                               c["useWeights"], THR, useCR)["log_alpha"]
        delta = c["grid"][1] - c["grid"][0]
        for i in range(c["n"]):
            a_mp, stages = grd[i][prior]
            tie = any(gap < H.BUDGETS["lp"] * H.U * M for gap, M in stages)
            ties += tie
            if not tie and not abs(g[i] - a_mp) <= 1e-9 * delta:
                fails.append("fitDispGrid (prior %s): gene %d, m = %d: %r, the mp argmax is %r (gaps / (u M): %s)"
                             % (prior, i, c["m"], g[i], a_mp, [float(gap / (H.U * M)) for gap, M in stages]))
    assert ties <= 0.02 * 2 * c["n"], "%d ties among %d grid results" % (ties, 2 * c["n"])
    print("hp ratios %s useCR=%d: %s" % (H.shape_id(shape), useCR, {k: round(v, 3) for k, v in worst.items()}))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", H.DISP_SHAPES, ids=H.shape_id)
def test_fit_disp_frozen_and_grid_vs_mp(shape):
    _disp_case(shape)


@pytest.mark.parametrize("shape", [("factor", 3, 24, True), ("factor", 2, 16, True)], ids=H.shape_id)
def test_fit_disp_without_cox_reid_vs_mp(shape):
    _disp_case(shape, useCR=False)


@pytest.mark.parametrize("nw", ["1", "8"])
def test_fit_disp_rolled_waves_per_gene_vs_mp(monkeypatch, nw):
    monkeypatch.setenv("DSQ_WIDE_NW", nw)
    _disp_case(("paired", 31, 60, False))


def _beta_case(shape):
    c, post, step = H.beta_reference(shape)
    n, m, p = c["n"], c["m"], c["p"]
    alpha = np.exp(c["log_alpha"])
    fails, worst = [], {}
    for useQR in (True, False):
        # maxit = 0: the post-fit quantities at the caller's beta_mat
        o = native.fitBeta(c["y"], c["x"], c["nf"], alpha, c["contrast"], c["beta_drawn"], c["lam"], c["weights"],
                           c["useWeights"], 1e-8, 0, useQR, c["minmu"])
        assert (o["iter"] == 0).all() and (o["deviance"] == 0.0).all()
        assert (o["beta_mat"] == c["beta_drawn"]).all()
        for k in ("beta_var_mat", "hat_diagonals", "contrast_num", "contrast_denom"):
            got = np.asarray(o[k]).reshape(n, -1)
            for i in range(n):
                vals, Ms = post[i][k]
                for j in range(len(vals)):
                    r = _check(fails, "fitBeta(maxit=0, useQR=%s)$%s[%d]" % (useQR, k, j), i, m, got[i, j], vals[j], Ms[j],
                               H.BUDGETS[k])
                    worst[k] = max(worst.get(k, 0.0), r)
        # maxit = 1: one ridge-penalised weighted least-squares solve from the start values, and its deviance
        o = native.fitBeta(c["y"], c["x"], c["nf"], alpha, c["contrast"], c["beta_start"], c["lam"], c["weights"],
                           c["useWeights"], 1e-8, 1, useQR, c["minmu"])
        assert (o["iter"] == 1).all()
        for i in range(n):
            b1, Mb, dev = step[i]
            for k in range(p):
                r = _check(fails, "fitBeta(maxit=1, useQR=%s)$beta_mat[%d]" % (useQR, k), i, m, o["beta_mat"][i, k], b1[k], Mb,
                           H.BUDGETS["beta_step"])
                worst["beta_step"] = max(worst.get("beta_step", 0.0), r)
            if dev is None:                                   # beta_1 outside the box: out before the deviance
                assert o["deviance"][i] == 0.0, "gene %d: deviance %r after the |beta| > 30 exit" % (i, o["deviance"][i])
                continue
            r = _check(fails, "fitBeta(maxit=1, useQR=%s)$deviance" % useQR, i, m, o["deviance"][i], dev[0], dev[1],
                       H.BUDGETS["deviance"])
            worst["deviance"] = max(worst.get("deviance", 0.0), r)
    print("hp ratios %s: %s" % (H.shape_id(shape), {k: round(v, 4) for k, v in worst.items()}))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("shape", H.BETA_SHAPES, ids=H.shape_id)
def test_fit_beta_frozen_vs_mp(shape):
    _beta_case(shape)


@pytest.mark.parametrize("nw", ["1", "4", "8"])
def test_fit_beta_rolled_waves_per_gene_vs_mp(monkeypatch, nw):
    monkeypatch.setenv("DSQ_WIDE_NW", nw)
    _beta_case(("paired", 31, 60, False))


def _aux_host(shape, c):
    name = shape[0]
    if name == "nbinomLogLike":
        return native.nbinomLogLike(c["y"], c["mu"], np.exp(c["log_alpha"]), c["weights"], c["useWeights"])
    if name == "linearMu":
        return native.linearMu(c["y"], c["nf"], c["x"], c["mu_floor"])
    if name == "prefitMoments":
        return native.prefitMoments(c["y"], c["nf"], c["x"], c["weights"], c["useWeights"])
    return native.cooksDistance(c["y"], c["nf"], c["mu_fit"], c["H"], c["x"])


def _aux_dev(shape, c):
    """the _dev entry points on gene-major resident inputs (the handles of DeviceEngine)"""
    import torch
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine("cuda:0")
    name = shape[0]
    y, nf = E.counts(c["y"]), E.matrix(c["nf"])
    w = E.matrix(c["weights"]) if c["useWeights"] else None
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64).T), device="cuda:0")   # noqa: E731
    host = lambda t: t.cpu().numpy()                                                                       # noqa: E731
    if name == "nbinomLogLike":
        disp = torch.as_tensor(np.exp(c["log_alpha"]), device="cuda:0")
        return host(native.nbinomLogLike_dev(y, E.matrix(c["mu"]), disp, w, c["useWeights"]))
    q, a, r = dev(c["q"]), dev(c["a"]), dev(c["r"])
    if name == "linearMu":
        return host(native.linearMu_dev(y, nf, q, a, c["mu_floor"]).view())
    if name == "prefitMoments":
        o = native.prefitMoments_dev(y, nf, q, a, r, w, c["useWeights"])
        return {"baseMean": host(o["baseMean"]), "baseVar": host(o["baseVar"]), "roughDisp": host(o["roughDisp"]),
                "allZero": host(o["allZero"]) != 0, "beta_init": host(o["beta_init"]).T}
    o = native.cooksDistance_dev(y, nf, E.matrix(c["mu_fit"]), E.matrix(c["H"]), native.cell_index(c["x"]), c["p"])
    return {"cooks": host(o["cooks"].view()), "maxCooks": host(o["maxCooks"]), "robustDisp": host(o["robustDisp"])}


@pytest.mark.parametrize("abi", ["host", "dev"])
@pytest.mark.parametrize("shape", H.AUX_SHAPES, ids=H.aux_id)
def test_aux_kernels_vs_mp(shape, abi):
    """dsq_nbinom_loglike, dsq_linear_mu, dsq_prefit_moments and dsq_cooks_distance, host and _dev ABI.  Q, X R^-1 and R
    are inputs of these kernels: the host ABI takes them from the library's own host QR (numpy, as the statement's),
    the _dev ABI is handed the statement's."""
    c, ref = H.aux_reference(shape)
    got = (_aux_host if abi == "host" else _aux_dev)(shape, c)
    fails, worst = [], {}
    for fam, i, v, rv, M in H.aux_items(shape, c, ref, got):
        worst[fam] = max(worst.get(fam, 0.0), _check(fails, "%s (%s ABI)" % (fam, abi), i, c["m"], v, rv, M, H.BUDGETS[fam]))
    print("hp ratios %s %s: %s" % (H.aux_id(shape), abi, {k: float("%.3g" % v) for k, v in worst.items()}))
    assert not fails, "\n".join(fails[:20])
