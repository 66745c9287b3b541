"""-m gpu: the memory contract of the per-call _dev entry points on poisoned memory (tests/poison.py).

Python always hands these entries zero padding (native.to_gene_major allocates with torch.zeros) and often zero-filled
outputs: a read past m of a zero count, weight or mu is silent in most of their sums, and an output element that a kernel
never writes reads back as 0.  Here, per call:

  * every device buffer comes from an arena with 64 KiB guards around it; gene-major inputs have ld = round8(m) + 8 and
    garbage in the padding columns m .. ld-1 (-7 in int32 counts, NaN in doubles);
  * the outputs (and dsq_beta_prior_var_dev's workspace, of exactly its _workspace_bytes) start with every byte 0xFF, and
    again with every byte 0x00 -- through the wrappers of deseq2_amd/native.py with the arena behind torch.empty / torch.zeros,
    or through the C ABI directly where the wrapper fixes ld;
  * the expected value is the oracle's, bit for bit (tests/test_gpu_edge.py::_both) -- for the beta prior variance the line-cited
    mirror core.estimateBetaPriorVar, for weights_prep and xim the host statements of deseq2_amd/engine.py;
  * then Arena.check(): guards intact, inputs bytewise as they were, output padding as prefilled.

Shapes: one per kernel variant, from the catalogue in the docstring of tests/test_gpu_hp.py, at n = 37 genes (not a multiple
of any genes-per-workgroup); size factors as a matrix and as a vector.  Inputs by the suite's generators (tests/wide_cases.py
on the designs of deseq2_amd/simulate.py, tests/hp_reference.py for the aux shapes).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from deseq2_amd import _lib as L
from deseq2_amd import native, simulate
from deseq2_amd.engine import HostEngine, _weights_ok_host
from tests import hp_reference as H
from tests import poison, wide_cases
from tests.helpers import assert_same
from tests.poison import FF, ZERO

pytestmark = pytest.mark.gpu

N = 37
STATES = (FF, ZERO)
NAN = float("nan")
DEV = "cuda:0"


def _design(kind, p, m):
    if kind == "factor":
        return simulate.design_factor(m, p)
    if kind == "cont":
        return wide_cases.factor_cont(m, p - 1)
    assert kind == "paired" and m == 2 * (p - 1)
    return wide_cases.paired(p - 1)


_CASES = {}


def _case(kind, p, m, weights=False, special=None):
    """counts, factors, weights and start values of one shape (computed once, never modified)"""
    key = (kind, p, m, weights, special)
    if key not in _CASES:
        x = _design(kind, p, m)
        d = wide_cases.case(N, x, weights=weights, zero_w=special == "zero_w", seed=1000 * p + m)
        if special == "zero_w":
            # (3, 24): whole samples at zero weight (zero_w) and, in every second gene, a level below the threshold: a
            # column of the Cox-Reid matrix is dropped
            d["weights"][1::2, x[:, 1] == 1.0] = 0.005
            d["weights"][:, 0] = 1.0
        d["cells"] = native.cell_index(x)
        d["contrast"] = np.r_[1.0, np.zeros(p - 2), -1.0] if p > 1 else np.ones(1)
        _CASES[key] = d
    return _CASES[key]


def _id(s):
    return "%s-p%d-m%d%s" % (s[0], s[1], s[2], "".join("-" + str(v) for v in s[3:] if v))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _host(t):
    return t.cpu().numpy()


def _arena(nbytes=96 << 20):
    return poison.Arena.on_device(nbytes, DEV)


def _inputs(arena, d, nf_vector=False, mu=None):
    """the resident inputs of a fit call, all from the arena and watched"""
    ins = dict(y=arena.gene_major(d["counts"].astype(np.int32), -7, "y"),
               x=arena.put(d["x"].T, "x"),
               nf=arena.put(d["nf"][0], "sf") if nf_vector else arena.gene_major(d["nf"], NAN, "nf"),
               w=arena.gene_major(d["weights"], NAN, "weights") if d["useWeights"] else None)
    if mu is not None:
        ins["mu"] = arena.gene_major(mu, NAN, "mu")
    return ins


def _out_padding(arena, state, **handles):
    for k, h in handles.items():
        if h is not None:
            assert h.ld == poison.padded_ld(h.m) and arena.owns(h.t), k
            arena.padding(h, k, poison.BYTE[state])


# ---- fitBeta -------------------------------------------------------------------------------------------------------------
BETA_SHAPES = [("factor", 2, 6, False), ("factor", 3, 37, True), ("cont", 4, 100, False), ("cont", 4, 1500, False),
               ("cont", 7, 250, False), ("cont", 10, 503, False), ("cont", 10, 600, False),
               ("cont", 12, 60, False), ("paired", 31, 60, False), ("factor", 64, 130, True)]


@pytest.mark.parametrize("nf_vector", [False, True], ids=["nf_matrix", "sf_vector"])
@pytest.mark.parametrize("shape", BETA_SHAPES, ids=_id)
def test_fit_beta_dev(oracle, monkeypatch, shape, nf_vector):
    d = _case(*shape)
    args = (d["counts"], d["x"], d["nf"], d["alpha_init"], d["contrast"], d["beta_init"], d["lam"], d["weights"],
            d["useWeights"], 1e-8, 100, True, 0.5)
    if "want_beta" not in d:               # (the reference of a shape: computed once, shared by its cases)
        d["want_beta"] = oracle.fitBeta(*args, want_mu=True, mu_floor=0.5)
    want = d["want_beta"]
    for state in STATES:
        arena = _arena()
        i = _inputs(arena, d, nf_vector)
        al, ct, b0, lm = (arena.put(v, k) for k, v in (("alpha_hat", d["alpha_init"]), ("contrast", d["contrast"]),
                                                        ("beta_mat", d["beta_init"].T), ("lambda", d["lam"])))
        with arena.standing_in(monkeypatch, poison.BYTE[state]):
            o = native.fitBeta_dev(i["y"], i["x"], i["nf"], al, ct, b0, lm, i["w"], d["useWeights"], 1e-8, 100, True, 0.5,
                                   want_hat=True, want_mu=True, mu_floor=0.5, nf_is_vector=nf_vector, cells=d["cells"])
        what = "fitBeta_dev %s, prefill %s: " % (_id(shape), state)
        assert arena.owns(o["_pack"])
        for k in ("beta_mat", "beta_var_mat"):
            assert_same(_host(o[k]).T, want[k], what + k)
        for k in ("iter", "deviance"):
            assert_same(_host(o[k]), want[k], what + k)
        for k in ("contrast_num", "contrast_denom"):
            assert_same(_host(o[k]).reshape(-1, 1), want[k], what + k)
        assert_same(_host(o["hat_diagonals"].view()), want["hat_diagonals"], what + "hat_diagonals")
        assert_same(_host(o["mu"].view()), want["mu"], what + "mu")
        _out_padding(arena, state, hat_diagonals=o["hat_diagonals"], mu=o["mu"])
        arena.check()


def test_fit_beta_dev_r_layout(oracle):
    """dsq_fit_beta_dev on DEVICE pointers in R's column-major layout (tests/test_gpu_edge.py::test_device_pointers_in_r_layout
    hands it zero-filled outputs): the same call on prefilled outputs from the arena"""
    d = _case("cont", 4, 100)
    n, m = d["counts"].shape
    p = d["x"].shape[1]
    want = oracle.fitBeta(d["counts"], d["x"], d["nf"], d["alpha_init"], d["contrast"], d["beta_init"], d["lam"], d["weights"], False,
                          1e-8, 100, True, 0.5, want_mu=True, mu_floor=0.5)
    for state in STATES:
        arena = _arena()
        y, x, nf, b0 = (arena.put(v.T, k) for k, v in (("y", d["counts"].astype(np.int32)), ("x", d["x"]), ("nf", d["nf"]),
                                                       ("beta_mat", d["beta_init"])))
        al, ct, lm = (arena.put(v, k) for k, v in (("alpha_hat", d["alpha_init"]), ("contrast", d["contrast"]), ("lambda", d["lam"])))
        out = {k: arena.empty(s, torch.float64, poison.BYTE[state], k) for k, s in
               (("beta_mat", (p, n)), ("beta_var_mat", (p, n)), ("iter", (n,)), ("hat", (m, n)), ("cn", (n,)), ("cd", (n,)),
                ("dev", (n,)), ("mu", (m, n)))}
        a = L.DsqFitBetaArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_p(y), y_type=L.DSQ_Y_INT32, x=_p(x), nf=_p(nf),
                             nf_is_vector=0, alpha_hat=_p(al), contrast=_p(ct), beta_mat=_p(b0), lambda_=_p(lm), weights=None,
                             useWeights=0, tol=1e-8, maxit=100, useQR=1, minmu=0.5, cell_of=d["cells"].ctypes.data_as(C.c_void_p),
                             ncell=int(d["cells"].max()) + 1)
        o = L.DsqFitBetaOut(beta_mat=_p(out["beta_mat"]), beta_var_mat=_p(out["beta_var_mat"]), iter=_p(out["iter"]),
                            hat_diagonals=_p(out["hat"]), contrast_num=_p(out["cn"]), contrast_denom=_p(out["cd"]),
                            deviance=_p(out["dev"]), mu=_p(out["mu"]), mu_floor=0.5)
        L.check(L.lib().dsq_fit_beta_dev(C.byref(a), C.byref(o), _stream()))
        what = "fitBeta_dev, R layout, prefill %s: " % state
        for k, kw in (("beta_mat", "beta_mat"), ("beta_var_mat", "beta_var_mat"), ("hat", "hat_diagonals"), ("mu", "mu")):
            assert_same(_host(out[k]).T, want[kw], what + kw)
        for k, kw in (("iter", "iter"), ("dev", "deviance")):
            assert_same(_host(out[k]), want[kw], what + kw)
        for k, kw in (("cn", "contrast_num"), ("cd", "contrast_denom")):
            assert_same(_host(out[k]).reshape(-1, 1), want[kw], what + kw)
        arena.check()


# ---- fitDisp / fitDispGrid -----------------------------------------------------------------------------------------------
DISP_SHAPES = [("factor", 2, 6, False), ("factor", 3, 65, False), ("factor", 10, 130, False), ("factor", 10, 256, False),
               ("factor", 10, 2561, False), ("factor", 10, 2000, False), ("factor", 3, 24, True, "zero_w"),
               ("cont", 5, 40, False), ("cont", 7, 257, False), ("cont", 10, 1025, False),
               ("cont", 12, 60, False), ("paired", 31, 60, False), ("factor", 48, 96, False), ("factor", 64, 130, True)]
DISP_KEYS = ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp", "last_d2lp", "iter", "iter_accept")


def _disp_inputs(oracle, d):
    if "mu_hat" not in d:
        ob = oracle.fitBeta(d["counts"], d["x"], d["nf"], d["alpha_init"], d["contrast"], d["beta_init"], d["lam"], d["weights"],
                            d["useWeights"], 1e-8, 100, True, 0.5, want_mu=True, mu_floor=0.5)
        d["mu_hat"] = np.where(np.isfinite(ob["mu"]), ob["mu"], 0.5)
    la = np.log(d["alpha_init"])
    w = np.maximum(d["weights"], 1e-6) if d["useWeights"] else d["weights"]
    return la, w


@pytest.mark.parametrize("shape", DISP_SHAPES, ids=_id)
def test_fit_disp_dev(oracle, monkeypatch, shape):
    d = _case(*shape)
    la, w = _disp_inputs(oracle, d)
    want = oracle.fitDisp(d["counts"], d["x"], d["mu_hat"], la, la - 0.1, 0.8, np.log(1e-9), 1.0, 1e-6, 100, True, w,
                          d["useWeights"], 1e-2, True)
    for state in STATES:
        arena = _arena()
        i = _inputs(arena, dict(d, weights=w), mu=d["mu_hat"])
        lad, pmd = arena.put(la, "log_alpha"), arena.put(la - 0.1, "prior_mean")
        with arena.standing_in(monkeypatch, poison.BYTE[state]):
            o = native.fitDisp_dev(i["y"], i["x"], i["mu"], lad, pmd, 0.8, np.log(1e-9), 1.0, 1e-6, 100, True, i["w"],
                                   d["useWeights"], 1e-2, True, want_d2lp=True, cells=d["cells"])
        assert arena.owns(o["_pack"])
        for k in DISP_KEYS:
            assert_same(_host(o[k]), want[k], "fitDisp_dev %s, prefill %s: %s" % (_id(shape), state, k))
        arena.check()


@pytest.mark.parametrize("shape", DISP_SHAPES, ids=_id)
def test_fit_disp_grid_dev(oracle, monkeypatch, shape):
    d = _case(*shape)
    la, w = _disp_inputs(oracle, d)
    m = d["counts"].shape[1]
    grid = np.linspace(np.log(1e-8), np.log(max(10, m)), 12)
    want = oracle.fitDispGrid(d["counts"], d["x"], d["mu_hat"], grid, la, 1.0, True, w, d["useWeights"], 1e-2, True)
    for state in STATES:
        arena = _arena()
        i = _inputs(arena, dict(d, weights=w), mu=d["mu_hat"])
        gd, pmd = arena.put(grid, "disp_grid"), arena.put(la, "prior_mean")
        with arena.standing_in(monkeypatch, poison.BYTE[state]):
            o = native.fitDispGrid_dev(i["y"], i["x"], i["mu"], gd, pmd, 1.0, True, i["w"], d["useWeights"], 1e-2, True,
                                       cells=d["cells"])
        assert arena.owns(o["log_alpha"])
        assert_same(_host(o["log_alpha"]), want["log_alpha"], "fitDispGrid_dev %s, prefill %s" % (_id(shape), state))
        arena.check()


# ---- the aux entries on the AUX_SHAPES of tests/hp_reference.py (its inputs, at its gene counts; the mp side is not used) -----
_AUX = {}


def _aux_case(shape):
    if shape not in _AUX:
        name, kind, p, m, w = shape
        c = H.make_case(kind, p, m, weights=w, big_every=2 if name == "cooksDistance" else 1)
        c["mu_floor"] = 0.5 if m == 24 else 0.0
        _AUX[shape] = c
    return _AUX[shape]


def _aux_inputs(arena, c, nf_vector):
    nf = np.broadcast_to(c["nf"][0], c["nf"].shape).copy() if nf_vector else c["nf"]     # a vector: the same factors in every row
    return nf, dict(y=arena.gene_major(c["y"], -7, "y"),
                    nf=arena.put(nf[0], "sf") if nf_vector else arena.gene_major(nf, NAN, "nf"),
                    w=arena.gene_major(c["weights"], NAN, "weights") if c["useWeights"] else None)


def _qr_dev(arena, oracle, x):
    return tuple(arena.put(np.ascontiguousarray(np.asarray(z).T), k) for k, z in zip("qar", oracle.design_qr(x)))


@pytest.mark.parametrize("nf_vector", [False, True], ids=["nf_matrix", "sf_vector"])
@pytest.mark.parametrize("shape", [s for s in H.AUX_SHAPES if s[0] != "nbinomLogLike"], ids=H.aux_id)
def test_aux_dev(oracle, monkeypatch, shape, nf_vector):
    """prefitMoments_dev, linearMu_dev and cooksDistance_dev; on the cooksDistance shapes also replaceOutliers_dev (on the
    oracle's Cook's distances) and the intercept fit"""
    name = shape[0]
    c = _aux_case(shape)
    m, p = c["m"], c["p"]
    for state in STATES:
        arena = _arena()
        nf, i = _aux_inputs(arena, c, nf_vector)
        what = "%s_dev %s, prefill %s: " % (name, H.aux_id(shape), state)
        if name == "prefitMoments":
            want = oracle.prefitMoments(c["y"], nf, c["x"], c["weights"], c["useWeights"])
            q, a, r = _qr_dev(arena, oracle, c["x"])
            with arena.standing_in(monkeypatch, poison.BYTE[state]):
                o = native.prefitMoments_dev(i["y"], i["nf"], q, a, r, i["w"], c["useWeights"], nf_is_vector=nf_vector)
            for k in ("baseMean", "baseVar", "roughDisp"):
                assert_same(_host(o[k]), want[k], what + k)
            assert_same(_host(o["allZero"]) != 0, want["allZero"], what + "allZero")
            assert_same(_host(o["beta_init"]).T, want["beta_init"], what + "beta_init")
        elif name == "linearMu":
            want = oracle.linearMu(c["y"], nf, c["x"], c["mu_floor"])
            q, a, _ = _qr_dev(arena, oracle, c["x"])
            with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):
                mu = native.linearMu_dev(i["y"], i["nf"], q, a, c["mu_floor"], nf_is_vector=nf_vector)
            assert_same(_host(mu.view()), want, what + "mu")
            _out_padding(arena, state, mu=mu)
        else:
            alpha = np.exp(c["log_alpha"])
            fit = oracle.fitBeta(c["y"], c["x"], nf, alpha, c["contrast"], c["beta_start"], c["lam"], c["weights"], False, 1e-8, 100,
                                 True, 0.5, want_mu=True, mu_floor=0.5)
            mu_h, H_h = np.where(np.isfinite(fit["mu"]), fit["mu"], 0.5), np.nan_to_num(fit["hat_diagonals"])
            want = oracle.cooksDistance(c["y"], nf, mu_h, H_h, c["x"])
            mu_d, H_d = arena.gene_major(mu_h, NAN, "mu"), arena.gene_major(H_h, NAN, "H")
            with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):
                o = native.cooksDistance_dev(i["y"], i["nf"], mu_d, H_d, native.cell_index(c["x"]), p, nf_is_vector=nf_vector)
            assert_same(_host(o["cooks"].view()), want["cooks"], what + "cooks")
            for k in ("maxCooks", "robustDisp"):
                assert_same(_host(o[k]), want[k], what + k)
            _out_padding(arena, state, cooks=o["cooks"])
            # replaceOutliers on those distances: a cutoff that replaces in some rows and not in others
            ck = want["cooks"]
            cutoff = float(np.nanquantile(ck, 0.9))
            replaceable = np.arange(m) % 3 != 0
            wr = oracle.replaceOutliers(c["y"], nf, ck, cutoff, replaceable)
            assert wr["replace"].sum() > 0
            ck_d = arena.gene_major(ck, NAN, "cooks")
            with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):
                ro = native.replaceOutliers_dev(i["y"], i["nf"], ck_d, cutoff, replaceable, nf_is_vector=nf_vector)
            assert_same(_host(ro["counts"].view()), wr["counts"], what + "replaceOutliers counts")
            assert_same(_host(ro["replace"]) != 0, wr["replace"], what + "replaceOutliers replace")
            _out_padding(arena, state, newCounts=ro["counts"])
            # the intercept fit (design ~ 1) on the same rows, with and without the hat diagonals
            for want_hat in (True, False):
                wi = oracle.interceptFit(c["y"], nf, alpha, None, False, 0.5, want_hat)
                al = arena.put(alpha, "alpha")
                with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):
                    io = native.interceptFit_dev(i["y"], i["nf"], al, None, False, 0.5, want_hat, nf_is_vector=nf_vector)
                pk = _host(io["_pack"])
                assert_same(pk[0], wi["beta"], what + "interceptFit beta")
                assert_same(pk[1], wi["betaSE"], what + "interceptFit betaSE")
                assert_same(_host(io["mu"].view()), wi["mu"], what + "interceptFit mu")
                if want_hat:
                    assert_same(_host(io["hat_diagonals"].view()), wi["hat_diagonals"], what + "interceptFit hat")
                _out_padding(arena, state, mu=io["mu"], hat=io["hat_diagonals"])
        arena.check()


@pytest.mark.parametrize("shape", [s for s in H.AUX_SHAPES if s[0] == "nbinomLogLike"] + [("nbinomLogLike", "factor", 3, 37, True)],
                         ids=H.aux_id)
def test_nbinom_loglike_and_weighted_intercept_dev(oracle, monkeypatch, shape):
    c = _aux_case(shape)
    disp = np.exp(c["log_alpha"])
    want = oracle.nbinomLogLike(c["y"], c["mu"], disp, c["weights"], c["useWeights"])
    wi = oracle.interceptFit(c["y"], c["nf"], disp, c["weights"], c["useWeights"], 0.0, True)
    for state in STATES:
        arena = _arena()
        _, i = _aux_inputs(arena, c, False)
        mu_d, dd = arena.gene_major(c["mu"], NAN, "mu"), arena.put(disp, "disp")
        with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):
            ll = native.nbinomLogLike_dev(i["y"], mu_d, dd, i["w"], c["useWeights"])
            io = native.interceptFit_dev(i["y"], i["nf"], dd, i["w"], c["useWeights"], 0.0, True)
        what = "%s, prefill %s: " % (H.aux_id(shape), state)
        assert_same(_host(ll), want, what + "nbinomLogLike_dev")
        pk = _host(io["_pack"])
        assert_same(pk[0], wi["beta"], what + "interceptFit beta")
        assert_same(pk[1], wi["betaSE"], what + "interceptFit betaSE")
        assert_same(_host(io["mu"].view()), wi["mu"], what + "interceptFit mu")
        assert_same(_host(io["hat_diagonals"].view()), wi["hat_diagonals"], what + "interceptFit hat")
        _out_padding(arena, state, mu=io["mu"], hat=io["hat_diagonals"])
        arena.check()


def test_parametric_dispersion_fit_dev(oracle, monkeypatch):
    rng = np.random.default_rng(7)
    means = np.exp(rng.uniform(np.log(2), np.log(5000), 337))
    disps = (0.05 + 3.0 / means) * np.exp(rng.normal(0, 0.4, 337))
    want = oracle.parametricDispersionFit(means, disps)
    for state in STATES:
        arena = _arena()
        md, dd = arena.put(means, "means"), arena.put(disps, "disps")
        with arena.standing_in(monkeypatch, poison.BYTE[state], zeros=True):        # (coefs[2] + status word: 24 bytes)
            got = native.parametricDispersionFit_dev(md, dd)
        assert_same(got, want, "parametricDispersionFit_dev, prefill %s" % state)
        arena.check()


# ---- weights_prep, xim and the layout converters: the C ABI directly, at ld = round8(m) + 8 --------------------------------
@pytest.mark.parametrize("p,m", [(5, 37), (12, 60)], ids=lambda v: str(v))
def test_weights_prep_dev(p, m):
    rng = np.random.default_rng(p * 1000 + m)
    x = simulate.design_factor(m, p)
    w = rng.uniform(0.02, 1.0, (N, m))
    w[rng.uniform(size=w.shape) < 0.05] = 0.0                # exact zeros
    w[3, x[:, 2] == 1] = 0.0                                 # a level without a sample: weightsFail
    w[10, x[:, p - 1] == 1] = 0.005                          # ... only below the threshold
    w[20] = 0.0                                              # apply(w, 1, max) = 0: NaN weights
    with np.errstate(all="ignore"):
        want = w / w.max(axis=1, keepdims=True)
        ok = _weights_ok_host(np.nan_to_num(want, nan=0.0), x, 1e-2, True)
    keep = ~np.isnan(want).any(axis=1)
    for state in STATES:
        arena = _arena()
        byte = poison.BYTE[state]
        wd, xd = arena.gene_major(w, NAN, "weights"), arena.put(x.T, "x")
        ld = wd.ld
        wn = native.GeneMajor(arena.empty((N, ld), torch.float64, byte, "w_norm"), m)
        wf = native.GeneMajor(arena.empty((N, ld), torch.float64, byte, "w_floor"), m)
        fz = arena.empty(N, torch.int32, byte, "weightsFail")
        neg = arena.empty(1, torch.int32, 0, "any_negative")             # (|= 1: the caller zeroes it first, the header says)
        _out_padding(arena, state, w_norm=wn, w_floor=wf)
        L.check(L.lib().dsq_weights_prep_dev(_p(wd.t), _p(xd), N, m, p, ld, 1e-2, _p(wn.t), _p(wf.t), _p(fz), _p(neg), _stream()))
        what = "weights_prep p=%d m=%d, prefill %s: " % (p, m, state)
        assert_same(_host(wn.view()), want, what + "w_norm")
        assert_same(_host(wf.view()), np.where(np.isnan(want), want, np.maximum(want, 1e-6)), what + "w_floor")
        fail = _host(fz)
        assert set(np.unique(fail)) <= {0, 1}, what + "weightsFail holds %s" % np.unique(fail)
        assert fail[3] and fail[20] and (fail[keep].astype(bool) == ~ok[keep]).all(), what + "weightsFail"
        assert int(_host(neg)[0]) == 0
        arena.check()


@pytest.mark.parametrize("m", [6, 64, 130], ids=lambda v: "m%d" % v)
def test_xim_dev(m):
    nf = np.exp(np.random.default_rng(m).normal(0, 0.3, (N, m)))
    want = HostEngine().xim(nf)
    for state in STATES:
        arena = _arena()
        nfd = arena.gene_major(nf, NAN, "nf")
        scratch = arena.empty(m, torch.float64, poison.BYTE[state], "scratch_m")      # exactly m doubles: an overrun is in a guard
        out = arena.empty(1, torch.float64, poison.BYTE[state], "out")
        L.check(L.lib().dsq_xim_dev(_p(nfd.t), N, m, nfd.ld, _p(scratch), _p(out), _stream()))
        assert float(_host(out)[0]) == want, "xim m=%d, prefill %s" % (m, state)
        arena.check()


@pytest.mark.parametrize("m", [6, 37, 64, 130], ids=lambda v: "m%d" % v)
def test_layout_converters(m):
    rng = np.random.default_rng(m)
    a = rng.normal(size=(N, m))
    k = rng.integers(0, 2 ** 31 - 1, size=(N, m)).astype(np.int32)
    ld = poison.padded_ld(m)
    lib = L.lib()
    for state in STATES:
        arena = _arena()
        byte = poison.BYTE[state]
        a_r, k_r, kf_r = arena.put(a.T, "f64, R layout"), arena.put(k.T, "i32, R layout"), arena.put(k.T.astype(np.float64), "counts f64")
        a_g = native.GeneMajor(arena.empty((N, ld), torch.float64, byte, "gm f64"), m)
        k_g = native.GeneMajor(arena.empty((N, ld), torch.int32, byte, "gm i32"), m)
        kf_g = native.GeneMajor(arena.empty((N, ld), torch.int32, byte, "gm i32 from f64"), m)
        bad = arena.empty(2, torch.int32, 0, "bad")
        back = arena.empty((m, N), torch.float64, byte, "back to R layout")
        _out_padding(arena, state, gm_f64=a_g, gm_i32=k_g, gm_counts=kf_g)
        L.check(lib.dsq_to_gene_major_f64(_p(a_r), _p(a_g.t), N, m, ld, _stream()))
        L.check(lib.dsq_to_gene_major_i32(_p(k_r), _p(k_g.t), N, m, ld, _stream()))
        L.check(lib.dsq_counts_f64_to_gene_major_i32(_p(kf_r), _p(kf_g.t), N, m, ld, _p(bad), _stream()))
        # from gene-major: the input's padding holds NaN
        src = arena.gene_major(a, NAN, "gm input")
        L.check(lib.dsq_from_gene_major_f64(_p(src.t), _p(back), N, m, src.ld, _stream()))
        what = "m=%d, prefill %s: " % (m, state)
        assert_same(_host(a_g.view()), a, what + "to_gene_major_f64")
        assert_same(_host(k_g.view()), k, what + "to_gene_major_i32")
        assert_same(_host(kf_g.view()), k, what + "counts_f64_to_gene_major_i32")
        assert int(_host(bad)[0]) == 0
        assert_same(_host(back).T, a, what + "from_gene_major_f64")
        arena.check()


# ---- the beta prior variance with a workspace of exactly its _workspace_bytes ----------------------------------------------
@pytest.mark.parametrize("expanded", [False, True], ids=["standard", "expanded"])
def test_beta_prior_var_dev(monkeypatch, expanded):
    rng = np.random.default_rng(5)
    n = 337
    factors = {"batch": np.arange(24) % 3, "condition": (np.arange(24) >= 12).astype(int)}
    cf = native.coef_factor_codes(factors)
    p = cf.size
    mle = rng.normal(0, 1.5, (n, p))
    mle[::17] = np.nan
    base, fit = np.exp(rng.normal(4, 2, n)), np.exp(rng.normal(-2, 1, n))
    az = (np.arange(n) % 17 == 0).astype(np.int32)
    kw = {}
    if expanded:
        kw = dict(prior_coef_factor=native.coef_factor_codes(factors, expanded=True))   # (no -1 column: no prior_coef_src)
    # the expected value: the line-cited mirror of R/core.R:1601-1689 (core.estimateBetaPriorVar), not the library's host entry
    from deseq2_amd import core
    _, names = core.standard_model_matrix(factors)
    live = az == 0
    view = type("V", (), {"mcols": {"baseMean": base[live], "dispFit": fit[live]}})()
    with np.errstate(all="ignore"):
        want, _ = core.estimateBetaPriorVar(view, mle[live], names, modelMatrixType="expanded" if expanded else "standard",
                                            factors=factors)
    want = np.asarray(want)
    args = L.DsqBetaPriorArgs(n=n, p=p, coef_factor=cf.ctypes.data_as(C.c_void_p), expanded=int(expanded), p_prior=int(want.size),
                              prior_coef_factor=kw["prior_coef_factor"].ctypes.data_as(C.c_void_p) if expanded else None,
                              upperQuantile=0.05)
    need = int(L.lib().dsq_beta_prior_var_workspace_bytes(n, L.lib().dsq_beta_prior_var_columns(C.byref(args))))
    for state in STATES:
        arena = _arena()
        md, bd, fd, ad = arena.put(mle.T, "mle_beta"), arena.put(base, "baseMean"), arena.put(fit, "dispFit"), arena.put(az, "allZero")
        with arena.standing_in(monkeypatch, poison.BYTE[state]):          # (the wrapper asks torch.empty for exactly the bytes)
            got = native.estimateBetaPriorVar_dev(md, bd, fd, ad, cf, **kw)
        # the workspace the wrapper asked torch.empty for: exactly dsq_beta_prior_var_workspace_bytes, a guard right behind it
        assert arena.blocks[-1][2] == "torch.empty" and arena.blocks[-1][1] == need > 0
        assert_same(got, want, "beta_prior_var_dev expanded=%s, prefill %s" % (expanded, state))
        arena.check()
