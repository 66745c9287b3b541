"""CPU: adaptive shrinkage.  The host engine's statement (deseq2_amd/ash_host.py) against the numpy
specification (tests/ash_spec.py) to the bit; the specification against 50-digit arithmetic (L, every posterior quantity at a
fixed pi, the two threshold tails, each within the bound DESIGN.md section 23 derives from its conditioning), against the
optimality certificate formed at 50 digits, and against scipy's SLSQP on the simplex; the edges; and core.lfcShrinkAshr along
R/lfcShrink.R:156-209, 442-518 on HostEngine(oracle)."""
import ctypes as C
from collections import OrderedDict

import mpmath as mp
import numpy as np
import pytest

from deseq2_amd import ash_host as H
from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import ash_cases as AC
from tests import ash_spec as S
from tests.helpers import assert_same

U = 2.0 ** -53
SEEDED = ((300, 6), (2000, 12))          # (the shapes of the issue that a 50-digit certificate covers in seconds)
_FITS = {}


def _fit(oracle, key, b, s, threshold=None):
    if key not in _FITS:
        _FITS[key] = S.fit(oracle, b, s, threshold)
    return _FITS[key]


# ---- the host engine is the specification
@pytest.mark.parametrize("name", list(AC.gpu_cases()))
def test_host_engine_equals_the_specification(oracle, name):
    c = AC.gpu_cases()[name]
    want = _fit(oracle, name, c["b"], c["s"], c["threshold"])
    got = HostEngine(oracle).ash_fit(c["b"], c["s"], threshold=c["threshold"])
    for k in S.KEYS:
        assert_same(got[k], want[k], "%s: %s" % (name, k))
    assert (want["flag"] == 0).all()


def test_constants_and_abi():
    from deseq2_amd import _lib as L
    assert L.DSQ_ASH_MAX_K == S.MAX_K == H.MAX_K and H.SLICE_ROWS == S.SLICE == AC.SLICE and H.TRIALS == S.TRIALS
    assert L.lib().dsq_ash_slice_rows() == S.SLICE
    n, cols = 1000, 3
    slices = -(-n // S.SLICE)
    assert L.lib().dsq_ash_workspace_bytes(n, cols) == 8 * cols * (2152 + 32 + 4 + 65 * n + slices * (2152 + 32 + 1)) + 64
    assert L.lib().dsq_ash_workspace_bytes(0, 1) == 0
    # every argument check is made before a device is asked for
    z = np.zeros(64)
    p = z.ctypes.data
    out = dict(PosteriorMean=p, PosteriorSD=p, NegativeProb=p, PositiveProb=p, lfsr=p, le_T=p, gt_mT=p, pi=p, sd=p, K=p, iter=p, flag=p,
               loglik=p)
    ok = dict(n=4, C=1, ld=4, betahat=p, sebetahat=p, has_threshold=0, threshold=0.0, maxit=100)
    for bad in (dict(n=0), dict(C=0), dict(ld=3), dict(betahat=None), dict(has_threshold=1, threshold=-1.0),
                dict(has_threshold=1, threshold=float("nan")), dict(maxit=-1)):
        a, o = L.DsqAshArgs(**dict(ok, **bad)), L.DsqAshOut(**out)
        assert L.lib().dsq_ash(C.byref(a), C.byref(o)) == L.DSQ_ERR_ARG, bad
        assert L.lib().dsq_ash_dev(C.byref(a), C.byref(o), p, 1 << 30, None) == L.DSQ_ERR_ARG, bad
    a, o = L.DsqAshArgs(**ok), L.DsqAshOut(**dict(out, lfsr=None))
    assert L.lib().dsq_ash(C.byref(a), C.byref(o)) == L.DSQ_ERR_ARG


# ---- the specification against 50 digits
SIGMA = np.array([1e-4, 1e-2, 0.1, 1.0, 10.0, 1e3])
PI = np.array([0.3, 0.05, 0.25, 0.2, 0.15, 0.05])
ROWS_BS = [(0.1, 1.0), (5.0, 0.5), (-19.0, 0.5), (3e-3, 1e-3), (-2.5, 40.0), (38.0, 1.0), (1e-6, 1e-5), (-700.0, 20.0)]


def test_specification_against_50_digits(oracle):
    """sigma_k from 1e-4 s to 1e6 s, |b| / s up to 38, tails down to 1e-300.  The bounds are those of DESIGN.md section 23:
    l is a sum of a logarithm (1 ulp) and a quotient, so its absolute error is at most 4 U (1 + |l|); exp turns the absolute
    error of l - lnorm into a relative one: eL = 8 U (1 + |l| + |lnorm|) + 2 U.  At a fixed pi every sum has terms of one sign:
    e = 2 max_k eL + (K + 8) U relative on u, w, PosteriorMean (|m_k| <= |b|); (m - PM)^2 moves by at most 4 e b^2, so
    |var - var*| <= e (var* + 4 b^2); a normal tail at z carries 16 U of Cody's fit and 4 z^2 U from exp(-z^2 / 2)."""
    mp.mp.dps = 50
    b, s = np.array([r[0] for r in ROWS_BS]), np.array([r[1] for r in ROWS_BS])
    L, lnorm, keep = S.block(oracle, b, s, SIGMA)
    T = 0.75
    for i, (bi, si) in enumerate(ROWS_BS):
        B, Sd = mp.mpf(bi), mp.mpf(si)
        l = [-mp.log(2 * mp.pi * (Sd * Sd + mp.mpf(g) ** 2)) / 2 - B * B / (2 * (Sd * Sd + mp.mpf(g) ** 2)) for g in SIGMA]
        top = max(l)
        eL = 0.0
        for k in range(SIGMA.size):
            want = mp.exp(l[k] - top)
            ek = 8 * U * (1 + float(abs(l[k])) + float(abs(top))) + 2 * U
            eL = max(eL, ek)
            assert abs(mp.mpf(L[i, k]) - want) <= ek * want + mp.mpf("1e-300"), (i, k)
        assert abs(mp.mpf(lnorm[i]) - top) <= 4 * U * (1 + float(abs(top)))
        # the posterior at PI, from the 50-digit L
        Lx = [mp.exp(v - top) for v in l]
        u = sum(mp.mpf(p) * v for p, v in zip(PI, Lx))
        w = [mp.mpf(p) * v / u for p, v in zip(PI, Lx)]
        m = [B * mp.mpf(g) ** 2 / (mp.mpf(g) ** 2 + Sd * Sd) for g in SIGMA]
        v = [mp.mpf(g) ** 2 * Sd * Sd / (mp.mpf(g) ** 2 + Sd * Sd) for g in SIGMA]
        pm = sum(a * c for a, c in zip(w, m))
        var = sum(a * (c + (d - pm) ** 2) for a, c, d in zip(w, v, m))
        e = 2 * eL + (SIGMA.size + 8) * U
        tail = lambda z: (e + (16 + 4 * float(z) ** 2) * U)
        z0 = [-d / mp.sqrt(c) for d, c in zip(m, v)]
        zl = [(T - d) / mp.sqrt(c) for d, c in zip(m, v)]
        zg = [(-T - d) / mp.sqrt(c) for d, c in zip(m, v)]
        want = {"PosteriorMean": (pm, e * abs(B)), "PosteriorSD": (mp.sqrt(var), e * (var + 4 * B * B) / (2 * mp.sqrt(var)) + 2 * U * mp.sqrt(var)),
                "NegativeProb": (sum(a * mp.ncdf(z) for a, z in zip(w, z0)), sum(a * mp.ncdf(z) * tail(z) for a, z in zip(w, z0))),
                "PositiveProb": (sum(a * mp.ncdf(-z) for a, z in zip(w, z0)), sum(a * mp.ncdf(-z) * tail(z) for a, z in zip(w, z0))),
                "le_T": (sum(a * mp.ncdf(z) for a, z in zip(w, zl)), sum(a * mp.ncdf(z) * tail(z) for a, z in zip(w, zl))),
                "gt_mT": (sum(a * mp.ncdf(-z) for a, z in zip(w, zg)), sum(a * mp.ncdf(-z) * tail(z) for a, z in zip(w, zg)))}
        got, _ = H.posterior(oracle.unary, b[i:i + 1], s[i:i + 1], L[i:i + 1], lnorm[i:i + 1], keep[i:i + 1], SIGMA, PI, T)
        for k, (val, bound) in want.items():
            err = abs(mp.mpf(got[k][0]) - val)
            print("row %d %-14s %.3e  err %.2e  bound %.2e" % (i, k, float(val), float(err), float(bound)))
            assert err <= bound + mp.mpf("1e-300"), (i, k)
    # the small tail is kept: R's 1 - cdf would return 0 here
    got, _ = H.posterior(oracle.unary, np.array([-30.0]), np.array([0.5]), *S.block(oracle, np.array([-30.0]), np.array([0.5]), SIGMA),
                         SIGMA, PI, 15.0)
    assert 0.0 < got["gt_mT"][0] < 1e-100 and 1.0 - (1.0 - got["gt_mT"][0]) == 0.0


def _certificate(b, s, fit):
    """max_k D_k - 1 at 50 digits, D_k = (1/n) sum_i L_ik / u_i, and the rounding bound of the device's own g"""
    mp.mp.dps = 50
    K = int(fit["K"][0])
    pi, sigma = fit["pi"][0, :K], fit["sd"][0, :K]
    keep = S.kept(b, s)
    D = [mp.mpf(0)] * K
    lmax = 0.0
    for bi, si in zip(b[keep], s[keep]):
        l = [-mp.log(2 * mp.pi * (mp.mpf(si) ** 2 + mp.mpf(g) ** 2)) / 2 - mp.mpf(bi) ** 2 / (2 * (mp.mpf(si) ** 2 + mp.mpf(g) ** 2))
             for g in sigma]
        top = max(l)
        lmax = max(lmax, float(abs(top)))
        Lr = [mp.exp(v - top) for v in l]
        u = sum(mp.mpf(p) * v for p, v in zip(pi, Lr))
        D = [d + v / u for d, v in zip(D, Lr)]
    n = int(keep.sum())
    gap = max(D) / n - 1
    # g_k = 1 - (sum_i z_ik) / n in floating point: z = L / u carries 2 eL + (K + 2) U (test above), the sum of n positive terms
    # in groups of 16, 8 and n / 128 adds (16 + 8 + n / 128) U, the quotient and the difference 2 U; times D_k <= max D
    eL = 8 * U * (1 + 2 * (lmax + 40.0)) + 2 * U
    bound = float(max(D) / n) * (2 * eL + (K + 2) * U + (24 + n / 128.0 + 2) * U)
    return float(gap), bound, n


@pytest.mark.parametrize("shape", SEEDED + ("K64", "K7", "excluded"), ids=str)
def test_optimality_certificate(oracle, shape):
    """By concavity loglik* - loglik(pi) <= n (max_k D_k - 1): the returned pi is within n (1e-8 + rounding) of the optimum"""
    if isinstance(shape, tuple):
        b, s = AC.seeded(*shape)
        fit = _fit(oracle, shape, b, s)
    else:
        c = AC.gpu_cases()[shape]
        b, s = c["b"][:, 0], c["s"][:, 0]
        fit = _fit(oracle, shape, c["b"], c["s"], c["threshold"])
    K = int(fit["K"][0])
    pi = fit["pi"][0, :K]
    assert fit["flag"][0] == 0 and (pi >= 0).all() and abs(pi.sum() - 1.0) <= 4 * 2.0 ** -52
    assert 1 <= fit["iter"][0] <= 40                       # (a specification that needs hundreds of iterations has a bug)
    gap, bound, n = _certificate(b, s, fit)
    print("%s: n = %d, K = %d, %d iterations, %d weights above 0, max D - 1 = %.3e (rounding bound of g %.1e)"
          % (shape, n, K, fit["iter"][0], (pi > 0).sum(), gap, bound))
    assert gap <= 1e-8 + bound


# (measured on this specification at 300 x 6 and 2 000 x 12, profiles/ash.md: the larger of the two; scipy's own stopping
#  error dominates it)
SCIPY_MEASURED = {"PosteriorMean": 7.8e-8, "PosteriorSD": 2.8e-8, "lfsr": 5.7e-9}


@pytest.mark.parametrize("shape", SEEDED, ids=str)
def test_specification_against_scipy(oracle, shape):
    """SLSQP on the simplex from the same start never finds a higher likelihood (by more than n 1e-8); its posterior
    quantities differ by its own stopping error, asserted at 4 x the measured figure"""
    from scipy.optimize import minimize
    b, s = AC.seeded(*shape)
    fit = _fit(oracle, shape, b, s)
    K = int(fit["K"][0])
    L, lnorm, keep = S.block(oracle, b, s, fit["sd"][0, :K])
    n = int(keep.sum())
    f = lambda x: -np.log(np.maximum(L @ x, 1e-300)).sum() / n
    df = lambda x: -(L / np.maximum(L @ x, 1e-300)[:, None]).sum(0) / n
    r = minimize(f, np.full(K, 1.0 / K), jac=df, method="SLSQP", bounds=[(0.0, 1.0)] * K,
                 constraints=[{"type": "eq", "fun": lambda x: x.sum() - 1.0, "jac": lambda x: np.ones(K)}],
                 options={"maxiter": 1000, "ftol": 1e-14})
    x = np.maximum(r.x, 0.0)
    x = x / x.sum()
    ours = np.log(L @ fit["pi"][0, :K]).sum() + lnorm.sum()
    theirs = np.log(L @ x).sum() + lnorm.sum()
    assert abs(ours - fit["loglik"][0]) <= 1e-9 * abs(ours)
    assert ours >= theirs - n * 1e-8
    post, _ = H.posterior(oracle.unary, b, s, L, lnorm, keep, fit["sd"][0, :K], x)
    for k, lim in SCIPY_MEASURED.items():
        d = np.nanmax(np.abs(post[k] - fit[k][0]))
        print("%s: loglik ours - scipy = %.3e, max |%s - scipy's| = %.3e" % (shape, ours - theirs, k, d))
        assert d <= 4 * lim


# ---- edges
def test_edges(oracle):
    E = HostEngine(oracle)
    one = E.ash_fit(np.array([np.nan, 1.5, 0.3]), np.array([1.0, 0.5, np.nan]))          # one kept row
    assert np.isnan(one["PosteriorMean"][0, [0, 2]]).all() and np.isfinite(one["PosteriorMean"][0, 1]) and one["flag"][0] == 0
    with pytest.raises(ValueError, match="no row"):
        E.ash_fit(np.array([np.nan, 1.0]), np.array([1.0, -1.0]))
    with pytest.raises(ValueError, match="no row"):
        core.ash(np.array([np.nan, 1.0]), np.array([1.0, 0.0]), engine=E)
    b, s = AC.wide_column(70, 7, top=170.0)
    with pytest.raises(NotImplementedError, match="65"):
        E.ash_fit(b, s)
    assert E.ash_fit(*AC.wide_column(70, 7))["K"][0] == 64 and E.ash_fit(*AC.null_column(50, 1))["K"][0] == 7
    c = AC.gpu_cases()["C3"]
    w = _fit(oracle, "C3", c["b"], c["s"], None)
    assert len(set(w["K"])) > 1 and len(set(w["iter"])) == 3
    for j in range(3):                                     # a batch is its columns, one by one
        solo = S.fit(oracle, c["b"][:, j], c["s"][:, j])
        for k in S.KEYS:
            assert_same(solo[k][0], w[k][j], "column %d alone: %s" % (j, k))
    # ceil(2 log2 r) is exact at the powers of sqrt(2)
    assert [H.ceil_2log2(r) for r in (1.0, 2.0, 8.0, 2.0 ** 0.5, np.nextafter(2.0, 3.0), np.nextafter(2.0, 0.0), 0.5)] == [0, 2, 6, 2, 3, 2, -2]
    r = core.ash(np.array([0.1, 2.0, -3.0, np.nan]), np.array([1.0, 0.5, 0.7, 1.0]), lfcThreshold=1.0, engine=E)
    assert set(r) >= {"fitted_g", "result", "loglik"} and (r["fitted_g"]["mean"] == 0).all()
    assert np.isnan(r["result"]["PosteriorMean"][3]) and r["result"]["lfdr"][0] == 0.0 and abs(r["fitted_g"]["pi"].sum() - 1) < 1e-15
    assert_same(r["result"]["svalue"], core.svalue(r["result"]["lfsr"]), "svalue")


# ---- lfcShrinkAshr along R/lfcShrink.R
@pytest.fixture(scope="module")
def three(oracle):
    from tests.lfcshrink_cases import counts
    f = OrderedDict(condition=np.repeat([0, 1, 2], 4))
    x, _ = core.standard_model_matrix(f)
    k = counts(150, x, 5)
    k[[3, 77]] = 0
    dds = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f, minReplicatesForReplace=np.inf)
    return dds, k, x, f


def test_lfcShrinkAshr_follows_R(oracle, three, capsys):
    dds, k, x, f = three
    A = core.lfcShrinkAshr
    with pytest.raises(TypeError, match="DESeqDataSet"):
        A(None, coef=1)
    with pytest.raises(ValueError, match="res should be a DESeqResults object"):
        A(dds, res=3)
    with pytest.raises(RuntimeError, match="first run DESeq"):
        A(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), coef=1)
    with pytest.raises(ValueError, match="lfcThreshold >= 0"):
        A(dds, coef=1, lfcThreshold=-1)
    with pytest.raises(ValueError, match="coef %in% resultsNamesDDS"):
        A(dds, coef="nope")
    with pytest.raises(ValueError, match="coef <= length"):
        A(dds, coef=7)
    with pytest.raises(ValueError, match="one of coef or contrast required"):
        A(dds)
    with pytest.raises(NotImplementedError, match="mixcompdist"):
        A(dds, coef=1, mixcompdist="uniform")
    with pytest.raises(TypeError):
        A(dds, coef=1, nonsense=1)
    with pytest.raises(NotImplementedError, match="lfcShrinkAshr"):
        core.lfcShrink(dds, coef=1, type="ashr")
    bp = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f, betaPrior=True, minReplicatesForReplace=np.inf)
    with pytest.raises(ValueError, match="betaPrior=FALSE"):
        A(bp, coef=1)
    capsys.readouterr()
    # the default columns, the citation, the descriptions, priorInfo, NaN on the all-zero rows
    base = core.results(dds, name=1)
    res, fit = A(dds, coef=1, returnList=True)
    err = capsys.readouterr().err
    assert "using 'ashr' for LFC shrinkage" in err and "Stephens, M. (2016)" in err and "FSOS" not in err
    assert res.columns == ["baseMean", "log2FoldChange", "lfcSE", "pvalue", "padj"]
    want = S.fit(oracle, np.asarray(base["log2FoldChange"]), np.asarray(base["lfcSE"]))
    assert_same(np.asarray(res["log2FoldChange"]), want["PosteriorMean"][0], "PosteriorMean")
    assert_same(np.asarray(res["lfcSE"]), want["PosteriorSD"][0], "PosteriorSD")
    assert_same(np.asarray(res["pvalue"]), np.asarray(base["pvalue"]), "pvalue")
    assert_same(np.asarray(res["padj"]), np.asarray(base["padj"]), "padj")
    assert np.isnan(np.asarray(res["log2FoldChange"])[[3, 77]]).all() and np.isnan(np.asarray(res["lfcSE"])[[3, 77]]).all()
    d = res.metadata["description"]
    assert d["log2FoldChange"].startswith("log2 fold change (MMSE): ") and d["lfcSE"].startswith("posterior SD: ")
    assert res.metadata["lfcThreshold"] == 0 and res.priorInfo["type"] == "ashr"
    K = int(want["K"][0])
    assert_same(res.priorInfo["fitted_g"]["pi"], want["pi"][0, :K], "fitted_g$pi")
    assert_same(fit["fitted_g"]["sd"], want["sd"][0, :K], "fitted_g$sd")
    assert fit["loglik"] == want["loglik"][0] and set(fit["result"]) >= {"PosteriorMean", "PosteriorSD", "lfsr", "svalue", "lfdr"}
    # svalue = TRUE: res[, 1:3] and the s-values of lfsr
    sv = A(dds, coef=1, svalue=True, quiet=True)
    assert capsys.readouterr().err == ""
    assert sv.columns == ["baseMean", "log2FoldChange", "lfcSE", "svalue"] and sv.metadata["description"]["svalue"].startswith("s-value: ")
    assert_same(np.asarray(sv["svalue"]), S_svalue(want["lfsr"][0]), "svalue")
    # lfcThreshold > 0: the FSOS message, s-values of P(beta <= T) / P(beta > -T) by the sign of the posterior mean
    th = A(dds, coef=1, lfcThreshold=0.5)
    assert "computing FSOS 'false sign or small' s-values (T=0.5)" in capsys.readouterr().err
    wt = S.fit(oracle, np.asarray(base["log2FoldChange"]), np.asarray(base["lfcSE"]), 0.5)
    with np.errstate(invalid="ignore"):
        lf = np.where(wt["PosteriorMean"][0] > 0, wt["le_T"][0], wt["gt_mT"][0])
    assert th.columns == ["baseMean", "log2FoldChange", "lfcSE", "svalue"] and th.metadata["lfcThreshold"] == 0.5
    assert_same(np.asarray(th["svalue"]), S_svalue(lf), "FSOS svalue")
    # a res of a contrast is used as given (coef and contrast ignored); a list of contrasts equals one call each
    cons = [("condition", 2, 1), ("condition", 1, 0), [0.0, 1.0, 1.0]]
    rc = core.resultsContrasts(dds, [cons[0]])[0]
    given = A(dds, coef=1, res=rc, quiet=True)
    direct = A(dds, contrast=cons[0], quiet=True)
    many = A(dds, contrast=cons, quiet=True)
    assert isinstance(many, list) and len(many) == 3
    for col in direct.columns:
        assert_same(np.asarray(given[col]), np.asarray(direct[col]), "res given: " + col)
    for c, got in zip(cons, many):
        solo = A(dds, contrast=c, quiet=True)
        assert got.metadata["description"] == solo.metadata["description"]
        for col in solo.columns:
            assert_same(np.asarray(got[col]), np.asarray(solo[col]), "%s: %s" % (c, col))
        assert_same(got.priorInfo["fitted_g"]["pi"], solo.priorInfo["fitted_g"]["pi"], "fitted_g")
    assert many[0].metadata["description"]["lfcSE"] == "posterior SD: condition 2 vs 1"
    # standard errors that are all NA
    broken = core.results(dds, name=1)
    broken["lfcSE"] = np.full(dds.n, np.nan)
    with pytest.raises(ValueError, match="requires standard errors"):
        A(dds, res=broken, quiet=True)


def S_svalue(lfsr):
    """apeglm_svalue (R/lfcShrink.R:523-528)"""
    order = np.argsort(lfsr, kind="stable")
    cm = np.cumsum(lfsr[order]) / np.arange(1, lfsr.size + 1)
    rank = np.empty(lfsr.size, np.int64)
    rank[order] = np.arange(lfsr.size)
    return cm[rank]
