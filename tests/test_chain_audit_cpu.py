"""No GPU: tests/hp_reference.py: chain_audit -- every derived column of one DESeq() call against its 50-digit statement -- holds
for the reference chain (core.DESeq over HostEngine(oracle)) within hp_reference.BUDGETS on every case of tests/chain_cases.py
(the ratios are printed, run with -s), the inputs satisfy the preconditions that make the audit bite, and a wrong column of
each kind -- a one-sided p-value, a natural-log beta over a log2 betaSE, a MAD without its 1.4826, ... -- fails it."""
import numpy as np
import pytest

from deseq2_amd import core
from deseq2_amd.engine import HostEngine
from tests import chain_cases as CC
from tests import hp_reference as H

CASES = CC.cases()
_RUNS = {}


def _run(oracle, name):
    if name not in _RUNS:
        c = CASES[name]
        dds = core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], normalizationFactors=c.get("normalizationFactors"),
                                weights=c.get("weights"), engine=HostEngine(oracle))
        core.DESeq(dds, **CC.chain_kwargs(c))
        _RUNS[name] = CC.result_of(dds)
    return _RUNS[name]


def _fits(oracle):
    return {"exact": oracle.parametricDispersionFit, "restated": (core.parametricDispersionFit, 1e-9)}


def _refitted(res):
    return bool(np.nansum(res["replace"]) > 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_audit_holds_for_the_oracle_chain(oracle, name):
    c, res = CASES[name], _run(oracle, name)
    R = H.chain_audit(c, res, scalars=not _refitted(res), trend_fits=_fits(oracle))
    print("%s %s ties %s" % (name, R.summary(), R.ties))
    assert not R.failures, R.failures[:10]
    for k, v in R.ratios.items():
        K = H.BUDGETS[H._BUDGET_OF.get(k, k)]
        assert v <= K, "%s %s: ratio %.3g over K = %g (row %s)" % (name, k, v, K, R.where[k])
    live = np.nan_to_num(res["allZero"], nan=1.0) == 0
    assert R.ties.get("dispOutlier", 0) <= 0.01 * live.sum()              # the tie cap of the dispOutlier rule
    lrt = c.get("test") == "LRT"
    for fam in ("baseMean", "dispMAP", "dispersion", "mu", "betaSE", "cooks", "maxCooks", "dispPriorVar") + (
            ("LRTStatistic", "LRTPvalue") if lrt else ("stat", "pvalue")) + (() if _refitted(res) else ("varLogDispEsts", "trend")):
        assert R.counts.get(fam, 0) > 0, fam
    assert _refitted(res) == (name in [a for a, _ in CC.REFIT_PAIRS]), "a refitted case needs its twin in REFIT_PAIRS"


@pytest.mark.parametrize("refit,plain", CC.REFIT_PAIRS)
def test_a_refit_reuses_the_all_gene_scalars(oracle, refit, plain):
    """refitWithoutOutliers takes the trend, varLogDispEsts, dispPriorVar and the beta prior variance as the first pass left them
    (R/core.R:2512-2527): audited on the run without a refit, bit-identical on the run with it"""
    a, b = _run(oracle, refit), _run(oracle, plain)
    assert _refitted(a) and not _refitted(b)
    fa, fb = a["dispersionFunction"], b["dispersionFunction"]
    assert np.array_equal(np.asarray(fa["coefficients"]), np.asarray(fb["coefficients"]))
    assert fa["varLogDispEsts"] == fb["varLogDispEsts"] and fa["dispPriorVar"] == fb["dispPriorVar"]
    if "betaPriorVar" in a:
        assert np.array_equal(a["betaPriorVar"], b["betaPriorVar"])


def test_the_inputs_make_every_mutant_observable(oracle):
    for name in ("bc_outliers", "bc_4200"):
        res = _run(oracle, name)
        st = np.abs(res["stat"][np.isfinite(res["stat"])])
        m = CASES[name]["x"].shape[0]
        assert np.nansum(res["dispOutlier"]) >= 1 and np.nansum(res["replace"]) >= 1
        assert ((res["dispMAP"] == H.MIN_DISP) | (res["dispMAP"] == max(10, m))).sum() >= 1
        assert (st > 5.66).any() and (st < 0.674).any() and ((st > 0.674) & (st < 5.66)).any()       # the three ranges of pnorm
    assert _run(oracle, "factor4_mean")["dispersionFunction"]["dispPriorVar"] > 0.25                  # off its floor
    assert _run(oracle, "bc_no_refit")["dispersionFunction"]["dispPriorVar"] == 0.25                  # on it


def _mutants(c, res):
    """name -> (inputs, wrong result, scalars)"""
    from scipy import special
    LOG2E = np.log2(np.e)
    fn = res["dispersionFunction"]
    m, p = c["x"].shape
    live = np.nan_to_num(res["allZero"], nan=1.0) == 0

    def mut(**kw):
        r = dict(res)
        r.update(kw)
        return r
    out = {}
    out["one_sided_pvalue"] = mut(pvalue=res["pvalue"] / 2)
    out["natural_log_beta_over_log2_se"] = mut(stat=res["beta"] / LOG2E / res["betaSE"])
    dge, dfit = res["dispGeneEst"], res["dispFit"]
    use = live & (np.nan_to_num(dge) >= 100 * H.MIN_DISP)
    r_ = np.log(dge[use]) - np.log(dfit[use])
    mad0 = np.median(np.abs(r_ - np.median(r_)))
    out["mad_without_1.4826"] = mut(dispersionFunction=dict(fn, varLogDispEsts=float(mad0 ** 2)))
    v = fn["varLogDispEsts"]
    out["prior_var_without_floor"] = mut(dispersionFunction=dict(fn, dispPriorVar=float(v - special.polygamma(1, (m - p) / 2))))
    out["prior_var_trigamma_m_minus_p"] = mut(dispersionFunction=dict(fn, dispPriorVar=float(max(v - special.polygamma(1, m - p), 0.25))))
    with np.errstate(invalid="ignore", divide="ignore"):
        sd1 = (np.log(dge) > np.log(dfit) + 1 * np.sqrt(v)) & live
    out["outlier_sd_1"] = mut(dispOutlier=np.where(live, sd1.astype(float), np.nan),
                              dispersion=np.where(sd1, dge, res["dispMAP"]))
    out["dispersion_map_on_outlier_rows"] = mut(dispersion=res["dispMAP"])
    if fn["fitType"] == "parametric":
        a, e = fn["coefficients"]
        with np.errstate(divide="ignore"):
            out["dispfit_coefficients_swapped"] = mut(dispFit=e + a / res["baseMean"])
    out["max_cooks_over_all_samples"] = mut(maxCooks=np.where(live, res["cooks"].max(axis=1), np.nan))
    if _refitted(res):
        rep = np.nan_to_num(res["replace"]) == 1
        nf = np.broadcast_to(c["sizeFactors"][None, :], c["counts"].shape)
        cn = np.sort(c["counts"] / nf, axis=1)
        k = int(np.floor(m * 0.2))
        tm = cn[:, k:m - k].mean(axis=1)
        rounded = np.where(res["replaceCounts"] != c["counts"], np.rint(tm[:, None] * nf).astype(res["replaceCounts"].dtype),
                           res["replaceCounts"])
        assert (rounded != res["replaceCounts"]).any()                 # (some replacement has a fractional part above one half)
        out["replacement_rounded"] = mut(replaceCounts=rounded)
        old = (c["counts"] / nf).mean(axis=1)
        out["base_mean_of_a_replaced_row_left"] = mut(baseMean=np.where(rep, old, res["baseMean"]))
    return out


@pytest.mark.parametrize("name", ["bc_outliers", "bc_no_refit", "factor4_mean"])
def test_chain_mutants_fail_the_audit(oracle, name):
    c, res = CASES[name], _run(oracle, name)
    scalars = not _refitted(res)
    seen = set()
    for mname, wrong in _mutants(c, res).items():
        if mname in ("mad_without_1.4826",) and not scalars:
            continue
        if mname == "prior_var_trigamma_m_minus_p" and res["dispersionFunction"]["dispPriorVar"] == 0.25:
            continue                                                   # (both on the floor: factor4_mean sees this one)
        if mname == "prior_var_without_floor" and res["dispersionFunction"]["dispPriorVar"] > 0.25:
            continue
        e = H.chain_audit(c, wrong, scalars=scalars, trend_fits=None).excess()
        print("%s mutant %s: %.3g x the budget" % (name, mname, e))
        assert e >= 10.0, "mutant %s is invisible at %s: %.3g x the budget" % (mname, name, e)
        seen.add(mname)
    want = {"bc_outliers": {"replacement_rounded", "base_mean_of_a_replaced_row_left", "max_cooks_over_all_samples", "one_sided_pvalue"},
            "bc_no_refit": {"mad_without_1.4826", "prior_var_without_floor", "outlier_sd_1", "dispersion_map_on_outlier_rows",
                            "dispfit_coefficients_swapped", "natural_log_beta_over_log2_se"},
            "factor4_mean": {"prior_var_trigamma_m_minus_p"}}[name]
    assert want <= seen, want - seen


def test_beta_prior_var_from_the_unweighted_quantile_fails(oracle):
    name = "factor4_prior_expanded_no_refit"
    c, res = CASES[name], _run(oracle, name)
    live = np.nan_to_num(res["allZero"], nan=1.0) == 0
    wrong = [v for v, _ in H.beta_prior_var(res["mle_beta"][live], res["baseMean"][live], res["dispFit"][live], c["x_names"],
                                            c["factors"], True, weighted=False)]
    r = dict(res, betaPriorVar=np.array([float(v) for v in wrong]))
    e = H.chain_audit(c, r, trend_fits=None, rows=H.heavy_rows(res, 4)).excess()
    print("unweighted quantile: %.3g x the budget" % e)
    assert e >= 10.0


def test_cooks_cutoff_against_scipy():
    from scipy.stats import f as fdist
    for p, m in ((2, 8), (3, 16), (4, 28), (13, 24)):
        assert abs(float(H.cooks_cutoff_mp(p, m)) - fdist.ppf(.99, p, m - p)) <= 1e-12 * fdist.ppf(.99, p, m - p)


def test_lrt_p_values_against_mpmath():
    """host code of the LRT path: pchisq(stat, df, lower.tail = FALSE) (R/core.R:1878) against the regularised upper incomplete
    gamma function"""
    mp = H.mp
    rng = np.random.default_rng(3)
    stat = np.concatenate([np.exp(rng.uniform(-20, 6.5, 300)), [0.0, 1e-300, 700.0]])
    for df in (1, 2, 3, 12):
        got = core.pchisq_upper(stat, df)
        for s, g in zip(stat, got):
            want = mp.gammainc(mp.mpf(df) / 2, mp.mpf(float(s)) / 2, mp.inf, regularized=True)
            assert abs(mp.mpf(float(g)) - want) <= 1e-12 * want + mp.mpf(2) ** -1074, (s, df, g, want)
    assert np.isnan(core.pchisq_upper(np.array([np.nan]), 2)[0])


@pytest.mark.parametrize("weights", [False, True])
def test_use_t_p_values_of_the_wald_test(oracle, weights):
    """nbinomWaldTest(useT = TRUE) (R/core.R:1474-1505) run through core on the oracle engine: the returned WaldPvalue is
    2 pt(|stat|, df, lower.tail = FALSE) = I_{df / (df + stat^2)}(df / 2, 1 / 2) at the returned statistic, df = m - p, or the
    row sum of the normalised weights - p; rows with df <= 0 are NA.  (A one-sided or a wrong-df p-value is off by orders of
    magnitude more than the 1e-12 scipy's pt is held to here.)"""
    mp = H.mp
    c = CASES["bc_weights" if weights else "two_group"]
    n = 60
    w = None
    if weights:
        w = c["weights"][:n].copy()
        w[3, 2:] = 0.0                                                          # df <= 0 on one row
    dds = core.DESeqDataSet(c["counts"][:n], c["x"], sizeFactors=c["sizeFactors"], weights=w, engine=HostEngine(oracle))
    core.DESeq(dds, useT=True, minReplicatesForReplace=np.inf)
    stat, pval = np.asarray(dds.mcols["WaldStatistic"]), np.asarray(dds.mcols["WaldPvalue"])
    m, p = c["x"].shape
    wn = w / w.max(axis=1, keepdims=True) if weights else None
    checked = 0
    for i in range(n):
        if not np.isfinite(stat[i]).all():
            continue
        df = (mp.fsum(mp.mpf(float(t)) for t in wn[i]) if weights else mp.mpf(m)) - p
        for k in range(p):
            if df <= 0:
                assert np.isnan(pval[i, k])
                continue
            want = mp.betainc(df / 2, mp.mpf(1) / 2, 0, df / (df + mp.mpf(float(stat[i, k])) ** 2), regularized=True)
            assert abs(mp.mpf(float(pval[i, k])) - want) <= 1e-12 * want, (i, k, pval[i, k], want)
            checked += 1
    assert checked > 100


@pytest.mark.parametrize("name", ["bc_no_refit", "bc_weights"])
def test_the_reduced_log_likelihood_of_the_oracle(oracle, name):
    """logLikeReduced is not a column of core.DESeq(): the oracle's closed-form ~ 1 fit (R/fitNbinomGLMs.R:99-137) at the chain's
    dispersions, held to the audit's statement -- where the logLikeReduced budget was measured"""
    c = dict(CASES[name], test="LRT")
    dds = core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], weights=c.get("weights"), engine=HostEngine(oracle))
    core.DESeq(dds, **CC.chain_kwargs(c))
    res = CC.result_of(dds)
    nz = dds.attrs["nz_rows"]
    sub = dds.subset(nz)
    sub.mcols["dispersion"] = dds.mcols["dispersion"][nz]
    w, useW = core.getAndCheckWeights(sub)
    red = core.fitNbinomGLMs(sub, modelMatrix=np.ones((dds.m, 1)), weights=w, useWeights=useW, want_hat=False, want_loglike=True)
    res["logLikeReduced"] = np.full(dds.n, np.nan)
    res["logLikeReduced"][nz] = red["logLike"]
    R = H.chain_audit(c, res, scalars=False)
    print("%s (LRT) %s" % (name, R.summary()))
    assert not R.failures and R.counts["logLikeReduced"] > 0
    for k in ("logLikeReduced", "LRTStatistic"):
        assert R.ratios[k] <= H.BUDGETS[k] / 2, (k, R.ratios[k])
    wrong = dict(res, logLikeReduced=res["logLike"])                            # the full model's for the reduced one
    assert H.chain_audit(c, wrong, scalars=False).excess() >= 10.0
