"""The analyses tests/hp_reference.py: chain_audit runs on (tests/test_chain_audit_cpu.py over the oracle chain,
tests/test_gpu_chain_audit.py over the device), and the adapter from a core / fused DESeqDataSet to the names
native.DESeq() returns.  The shapes are the smallest at which every glue kernel still takes each of its paths; the seeds
were chosen on the CPU, over the oracle chain alone, so that the preconditions of test_chain_audit_cpu.py hold."""
import numpy as np

from deseq2_amd import simulate


def design_batch_condition_16():
    """~ batch + condition on 16 samples, 8 per condition; one sample of each condition sits in the second batch, so that the
    design cells have 7, 1, 7 and 1 members: the cells of 7 are replaceable at minReplicatesForReplace = 7, the cells of 1
    do not count for maxCooks (recordMaxCooks: cells of >= 3)"""
    m = 16
    cond = (np.arange(m) >= 8).astype(np.float64)
    batch = np.isin(np.arange(m), (7, 15)).astype(np.float64)
    return np.column_stack([np.ones(m), batch, cond])


def design_paired(patients):
    pat = np.repeat(np.arange(patients), 2)
    return np.column_stack([np.ones(2 * patients)] + [(pat == k).astype(float) for k in range(1, patients)]
                           + [np.tile([0.0, 1.0], patients)])


def _plant(counts, seed, spikes=8, flat=4, zero_every=97, spike_cols=None):
    """count outliers (one count 40 x the row maximum), rows without any dispersion (the same count in every sample:
    dispGeneEst and dispMAP end on the minDisp clamp) and all-zero rows"""
    rng = np.random.default_rng(seed)
    c = counts.copy()
    n, m = c.shape
    rows = rng.choice(n, spikes + flat, replace=False)
    for r in rows[:spikes]:
        j = rng.integers(m) if spike_cols is None else rng.choice(spike_cols)
        c[r, j] = int(c[r].max() * 40 + 1000)
    for r in rows[spikes:]:
        c[r] = 200 + 50 * int(rng.integers(1, 9))
    if zero_every:
        c[5::zero_every] = 0
    return c


def _case(n, x, seed, sf_sd=0.2, **kw):
    m = x.shape[0]
    sf = np.exp(np.random.default_rng(seed + 1000).normal(0, sf_sd, m))
    d = simulate.make_counts(n, x, seed=seed, size_factors=sf)
    c = d["counts"]
    if c.shape[0] < n:                                    # (make_counts drops all-zero draws: keep the row count of the table)
        c = np.vstack([c, c[: n - c.shape[0]]])
    return {"counts": _plant(c, seed, **kw.pop("plant", {})), "x": x, "sizeFactors": sf, **kw}


def cases():
    xbc, rng = design_batch_condition_16(), np.random.default_rng(77)
    out = {"two_group": _case(600, simulate.design_two_group(8), 11)}
    bc = _case(600, xbc, 12, plant={"spike_cols": [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14], "spikes": 10})
    out["bc_outliers"] = dict(bc, minReplicatesForReplace=7)
    out["bc_no_refit"] = dict(bc, minReplicatesForReplace=np.inf)
    w = rng.uniform(0.05, 1.0, bc["counts"].shape)
    w[rng.uniform(size=w.shape) < 0.04] = 0.0
    out["bc_weights"] = dict(_case(600, xbc, 13), weights=w, minReplicatesForReplace=np.inf)
    nfm = np.exp(rng.normal(0, 0.2, bc["counts"].shape))
    out["bc_nf_matrix"] = dict(_case(600, xbc, 14), normalizationFactors=nfm, minReplicatesForReplace=np.inf)
    x4 = simulate.design_factor(28, 4)
    f4 = {"group": (np.arange(28) * 4) // 28}
    names4 = ["Intercept", "group1", "group2", "group3"]
    c4 = _case(400, x4, 15)
    for mmt in ("expanded", "standard"):                  # cells of 7: with the refit, and without it for the all-gene scalars
        pc = dict(c4, betaPrior=True, factors=f4, x_names=names4, modelMatrixType=mmt)
        out["factor4_prior_" + mmt] = pc
        out["factor4_prior_%s_no_refit" % mmt] = dict(pc, minReplicatesForReplace=np.inf)
    out["factor4_mean"] = dict(c4, fitType="mean")
    out["factor4_mean_no_refit"] = dict(c4, fitType="mean", minReplicatesForReplace=np.inf)
    out["paired12"] = _case(300, design_paired(12), 16, plant={"spikes": 4})
    big = _case(4200, xbc, 17)
    out["bc_4200"] = dict(big, minReplicatesForReplace=7)
    out["bc_4200_no_refit"] = dict(big, minReplicatesForReplace=np.inf)
    out["bc_lrt"] = dict(bc, test="LRT", minReplicatesForReplace=7)          # nbinomLRT against ~ 1, refit included
    return out


def native_kwargs(c):
    keys = ("normalizationFactors", "weights", "minReplicatesForReplace", "betaPrior", "factors", "modelMatrixType", "fitType", "test")
    return {k: c[k] for k in keys if k in c}


# every case whose run refits replaced rows, with the run on the same data that does not: the all-gene scalars are audited on
# the second and must be bit-identical on the first (R/core.R:2512-2527)
REFIT_PAIRS = [("bc_outliers", "bc_no_refit"), ("bc_lrt", "bc_no_refit"), ("bc_4200", "bc_4200_no_refit"),
               ("factor4_mean", "factor4_mean_no_refit"), ("factor4_prior_expanded", "factor4_prior_expanded_no_refit"),
               ("factor4_prior_standard", "factor4_prior_standard_no_refit")]


def chain_kwargs(c):
    keys = ("minReplicatesForReplace", "betaPrior", "factors", "modelMatrixType", "fitType", "test")
    kw = {k: c[k] for k in keys if k in c}
    if kw.get("test") == "LRT":
        kw["reduced"] = np.ones((c["x"].shape[0], 1))
    return kw


def result_of(dds):
    """what core.DESeq() / fused.DESeq() left on the object, under the names of native.DESeq()'s result"""
    from scipy.stats import f as fdist
    E = dds.engine
    mc = dds.mcols
    n = dds.n
    res = {k: np.asarray(mc[k], np.float64) for k in ("baseMean", "baseVar", "allZero", "dispGeneEst", "dispGeneIter", "dispFit",
                                                      "dispMAP", "dispersion", "dispIter", "dispOutlier", "beta", "betaSE",
                                                      "betaIter", "maxCooks")}
    if "WaldStatistic" in mc:
        res["stat"], res["pvalue"] = np.asarray(mc["WaldStatistic"], np.float64), np.asarray(mc["WaldPvalue"], np.float64)
    else:
        res["LRTStatistic"], res["LRTPvalue"] = np.asarray(mc["LRTStatistic"], np.float64), np.asarray(mc["LRTPvalue"], np.float64)
        res["df"] = dds.p - 1
    res["logLike"] = np.asarray(mc["deviance"], np.float64) / -2.0
    res["replace"] = np.asarray(mc["replace"], np.float64) if "replace" in mc else np.full(n, np.nan)
    nz = dds.attrs.get("nz_rows")
    for k in ("mu", "H", "cooks", "replaceCounts"):
        if k not in dds.assays:
            continue
        a = np.asarray(E.to_numpy(dds.assays[k]))
        if nz is not None and a.shape[0] != n:
            full = np.zeros((n, a.shape[1]), a.dtype)
            full[nz] = a
            a = full
        res[k] = a
    res["dispersionFunction"] = dict(dds.dispersionFunction)
    m, p = dds.x.shape
    run = getattr(dds, "_fused_run", None)               # the resident chain keeps the cutoff it ran with; core.replaceOutliers
    res["cooksCutoff"] = float(run.cooksCutoff) if run is not None else float(fdist.ppf(.99, p, m - p))   # computes this expression inline
    if dds.attrs.get("betaPrior"):
        res["betaPriorVar"] = np.asarray(dds.attrs["betaPriorVar"], np.float64)
        res["mle_beta"] = np.asarray(mc["MLE_beta"], np.float64)
    return res
