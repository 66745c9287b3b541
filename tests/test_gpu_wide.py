"""-m gpu: wide designs, 11 <= p <= 48: generic kernel pairs (loops not unrolled, p x p state in scratch memory)
over the design zero-padded to 16, 24, 32 or 48 columns (csrc/capi.hip, "wide designs").  Padding must be invisible: every
output identical to the oracle run at the TRUE p."""
import numpy as np
import pytest

from deseq2_amd import core, native, simulate
from deseq2_amd.engine import DeviceEngine, HostEngine
from tests.helpers import assert_same, make_case
from tests.wide_cases import paired as _paired_design      # ~ patient + treatment (2 * patients samples, p = patients + 1)

pytestmark = pytest.mark.gpu

BETA_KEYS = ["iter", "beta_mat", "beta_var_mat", "deviance", "contrast_num", "contrast_denom", "hat_diagonals"]
DISP_KEYS = ["iter", "iter_accept", "log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp",
             "last_d2lp"]


@pytest.mark.parametrize("levels,m,useW,useQR", [(11, 66, False, True), (12, 60, True, True), (13, 91, False, False),
                                                 (16, 96, True, False), (16, 160, False, True), (14, 500, False, True),
                                                 (17, 85, False, True), (20, 100, True, False), (24, 120, False, True)])
def test_wide_native_routines_match_oracle(oracle, levels, m, useW, useQR):
    d = make_case(120, m, ("factor", levels), seed=levels + m, weights=useW, sf_random=True)
    p = d["x"].shape[1]
    assert p == levels
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    lam[3] = 0.7                                           # one real ridge penalty among the wide priors
    contrast = np.zeros(p); contrast[0] = 1.0; contrast[p - 1] = -1.0
    bargs = (d["counts"], d["x"], d["nf"], d["alpha_init"], contrast, d["beta_init"], lam, d["weights"], useW, 1e-8,
             100, useQR, 0.5)
    gb, ob = native.fitBeta(*bargs), oracle.fitBeta(*bargs)
    for k in BETA_KEYS:
        assert_same(gb[k], ob[k], "fitBeta$" + k)
    assert (ob["iter"] < 100).mean() > 0.8
    mu = oracle.fittedMu(d["x"], d["nf"], ob["beta_mat"], 0.5)
    mu = np.where(np.isfinite(mu), mu, 0.5)
    la = np.log(d["alpha_init"])
    w = np.maximum(d["weights"], 1e-6) if useW else d["weights"]
    for prior in (False, True):
        dargs = (d["counts"], d["x"], mu, la, la - 0.1, 0.8, np.log(1e-9), 1.0, 1e-6, 100, prior, w, useW, 1e-2, True)
        gd, od = native.fitDisp(*dargs), oracle.fitDisp(*dargs)
        for k in DISP_KEYS:
            assert_same(gd[k], od[k], "fitDisp$" + k)
    grid = np.linspace(np.log(1e-8), np.log(max(10, m)), 15)
    gargs = (d["counts"][:40], d["x"], mu[:40], grid, la[:40], 1.0, True, w[:40], useW, 1e-2, True)
    assert_same(native.fitDispGrid(*gargs)["log_alpha"], oracle.fitDispGrid(*gargs)["log_alpha"], "fitDispGrid")


@pytest.mark.parametrize("levels,m,useW", [(11, 66, False), (16, 96, True), (20, 100, False), (24, 120, True)])
def test_wide_optim_rows_match_oracle(oracle, levels, m, useW):
    """dsq_optim_rows on a wide design (the rows fitNbinomGLMsOptim re-fits, R/fitNbinomGLMs.R:340-407): the padded
    kernel against the oracle's iteration at the true p, every output"""
    d = make_case(24, m, ("factor", levels), seed=3 * levels + m, weights=useW, sf_random=True)
    y = d["counts"].copy()
    y[3] = 0; y[3, 5:9] = 1000                      # rows the IRLS cannot fit
    y[11] = 0; y[11, -1] = 7
    y[20, : m // 2] = 0
    p = levels
    lam = np.full(p, 1e-6)
    lam[-1] = 0.5
    start = np.random.default_rng(3).normal(0, 1.0, (y.shape[0], p))
    args = (y, d["x"], d["nf"], d["alpha_init"], lam, d["weights"], useW, start, 0.5)
    got, want = native.optimRows(*args), oracle.optimRows(*args)
    for k in ("beta", "betaSE", "conv", "mu", "logLike"):
        assert_same(np.asarray(got[k], float), np.asarray(want[k], float), "wide optimRows$" + k)
    assert want["conv"].mean() > 0.8


def test_wide_chain_with_optim_rows_matches_oracle(oracle):
    """a wide analysis with rows the IRLS does not fit (a continuous covariate next to a 15-level factor): the
    call-by-call chain on the device, optim rows included, against the oracle chain"""
    m = 90
    x = np.column_stack([simulate.design_factor(m, 15), np.random.default_rng(5).normal(size=m)])
    d = simulate.make_counts(150, x, seed=8, beta_sd=np.array([0.5] * 14 + [0.3]))
    y = d["counts"].copy()
    y[7] = 0; y[7, 40:43] = 3000
    y[19] = 0; y[19, -1] = 11
    E = DeviceEngine("cuda:0")
    calls, inner = [], E.optim_rows
    E.optim_rows = lambda *a_, **k_: (calls.append(a_[0].shape[0] if hasattr(a_[0], "shape") else 1), inner(*a_, **k_))[1]
    a = core.DESeq(core.DESeqDataSet(y, x, engine=E), minReplicatesForReplace=np.inf)
    assert calls, "no row went to the optim fallback: the case does not exercise it"
    b = core.DESeq(core.DESeqDataSet(y, x, engine=HostEngine(oracle)), minReplicatesForReplace=np.inf)
    for k in ("dispGeneEst", "dispersion", "beta", "betaSE", "WaldStatistic", "betaConv", "betaIter", "deviance"):
        assert_same(a.mcols[k], b.mcols[k], "wide DESeq() with optim rows$" + k)


@pytest.mark.parametrize("p,m,useW,useQR", [
    (10, 200, False, True), (10, 500, True, True), (10, 130, False, False),       # stored-row QR (LDS) from p = 10
    (9, 250, False, True), (9, 300, True, True), (7, 256, False, True), (7, 257, False, True),   # serial Gram up to m = 256 below p = 10
    (16, 120, False, True), (16, 400, True, True), (24, 100, False, True), (24, 260, False, True), (12, 1100, False, True),
    # round 4: rows in registers, four trips (m + p <= 256) / eight trips (<= 512, p <= 10) and the first shapes beyond
    (8, 248, True, True), (8, 440, False, True), (10, 502, False, True), (10, 503, False, True), (16, 304, False, True), (16, 305, True, True)])
def test_general_path_kernels_match_oracle(oracle, p, m, useW, useQR):
    """designs with a CONTINUOUS covariate (one design cell per sample) at the widths where round 3 changed the general
    kernels: fitBeta's stored-row Householder QR (rows of the least squares in LDS, p >= 10; the replay where they do
    not fit) and fitDisp's entry-per-lane Cox-Reid Gram (serial sums, p >= 7 and m <= 256 / 1024) -- every output
    identical to the oracle at the true p, on both sides of each threshold"""
    rng = np.random.default_rng(100 * p + m)
    levels = p - 1
    x = np.column_stack([simulate.design_factor(m, levels), rng.normal(0.0, 0.5, m)])
    assert x.shape[1] == p and np.linalg.matrix_rank(x) == p
    d = simulate.make_counts(90, x, seed=p + m, beta_sd=np.array([0.5] * (p - 2) + [0.3]),
                             size_factors=np.exp(rng.normal(0, 0.2, m)))
    counts = d["counts"]
    n = counts.shape[0]
    nf = np.broadcast_to(d["size_factors"][None, :], (n, m)).copy()
    w = np.ones((n, m))
    if useW:
        w = rng.uniform(0.05, 1.0, (n, m))
        w[rng.uniform(size=(n, m)) < 0.02] = 0.0
        w = w / w.max(axis=1, keepdims=True)
    from tests.helpers import beta_init_qr, rough_alpha
    with np.errstate(all="ignore"):
        binit = beta_init_qr(counts.astype(float), nf, x)
        alpha = np.nan_to_num(rough_alpha(counts.astype(float), nf, x), nan=0.1)
    alpha = np.clip(alpha, 1e-8, max(10, m))
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    contrast = np.zeros(p); contrast[-1] = 1.0
    bargs = (counts, x, nf, alpha, contrast, binit, lam, w, useW, 1e-8, 100, useQR, 0.5)
    gb, ob = native.fitBeta(*bargs), oracle.fitBeta(*bargs)
    for k in BETA_KEYS:
        assert_same(gb[k], ob[k], "general fitBeta$" + k)
    mu = oracle.fittedMu(x, nf, ob["beta_mat"], 0.5)
    mu = np.where(np.isfinite(mu), mu, 0.5)
    la = np.log(alpha)
    wd = np.maximum(w, 1e-6) if useW else w
    for prior in (False, True):
        dargs = (counts, x, mu, la, la - 0.1, 0.8, np.log(1e-9), 1.0, 1e-6, 100, prior, wd, useW, 1e-2, True)
        gd, od = native.fitDisp(*dargs), oracle.fitDisp(*dargs)
        for k in DISP_KEYS:
            assert_same(gd[k], od[k], "general fitDisp$" + k)
    grid = np.linspace(np.log(1e-8), np.log(max(10, m)), 12)
    gargs = (counts[:24], x, mu[:24], grid, la[:24], 1.0, True, wd[:24], useW, 1e-2, True)
    assert_same(native.fitDispGrid(*gargs)["log_alpha"], oracle.fitDispGrid(*gargs)["log_alpha"], "general fitDispGrid")


def test_wide_chain_lrt_matches_oracle(oracle):
    """12-level factor, nbinomLRT against the intercept: the whole DESeq() chain on the HBM-resident engine"""
    m = 96
    x = simulate.design_factor(m, 12)
    d = simulate.make_counts(200, x, seed=61)
    a = core.DESeq(core.DESeqDataSet(d["counts"], x, engine=DeviceEngine("cuda:0")), test="LRT",
                   reduced=np.ones((m, 1)))
    b = core.DESeq(core.DESeqDataSet(d["counts"], x, engine=HostEngine(oracle)), test="LRT", reduced=np.ones((m, 1)))
    for k in ("dispGeneEst", "dispGeneIter", "dispersion", "dispIter", "beta", "betaSE", "LRTStatistic", "LRTPvalue",
              "fullBetaConv", "betaIter", "deviance", "maxCooks"):
        assert_same(a.mcols[k], b.mcols[k], "wide LRT DESeq()$" + k)


def _native_triplet_vs_oracle(oracle, counts, x, sf, tag, useW=False, seed=0):
    n, m = counts.shape
    p = x.shape[1]
    nf = np.broadcast_to(np.asarray(sf)[None, :], (n, m)).copy()
    rng = np.random.default_rng(seed)
    w = np.ones((n, m))
    if useW:
        w = rng.uniform(0.05, 1.0, (n, m))
        w = w / w.max(axis=1, keepdims=True)
    from tests.helpers import beta_init_qr, rough_alpha
    with np.errstate(all="ignore"):
        binit = beta_init_qr(counts.astype(float), nf, x)
        alpha = np.nan_to_num(rough_alpha(counts.astype(float), nf, x), nan=0.1)
    alpha = np.clip(alpha, 1e-8, max(10, m))
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    contrast = np.zeros(p); contrast[-1] = 1.0
    bargs = (counts, x, nf, alpha, contrast, binit, lam, w, useW, 1e-8, 100, True, 0.5)
    gb, ob = native.fitBeta(*bargs), oracle.fitBeta(*bargs)
    for k in BETA_KEYS:
        assert_same(gb[k], ob[k], tag + " fitBeta$" + k)
    assert (ob["iter"] < 100).mean() > 0.7
    mu = oracle.fittedMu(x, nf, ob["beta_mat"], 0.5)
    mu = np.where(np.isfinite(mu), mu, 0.5)
    la = np.log(alpha)
    wd = np.maximum(w, 1e-6) if useW else w
    for prior in (False, True):
        dargs = (counts, x, mu, la, la - 0.1, 0.8, np.log(1e-9), 1.0, 1e-6, 100, prior, wd, useW, 1e-2, True)
        gd, od = native.fitDisp(*dargs), oracle.fitDisp(*dargs)
        for k in DISP_KEYS:
            assert_same(gd[k], od[k], tag + " fitDisp$" + k)
    grid = np.linspace(np.log(1e-8), np.log(max(10, m)), 12)
    gargs = (counts[:24], x, mu[:24], grid, la[:24], 1.0, True, wd[:24], useW, 1e-2, True)
    assert_same(native.fitDispGrid(*gargs)["log_alpha"], oracle.fitDispGrid(*gargs)["log_alpha"], tag + " fitDispGrid")


@pytest.mark.parametrize("patients,useW", [(30, False), (26, True), (45, False)])
def test_paired_designs_beyond_24_columns(oracle, patients, useW):
    """round 5 (VERDICT r4 missing #1): `~ patient + treatment` -- 30 patients: p = 31, 60 cells, the 32-column build;
    45 patients: p = 46 on the 48-column build -- through fitBeta / fitDisp / fitDispGrid, identical to the oracle at
    the true p.  The reference has no width limit (src/DESeq2.cpp:283-465)."""
    x = _paired_design(patients)
    rng = np.random.default_rng(patients)
    sf = np.exp(rng.normal(0, 0.2, x.shape[0]))
    d = simulate.make_counts(70, x, seed=patients, beta_sd=np.array([0.4] * (patients - 1) + [1.0]), size_factors=sf)
    _native_triplet_vs_oracle(oracle, d["counts"], x, sf, "paired %d" % patients, useW=useW, seed=patients)


@pytest.mark.parametrize("levels,m", [(28, 112), (32, 128), (40, 160), (48, 192)])
def test_factors_of_up_to_48_levels(oracle, levels, m):
    """a 40-level factor (and the edges of the 32- and 48-column builds): cells of four samples; up to 32 levels both
    routines run cell-collapsed (fitBeta's collapsed least squares: 32 cells + 32 columns = the 64 lanes of a wave; the
    shared spec, include/dsq_arith_spec.h, says so to kernels and oracle alike), beyond that the general kernels"""
    d = make_case(80, m, ("factor", levels), seed=levels + m, sf_random=True)
    _native_triplet_vs_oracle(oracle, d["counts"], d["x"], d["size_factors"], "factor %d" % levels)


def test_wide_chain_paired_design_matches_oracle(oracle):
    """the whole DESeq() chain (fused device chain and the one-call host entry) on a paired design with 30 patients"""
    from deseq2_amd import fused
    x = _paired_design(30)
    d = simulate.make_counts(160, x, seed=77, beta_sd=np.array([0.4] * 29 + [1.0]))
    E = DeviceEngine("cuda:0")
    a = core.DESeqDataSet(d["counts"], x, engine=E)
    assert fused.supported(a)
    fused.DESeq(a)
    assert a.attrs.get("fused")
    b = core.DESeq(core.DESeqDataSet(d["counts"], x, engine=HostEngine(oracle)))
    for k in ("dispGeneEst", "dispGeneIter", "dispersion", "dispIter", "beta", "betaSE", "WaldStatistic", "betaIter", "deviance"):
        assert_same(a.mcols[k], b.mcols[k], "paired-design chain$" + k)
    res = native.DESeq(d["counts"], x, np.ones(x.shape[0]), assays=())
    for k, kr in (("dispGeneEst", "dispGeneEst"), ("dispersion", "dispersion"), ("beta", "beta"), ("betaSE", "betaSE"),
                  ("stat", "WaldStatistic")):
        assert_same(np.asarray(res[k], float), np.asarray(b.mcols[kr], float), "paired-design dsq_deseq$" + k)


@pytest.mark.parametrize("p,m", [(12, 60), (16, 130), (24, 120), (31, 93), (46, 200), (56, 150), (64, 200)])
def test_wide_weights_prep_matches_host(p, m):
    """getAndCheckWeights (R/core.R:2697-2751) on designs of more than 10 columns (round 5: weights_prep_wide_kernel, the
    Gram matrices entry-per-lane, the rank test one column per lane): normalised weights, their floor and the
    weightsFail flags against the host mirror -- rows that lose a whole level, a column pair that becomes collinear
    and rows with all-zero weights included"""
    _weights_prep_case(p, m, 300)


def _weights_prep_case(p, m, n, zero_row=None):
    from deseq2_amd.engine import _weights_ok_host
    rng = np.random.default_rng(p * 1000 + m)
    x = simulate.design_factor(m, p)
    w = rng.uniform(0.02, 1.0, (n, m))
    w[rng.uniform(size=w.shape) < 0.05] = 0.0
    w[3, x[:, 2] == 1] = 0.0                               # a level without a sample: rank(w * X) < p
    w[10, x[:, p - 1] == 1] = 0.005                        # ... only below the threshold: the second test's column drop
    w[20] = 0.0                                            # apply(w, 1, max) = 0: NaN weights
    if zero_row is not None:
        w[zero_row] = 0.0
    w[30, (x[:, 1] == 0) & (x[:, 4] == 0)] = 0.0           # only levels 1 and 4 (and no reference sample) left
    E = DeviceEngine("cuda:0")
    wn, wf, fz, neg = E.weights_prep(E.matrix(w), x, 1e-2)
    with np.errstate(all="ignore"):
        want = w / w.max(axis=1, keepdims=True)
        ok = _weights_ok_host(np.nan_to_num(want, nan=0.0), x, 1e-2, True)
    got = E.to_numpy(wn)
    assert_same(got, want, "w_norm")
    assert_same(E.to_numpy(wf), np.where(np.isnan(want), want, np.maximum(want, 1e-6)), "w_floor")
    fail = E._host(fz).numpy().astype(bool)
    assert fail[3] and fail[20] and fail[30]
    keep = ~np.isnan(want).any(axis=1)
    assert (fail[keep] == ~ok[keep]).all(), np.flatnonzero(fail[keep] != ~ok[keep])
    assert int(E._host(neg).numpy()[0]) == 0
    return fail


@pytest.mark.parametrize("p,m", [(5, 10), (12, 24)])
def test_weights_prep_past_one_round(p, m):
    """the gene loops of weights_prep_kernel (`g += gridDim.x * waves`; aux_grid_fwd: eight workgroups of four waves per CU)
    and weights_prep_wide_kernel (`g += gridDim.x`; launch_weights_prep: at most 256 x 8 workgroups of one gene), csrc/aux.hip:
    five rows more than a round, the last one with all-zero weights -- the same checks as above on every row"""
    import torch
    rnd = 256 * 8 if p > 10 else 8 * torch.cuda.get_device_properties(0).multi_processor_count * 4
    n = rnd + 5
    fail = _weights_prep_case(p, m, n, zero_row=n - 1)
    assert fail.shape == (n,) and fail[n - 1] and not fail[rnd:n - 1].all()


def _chain_three_ways(oracle, counts, x, sf, tag, weights=None, **kw):
    """fused device chain == call-by-call chain on the device == the oracle's chain (HostEngine), every column"""
    from deseq2_amd import fused
    E = DeviceEngine("cuda:0")
    a = core.DESeqDataSet(counts, x, sizeFactors=sf, weights=weights, engine=E)
    assert fused.supported(a, **{k: v for k, v in kw.items() if k != "minReplicatesForReplace"})
    fused.DESeq(a, **kw)
    assert a.attrs.get("fused")
    b = core.DESeq(core.DESeqDataSet(counts, x, sizeFactors=sf, weights=weights, engine=E), **kw)
    c = core.DESeq(core.DESeqDataSet(counts, x, sizeFactors=sf, weights=weights, engine=HostEngine(oracle)), **kw)
    keys = [k for k in c.mcols if k != "rowsForOptim"]
    for k in keys:
        assert_same(np.asarray(b.mcols[k], np.float64), np.asarray(c.mcols[k], np.float64), tag + " call-by-call vs oracle$" + k)
        assert_same(np.asarray(a.mcols[k], np.float64), np.asarray(c.mcols[k], np.float64), tag + " fused vs oracle$" + k)
    return a, c


def test_wide_chain_with_observation_weights(oracle):
    """VERDICT r4 missing #4: a 14-level factor WITH observation weights stays on the fused chain (cells of 8: count
    outliers are replaced and their rows refitted), a row whose weights fail included"""
    m = 112
    x = simulate.design_factor(m, 14)
    rng = np.random.default_rng(31)
    sf = np.exp(rng.normal(0, 0.2, m))
    d = simulate.make_counts(260, x, seed=31, size_factors=sf)
    counts = d["counts"].copy()
    n = counts.shape[0]
    for r in rng.choice(n, 5, replace=False):
        counts[r, rng.integers(m)] = int(counts[r].max() * 40 + 1000)
    w = rng.uniform(0.05, 1.0, (n, m))
    w[rng.uniform(size=w.shape) < 0.02] = 0.0
    w[9, x[:, 5] == 1] = 0.0
    a, c = _chain_three_ways(oracle, counts, x, sf, "wide weights", weights=w)
    assert c.mcols["weightsFail"][9] and np.isnan(a.mcols["dispersion"][9])
    assert a.attrs["status"]["N_REFIT"] >= 1
    res = native.DESeq(counts, x, sf, weights=w, assays=())
    for k, kr in (("dispGeneEst", "dispGeneEst"), ("dispersion", "dispersion"), ("beta", "beta"), ("betaSE", "betaSE"),
                  ("stat", "WaldStatistic")):
        assert_same(np.asarray(res[k], float), np.asarray(c.mcols[kr], float), "wide weights dsq_deseq$" + k)


@pytest.mark.parametrize("patients,reps,minrep", [(12, 4, 3), (30, 1, 7), (52, 1, 7)])
def test_wide_chain_lrt_against_a_wide_reduced_model(oracle, patients, reps, minrep):
    """VERDICT r4 missing #4: `~ patient + treatment` tested by nbinomLRT against `~ patient` -- a reduced model of 12
    (30) columns under a full model of 13 (31): the reduced fit runs at its own padded width inside the chain
    (R/core.R:1856-1868), also on the rows the outlier replacement refits (12 patients, minReplicatesForReplace = 3)"""
    m = 2 * reps * patients
    pat = np.repeat(np.arange(patients), 2 * reps)
    trt = np.tile(np.repeat([0.0, 1.0], reps), patients)
    x = np.column_stack([np.ones(m)] + [(pat == k).astype(float) for k in range(1, patients)] + [trt])
    red = np.ascontiguousarray(x[:, :-1])
    rng = np.random.default_rng(patients)
    sf = np.exp(rng.normal(0, 0.2, m))
    d = simulate.make_counts(220, x, seed=patients + 5, beta_sd=np.array([0.4] * (patients - 1) + [1.0]), size_factors=sf)
    counts = d["counts"].copy()
    for r in rng.choice(counts.shape[0], 5, replace=False):
        counts[r, rng.integers(m)] = int(counts[r].max() * 40 + 1000)
    a, c = _chain_three_ways(oracle, counts, x, sf, "wide reduced %d" % patients, test="LRT", reduced=red,
                             minReplicatesForReplace=minrep)
    assert np.isfinite(np.asarray(c.mcols["LRTPvalue"], float)).mean() > 0.9
    if minrep == 3:
        assert a.attrs["status"]["N_REFIT"] >= 1
    res = native.DESeq(counts, x, sf, test="LRT", reduced=red, minReplicatesForReplace=minrep, assays=())
    for k, kr in (("dispersion", "dispersion"), ("beta", "beta"), ("betaSE", "betaSE")):
        assert_same(np.asarray(res[k], float), np.asarray(c.mcols[kr], float), "wide reduced dsq_deseq$" + k)
    lrt = 2 * (np.asarray(res["logLike"], float) - np.asarray(res["logLikeReduced"], float))
    assert_same(lrt, np.asarray(c.mcols["LRTStatistic"], float), "wide reduced dsq_deseq$LRTStatistic")


@pytest.mark.parametrize("levels,mode", [(12, "expanded"), (14, "standard"), (10, "expanded"), (20, "expanded_weights")])
def test_wide_chain_with_beta_prior(oracle, levels, mode):
    """nbinomWaldTest(betaPrior = TRUE) on factors of 10 ... 20 levels (R/core.R:1416-1432, R/fitNbinomGLMs.R:242-337): the
    expanded model matrix has levels + 1 columns (10 levels: 11 -- the first one beyond the register kernels), the prior
    pass runs at ITS padded width on the chain; fused == call-by-call == oracle chain, and the one-call host entry with
    the prior variance estimated inside the library"""
    m = levels * 8                                          # cells of 8: outliers are replaced, their rows refitted
    factors = {"condition": np.repeat(np.arange(levels), 8)}
    x, _ = core.standard_model_matrix(factors)
    assert x.shape[1] == levels
    rng = np.random.default_rng(levels)
    sf = np.exp(rng.normal(0, 0.2, m))
    d = simulate.make_counts(240, x, seed=levels + 3, size_factors=sf)
    counts = d["counts"].copy()
    for r in rng.choice(counts.shape[0], 5, replace=False):
        counts[r, rng.integers(m)] = int(counts[r].max() * 40 + 1000)
    w = None
    if mode == "expanded_weights":
        w = rng.uniform(0.05, 1.0, counts.shape)
        w[rng.uniform(size=w.shape) < 0.02] = 0.0
    kw = dict(betaPrior=True, factors=factors)
    if mode == "standard":
        kw["modelMatrixType"] = "standard"
    a, c = _chain_three_ways(oracle, counts, x, sf, "wide betaPrior %d %s" % (levels, mode), weights=w, **kw)
    assert np.asarray(a.mcols["beta"]).shape[1] == (levels if mode == "standard" else levels + 1)
    assert_same(np.asarray(a.attrs["betaPriorVar"]), np.asarray(c.attrs["betaPriorVar"]), "betaPriorVar")
    assert a.attrs["status"]["N_REFIT"] >= 1 or w is not None
    res = native.DESeq(counts, x, sf, weights=w, assays=(), betaPrior=True, factors=factors, modelMatrixType=kw.get("modelMatrixType"))
    assert_same(res["betaPriorVar"], np.asarray(c.attrs["betaPriorVar"]), "dsq_deseq: betaPriorVar")
    for k, kr in (("dispersion", "dispersion"), ("beta", "beta"), ("betaSE", "betaSE"), ("stat", "WaldStatistic"), ("mle_beta", "MLE_beta")):
        assert_same(np.asarray(res[k], float), np.asarray(c.mcols[kr], float), "wide betaPrior dsq_deseq$" + k)


@pytest.mark.parametrize("kind,levels,useW", [("paired", 55, False), ("paired", 63, True), ("factor", 56, False), ("factor", 64, False)])
def test_designs_of_49_to_64_columns(oracle, kind, levels, useW):
    """round 6: DSQ_MAX_P = 64.  49 .. 64 columns run on the 64-column build, whose fits are the rolled
    kernels alone (fit_beta_wide.hip, fit_disp_wide.hip): `~ patient + treatment` with 55 / 63 patients (p = 56 / 64),
    factors of 56 / 64 levels with four samples each -- fitBeta, fitDisp (with and without prior, d2 included), fitDispGrid
    identical to the oracle at the true p."""
    if kind == "paired":
        x = _paired_design(levels)
        rng = np.random.default_rng(levels)
        sf = np.exp(rng.normal(0, 0.2, x.shape[0]))
        d = simulate.make_counts(48, x, seed=levels, beta_sd=np.array([0.4] * (levels - 1) + [1.0]), size_factors=sf)
        _native_triplet_vs_oracle(oracle, d["counts"], x, sf, "paired %d" % levels, useW=useW, seed=levels)
    else:
        d = make_case(48, 4 * levels, ("factor", levels), seed=levels, sf_random=True)
        _native_triplet_vs_oracle(oracle, d["counts"], d["x"], d["size_factors"], "factor %d" % levels, useW=useW)


def test_wide_chain_on_a_56_column_design(oracle):
    """the whole DESeq() chain (fused device chain and the one-call host entry) on a paired design with 55 patients"""
    from deseq2_amd import fused
    x = _paired_design(55)
    d = simulate.make_counts(96, x, seed=56, beta_sd=np.array([0.4] * 54 + [1.0]))
    E = DeviceEngine("cuda:0")
    a = core.DESeqDataSet(d["counts"], x, engine=E)
    assert fused.supported(a)
    fused.DESeq(a)
    assert a.attrs.get("fused")
    b = core.DESeq(core.DESeqDataSet(d["counts"], x, engine=HostEngine(oracle)))
    for k in ("dispGeneEst", "dispGeneIter", "dispersion", "dispIter", "beta", "betaSE", "WaldStatistic", "betaIter", "deviance"):
        assert_same(a.mcols[k], b.mcols[k], "56-column chain$" + k)
    res = native.DESeq(d["counts"], x, np.ones(x.shape[0]), assays=())
    for k, kr in (("dispGeneEst", "dispGeneEst"), ("dispersion", "dispersion"), ("beta", "beta"), ("betaSE", "betaSE"),
                  ("stat", "WaldStatistic")):
        assert_same(np.asarray(res[k], float), np.asarray(b.mcols[kr], float), "56-column dsq_deseq$" + k)


def test_long_rows_beyond_48_columns_are_refused():
    """49 .. 64 columns: fitDisp takes rows of at most 1024 samples (the serial Gram sums of the arithmetic spec) -- longer
    ones are refused, not fitted otherwise"""
    from deseq2_amd import _lib
    d = make_case(4, 1100, ("factor", 50), seed=3)
    mu = np.full(d["counts"].shape, 10.0)
    la = np.zeros(4)
    with pytest.raises(_lib.DsqError):
        native.fitDisp(d["counts"], d["x"], mu, la, la, 1.0, np.log(1e-9), 1.0, 1e-6, 100, False, d["weights"], False, 1e-2, True)


def test_too_wide_is_refused():
    from deseq2_amd import _lib
    d = make_case(10, 195, ("factor", 65), seed=1)
    p = 65
    with pytest.raises(_lib.DsqError):
        native.fitBeta(d["counts"], d["x"], d["nf"], d["alpha_init"], np.r_[1.0, np.zeros(p - 1)], d["beta_init"],
                       np.full(p, 1e-6), d["weights"], False, 1e-8, 100, True, 0.5)


@pytest.mark.parametrize("geometry", [{}, {"DSQ_WIDE_LDS": "0"}, {"DSQ_WIDE_NW": "1"}, {"DSQ_WIDE_NW": "2"}, {"DSQ_WIDE_NW": "4"},
                                      {"DSQ_WIDE_NW": "8"}, {"DSQ_WIDE_LDS": "0", "DSQ_WIDE_NW": "1"}, {"DSQ_WIDE_LDS": "0", "DSQ_WIDE_NW": "2"},
                                      {"DSQ_WIDE_LDS": "0", "DSQ_WIDE_NW": "8"}, {"DSQ_WIDE_PADDED": "1"}])
def test_rolled_fit_beta_in_every_geometry(oracle, monkeypatch, geometry):
    """round 6: the rolled fitBeta kernel of the wide designs without cells (csrc/fit_beta_wide.hip) in each of its launch
    geometries -- the gene's slab in LDS or in global memory, 1 / 2 / 4 / 8 waves per gene -- on a paired design (p = 19, 36
    cells), with and without weights, QR and normal equations, the contrast-only mode (maxit = 0, R/results.R:797), a row
    with every second sample at 3000 and the others at zero (fitted means on the minmu floor) and an all-but-one-zero row: every
    output identical to the oracle's in every geometry (which wave takes a sum does not enter the result).  The default runs
    at the design's own width (19 columns of the 24-column build), DSQ_WIDE_PADDED=1 at the padded one."""
    for k, v in geometry.items():
        monkeypatch.setenv(k, v)
    x = _paired_design(18)
    m, p = x.shape
    rng = np.random.default_rng(19)
    sf = np.exp(rng.normal(0, 0.2, m))
    d = simulate.make_counts(90, x, seed=19, beta_sd=np.array([0.4] * 17 + [1.0]), size_factors=sf)
    y = d["counts"].copy()
    y[3] = 0
    y[3, 5] = 7                                            # a single count
    y[4] = 0
    y[4, ::2] = 3000                                       # every patient's first sample 3000, the second 0
    nf = np.broadcast_to(sf, y.shape).copy()
    w = rng.uniform(0.2, 1.0, y.shape)
    w[7, :4] = 0.0
    from tests.helpers import beta_init_qr, rough_alpha
    with np.errstate(all="ignore"):
        b0 = beta_init_qr(y.astype(float), nf, x)
        a0 = rough_alpha(y.astype(float), nf, x)
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    lam[2] = 0.5
    con = np.zeros(p); con[-1] = 1.0
    for useW in (False, True):
        for useQR in (True, False):
            args = (y, x, nf, a0, con, b0, lam, w if useW else np.ones(y.shape), useW, 1e-8, 100, useQR, 0.5)
            g, o = native.fitBeta(*args), oracle.fitBeta(*args)
            for k in BETA_KEYS:
                assert_same(g[k], o[k], "rolled fitBeta$%s (weights %s, QR %s, %r)" % (k, useW, useQR, geometry))
            if not useW and useQR:
                fitted = (g, o)
    # the contrast-only call on the fitted coefficients
    c2 = np.zeros(p); c2[1] = 1.0; c2[2] = -1.0
    args0 = (y, x, nf, a0, c2, fitted[1]["beta_mat"], lam, np.ones(y.shape), False, 1e-8, 0, True, 0.5)
    g0, o0 = native.fitBeta(*args0), oracle.fitBeta(*args0)
    for k in BETA_KEYS:
        assert_same(g0[k], o0[k], "rolled fitBeta (maxit = 0)$%s (%r)" % (k, geometry))
    assert (o0["iter"] == 0).all()


@pytest.mark.parametrize("geometry", [{}, {"DSQ_WIDE_NW": "1"}, {"DSQ_WIDE_NW": "2"}, {"DSQ_WIDE_NW": "4"}, {"DSQ_WIDE_NW": "8"},
                                      {"DSQ_DISP_ROLLED": "0"}])
def test_rolled_fit_disp_in_every_geometry(oracle, monkeypatch, geometry):
    """round 6: the rolled fitDisp / fitDispGrid / d2log_posterior kernel of the wide designs without cells
    (csrc/fit_disp_wide.hip) with 1 / 2 / 4 / 8 waves per gene, and the per-width kernel it replaces (DSQ_DISP_ROLLED=0), on
    a paired design (p = 27 on the 32-column build, 52 cells): with and without weights (a row with a sample group below the
    weight threshold: a dropped column), with and without prior and Cox-Reid term, an all-zero row and a row on the minmu
    floor -- every output identical to the oracle's in every geometry (which thread takes a matrix entry, which wave a row of
    an elimination step, does not enter the result)."""
    for k, v in geometry.items():
        monkeypatch.setenv(k, v)
    x = _paired_design(26)
    m, p = x.shape
    rng = np.random.default_rng(27)
    sf = np.exp(rng.normal(0, 0.2, m))
    d = simulate.make_counts(60, x, seed=27, beta_sd=np.array([0.4] * 25 + [1.0]), size_factors=sf)
    y = d["counts"].copy()
    y[2] = 0
    y[5] = 0
    y[5, ::2] = 2000
    nf = np.broadcast_to(sf, y.shape).copy()
    from tests.helpers import beta_init_qr, rough_alpha
    with np.errstate(all="ignore"):
        alpha = np.nan_to_num(rough_alpha(y.astype(float), nf, x), nan=0.1)
    alpha = np.clip(alpha, 1e-8, 10.0)
    la = np.log(alpha)
    mu = np.maximum(nf * np.exp(rng.normal(3, 1, (y.shape[0], 1))), 0.5)
    mu[5] = 0.5
    for useW in (False, True):
        w = np.ones(y.shape)
        if useW:
            w = rng.uniform(0.05, 1.0, y.shape)
            w[7, x[:, 3] == 1] = 1e-4                      # patient 3's samples below the threshold: column 3 is dropped
            w = np.maximum(w / w.max(axis=1, keepdims=True), 1e-6)
        for prior, useCR in ((False, True), (True, True), (True, False)):
            dargs = (y, x, mu, la, la - 0.2, 0.7, np.log(1e-9), 1.0, 1e-6, 100, prior, w, useW, 1e-2, useCR)
            gd, od = native.fitDisp(*dargs), oracle.fitDisp(*dargs)
            for k in DISP_KEYS:
                assert_same(gd[k], od[k], "rolled fitDisp$%s (useW=%d prior=%d CR=%d, %r)" % (k, useW, prior, useCR, geometry))
        grid = np.linspace(np.log(1e-8), np.log(10.0), 10)
        gargs = (y, x, mu, grid, la, 1.0, True, w, useW, 1e-2, True)
        assert_same(native.fitDispGrid(*gargs)["log_alpha"], oracle.fitDispGrid(*gargs)["log_alpha"],
                    "rolled fitDispGrid (useW=%d, %r)" % (useW, geometry))
