"""-m gpu: the memory contract of the DESeq() chain (dsq_deseq_dev, csrc/pipeline.hip) on poisoned memory (tests/poison.py).

The value suites run the fused chain right after the call-by-call chain on the same data, so the caching allocator hands it
blocks that hold the correct intermediates of the same analysis: a vector of the workspace that a phase reads before any phase
has written it would still give the right answer.  Here every buffer the chain is handed comes from an arena: the workspace
(exactly dsq_deseq_workspace_bytes bytes, so that an overrun lands in a guard), the result block and the five assays start
in one of three states -- every byte 0xFF, every byte 0x00, or LEFT BY ANOTHER ANALYSIS: the bytes a run of the same shape and
options on other data (another seed, its own outliers and zero rows elsewhere) left in them -- and the padding columns
m .. ld-1 of every gene-major input hold garbage (-7 in the counts, NaN in the weights and -- case 10, the one analysis that
reads a normalization-factor matrix; the others read the m size factors -- in the factors; ld = round8(m) + 8, so there is
padding at every m).  Every other device input of the chain (design, its QR, the reduced and prior designs, size factors,
dispersion grid, weightsFail flags, the caller's trend values) is an arena copy as well, guarded and watched.  Per case:

  (a) the three runs agree bit for bit on every defined element of every output;
  (b) they equal the call-by-call chain of core.DESeq on clean memory (test_gpu_fused._compare);
  (c) every guard byte is intact, no input was written, and the padding of the assays is as it was (Arena.check).

One case per branch of the chain that owns workspace vectors or fills of its own, each asserted from status / attrs to have
been taken.  The chain is driven through fused.DESeq with a _Run subclass that poisons after __init__ -- what the chain is
asked to do is what fused.DESeq asks of it, host steps between launches (betaPrior, the caller's trend) included.
"""
import numpy as np
import pytest

from deseq2_amd import _lib as L
from deseq2_amd import core, fused, simulate
from deseq2_amd.engine import DeviceEngine
from deseq2_amd.native import GeneMajor
from tests import poison
from tests.poison import FF, ZERO, LEFT
from tests.test_gpu_fused import _compare, _smooth_trend, _spike_outliers

pytestmark = pytest.mark.gpu

REAL_RUN = fused._Run
BUFFERS = ("workspace", "blob", "mu_hat", "mu", "H", "cooks", "replaceCounts")     # what the chain is handed dirty
ASSAYS = ("mu_hat", "mu", "H", "cooks", "replaceCounts")
DEVICE_INPUTS = ("x", "q", "a", "r", "disp_grid", "nf", "force_zero", "x_prior", "x_red", "q_red", "a_red", "r_red")   # beside y / weights_*
OPTIM_ROW = np.array([0, 0, 0, 0, 0, 1000, 1000, 0, 0, 0, 0, 0, 0, 0, 0, 2])    # tests/testthat/test_optim.R:30-39


@pytest.fixture(scope="module")
def E():
    return DeviceEngine("cuda:0")


# ---- the cases: data(v) builds the analysis (v = 0) or the other analysis of the same shape and options (v = 1) -------
def _counts(n, x, v, seed, n0=None, **kw):
    """the analysis' counts by the suite's generator; the other analysis: another seed, the same number of rows"""
    if v == 0:
        return simulate.make_counts(n, x, seed=seed, **kw)
    return simulate.make_counts(n0, x, seed=seed + 1000, drop_all_zero=False, **{k: w for k, w in kw.items() if k != "drop_all_zero"})


def _wald_outliers(v, n0=None):
    x = simulate.design_batch_condition(48)                 # cells of 8 >= 7: replaceOutliers + refit
    d = _counts(300, x, v, 3, n0, size_factors=np.exp(np.random.default_rng(1 + v).normal(0, .2, 48)))
    return dict(counts=_spike_outliers(d["counts"], np.random.default_rng(5 + v)), x=x, sf=d["size_factors"])


def _two_group(v, n0=None):
    x = simulate.design_two_group(10)                       # groups == columns: linear mu; cells of 5: no replacement
    d = _counts(300, x, v, 4, n0)
    return dict(counts=d["counts"], x=x, sf=d["size_factors"])


def _zero_rows_stragglers(v, n0=None):
    x = simulate.design_batch_condition(24)
    d = _counts(400, x, v, 6, n0, drop_all_zero=False)
    counts = d["counts"].copy()
    counts[5 * v::41 - 4 * v] = 0
    return dict(counts=counts, x=x, sf=d["size_factors"], kw=dict(disp_maxit=4))     # 4 line-search steps: many grid refits


def _optim_rows(v, n0=None):
    x = simulate.design_two_group(16)
    xb = np.column_stack([x, (np.arange(16) % 2).astype(float)])      # p = 3, groups != columns: GLM mu
    d = _counts(300, xb, v, 8, n0)
    counts = d["counts"].copy()
    for r in ((3, 77, 200), (9, 50, 150))[v]:
        counts[r] = OPTIM_ROW
    return dict(counts=counts, x=xb, sf=d["size_factors"], kw=dict(minReplicatesForReplace=np.inf))


def _weights(v, n0=None):
    x = simulate.design_batch_condition(42)                 # cells of 7
    d = _counts(300, x, v, 9, n0)
    counts = _spike_outliers(d["counts"], np.random.default_rng(6 + v), k=4)
    rng = np.random.default_rng(2 + v)
    w = rng.uniform(0.05, 1.0, counts.shape)
    w[rng.uniform(size=w.shape) < 0.02] = 0.0               # exact zeros
    w[(7, 19)[v], x[:, 3] == 1] = 0.0                       # a gene loses a whole condition: weightsFail
    return dict(counts=counts, x=x, sf=d["size_factors"], weights=w)


def _lrt_intercept(v, n0=None):
    x = simulate.design_factor(60, 5)                       # cells of 12
    d = _counts(300, x, v, 10, n0, intercept_mean=2.0)
    return dict(counts=_spike_outliers(d["counts"], np.random.default_rng(7 + v), k=5), x=x, sf=d["size_factors"],
                kw=dict(test="LRT", reduced=np.ones((60, 1))))


def _lrt_reduced2(v, n0=None):
    x = simulate.design_factor(48, 6)
    d = _counts(300, x, v, 31, n0)
    counts = _spike_outliers(d["counts"], np.random.default_rng(2 + v), k=5)
    r = (9, 23)[v]
    counts[r] = 0
    counts[r, 28:30] = 3000                                 # a row for the optim fallback of both fits
    red = np.column_stack([np.ones(48), (np.arange(48) >= 24).astype(float)])      # 1 < p_red = 2 < p = 6
    return dict(counts=counts, x=x, sf=d["size_factors"], kw=dict(test="LRT", reduced=red, minmu=1e-6))


def _beta_prior_expanded(v, n0=None):
    factors = {"condition": np.repeat([0, 1, 2], 8)}        # the expanded model matrix: 4 columns, rank 3
    x, _ = core.standard_model_matrix(factors)
    d = _counts(300, x, v, 44, n0)
    counts = _spike_outliers(d["counts"], np.random.default_rng(6 + v), k=5)
    r = (5, 31)[v]
    counts[r] = 0
    counts[r, -2:] = 4000                                   # a row for the optim fallback
    return dict(counts=counts, x=x, sf=d["size_factors"], kw=dict(betaPrior=True, factors=factors))


def _wide12_outliers(v, n0=None):
    x = simulate.design_factor(96, 12)                      # p = 12 on the 16-column build (pk > p); cells of 8: refit
    d = _counts(200, x, v, 33, n0)
    return dict(counts=_spike_outliers(d["counts"], np.random.default_rng(12 + v), k=5), x=x, sf=d["size_factors"])


def _wide17_weights_lrt(v, n0=None):
    """wide17_outliers_optim of tests/test_gpu_deseq_host.py (p = 17 on the 24-column build, cells of 8, an optim row) with
    observation weights, as an LRT against the first 12 columns: the reduced fit at a padded width of its own (16 > 12)"""
    if v == 0:
        from tests.test_gpu_deseq_host import CASES
        counts, x, sf, _ = CASES["wide17_outliers_optim"]
    else:
        x = simulate.design_factor(136, 17)
        d = _counts(260, x, v, 32, n0)
        counts, sf = _spike_outliers(d["counts"], np.random.default_rng(34), k=5), d["size_factors"]
        counts[11] = 0
        counts[11, 70:72] = 3000
    w = np.random.default_rng(40 + v).uniform(0.2, 1.0, counts.shape)
    return dict(counts=counts, x=x, sf=sf, weights=w, kw=dict(test="LRT", reduced=np.ascontiguousarray(x[:, :12])))


def _callers_trend_refit(v, n0=None):
    x = simulate.design_two_group(16)                       # cells of 8: DSQ_PH_OUTLIERS_DETECT / _REFIT in two calls
    d = _counts(300, x, v, 42, n0)
    return dict(counts=_spike_outliers(d["counts"], np.random.default_rng(8 + v), k=6), x=x, sf=d["size_factors"],
                kw=dict(fitType=_smooth_trend))


def _nf_matrix(v, n0=None):
    x = simulate.design_batch_condition(48)
    d = _counts(300, x, v, 3, n0, drop_all_zero=False)
    counts = _spike_outliers(d["counts"], np.random.default_rng(8 + v))
    counts[3 * v::41 + 2 * v] = 0         # all-zero rows: the chain averages the factors over the OTHER rows (xim)
    nf = np.exp(np.random.default_rng(21 + v).normal(0, 0.2, counts.shape))
    return dict(counts=counts, x=x, sf=None, nf=nf)


def _fit_mean(v, n0=None):
    x = simulate.design_two_group(12)
    d = _counts(300, x, v, 31, n0)
    return dict(counts=d["counts"], x=x, sf=d["size_factors"], kw=dict(fitType="mean"))


def _trend_fails(v, n0=None):
    x = simulate.design_two_group(12)                       # the parametric trend does not fit: the mean, on the device
    return dict(counts=simulate.make_counts_trend_fails(400, x, seed=5 + v), x=x, sf=np.ones(12))


def _sixteen_workgroups(v, n0=None):
    x = simulate.design_two_group(8)                        # 16 384 genes: the smallest analysis on prior_var_kernel<16>
    d = simulate.make_counts(16384, x, seed=62 + 1000 * v, drop_all_zero=False)
    counts = d["counts"].copy()
    counts[v::29 + 2 * v] = 0
    return dict(counts=counts, x=x, sf=d["size_factors"])


def _taken(**at_least):
    def check(b):
        st = b.attrs["status"]
        for k, lo in at_least.items():
            assert sum(st[q] for q in k.split("__")) >= lo, (k, st)
    return check


def _ws(run, p):
    return int(L.lib().dsq_deseq_workspace_bytes(run.n, run.m, p, 0))


def _linear_mu(b):
    a = b._fused_run.args
    assert a.linearMu == 1 and a.do_replace == 0 and "replace" not in b.mcols


def _padded(p_red=None):
    """a wide design on a zero-padded build (include/deseq2_mi355x.h, DSQ_MAX_P: 11..64 columns on 16, 24, 32, 48 or 64): the
    library sizes the workspace by the padded width, so p columns cost what the build's width costs -- and more than 10"""
    def check(b):
        run = b._fused_run
        wide = min(w for w in (16, 24, 32, 48, 64) if w >= run.p)
        assert run.p < wide and _ws(run, run.p) == _ws(run, wide) > _ws(run, 10), (run.p, wide)
        if p_red is not None:
            wr = min(w for w in (16, 24, 32, 48, 64) if w >= p_red)
            assert run.args.p_red == p_red < wr and run.args.x_red and _ws(run, p_red) == _ws(run, wr) > _ws(run, 10)
            assert run.args.useWeights == 1
        _taken(N_REFIT=1)(b)
    return check


def _nf_is_matrix(b):
    a = b._fused_run.args
    assert a.nf_is_vector == 0 and a.nf == b.nf.t.data_ptr()
    _taken(N_REFIT=1)(b)


def _weights_fail(b):
    assert b.mcols["weightsFail"][7] and np.isnan(b.mcols["dispersion"][7])


def _is_mean(b):
    assert b.dispersionFunction["fitType"] == "mean"


def _is_prior(b):
    assert b.attrs["betaPrior"] and b.mcols["beta"].shape[1] == 4 and b.mcols["MLE_beta"].shape[1] == 3
    _taken(N_REFIT=1)(b)


def _is_custom(b):
    assert b.dispersionFunction["fitType"] == "custom"
    _taken(N_REFIT=1)(b)


def _is_large(b):
    # the sixteen-workgroup prior variance and its selection workspace are taken from 16 384 trend values (csrc/trend.hip,
    # prior_var_blocks); the trend runs over this call's own genes when no gathered vectors are given
    a, st = b._fused_run.args, b.attrs["status"]
    assert a.n >= 16384 and not a.trend_mean and a.n_trend == 0 and st["N_TREND"] > 0 and st["TREND_STATUS"] == 0
    assert int(np.asarray(b.mcols["allZero"], bool).sum()) > 500


CASES = {
    "1_wald_batch_condition_outliers": (_wald_outliers, _taken(N_REPLACE=3, N_REFIT=3)),
    "2_two_group_linear_mu": (_two_group, _linear_mu),
    "3_zero_rows_and_grid_stragglers": (_zero_rows_stragglers, _taken(N_GRID_GENEEST=11, N_GRID_MAP=11)),
    "4_optim_fallback_rows": (_optim_rows, _taken(N_OPTIM_GENEEST__N_OPTIM_TEST=1)),
    "5_weights_zero_and_failing": (_weights, _weights_fail),
    "6_lrt_intercept": (_lrt_intercept, _taken(N_REFIT=1)),
    "6_lrt_reduced_matrix": (_lrt_reduced2, _taken(N_REFIT=1)),
    "7_beta_prior_expanded": (_beta_prior_expanded, _is_prior),
    "8_wide12_outliers": (_wide12_outliers, _padded()),
    "8_wide17_weights_lrt_reduced12": (_wide17_weights_lrt, _padded(p_red=12)),
    "9_callers_trend_two_outlier_calls": (_callers_trend_refit, _is_custom),
    "10_normalization_factor_matrix": (_nf_matrix, _nf_is_matrix),
    "11_fit_type_mean": (_fit_mean, _is_mean),
    "11_trend_fails_mean_substituted": (_trend_fails, _is_mean),
    "12_sixteen_workgroup_prior_variance": (_sixteen_workgroups, _is_large),
}


# ---- one run of the chain on poisoned memory --------------------------------------------------------------------------
def _bytes(t, x):
    return x.reshape(-1).view(t.uint8)


def _poisoned_run(arena, state, donor, runs):
    class Run(REAL_RUN):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            t, m = self.t, self.m
            neg = self.negflag[:1].clone() if self.neg is not None else None
            for k in BUFFERS:
                flat = _bytes(t, getattr(self, k))
                if state == LEFT:
                    assert flat.numel() == donor[k].numel(), "the other analysis has another shape: " + k
                    flat.copy_(donor[k])
                else:
                    flat.fill_(poison.BYTE[state])
            if neg is not None:
                self.negflag[:1] = neg         # (set by __init__ from weights_prep: an input of the chain, not its output)
            if self.useWeights:               # the library's own normalised weights are inputs of the chain as well
                for k in ("w_norm", "w_floor"):
                    h = getattr(self, k)
                    c = GeneMajor(arena.empty(h.t.shape, h.t.dtype, 0, k), h.m)
                    c.t.copy_(h.t)
                    poison.poison_padding(c, float("nan"))
                    arena.unchanged(c.t, "input " + k)
                    setattr(self, k, c)
                self.args.weights_norm, self.args.weights_floor = self.w_norm.t.data_ptr(), self.w_floor.t.data_ptr()
            for k in ASSAYS:
                arena.padding(GeneMajor(getattr(self, k), m), k)
            # the design-side device inputs (the engine's cached tensors): arena copies, watched, in their place
            dds = a[0]
            have = [dds.xh, self.grid, getattr(self, "sf_dev", None), self.force_zero, dds.nf.t] + list(self.keep)
            self.arena_inputs = {}
            for f in DEVICE_INPUTS:
                ptr = getattr(self.args, f)
                if not ptr:
                    continue
                src = [v for v in have if v is not None and v.data_ptr() == ptr]
                assert src, "no tensor behind DsqDeseqArgs." + f
                if arena.owns(src[0]):
                    c = src[0]
                    arena.unchanged(c, "input " + f)
                else:
                    c = arena.empty(src[0].shape, src[0].dtype, 0, f)
                    c.copy_(src[0])
                    arena.unchanged(c, "input " + f)
                    setattr(self.args, f, c.data_ptr())
                self.arena_inputs[f] = c
            runs.append(self)

        def launch(self, phases, trend=None):
            # the caller's trend values (dispFit_in), which the caller rewrites between two launches: from the arena, and
            # unwritten by each launch
            t = self.t
            fit = getattr(self, "_fit_in", None)
            if fit is not None and not arena.owns(fit):
                c = arena.empty(fit.shape, fit.dtype, 0, "dispFit_in")
                c.copy_(fit)
                fit = self._fit_in = c
                self.args.dispFit_in = c.data_ptr()
            before = None if fit is None else fit.clone()
            super().launch(phases, trend)
            if fit is not None:
                t.cuda.synchronize()
                assert self.args.dispFit_in == fit.data_ptr() and t.equal(fit.view(t.int64), before.view(t.int64)), \
                    "dispFit_in was written by the launch of phases %d" % phases
    return Run


def _dataset(E, arena, d):
    dds = core.DESeqDataSet(d["counts"], d["x"], sizeFactors=d.get("sf"), normalizationFactors=d.get("nf"),
                            weights=d.get("weights"), engine=E)
    if arena is None:
        return dds
    # the same matrices at ld = round8(m) + 8 with garbage in the padding columns
    nf = d["nf"] if d.get("nf") is not None else np.broadcast_to(dds.sizeFactors[None, :], d["counts"].shape)
    dds.y = arena.gene_major(dds.counts_host, -7, "counts")
    dds.nf = arena.gene_major(np.asarray(nf, np.float64), float("nan"), "nf")
    if d.get("weights") is not None:
        dds.weights_h = arena.gene_major(np.asarray(d["weights"], np.float64), float("nan"), "weights")
    return dds


def _run(E, monkeypatch, d, state, donor=None, nbytes=256 << 20):
    """fused.DESeq on poisoned memory: (dataset, run, arena)"""
    t = E.torch
    arena = poison.Arena.on_device(nbytes, E.device)
    dds = _dataset(E, arena, d)
    kw = d.get("kw", {})
    assert fused.supported(dds, **kw)
    runs = []
    with monkeypatch.context() as mp:
        mp.setattr(fused, "_Run", _poisoned_run(arena, state, donor, runs))
        # (LEFT: the chain's buffers get the other analysis' bytes in Run.__init__; whatever else is allocated: 0xFF)
        with arena.standing_in(mp, poison.BYTE.get(state, 0xFF)):
            fused.DESeq(dds, **kw)
    t.cuda.synchronize()
    assert dds.attrs.get("fused") and len(runs) == 1
    run = runs[0]
    assert run.workspace.numel() == int(L.lib().dsq_deseq_workspace_bytes(run.n, run.m, max(run.p, run._pcol), 0))
    lo, hi = arena.addr, arena.addr + arena.size
    for k in BUFFERS:
        assert lo + poison.MARGIN <= getattr(run, k).data_ptr() < hi - poison.MARGIN, k + " is not from the arena"
    for f in ("y", "weights_raw", "weights_norm", "weights_floor", "dispFit_in") + DEVICE_INPUTS:    # every device input
        ptr = getattr(run.args, f)
        assert not ptr or lo + poison.MARGIN <= ptr < hi - poison.MARGIN, "DsqDeseqArgs.%s is not from the arena" % f
    return dds, run, arena


def _left_by(t, run):
    return {k: _bytes(t, getattr(run, k)).clone() for k in BUFFERS}


def _defined(run):
    """every defined element of every output of dsq_deseq_dev, on the host.  Left out -- and nothing else:
      * the spare scalars behind DSQ_SC_FIT_USED: include/deseq2_mi355x.h, DsqDeseqOut "scalars: DSQ_SC_COEF0 ..
        DSQ_SC_FIT_USED are written, the spare entries behind them are not" (tests/test_gpu_fused.py:356-358);
      * mu_hat rows of all-zero genes: DsqDeseqOut "mu_hat: rows of all-zero genes are left as they were"
        (tests/test_gpu_fused.py:366-367);
      * replaceCounts rows with replace == 0: DsqDeseqOut "replaceCounts: only the rows with replace != 0 are written"
        (tests/test_gpu_fused.py:368);
      * the padding columns m .. ld-1 of the assays: DsqDeseqOut "padding columns are not written" (checked by Arena.check)."""
    t, m = run.t, run.m
    out = {k: getattr(run, k) for k in ("baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "betaIter",
                                        "logLike", "logLikeReduced", "maxCooks", "allZero", "dispGeneIter", "dispIter", "dispOutlier",
                                        "betaConv", "replace", "optim_geneest", "optim_test", "status")}
    if run.test != "LRT":          # DsqDeseqOut: "every per-gene column (logLikeReduced under the Wald test too: NA)"
        assert bool(t.isnan(run.logLikeReduced).all()), "logLikeReduced under the Wald test is not NA in every row"
    for i, k in enumerate(("beta", "betaSE", "stat", "pvalue")[: run._nmat]):
        out[k] = run.mat[i]
    if run.mle is not None:
        out["mle_beta"] = run.mle
    out["scalars"] = run.scalars[: L.DSQ_SC_FIT_USED + 1]
    for k in ("mu", "H", "cooks"):                           # in full: NA in the all-zero rows
        out[k] = getattr(run, k)[:, :m]
    out["mu_hat"] = run.mu_hat[run.allZero == 0][:, :m]
    out["replaceCounts"] = run.replaceCounts[run.replace != 0][:, :m]
    return {k: v.contiguous().cpu().numpy() for k, v in out.items()}


def _same_bits(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape, "%s: %s has shape %s vs %s" % (what, k, a[k].shape, b[k].shape)
        ua, ub = a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)
        if not (ua == ub).all():
            item = a[k].dtype.itemsize
            bad = np.unique(np.flatnonzero(ua != ub) // item)
            i = int(bad[0])
            raise AssertionError("%s: output %s differs in %d of %d elements, the first at flat index %d: %r vs %r"
                                 % (what, k, bad.size, a[k].size, i, a[k].reshape(-1)[i], b[k].reshape(-1)[i]))


@pytest.mark.parametrize("case", list(CASES))
def test_chain_on_poisoned_memory(E, monkeypatch, case):
    build, taken = CASES[case]
    t = E.torch
    d = build(0)
    n = d["counts"].shape[0]
    large = n >= 16384
    if large:
        # the library's cached slabs (capi_ws_get) dirty as well: a differently shaped analysis on the same stream first
        fused.DESeq(_dataset(E, None, _weights(1, 300)))
    # the other analysis of the same shape and options, on the same kind of memory; what it left behind
    other = build(1, n)
    assert other["counts"].shape == d["counts"].shape and not (other["counts"] == d["counts"]).all()
    _, orun, oarena = _run(E, monkeypatch, other, FF)
    oarena.check()
    donor = _left_by(t, orun)
    del orun, oarena
    # (b)'s reference: the call-by-call chain on clean memory
    ref = _dataset(E, None, d)
    core.DESeq(ref, **d.get("kw", {}))
    got = {}
    for state in ((FF, LEFT) if large else (FF, ZERO, LEFT)):
        b, run, arena = _run(E, monkeypatch, d, state, donor)
        taken(b)
        _compare(ref, b, "%s, prefill %s" % (case, state))                       # (b)
        arena.check()                                                            # (c)
        got[state] = _defined(run)
        del b, run, arena
    for state in got:                                                            # (a)
        if state != FF:
            _same_bits(got[FF], got[state], "%s: prefill %s against %s" % (case, FF, state))
