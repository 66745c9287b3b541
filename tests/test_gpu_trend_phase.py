"""-m gpu: the trend phase of the DESeq() chain (DSQ_PH_TREND, csrc/trend.hip) driven ALONE on vectors the test makes, at the
smallest shapes at which its exact selection can go wrong: odd and even counts, the upper middle as a tie and as a
distinct value, every radix pass without the direct-ranking exit, the exit at exactly 1024 candidates, residuals of both
signs, entries below the threshold among the kept ones, and the sizes on either side of the one-workgroup / sixteen-
workgroup rule (16 384 values).  The reference is numpy's sort on residuals taken with the engine's own logarithm, so
every comparison is `==` on the bits."""
import numpy as np
import pytest

from deseq2_amd import _lib as L
from deseq2_amd import core, fused, native, simulate
from deseq2_amd.engine import DeviceEngine

pytestmark = pytest.mark.gpu

SC_COEF0, SC_COEF1, SC_VAR_LOG_DISP, SC_DISP_PRIOR_VAR, SC_FIT_USED = (L.DSQ_SC_COEF0, L.DSQ_SC_COEF1, L.DSQ_SC_VAR_LOG_DISP,
                                                                        L.DSQ_SC_DISP_PRIOR_VAR, L.DSQ_SC_FIT_USED)
MIN_DISP = 1e-8


@pytest.fixture(scope="module")
def E():
    return DeviceEngine("cuda:0")


@pytest.fixture(scope="module")
def dds(E):
    x = simulate.design_two_group(12)                       # m - p = 10 > 3: the trigamma form of the prior variance
    d = simulate.make_counts(4, x, seed=3, drop_all_zero=False)
    return core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=E)


def _trend(E, dds, means, disps, given=None, fitType="parametric", run=None):
    """DSQ_PH_TREND alone over (means, disps); given: the caller's trend values (dispFit_in + trend_fit_in).
    -> (status, scalars, run)"""
    n_trend = int(np.size(disps))
    if run is None:
        run = fused._Run(dds, "Wald", 7, n_trend, {})
    run.args.fitType = L.DSQ_FIT[fitType]
    keep = [E._vec(means), E._vec(disps)]
    if given is not None:
        keep += [E._vec(np.ones(dds.n)), E._vec(given)]
        run.args.dispFit_in, run.args.trend_fit_in = fused._ptr(keep[2]), fused._ptr(keep[3])
    else:
        run.args.dispFit_in, run.args.trend_fit_in = None, None
    run.launch(L.DSQ_PH_TREND, trend=(keep[0], keep[1]))
    st, sc = run.read_status()
    return st, np.array(sc), run


def _residuals(disps, fit):
    kept = disps >= MIN_DISP * 100.0
    return native.unary("log", disps[kept]) - native.unary("log", fit[kept])


def _median(s):
    k = s.size
    s = np.sort(s)
    return (s[(k - 1) // 2] + s[k // 2]) * 0.5


def _check_prior_var(st, sc, r, expVarLogDisp, what):
    k = int(r.size)
    assert st["N_ABOVE_MIN"] == k, what
    if k == 0:
        assert np.isnan(sc[SC_VAR_LOG_DISP]) and np.isnan(sc[SC_DISP_PRIOR_VAR]), what
        return
    med = _median(r)
    mad = 1.4826 * _median(np.abs(r - med))
    v = mad * mad                                           # (1.4826 med2) ** 2 as the IEEE product
    pv = max(v - expVarLogDisp, 0.25)
    print("%s: k=%d med=%r varLogDispEsts=%r (device %r) dispPriorVar=%r (device %r)"
          % (what, k, med, v, sc[SC_VAR_LOG_DISP], pv, sc[SC_DISP_PRIOR_VAR]))
    assert sc[SC_VAR_LOG_DISP] == v, what
    assert sc[SC_DISP_PRIOR_VAR] == pv, what


def _given(E, dds, disps, fit, what, run=None):
    """the caller's-trend form: the residuals are log(disps) - log(fit), independent of any fit"""
    means = np.full(disps.size, 100.0)
    st, sc, run = _trend(E, dds, means, disps, given=fit, run=run)
    assert st["TREND_STATUS"] == 0 and sc[SC_FIT_USED] == L.DSQ_FIT["given"], what
    assert np.isnan(sc[SC_COEF0]) and np.isnan(sc[SC_COEF1]), what
    r = _residuals(disps, fit)
    _check_prior_var(st, sc, r, run.args.expVarLogDisp, what)
    return r, run


def _parametric(E, dds, n, seed, below=0, run=None):
    """a Gamma-scattered trend the parametric fit converges on; `below` entries under the threshold scattered among them"""
    rng = np.random.default_rng(seed)
    means = np.exp(rng.uniform(np.log(5.0), np.log(5000.0), n))
    disps = (0.05 + 2.0 / means) * np.exp(0.6 * rng.standard_normal(n))
    if below:
        disps[rng.choice(n, below, replace=False)] = MIN_DISP
    what = "parametric, n_trend = %d, %d below the threshold" % (n, below)
    st, sc, run = _trend(E, dds, means, disps, run=run)
    assert st["TREND_STATUS"] == 0 and sc[SC_FIT_USED] == L.DSQ_FIT["parametric"], what
    assert st["N_TREND"] == n - below, what
    fit = sc[SC_COEF0] + sc[SC_COEF1] / means
    r = _residuals(disps, fit)
    _check_prior_var(st, sc, r, run.args.expVarLogDisp, what)
    return r


def _left_after_passes(r, n, rank):
    """numpy mirror of the selection's bookkeeping: the candidates left after each radix pass (digits of 11, 11, 11, 11, 11,
    9 bits of the order-preserving key) for the rank-th smallest of the residuals `r` and n - len(r) entries of +inf"""
    v = np.concatenate([r, np.full(n - r.size, np.inf)])
    u = v.view(np.uint64)
    keys = np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))
    left, shift = [], 64
    while shift > 0:
        bits = 11 if shift >= 20 else shift
        shift -= bits
        dig = (keys >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
        d = np.sort(dig)[rank]
        rank -= int((dig < d).sum())
        keys = keys[dig == d]
        left.append(int(keys.size))
    return left


# ---- one workgroup (fewer than 16 384 values) ------------------------------------------------------------------------
@pytest.mark.parametrize("disps", [
    [0.3], [0.3, 0.3], [0.3, 0.7], [0.3, 0.7, 0.1],
    [0.3, 0.7, 0.7, 2.0],             # even count, the upper middle a tie
    [0.3, 0.7, 0.9, 2.0],             # ... a distinct value
    [0.5, 0.5, 0.5, 0.5],
], ids=lambda v: "-".join("%g" % x for x in v))
def test_tiny_counts_odd_even_tie_and_distinct_upper_middle(E, dds, disps):
    disps = np.array(disps)
    _given(E, dds, disps, np.full(disps.size, 0.4), "n_trend = %d" % disps.size)


def test_no_entry_above_the_threshold(E, dds):
    r, _ = _given(E, dds, np.full(7, MIN_DISP), np.full(7, 0.4), "none above")
    assert r.size == 0


def test_identical_residuals_run_every_pass(E, dds):
    """1500 equal residuals: the candidates never drop to 1024, so all six passes run and the result is the prefix"""
    r, _ = _given(E, dds, np.full(1500, 0.3), np.full(1500, 0.4), "1500 identical")
    assert min(_left_after_passes(r, 1500, (1500 - 1) // 2)) == 1500


def _ties_at_the_median(rng, n, ties):
    """n values, `ties` of them equal and across the median, the rest distinct on either side"""
    lo = (n - ties) // 2
    disps = np.concatenate([rng.uniform(0.01, 0.2, lo), np.full(ties, 0.3), rng.uniform(0.5, 4.0, n - ties - lo)])
    return rng.permutation(disps)


def test_more_than_1024_ties_at_the_median_and_exactly_1024_candidates(E, dds):
    rng = np.random.default_rng(11)
    disps = _ties_at_the_median(rng, 3000, 1025)
    r, _ = _given(E, dds, disps, np.full(3000, 0.4), "3000, 1025 equal at the median")
    assert min(_left_after_passes(r, 3000, (3000 - 1) // 2)) == 1025           # never ranked directly
    # the first pass (sign and the ten high exponent bits: one bin is [0.5, 2)) leaves exactly 1024: the direct exit's edge
    res = np.concatenate([rng.uniform(0.13, 0.49, 988), rng.uniform(0.51, 1.9, 1024), rng.uniform(2.1, 7.9, 988)])
    disps = rng.permutation(np.exp(res))
    r, _ = _given(E, dds, disps, np.ones(3000), "3000, 1024 candidates after the first pass")
    assert _left_after_passes(r, 3000, (3000 - 1) // 2)[0] == 1024


def test_both_signs_zeros_and_entries_below_the_threshold(E, dds):
    rng = np.random.default_rng(12)
    fit = np.exp(rng.uniform(np.log(0.05), np.log(2.0), 2001))
    disps = fit * np.exp(rng.standard_normal(2001))
    disps[rng.choice(2001, 300, replace=False)] = MIN_DISP                     # +inf in the selection: they sort last
    zero = rng.choice(np.flatnonzero(disps > MIN_DISP), 40, replace=False)
    disps[zero] = fit[zero]                                                    # exact zeros
    r, _ = _given(E, dds, disps, fit, "both signs")
    assert (r < 0).sum() > 500 and (r > 0).sum() > 500 and (r == 0).sum() == 40 and r.size == 1701
    _parametric(E, dds, 3001, seed=13, below=500)


def test_largest_input_on_one_workgroup(E, dds):
    _parametric(E, dds, 16383, seed=14)


# ---- sixteen workgroups (from 16 384 values) --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16384, 16385])
def test_threshold_of_the_sixteen_workgroup_path(E, dds, n):
    _parametric(E, dds, n, seed=15)                         # (an even and an odd count)


def test_sixteen_workgroups_identical_residuals(E, dds):
    """no early exit, and the upper middle of the even count is a tie found across workgroups"""
    r, _ = _given(E, dds, np.full(16384, 0.3), np.full(16384, 0.4), "16384 identical")
    assert min(_left_after_passes(r, 16384, (16384 - 1) // 2)) == 16384


def test_sixteen_workgroups_more_than_1024_ties_at_the_median(E, dds):
    disps = _ties_at_the_median(np.random.default_rng(16), 20000, 1025)
    r, _ = _given(E, dds, disps, np.full(20000, 0.4), "20000, 1025 equal at the median")
    assert min(_left_after_passes(r, 20000, (20000 - 1) // 2)) == 1025


def test_sixteen_workgroups_none_above_then_an_ordinary_call(E, dds):
    """every workgroup leaves at the first barrier; the next call on the same buffers finds the barrier words in order"""
    r, run = _given(E, dds, np.full(16384, MIN_DISP), np.full(16384, 0.4), "16384, none above")
    assert r.size == 0
    _parametric(E, dds, 16384, seed=17, run=run)


# ---- fitType = "mean": the two cut points of the trimmed mean by the same selection -----------------------------------
def _mean_case(E, dds, disps, what):
    means = np.full(disps.size, 100.0)
    st, sc, run = _trend(E, dds, means, disps, fitType="mean")
    ref = core.trimmed_mean_fit(disps, MIN_DISP)
    print("%s: trimmed mean %r (device %r)" % (what, ref, sc[SC_COEF0]))
    assert st["TREND_STATUS"] == 0 and sc[SC_FIT_USED] == L.DSQ_FIT["mean"], what
    assert sc[SC_COEF0] == ref and sc[SC_COEF1] == 0.0, what
    _check_prior_var(st, sc, _residuals(disps, np.full(disps.size, ref)), run.args.expVarLogDisp, what)


@pytest.mark.parametrize("N", [999, 1000])
def test_trimmed_mean_cut_ranks(E, dds, N):
    """N = 999: k = floor(N / 1000) = 0, the extremes themselves; N = 1000: k = 1"""
    rng = np.random.default_rng(N)
    disps = np.concatenate([np.exp(rng.uniform(np.log(1e-3), np.log(5.0), N)), np.full(37, MIN_DISP)])
    _mean_case(E, dds, rng.permutation(disps), "mean, N = %d" % N)


def test_trimmed_mean_ties_at_both_cut_points(E, dds):
    rng = np.random.default_rng(18)
    disps = np.concatenate([np.full(5, 2e-3), np.exp(rng.uniform(np.log(1e-2), np.log(2.0), 2489)), np.full(6, 4.0)])
    assert np.floor(disps.size * 0.001) == 2                 # ranks 2 and N - 3 lie inside the runs of equal values
    _mean_case(E, dds, rng.permutation(disps), "mean, N = 2500, ties at both cut points")
