"""-m gpu: the head of the DESeq() chain -- the moments kernel in front of the first fit (csrc/aux.hip: prefit_kernel,
which takes the quotient y / nf once per sample and keeps it for its second sweep) and the ordered compactions on many
workgroups (csrc/pipeline.hip: compact_count_kernel / compact_write_kernel) -- at the small shapes where they can go
wrong.

Moments: native.prefitMoments == oracle.prefitMoments on the bits, at row lengths around every bound of the kernel (one
wave trip: 64; the quotient in registers: up to 512 samples; in a wave-private LDS slice: up to 1024; the four-sweep code
beyond, as at every design of more than 10 columns), on the tiled build for long rows (m p >= 8192) with a ragged last
tile, with and without weights, the size factors as a vector and as a matrix, gene counts that leave idle waves in the
last block, all-zero rows first, last and inside.

Compactions: seen through what depends on the ORDER of their lists -- the parametric trend fit sums its input in index
order, and the fits run on the listed non-zero rows --, at gene counts on either side of the tile boundaries (1024
elements per workgroup) and with several tiles in front of a workgroup, with nothing, the ends, a whole tile and all
but one element dropped."""
import numpy as np
import pytest

from deseq2_amd import _lib as L
from deseq2_amd import core, native, simulate
from deseq2_amd.engine import DeviceEngine
from tests import test_gpu_fused as chain
from tests import test_gpu_trend_phase as trend
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

TILE = 1024                    # kCompactTile
KEYS = ("baseMean", "baseVar", "allZero", "roughDisp", "beta_init")


@pytest.fixture(scope="module")
def E():
    return DeviceEngine("cuda:0")


# ---- the moments kernel ---------------------------------------------------------------------------------------------
def _prefit_case(n, m, p, seed):
    rng = np.random.default_rng(seed)
    x = np.column_stack([np.ones(m)] + [rng.normal(0.0, 1.0, m) for _ in range(p - 1)])
    sf = np.exp(rng.normal(0.0, 0.25, m))
    lam = np.exp(rng.normal(3.0, 1.5, n))[:, None] * sf[None, :]
    counts = rng.poisson(lam).astype(np.int32)
    counts[rng.uniform(size=counts.shape) < 0.1] = 0
    counts[:, 0] = np.maximum(counts[:, 0], 1)       # (no all-zero row by chance)
    if n >= 3:
        counts[0] = 0; counts[n // 2] = 0; counts[n - 1] = 0
    w = rng.uniform(0.05, 1.0, (n, m))
    w[rng.uniform(size=(n, m)) < 0.02] = 0.0
    w = w / w.max(axis=1, keepdims=True)
    nfm = np.exp(rng.normal(0.0, 0.1, (n, m))) * sf[None, :]
    return dict(counts=counts, x=x, sf=sf, nfm=nfm, w=w)


def _prefit_dev(E, c, useW):
    """the size factors as an m-vector (nf_is_vector): the resident entry point"""
    import torch
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64).T), device="cuda:0")   # noqa: E731
    host = lambda t: t.cpu().numpy()                                                                       # noqa: E731
    q, a, r = (dev(z) for z in native.design_qr(c["x"]))
    o = native.prefitMoments_dev(E.counts(c["counts"]), torch.as_tensor(c["sf"], device="cuda:0"), q, a, r,
                                 E.matrix(c["w"]) if useW else None, useW, nf_is_vector=True)
    return {"baseMean": host(o["baseMean"]), "baseVar": host(o["baseVar"]), "roughDisp": host(o["roughDisp"]),
            "allZero": host(o["allZero"]) != 0, "beta_init": host(o["beta_init"]).T}


# (m, p): the bounds of the kernel and their neighbours
SHAPES = [(2, 1), (63, 2), (64, 4), (65, 4), (65, 10),
          (511, 4), (512, 4), (513, 4), (512, 10), (513, 2),          # registers | LDS slice
          (1023, 4), (1024, 4), (1025, 4), (1024, 2), (1025, 2),      # LDS slice | four sweeps
          (820, 10), (1024, 10), (1025, 10),                          # tiled (m p = 8200: just over 8192; 820 = 3 x 256 + 52)
          (482, 17), (700, 20), (600, 24)]                            # wide designs (p > 10), tiled: the four-sweep code


@pytest.mark.parametrize("nf_vector", [False, True], ids=["nf_matrix", "sf_vector"])
@pytest.mark.parametrize("useW", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("m,p", SHAPES, ids=lambda v: str(v))
def test_prefit_moments_at_the_bounds_of_the_kept_quotient(E, oracle, m, p, useW, nf_vector):
    c = _prefit_case(41, m, p, seed=100 * m + p)
    nf = np.broadcast_to(c["sf"][None, :], c["counts"].shape).copy() if nf_vector else c["nfm"]
    with np.errstate(all="ignore"):
        want = oracle.prefitMoments(c["counts"], nf, c["x"], c["w"], useW)
    got = _prefit_dev(E, c, useW) if nf_vector else native.prefitMoments(c["counts"], nf, c["x"], c["w"], useW)
    assert want["allZero"][[0, 20, 40]].all() and want["allZero"].sum() == 3
    for k in KEYS:
        assert_same(got[k], want[k], "prefitMoments m=%d p=%d$%s" % (m, p, k))


def test_prefit_moments_rejects_a_row_of_one_sample(E):
    """m = 1 never reaches the kernel (the variance divides by m - 1, the design needs m > p): the entry point's argument
    check turns it away, so the shortest row of the cases above is m = 2"""
    c = _prefit_case(5, 1, 1, seed=1)
    with pytest.raises(Exception):
        native.prefitMoments(c["counts"], c["nfm"], c["x"], c["w"], False)


@pytest.mark.parametrize("n", [1, 5, 61])
@pytest.mark.parametrize("m,p", [(512, 4), (1024, 4), (820, 10), (1025, 10)], ids=lambda v: str(v))
def test_prefit_moments_idle_waves_in_the_last_block(E, oracle, n, m, p):
    c = _prefit_case(n, m, p, seed=7 * m + n)
    for useW in (False, True):
        want = oracle.prefitMoments(c["counts"], c["nfm"], c["x"], c["w"], useW)
        got = native.prefitMoments(c["counts"], c["nfm"], c["x"], c["w"], useW)
        for k in KEYS:
            assert_same(got[k], want[k], "prefitMoments n=%d m=%d p=%d weights=%s$%s" % (n, m, p, useW, k))
    assert want["allZero"].sum() == (3 if n >= 3 else 0)


# ---- mode 1: the trend's (mean, disp) pairs -------------------------------------------------------------------------
THRESH = 100.0 * trend.MIN_DISP


@pytest.fixture(scope="module")
def dds(E):
    x = simulate.design_two_group(12)
    d = simulate.make_counts(4, x, seed=3, drop_all_zero=False)
    return core.DESeqDataSet(d["counts"], x, sizeFactors=d["size_factors"], engine=E)


def _trend_vectors(n, seed):
    rng = np.random.default_rng(seed)
    means = np.exp(rng.uniform(np.log(5.0), np.log(5000.0), n))
    disps = (0.05 + 2.0 / means) * np.exp(0.6 * rng.standard_normal(n))
    return means, disps


def _drop(disps, pattern):
    """dispersions AT the threshold (kept is `>`) and below it"""
    d = disps.copy()
    n = d.size
    if pattern == "ends":
        d[0] = THRESH; d[n - 1] = trend.MIN_DISP
    elif pattern == "tile":
        d[TILE:2 * TILE:2] = THRESH; d[TILE + 1:2 * TILE:2] = trend.MIN_DISP
    elif pattern == "one":
        keep = n // 2
        d[np.arange(n) % 2 == 0] = THRESH; d[np.arange(n) % 2 == 1] = trend.MIN_DISP
        d[keep] = disps[keep]
    return d


@pytest.mark.parametrize("n,pattern", [(n, "none") for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3)] +
                         [(n, "ends") for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3)] +
                         [(2 * TILE + 1, "tile"), (5 * TILE + 3, "tile")])
def test_trend_pairs_keep_their_order(E, oracle, dds, n, pattern):
    """the parametric fit sums the kept pairs in index order: its coefficients are those of the oracle's fit on the pairs
    numpy keeps, and the count is numpy's"""
    means, disps = _trend_vectors(n, seed=n)
    disps = _drop(disps, pattern)
    keep = disps > THRESH
    want = oracle.parametricDispersionFit(means[keep], disps[keep])
    st, sc, run = trend._trend(E, dds, means, disps)
    what = "n_trend = %d, dropped: %s" % (n, pattern)
    assert st["TREND_STATUS"] == 0 and sc[trend.SC_FIT_USED] == L.DSQ_FIT["parametric"], what
    assert st["N_TREND"] == int(keep.sum()), what
    assert_same(np.array([sc[trend.SC_COEF0], sc[trend.SC_COEF1]]), want, what + ": coefficients")
    fit = sc[trend.SC_COEF0] + sc[trend.SC_COEF1] / means
    trend._check_prior_var(st, sc, trend._residuals(disps, fit), run.args.expVarLogDisp, what)


@pytest.mark.parametrize("n,pattern", [(1, "none"), (1, "one"), (TILE + 1, "one"), (5 * TILE + 3, "one")])
def test_trend_pairs_one_element(E, dds, n, pattern):
    """too few pairs for a fit: the caller's trend, and the count of the kept pairs"""
    means, disps = _trend_vectors(n, seed=n + 1)
    disps = _drop(disps, pattern)
    st, sc, run = trend._trend(E, dds, means, disps, given=np.full(n, 0.4))
    what = "n_trend = %d, dropped: %s" % (n, pattern)
    assert st["N_TREND"] == int((disps > THRESH).sum()) == 1, what
    trend._check_prior_var(st, sc, trend._residuals(disps, np.full(n, 0.4)), run.args.expVarLogDisp, what)


# ---- mode 0: the list of the non-zero rows, through the whole chain -------------------------------------------------
def _chain_counts(n, pattern, seed):
    x = simulate.design_two_group(10)                       # m = 10: a case takes seconds; cells of 5: no outlier refit
    d = simulate.make_counts(n + n // 4 + 8, x, seed=seed, drop_all_zero=False)
    nonzero = np.flatnonzero(d["counts"].sum(axis=1) > 0)[:n]
    assert nonzero.size == n
    counts = d["counts"][nonzero].copy()
    if pattern == "ends":
        counts[0] = 0; counts[n - 1] = 0
    elif pattern == "tile":
        counts[TILE:2 * TILE] = 0
    elif pattern == "one":
        keep = counts[n // 2].copy()
        counts[:] = 0
        counts[n // 2] = keep
    return counts, x, d["size_factors"]


@pytest.mark.parametrize("n,pattern", [(n, "none") for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3)] +
                         [(n, "ends") for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3)] +
                         [(2 * TILE + 1, "tile"), (5 * TILE + 3, "tile")])
def test_fused_chain_lists_the_non_zero_rows_in_order(E, n, pattern):
    """every per-gene column, the NA pattern of the all-zero rows, the trend's coefficients and the prior variance of the
    fused chain == the call-by-call chain's"""
    counts, x, sf = _chain_counts(n, pattern, seed=n)
    a, b = chain._both(E, counts, x, sf)
    zero = counts.sum(axis=1) == 0
    assert b.attrs["status"]["N_NONZERO"] == int((~zero).sum())
    assert_same(np.asarray(b.mcols["allZero"], bool), zero, "allZero")
    assert_same(np.isnan(np.asarray(b.mcols["dispGeneEst"], float)), zero, "NA pattern of dispGeneEst")
    assert_same(np.isnan(np.asarray(b.mcols["dispersion"], float)), zero, "NA pattern of dispersion")
    chain._compare(a, b, "n = %d, dropped: %s" % (n, pattern))


@pytest.mark.parametrize("n,pattern", [(1, "none"), (TILE + 1, "one"), (5 * TILE + 3, "one")])
def test_fused_chain_one_non_zero_row(E, n, pattern):
    """one listed row (one gene cannot carry a parametric trend: fitType = "mean")"""
    counts, x, sf = _chain_counts(n, pattern, seed=n + 2)
    a, b = chain._both(E, counts, x, sf, fitType="mean")
    zero = counts.sum(axis=1) == 0
    assert b.attrs["status"]["N_NONZERO"] == 1
    assert_same(np.isnan(np.asarray(b.mcols["dispersion"], float)), zero, "NA pattern of dispersion")
    chain._compare(a, b, "n = %d, dropped: %s, one row listed" % (n, pattern))
