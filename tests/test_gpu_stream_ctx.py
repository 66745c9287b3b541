"""The per-(device, stream) context of the library's host side (csrc/ctx.hip): workspace slots, the pinned upload ring
and the side stream belong to one (device, stream) and are latched afresh by every entry point and every worker job.

Everything here is compared BIT FOR BIT with a plain single-range call of the same analysis:
  * the pinned ring wraps around (more than kPinRing = 8 table uploads per context) under three worker threads;
  * dsq_release_workspace() destroys the contexts between calls -- on two torch streams for the device chain, and under
    the persistent worker threads (which outlive the release) for the host entry;
  * two devices (skipped on a one-device machine): the worker of device 1 uploads its own design cells and outlier
    metadata through its own ring, on its own stream.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from deseq2_amd import _lib, core, fused, native, simulate
from deseq2_amd.engine import DeviceEngine
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

K_PIN_RING = 8          # csrc/ctx.hip

GENE_COLS = ("baseMean", "baseVar", "allZero", "dispGeneEst", "dispGeneIter", "dispFit", "dispMAP", "dispersion", "dispIter",
             "dispOutlier", "beta", "betaSE", "betaIter", "betaConv", "logLike", "maxCooks", "stat", "pvalue", "replace")
COUNTERS = ("N_NONZERO", "N_REPLACE", "N_REFIT", "N_OPTIM_GENEEST", "N_OPTIM_TEST", "N_GRID_GENEEST", "N_GRID_MAP")


def _spike(counts, seed, k=6):
    rng = np.random.default_rng(seed)
    counts = counts.copy()
    for r in rng.choice(counts.shape[0], k, replace=False):
        counts[r, rng.integers(counts.shape[1])] = int(counts[r].max() * 40 + 1000)
    return counts


def _designs():
    xa = simulate.design_batch_condition(48)                 # 4 cells of 12: outliers are replaced and refitted
    da = simulate.make_counts(600, xa, seed=3, size_factors=np.exp(np.random.default_rng(1).normal(0, .2, 48)))
    ca = _spike(da["counts"], 5)
    ca[::53] = 0
    xb = simulate.design_factor(40, 5)                       # 5 cells of 8: other cells, other outlier metadata
    db = simulate.make_counts(450, xb, seed=9)
    return {"A": (ca, xa, da["size_factors"]), "B": (_spike(db["counts"], 12, 5), xb, db["size_factors"])}


DESIGNS = _designs()


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _host(name, shards, devices=None):
    counts, x, sf = DESIGNS[name]
    with _env(DSQ_HOST_SHARDS=shards, DSQ_HOST_DEVICES=devices):
        return native.DESeq(counts, x, sf, assays=("mu", "H", "cooks"))      # (raises unless the call returns DSQ_OK)


def _same_host(res, ref, what):
    for k in GENE_COLS:
        assert_same(np.asarray(res[k], float), np.asarray(ref[k], float), "%s: %s" % (what, k))
    assert_same(res["dispersionFunction"]["coefficients"], ref["dispersionFunction"]["coefficients"], what + ": trend")
    for k in COUNTERS:
        assert res["status"][k] == ref["status"][k], (what, k)
    # assays: all-zero rows hold whatever the kernels left (never read)
    nz = ~np.asarray(ref["allZero"], bool)
    for k in ("mu", "H", "cooks"):
        assert_same(res[k][nz], ref[k][nz], "%s: assays$%s" % (what, k))


@pytest.fixture(scope="module")
def single_range():
    """the reference of every test: one range, on the caller's thread, device and null stream"""
    ref = {name: _host(name, 1, 1) for name in DESIGNS}
    assert ref["A"]["status"]["N_REFIT"] >= 3 and ref["B"]["status"]["N_REFIT"] >= 1      # both upload outlier metadata
    return ref


def test_pinned_ring_wraps_around(single_range):
    """More than kPinRing host calls in one process, two designs with different cells in turn (so every call uploads its
    cell tables and its outlier metadata through the ring of each worker's context), three ranges."""
    for i in range(K_PIN_RING + 4):
        name = "AB"[i % 2]
        _same_host(_host(name, 3), single_range[name], "call %d (design %s, 3 ranges)" % (i, name))


def _fused(name, E, stream=None):
    import torch
    counts, x, sf = DESIGNS[name]
    b = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
    assert fused.supported(b)
    if stream is None:
        fused.DESeq(b)
    else:
        with torch.cuda.stream(stream):
            fused.DESeq(b)
    torch.cuda.synchronize()
    assert b.attrs.get("fused")
    out = {k: np.array(np.asarray(b.mcols[k], dtype=np.float64)) for k in sorted(b.mcols)}
    out["trend"] = np.array(np.asarray(b.dispersionFunction["coefficients"], dtype=np.float64))
    return out


def test_release_and_reuse(single_range):
    """The device chain on the current torch stream and on a second one, dsq_release_workspace(), both again; then the
    host entry in three ranges before and after another release (the worker threads outlive it).  A context pointer
    kept across the release would be stale here."""
    import torch
    E = DeviceEngine("cuda:0")
    L = _lib.lib()
    second = torch.cuda.Stream()
    first = {}
    for rnd in range(2):
        for sname, st in (("current", None), ("second", second)):
            for name in "AB":
                got = _fused(name, E, st)
                ref = first.setdefault(name, got)
                assert sorted(got) == sorted(ref)
                for k in sorted(got):
                    assert_same(got[k], ref[k], "round %d, %s stream, design %s: %s" % (rnd, sname, name, k))
        assert L.dsq_release_workspace() == _lib.DSQ_OK
    # ... and the device chain computes what the single-range host call does
    for name in "AB":
        for k in ("dispGeneEst", "dispersion", "beta", "betaSE", "maxCooks"):
            assert_same(first[name][k], np.asarray(single_range[name][k], float), "device chain, design %s: %s" % (name, k))
    for rnd in range(2):
        for name in "AB":
            _same_host(_host(name, 3), single_range[name], "host entry, round %d, design %s" % (rnd, name))
        assert L.dsq_release_workspace() == _lib.DSQ_OK
    for name in "AB":
        _same_host(_host(name, 3), single_range[name], "host entry after the last release, design %s" % name)


@pytest.mark.parametrize("shards", [2, 4])
def test_two_devices(single_range, shards):
    """DSQ_HOST_DEVICES=2: worker k serves device k % 2, so a worker of device 1 uploads the design cells and the outlier
    metadata of its range -- through the ring, the events and the stream of ITS context.  Twice in a row."""
    if _lib.lib().dsq_device_count() < 2:
        pytest.skip("one device visible: the two-device path cannot run here")
    for i in range(2):
        _same_host(_host("A", shards, 2), single_range["A"], "2 devices, %d ranges, call %d" % (shards, i))
