"""-m gpu: Student's t on the device against its numpy statement deseq2_amd/student_t.py on the oracle's
exp / log / log1p / stirlerr, BIT FOR BIT: dpt_upper / dpt_lower through the math hook, the elementwise pass dsq_pt_dev,
the results table with degrees of freedom, the contrasts with degrees of freedom, and a useT analysis end to end."""
from collections import OrderedDict

import json
import os

import numpy as np
import pytest

from deseq2_amd import student_t as S
from tests import results_spec as RS
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pt_golden.json")))
ALT = ("greaterAbs", "lessAbs", "greater", "less", "greaterAbs2014")


def test_math_hook_ops_10_and_11(oracle):
    """the golden arguments (every range switch of the method on either side, q^2 overflowing, df up to 1e8) and 4096 seeded
    pairs, |q| log-uniform over 1e-10 .. 1e4 with both signs, df log-uniform over 0.05 .. 1e8; then the special values"""
    from deseq2_amd import native
    rec = GOLD["normal"] + GOLD["tiny"]
    rng = np.random.Generator(np.random.PCG64(21))
    q = np.concatenate([[float(e[1]) for e in rec], 10.0 ** rng.uniform(-10, 4, 4096) * rng.choice([-1.0, 1.0], 4096),
                        [np.nan, 1.0, 1.0, 1.0, np.inf, -np.inf, 0.0, -0.0, 2.5, -2.5, np.inf]])
    df = np.concatenate([[float(e[2]) for e in rec], 10.0 ** rng.uniform(np.log10(0.05), 8, 4096),
                         [3.0, np.nan, 0.0, -1.0, 4.0, 4.0, 0.3, 0.3, np.inf, np.inf, np.inf]])
    assert_same(native.test_math(10, q, df), S.pt_upper(oracle, q, df), "dpt_upper")
    assert_same(native.test_math(11, q, df), S.pt_lower(oracle, q, df), "dpt_lower")


def _pt_inputs():
    rng = np.random.Generator(np.random.PCG64(22))
    n, K = 300, 3                                  # 900 entries: three full blocks of 256 and a ragged one
    q = rng.normal(0, 5, (n, K))
    q[rng.uniform(size=(n, K)) < 0.05] *= 1e3
    q[4, 1], q[5, 2], q[6, 0] = np.nan, np.inf, -np.inf
    df = 10.0 ** rng.uniform(-1, 3, n)
    df[10], df[11], df[12], df[13] = np.nan, np.inf, 0.0, -2.0
    keep = (rng.uniform(size=(n, K)) < 0.1).astype(np.int32)
    return n, K, q, df, keep


@pytest.mark.parametrize("tail", ["lower", "upper", "two_sided"])
def test_pt_dev(oracle, tail):
    """dsq_pt_dev on resident tensors, out of place and in place, with and without keep flags; dsq_pt on host arrays"""
    import torch
    from deseq2_amd import native
    n, K, q, df, keep = _pt_inputs()
    want = {"lower": S.pt_lower, "upper": S.pt_upper, "two_sided": S.pt_two_sided}[tail](oracle, q, df[:, None])
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a.T), device=dev)
    qd, dfd, kd = up(q), torch.as_tensor(df, device=dev), up(keep)
    out = torch.full((K, n), -7.25, dtype=torch.float64, device=dev)
    native.pt_dev(qd, dfd, tail, out=out)
    assert_same(out.cpu().numpy().T, want, "out of place")
    assert_same(qd.cpu().numpy().T, q, "q untouched")
    out = torch.full((K, n), -7.25, dtype=torch.float64, device=dev)
    native.pt_dev(qd, dfd, tail, keep=kd, out=out)
    assert_same(out.cpu().numpy().T, np.where(keep != 0, -7.25, want), "keep, out of place")
    q2 = qd.clone()
    native.pt_dev(q2, dfd, tail, keep=kd, out=q2)
    assert_same(q2.cpu().numpy().T, np.where(keep != 0, q, want), "keep, in place")
    q3 = qd.clone()
    native.pt_dev(q3, dfd, tail, out=q3)
    assert_same(q3.cpu().numpy().T, want, "in place")
    assert_same(native.pt(q, df, tail), want, "dsq_pt")
    assert_same(native.pt(q, df, tail, keep=keep), np.where(keep != 0, q, want), "dsq_pt, keep")
    assert_same(native.pt(q[:, 0], df, tail), want[:, 0], "dsq_pt, a vector")


def _results_inputs():
    rng = np.random.Generator(np.random.PCG64(23))
    n, p = 300, 3                                  # two blocks of the table kernel, the last one ragged
    beta = rng.normal(0, 1.5, (n, p))
    se = np.exp(rng.normal(-1, 0.6, (n, p)))
    beta[3, 2], se[4, 2], se[5, 2], beta[6, 2] = np.nan, np.nan, 0.0, 0.0
    with np.errstate(all="ignore"):
        stat = beta / se
    pv = rng.uniform(size=(n, p))
    bm = np.exp(rng.normal(3, 2, n))
    bm[7], bm[8] = 0.0, 0.0
    replace = np.zeros(n, np.int32)
    replace[[7, 20]] = 1
    na_mask = np.zeros(n, np.int32)
    na_mask[[9, 30]] = 1
    df = rng.uniform(0.5, 14, n)
    df[11], df[12], df[13] = np.nan, np.inf, 0.05
    return n, beta, se, stat, pv, bm, replace, na_mask, df


@pytest.mark.parametrize("alt", ALT)
def test_results_with_degrees_of_freedom(oracle, alt):
    from deseq2_amd import native
    from deseq2_amd.engine import HostEngine
    n, beta, se, stat, pv, bm, replace, na_mask, df = _results_inputs()
    theta = np.linspace(0, 0.9, 7)
    T = 0.75
    got = native.results(beta, se, stat, pv, bm, 2, replace=replace, na_mask=na_mask, lfcThreshold=T, altHypothesis=alt,
                         theta=theta, alpha=0.1, df=df)
    ref = HostEngine(oracle).results(beta[:, 2], se[:, 2], stat[:, 2], pv[:, 2], bm, replace, na_mask, T, alt, df=df,
                                     theta=theta, alpha=0.1)
    for c in ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue"):
        assert_same(got[c], ref.column(c), "%s, df: %s" % (alt, c))
    for j in range(theta.size):
        assert_same(got["filtPadj"][:, j], ref.padj_column(j), "%s, df: filtPadj[, %d]" % (alt, j))
    assert_same(got["numRej"], ref.numRej, alt + ", df: numRej")
    assert np.isnan(got["pvalue"][11]) and np.isfinite(got["pvalue"][[12, 13]]).all()
    # df = NULL: the normal-distribution table, as before
    plain = native.results(beta, se, stat, pv, bm, 2, replace=replace, na_mask=na_mask, lfcThreshold=T, altHypothesis=alt,
                           theta=theta, alpha=0.1)
    spec = RS.results(oracle, beta[:, 2], se[:, 2], stat[:, 2], pv[:, 2], bm, replace == 1, na_mask == 1, T, alt, theta=theta,
                      alpha=0.1)
    for c in ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "filtPadj", "numRej"):
        assert_same(plain[c], spec[c], "%s, no df: %s" % (alt, c))
    assert not np.array_equal(plain["pvalue"], got["pvalue"], equal_nan=True)
    assert_same(plain["stat"], got["stat"], alt + ": stat does not depend on the distribution")
    # dsq_results_dev itself, on resident tensors
    import torch
    dev = torch.device("cuda:0")
    up = lambda a, dt=np.float64: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt)), device=dev)
    r = native.results_dev(up(beta.T), up(se.T), up(stat.T), up(pv.T), up(bm), 2, replace=up(replace, np.int32),
                           na_mask=up(na_mask, np.int32), lfcThreshold=T, altHypothesis=alt, theta=up(theta), alpha=0.1, df=up(df))
    torch.cuda.synchronize()
    for i, c in enumerate(("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue")):
        assert_same(r["table"][i].cpu().numpy(), got[c], "%s, dsq_results_dev: %s" % (alt, c))
    assert_same(r["filtPadj"].cpu().numpy().T, got["filtPadj"], alt + ", dsq_results_dev: filtPadj")
    cutoffs, numRej, status = native.results_small(r["_small"].cpu().numpy(), r["K"])
    assert status == 0
    assert_same(numRej, got["numRej"], alt + ", dsq_results_dev: numRej")


def _contrast_case(kind, p, m, K, seed, weights):
    from deseq2_amd import simulate
    rng = np.random.Generator(np.random.PCG64(seed))
    n = 70
    if kind == "factor":
        x = simulate.design_factor(m, p)
    else:
        x = np.column_stack([simulate.design_factor(m, p - 1), rng.normal(0.0, 0.5, m)])
    beta = np.column_stack([rng.normal(3.0, 1.5, n)] + [rng.normal(0, 0.7, n) for _ in range(p - 1)])
    nf = np.exp(rng.normal(0, 0.3, (n, m)))
    alpha = np.exp(rng.normal(-2, 1, n))
    allZero = np.zeros(n, np.int32)
    allZero[[2, 40]] = 1
    beta[1, p - 1] = np.nan
    w = None
    if weights:
        w = rng.uniform(0.05, 1.0, (n, m))
        w = w / w.max(axis=1, keepdims=True)
    ct = rng.integers(-2, 3, (p, K)).astype(np.float64)
    ct[0, ct.any(axis=0) == 0] = 1.0
    lam = np.exp(rng.normal(-10, 3, p))
    counts = (rng.poisson(2.0, (n, m)) * (rng.uniform(size=(n, m)) < 0.4)).astype(np.int32)
    counts[rng.uniform(size=n) < 0.3] = 0
    counts[5], counts[6] = 0, 3                    # row 5: "all zero" under every non-empty mask, row 6: under none
    mask = (rng.uniform(size=(K, m)) < 0.3).astype(np.int32)
    mask[:, 0] = 1                                 # (no mask empty by chance)
    if K > 3:
        mask[3] = 0                                # a mask that selects no sample: every live row is "all zero"
    rule = np.ones(K, np.int32)
    if K > 4:
        rule[4] = 0
    df = (w.sum(axis=1) if weights else np.full(n, float(m))) - p
    df[5], df[6] = np.nan, -0.5                    # (NA degrees of freedom: p-value 1 where the all-zero rule fired, else NA)
    return dict(x=x, beta=beta, nf=nf, alpha=alpha, allZero=allZero, w=w, ct=ct, lam=lam, counts=counts, mask=mask, rule=rule,
                df=np.where(df > 0, df, np.nan), n=n, m=m, p=p, K=K)


@pytest.mark.parametrize("K", [1, 37])
@pytest.mark.parametrize("kind,p,m,weights", [("factor", 4, 12, False), ("cont", 3, 9, True)])
def test_contrasts_with_degrees_of_freedom(oracle, kind, p, m, weights, K):
    """the cell path (p = 4, m = 12) and the per-sample path (a continuous covariate, p = 3, m = 9, weights); K = 37: several
    trips of 64 / p contrasts per wave"""
    from deseq2_amd import native
    from deseq2_amd.engine import HostEngine
    d = _contrast_case(kind, p, m, K, 100 * p + K, weights)
    call = lambda df: native.contrasts(d["x"], d["nf"], d["alpha"], d["beta"], d["lam"], d["ct"], weights=d["w"],
                                       useWeights=weights, minmu=0.5, allZero=d["allZero"], counts=d["counts"],
                                       sample_mask=d["mask"], rule_applies=d["rule"], df=df)
    got, plain = call(d["df"]), call(None)
    ref = HostEngine(oracle).contrasts(d["counts"], d["x"], d["nf"], d["alpha"], d["beta"], d["lam"], d["ct"], d["w"], weights, 0.5,
                                       d["allZero"], sample_mask=d["mask"], rule_applies=d["rule"], df=d["df"])
    for i, c in enumerate(("log2FoldChange", "lfcSE", "stat", "pvalue")):
        assert_same(got[c], ref.table[i], "%s K=%d: %s" % (kind, K, c))
    assert_same(got["contrastAllZero"] != 0, ref.flag_matrix, "flags")
    for c in ("log2FoldChange", "lfcSE", "stat", "contrastAllZero"):
        assert_same(got[c], plain[c], "%s K=%d: %s with and without df" % (kind, K, c))
    z = got["contrastAllZero"] != 0
    ruled = d["rule"] != 0
    empty = ~d["mask"].any(axis=1)                                                        # (column 3 at K = 37, none at K = 1)
    assert (got["pvalue"][z] == 1.0).all() and z[5, 0] and z[5][ruled].all() and (z[6] == empty).all()
    assert np.isnan(got["pvalue"][6][~empty]).all() and np.isnan(got["pvalue"][5][~z[5]]).all()
    assert np.isnan(got["pvalue"][[2, 40]]).all() and (z[:, empty].sum(axis=0) == 68).all() and empty.sum() == (K > 3)
    live = ~z & np.isfinite(d["df"])[:, None] & np.isfinite(plain["pvalue"])
    assert live[:, 0].sum() >= 20                  # every call, the one-contrast call too, compares real t p-values
    assert (got["pvalue"][live] >= plain["pvalue"][live]).all()                           # (heavier tails)
    assert not np.array_equal(got["pvalue"][live], plain["pvalue"][live])
    # dsq_contrasts_dev itself, on resident data
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine("cuda:0")
    r = E.contrasts(E.counts(d["counts"]), d["x"], E.matrix(d["nf"]), d["alpha"], d["beta"], d["lam"], d["ct"],
                    E.matrix(d["w"]) if weights else None, weights, 0.5, d["allZero"], sample_mask=d["mask"],
                    rule_applies=d["rule"], df=d["df"])
    for i, c in enumerate(("log2FoldChange", "lfcSE", "stat", "pvalue")):
        assert_same(r.table[i].cpu().numpy().T, got[c], "%s K=%d, dsq_contrasts_dev: %s" % (kind, K, c))
    assert_same(r.flag_matrix.cpu().numpy().T, got["contrastAllZero"], "dsq_contrasts_dev: flags")


def test_use_t_analysis_end_to_end(oracle):
    """fused.DESeq(useT = True) on the device, then results(lfcThreshold = 1) and three contrasts, against the same calls on
    core.DESeq over HostEngine(oracle)"""
    from deseq2_amd import core, fused, simulate
    from deseq2_amd.engine import DeviceEngine, HostEngine
    f = OrderedDict(condition=np.repeat([0, 1, 2], 4))
    x, _ = core.standard_model_matrix(f)
    k = simulate.make_counts(200, x, seed=31, drop_all_zero=False)["counts"]
    k[[9, 120]] = 0
    k[7, f["condition"] != 0] = 0
    k[7, f["condition"] == 0] = [30, 41, 28, 35]
    # weights in 64ths with a 1 in every row: the normalised weights and their row sums are exact in any order.  (The order of
    # that host-side row sum is numpy's and follows the layout of the engine's handle, so two ENGINES may differ in the last
    # bit of a rounded sum -- tests/test_gpu_testthat.py holds their useT p-values to 1e-12 for that reason; the two chain
    # drivers on one engine agree bit for bit on any weights, tests/test_gpu_fused.py.)
    rng = np.random.Generator(np.random.PCG64(32))
    w = rng.integers(20, 65, k.shape) / 64.0
    w[np.arange(200), rng.integers(0, 12, 200)] = 1.0
    w[3] = 6 / 64.0
    w[3, 0] = 1.0                                  # sum(w) - p <= 0
    a = core.DESeqDataSet(k, x, weights=w, engine=DeviceEngine("cuda:0"))
    assert fused.supported(a, useT=True)
    fused.DESeq(a, useT=True)
    b = core.DESeq(core.DESeqDataSet(k, x, weights=w, engine=HostEngine(oracle)), useT=True)
    assert_same(a.mcols["tDegreesFreedom"], b.mcols["tDegreesFreedom"], "tDegreesFreedom")
    tdf = a.mcols["tDegreesFreedom"]
    assert np.isnan(tdf[[3, 9, 120]]).all() and np.isfinite(tdf).sum() == 197 and (tdf[np.isfinite(tdf)] % 1 != 0).sum() > 150
    cols = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj")
    ra, rb = (core.results(d, lfcThreshold=1, altHypothesis="greaterAbs") for d in (a, b))
    for c in cols:
        assert_same(ra[c], rb[c], "results: " + c)
    assert np.isfinite(ra["pvalue"]).sum() > 150
    for d in (a, b):
        d.attrs["factors"] = f
    forms = [("condition", 1, 0), ("condition", 2, 1), [0, 1, 0.5]]
    for form, ca, cb in zip(forms, core.resultsContrasts(a, forms), core.resultsContrasts(b, forms)):
        for c in cols:
            assert_same(ca[c], cb[c], "contrast %r: %s" % (form, c))
    assert core.resultsContrasts(a, forms[1:2])[0]["pvalue"][7] == 1.0
    q = np.asarray(ra["stat"])
    assert_same(core.pt(q, b.mcols["tDegreesFreedom"], engine=a.engine), S.pt_lower(oracle, q, b.mcols["tDegreesFreedom"]), "core.pt")
