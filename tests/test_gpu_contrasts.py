"""K contrasts from one covariance pass per gene on the device (csrc/contrasts.hip) against the
oracle's fitBeta(contrast = c_k, maxit = 0) plus the scalings of tests/contrast_spec.py, BIT FOR BIT (NaN included): the Gram
sums take the cell-collapsed form exactly where dsq_fit_beta_dev does, every other operation is the oracle's in its order."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest

from tests import contrast_spec as CS
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

TAB = ("log2FoldChange", "lfcSE", "stat", "pvalue")


# ---- designs ----------------------------------------------------------------------------------------------------------------
def _design(kind, p, m, seed):
    from deseq2_amd import simulate
    rng = np.random.default_rng(seed)
    if kind == "factor":                      # p levels: p design cells -> the cell path up to 32 columns
        return simulate.design_factor(m, p)
    if kind == "cont":                        # the same width with one continuous covariate: a cell per sample -> the general path
        cols = [simulate.design_factor(m, p - 1)] if p > 1 else []
        return np.column_stack(cols + [rng.normal(0.0, 0.5, m)])
    assert kind == "paired" and p == 13       # ~ patient + treatment, 11 x 3 = 33 cells: the general path by the cell count
    pat, trt = np.arange(m) % 11, (np.arange(m) // 11) % 3
    x = np.column_stack([np.ones(m)] + [(pat == a) for a in range(1, 11)] + [(trt == t) for t in (1, 2)]).astype(np.float64)
    assert np.unique(x, axis=0).shape[0] == 33
    return x


def _case(kind, p, m, n, K, seed, nf_vector=False, weights=False, alpha=None, rule=True):
    rng = np.random.default_rng(seed)
    x = _design(kind, p, m, seed)
    beta = np.column_stack([rng.normal(3.0, 1.5, n)] + [rng.normal(0, 0.7, n) for _ in range(p - 1)])
    if kind == "cont" and p == 1:
        beta = rng.normal(0, 0.7, (n, 1))
    sf = np.exp(rng.normal(0, 0.3, m))
    nf = np.broadcast_to(sf[None, :], (n, m)).copy() if nf_vector else np.exp(rng.normal(0, 0.3, (n, m)))
    a = np.exp(rng.normal(-2, 1, n)) if alpha is None else np.full(n, alpha)
    allZero = np.zeros(n, np.int32)
    if n >= 3:
        beta[0, 0] = -25.0                    # every mean of the row sits on minmu
        beta[1, p - 1] = np.nan               # a NaN coefficient
        allZero[2] = 1                        # an all-zero row: NA
    if n >= 65:
        beta[5, 0] = -1.5                     # some means on minmu, some above
    w = None
    if weights:
        w = rng.uniform(0.05, 1.0, (n, m))
        w[rng.uniform(size=(n, m)) < 0.1] = 0.0
        w = w / w.max(axis=1, keepdims=True)
    ct = rng.integers(-2, 3, (p, K)).astype(np.float64)
    ct[:, ::3] = rng.normal(0, 1, ct[:, ::3].shape)
    ct[0, ct.any(axis=0) == 0] = 1.0
    lam = np.exp(rng.normal(-10, 3, p))
    counts = (rng.poisson(2.0, (n, m)) * (rng.uniform(size=(n, m)) < 0.4)).astype(np.int32)
    counts[rng.uniform(size=n) < 0.3] = 0
    mask = rule_applies = None
    if rule:
        mask = (rng.uniform(size=(K, m)) < 0.3).astype(np.int32)
        mask[0] = 0                           # a mask that selects no sample: every row is "all zero"
        if K > 1:
            mask[1] = 1                       # ... all samples
        if K > 2:
            mask[2] = 0
            mask[2, m // 2] = 1               # ... one sample
        rule_applies = (rng.uniform(size=K) < 0.7).astype(np.int32)
        rule_applies[:3] = 1
    return dict(x=x, beta=beta, sf=sf, nf=nf, nf_vector=nf_vector, alpha=a, allZero=allZero, w=w, ct=ct, lam=lam, counts=counts,
                mask=mask, rule=rule_applies, n=n, m=m, p=p, K=K, minmu=0.5)


def _reference(O, d, ks=None):
    """the oracle's fitBeta(maxit = 0) per contrast + the spec's scalings, NA rows and all-zero rule"""
    n, m, K = d["n"], d["m"], d["K"]
    ks = range(K) if ks is None else ks
    out = {k: np.full((n, K), np.nan) for k in TAB}
    flags = np.zeros((n, K), np.int32)
    live = d["allZero"] == 0
    w = d["w"] if d["w"] is not None else np.ones((n, m))
    for k in ks:
        r = O.fitBeta(np.zeros((n, m)), d["x"], d["nf"], d["alpha"], d["ct"][:, k], d["beta"], d["lam"], w, d["w"] is not None, 1e-8,
                      0, False, d["minmu"])
        lfc, se = CS.LOG2E * r["contrast_num"].reshape(-1), CS.LOG2E * r["contrast_denom"].reshape(-1)
        with np.errstate(all="ignore"):
            stat = lfc / se
        pv = O.unary("pnorm_upper2", stat)
        if d["mask"] is not None and d["rule"][k]:
            flags[:, k] = CS.all_zero(d["counts"], d["mask"][k], ~live)
        z = flags[:, k] == 1
        lfc, stat, pv = np.where(z, 0.0, lfc), np.where(z, 0.0, stat), np.where(z, 1.0, pv)
        for name, v in zip(TAB, (lfc, se, stat, pv)):
            out[name][live, k] = v[live]
    out["contrastAllZero"] = flags
    return out


def _dev(d, cols=None, flags_only=False, cells=True):
    """dsq_contrasts_dev through ctypes on poisoned output buffers; returns host copies (n x K)"""
    import torch
    from deseq2_amd import _lib as L, native
    dev = torch.device("cuda:0")
    n, m, p = d["n"], d["m"], d["p"]
    ct = d["ct"] if cols is None else d["ct"][:, cols]
    mask, rule = d["mask"], d["rule"]
    if cols is not None and mask is not None:
        mask, rule = mask[cols], rule[cols]
    K = ct.shape[1]
    ld = native.gene_major_ld(m) + 8                     # (a leading dimension beyond the row length)
    def gm(a, dt):
        t = torch.full((n, ld), 99, dtype=dt, device=dev)
        t[:, :m] = torch.as_tensor(np.ascontiguousarray(a), device=dev)
        return t
    up = lambda a, dt=np.float64: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt)), device=dev)
    keep = dict(x=up(d["x"].T), nf=up(d["sf"]) if d["nf_vector"] else gm(d["nf"], torch.float64), alpha=up(d["alpha"]),
                beta=up(d["beta"].T), lam=up(d["lam"]), ct=up(ct.T), az=up(d["allZero"], np.int32))
    if d["w"] is not None:
        keep["w"] = gm(d["w"], torch.float64)
    if mask is not None:
        keep.update(y=gm(d["counts"], torch.int32), mask=up(mask, np.int32), rule=up(rule, np.int32))
    table = torch.full((4, K, n), -7.25, dtype=torch.float64, device=dev)
    flags = torch.full((K, n), -9, dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    cell = native.cell_index(d["x"]) if cells else None
    a = L.DsqContrastsArgs(n=n, m=m, p=p, K=K, ld=ld, x=ptr(keep["x"]), nf=ptr(keep["nf"]), nf_is_vector=int(d["nf_vector"]),
                           alpha_hat=ptr(keep["alpha"]), beta=ptr(keep["beta"]), lambda_=ptr(keep["lam"]), weights=ptr(keep.get("w")),
                           useWeights=int(d["w"] is not None), minmu=d["minmu"], contrasts=None if flags_only else ptr(keep["ct"]),
                           allZero=ptr(keep["az"]), counts=ptr(keep.get("y")), sample_mask=ptr(keep.get("mask")),
                           rule_applies=ptr(keep.get("rule")), cell_of=None if cell is None else cell.ctypes.data_as(C.c_void_p),
                           ncell=0 if cell is None else int(cell.max()) + 1)
    o = L.DsqContrastsOut(log2FoldChange=ptr(table[0]), lfcSE=ptr(table[1]), stat=ptr(table[2]), pvalue=ptr(table[3]),
                          contrastAllZero=ptr(flags))
    L.check(L.lib().dsq_contrasts_dev(C.byref(a), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = {k: table[i].cpu().numpy().T for i, k in enumerate(TAB)}
    out["contrastAllZero"] = flags.cpu().numpy().T
    return out


def _compare(got, ref, what, ks=None):
    for k in TAB + ("contrastAllZero",):
        a, b = (got[k], ref[k]) if ks is None else (got[k][:, ks], ref[k][:, ks])
        assert_same(a, b, "%s %s" % (what, k))


# p: the lane-per-column, rolled and cell-width boundaries; m, n, K: one wave, its edges, several trips; every value of the
# grid occurs, the large K with the narrow designs and the wide designs with the small K
GRID = [
    # kind, p, m, n, K, nf_vector, weights, alpha
    ("factor", 1, 2, 1, 1, False, False, None),
    ("cont", 1, 63, 3, 130, True, False, None),
    ("factor", 2, 3, 3, 65, False, True, None),
    ("cont", 2, 64, 65, 2, False, False, 1e-8),
    ("factor", 6, 7, 3, 64, True, False, 10.0),
    ("cont", 6, 65, 65, 2, False, True, None),
    ("factor", 7, 130, 65, 130, False, False, None),
    ("cont", 7, 8, 1, 1, False, False, None),
    ("factor", 10, 11, 3, 65, False, False, 1e-8),
    ("cont", 10, 63, 65, 64, True, True, None),
    ("factor", 11, 12, 3, 2, False, False, None),
    ("cont", 11, 64, 65, 2, False, False, 10.0),
    ("factor", 12, 65, 65, 64, False, True, None),
    ("cont", 12, 13, 1, 1, True, False, None),
    ("paired", 13, 63, 3, 2, False, False, None),
    ("paired", 13, 130, 65, 65, True, True, None),
    ("factor", 32, 33, 3, 2, False, False, None),
    ("factor", 32, 130, 65, 2, True, True, 1e-8),
    ("cont", 32, 64, 3, 65, False, False, None),
    ("factor", 33, 34, 3, 2, False, False, None),
    ("cont", 33, 65, 65, 1, False, True, None),
    ("factor", 48, 49, 3, 2, True, False, 10.0),
    ("cont", 48, 130, 65, 2, False, False, None),
    ("factor", 64, 65, 3, 2, False, False, None),
    ("cont", 64, 130, 65, 1, False, True, None),
    ("cont", 64, 65, 1, 64, True, False, 1e-8),
]


@pytest.mark.parametrize("case", GRID, ids=["%s-p%d-m%d-n%d-K%d%s%s%s" % (c[0], c[1], c[2], c[3], c[4], "-sf" if c[5] else "",
                                                                       "-w" if c[6] else "", "" if c[7] is None else "-a%g" % c[7])
                                            for c in GRID])
def test_contrasts_dev_equals_oracle(oracle, case):
    kind, p, m, n, K, nfv, wts, alpha = case
    d = _case(kind, p, m, n, K, seed=p * 1000 + m * 7 + K, nf_vector=nfv, weights=wts, alpha=alpha)
    ks = None if K * p * p * n <= 4e6 else sorted(set([0, 1, 2, K // 2, K - 2, K - 1]) & set(range(K)))   # (the oracle's time)
    ref = _reference(oracle, d, ks)
    got = _dev(d)
    _compare(got, ref, "%s p=%d m=%d n=%d K=%d" % (kind, p, m, n, K), ks)
    assert (got["contrastAllZero"][:, 0] == (d["allZero"] == 0) * d["rule"][0]).all()       # (the empty mask)
    if n >= 3:
        assert np.isnan(got["log2FoldChange"][1][got["contrastAllZero"][1] == 0]).all() and np.isnan(got["pvalue"][2]).all()


def test_cell_choice_is_fit_betas(oracle):
    """the same factor design with and without the cell labels: two orders of the Gram sum, each equal to the oracle run in
    that mode, and not equal to each other everywhere"""
    d = _case("factor", 6, 65, 65, 2, seed=4, rule=False)
    with_cells, without = _dev(d), _dev(d, cells=False)
    w = np.ones((65, 65))
    for k in range(2):
        for mode, got in ((1, with_cells), (0, without)):
            r = oracle.fitBeta(np.zeros((65, 65)), d["x"], d["nf"], d["alpha"], d["ct"][:, k], d["beta"], d["lam"], w, False, 1e-8, 0,
                               False, 0.5, cell_mode=mode)
            live = d["allZero"] == 0
            assert_same(got["lfcSE"][live, k], (CS.LOG2E * r["contrast_denom"].reshape(-1))[live], "cell_mode %d" % mode)
    assert not np.array_equal(with_cells["lfcSE"], without["lfcSE"], equal_nan=True)


def test_K_contrasts_equal_K_calls(oracle):
    for kind, p, m in (("factor", 6, 65), ("cont", 12, 64), ("cont", 33, 65)):
        d = _case(kind, p, m, 65, 5, seed=p, weights=True)
        all_k = _dev(d)
        for k in range(5):
            one = _dev(d, cols=[k])
            for c in TAB + ("contrastAllZero",):
                assert_same(one[c][:, 0], all_k[c][:, k], "%s p=%d contrast %d %s" % (kind, p, k, c))


def test_flags_only(oracle):
    for m, n, K in ((2, 1, 1), (65, 65, 3), (130, 3, 65)):
        d = _case("factor", 2, m, n, K, seed=m)
        got = _dev(d, flags_only=True)
        want = np.zeros((n, K), np.int32)
        for k in range(K):
            if d["rule"][k]:
                want[:, k] = CS.all_zero(d["counts"], d["mask"][k], d["allZero"] != 0)
        assert_same(got["contrastAllZero"], want, "flags only m=%d" % m)
        assert (got["log2FoldChange"] == -7.25).all()                    # (the table outputs are not written)


def test_host_entry_equals_dev(oracle):
    from deseq2_amd import native
    for kind, p, m, n, K, nfv, wts in (("factor", 6, 65, 65, 3, False, True), ("cont", 33, 64, 3, 2, True, False)):
        d = _case(kind, p, m, n, K, seed=11, nf_vector=nfv, weights=wts)
        dv = _dev(d)
        h = native.contrasts(d["x"], d["sf"] if nfv else d["nf"], d["alpha"], d["beta"], d["lam"], d["ct"], weights=d["w"],
                             useWeights=wts, minmu=0.5, allZero=d["allZero"], counts=d["counts"], sample_mask=d["mask"],
                             rule_applies=d["rule"])
        for c in TAB + ("contrastAllZero",):
            assert_same(h[c], dv[c], "host entry %s %s" % (kind, c))
    d = _case("factor", 2, 65, 65, 3, seed=3)
    hf = native.contrasts(None, None, None, None, None, None, allZero=d["allZero"], counts=d["counts"], sample_mask=d["mask"],
                          rule_applies=d["rule"])
    assert_same(hf["contrastAllZero"], _dev(d, flags_only=True)["contrastAllZero"], "host flags only")


def test_rows_beyond_the_lds_are_refused():
    from deseq2_amd import _lib as L
    mx = int(L.lib().dsq_contrasts_max_m(64))
    d = _case("cont", 64, 65, 1, 1, seed=1, rule=False)
    _dev(d)
    d2 = dict(d, m=mx + 1, x=np.zeros((mx + 1, 64)), nf=np.ones((1, mx + 1)), sf=np.ones(mx + 1))
    with pytest.raises(L.DsqError) as ei:
        _dev(d2, cells=False)
    assert ei.value.code == 2


# ---- core.resultsContrasts: the device engine against the host engine -------------------------------------------------------
def _analysis_inputs(which):
    from deseq2_amd import core, simulate
    if which == "factor3":
        f = OrderedDict(condition=np.repeat([0, 1, 2], 4))
        n = 300
    else:                                        # ~ patient + treatment: 11 patients, 2 treatments: 12 columns, 22 cells
        f = OrderedDict(patient=np.tile(np.arange(11), 2), treatment=np.repeat([0, 1], 11))
        n = 200
    x, _ = core.standard_model_matrix(f)
    k = simulate.make_counts(n, x, seed=17, drop_all_zero=False)["counts"]
    last = list(f)[-1]
    k[7, f[last] != 0] = 0                       # zeros in the contrasted groups
    k[7, f[last] == 0] = 40 + np.arange(int((f[last] == 0).sum()))
    k[9] = 0                                     # an all-zero gene
    p = x.shape[1]
    c1 = np.zeros(p)
    c1[p - 1], c1[1] = 1.0, -1.0
    c2 = np.zeros(p)
    c2[1:3] = 0.5
    contrasts = [c1, c2, (last, 1, 0), (last, 0, 1)] + ([("condition", 1, 2)] if which == "factor3" else [])
    return f, x, k, contrasts


@pytest.mark.parametrize("chain", ["calls", "fused"])
@pytest.mark.parametrize("which", ["factor3", "paired12"])
def test_results_contrasts_device_equals_host(oracle, which, chain):
    import torch
    from deseq2_amd import core, fused
    from deseq2_amd.engine import DeviceEngine, HostEngine
    f, x, k, contrasts = _analysis_inputs(which)
    host = core.DESeq(core.DESeqDataSet(k, x, engine=HostEngine(oracle)), factors=f)
    dev = core.DESeqDataSet(k, x, engine=DeviceEngine())
    dev = core.DESeq(dev, factors=f) if chain == "calls" else fused.DESeq(dev)
    if dev.attrs.get("factors") is None:
        dev.attrs["factors"] = f                 # (the fused chain records the factors of a beta-prior analysis only)
    for kw in (dict(), dict(independentFiltering=False, cooksCutoff=False), dict(lfcThreshold=0.5, altHypothesis="greater")):
        rd, rh = core.resultsContrasts(dev, contrasts, **kw), core.resultsContrasts(host, contrasts, **kw)
        for i, (a, b) in enumerate(zip(rd, rh)):
            # residency: the columns of the table are device tensors until one is asked for
            assert all(torch.is_tensor(v) and v.is_cuda for v in a.tab.resident.values()), "contrast %d: resident columns" % i
            for c in core.DESeqResults.COLUMNS:
                assert_same(a[c], b[c], "%s %s %r contrast %d %s" % (which, chain, kw, i, c))
            assert a.metadata["contrast"] == b.metadata["contrast"]
            if not kw:
                assert np.isnan(rh[0]["pvalue"][9])
                if which == "factor3":
                    assert rh[0]["log2FoldChange"][7] == 0 and rh[0]["pvalue"][7] == 1 and rh[0]["lfcSE"][7] > 0


def test_engine_outputs_stay_resident(oracle):
    """DeviceEngine.contrasts returns device tensors: nothing n-sized comes to the host before a column is asked for"""
    import torch
    from deseq2_amd.engine import DeviceEngine, HostEngine
    d = _case("factor", 6, 65, 65, 3, seed=2, nf_vector=True)
    E = DeviceEngine()
    args = lambda e: (e.counts(d["counts"]), d["x"], None, d["alpha"], d["beta"], d["lam"], d["ct"], None, False, 0.5, d["allZero"] != 0)
    kw = dict(sample_mask=d["mask"], rule_applies=d["rule"], sizeFactors=d["sf"])
    r = E.contrasts(*args(E), **kw)
    assert all(torch.is_tensor(t) and t.is_cuda and t.shape == (3, 65) for t in r.table) and r.flag_matrix.is_cuda
    assert all(torch.is_tensor(v) and v.is_cuda and v.shape == (65,) for v in r.columns(1)) and r.flags(1).is_cuda
    h = HostEngine(oracle).contrasts(*args(HostEngine(oracle)), **kw)
    for i in range(4):
        assert_same(r.table[i].cpu().numpy().T, h.table[i], "engine " + TAB[i])
    assert_same(r.flag_matrix.cpu().numpy().T != 0, h.flag_matrix, "engine flags")
