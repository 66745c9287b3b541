"""K contrasts from one covariance pass per gene on the device (csrc/contrasts.hip) against the
oracle's fitBeta(contrast = c_k, maxit = 0) plus the scalings of tests/contrast_spec.py, BIT FOR BIT (NaN included): the Gram
sums take the cell-collapsed form exactly where dsq_fit_beta_dev does, every other operation is the oracle's in its order."""
import ctypes as C
import re
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
    if kind == "unbalanced":                  # two levels, one sample in the second (in the middle of the row): cells of m - 1 and 1
        assert p == 2
        return np.column_stack([np.ones(m), (np.arange(m) == m // 3).astype(np.float64)])
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
        with np.errstate(invalid="ignore"):   # (a row whose weights are all 0 -- it happens at m = 4 and 24 000 rows -- is NaN throughout)
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


def _reference(O, d, ks=None, cell_mode=1):
    """the oracle's fitBeta(maxit = 0) per contrast + the spec's scalings, NA rows and all-zero rule; cell_mode = 0: the
    per-sample order of the Gram sums whatever the design (the device called without cell labels)"""
    n, m, K = d["n"], d["m"], d["K"]
    ks = range(K) if ks is None else ks
    out = {k: np.full((n, K), np.nan) for k in TAB}
    flags = np.zeros((n, K), np.int32)
    live = d["allZero"] == 0
    w = d["w"] if d["w"] is not None else np.ones((n, m))
    for k in ks:
        r = O.fitBeta(np.zeros((n, m)), d["x"], d["nf"], d["alpha"], d["ct"][:, k], d["beta"], d["lam"], w, d["w"] is not None, 1e-8,
                      0, False, d["minmu"], cell_mode=cell_mode)
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


# ---- the launch rule of csrc/contrasts.hip restated, and the line launch_contrasts prints under DSQ_VERBOSE ------------------
# ct_shared_doubles / ct_gene_doubles / ct_waves_per_gene / contrasts_max_m / launch_contrasts, csrc/contrasts.hip; DSQ_CMAX and
# DSQ_P_WIDE, csrc/dsq_internal.hpp.  test_launch_rule_restatement holds this copy to dsq_contrasts_max_m for every width.
CT_WAVES, CT_CU_LDS, CT_CMAX, CT_P_WIDE = 4, 160 * 1024, 32, 64


def ct_shared_doubles(p, ncell):
    return p + ncell * p


def ct_gene_doubles(p, m, cell, wpg):
    return 3 * p * p + 2 * p + 64 * wpg + (CT_CMAX if cell else m) + (p + 1) // 2


def ct_lds(p, m, ncell, wpg):
    return 8 * (ct_shared_doubles(p, ncell) + (CT_WAVES // wpg) * ct_gene_doubles(p, m, ncell > 0, wpg))


def ct_waves_per_gene(p, m, ncell=0):
    wpg = 1 if p <= 16 else 2 if p <= 32 else 4
    while wpg <= CT_WAVES:
        if ct_lds(p, m, ncell, wpg) <= CT_CU_LDS:
            return wpg
        wpg *= 2
    return 0


def ct_max_m(p):
    return (CT_CU_LDS - 8 * (ct_shared_doubles(p, 0) + ct_gene_doubles(p, 0, False, CT_WAVES))) // 8


def ct_last_m(p, wpg):
    """the longest per-sample row that wpg waves per gene take: the largest m with ct_lds(p, m, 0, wpg) <= CT_CU_LDS"""
    gpw = CT_WAVES // wpg
    return (CT_CU_LDS // 8 - ct_shared_doubles(p, 0)) // gpw - ct_gene_doubles(p, 0, False, wpg)


def ct_round(p, m, ncell, cus):
    """genes of one grid round: workgroups per CU by the LDS (at most eight) x CUs x genes per workgroup"""
    wpg = ct_waves_per_gene(p, m, ncell)
    bpc = max(1, min(8, CT_CU_LDS // ct_lds(p, m, ncell, wpg)))
    return cus * bpc * (CT_WAVES // wpg)


LAUNCH_LINE = re.compile(r"\[dsq\] contrasts p=(\d+) m=(\d+) K=(\d+): (cell|per-sample) path, (\d+) waves per gene, lds=(\d+), grid (\d+)")


def _dev_line(d, monkeypatch, capfd, **kw):
    """_dev under DSQ_VERBOSE: the result and the launch line as dict(path, wpg, lds, grid, round = genes of one grid round)"""
    monkeypatch.setenv("DSQ_VERBOSE", "1")
    capfd.readouterr()
    got = _dev(d, **kw)
    err = capfd.readouterr().err
    monkeypatch.delenv("DSQ_VERBOSE")
    lines = LAUNCH_LINE.findall(err)
    assert len(lines) == 1, "no launch line in %r" % err
    p, m, K, path, wpg, lds, grid = lines[0]
    assert (int(p), int(m), int(K)) == (d["p"], d["m"], d["K"])
    print(err.strip())
    return got, dict(path=path, wpg=int(wpg), lds=int(lds), grid=int(grid), round=int(grid) * (CT_WAVES // int(wpg)))


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_launch_rule_restatement():
    """the Python copy of the launch formulas against the library for every width, and against itself: ct_last_m is the last m
    at which ct_waves_per_gene still answers wpg, one more doubles the waves (or is refused at four)"""
    from deseq2_amd import _lib as L
    for p in range(1, CT_P_WIDE + 1):
        assert ct_max_m(p) == int(L.lib().dsq_contrasts_max_m(p)), p
        assert ct_last_m(p, CT_WAVES) == ct_max_m(p)
        wpg = ct_waves_per_gene(p, 1)
        assert wpg == (1 if p <= 16 else 2 if p <= 32 else 4)
        while wpg <= CT_WAVES:
            last = ct_last_m(p, wpg)
            assert ct_waves_per_gene(p, last) == wpg and ct_waves_per_gene(p, last + 1) == (2 * wpg if wpg < CT_WAVES else 0), (p, wpg)
            wpg *= 2
    # what the formulas give on the 160 KiB of a gfx950 CU: a change of the kernel's LDS layout shows here first
    assert (ct_max_m(2), ct_max_m(12), ct_max_m(64)) == (20205, 19750, 7712)
    assert (ct_last_m(2, 1), ct_last_m(2, 2), ct_last_m(12, 1), ct_last_m(12, 2), ct_last_m(32, 2)) == (5038, 10094, 4591, 9644, 6944)


# ---- past one grid round: the gene loop's second, third and tail trips on LDS the trip before left behind --------------------
def _plant(d, rnd):
    """rows laid out by the round so that a slot meets, trip after trip: an all-zero row (nothing written to its LDS) / a NaN
    coefficient (NaN all over its LDS) / a row on minmu, then a live row, then the same again; the reverse orders in the
    next slots; and in the tail trip (rows 3 rnd ...) live rows after a NaN, an all-zero and a minmu row"""
    n, p = d["n"], d["p"]
    def zero(g): d["allZero"][g] = 1
    def nan(g): d["beta"][g, p - 1] = np.nan
    def minmu(g): d["beta"][g, 0] = -25.0
    s = rnd // 2
    for i, special in enumerate((zero, nan, minmu)):
        special(s + i), special(2 * rnd + s + i)                   # special, live, special
        special(rnd + s + 3 + i)                                   # live, special, live
    for i, special in enumerate((nan, zero, minmu)):
        if 3 * rnd + i < n:
            special(2 * rnd + i)                                   # ... then the live row of the tail trip
    planted = np.r_[s + np.arange(3), 2 * rnd + s + np.arange(3), rnd + s + 3 + np.arange(3)]
    live = np.r_[rnd + s + np.arange(3), s + 3 + np.arange(3), 2 * rnd + s + 3 + np.arange(3), np.arange(3 * rnd, n)]
    return planted, live


TRIPS = [
    # kind, p, m, K, r, weights, rule
    ("cont", 2, 4, 3, 1, True, False),
    ("cont", 2, 4, 3, 3, False, True),
    ("cont", 12, 13, 7, 1, False, False),
    ("cont", 12, 13, 7, 3, True, True),
    ("cont", 64, 65, 2, 1, True, False),
    ("cont", 64, 65, 2, 3, False, True),
    ("factor", 6, 12, 3, 1, False, False),
    ("factor", 6, 12, 3, 3, True, True),
]


@pytest.mark.parametrize("case", TRIPS, ids=["%s-p%d-m%d-K%d-3rounds+%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "-w" if c[5] else "",
                                                                               "-rule" if c[6] else "") for c in TRIPS])
def test_gene_loop_past_one_round(oracle, monkeypatch, capfd, case):
    """The persistent gene loop of contrasts_kernel, `base += gridDim.x * gpw`: n = 3 rounds + r genes, so every slot makes
    three trips on the LDS of the trip before and r slots a fourth -- the tail trip, in which the other slots of a workgroup
    (or of the grid, at one gene per workgroup) are inactive and only walk the barriers.  _plant puts all-zero, NaN and minmu
    rows before and after live rows of the same slot.  The round is worked out from the restated launch rule and the CU
    count, and the launch line must confirm it; every row of every trip is compared.  The `cont` designs are given without
    cell labels (a row of 4 or 13 samples has few enough distinct design rows for the cell path), so that the per-sample
    path and its samp[m] are what is carried from trip to trip; the oracle then runs in cell_mode = 0."""
    kind, p, m, K, r, wts, rule = case
    ncell = p if kind == "factor" else 0
    rnd = ct_round(p, m, ncell, _cus())
    n = 3 * rnd + r
    d = _case(kind, p, m, n, K, seed=p * 1000 + m * 7 + K + r, weights=wts, rule=rule)
    planted, live = _plant(d, rnd)
    got, line = _dev_line(d, monkeypatch, capfd, cells=ncell > 0)
    assert line["path"] == ("cell" if ncell else "per-sample") and line["wpg"] == ct_waves_per_gene(p, m, ncell)
    assert line["round"] == rnd, "the rows were laid out for a round of %d genes, the launch took %d" % (rnd, line["round"])
    assert line["grid"] * (CT_WAVES // line["wpg"]) < n and n == 3 * line["round"] + r
    ref = _reference(oracle, d, cell_mode=int(ncell > 0))
    _compare(got, ref, "%s p=%d m=%d n=%d K=%d" % (kind, p, m, n, K))
    nan_rows = planted[1::3]
    assert np.isnan(got["pvalue"][planted[::3]]).all()                                                     # (the all-zero rows)
    assert np.isnan(got["log2FoldChange"][nan_rows][got["contrastAllZero"][nan_rows] == 0]).all()         # (the NaN coefficients)
    assert np.isfinite(ref["lfcSE"][live]).all() and np.isfinite(ref["pvalue"][live]).all()


# ---- long rows on the per-sample path: the waves per gene on both sides of each LDS threshold, and the limit itself --------
def _long_rows():
    rows = [(p, m, 3, None, "workload") for p in (4, 12) for m in (500, 2000)]     # (C3: m = 500)
    for p, wpg in ((2, 1), (2, 2), (12, 1), (12, 2), (32, 2)):
        last = ct_last_m(p, wpg)
        rows += [(p, last, 3, wpg, "last"), (p, last + 1, 3, 2 * wpg, "first")]
    rows += [(p, ct_max_m(p), 3, CT_WAVES, "limit") for p in (2, 12, 64)]
    rows.append((2, ct_last_m(2, 1) + 1, 70, 2, "contrast-trips"))  # 32 contrasts per wave and trip, two waves: a second trip at sw > 0
    return rows


LONG = _long_rows()


@pytest.mark.parametrize("idx", range(len(LONG)), ids=["p%d-m%d-K%d-%s%s" % (c[0], c[1], c[2], c[4], "-wpg%d" % c[3] if c[3] else "")
                                                       for c in LONG])
def test_long_rows_per_sample(oracle, monkeypatch, capfd, idx):
    """Rows of 500 ... dsq_contrasts_max_m(p) samples on the per-sample path: samp[m] in LDS, the Gram tasks, elimination
    rows and contrasts split over 2 and 4 waves of a gene at NARROW designs too (cpw = 64 / p > 1 with sw > 0).  "last" /
    "first": the last m that ct_waves_per_gene gives wpg waves and the first it gives 2 wpg (ct_last_m, from the restated
    formulas); "limit": m == dsq_contrasts_max_m(p); the launch line must name the waves expected on either side."""
    from deseq2_amd import _lib as L
    p, m, K, wpg, what = LONG[idx]
    d = _case("cont", p, m, 5, K, seed=p * 1000 + m * 7 + K, weights=bool(idx & 1))
    got, line = _dev_line(d, monkeypatch, capfd)
    assert line["path"] == "per-sample" and line["wpg"] == ct_waves_per_gene(p, m) and line["lds"] <= CT_CU_LDS
    if wpg is not None:
        assert line["wpg"] == wpg
    if what == "limit":
        assert m == int(L.lib().dsq_contrasts_max_m(p)) and line["lds"] + 8 > CT_CU_LDS
    if what == "contrast-trips":
        assert K > line["wpg"] * (64 // p)
    _compare(got, _reference(oracle, d), "cont p=%d m=%d K=%d" % (p, m, K))


# ---- cells longer than a wave: the multi-trip cell sum `k = s0 + ((lane - s0) & 63); k < s1; k += 64` ------------------------
LONG_CELLS = [("factor", 2, 130, False), ("factor", 2, 131, False), ("factor", 2, 2000, True), ("factor", 6, 2000, False),
              ("unbalanced", 2, 201, False)]


@pytest.mark.parametrize("case", LONG_CELLS, ids=["%s-p%d-m%d%s" % (c[0], c[1], c[2], "-w" if c[3] else "") for c in LONG_CELLS])
def test_cells_longer_than_a_wave(oracle, monkeypatch, capfd, case):
    """design cells of 65 ... 1 000 samples on the cell path (cell labels given; the oracle in cell_mode = 1): a lane's
    partial of the cell sum takes several trips, the cells start at positions that are no multiple of 64, and one design
    has a cell of one sample beside one of 200"""
    from deseq2_amd import native
    kind, p, m, wts = case
    d = _case(kind, p, m, 5, 3, seed=p * 1000 + m, weights=wts)
    sizes = np.bincount(native.cell_index(d["x"]))
    assert sizes.size == p and sizes.max() > 64 and (kind != "unbalanced" or sorted(sizes) == [1, 200])
    got, line = _dev_line(d, monkeypatch, capfd)
    assert line["path"] == "cell" and line["wpg"] == 1
    _compare(got, _reference(oracle, d), "%s p=%d m=%d" % (kind, p, m))


def test_cell_choice_at_2000_samples(oracle, monkeypatch, capfd):
    """test_cell_choice_is_fit_betas at m = 2 000: with the labels the cell path, without them the per-sample path, each equal
    to the oracle in that mode and not equal to each other -- a silent fall-back to the per-sample order cannot pass"""
    n, m = 5, 2000
    d = _case("factor", 6, m, n, 2, seed=4, rule=False)
    (with_cells, l1), (without, l0) = _dev_line(d, monkeypatch, capfd), _dev_line(d, monkeypatch, capfd, cells=False)
    assert l1["path"] == "cell" and l0["path"] == "per-sample"
    w = np.ones((n, m))
    live = d["allZero"] == 0
    for k in range(2):
        for mode, got in ((1, with_cells), (0, without)):
            r = oracle.fitBeta(np.zeros((n, m)), d["x"], d["nf"], d["alpha"], d["ct"][:, k], d["beta"], d["lam"], w, False, 1e-8, 0,
                               False, 0.5, cell_mode=mode)
            assert_same(got["lfcSE"][live, k], (CS.LOG2E * r["contrast_denom"].reshape(-1))[live], "cell_mode %d" % mode)
    assert not np.array_equal(with_cells["lfcSE"], without["lfcSE"], equal_nan=True)


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
