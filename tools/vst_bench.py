"""Timing of the variance stabilizing transformation on the device (dsq_vst_dev, csrc/vst.hip) on resident matrices of the
C3 (50 000 x 500) and C4 (60 000 x 2 000) shapes, gene-major int32 counts, every kind, size factors and (--norm-matrix) a
normalization-factor matrix.  Next to each: the same quantity with stock torch ops on the same resident tensors in the
same run (the baseline), and a plain device copy of as many bytes as the algorithm moves (4 n m read + 8 n m written,
+ 8 n m with a matrix), whose rate is the yardstick of the "fraction of the copy rate" column.  HIP events, warm-up,
>= 20 repetitions, median and spread, a 512 MB buffer rewritten between repetitions so that no input is served from
the last-level cache; one JSON line per shape.

    python tools/vst_bench.py [--reps 20] [--shapes C3,C4] [--norm-matrix] [--e2e]

--e2e also times core.vst end to end on C3 (size factors given) and the share of it spent in the 1 000-gene dispersion fit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C3": (50000, 500), "C4": (60000, 2000)}
KINDS = ("parametric", "mean", "spline", "log2", "normalized")


def _events(torch, fn, warmup, reps, flush):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        flush.add_(1)                                   # evict the inputs from the last-level cache
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "iqr_ms": float(np.subtract(*np.percentile(ms, [75, 25]))), "reps": int(reps)}


def _torch_statement(torch, kind, k, nf, p):
    """the formulas of R/vst.R with stock torch ops (several passes and temporaries)"""
    q = k.to(torch.float64) / nf
    ln2 = float(np.log(2))
    if kind == "parametric":
        a, e = p["asymptDisp"], p["extraPois"]
        return torch.log((1 + e + 2 * a * q + 2 * torch.sqrt(a * q * (1 + e + a * q))) / (4 * a)) / ln2
    if kind == "mean":
        al = p["alpha"]
        return (2 * torch.asinh(torch.sqrt(al * q)) - float(np.log(al)) - float(np.log(4))) / ln2
    if kind == "spline":
        x, y, b, c, d = p["table_dev"]
        u = torch.asinh(q)
        i = (torch.searchsorted(x, u, right=True) - 1).clamp_(0, x.numel() - 1)
        dx = u - x[i]
        return p["eta"] * (y[i] + dx * (b[i] + dx * (c[i] + dx * d[i]))) + p["xi"]
    if kind == "log2":
        return torch.log2(q + p["pc"])
    return q


def bench_shape(name, reps, norm_matrix, warmup=3):
    import torch
    from deseq2_amd import core, native
    n, m = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(n + m)
    mu = torch.exp2(torch.randn(n, 1, device=dev, generator=g) * 2 + 7) * torch.exp(torch.randn(m, device=dev, generator=g) * 0.3)
    ld = native.gene_major_ld(m)
    yt = torch.zeros((n, ld), dtype=torch.int32, device=dev)
    yt[:, :m] = torch.poisson(mu, generator=g).to(torch.int32)
    y = native.GeneMajor(yt, m)
    sf = torch.exp(torch.randn(m, device=dev, dtype=torch.float64, generator=g) * 0.3)
    if norm_matrix:
        nft = torch.ones((n, ld), dtype=torch.float64, device=dev)
        nft[:, :m] = torch.exp(torch.randn((n, m), device=dev, dtype=torch.float64, generator=g) * 0.3)
        nf = native.GeneMajor(nft, m)
        nf_t = nf.view()
    else:
        nf, nf_t = sf, sf[None, :]
    flush = torch.zeros(64 * 1024 * 1024, dtype=torch.float64, device=dev)
    out = native.GeneMajor(torch.zeros((n, ld), dtype=torch.float64, device=dev), m)
    table = core.vst_spline_table(lambda v: 0.05 + 2.0 / v, float(yt.max()) / float(sf.min()) * 2, 1.0)
    params = {"parametric": dict(asymptDisp=0.05, extraPois=2.0), "mean": dict(alpha=0.07),
              "spline": dict(table=table, eta=0.4, xi=-1.0), "log2": dict(pc=1.0), "normalized": {}}
    traffic = (4.0 + 8.0 + (8.0 if norm_matrix else 0.0)) * n * m
    res = {"shape": name, "n": n, "m": m, "norm_matrix": bool(norm_matrix), "traffic_bytes": traffic}
    # the yardstick: a device-to-device copy that moves the same number of bytes (half read, half written)
    src = torch.empty(int(traffic // 16), dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    res["copy"] = _events(torch, lambda: dst.copy_(src), warmup, reps, flush)
    copy_rate = traffic / (res["copy"]["median_ms"] * 1e-3)
    res["copy_rate_TBps"] = copy_rate / 1e12
    del src, dst
    yv = y.view()
    for kind in KINDS:
        p = params[kind]
        r = {"device": _events(torch, lambda: native.vst_dev(y, nf, kind, out=out, **p), warmup, reps, flush)}
        tp = dict(p)
        if kind == "spline":
            tp["table_dev"] = [torch.as_tensor(row, device=dev) for row in table]
        ref = _torch_statement(torch, kind, yv, nf_t, tp)
        r["max_abs_diff_vs_torch"] = float((out.view() - ref).abs().max())
        del ref
        r["torch_ops"] = _events(torch, lambda: _torch_statement(torch, kind, yv, nf_t, tp), 2, max(5, reps // 4), flush)
        rate = traffic / (r["device"]["median_ms"] * 1e-3)
        r["rate_TBps"] = rate / 1e12
        r["fraction_of_copy_rate"] = rate / copy_rate
        r["torch_fraction_of_copy_rate"] = traffic / (r["torch_ops"]["median_ms"] * 1e-3) / copy_rate
        r["speedup_vs_torch_ops"] = r["torch_ops"]["median_ms"] / r["device"]["median_ms"]
        res[kind] = r
    res["rowstats"] = _events(torch, lambda: native.vstRowStats_dev(y, nf), warmup, reps, flush)
    return res


def bench_e2e(reps=5):
    """core.vst on C3, size factors given, wall clock around a synchronised call; the engine's timing hooks give the device
    time of every launch, of which everything but vst_transform / vst_rowstats belongs to the 1 000-gene dispersion fit"""
    import torch
    from deseq2_amd import core, simulate
    from deseq2_amd.engine import DeviceEngine
    n, m = SHAPES["C3"]
    x = simulate.design_two_group(m)
    d = simulate.make_counts(n, x, seed=3, intercept_mean=6.0)
    E = DeviceEngine()
    sf = np.exp(np.random.default_rng(1).normal(0, 0.2, m))
    dds0 = core.DESeqDataSet(d["counts"], x, sizeFactors=sf, engine=E)
    ts = []
    for i in range(reps + 1):
        dds = core._shallow(dds0)
        dds.dispersionFunction = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = core.vst(dds)
        torch.cuda.synchronize()
        if i:
            ts.append(time.perf_counter() - t0)
    E.record = []
    dds = core._shallow(dds0)
    dds.dispersionFunction = None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = core.vst(dds)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    rec, E.record = E.record, None
    own = sum(ms for nm, _, ms in rec if nm.startswith("vst_"))
    fit = sum(ms for nm, _, ms in rec if not nm.startswith("vst_"))
    return {"vst_C3": {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)),
                       "profiled_wall_s": wall, "device_ms_transform_and_rowstats": own, "device_ms_dispersion_fit": fit,
                       "fitType": t.dds.dispersionFunction["fitType"], "launches": [nm for nm, _, _ in rec]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="C3,C4")
    ap.add_argument("--norm-matrix", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "vst_bench.py measures on the GPU only"
    for s in a.shapes.split(","):
        print(json.dumps(bench_shape(s, a.reps, False)), flush=True)
        if a.norm_matrix:
            print(json.dumps(bench_shape(s, a.reps, True)), flush=True)
    if a.e2e:
        print(json.dumps(bench_e2e()), flush=True)


if __name__ == "__main__":
    main()
