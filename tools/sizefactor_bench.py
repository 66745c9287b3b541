"""Timing of estimateSizeFactors on the device (dsq_size_factors_dev, csrc/size_factors.hip) on resident matrices of the
C3 (50 000 x 500) and C4 (60 000 x 2 000) shapes, against two yardsticks that are not the code under test:
  (a) the same quantity with stock torch ops on the same resident tensors (log, row mean, masked per-column nanmedian),
  (b) the numpy statement on the host (HostEngine.size_factors).
HIP events, warm-up, >= 20 repetitions, median and spread; one JSON line per shape.  The bandwidth figure is the
algorithmic traffic -- 9 sweeps over the 4 n m bytes of counts (loggeomeans + 8 selection passes; d_ij is recomputed in
every pass, no keys are stored) -- over the median time, as a fraction of the 8 TB/s HBM peak.

    python tools/sizefactor_bench.py [--reps 20] [--shapes C3,C4] [--chain]

--chain also times one C3 fused.DESeq step with sfType="ratio" against sfType=None on the same library."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"C3": (50000, 500), "C4": (60000, 2000)}
HBM_PEAK = 8.0e12


def _events(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "iqr_ms": float(np.subtract(*np.percentile(ms, [75, 25]))), "reps": int(reps)}


def _torch_statement(torch, y):
    logk = torch.log(y.to(torch.float64))
    lgm = logk.mean(dim=1)
    keep = torch.isfinite(lgm)[:, None] & (y > 0)
    d = torch.where(keep, logk - lgm[:, None], torch.full((), float("nan"), dtype=torch.float64, device=y.device))
    return torch.exp(torch.nanmedian(d, dim=0).values)


def bench_shape(name, reps, warmup=3):
    import torch
    from deseq2_amd import native
    from deseq2_amd.engine import HostEngine
    n, m = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(n + m)
    mu = torch.exp2(torch.randn(n, 1, device=dev, generator=g) * 2 + 7) * torch.exp(torch.randn(m, device=dev, generator=g) * 0.3)
    ld = native.gene_major_ld(m)
    yt = torch.zeros((n, ld), dtype=torch.int32, device=dev)
    yt[:, :m] = torch.poisson(mu, generator=g).to(torch.int32)
    y = native.GeneMajor(yt, m)
    wsb = int(native.L.lib().dsq_size_factors_workspace_bytes(n, m))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = {"shape": name, "n": n, "m": m}
    r = native.sizeFactors_dev(y, workspace=ws)
    sf = r["sizeFactors"].cpu().numpy()
    out["device"] = _events(torch, lambda: native.sizeFactors_dev(y, workspace=ws), warmup, reps)
    yv = y.view()
    ref_t = _torch_statement(torch, yv).cpu().numpy()
    out["torch_ops"] = _events(torch, lambda: _torch_statement(torch, yv), 2, max(5, reps // 4))
    kh = yv.cpu().numpy()
    t0 = time.perf_counter()
    ref_h = HostEngine(native).size_factors(kh)["sizeFactors"]
    out["numpy_host_s"] = time.perf_counter() - t0
    out["max_rel_diff_vs_numpy"] = float(np.max(np.abs(sf / ref_h - 1)))
    out["max_rel_diff_vs_torch_lower_median"] = float(np.max(np.abs(sf / ref_t - 1)))
    traffic = 9 * 4.0 * n * m
    out["traffic_bytes"] = traffic
    out["hbm_fraction"] = traffic / (out["device"]["median_ms"] * 1e-3) / HBM_PEAK
    out["speedup_vs_torch_ops"] = out["torch_ops"]["median_ms"] / out["device"]["median_ms"]
    out["speedup_vs_numpy_host"] = out["numpy_host_s"] * 1e3 / out["device"]["median_ms"]
    return out


def bench_chain(reps=5):
    """one C3 fused.DESeq step with and without sfType="ratio" (wall clock around a synchronised step)"""
    import torch
    from deseq2_amd import core, fused, simulate
    from deseq2_amd.engine import DeviceEngine
    n, m = SHAPES["C3"]
    x = simulate.design_two_group(m)
    d = simulate.make_counts(n, x, seed=3)
    E = DeviceEngine()
    res = {}
    for label, kw in (("sfType_none", {}), ("sfType_ratio", {"sfType": "ratio"})):
        ts = []
        for i in range(reps + 1):
            dds = core.DESeqDataSet(d["counts"], x, sizeFactors=None if kw else np.ones(m), engine=E)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fused.DESeq(dds, **kw)
            torch.cuda.synchronize()
            if i:
                ts.append(time.perf_counter() - t0)
        res[label] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}
    res["added_s"] = res["sfType_ratio"]["median_s"] - res["sfType_none"]["median_s"]
    return {"chain_C3": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="C3,C4")
    ap.add_argument("--chain", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "sizefactor_bench.py measures on the GPU only"
    for s in a.shapes.split(","):
        print(json.dumps(bench_shape(s, a.reps)), flush=True)
    if a.chain:
        print(json.dumps(bench_chain()), flush=True)


if __name__ == "__main__":
    main()
