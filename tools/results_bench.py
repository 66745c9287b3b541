"""Timing of results() on the device (dsq_results_dev, csrc/results.hip) on resident columns: n = 50 000 and 60 000 genes,
K = 50 filter thresholds, p-values with 10 % NA, baseMean with 5 % zeros as the filter.  Next to it, in the same run:
  - the same quantity with stock torch ops on the same resident tensors (torch.quantile, torch.sort, cumsum, cummin,
    scatter): the baseline a user without the kernels would write;
  - the numpy specification on the host (tests/results_spec.py: one p.adjust per threshold, as R runs it).
HIP events around the device paths (warm-up, >= 20 repetitions, median and spread, a 512 MB buffer rewritten between
repetitions so that no input is served from the last-level cache), a host clock around the numpy statement.  The three
results are compared before anything is timed.  One JSON line per n.

    python tools/results_bench.py [--reps 20] [--n 50000,60000] [--K 50] [--no-host]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/results_bench.py --reps 5 --no-host`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def torch_statement(torch, p, f, theta, alpha):
    """filtered_p with p.adjust(., "BH") over all thresholds from one torch.sort; returns (filtPadj K x n, numRej)"""
    n, K = p.numel(), theta.numel()
    inf = float("inf")
    cut = torch.quantile(f, theta)                       # (linear interpolation: type 7)
    isna = torch.isnan(p)
    ps, order = torch.sort(torch.where(isna, torch.full_like(p, inf), p))
    nv = n - int(isna.sum())
    valid = torch.arange(n, device=p.device) < nv
    use = (f[order][None, :] >= cut[:, None]) & valid[None, :]
    r = torch.cumsum(use, dim=1)
    mS = r[:, -1:].to(torch.float64)
    v = torch.where(use, (mS / r.clamp(min=1).to(torch.float64)) * ps[None, :], torch.full((), inf, dtype=torch.float64, device=p.device))
    suf = torch.flip(torch.cummin(torch.flip(v, [1]), dim=1).values, [1])
    padj = torch.where(use, suf.clamp(max=1.0), torch.full((), float("nan"), dtype=torch.float64, device=p.device))
    out = torch.empty((K, n), dtype=torch.float64, device=p.device)
    out.scatter_(1, order[None, :].expand(K, n), padj)
    return out, (out < alpha).sum(dim=1)


def bench(n, K, reps, host, warmup=3):
    import torch
    from deseq2_amd import native
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(n + K)
    lfc = rng.normal(0, 1.5, n)
    se = np.exp(rng.normal(-1, 0.5, n))
    stat = lfc / se
    pv = rng.uniform(size=n) ** 2
    pv[rng.uniform(size=n) < 0.1] = np.nan
    bm = np.exp(rng.normal(4, 2, n))
    bm[rng.uniform(size=n) < 0.05] = 0.0
    lo = float(np.mean(bm == 0))
    theta = np.linspace(lo, 0.95, K)
    alpha = 0.1
    t = lambda a: torch.as_tensor(a, device=dev)
    d = {k: t(v) for k, v in dict(lfc=lfc, se=se, stat=stat, pv=pv, bm=bm, theta=theta).items()}
    flush = torch.zeros(64 * 1024 * 1024, dtype=torch.float64, device=dev)

    def ours():
        return native.results_dev(d["lfc"], d["se"], d["stat"], d["pv"], d["bm"], 0, theta=d["theta"], alpha=alpha)

    def stock():
        return torch_statement(torch, d["pv"], d["bm"], d["theta"], alpha)
    r = ours()
    torch.cuda.synchronize()
    got = r["filtPadj"].cpu().numpy()
    cut, nrej, status = native.results_small(r["_small"].cpu().numpy(), K)
    assert status == 0
    so, sn = stock()
    same = lambda a, b: bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    out = {"n": n, "K": K, "alpha": alpha, "device": torch.cuda.get_device_name(0),
           "torch_equals_device": same(so.cpu().numpy(), got) and bool((sn.cpu().numpy() == nrej).all()),
           "numRej_max": int(nrej.max())}
    if host:
        from oracle import oracle as O
        from tests import results_spec as S
        t0 = time.perf_counter()
        ref = S.results(O, lfc, se, stat, pv, bm, theta=theta, alpha=alpha)
        out["numpy_spec_host_ms"] = (time.perf_counter() - t0) * 1e3
        out["spec_equals_device"] = same(ref["filtPadj"], got.T) and bool((ref["numRej"] == nrej).all()) and same(ref["cutoffs"], cut)
    out["dsq_results_dev"] = _events(torch, ours, warmup, reps, flush)
    out["torch_statement"] = _events(torch, stock, warmup, reps, flush)
    out["speedup_vs_torch"] = out["torch_statement"]["median_ms"] / out["dsq_results_dev"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", default="50000,60000")
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("results_bench needs a GPU: a CPU run gives no time")
    for n in (int(v) for v in a.n.split(",")):
        print(json.dumps(bench(n, a.K, a.reps, not a.no_host)), flush=True)


if __name__ == "__main__":
    main()
