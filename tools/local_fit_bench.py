#!/usr/bin/env python
"""Times the local-regression dispersion trend (csrc/local_fit.hip, fitType = "local") on resident vectors at the sizes the
project is built for, against the same estimator in stock torch ops on the same device and against the numpy specification
on the host (profiles/local_fit.md).

    python tools/local_fit_bench.py [--shapes 20000,50000,60000] [--reps 5] [--inner 3] [--spec-points 8] [--out FILE]

  A shape is N = n: n genes, all of them in the fit set, the trend evaluated at every gene's mean.
  ours      device events around --inner back-to-back calls of dsq_local_fit_dev: the fit alone (keys, radix sort, gather)
            and the evaluation of a kept fit handle at the n means; warm, the median of --reps windows after one warm-up
            window, divided by --inner
  torch     the same estimator in stock ops, timed the same way.  Fit: log, sort, gather.  Evaluation, in batches of 512
            points: the k-th smallest |x - z| by kthvalue over the 512 x N distances, the tricube weights, the eight sums by
            sum(dim = 1), torch.linalg.solve on the 3 x 3 systems, exp
  spec      tests/local_fit_spec.py on the host at --spec-points of the means, per point, and that figure times n (an
            extrapolation, said so in the output: the whole list would take hours)
  work      23 f64 operations per window point (the division counted as one: it is a dozen instructions), k n window
            points; over the time, as a share of the 78.6 TF f64 vector peak (which counts a fused multiply-add as two,
            and this kernel has none: half of it is the most it could reach).  Also the bytes of the fit block the waves
            read (24 k n: every evaluation point reads its own window) over the time
  copy      a device-to-device copy of 1 GiB of float64 (read + write = 2 GiB moved), timed the same way
The device's values are compared with torch's by the largest relative difference.  Inputs are drawn on the device from a
seed.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOPS_PER_POINT = 23.0
F64_VECTOR_PEAK = 78.6e12


def window_ms(torch, fn, reps, inner):
    """median over `reps` event-timed windows of `inner` calls, after one warm-up window; per call"""
    times = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1) / inner)
    return sorted(times)[len(times) // 2], [round(t, 4) for t in times]


def torch_fit(torch, means, disps):
    x, o = torch.sort(torch.log(means), stable=True)
    return x, torch.log(disps)[o], means[o]


def torch_eval(torch, fit, q, k, batch=512):
    x, y, w = fit
    out = torch.empty_like(q)
    for b in range(0, q.numel(), batch):
        z = torch.log(q[b:b + batch])[:, None]
        d = x[None, :] - z
        h = torch.kthvalue(d.abs(), k, dim=1).values[:, None]
        t = d / h
        a = t.abs()
        W = torch.where(a < 1, w[None, :] * (1 - a ** 3) ** 3, torch.zeros_like(a))
        p = [W]
        for _ in range(4):
            p.append(p[-1] * t)
        S = [v.sum(dim=1) for v in p]
        T = torch.stack([(v * y[None, :]).sum(dim=1) for v in p[:3]], dim=1)
        G = torch.stack([torch.stack([S[i + j] for j in range(3)], dim=1) for i in range(3)], dim=1)
        out[b:b + batch] = torch.exp(torch.linalg.solve(G, T)[:, 0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000,50000,60000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--spec-points", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from deseq2_amd import native
    from oracle import oracle as O
    from tests import local_fit_spec as S
    if not torch.cuda.is_available():
        raise SystemExit("local_fit_bench.py measures on the GPU: none found")
    src = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    copy_ms, copy_all = window_ms(torch, lambda: dst.copy_(src), a.reps, 10)
    copy_rate = 2.0 * src.numel() * 8 / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()
    lines = []
    for shape in a.shapes.split(","):
        n = int(shape)
        g = torch.Generator(device="cuda").manual_seed(n)
        means = torch.exp(torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * np.log(1e5))
        disps = (0.05 + 3.0 / means) * torch.exp(0.3 * torch.randn(n, generator=g, device="cuda", dtype=torch.float64))
        k = S.bandwidth(n)
        rec = {"N": n, "n_eval": n, "k": k, "copy_rate_TB_s": copy_rate / 1e12, "copy_ms_all": copy_all}
        # ---- ours
        built = native.local_fit_dev(means, disps, 1e-8, evaluate=False)
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        fit_ms, fit_all = window_ms(torch, lambda: native.local_fit_dev(means, disps, 1e-8, evaluate=False), a.reps, a.inner)
        ev_ms, ev_all = window_ms(torch, lambda: native.local_fit_dev(fit=built["fit"], eval_means=means, minDisp=1e-8, out=out),
                                  a.reps, a.inner)
        st = native.local_fit_dev(fit=built["fit"], eval_means=means, minDisp=1e-8, out=out)["status"].cpu().numpy()
        flops = FLOPS_PER_POINT * k * n
        rec["ours"] = {"fit_ms": fit_ms, "fit_ms_all": fit_all, "eval_ms": ev_ms, "eval_ms_all": ev_all, "status": [int(v) for v in st],
                       "eval_TFLOP_s": flops / (ev_ms * 1e-3) / 1e12, "share_of_f64_vector_peak": flops / (ev_ms * 1e-3) / F64_VECTOR_PEAK,
                       "fit_block_reads_GB": 24.0 * k * n / 1e9, "fit_block_read_rate_TB_s": 24.0 * k * n / (ev_ms * 1e-3) / 1e12}
        # ---- stock torch
        tfit = torch_fit(torch, means, disps)
        tf_ms, _ = window_ms(torch, lambda: torch_fit(torch, means, disps), a.reps, a.inner)
        te_ms, te_all = window_ms(torch, lambda: torch_eval(torch, tfit, means, k), 2, 1)
        ref = torch_eval(torch, tfit, means, k)
        rec["torch"] = {"fit_ms": tf_ms, "eval_ms": te_ms, "eval_ms_all": te_all,
                        "max_rel_diff_ours_vs_torch": float(((out - ref).abs() / ref.abs()).max().item())}
        # ---- the numpy specification on the host, at a few points
        hm, hd = means.cpu().numpy(), disps.cpu().numpy()
        t0 = time.perf_counter()
        sfit = S.local_fit(O, hm, hd, 1e-8)
        t1 = time.perf_counter()
        pts = np.linspace(0, n - 1, a.spec_points).astype(np.int64)
        sv, _ = S.evaluate(O, sfit, hm[pts])
        t2 = time.perf_counter()
        dev = out.cpu().numpy()[pts]
        rec["spec"] = {"fit_ms": (t1 - t0) * 1e3, "eval_ms_per_point": (t2 - t1) * 1e3 / pts.size, "points_timed": int(pts.size),
                       "eval_ms_extrapolated_to_n": (t2 - t1) * 1e3 / pts.size * n,
                       "device_equals_spec_at_those_points": bool((dev.view(np.uint64) == sv.view(np.uint64)).all())}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del means, disps, out, ref, tfit, built
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
