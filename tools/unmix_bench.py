#!/usr/bin/env python
"""Times dsq_unmix_dev (csrc/unmix.hip) at the sizes the project is built for, against the same quantity in stock torch ops
on the same device and against R's optim call restated through scipy on the host (profiles/unmix.md).

    python tools/unmix_bench.py [--shapes 20000x500x8,60000x2000x16] [--reps 3] [--lbfgsb-samples 2] [--out FILE]

  ours      dsq_unmix_dev on resident inputs: device events around the call (preparation kernel + fit kernel), the
            median of --reps after one warm-up; the distribution of the iteration counts and of the flags
  torch     a batched reweighted Gauss-Newton iteration on the same objective and box: f = pure p, r, J, A = J'WJ, b = J'Wr
            by einsum over chunks of samples, (A + lambda diag A) d = b by torch.linalg.solve, p <- clip(p + d), with a fixed
            lambda and no acceptance test, run for the MEDIAN number of iterations ours took: time per iteration and total;
            the mean loss it reaches is printed beside ours (it is not the same iteration: the comparison is of time for the
            same kind of work, as profiles/results.md does for results())
  lbfgsb    tests/unmix_lbfgsb.py on the first --lbfgsb-samples samples, on the host: seconds per sample, and the loss
Inputs are mixtures drawn on the device from a seed.  One JSON line per (shape, power)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LN2 = float(np.log(2.0))


def make_inputs(torch, n, m, k, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    torch.manual_seed(seed)                                   # (the Dirichlet weights are drawn on the host)
    base = torch.round(400.0 * torch.rand((n, k), generator=g, device="cuda", dtype=torch.float64) ** 2)
    base[torch.rand((n, k), generator=g, device="cuda") < 0.2] = 0.0
    w = torch.distributions.Dirichlet(torch.ones(k, dtype=torch.float64)).sample((m,)).to("cuda")
    ld = (m + 7) & ~7
    x = torch.zeros((n, ld), dtype=torch.float64, device="cuda")
    x[:, :m] = torch.poisson(1.5 * base @ w.T, generator=g)
    return x, base.contiguous()


def v_torch(torch, q, alpha):
    z = torch.sqrt(alpha * q)
    return (2.0 * torch.asinh(z) - np.log(alpha) - np.log(4.0)) / LN2, alpha / (LN2 * z * torch.sqrt(z * z + 1.0))


def torch_gauss_newton(torch, x, pure, m, alpha, power, iters, chunk, lam=1e-3):
    """p (m x k) and the loss after `iters` steps; stock ops only"""
    n, k = pure.shape
    P = torch.ones((m, k), dtype=torch.float64, device="cuda")
    loss = torch.zeros(m, dtype=torch.float64, device="cuda")
    eye = torch.eye(k, dtype=torch.float64, device="cuda")
    for s0 in range(0, m, chunk):
        s1 = min(m, s0 + chunk)
        target = v_torch(torch, x[:, s0:s1], alpha)[0].T.contiguous()              # (c, n)
        p = P[s0:s1]
        for _ in range(iters + 1):
            f = p @ pure.T                                                         # (c, n)
            vf, slope = v_torch(torch, f, alpha)
            r = target - vf
            loss[s0:s1] = (r.abs() if power == 1 else r * r).sum(dim=1)
            w = 1.0 / r.abs().clamp_min(1e-8) if power == 1 else torch.ones_like(r)
            live = torch.isfinite(slope)
            wd = torch.where(live, w * slope * slope, 0.0)                         # (c, n): w v'^2
            A = torch.einsum("cn,ni,nj->cij", wd, pure, pure)
            b = torch.einsum("cn,ni->ci", torch.where(live, w * slope * r, 0.0), pure)
            M = A + lam * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)) + 1e-300 * eye
            d = torch.linalg.solve(M, b)
            p = (p + d).clamp(1e-6, 100.0)
        P[s0:s1] = p
    return P, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x500x8,60000x2000x16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lbfgsb-samples", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from deseq2_amd import native
    from tests import unmix_lbfgsb
    lines = []
    for shape in a.shapes.split(","):
        n, m, k = (int(v) for v in shape.split("x"))
        x, pure = make_inputs(torch, n, m, k, seed=n + m + k)
        X = native.GeneMajor(x, m)
        ws = torch.empty(n * m * 8, dtype=torch.uint8, device="cuda")
        for power in (2, 1):
            times = []
            for rep in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = native.unmix_dev(X, pure, alpha=a.alpha, power=power, workspace=ws)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1))
            it, flag, loss = r["iter"].cpu().numpy(), r["flag"].cpu().numpy(), r["loss"].cpu().numpy()
            med = int(np.median(it))
            chunk = max(1, min(m, (1 << 28) // (n * k)))
            torch_gauss_newton(torch, x, pure, min(m, chunk), a.alpha, power, 1, chunk)          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, tl = torch_gauss_newton(torch, x, pure, m, a.alpha, power, med, chunk)
            torch.cuda.synchronize()
            t_torch = time.perf_counter() - t0
            rec = {"n": n, "m": m, "k": k, "power": power, "alpha": a.alpha, "ours_ms": sorted(times)[len(times) // 2],
                   "ours_ms_all": [round(t, 3) for t in times],
                   "iter_quantiles_0_25_50_75_100": [int(v) for v in np.quantile(it, [0, .25, .5, .75, 1])],
                   "iter_mean": float(it.mean()), "flags_0_1_2": [int((flag == f).sum()) for f in (0, 1, 2)],
                   "loss_mean": float(loss.mean()), "torch_iters": med, "torch_ms": 1e3 * t_torch,
                   "torch_ms_per_iter": 1e3 * t_torch / (med + 1), "torch_loss_mean": float(tl.mean().item()),
                   "torch_chunk": chunk}
            if a.lbfgsb_samples > 0:
                s = min(m, a.lbfgsb_samples)
                xh, ph = x[:, :s].cpu().numpy(), pure.cpu().numpy()
                t0 = time.perf_counter()
                ref = unmix_lbfgsb.unmix_lbfgsb(xh, ph, alpha=a.alpha, power=power)
                rec["lbfgsb_s_per_sample"] = (time.perf_counter() - t0) / s
                ours = [unmix_lbfgsb.sum_loss(r["p"][i].cpu().numpy(), xh[:, i], ph, alpha=a.alpha, power=power) for i in range(s)]
                rec["lbfgsb_loss"], rec["ours_loss_same_samples"] = [float(v) for v in ref["loss"]], [float(v) for v in ours]
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
