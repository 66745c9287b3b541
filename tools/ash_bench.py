#!/usr/bin/env python
"""Times adaptive shrinkage (dsq_ash_dev, csrc/ash.hip) at the sizes the project is measured at.

  ours      DeviceEngine-level: native.ash_dev on resident columns with a reused workspace, a host clock around the call (it
            ends in a stream synchronisation); iterations and read-backs per fit (2 per iteration + 2) from the outputs
  torch     the same sequential quadratic programme in stock torch ops on the same device, float64: L by elementwise ops, u by
            a matrix-vector product, the Gram matrix z'z by torch.matmul, the 32 trial points by one matmul; the K x K active-set
            solve on the host by the same routine (deseq2_amd/ash_host.qp); one column after the other
  numpy     the host statement (deseq2_amd/ash_host.fit) at C = 1
  copy      the device-to-device copy rate of the same run (256 MiB)

Shapes: n = 20 000 / 50 000 / 60 000, C = 1 and C = 45 (all pairs of a 10-level factor).  One JSON line per shape.
    python tools/ash_bench.py [--reps 5] [--shapes 20000,50000,60000] [--cols 1,45]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_fit(torch, b, s, sigma, maxit=100):
    from deseq2_amd import ash_host as H
    keep = torch.isfinite(b) & torch.isfinite(s) & (s > 0)
    b, s = b[keep], s[keep]
    n, K = b.numel(), sigma.numel()
    v = (s * s)[:, None] + (sigma * sigma)[None, :]
    l = -0.5 * torch.log(2 * np.pi * v) - 0.5 * (b * b)[:, None] / v
    L = torch.exp(l - l.max(dim=1, keepdim=True).values)
    x = np.full(K, 1.0 / K)
    ts = torch.as_tensor(H.step_sizes(), device=b.device)
    it = backs = 0

    def evaluate(x):
        xt = torch.as_tensor(x, device=b.device)
        u = L @ xt
        z = L / u[:, None]
        rec = torch.cat([(-torch.log(u).sum() / n + xt.sum()).reshape(1), 1.0 - z.sum(0) / n, ((z.T @ z) / n).reshape(-1)]).cpu().numpy()
        return rec[0], rec[1:1 + K], rec[1 + K:].reshape(K, K) + H.RIDGE * np.eye(K)
    phi, g, Hm = evaluate(x)
    backs += 1
    while g.min() < -H.STOP and it < maxit:
        it += 1
        d = H.qp(Hm, g, x)
        X = torch.clamp(torch.as_tensor(x, device=b.device)[None, :] + ts[:, None] * torch.as_tensor(d, device=b.device)[None, :], min=0.0)
        cand = (-torch.log(L @ X.T).sum(0) / n + X.sum(1)).cpu().numpy()
        backs += 1
        ok = np.flatnonzero(cand <= phi + H.SUFF_DECREASE * H.step_sizes() * float(g @ d))
        if ok.size == 0:
            break
        x = np.maximum(x + H.step_sizes()[ok[0]] * d, 0.0)
        phi, g, Hm = evaluate(x)
        backs += 1
    return x / x.sum(), it, backs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="20000,50000,60000")
    ap.add_argument("--cols", default="1,45")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import torch
    from deseq2_amd import _lib, native
    from deseq2_amd import ash_host as H
    from tests import ash_cases as AC
    dev = torch.device("cuda:0")
    buf = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        dst.copy_(buf)
    torch.cuda.synchronize()
    copy_gbs = 10 * 2 * buf.numel() / (time.perf_counter() - t0) / 1e9
    del buf, dst
    for n in (int(v) for v in a.shapes.split(",")):
        for C in (int(v) for v in a.cols.split(",")):
            cols = [AC.column(n, 1000 + c, m=48) for c in range(C)]
            b = torch.as_tensor(np.stack([c[0] for c in cols]), device=dev)
            s = torch.as_tensor(np.stack([c[1] for c in cols]), device=dev)
            ws = torch.empty(int(_lib.lib().dsq_ash_workspace_bytes(n, C)), dtype=torch.uint8, device=dev)
            r = native.ash_dev(b, s, threshold=1.0, workspace=ws)               # warm-up
            ours = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = native.ash_dev(b, s, threshold=1.0, workspace=ws)
                ours.append((time.perf_counter() - t0) * 1e3)
            iters, K = r["iter"].cpu().numpy(), r["K"].cpu().numpy()
            sig = r["sd"].cpu().numpy()
            backs = 2 * int(iters.max()) + 2
            tt = []
            for _ in range(max(1, a.reps // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tit = [torch_fit(torch, b[c], s[c], torch.as_tensor(sig[c, :K[c]], device=dev))[1] for c in range(C)]
                torch.cuda.synchronize()
                tt.append((time.perf_counter() - t0) * 1e3)
            out = {"n": n, "C": C, "K": [int(K.min()), int(K.max())], "iter": [int(iters.min()), int(iters.max())], "flags": int(r["flag"].sum()),
                   "readbacks": backs, "ours_ms": round(float(np.median(ours)), 3), "ours_all_ms": [round(v, 3) for v in ours],
                   "ms_per_readback": round(float(np.median(ours)) / backs, 4),
                   "torch_ms": round(float(np.median(tt)), 3), "torch_iter": [int(min(tit)), int(max(tit))],
                   "torch_over_ours": round(float(np.median(tt) / np.median(ours)), 2), "copy_GBps": round(copy_gbs, 1),
                   "workspace_MiB": round(ws.numel() / 2 ** 20, 1)}
            if C == 1 and not a.no_numpy:
                t0 = time.perf_counter()
                H.fit(native.unary, cols[0][0], cols[0][1], threshold=1.0)
                out["numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(out), flush=True)
            del ws, b, s


if __name__ == "__main__":
    main()
