"""Timing of K contrasts from one covariance pass per gene (dsq_contrasts_dev, csrc/contrasts.hip) on resident data, next to
what a user could do before it existed: K launches of dsq_fit_beta_dev with maxit = 0, without hat diagonals or fitted
means, one per contrast (getContrast, R/results.R:797-807).  Both read the same resident tensors and both are consumed
inside the timed region (a device-side sum over the outputs).  The two results are compared bit for bit before anything is
timed.  HIP events, warm-up, >= 10 repetitions, median and spread, a 512 MB buffer rewritten between repetitions so that no
input is served from the last-level cache.  One JSON line per (shape, K).

    python tools/contrasts_bench.py [--reps 10] [--only factor10,paired32,factor48,C3] [--n 20000]

Shapes: 20 000 x 60 with a 10-level factor (K = 45: all pairs, and K = 1); 20 000 x 62 ~ patient + treatment with 30 patients
(p = 32 after the intercept and the treatment; K = 1, 8); 20 000 x 96 with a 48-level factor (K = 1, 47); C3 = 50 000 x 500
~ batch + condition (p = 4; K = 1, 6)."""
import argparse
import hashlib
import json
import os
import sys

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


def _shape(name, n):
    from deseq2_amd import simulate
    if name == "factor10":
        x = simulate.design_factor(60, 10)
        pairs = [(a, b) for a in range(10) for b in range(a + 1, 10)]
        return n, x, pairs, (45, 1)
    if name == "paired32":
        m = 62
        pat, trt = np.arange(m) % 31, np.arange(m) // 31          # 31 patients x 2 treatments: 1 + 30 + 1 = 32 columns
        x = np.column_stack([np.ones(m)] + [(pat == a) for a in range(1, 31)] + [trt == 1]).astype(np.float64)
        pairs = [(a, b) for a in range(1, 9) for b in (31,)]
        return n, x, pairs, (1, 8)
    if name == "factor48":
        x = simulate.design_factor(96, 48)
        return n, x, [(0, b) for b in range(1, 48)], (1, 47)
    if name == "C3":
        x = simulate.design_batch_condition(500)
        return 50000, x, [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], (1, 6)
    raise SystemExit("unknown shape " + name)


def _contrast_matrix(p, pairs):
    """level a against level b of a treatment-coded factor (level 0 is the intercept's)"""
    c = np.zeros((p, len(pairs)))
    for k, (a, b) in enumerate(pairs):
        if b:
            c[b, k] += 1.0
        if a:
            c[a, k] -= 1.0
    return c


def bench(name, n, reps, warmup=2):
    import torch
    from deseq2_amd import native
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine()
    dev = E.device
    n, x, pairs, Ks = _shape(name, n)
    m, p = x.shape
    rng = np.random.default_rng(len(name) + n)
    beta = np.column_stack([rng.normal(3.0, 1.5, n)] + [rng.normal(0, 0.5, n) for _ in range(p - 1)])
    sf = np.exp(rng.normal(0, 0.2, m))
    alpha = np.exp(rng.normal(-2, 1, n))
    lam = np.full(p, 1e-6 / np.log(2) ** 2)
    mu = sf[None, :] * np.exp(beta @ x.T)
    y = E.counts(rng.poisson(np.minimum(mu, 1e6)).astype(np.int32))
    xd = E.design(x)
    cells = E._cells.get(xd.data_ptr())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    sfd, ad, bd, ld_ = t(sf), t(alpha), t(beta.T), t(lam)
    flush = torch.zeros(64 * 1024 * 1024, dtype=torch.float64, device=dev)
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deseq2_amd", "libdeseq2_mi355x.so")
    digest = hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]
    out = []
    for K in Ks:
        c = _contrast_matrix(p, pairs[:K])
        cd = t(c.T)

        def ours():
            r = native.contrasts_dev(xd, sfd, ad, bd, ld_, cd, minmu=0.5, nf_is_vector=True, cells=cells)
            return r["table"], r["table"].sum()

        def baseline():
            acc, keep = torch.zeros((), dtype=torch.float64, device=dev), []
            for k in range(K):
                r = native.fitBeta_dev(y, xd, sfd, ad, cd[k], bd, ld_, None, False, 1e-8, 0, False, 0.5, want_hat=False, want_mu=False,
                                       nf_is_vector=True, cells=cells)
                keep.append((r["contrast_num"], r["contrast_denom"]))
                acc = acc + r["contrast_num"].sum() + r["contrast_denom"].sum()
            return keep, acc
        tab, _ = ours()
        base, _ = baseline()
        torch.cuda.synchronize()
        L2E = 1.4426950408889634
        same = all(bool(torch.equal(tab[0][k], L2E * base[k][0]) and torch.equal(tab[1][k], L2E * base[k][1])) for k in range(K))
        res = {"shape": name, "n": n, "m": m, "p": p, "K": K, "cells": int(cells.max()) + 1, "device": torch.cuda.get_device_name(0),
               "library_sha256": digest, "equals_K_fit_beta_launches": same}
        res["dsq_contrasts_dev"] = _events(torch, ours, warmup, reps, flush)
        res["K_fit_beta_launches"] = _events(torch, baseline, warmup, reps, flush)
        res["speedup"] = res["K_fit_beta_launches"]["median_ms"] / res["dsq_contrasts_dev"]["median_ms"]
        out.append(res)
        print(json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="factor10,paired32,factor48,C3")
    ap.add_argument("--n", type=int, default=20000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contrasts_bench needs a GPU: a CPU run gives no time")
    for name in a.only.split(","):
        bench(name, a.n, a.reps)


if __name__ == "__main__":
    main()
