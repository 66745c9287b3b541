#!/usr/bin/env python
"""Times the sample PCA / sample distance kernels (csrc/explore.hip) on resident float64 matrices at the sizes the project is
built for, against the same quantities in stock torch ops on the same device and in numpy / scipy on the host
(profiles/explore.md).

    python tools/explore_bench.py [--shapes 20000x48,50000x500,60000x2000] [--reps 3] [--host-pair-rows 2e10] [--out FILE]

  ours      device events around dsq_top_var_dev (row_vars_kernel + keys + radix sort + take, ntop = 500), around
            dsq_sample_pairs_dev for the Gram of the 500 selected rows, and around it for the full `dist`; warm, the median of
            --reps after one warm-up call
  torch     torch.var(dim = 1) + torch.topk(500); the matmul of the centred selection; torch.cdist(x^T, x^T,
            compute_mode = "donot_use_mm_for_euclid_dist") on a contiguous m x n copy made outside the timed window; device
            events, warm, one warm-up call each
  host      numpy.var(ddof = 1) + argsort; the centred selection's cross-product; scipy pdist -- the latter only while
            n m (m - 1) / 2 <= --host-pair-rows (else "not measured"); numpy.linalg.eigh of the m x m Gram matrix (the
            host step of pca on both engines)
  share     for `dist`: 3 f64 operations (subtract, multiply, add) per row and per pair i <= j over the device time, against
            the 78.6 TF f64 vector peak the README quotes (which counts a fused multiply-add as two)
Inputs are drawn on the device from a seed.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F64_VECTOR_PEAK = 78.6e12
NTOP = 500


def make_input(torch, n, m, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ld = (m + 7) & ~7
    x = torch.zeros((n, ld), dtype=torch.float64, device="cuda")
    level = 8.0 + 3.0 * torch.randn((n, 1), generator=g, device="cuda", dtype=torch.float64)
    spread = 0.05 + torch.rand((n, 1), generator=g, device="cuda", dtype=torch.float64)
    group = (torch.arange(m, device="cuda") * 3 // m).to(torch.float64)[None, :]
    effect = torch.randn((n, 1), generator=g, device="cuda", dtype=torch.float64) * (torch.rand((n, 1), generator=g, device="cuda") < 0.1)
    x[:, :m] = level + effect * group + spread * torch.randn((n, m), generator=g, device="cuda", dtype=torch.float64)
    return x


def device_ms(torch, fn, reps):
    """median of `reps` event-timed calls after one warm-up; the last result"""
    times, out = [], None
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], [round(t, 3) for t in times], out


def host_s(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x48,50000x500,60000x2000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-pair-rows", type=float, default=2e10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scipy.spatial.distance import pdist
    from deseq2_amd import native
    if not torch.cuda.is_available():
        raise SystemExit("explore_bench.py measures on the GPU: none found")
    lines = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        x = make_input(torch, n, m, seed=n + m)
        X = native.GeneMajor(x, m)
        xv = x[:, :m]
        rec = {"n": n, "m": m, "ntop": NTOP}
        # ours
        rec["ours_top_var_ms"], rec["ours_top_var_ms_all"], tv = device_ms(torch, lambda: native.top_var_dev(X, NTOP), a.reps)
        rows = tv["select"]
        centre = tv["rowMean"].index_select(0, rows.to(torch.int64))
        rec["ours_gram_ms"], rec["ours_gram_ms_all"], G = device_ms(
            torch, lambda: native.sample_pairs_dev(X, "gram", rows=rows, centre=centre), a.reps)
        rec["ours_dist_ms"], rec["ours_dist_ms_all"], D = device_ms(torch, lambda: native.sample_pairs_dev(X, "dist"), a.reps)
        ops = 3.0 * n * (m * (m + 1) / 2.0)
        rec["dist_f64_ops"] = ops
        rec["dist_share_of_f64_vector_peak"] = ops / (rec["ours_dist_ms"] * 1e-3) / F64_VECTOR_PEAK
        # torch
        def t_var():
            v = torch.var(xv, dim=1)
            return v, torch.topk(v, NTOP).indices
        rec["torch_var_topk_ms"], _, (tvar, tsel) = device_ms(torch, t_var, a.reps)

        def t_gram():
            c = xv.index_select(0, tsel)
            c = c - c.mean(dim=1, keepdim=True)
            return c.T @ c
        rec["torch_gram_ms"], _, TG = device_ms(torch, t_gram, a.reps)
        xt = xv.T.contiguous()
        torch_reps = a.reps if n * m * m < 5e10 else 1
        rec["torch_cdist_ms"], _, TD = device_ms(
            torch, lambda: torch.cdist(xt, xt, compute_mode="donot_use_mm_for_euclid_dist"), torch_reps)
        rec["torch_cdist_reps"] = torch_reps
        off = ~torch.eye(m, dtype=torch.bool, device="cuda")
        rec["dist_max_rel_diff_vs_torch"] = float(((D - TD).abs()[off] / TD[off]).max().item())
        rec["var_max_rel_diff_vs_torch"] = float(((tv["rowVar"] - tvar).abs() / tvar).max().item())
        rec["ours_dist_over_torch_cdist"] = rec["ours_dist_ms"] / rec["torch_cdist_ms"]
        rec["ours_gram_over_torch_gram"] = rec["ours_gram_ms"] / rec["torch_gram_ms"]
        del xt, TD
        # host
        A = xv.cpu().numpy()
        rec["host_var_argsort_s"], (hv, hsel) = host_s(lambda: (lambda v: (v, np.argsort(-v, kind="stable")[:NTOP]))(np.var(A, axis=1, ddof=1)))

        def h_gram():
            c = A[hsel]
            c = c - c.mean(axis=1, keepdims=True)
            return c.T @ c
        rec["host_gram_s"], _ = host_s(h_gram)
        if n * m * (m - 1) / 2.0 <= a.host_pair_rows:
            rec["host_pdist_s"], _ = host_s(lambda: pdist(A.T))
        else:
            rec["host_pdist_s"] = "not measured"
        Gh = G.cpu().numpy()
        rec["host_eigh_s"], _ = host_s(lambda: np.linalg.eigh(Gh))
        rec["assay_bytes"] = n * m * 8
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, X, xv, A
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
