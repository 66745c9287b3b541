#!/usr/bin/env python
"""Times the count-helper kernels (csrc/count_helpers.hip) on resident int32 counts at the sizes the project is built for,
against the same quantities in stock torch ops on the same device and against the bytes each must move at the measured
HBM copy rate (profiles/count_helpers.md).

    python tools/count_helpers_bench.py [--shapes 20000x48,50000x500,60000x2000] [--reps 7] [--inner 20] [--out FILE]

  ours      device events around --inner back-to-back calls of dsq_collapse_dev (pairs of technical replicates, and the
            pattern 1-2-1-1), dsq_col_sums_dev and dsq_fpm_dev (the three kinds) through ctypes on preallocated outputs;
            warm, the median of --reps windows after one warm-up window, divided by --inner
  torch     the same quantity in stock ops, timed the same way: zeros(n, g, int64).index_add_(1, code, y.to(int64)) and,
            for the pairs, the strided gather-sum y[:, 0::2] + y[:, 1::2] in int64; y.sum(0, dtype = int64); the division
            chains 1e6 * (y / lib), 1e3 * (f / bp), (1e3 * f) / L in float64
  bytes     what the quantity must move: 4 n m in + 4 n g out (collapse), 4 n m (colSums), 4 n m in + 8 n m out (fpm,
            fpkm with basepairs), + 8 n m in (fpkm with avgTxLength); over the time, as a share of the copy rate
  copy      a device-to-device copy of 1 GiB of float64 (read + write = 2 GiB moved), timed the same way
Results are compared with torch's (integers exactly, quotients by the largest relative difference).  Inputs are drawn on the
device from a seed.  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def groups(np, m, pattern):
    """codes of the m samples: "pairs" (j // 2) or "1211" (group sizes 1, 2, 1, 1 repeating)"""
    if pattern == "pairs":
        return np.arange(m) // 2
    codes, c = [], 0
    while len(codes) < m:
        codes.extend([c] * (1, 2, 1, 1)[c % 4])
        c += 1
    return np.asarray(codes[:m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x48,50000x500,60000x2000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from deseq2_amd import _lib as L
    from deseq2_amd import native
    if not torch.cuda.is_available():
        raise SystemExit("count_helpers_bench.py measures on the GPU: none found")
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    copy_ms, copy_all = window_ms(torch, lambda: dst.copy_(src), a.reps, a.inner)
    copy_rate = 2.0 * src.numel() * 8 / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()
    lines = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(n + m)
        ld = native.gene_major_ld(m)
        yt = torch.zeros((n, ld), dtype=torch.int32, device="cuda")
        yt[:, :m] = torch.randint(0, 50000, (n, m), generator=g, device="cuda", dtype=torch.int32)
        yv = yt[:, :m]
        rec = {"n": n, "m": m, "copy_ms_per_GiB_moved": copy_ms / 2.0, "copy_rate_TB_s": copy_rate / 1e12, "copy_ms_all": copy_all}

        def share(nbytes, ms):
            return nbytes / copy_rate / (ms * 1e-3)
        # ---- collapse
        for pattern in ("pairs", "1211"):
            codes = groups(np, m, pattern)
            ng = int(codes.max()) + 1
            members = torch.as_tensor(np.argsort(codes, kind="stable").astype(np.int32), device="cuda")
            offsets = torch.as_tensor(np.concatenate([[0], np.cumsum(np.bincount(codes))]).astype(np.int32), device="cuda")
            ldo = native.gene_major_ld(ng)
            out = torch.zeros((n, ldo), dtype=torch.int32, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            ca = L.sized(L.DsqCollapseArgs, n=n, m=m, g=ng, ld=ld, y=yt.data_ptr(), members=members.data_ptr(), offsets=offsets.data_ptr())
            co = L.sized(L.DsqCollapseOut, ld=ldo, out=out.data_ptr(), status=status.data_ptr())
            ms, every = window_ms(torch, lambda: L.check(lib.dsq_collapse_dev(C.byref(ca), C.byref(co), st)), a.reps, a.inner)
            code_t = torch.as_tensor(codes, device="cuda")
            t_ms, _ = window_ms(torch, lambda: torch.zeros((n, ng), dtype=torch.int64, device="cuda").index_add_(1, code_t, yv.to(torch.int64)),
                                a.reps, a.inner)
            ref = torch.zeros((n, ng), dtype=torch.int64, device="cuda").index_add_(1, code_t, yv.to(torch.int64))
            nbytes = 4.0 * n * m + 4.0 * n * ng
            rec["collapse_" + pattern] = {"g": ng, "ours_ms": ms, "ours_ms_all": every, "torch_index_add_ms": t_ms, "bytes": nbytes,
                                          "share_of_copy_rate": share(nbytes, ms), "equal_to_torch": bool((out[:, :ng].to(torch.int64) == ref).all()),
                                          "status": int(status.item())}
            if pattern == "pairs" and m % 2 == 0:
                rec["collapse_pairs"]["torch_gather_sum_ms"], _ = window_ms(
                    torch, lambda: yv[:, 0::2].to(torch.int64) + yv[:, 1::2].to(torch.int64), a.reps, a.inner)
            del out, ref
        # ---- colSums
        sums = torch.empty(m, dtype=torch.int64, device="cuda")
        sa = L.sized(L.DsqColSumsArgs, n=n, m=m, ld=ld, y=yt.data_ptr())
        so = L.sized(L.DsqColSumsOut, sums=sums.data_ptr())
        ms, every = window_ms(torch, lambda: L.check(lib.dsq_col_sums_dev(C.byref(sa), C.byref(so), st)), a.reps, a.inner)
        t_ms, _ = window_ms(torch, lambda: yv.sum(0, dtype=torch.int64), a.reps, a.inner)
        rec["col_sums"] = {"ours_ms": ms, "ours_ms_all": every, "torch_sum_ms": t_ms, "bytes": 4.0 * n * m,
                           "share_of_copy_rate": share(4.0 * n * m, ms), "equal_to_torch": bool((sums == yv.sum(0, dtype=torch.int64)).all())}
        # ---- fpm / fpkm
        libsz = sums.to(torch.float64)
        bp = torch.randint(200, 9000, (n,), generator=g, device="cuda").to(torch.float64)
        tl = torch.zeros((n, ld), dtype=torch.float64, device="cuda")
        tl[:, :m] = 100.0 + 4000.0 * torch.rand((n, m), generator=g, device="cuda", dtype=torch.float64)
        tlv = tl[:, :m]
        fout = torch.zeros((n, ld), dtype=torch.float64, device="cuda")
        for kind, nbytes in (("fpm", 12.0 * n * m), ("fpkm_basepairs", 12.0 * n * m), ("fpkm_txlen", 20.0 * n * m)):
            fa = L.sized(L.DsqFpmArgs, n=n, m=m, ld=ld, y=yt.data_ptr(), kind=L.DSQ_FPM[kind], lib=libsz.data_ptr(),
                         basepairs=bp.data_ptr(), txlen=tl.data_ptr())
            fo = L.sized(L.DsqFpmOut, out=fout.data_ptr())
            ms, every = window_ms(torch, lambda: L.check(lib.dsq_fpm_dev(C.byref(fa), C.byref(fo), st)), a.reps, a.inner)

            def chain():
                f = 1e6 * (yv / libsz)
                if kind == "fpkm_basepairs":
                    return 1e3 * (f / bp[:, None])
                return (1e3 * f) / tlv if kind == "fpkm_txlen" else f
            t_ms, _ = window_ms(torch, chain, a.reps, a.inner)
            ref = chain()
            rec[kind] = {"ours_ms": ms, "ours_ms_all": every, "torch_chain_ms": t_ms, "bytes": nbytes, "share_of_copy_rate": share(nbytes, ms),
                         "max_rel_diff_vs_torch": float(((fout[:, :m] - ref).abs() / ref.abs().clamp_min(1e-300)).max().item())}
            del ref
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del yt, yv, tl, tlv, fout
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
