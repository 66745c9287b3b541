#!/usr/bin/env python
"""Times apeglm shrinkage (csrc/apeglm.hip, core.lfcShrinkApeglm) on resident data at the sizes the project is built for,
against the same iteration batched in stock torch ops on the same device and against the numpy specification on the host
(profiles/apeglm.md).

    python tools/apeglm_bench.py [--shapes 20000x48x2,50000x500x4,60000x2000x10] [--reps 3] [--torch-reps 3] [--spec-rows 16] [--out FILE]

  A shape is n x m x p: n genes, m samples, an intercept, a two-level condition and p - 2 continuous covariates; counts drawn
  on the device from the model; both starts (init = the true coefficients plus noise, standing for the MLE); the prior scale
  by core.apeglm_prior_scale from that column.
  kernel    device events around one dsq_apeglm_dev call on resident inputs; warm, the median of --reps calls
  call      the whole core.lfcShrinkApeglm(dds, coef, res) on an object made by from_device, wall clock, outputs on the host
  torch     the same damped Newton iteration batched over the genes in stock ops (matmul, einsum, cholesky_ex,
            cholesky_solve, boolean indexing to keep the active rows; the same acceptance rule, the resolution of F relative
            to the summed magnitudes), both starts, timed like the kernel, --torch-reps runs after a warm-up; its
            iteration counts and its rows at maxit are reported beside the device's
  spec      tests/apeglm_spec.py on the host on --spec-rows rows, and that figure times n / rows (an extrapolation, said so)
  work      per evaluation and sample 5 p + p (p + 1) + 17 f64 operations (a division counted as one; exp, log1p and the
            log of the factor not counted), evaluations counted as iterations + 1 per start (rejected trials are not
            recorded, so this is a lower bound); over the kernel time, as a share of the 78.6 TF f64 vector peak (which
            counts a fused multiply-add as two, and this kernel has none: half of it is the most it could reach)
  copy      a device-to-device copy of 1 GiB of float64 (read + write = 2 GiB moved), event-timed in the same run
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_VECTOR_PEAK = 78.6e12
ARMIJO, RES = 1e-4, 2.0 ** -44


def event_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    r = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2], [round(t, 3) for t in times], r


def simulate(torch, n, m, p, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    f64 = dict(dtype=torch.float64, device="cuda")
    rn = lambda *s: torch.randn(*s, generator=g, **f64)
    x = torch.ones((m, p), **f64)
    x[:, 1] = (torch.arange(m, device="cuda") % 2).to(torch.float64)
    if p > 2:
        x[:, 2:] = rn(m, p - 2)
    sf = torch.exp(0.3 * rn(m))
    beta = torch.zeros((n, p), **f64)
    beta[:, 0] = 4.0 + 1.5 * rn(n)
    beta[:, 1:] = 0.3 * rn(n, p - 1)
    big = torch.rand(n, generator=g, **f64) < 0.1
    beta[big, p - 1] = torch.where(torch.rand(int(big.sum()), generator=g, **f64) < 0.5, -2.5, 2.5).to(torch.float64)
    disp = torch.exp(torch.rand(n, generator=g, **f64) * 4.6 - 4.6)                     # 0.01 .. 1
    mu = sf[None, :] * torch.exp(torch.clamp(beta @ x.T, -20.0, 12.0))
    lam = torch._standard_gamma((1.0 / disp)[:, None].expand(n, m).contiguous()) * (disp[:, None] * mu)
    y = torch.poisson(lam).clamp(max=2.0 ** 31 - 1).to(torch.int32)
    init = beta + 0.05 * rn(n, p)
    return y, x, sf, disp, init


def torch_apeglm(torch, Y, x, sf, disp, init, c, S, tol=1e-8, maxit=100, chunk_elems=1 << 26):
    """the iteration of tests/apeglm_spec.py batched over the genes in stock ops; (map n x p, F n, iter n x 2, start n)"""
    n, m = Y.shape
    p = x.shape[1]
    o = torch.log(sf)
    shrink = torch.ones(p, dtype=torch.bool, device=Y.device)
    shrink[0] = False
    ds2, ns2 = S * S, 225.0

    def ev(y, a, b):
        eta = b @ x.T + o
        mu = torch.exp(eta)
        am = a[:, None] * mu
        t1, t2 = y * eta, (y + 1.0 / a[:, None]) * torch.log1p(am)
        F = -(t1 - t2).sum(1)
        M = (t1.abs() + t2).sum(1)                     # the magnitudes F is summed from: what its resolution is relative to
        d1 = 1.0 + am
        g = -(((y - mu) / d1) @ x)
        H = torch.einsum("gm,mk,ml->gkl", mu * (1.0 + a[:, None] * y) / (d1 * d1), x, x)
        bb = b * b
        prior = torch.where(shrink, torch.log1p(bb / ds2), bb / (2.0 * ns2)).sum(1)
        F, M = F + prior, M + prior
        g = g + torch.where(shrink, 2.0 * b / (ds2 + bb), b / ns2)
        H = H + torch.diag_embed(torch.where(shrink, 2.0 * (ds2 - bb) / (ds2 + bb) ** 2, torch.full_like(bb, 1.0 / ns2)))
        return F, g, H, M

    def search(y, a, b):
        G = y.shape[0]
        F, g, H, Mg = ev(y, a, b)
        lam = torch.zeros(G, dtype=torch.float64, device=y.device)
        it = torch.zeros(G, dtype=torch.float64, device=y.device)
        act = torch.isfinite(F).nonzero().flatten()
        for _ in range(20 * maxit):
            if act.numel() == 0:
                break
            Ha, ga, la = H[act], g[act], lam[act]
            M = Ha + torch.diag_embed(la[:, None] * torch.diagonal(Ha, dim1=1, dim2=2).abs())
            L, info = torch.linalg.cholesky_ex(M)
            s = torch.cholesky_solve(-ga[:, :, None], torch.where(torch.isfinite(L), L, torch.ones_like(L)))[:, :, 0]
            bt = b[act] + s
            Ft, gt, Ht, Mt = ev(y[act], a[act], bt)
            pred = -(ga * s).sum(1)
            Fa = F[act]
            res = RES * Mg[act].clamp(min=1.0)
            ok = (info == 0) & torch.isfinite(Ft) & torch.where(pred > res, Ft <= Fa - ARMIJO * pred, Ft <= Fa + res)
            ia = act[ok]
            b[ia], F[ia], g[ia], H[ia], Mg[ia] = bt[ok], Ft[ok], gt[ok], Ht[ok], Mt[ok]
            it[ia] += 1
            stop = ok & (la == 0) & (s.abs().amax(1) < tol)
            la = torch.where(ok, la * 0.1, torch.where(la < 1e-4, torch.full_like(la, 1e-4), la * 10.0))
            la = torch.where(ok & (la < 1e-7), torch.zeros_like(la), la)
            lam[act] = la
            it[act[~ok & (la > 1e12)]] += 1
            act = act[~stop & ~(ok & (it[act] >= maxit)) & ~(~ok & (la > 1e12))]
        return b, F, it

    out_b = torch.empty((n, p), dtype=torch.float64, device=Y.device)
    out_F = torch.empty(n, dtype=torch.float64, device=Y.device)
    out_it = torch.zeros((n, 2), dtype=torch.float64, device=Y.device)
    out_st = torch.zeros(n, dtype=torch.float64, device=Y.device)
    rows = max(1, min(n, chunk_elems // m))
    for r0 in range(0, n, rows):
        sl = slice(r0, min(n, r0 + rows))
        y, a = Y[sl].to(torch.float64), disp[sl]
        b0 = torch.zeros((y.shape[0], p), dtype=torch.float64, device=Y.device)
        b0[:, 0] = torch.log((y / sf).mean(1).clamp(min=0.1))
        ba, Fa, ita = search(y, a, b0)
        bb_, Fb, itb = search(y, a, init[sl].clamp(-30.0, 30.0).clone())
        won = Fb < Fa
        out_b[sl], out_F[sl] = torch.where(won[:, None], bb_, ba), torch.where(won, Fb, Fa)
        out_it[sl, 0], out_it[sl, 1], out_st[sl] = ita, itb, won.to(torch.float64)
    return out_b, out_F, out_it, out_st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x48x2,50000x500x4,60000x2000x10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--spec-rows", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from deseq2_amd import core, native
    from deseq2_amd.engine import DeviceEngine
    from oracle import oracle as O
    from tests import apeglm_spec as S
    if not torch.cuda.is_available():
        raise SystemExit("apeglm_bench.py measures on the GPU: none found")
    src = torch.ones(1 << 27, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    copy_ms, copy_all, _ = event_ms(torch, lambda: dst.copy_(src), 10)
    copy_rate = 2.0 * src.numel() * 8 / (copy_ms * 1e-3)
    del src, dst
    torch.cuda.empty_cache()
    E = DeviceEngine()
    lines = []
    for shape in a.shapes.split(","):
        n, m, p = (int(v) for v in shape.split("x"))
        c = p - 1
        Y, x, sf, disp, init = simulate(torch, n, m, p, seed=n + m)
        ns = np.zeros(p, bool)
        ns[0] = True
        hx, hsf, hdisp, hinit = x.cpu().numpy(), sf.cpu().numpy(), disp.cpu().numpy(), init.cpu().numpy()
        # a standard error for the prior scale: the two-group variance of a log mean at the row's mean and dispersion
        base = (Y.to(torch.float64) / sf).mean(1).clamp(min=0.5).cpu().numpy()
        se = np.sqrt((1.0 / base + hdisp) * 4.0 / m)
        scale = core.apeglm_prior_scale(np.stack([hinit[:, c], se], axis=1))
        rec = {"shape": shape, "prior_scale": scale, "copy_rate_TB_s": copy_rate / 1e12, "copy_ms_all": copy_all}
        # ---- the kernel on resident inputs
        yg = native.to_gene_major(Y.T.contiguous())
        xd = x.T.contiguous()
        fn = lambda: native.apeglm_dev(yg, xd, sf, disp, c, ns, scale, init=init)
        k_ms, k_all, r = event_ms(torch, fn, a.reps)
        it = r["iter"].cpu().numpy()
        start, conv = r["start"].cpu().numpy(), r["conv"].cpu().numpy()
        fitted = ~np.isnan(conv)
        evals = float((it[fitted] + 1).sum())
        flops = evals * m * (5.0 * p + p * (p + 1) + 17.0)
        rec["ours"] = {"kernel_ms": k_ms, "kernel_ms_all": k_all, "rows_fitted": int(fitted.sum()),
                       "conv_counts": {str(int(v)): int((conv[fitted] == v).sum()) for v in np.unique(conv[fitted])},
                       "iter_median": [float(np.median(it[fitted, 0])), float(np.median(it[fitted, 1]))],
                       "iter_max": [float(it[fitted, 0].max()), float(it[fitted, 1].max())],
                       "share_won_by_second_start": float((start[fitted] == 1).mean()),
                       "counted_GFLOP": flops / 1e9, "TFLOP_s": flops / (k_ms * 1e-3) / 1e12,
                       "share_of_f64_vector_peak": flops / (k_ms * 1e-3) / F64_VECTOR_PEAK}
        # ---- the whole lfcShrinkApeglm call on an object made by from_device
        dds = core.DESeqDataSet.from_device(E, Y.T.contiguous(), None, hx, sizeFactors=hsf)     # (the factors are the m-vector)
        dds.mcols.update(beta=hinit / np.log(2), dispersion=hdisp, baseMean=base, allZero=~fitted)
        tab = core._ColumnsTab({"baseMean": base, "log2FoldChange": hinit[:, c] / np.log(2), "lfcSE": se / np.log(2),
                                "stat": hinit[:, c] / se, "pvalue": np.full(n, 0.5)})
        res = core.DESeqResults(tab, {"type": "none"}, E)
        res["padj"] = np.full(n, 0.5)
        res.coef = c
        core.lfcShrinkApeglm(dds, coef=c, res=res, quiet=True)
        walls = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = core.lfcShrinkApeglm(dds, coef=c, res=res, quiet=True)
            walls.append((time.perf_counter() - t0) * 1e3)
        rec["call"] = {"lfcShrinkApeglm_ms": sorted(walls)[len(walls) // 2], "ms_all": [round(v, 2) for v in walls],
                       "prior_scale": out.priorInfo["prior_control"]["prior_scale"]}
        del dds
        # ---- stock torch
        t_ms, t_all, tr = event_ms(torch, lambda: torch_apeglm(torch, Y, x, sf, disp, init, c, scale), a.torch_reps)
        ours_map = r["map"]
        same_start = (tr[3] == r["start"]) & torch.isfinite(r["objective"])
        tit = tr[2].cpu().numpy()[fitted]
        rec["torch"] = {"ms": t_ms, "ms_all": t_all, "over_ours": t_ms / k_ms,
                        "iter_median": [float(np.median(tit[:, 0])), float(np.median(tit[:, 1]))],
                        "iter_max": [float(tit[:, 0].max()), float(tit[:, 1].max())],
                        "rows_at_maxit": int((tit >= 100).any(axis=1).sum()),
                        "rows_same_start": int(same_start.sum()),
                        "max_abs_map_diff_on_those": float((tr[0] - ours_map)[same_start].abs().max().item()),
                        "rows_torch_F_lower_by_1e-6": int((tr[1] < r["objective"] - 1e-6).sum())}
        del tr
        # ---- the numpy specification on the host, on a few rows
        rows = np.linspace(0, n - 1, a.spec_rows).astype(np.int64)
        hy = Y[torch.as_tensor(rows, device="cuda")].cpu().numpy()
        t0 = time.perf_counter()
        sp = S.fit(O, hy, hx, hsf, hdisp[rows], c, ns, scale, init=hinit[rows])
        dt = (time.perf_counter() - t0) * 1e3
        dev_rows = {k: r[k].cpu().numpy()[rows] for k in ("map", "sd", "fsr", "objective", "conv", "start")}
        rec["spec"] = {"rows_timed": int(rows.size), "ms_per_row": dt / rows.size, "ms_extrapolated_to_n": dt / rows.size * n,
                       "device_equals_spec_on_those_rows": bool(all(
                           np.array_equal(dev_rows[k], sp[k], equal_nan=True) for k in dev_rows))}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del Y, yg, r, init, disp
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
