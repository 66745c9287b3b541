#!/usr/bin/env python
"""Times the solve of estimateSizeFactors(type = "iterate") (dsq_sf_iterate_dev, csrc/sf_iterate.hip) at the sizes the project
is built for, against the same Newton iteration in stock torch ops on the same device and, at the small shape, against R's
optim call restated through scipy on the host (profiles/sf_iterate.md).

    python tools/sf_iterate_bench.py [--shapes 20000x48,50000x500] [--reps 5] [--lbfgsb-below 2000000] [--whole] [--out FILE]

  ours      dsq_sf_iterate_dev on resident inputs with a reused workspace: a host clock around the call (it ends in a stream
            synchronisation and its outputs are read), the median of --reps after one warm-up; iterations and evaluations
  torch     the same iteration (same objective, cut, step, Armijo test and stopping rules) in stock torch ops: the density
            by lgamma / log with its mu-independent part summed once, the cut by torch.quantile, F, g and h by masked sums,
            one .item() per evaluation; the parent commit has no solve, so this is the baseline there is
  lbfgsb    tests/sf_iterate_lbfgsb.py on the host, for shapes of at most --lbfgsb-below cells: seconds, evaluations, F
  whole     core.estimateSizeFactors(type = "iterate") on a DeviceEngine (the dispersion steps of every round included):
            seconds after one warm-up call, and the number of outer rounds
The per-kernel split comes from a kernel trace of `--reps 1 --only-ours` taken in a run of its own.
Inputs are negative binomial counts drawn on the device from a seed.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(torch, n, m, seed):
    """counts ~ NB(q_i true_sf_j, a_i) with one planted zero per gene; the current factors 10 % off the true ones; mu the
    intercept fit at them, floored at 0.5"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f64 = dict(dtype=torch.float64, device="cuda")
    true_sf = torch.exp(0.5 * torch.randn(m, generator=g, **f64))
    q = torch.exp(4.0 + 1.5 * torch.randn((n, 1), generator=g, **f64))
    a = 0.01 + 0.49 * torch.rand(n, generator=g, **f64)
    mean = q * true_sf[None, :]
    torch.manual_seed(seed)
    lam = torch._standard_gamma((1.0 / a)[:, None].expand(n, m).contiguous()) * (a[:, None] * mean)
    k = torch.poisson(lam, generator=g)
    k[torch.arange(n, device="cuda"), torch.randint(0, m, (n,), generator=g, device="cuda")] = 0.0
    k[k.sum(dim=1) == 0, 0] = 1.0
    sf = true_sf * torch.exp(0.1 * torch.randn(m, generator=g, **f64))
    mu = ((k / sf[None, :]).mean(dim=1, keepdim=True) * sf[None, :]).clamp_min(0.5)
    return k, mu, sf, a


def torch_solve(torch, k, mu, sf, a, Q=0.05, maxit=100):
    """the iteration of csrc/sf_iterate.hip in stock ops; returns (s, F, iter, evals, flag)"""
    m = k.shape[1]
    size = (1.0 / a)[:, None]
    q = mu / sf[None, :]
    al = a[:, None]
    const = (torch.lgamma(k + size) - torch.lgamma(size) - torch.lgamma(k + 1.0)).sum(dim=1)

    def evaluate(e):
        mun = q * e[None, :]
        den = size + mun
        L = const + (size * torch.log(size / den) + torch.xlogy(k, mun / den)).sum(dim=1)
        kept = L > torch.quantile(L, Q)
        return kept, float(torch.where(kept, L, 0.0).sum().item())

    def direction(kept, e):
        mun = q * e[None, :]
        opm = 1.0 + al * mun
        w = kept[:, None]
        g = torch.where(w, (k - mun) / opm, 0.0).sum(dim=0)
        h = torch.where(w, mun * (1.0 + al * k) / (opm * opm), 0.0).sum(dim=0)
        lam = (g / h).sum() / (1.0 / h).sum()
        d = (g - lam) / h
        return d, float((g * d).sum().item())

    ls = torch.log(sf)
    s = ls - ls.mean()
    e = torch.exp(s)
    kept, F = evaluate(e)
    it, evals, flag = 0, 1, 1
    while it < maxit:
        it += 1
        d, gd = direction(kept, e)
        t, ok = 1.0, False
        for _ in range(30):
            st = s + t * d
            st = st - st.mean()
            et = torch.exp(st)
            keptt, Ft = evaluate(et)
            evals += 1
            if Ft >= F + 1e-4 * t * gd:
                ok = True
                break
            t *= 0.5
        if not ok:
            flag = 0 if gd <= 1e-10 * abs(F) else 1
            break
        gain, s, e, kept, F = Ft - F, st, et, keptt, Ft
        if gain <= 1e-10 * abs(F):
            flag = 0
            break
    return s, F, it, evals, flag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20000x48,50000x500")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lbfgsb-below", type=int, default=2000000)
    ap.add_argument("--only-ours", action="store_true")
    ap.add_argument("--whole", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from deseq2_amd import _lib, native
    lines = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        k, mu, sf, disp = make_inputs(torch, n, m, seed=n + m)
        ld = (m + 7) & ~7
        yt = torch.zeros((n, ld), dtype=torch.int32, device="cuda")
        yt[:, :m] = k.to(torch.int32)
        mt = torch.zeros((n, ld), dtype=torch.float64, device="cuda")
        mt[:, :m] = mu
        Y, M = native.GeneMajor(yt, m), native.GeneMajor(mt, m)
        rows = torch.ones(n, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(_lib.lib().dsq_sf_iterate_workspace_bytes(n, m)), dtype=torch.uint8, device="cuda")
        times = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = native.sf_iterate_dev(Y, M, sf, disp, rows, workspace=ws)
            pack = r["_pack"].cpu().numpy()                     # the results are consumed
            if rep:
                times.append(1e3 * (time.perf_counter() - t0))
        F, it, evals, flag = float(pack[2 * m]), int(pack[2 * m + 1]), int(pack[2 * m + 2]), int(pack[2 * m + 3])
        med = sorted(times)[len(times) // 2]
        rec = {"n": n, "m": m, "ours_ms": med, "ours_ms_all": [round(t, 3) for t in times], "ours_ms_per_eval": med / evals,
               "iter": it, "evals": evals, "flag": flag, "F": F, "workspace_MiB": ws.numel() / 2 ** 20}
        if not a.only_ours:
            torch_solve(torch, k, mu, sf, disp, maxit=1)                                # warm-up
            tt = []
            for rep in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ts, tF, tit, tev, tflag = torch_solve(torch, k, mu, sf, disp)
                ts = ts.cpu().numpy()
                tt.append(1e3 * (time.perf_counter() - t0))
            tmed = sorted(tt)[len(tt) // 2]
            rec.update(torch_ms=tmed, torch_ms_all=[round(t, 3) for t in tt], torch_ms_per_eval=tmed / tev, torch_iter=tit,
                       torch_evals=tev, torch_flag=tflag, torch_F=tF, torch_over_ours=tmed / med,
                       max_abs_s_torch_minus_ours=float(np.abs(ts - pack[:m]).max()))
            if n * m <= a.lbfgsb_below:
                from tests import sf_iterate_lbfgsb
                c = dict(counts=k.cpu().numpy(), mu=mu.cpu().numpy(), sf=sf.cpu().numpy(), disp=disp.cpu().numpy(),
                         rows=np.ones(n, np.int32))
                t0 = time.perf_counter()
                b = sf_iterate_lbfgsb.sf_iterate_lbfgsb(**c)
                rec.update(lbfgsb_s=time.perf_counter() - t0, lbfgsb_nfev=b["nfev"], lbfgsb_F=b["F"],
                           lbfgsb_convergence=b["convergence"], ours_F_same_statement=sf_iterate_lbfgsb.fn_of(**c)(pack[:m]),
                           max_abs_s_lbfgsb_minus_ours=float(np.abs(b["s"] - pack[:m]).max()))
        if a.whole:
            from deseq2_amd import core
            from deseq2_amd.engine import DeviceEngine
            kh = k.cpu().numpy().astype(np.int32)
            E = DeviceEngine()
            for rep in range(2):
                dds = core.DESeqDataSet(kh, np.ones((m, 1)), engine=E)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    core.estimateSizeFactors(dds, type="iterate")
                    rec["whole_rounds"] = dds.attrs["sfIterateRounds"]
                except ValueError as ex:
                    rec["whole_error"] = str(ex)
                torch.cuda.synchronize()
                rec["whole_s"] = time.perf_counter() - t0
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
