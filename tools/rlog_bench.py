"""Time the rlog fit kernel (csrc/rlog.hip) on resident data: event timing, one warm-up launch, the median of --reps.
    python tools/rlog_bench.py --n 20000 --m 63 --dense      # ... and the dense route to the same fit: dsq_fit_beta_dev
                                                            # on [1 | I_m] (p = m + 1 <= 64, useQR), timed in the same run
Prints one JSON line: ms, iterations per gene, the bytes the sweeps move (counts 4 B and, with a matrix, factors 8 B per
sample and sweep: 3 sweeps per iteration; state 8 B read + 8 B written per sample and iteration where it does not sit in
registers; 8 B per sample of output) and that as a fraction of --hbm-gbs.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def simulate(n, m, seed):
    rng = np.random.default_rng(seed)
    base = np.exp(rng.normal(3.0, 2.5, n))
    sf = np.exp(rng.normal(0.0, 0.3, m))
    disp = 0.05 + 1.0 / np.maximum(base, 0.5)
    mu = base[:, None] * np.exp(rng.normal(0.0, 1.0, (n, m))) * sf[None, :]
    k = rng.poisson(rng.gamma(1.0 / disp[:, None], mu * disp[:, None]))
    return np.minimum(k, 2 ** 31 - 1).astype(np.int32), sf, disp


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=63)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--betaPriorVar", type=float, default=1.0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the fraction is taken of (MI355X: 8 TB/s)")
    a = ap.parse_args()
    import torch
    from deseq2_amd import native
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine()
    k, sf, disp = simulate(a.n, a.m, a.seed)
    y = E.counts(k)
    sfd, dd = E._vec(sf), E._vec(disp)
    out = native.GeneMajor(torch.zeros((y.n, y.ld), dtype=torch.float64, device=E.device), y.m)
    ms, r = timed(torch, lambda: native.rlog_dev(y, sfd, dd, a.betaPriorVar, out=out), a.reps)
    it = r["iter"].cpu().numpy()
    fitted = r["flag"].cpu().numpy() == 0
    iters = float(it[fitted].sum())
    state = 0 if a.m <= 256 else 16
    bytes_moved = iters * a.m * (3 * 4 + state) + float(fitted.sum()) * a.m * (4 + 8)
    res = {"n": a.n, "m": a.m, "rlog_ms": round(ms, 3), "iter_per_gene": round(iters / max(1, int(fitted.sum())), 2),
           "at_maxit": int((it[fitted] >= 100).sum()), "regime": "registers" if a.m <= 256 else ("lds" if a.m <= 2048 else "row"),
           "gbytes": round(bytes_moved / 1e9, 3), "hbm_fraction": round(bytes_moved / 1e6 / ms / a.hbm_gbs, 5)}
    if a.dense:
        if a.m + 1 > 64:
            raise SystemExit("--dense: the dense fit stops at 64 design columns")
        p = a.m + 1
        x = np.hstack([np.ones((a.m, 1)), np.eye(a.m)])
        q = k / sf[None, :]
        b0 = np.zeros((a.n, p))
        with np.errstate(divide="ignore"):
            b0[:, 0] = np.log(q.mean(axis=1))
        nz = (k != 0).any(axis=1)
        b0[~nz, 0] = 0.0
        lam = np.r_[1e-6, np.full(a.m, 1.0 / a.betaPriorVar)] / np.log(2) ** 2
        xd = E.design(x)
        bd = torch.as_tensor(np.ascontiguousarray(b0.T), device=E.device)
        cd, ld_ = E._vec(np.r_[1.0, np.zeros(p - 1)]), E._vec(lam)
        dms, rd = timed(torch, lambda: native.fitBeta_dev(y, xd, sfd, dd, cd, bd, ld_, None, False, 1e-4, 100, True, 0.5,
                                                          want_hat=False, nf_is_vector=True), a.reps)
        res.update(dense_ms=round(dms, 3), dense_over_rlog=round(dms / ms, 2))
        beta = np.asarray(rd["beta_mat"].cpu().numpy() if torch.is_tensor(rd["beta_mat"]) else rd["beta_mat"])
        beta = beta.T if beta.shape[0] == p else beta
        dense = np.log2(np.e) * beta @ x.T
        mine = out.view().cpu().numpy()
        dit = np.asarray(rd["iter"].cpu().numpy()).reshape(-1)
        ok = fitted & (dit == it)
        res.update(dense_rows_same_iter=int(ok.sum()), dense_rows_fitted=int(fitted.sum()),
                   dense_max_rel_diff=float((np.abs(mine[ok] - dense[ok]) / np.maximum(np.abs(dense[ok]), 1.0)).max()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
