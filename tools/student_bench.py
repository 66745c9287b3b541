"""Timing of the Student-t paths at n = 20 000 on resident data, each next to the same call without
degrees of freedom (the normal-distribution path, whose kernels this feature leaves as they were):

  * dsq_pt_dev, the elementwise pass (csrc/student.hip), two-sided, K = 1 and K = 45 columns;
  * dsq_results_dev, a threshold test (lfcThreshold = 1, greaterAbs) with independent filtering over 50 quantiles, with and
    without df;
  * dsq_contrasts_dev, the 45 pairs of a 10-level factor on 20 000 x 60 (the factor10 case of tools/contrasts_bench.py), with
    and without df -- and the share of the call the pt pass takes.

HIP events, 2 warm-up calls, >= 10 repetitions, median and spread, a 512 MB buffer rewritten between repetitions so that no
input is served from the last-level cache.  One JSON line per measurement.

    python tools/student_bench.py [--reps 10] [--n 20000] [--skip-t]

--skip-t: only the calls without df (what a tree from before the feature can run: the parent's side of the comparison)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--skip-t", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("student_bench needs a GPU: a CPU run gives no time")
    from deseq2_amd import _lib, native, simulate
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine()
    dev = E.device
    n, reps = a.n, a.reps
    rng = np.random.default_rng(7)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    flush = torch.zeros(64 * 1024 * 1024, dtype=torch.float64, device=dev)
    digest = hashlib.sha256(open(_lib.SO_PATH, "rb").read()).hexdigest()[:16]
    head = {"n": n, "device": torch.cuda.get_device_name(0), "library_sha256": digest}

    def report(what, r, **extra):
        print(json.dumps(dict(head, what=what, **extra, **r)), flush=True)

    df = t(rng.uniform(2.0, 40.0, n))                   # sum(weights) - p of a small analysis: fractional
    # ---- the elementwise pass
    if not a.skip_t:
        for K in (1, 45):
            q = t(rng.normal(0, 3, (K, n)))
            out = torch.empty_like(q)
            report("dsq_pt_dev two-sided", _events(torch, lambda: native.pt_dev(q, df, "two_sided", out=out), 2, reps, flush), K=K)
    # ---- the results table
    p = 4
    beta, se = rng.normal(0, 1.5, (p, n)), np.exp(rng.normal(-1, 0.5, (p, n)))
    cols = [t(v) for v in (beta, se, beta / se, rng.uniform(size=(p, n)))]
    bm = t(np.exp(rng.normal(4, 2, n)))
    theta = t(np.linspace(0, 0.95, 50))
    for d in ([None] if a.skip_t else [None, df]):
        kw = {} if d is None else {"df": d}
        fn = lambda: native.results_dev(cols[0], cols[1], cols[2], cols[3], bm, p - 1, lfcThreshold=1.0, altHypothesis="greaterAbs",
                                        theta=theta, alpha=0.1, **kw)
        report("dsq_results_dev lfcThreshold=1 greaterAbs, 50 thetas", _events(torch, fn, 2, reps, flush), df=d is not None)
    # ---- the contrasts: all pairs of a 10-level factor
    x = simulate.design_factor(60, 10)
    m, p = x.shape
    pairs = [(i, j) for i in range(10) for j in range(i + 1, 10)]
    c = np.zeros((p, len(pairs)))
    for k, (i, j) in enumerate(pairs):
        if j:
            c[j, k] += 1.0
        if i:
            c[i, k] -= 1.0
    b = np.column_stack([rng.normal(3.0, 1.5, n)] + [rng.normal(0, 0.5, n) for _ in range(p - 1)])
    xd = E.design(x)
    cells = E._cells.get(xd.data_ptr())
    sfd, ad, bd, ld_, cd = t(np.exp(rng.normal(0, 0.2, m))), t(np.exp(rng.normal(-2, 1, n))), t(b.T), t(np.full(p, 1e-6 / np.log(2) ** 2)), t(c.T)
    times = {}
    for d in ([None] if a.skip_t else [None, df]):
        kw = {} if d is None else {"df": d}
        fn = lambda: native.contrasts_dev(xd, sfd, ad, bd, ld_, cd, minmu=0.5, nf_is_vector=True, cells=cells, **kw)["table"].sum()
        times[d is not None] = r = _events(torch, fn, 2, reps, flush)
        report("dsq_contrasts_dev factor10 K=45", r, df=d is not None)
    if not a.skip_t:
        share = 1.0 - times[False]["median_ms"] / times[True]["median_ms"]
        print(json.dumps(dict(head, what="share of the contrast call taken by the pt pass", share=share)), flush=True)


if __name__ == "__main__":
    main()
