"""Timing of lfcShrink(type = "normal") (core.lfcShrink).  One JSON line per measurement.

    python tools/lfcshrink_bench.py [--reps 10] [--n 20000] [--levels 2,10,48] [--skip-mirror] [--skip-shrink]

1. The prior variance of all columns at n genes for one factor of 2, 10 and 48 levels, standard and expanded model matrix
   (48 levels expanded: 47 level columns + 1 081 contrast columns), four ways that are compared bit for bit first:
     mirror     core.estimateBetaPriorVar, numpy on the host (once: it takes seconds);
     host_c     dsq_beta_prior_var, the library's host threads -- the yardstick;
     dev        dsq_beta_prior_var_dev on resident inputs (the call waits for the stream once and returns the host vector);
     dev_upload DeviceEngine.beta_prior_var: the same with the n (p + 2) doubles and the flags going up first.
   Wall-clock time around the whole call (the device entry returns only when its result is on the host), a warm-up, `reps`
   repetitions, median and spread.
2. core.lfcShrink end to end on a fused.DESeq analysis of n x 30 counts, a 10-level factor: by `coef` and by one character
   contrast, on the lean route (lfcThreshold = 0) and the full one (lfcThreshold = 1); the columns are read inside the
   timed region."""
import argparse
import hashlib
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _wall(fn, warmup, reps, sync):
    for _ in range(warmup):
        fn()
    sync()
    s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        s.append(1e3 * (time.perf_counter() - t0))
    s = np.array(s)
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "reps": int(reps)}


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(a.shape == b.shape and ((a == b) | (np.isnan(a) & np.isnan(b))).all())


def prior_var(E, n, levels, expanded, reps, mirror, tag):
    import torch
    from deseq2_amd import core, native
    rng = np.random.default_rng(levels + n)
    factors = OrderedDict(condition=np.arange(2 * levels) % levels)
    x, names = core.standard_model_matrix(factors)
    p = levels
    mle = rng.normal(0, 1.0, (n, p)) * rng.choice([1.0, 1.0, 1.0, 6.0], (n, 1))
    mle[:, 0] = rng.normal(5, 2, n)
    bm = np.exp(rng.normal(4, 2, n))
    dfit = 0.05 + 3.0 / bm
    az = rng.uniform(size=n) < 0.05
    mle[az] = np.nan
    cf = native.coef_factor_codes(factors)
    pcf = native.coef_factor_codes(factors, expanded=True) if expanded else None
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=E.device)
    d = (t(mle.T), t(bm), t(dfit), t(az.astype(np.int32), torch.int32))
    sync = torch.cuda.synchronize
    host_c = lambda: native.estimateBetaPriorVarHost(mle, bm, dfit, az, cf, prior_coef_factor=pcf)
    dev = lambda: native.estimateBetaPriorVar_dev(*d, cf, prior_coef_factor=pcf)
    up = lambda: E.beta_prior_var(mle, bm, dfit, az, cf, prior_coef_factor=pcf)
    ref = host_c()
    columns = p + (levels - 1) * (levels - 2) // 2 if expanded else p
    out = dict(tag, what="prior_var", n=n, levels=levels, matrix="expanded" if expanded else "standard", columns=columns,
               dev_equals_host_c=_same(dev(), ref), dev_upload_equals_host_c=_same(up(), ref))
    if mirror:
        view = type("V", (), {"mcols": {"baseMean": bm[~az], "dispFit": dfit[~az]}})()
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            pv, _ = core.estimateBetaPriorVar(view, mle[~az], names, modelMatrixType="expanded" if expanded else "standard",
                                              factors=factors)
        out["mirror"] = {"median_ms": 1e3 * (time.perf_counter() - t0), "reps": 1}
        out["mirror_equals_host_c"] = _same(pv, ref)
    out["host_c"] = _wall(host_c, 1, reps, sync)
    out["dev"] = _wall(dev, 2, reps, sync)
    out["dev_upload"] = _wall(up, 2, reps, sync)
    out["host_c_over_dev"] = out["host_c"]["median_ms"] / out["dev"]["median_ms"]
    print(json.dumps(out), flush=True)


def shrink(E, n, reps, tag):
    import torch
    from deseq2_amd import core, fused, simulate
    levels, m = 10, 30
    f = OrderedDict(condition=(np.arange(m) * levels) // m)
    x, _ = core.standard_model_matrix(f)
    assert np.array_equal(x, simulate.design_factor(m, levels))
    k = simulate.make_counts(n, x, seed=3, drop_all_zero=False)["counts"]
    dds = fused.DESeq(core.DESeqDataSet(k, x, engine=E))
    dds.attrs["factors"] = f
    read = lambda r: [np.asarray(r[c]) for c in core.DESeqResults.COLUMNS]
    for call in (dict(coef=9), dict(contrast=("condition", 9, 4))):
        res = core.results(dds, name=9) if "coef" in call else core.resultsContrasts(dds, [call["contrast"]])[0]
        for thr in (0, 1):
            fn = lambda: read(core.lfcShrink(dds, res=res, lfcThreshold=thr, quiet=True, **call))
            out = dict(tag, what="lfcShrink", n=n, m=m, levels=levels, call={k_: list(v) if isinstance(v, tuple) else v for k_, v in call.items()},
                       route="lean" if thr == 0 else "full", lfcThreshold=thr)
            out["lfcShrink"] = _wall(fn, 1, reps, torch.cuda.synchronize)
            print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--levels", default="2,10,48")
    ap.add_argument("--skip-mirror", action="store_true")
    ap.add_argument("--skip-shrink", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lfcshrink_bench needs a GPU: a CPU run gives no time")
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine()
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deseq2_amd", "libdeseq2_mi355x.so")
    tag = {"device": torch.cuda.get_device_name(0), "library_sha256": hashlib.sha256(open(so, "rb").read()).hexdigest()[:16]}
    for levels in (int(v) for v in a.levels.split(",")):
        for expanded in (False, True):
            prior_var(E, a.n, levels, expanded, a.reps, not a.skip_mirror, tag)
    if not a.skip_shrink:
        shrink(E, a.n, a.reps, tag)


if __name__ == "__main__":
    main()
