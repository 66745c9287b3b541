"""Argument blocks of the C ABI, built field by field, and the two ways to run them: through the host-pointer entry
(numpy arrays in R layout) and through its `_dev` twin (the same arrays as device buffers, R layout too, null stream).
Shared by tests/test_capi_cpu.py (status codes, no device) and tests/test_gpu_host_entries.py (host entry == twin)."""
import ctypes as C

import numpy as np

from deseq2_amd import _lib as L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fcol(a, dtype=None):
    return np.asfortranarray(np.asarray(a, dtype=dtype))


class Block:
    """one call: `scalars` and `inputs` (numpy arrays, R layout; None = NULL) fill the argument struct A; `outputs`
    (field -> (shape, dtype)) the out struct O; `host_only` names the input fields that stay host arrays in the twin;
    style: "ao" f(args, out), "mu" f(args, mu_floor, mu), "vec" f(args, out_vector)"""

    def __init__(self, name, A, O, scalars, inputs, outputs, host_only=(), out_scalars=None, style="ao", dev=None):
        self.name, self.A, self.O, self.style = name, A, O, style
        self.scalars, self.inputs, self.outputs = dict(scalars), dict(inputs), dict(outputs)
        self.host_only, self.out_scalars = tuple(host_only), dict(out_scalars or {})
        self.dev = name + "_dev" if dev is None else dev           # "": no twin

    def but(self, drop_out=(), **changes):
        """a copy with scalars / inputs replaced and the outputs in drop_out left NULL"""
        b = Block(self.name, self.A, self.O, self.scalars, self.inputs, self.outputs, self.host_only, self.out_scalars,
                  self.style, self.dev)
        for k, v in changes.items():
            if k in b.inputs:
                b.inputs[k] = v
            elif k in b.out_scalars:
                b.out_scalars[k] = v
            else:
                b.scalars[k] = v
        for k in drop_out:
            del b.outputs[k]
        return b

    def args(self, pointers):
        return self.A(**self.scalars, **pointers)


def _invoke(b, fn, a, out_ptrs, tail):
    if b.style == "mu":
        return fn(C.byref(a), float(b.out_scalars.get("mu_floor", 0.0)), out_ptrs["mu"], *tail)
    if b.style == "vec":
        return fn(C.byref(a), next(iter(out_ptrs.values())), *tail)
    o = b.O(**out_ptrs, **b.out_scalars)
    return fn(C.byref(a), C.byref(o), *tail)


def run_host(b, rows=None, check=True):
    """the host entry on numpy arrays; rows = [(lo, cnt), ...] goes through <name>_rows.  Returns the outputs (or the
    status code when check is False)"""
    keep = {k: (None if v is None else fcol(v)) for k, v in b.inputs.items()}
    outs = {k: np.zeros(shape, dtype=dt, order="F") for k, (shape, dt) in b.outputs.items()}
    a = b.args({k: ptr(v) for k, v in keep.items()})
    lib = L.lib()
    if rows is None:
        rc = _invoke(b, getattr(lib, b.name), a, {k: ptr(v) for k, v in outs.items()}, ())
        if rc and check:
            L.check(rc)
    else:
        for lo, cnt in rows:
            rc = _invoke(b, getattr(lib, b.name + "_rows"), a, {k: ptr(v) for k, v in outs.items()}, (int(lo), int(cnt)))
            if rc and check:
                L.check(rc)
    return outs if check else rc


def run_dev(b, check=True, extra_scalars=None, extra_dev_inputs=None, extra_outputs=None, dev=None):
    """the `_dev` twin on device copies of the same arrays (R layout, null stream), results back as numpy"""
    import torch
    tdt = {np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32}
    held, ptrs = [], {}
    for k, v in b.inputs.items():
        if v is None:
            ptrs[k] = None
        elif k in b.host_only:
            h = np.ascontiguousarray(v)
            held.append(h)
            ptrs[k] = ptr(h)
        else:
            t = torch.from_numpy(fcol(v).ravel(order="F").copy()).cuda()
            held.append(t)
            ptrs[k] = C.c_void_p(t.data_ptr())
    for k, t in (extra_dev_inputs or {}).items():
        held.append(t)
        ptrs[k] = C.c_void_p(t.data_ptr())
    shapes = dict(b.outputs)
    shapes.update(extra_outputs or {})
    outs = {k: torch.zeros(int(np.prod(shape)), dtype=tdt[np.dtype(dt)], device="cuda") for k, (shape, dt) in shapes.items()}
    a = b.A(**{**b.scalars, **(extra_scalars or {})}, **ptrs)
    torch.cuda.synchronize()
    rc = _invoke(b, getattr(L.lib(), dev or b.dev), a, {k: C.c_void_p(t.data_ptr()) for k, t in outs.items()}, (None,))
    torch.cuda.synchronize()
    if rc and check:
        L.check(rc)
    if not check:
        return rc
    return {k: t.cpu().numpy().reshape(shapes[k][0], order="F") for k, t in outs.items()}


F8, I4 = np.float64, np.int32


def blocks(d, float_counts=False, weights=False):
    """every block-taking host entry on the arrays of a tests.helpers.make_case dict (plus mu, H, cooks ... taken from
    simple closed forms: the entries are compared with their twins, not with a reference)"""
    y = fcol(d["counts"], F8 if float_counts else I4)
    yt = L.DSQ_Y_FLOAT64 if float_counts else L.DSQ_Y_INT32
    n, m = y.shape
    x = fcol(d["x"], F8)
    p = x.shape[1]
    nf = fcol(d["nf"], F8)
    w = fcol(d["weights"], F8) if weights else None
    useW = int(weights)
    alpha = np.ascontiguousarray(d["alpha_init"], F8)
    la = np.log(alpha)
    b0 = fcol(d["beta_init"], F8)
    mu = fcol(np.maximum(nf * np.exp(b0 @ x.T), 0.5))
    q, r = np.linalg.qr(x)
    xa = x @ np.linalg.inv(r)
    rng = np.random.Generator(np.random.PCG64(n + m))
    H = fcol(rng.uniform(0.01, 0.4, (n, m)))
    cooks = fcol(rng.exponential(1.0, (n, m)) ** 3)
    _, cell = np.unique(x, axis=0, return_inverse=True)
    cell = np.ascontiguousarray(np.asarray(cell).reshape(-1), I4)
    ncell = int(cell.max()) + 1         # given to the fits too: host entry and twin then run the same kernel
    head = dict(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y_type=yt)
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    B = {}
    B["fit_beta"] = Block(
        "dsq_fit_beta", L.DsqFitBetaArgs, L.DsqFitBetaOut,
        dict(head, p=p, nf_is_vector=0, useWeights=useW, tol=1e-8, maxit=100, useQR=1, minmu=0.5, ncell=ncell),
        dict(y=y, x=x, nf=nf, alpha_hat=alpha, contrast=np.r_[1.0, np.zeros(p - 1)], beta_mat=b0, lambda_=lam, weights=w,
             cell_of=cell),
        dict(beta_mat=((n, p), F8), beta_var_mat=((n, p), F8), iter=((n,), F8), hat_diagonals=((n, m), F8),
             contrast_num=((n,), F8), contrast_denom=((n,), F8), deviance=((n,), F8), mu=((n, m), F8)),
        host_only=("cell_of",), out_scalars=dict(mu_floor=0.5))
    disp_out = {k: ((n,), F8) for k in ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp",
                                        "last_d2lp")}
    disp_out.update(iter=((n,), I4), iter_accept=((n,), I4))
    B["fit_disp"] = Block(
        "dsq_fit_disp", L.DsqFitDispArgs, L.DsqFitDispOut,
        dict(head, p=p, log_alpha_prior_sigmasq=0.8, min_log_alpha=float(np.log(1e-9)), kappa_0=1.0, tol=1e-6, maxit=100,
             usePrior=1, useWeights=useW, weightThreshold=1e-2, useCR=1, ncell=ncell),
        dict(y=y, x=x, mu_hat=mu, log_alpha=la, log_alpha_prior_mean=la - 0.1,
             weights=None if w is None else np.maximum(w, 1e-6), cell_of=cell),
        disp_out, host_only=("cell_of",))
    grid = np.linspace(np.log(1e-8), np.log(max(10.0, m)), 12)
    B["fit_disp_grid"] = Block(
        "dsq_fit_disp_grid", L.DsqFitDispGridArgs, L.DsqFitDispGridOut,
        dict(head, p=p, ngrid=grid.size, log_alpha_prior_sigmasq=1.0, usePrior=1, useWeights=useW, weightThreshold=1e-2,
             useCR=1, ncell=ncell),
        dict(y=y, x=x, mu_hat=mu, disp_grid=grid, log_alpha_prior_mean=la,
             weights=None if w is None else np.maximum(w, 1e-6), cell_of=cell),
        dict(log_alpha=((n,), F8)), host_only=("cell_of",))
    prefit_in = dict(y=y, nf=nf, weights=w, q=fcol(q), a=fcol(xa), r=fcol(r))
    B["prefit_moments"] = Block(
        "dsq_prefit_moments", L.DsqPrefitArgs, L.DsqPrefitOut, dict(head, p=p, nf_is_vector=0, useWeights=useW), prefit_in,
        dict(baseMean=((n,), F8), baseVar=((n,), F8), allZero=((n,), I4), roughDisp=((n,), F8), beta_init=((n, p), F8)))
    B["linear_mu"] = Block(
        "dsq_linear_mu", L.DsqPrefitArgs, None, dict(head, p=p, nf_is_vector=0, useWeights=0),
        dict(prefit_in, weights=None, r=None), dict(mu=((n, m), F8)), out_scalars=dict(mu_floor=0.5), style="mu")
    B["nbinom_loglike"] = Block(
        "dsq_nbinom_loglike", L.DsqLogLikeArgs, None, dict(head, useWeights=useW), dict(y=y, mu=mu, disp=alpha, weights=w),
        dict(loglike=((n,), F8)), style="vec")
    B["intercept_fit"] = Block(
        "dsq_intercept_fit", L.DsqInterceptArgs, L.DsqInterceptOut, dict(head, nf_is_vector=0, useWeights=useW, mu_floor=0.5),
        dict(y=y, nf=nf, weights=w, alpha=alpha),
        dict(beta_log2=((n,), F8), betaSE=((n,), F8), mu=((n, m), F8), hat=((n, m), F8)))
    B["cooks_distance"] = Block(
        "dsq_cooks_distance", L.DsqCooksArgs, L.DsqCooksOut, dict(head, p=p, nf_is_vector=0, ncell=ncell),
        dict(y=y, nf=nf, mu=mu, H=H, cell_of=cell),
        dict(cooks=((n, m), F8), maxCooks=((n,), F8), robustDisp=((n,), F8)), host_only=("cell_of",))
    B["replace_outliers"] = Block(
        "dsq_replace_outliers", L.DsqReplaceArgs, L.DsqReplaceOut, dict(head, nf_is_vector=0, cooksCutoff=8.0, trim=0.2),
        dict(y=y, nf=nf, cooks=cooks, replaceable=np.ones(m, I4)),
        dict(newCounts=((n, m), I4), replace=((n,), I4)), host_only=("replaceable",))
    B["size_factors"] = Block(
        "dsq_size_factors", L.DsqSizeFactorArgs, L.DsqSizeFactorOut, dict(head, type=L.DSQ_SF["ratio"], workspace_bytes=0),
        dict(y=y, geoMeans=None, control=None, normMatrix=fcol(rng.uniform(0.5, 2.0, (n, m))), workspace=None),
        dict(sizeFactors=((m,), F8), loggeomeans=((n,), F8), normalizationFactors=((n, m), F8), status=((1,), I4)))
    B["vst"] = Block(
        "dsq_vst", L.DsqVstArgs, L.DsqVstOut,
        dict(head, nf_is_vector=0, kind=L.DSQ_VST["parametric"], asymptDisp=0.05, extraPois=2.5, alpha=0.1, pc=1.0, nknots=0,
             eta=1.0, xi=0.0),
        dict(y=y, nf=nf, spline=None), dict(out=((n, m), F8), rowMean=((n,), F8), rowMax=((n,), F8), bad=((1,), I4)),
        host_only=("spline",))
    B["optim_rows"] = Block(
        "dsq_optim_rows", L.DsqOptimArgs, L.DsqOptimOut, dict(head, p=p, nf_is_vector=0, useWeights=useW, minmu=0.5),
        dict(y=y, x=x, nf=nf, alpha_hat=alpha, lambda_=np.full(p, 1e-6), weights=w, beta_start=fcol(b0 / np.log(2))),
        dict(beta=((n, p), F8), betaSE=((n, p), F8), conv=((n,), I4), mu=((n, m), F8), logLike=((n,), F8)), dev="")
    return B


def run_twin(b):
    """run_dev with what two twins need beyond the block: dsq_size_factors_dev takes a caller's workspace,
    dsq_vst is dsq_vst_dev + dsq_vst_rowstats_dev with a zeroed `bad` flag"""
    import torch
    if b.name == "dsq_size_factors":
        L.lib().dsq_size_factors_workspace_bytes.restype = C.c_int64
        nb = int(L.lib().dsq_size_factors_workspace_bytes(b.scalars["n"], b.scalars["m"]))
        ws = torch.zeros(nb // 8 + 1, dtype=torch.float64, device="cuda")
        b2 = b.but(workspace_bytes=nb)
        del b2.inputs["workspace"]
        return run_dev(b2, extra_dev_inputs=dict(workspace=ws))
    if b.name == "dsq_vst":
        got = {}
        if "out" in b.outputs:
            got.update(run_dev(b.but(drop_out=[k for k in ("rowMean", "rowMax") if k in b.outputs]), dev="dsq_vst_dev"))
        if "rowMean" in b.outputs:
            got.update(run_dev(b.but(drop_out=[k for k in ("out",) if k in b.outputs]), dev="dsq_vst_rowstats_dev"))
        return got
    return run_dev(b)
