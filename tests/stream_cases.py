"""The case table of the stream-order tests (tests/test_gpu_stream_order.py runs it on a held stream, tests/stream_hold.py;
tests/test_stream_cases_cpu.py holds it to the conditions that let the GPU test fail).  Not a test itself.

One case per HOST-SIDE path of a `_dev` entry point: what the entry enqueues around its kernels (table uploads, memsets,
padding copies, layout conversions, a fork to the side stream), not the kernel variants.  A case is

  build(which)    which = 0: the true inputs, 1: the decoy -- the same builder on another seed (and another, equally valid,
                  design coding / ridge / contrast where the builder has no seed for them).  Returns a dict: `in` maps the
                  name of every DEVICE input to an In (the host array as it lies on the device, its domain, the sample
                  count m of a GeneMajor matrix); everything else is host-side (tables, scalars) and is taken from the true
                  build alone;
  call(h, d)      the call on torch's current stream: h maps the input names to the resident handles (tensors, GeneMajor),
                  h["ws"] is the caller-provided workspace of `workspace(d)` bytes where the entry takes one;
  want(O, d, a)   the expected values: the oracle, the numpy specification or the line-cited mirror the entry's own GPU
                  test compares with, on the arrays a[name] (the logical, unpadded inputs) and the host side of d;
  got(s, d)       the same keys from the snapshot of the call's outputs (host arrays).

Domains (In.dom), checked by the CPU test on both builds: "count" non-negative integers, "pos" finite and positive,
"flag" 0 / 1, ("index", hi) integers in [0, hi), ("offsets", hi) non-decreasing integers from 0 to hi, None: any finite or
non-finite VALUE that forms no address (a coefficient, a statistic, a p-value).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from deseq2_amd import _lib as L
from deseq2_amd import native, simulate
from tests import hp_reference as H
from tests import wide_cases

N = 37                      # genes of the fit cases: no multiple of any genes-per-workgroup (tests/test_gpu_entry_memory.py)
SEED_DECOY = 7919           # added to a builder's seed for the decoy


class In:
    def __init__(self, a, dom=None, m=None):
        self.a, self.dom, self.m = np.ascontiguousarray(a), dom, m

    @classmethod
    def gm(cls, a, dom=None):
        """an n x m matrix as it lies in a GeneMajor handle: ld = round8(m), padding columns zero (native.to_gene_major)"""
        a = np.asarray(a)
        n, m = a.shape
        buf = np.zeros((n, native.gene_major_ld(m)), dtype=a.dtype)
        buf[:, :m] = a
        return cls(buf, dom, m)

    def logical(self):
        return self.a if self.m is None else self.a[:, :self.m]


class Case:
    def __init__(self, name, entry, build, call, want, got, exempt=None, workspace=None, constant=()):
        self.name, self.entry, self.build, self.call, self.want, self.got = name, entry, build, call, want, got
        self.constant = tuple(constant)   # outputs with ONE value on every valid input (a status word, an error flag): compared
                                          # on the device, but no valid decoy can move them
        self.exempt = exempt              # key of EXEMPT: the entry states a host synchronisation itself
        self.workspace = workspace        # d -> bytes of the caller-provided workspace
        self._built = {}
        self._want = {}

    def data(self, which):
        if which not in self._built:
            self._built[which] = self.build(which)
        return self._built[which]

    def arrays(self, which):
        return {k: v.logical() for k, v in self.data(which)["in"].items()}

    def expected(self, O, which=0):
        """want() on the inputs of build(which) with the host side of the TRUE build: what a stale read would give"""
        if which not in self._want:
            with np.errstate(all="ignore"):
                self._want[which] = self.want(O, self.data(0), self.arrays(which))
        return self._want[which]


# The entries that state a host synchronisation THEMSELVES: late inputs and recycling are checked, the asynchrony assertion
# is not made.  key -> (entry, the words of include/deseq2_mi355x.h that grant it).  Exactly these; any other entry found to
# synchronise is a finding, not a new row.
EXEMPT = {
    "sf_iterate": ("dsq_sf_iterate_dev", "so the call SYNCHRONISES `stream` (a few dozen times) and the outputs are complete on return"),
    "beta_prior_var": ("dsq_beta_prior_var_dev", "Enqueues on `stream`, waits for it ONCE to bring the `columns` variances down"),
    "f64_counts": ("the fit and aux entries given DSQ_Y_FLOAT64 counts",
                   "given DSQ_Y_FLOAT64 counts they check the counts on the device and WAIT for `stream` once"),
}


def _host(t):
    return t.cpu().numpy()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _empty(shape, dtype, like):
    import torch
    return torch.empty(shape, dtype=dtype, device=like.device)


def other_coding(x):
    """the same design in another, equally valid coding: the non-intercept columns in reverse order, a two-column design with
    the other reference level.  Rows that were equal stay equal (the design cells are the same), the rank is the same."""
    x = np.asarray(x, np.float64)
    p = x.shape[1]
    if p == 1:
        return 2.0 * x
    if p == 2:
        return np.column_stack([x[:, 0], x[:, 0] - x[:, 1] if set(np.unique(x[:, 1])) <= {0.0, 1.0} else -x[:, 1]])
    return np.column_stack([x[:, 0]] + [x[:, j] for j in range(p - 1, 0, -1)])


# ================================================================================================ the fits
def _design(kind, p, m):
    if kind == "factor":
        return simulate.design_factor(m, p)
    if kind == "cont":
        return wide_cases.factor_cont(m, p - 1)
    raise ValueError(kind)


def _fit_data(kind, p, m, which, weights=False):
    """tests/test_gpu_entry_memory.py::_case at n = 37 (its generator, its seed; 8 spare rows for the all-zero ones)"""
    x = _design(kind, p, m)
    d = wide_cases.case(N + 8, x, weights=weights, seed=1000 * p + m + which * SEED_DECOY)
    assert d["counts"].shape[0] >= N
    d = wide_cases.take_rows(d, slice(0, N))
    d["cells"] = native.cell_index(x)
    d["contrast"] = np.r_[1.0, np.zeros(p - 2), -1.0] if p > 1 else np.ones(1)
    if which:
        d["x"], d["lam"], d["contrast"] = other_coding(x), 3.0 * d["lam"], d["contrast"][::-1].copy()
    return d


BETA_KEYS = ("beta_mat", "beta_var_mat", "iter", "deviance", "contrast_num", "contrast_denom", "hat_diagonals", "mu")


def _beta_want(O, d, a, r_layout=False):
    t = (lambda v: v.T) if r_layout else (lambda v: v)
    w = O.fitBeta(np.asarray(t(a["y"]), np.float64).astype(np.int32), a["x"].T, t(a["nf"]), a["alpha"], a["contrast"], a["beta0"].T, a["lam"],
                  t(a["w"]) if "w" in a else d["weights"], d["useWeights"], 1e-8, 100, True, 0.5, want_mu=True, mu_floor=0.5)
    return {k: w[k] for k in BETA_KEYS}


def _beta_build(kind, p, m, weights=False):
    def build(which):
        d = _fit_data(kind, p, m, which, weights)
        d["in"] = OrderedDict(y=In.gm(d["counts"].astype(np.int32), "count"), x=In(d["x"].T), nf=In.gm(d["nf"], "pos"),
                              alpha=In(d["alpha_init"], "pos"), contrast=In(d["contrast"]), beta0=In(d["beta_init"].T),
                              lam=In(d["lam"], "pos"))
        if weights:
            d["in"]["w"] = In.gm(d["weights"], "weight")
        return d
    return build


def _beta_call(h, d, cells=None):
    return native.fitBeta_dev(h["y"], h["x"], h["nf"], h["alpha"], h["contrast"], h["beta0"], h["lam"], h.get("w"), d["useWeights"],
                              1e-8, 100, True, 0.5, want_hat=True, want_mu=True, mu_floor=0.5,
                              cells=d["cells"] if cells is None else cells)


def _beta_got(s, d):
    out = {k: _host(s[k]).T for k in ("beta_mat", "beta_var_mat")}
    out.update({k: _host(s[k]) for k in ("iter", "deviance")})
    out.update({k: _host(s[k]).reshape(-1, 1) for k in ("contrast_num", "contrast_denom")})
    out.update(hat_diagonals=_host(s["hat_diagonals"].view()), mu=_host(s["mu"].view()))
    return out


def _beta_r_build(f64):
    def build(which):
        d = _fit_data("cont", 4, 100, which)
        y = d["counts"].astype(np.float64 if f64 else np.int32)
        d["in"] = OrderedDict(y=In(y.T, "count"), x=In(d["x"].T), nf=In(d["nf"].T, "pos"), alpha=In(d["alpha_init"], "pos"),
                              contrast=In(d["contrast"]), beta0=In(d["beta_init"].T), lam=In(d["lam"], "pos"))
        d["f64"] = f64
        return d
    return build


def _beta_r_call(h, d):
    """dsq_fit_beta_dev on device pointers in R's column-major layout (tests/test_gpu_entry_memory.py::test_fit_beta_dev_r_layout)"""
    import torch
    m, n = h["y"].shape
    p = h["x"].shape[0]
    out = {k: _empty(s, torch.float64, h["y"]) for k, s in
           (("beta_mat", (p, n)), ("beta_var_mat", (p, n)), ("iter", (n,)), ("hat", (m, n)), ("cn", (n,)), ("cd", (n,)),
            ("dev", (n,)), ("mu", (m, n)))}
    a = L.DsqFitBetaArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_p(h["y"]), y_type=L.DSQ_Y_FLOAT64 if d["f64"] else L.DSQ_Y_INT32,
                         x=_p(h["x"]), nf=_p(h["nf"]), nf_is_vector=0, alpha_hat=_p(h["alpha"]), contrast=_p(h["contrast"]),
                         beta_mat=_p(h["beta0"]), lambda_=_p(h["lam"]), weights=None, useWeights=0, tol=1e-8, maxit=100, useQR=1,
                         minmu=0.5, cell_of=d["cells"].ctypes.data_as(C.c_void_p), ncell=int(d["cells"].max()) + 1)
    o = L.DsqFitBetaOut(beta_mat=_p(out["beta_mat"]), beta_var_mat=_p(out["beta_var_mat"]), iter=_p(out["iter"]),
                        hat_diagonals=_p(out["hat"]), contrast_num=_p(out["cn"]), contrast_denom=_p(out["cd"]),
                        deviance=_p(out["dev"]), mu=_p(out["mu"]), mu_floor=0.5)
    L.check(L.lib().dsq_fit_beta_dev(C.byref(a), C.byref(o), _stream()))
    return out


def _beta_r_got(s, d):
    out = {kw: _host(s[k]).T for k, kw in (("beta_mat", "beta_mat"), ("beta_var_mat", "beta_var_mat"), ("hat", "hat_diagonals"), ("mu", "mu"))}
    out.update({kw: _host(s[k]) for k, kw in (("iter", "iter"), ("dev", "deviance"))})
    out.update({kw: _host(s[k]).reshape(-1, 1) for k, kw in (("cn", "contrast_num"), ("cd", "contrast_denom"))})
    return out


DISP_KEYS = ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp", "last_d2lp", "iter", "iter_accept")


def _mu_hat(d):
    """the means a dispersion fit is handed: the oracle's fitBeta means of the build's own inputs"""
    from oracle import oracle as O
    ob = O.fitBeta(d["counts"], d["x"], d["nf"], d["alpha_init"], d["contrast"], d["beta_init"], d["lam"], d["weights"], d["useWeights"],
                   1e-8, 100, True, 0.5, want_mu=True, mu_floor=0.5)
    return np.where(np.isfinite(ob["mu"]), ob["mu"], 0.5)


def _disp_build(kind, p, m, grid=False):
    def build(which):
        d = _fit_data(kind, p, m, which)
        la = np.log(d["alpha_init"])
        d["in"] = OrderedDict(y=In.gm(d["counts"].astype(np.int32), "count"), x=In(d["x"].T), mu=In.gm(_mu_hat(d), "pos"))
        if grid:
            d["in"].update(grid=In(np.linspace(np.log(1e-8), np.log(max(10, m)), 12) + 0.01 * which), prior=In(la))
        else:
            d["in"].update(la=In(la), prior=In(la - 0.1))
        return d
    return build


def _disp_call(h, d):
    return native.fitDisp_dev(h["y"], h["x"], h["mu"], h["la"], h["prior"], 0.8, np.log(1e-9), 1.0, 1e-6, 100, True, None, False, 1e-2,
                              True, want_d2lp=True, cells=d["cells"])


def _disp_want(O, d, a):
    w = O.fitDisp(a["y"], a["x"].T, a["mu"], a["la"], a["prior"], 0.8, np.log(1e-9), 1.0, 1e-6, 100, True, d["weights"], False, 1e-2, True)
    return {k: w[k] for k in DISP_KEYS}


def _grid_call(h, d):
    return native.fitDispGrid_dev(h["y"], h["x"], h["mu"], h["grid"], h["prior"], 1.0, True, None, False, 1e-2, True, cells=d["cells"])


def _grid_want(O, d, a):
    return {"log_alpha": O.fitDispGrid(a["y"], a["x"].T, a["mu"], a["grid"], a["prior"], 1.0, True, d["weights"], False, 1e-2, True)["log_alpha"]}


def _keys_got(keys):
    return lambda s, d: {k: _host(s[k]) for k in keys}


# ================================================================================================ aux and helper entries
def _aux_shape(name):
    return [s for s in H.AUX_SHAPES if s[0] == name][0]           # (the smallest shape of the entry)


def _aux_data(name, which, big_every=1):
    _, kind, p, m, w = _aux_shape(name)
    c = H.make_case(kind, p, m, weights=w, seed=1000 * p + m + which * SEED_DECOY, big_every=big_every)
    c["mu_floor"] = 0.5 if m == 24 else 0.0
    c["qar"] = _qar(c["x"])
    return c


def _qar(x):
    """Q, A = X R^-1 and R as the aux entries take them: the oracle's own factors (tests/test_gpu_entry_memory.py::_qr_dev)"""
    from oracle import oracle as O
    return tuple(np.ascontiguousarray(np.asarray(z).T) for z in O.design_qr(x))


def _prefit_build(which):
    c = _aux_data("prefitMoments", which)
    c["y"][2 + 3 * which] = 0                  # an all-zero row, another one in the decoy: the allZero flags differ
    q, a, r = c["qar"]
    if which:                                  # (the design is the builder's own: another valid Q / A / R of the same shapes)
        q, a, r = _qar(other_coding(c["x"]))
    c["in"] = OrderedDict(y=In.gm(c["y"], "count"), nf=In.gm(c["nf"], "pos"), q=In(q), a=In(a), r=In(r))
    return c


def _prefit_want(O, d, a):
    # the oracle takes the design and factors it itself: x from the resident Q and R (exactly the builder's x for build 0)
    x = d["x"] if np.array_equal(a["q"], d["qar"][0]) else other_coding(d["x"])
    w = O.prefitMoments(a["y"], a["nf"], x, d["weights"], d["useWeights"])
    return {"baseMean": w["baseMean"], "baseVar": w["baseVar"], "roughDisp": w["roughDisp"], "allZero": w["allZero"], "beta_init": w["beta_init"]}


def _prefit_got(s, d):
    out = {k: _host(s[k]) for k in ("baseMean", "baseVar", "roughDisp")}
    out.update(allZero=_host(s["allZero"]) != 0, beta_init=_host(s["beta_init"]).T)
    return out


def _linmu_build(which):
    c = _aux_data("linearMu", which)
    q, a, _ = c["qar"]
    if which:
        q, a, _ = _qar(other_coding(c["x"]))
    c["in"] = OrderedDict(y=In.gm(c["y"], "count"), nf=In.gm(c["nf"], "pos"), q=In(q), a=In(a))
    return c


def _linmu_want(O, d, a):
    x = d["x"] if np.array_equal(a["q"], d["qar"][0]) else other_coding(d["x"])
    return {"mu": O.linearMu(a["y"], a["nf"], x, d["mu_floor"])}


def _loglike_build(which):
    c = _aux_data("nbinomLogLike", which)
    c["in"] = OrderedDict(y=In.gm(c["y"], "count"), mu=In.gm(c["mu"], "pos"), disp=In(np.exp(c["log_alpha"]) * (1.0 + 0.5 * which), "pos"))
    return c


def _intercept_build(which):
    c = _aux_data("cooksDistance", which, big_every=2)
    c["in"] = OrderedDict(y=In.gm(c["y"], "count"), nf=In.gm(c["nf"], "pos"), alpha=In(np.exp(c["log_alpha"]) * (1.0 + 0.5 * which), "pos"))
    return c


def _intercept_want(O, d, a):
    w = O.interceptFit(a["y"], a["nf"], a["alpha"], None, False, 0.5, True)
    return {k: w[k] for k in ("beta", "betaSE", "mu", "hat_diagonals")}


def _intercept_got(s, d):
    pk = _host(s["_pack"])
    return {"beta": pk[0], "betaSE": pk[1], "mu": _host(s["mu"].view()), "hat_diagonals": _host(s["hat_diagonals"].view())}


def _paramfit_build(which):
    rng = np.random.default_rng(7 + which * SEED_DECOY)
    means = np.exp(rng.uniform(np.log(2), np.log(5000), 337))
    disps = (0.05 + 3.0 / means + 0.2 * which) * np.exp(rng.normal(0, 0.4, 337))
    return {"in": OrderedDict(means=In(means, "pos"), disps=In(disps, "pos"))}


def _paramfit_call(h, d):
    """dsq_parametric_dispersion_fit_dev through ctypes (the wrapper of native.py reads the coefficients back)"""
    import torch
    out = torch.zeros(3, dtype=torch.float64, device=h["means"].device)            # coefs[2] + the status word
    L.check(L.lib().dsq_parametric_dispersion_fit_dev(_p(h["means"]), _p(h["disps"]), h["means"].numel(), _p(out),
                                                      C.c_void_p(out.data_ptr() + 16), _stream()))
    return {"out": out}


def _paramfit_got(s, d):
    h = _host(s["out"])
    assert int(h[2:3].view(np.int32)[0]) == 0, "the parametric fit reports status %d" % int(h[2:3].view(np.int32)[0])
    return {"coefs": h[:2].copy()}


# ---- Cook's distances and replaceOutliers on a design with cells
def _cooks_data(which, p=3, m=12, variant=0):
    """the cooksDistance shape of hp_reference.AUX_SHAPES (variant 0), or a second data set of another shape and other
    cells (variant 1: p = 4, m = 20) for the back-to-back and two-stream cases; mu and H from the oracle's own fit"""
    from oracle import oracle as O
    if variant:
        p, m = 4, 20
    c = H.make_case("factor", p, m, seed=1000 * p + m + which * SEED_DECOY, big_every=2)
    alpha = np.exp(c["log_alpha"])
    fit = O.fitBeta(c["y"], c["x"], c["nf"], alpha, c["contrast"], c["beta_start"], c["lam"], c["weights"], False, 1e-8, 100, True, 0.5,
                    want_mu=True, mu_floor=0.5)
    c["mu_h"] = np.where(np.isfinite(fit["mu"]), fit["mu"], 0.5)
    c["H_h"] = np.nan_to_num(fit["hat_diagonals"])
    c["cells"] = native.cell_index(c["x"])
    return c


def _cooks_build(variant=0):
    def build(which):
        c = _cooks_data(which, variant=variant)
        c["in"] = OrderedDict(y=In.gm(c["y"], "count"), nf=In.gm(c["nf"], "pos"), mu=In.gm(c["mu_h"], "pos"), H=In.gm(c["H_h"], "nonneg"))
        return c
    return build


def _cooks_call(h, d):
    return native.cooksDistance_dev(h["y"], h["nf"], h["mu"], h["H"], d["cells"], d["p"])


def _cooks_want(O, d, a):
    w = O.cooksDistance(a["y"], a["nf"], a["mu"], a["H"], d["x"])
    return {k: w[k] for k in ("cooks", "maxCooks", "robustDisp")}


def _cooks_got(s, d):
    return {"cooks": _host(s["cooks"].view()), "maxCooks": _host(s["maxCooks"]), "robustDisp": _host(s["robustDisp"])}


def _replace_build(variant=0):
    def build(which):
        from oracle import oracle as O
        c = _cooks_data(which, variant=variant)
        ck = O.cooksDistance(c["y"], c["nf"], c["mu_h"], c["H_h"], c["x"])["cooks"]
        c["cutoff"] = float(np.nanquantile(ck, 0.9))
        c["replaceable"] = (np.arange(c["m"]) % 3 != variant)             # (two `replaceable` vectors: the two variants)
        c["in"] = OrderedDict(y=In.gm(c["y"], "count"), nf=In.gm(c["nf"], "pos"), cooks=In.gm(np.nan_to_num(ck, nan=0.0), "nonneg"))
        return c
    return build


def _replace_call(h, d):
    return native.replaceOutliers_dev(h["y"], h["nf"], h["cooks"], d["cutoff"], d["replaceable"])


def _replace_want(O, d, a):
    w = O.replaceOutliers(a["y"], a["nf"], a["cooks"], d["cutoff"], d["replaceable"])
    assert w["replace"].sum() > 0
    return {"counts": w["counts"], "replace": w["replace"]}


def _replace_got(s, d):
    return {"counts": _host(s["counts"].view()), "replace": _host(s["replace"]) != 0}


# ---- weights_prep, xim, the layout converters: the C ABI directly
def _wprep_build(which):
    p, m = 5, 37
    rng = np.random.default_rng(p * 1000 + m + which * SEED_DECOY)
    x = simulate.design_factor(m, p)
    w = rng.uniform(0.02, 1.0, (N, m))
    w[rng.uniform(size=w.shape) < 0.05] = 0.0
    w[3 + which, x[:, 2] == 1] = 0.0                    # a level without a sample: weightsFail
    w[10 + which, x[:, p - 1] == 1] = 0.005             # ... only below the threshold
    return {"in": OrderedDict(w=In.gm(w, "weight"), x=In((other_coding(x) if which else x).T)), "x": x, "m": m, "p": p}


def _wprep_call(h, d):
    import torch
    w = h["w"]
    m, p, ld = d["m"], d["p"], w.ld
    wn, wf = torch.zeros_like(w.t), torch.zeros_like(w.t)
    fz = _empty(N, torch.int32, w.t)
    neg = torch.zeros(1, dtype=torch.int32, device=w.t.device)          # (|= 1: the caller zeroes it first, the header says)
    L.check(L.lib().dsq_weights_prep_dev(_p(w.t), _p(h["x"]), N, m, p, ld, 1e-2, _p(wn), _p(wf), _p(fz), _p(neg), _stream()))
    return {"w_norm": native.GeneMajor(wn, m), "w_floor": native.GeneMajor(wf, m), "fail": fz, "neg": neg}


def _wprep_want(O, d, a):
    from deseq2_amd.engine import _weights_ok_host
    w = a["w"]
    want = w / w.max(axis=1, keepdims=True)
    ok = _weights_ok_host(np.nan_to_num(want, nan=0.0), a["x"].T, 1e-2, True)
    return {"w_norm": want, "w_floor": np.where(np.isnan(want), want, np.maximum(want, 1e-6)), "fail": ~ok, "neg": np.zeros(1, np.int32)}


def _wprep_got(s, d):
    return {"w_norm": _host(s["w_norm"].view()), "w_floor": _host(s["w_floor"].view()), "fail": _host(s["fail"]) != 0, "neg": _host(s["neg"])}


def _xim_build(which):
    m = 64
    return {"in": OrderedDict(nf=In.gm(np.exp(np.random.default_rng(m + which * SEED_DECOY).normal(0, 0.3, (N, m))), "pos")), "m": m}


def _xim_call(h, d):
    import torch
    nf = h["nf"]
    out = _empty(1, torch.float64, nf.t)
    L.check(L.lib().dsq_xim_dev(_p(nf.t), N, nf.m, nf.ld, _p(h["ws"]), _p(out), _stream()))
    return {"xim": out}


def _xim_want(O, d, a):
    from deseq2_amd.engine import HostEngine
    return {"xim": np.array([HostEngine().xim(a["nf"])])}


def _conv_build(which):
    m = 37
    rng = np.random.default_rng(m + which * SEED_DECOY)
    a = rng.normal(size=(N, m))
    k = rng.integers(0, 2 ** 31 - 1, size=(N, m)).astype(np.int32)
    return {"in": OrderedDict(a_r=In(a.T), k_r=In(k.T, "count"), kf_r=In(k.T.astype(np.float64), "count"), a_g=In.gm(a)), "m": m}


def _conv_call(h, d):
    """the four layout converters in one case (tests/test_gpu_entry_memory.py::test_layout_converters)"""
    import torch
    m = d["m"]
    ld = native.gene_major_ld(m)
    lib = L.lib()
    dev = h["a_r"].device
    a_g = native.GeneMajor(torch.zeros((N, ld), dtype=torch.float64, device=dev), m)
    k_g = native.GeneMajor(torch.zeros((N, ld), dtype=torch.int32, device=dev), m)
    kf_g = native.GeneMajor(torch.zeros((N, ld), dtype=torch.int32, device=dev), m)
    bad = torch.zeros(2, dtype=torch.int32, device=dev)
    back = torch.empty((m, N), dtype=torch.float64, device=dev)
    L.check(lib.dsq_to_gene_major_f64(_p(h["a_r"]), _p(a_g.t), N, m, ld, _stream()))
    L.check(lib.dsq_to_gene_major_i32(_p(h["k_r"]), _p(k_g.t), N, m, ld, _stream()))
    L.check(lib.dsq_counts_f64_to_gene_major_i32(_p(h["kf_r"]), _p(kf_g.t), N, m, ld, _p(bad), _stream()))
    L.check(lib.dsq_from_gene_major_f64(_p(h["a_g"].t), _p(back), N, m, h["a_g"].ld, _stream()))
    return {"a_g": a_g, "k_g": k_g, "kf_g": kf_g, "bad": bad, "back": back}


def _conv_want(O, d, a):
    return {"to_gene_major_f64": a["a_r"].T, "to_gene_major_i32": a["k_r"].T, "counts_f64_to_gene_major_i32": a["kf_r"].T.astype(np.int32),
            "from_gene_major_f64": a["a_g"], "bad": np.zeros(1, np.int32)}


def _conv_got(s, d):
    return {"to_gene_major_f64": _host(s["a_g"].view()), "to_gene_major_i32": _host(s["k_g"].view()),
            "counts_f64_to_gene_major_i32": _host(s["kf_g"].view()), "from_gene_major_f64": _host(s["back"]).T, "bad": _host(s["bad"])[:1]}


# ================================================================================================ size factors and transforms
def _sf_build(which):
    from tests.test_gpu_size_factors import _counts
    return {"in": OrderedDict(y=In.gm(_counts(997, 48, seed=997 * 3 + 48 + which * SEED_DECOY, zeros=0.005), "count"))}


def _sf_call(h, d):
    return native.sizeFactors_dev(h["y"], workspace=h["ws"])


def _sf_want(O, d, a):
    from tests import sf_spec
    r = sf_spec.size_factors(O, a["y"])
    return {"sizeFactors": r["sizeFactors"], "loggeomeans": r["loggeomeans"], "status": np.array([r["status"]], np.int32)}


def _sf_got(s, d):
    pk = _host(s["_pack"])
    return {"sizeFactors": _host(s["sizeFactors"]), "loggeomeans": _host(s["loggeomeans"]), "status": pk[-1:].view(np.int32)[:1].copy()}


def _vst_data(which):
    from tests.test_gpu_vst import _counts, _sf
    n, m = 300, 65
    return _counts(n, m, seed=n + m + which * SEED_DECOY), _sf(m, m + which * SEED_DECOY)


def _vst_build(kind):
    def build(which):
        from tests.test_gpu_vst import _kind_params
        k, nf = _vst_data(which)
        params = _kind_params(kind, *_vst_data(0), variant=0)            # (host side: the true build's, a spline table included)
        return {"in": OrderedDict(y=In.gm(k, "count"), nf=In(nf, "pos")), "params": params, "kind": kind}
    return build


def _vst_call(h, d):
    return {"out": native.vst_dev(h["y"], h["nf"], d["kind"], **d["params"])}


def _vst_want(O, d, a):
    from tests import vst_spec
    return {"out": vst_spec.transform(O, a["y"], a["nf"], d["kind"], **d["params"])}


def _rowstats_call(h, d):
    return {"pack": native.vstRowStats_dev(h["y"], h["nf"])}


def _rowstats_want(O, d, a):
    from tests import vst_spec
    mean, mx = vst_spec.row_stats(a["y"], a["nf"])
    return {"rowMean": mean, "rowMax": mx}


def _rowstats_got(s, d):
    pk = _host(s["pack"])
    return {"rowMean": pk[0], "rowMax": pk[1]}


def _rlog_build(which):
    from tests.rlog_cases import inputs
    d = inputs(37, 65, which * SEED_DECOY, nf_matrix=False)
    if which:
        d["counts"][5] = 0                      # (another all-zero row: the flags differ)
    d["in"] = OrderedDict(y=In.gm(d["counts"], "count"), nf=In(d["nf"], "pos"), dispFit=In(d["dispFit"], "pos"))
    return d


def _rlog_call(h, d):
    return native.rlog_dev(h["y"], h["nf"], h["dispFit"], d["betaPriorVar"])


def _rlog_want(O, d, a):
    from tests import rlog_spec
    r = rlog_spec.rlog_fit(O, a["y"], a["nf"], a["dispFit"], d["betaPriorVar"])
    return {k: r[k] for k in ("rlog", "intercept", "iter", "flag")}


def _rlog_got(s, d):
    return {"rlog": _host(s["rlog"].view()), "intercept": _host(s["intercept"]), "iter": _host(s["iter"]), "flag": _host(s["flag"])}


def _unmix_build(which):
    from tests.test_gpu_unmix import _inputs
    x, pure = _inputs(150, 5, 6, seed=9 + which * SEED_DECOY)
    return {"in": OrderedDict(x=In.gm(x, "nonneg"), pure=In(pure, "nonneg")), "n": 150, "m": 6, "k": 5}


def _unmix_call(h, d):
    return native.unmix_dev(h["x"], h["pure"], alpha=0.01, power=1, workspace=h["ws"])


def _unmix_want(O, d, a):
    from tests import unmix_spec
    r = unmix_spec.unmix_fit(O, a["x"], a["pure"], power=1, alpha=0.01)
    return {k: r[k] for k in ("p", "loss", "iter", "flag")}


def _apeglm_build(which):
    from tests import apeglm_cases
    c = apeglm_cases.make(37, 14, 3, seed=99 + which * SEED_DECOY)
    c["no_shrink"] = np.array([True, False, False])
    c["Y"][4 * which] = 0                       # an all-zero row (not fitted: conv is NA), another one in the decoy
    c["in"] = OrderedDict(y=In.gm(c["Y"], "count"), x=In((other_coding(c["x"]) if which else c["x"]).T), nf=In(c["nf"], "pos"),
                          disp=In(c["disp"], "pos"), init=In(c["init"]))
    return c


def _apeglm_call(h, d):
    return native.apeglm_dev(h["y"], h["x"], h["nf"], h["disp"], d["coef"], d["no_shrink"], 0.3, init=h["init"], threshold=0.5)


def _apeglm_want(O, d, a):
    from tests import apeglm_cases, apeglm_spec
    r = apeglm_spec.fit(O, a["y"], a["x"].T, a["nf"], a["disp"], d["coef"], d["no_shrink"], 0.3, init=a["init"], threshold=0.5)
    return {k: np.asarray(r[k]) for k in apeglm_cases.SPEC_KEYS}


def _apeglm_got(s, d):
    from tests import apeglm_cases
    return {k: _host(s[k]) for k in apeglm_cases.SPEC_KEYS}


# ================================================================================================ exploration, count helpers
def _explore_build(which):
    from tests import explore_cases
    A = explore_cases.matrix(explore_cases.L + 5, 12, seed=112 + which * SEED_DECOY)
    n = A.shape[0]
    rows = np.sort(np.random.default_rng(5 + which).choice(n, 20, replace=False)).astype(np.int32)
    from tests import explore_spec
    centre = explore_spec.row_vars(A)[0][rows]
    return {"in": OrderedDict(x=In.gm(A), rows=In(rows, ("index", n)), centre=In(centre)), "n": n}


def _topvar_call(h, d):
    return native.top_var_dev(h["x"], ntop=25)


def _topvar_want(O, d, a):
    from tests import explore_spec
    mean, var = explore_spec.row_vars(a["x"])
    return {"rowMean": mean, "rowVar": var, "select": np.asarray(explore_spec.top_var(var, 25), np.int64)}


def _topvar_got(s, d):
    return {"rowMean": _host(s["rowMean"]), "rowVar": _host(s["rowVar"]), "select": _host(s["select"]).astype(np.int64)}


def _pairs_call(h, d):
    return {"gram": native.sample_pairs_dev(h["x"], "gram", rows=h["rows"], centre=h["centre"]),
            "dist": native.sample_pairs_dev(h["x"], "dist")}


def _pairs_want(O, d, a):
    from tests import explore_spec
    return {"gram": explore_spec.pair_sums(a["x"], "gram", rows=a["rows"], centre=a["centre"]), "dist": explore_spec.sample_dists(a["x"])}


def _counts_build(which):
    from tests.test_gpu_count_helpers import _counts
    n, m = 203, 12
    y = _counts(n, m, seed=5 + which * SEED_DECOY)
    rng = np.random.default_rng(11 + which)
    members = np.argsort((np.arange(m) + which) % 5, kind="stable").astype(np.int32)
    offsets = np.array([0, 3, 6, 8, 10, 12] if not which else [0, 2, 5, 8, 11, 12], np.int32)
    lib = np.exp(rng.normal(13, 0.3, m))
    return {"in": OrderedDict(y=In.gm(y, "count"), members=In(members, ("index", m)), offsets=In(offsets, ("offsets", m)),
                              lib=In(lib, "pos")), "m": m}


def _collapse_call(h, d):
    out, status = native.collapse_dev(h["y"], h["members"], h["offsets"])
    return {"out": out, "status": status}


def _collapse_want(O, d, a):
    from tests import counts_spec
    out, status = counts_spec.collapse(a["y"], a["members"], a["offsets"])
    return {"out": out, "status": np.array([status], np.int32)}


def _collapse_got(s, d):
    return {"out": _host(s["out"].view()), "status": _host(s["status"])}


def _colsums_want(O, d, a):
    from tests import counts_spec
    return {"sums": counts_spec.col_sums(a["y"])}


def _fpm_want(O, d, a):
    from tests import counts_spec
    return {"fpm": counts_spec.fpm(a["y"], a["lib"])}


# ================================================================================================ the local-regression trend
def _local_build(which):
    from tests import local_fit_cases as CS
    means, disps = CS._trend(129, 6 + which * SEED_DECOY)
    if which:
        disps[::10] = 5e-8                      # below 10 minDisp: left out of the fit set, N and k differ
    q = np.exp(np.random.default_rng(3 + which).uniform(np.log(means.min()), np.log(means.max()), 65))
    return {"in": OrderedDict(means=In(means, "pos"), disps=In(disps, "pos"), q=In(q, "pos")), "minDisp": CS.MIN_DISP}


def _local_call(h, d):
    return native.local_fit_dev(h["means"], h["disps"], d["minDisp"], eval_means=h["q"])


def _local_want(O, d, a):
    from tests import local_fit_spec as S
    fit = S.local_fit(O, a["means"], a["disps"], d["minDisp"])
    out, nsing = S.evaluate(O, fit, a["q"])
    Nf = fit[0].size
    return {"dispFit": out, "status": np.array([Nf, fit[3], nsing, int(Nf == 0)], np.int32), "x": fit[0], "y": fit[1], "w": fit[2]}


def _local_got(s, d):
    blk, n = _host(s["fit"]), 129
    Nf = int(blk[:2].view(np.int32)[0])
    out = {"dispFit": _host(s["dispFit"]), "status": _host(s["status"])}
    out.update({name: blk[4 + j * n: 4 + j * n + Nf] for j, name in enumerate("xyw")})
    return out


# ================================================================================================ results, contrasts, pt
def _results_build(which):
    from tests.test_gpu_results import _family
    n = 1025
    cols, kw = _family(n, "masks", seed=n * 13 + 5 + which * SEED_DECOY)
    beta, se, stat, pv, bm = cols
    theta = np.linspace(0.31 + 0.01 * which, 0.95, 50)
    up = lambda v: np.ascontiguousarray(v.T)
    return {"in": OrderedDict(beta=In(up(beta)), betaSE=In(up(se)), stat=In(up(stat)), pvalue=In(up(pv)), baseMean=In(bm, "nonneg"),
                              replace=In(kw["replace"].astype(np.int32)), na_mask=In(kw["na_mask"].astype(np.int32), "flag"),
                              theta=In(theta, "prob")), "n": n}


def _results_call(h, d):
    return native.results_dev(h["beta"], h["betaSE"], h["stat"], h["pvalue"], h["baseMean"], 1, replace=h["replace"], na_mask=h["na_mask"],
                              theta=h["theta"])


RES_COLS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue")


def _results_want(O, d, a):
    from tests import results_spec
    r = results_spec.results(O, a["beta"][1], a["betaSE"][1], a["stat"][1], a["pvalue"][1], a["baseMean"], replace=a["replace"] == 1,
                             na_mask=a["na_mask"], theta=a["theta"])
    out = {k: r[k] for k in RES_COLS + ("filtPadj", "cutoffs", "numRej")}
    out["status"] = 0
    return out


def _results_got(s, d):
    table, K = _host(s["table"]), s["K"]
    cut, nr, st = native.results_small(_host(s["_small"]), K)
    out = {k: table[i] for i, k in enumerate(RES_COLS)}
    out.update(filtPadj=_host(s["filtPadj"]).T, cutoffs=cut, numRej=nr, status=st)
    return out


def _contrast_data(which, variant=0):
    """tests/test_gpu_contrasts.py::_case: K = 3 contrasts on a factor design (design cells); variant 1: another shape and
    another contrast set, for the back-to-back case"""
    from tests.test_gpu_contrasts import _case
    p, m, n, K = ((6, 14, 65, 3), (4, 11, 40, 3))[variant]
    return _case("factor", p, m, n, K, seed=p * 1000 + m * 7 + K + which * SEED_DECOY)


def _contrast_build(variant=0):
    def build(which):
        d = _contrast_data(which, variant)
        d["cells"] = native.cell_index(d["x"])
        if which:
            d["x"] = other_coding(d["x"])
        d["in"] = OrderedDict(x=In(d["x"].T), nf=In.gm(d["nf"], "pos"), alpha=In(d["alpha"], "pos"), beta=In(d["beta"].T), lam=In(d["lam"], "pos"),
                              ct=In(d["ct"].T), az=In(d["allZero"], "flag"), y=In.gm(d["counts"], "count"), mask=In(d["mask"], "flag"),
                              rule=In(d["rule"], "flag"))
        return d
    return build


def _contrast_call(h, d):
    return native.contrasts_dev(h["x"], h["nf"], h["alpha"], h["beta"], h["lam"], h["ct"], allZero=h["az"], counts=h["y"],
                                sample_mask=h["mask"], rule_applies=h["rule"], cells=d["cells"])


def _contrast_want(O, d, a):
    from tests.test_gpu_contrasts import _reference
    e = dict(d, x=a["x"].T, nf=a["nf"], alpha=a["alpha"], beta=a["beta"].T, lam=a["lam"], ct=a["ct"].T, allZero=a["az"], counts=a["y"],
             mask=a["mask"], rule=a["rule"])
    return _reference(O, e)


def _contrast_got(s, d):
    from tests.test_gpu_contrasts import TAB
    table = _host(s["table"])
    out = {k: table[i].T for i, k in enumerate(TAB)}
    out["contrastAllZero"] = _host(s["contrastAllZero"]).T
    return out


def _pt_build(which):
    rng = np.random.Generator(np.random.PCG64(22 + which * SEED_DECOY))
    n, K = 300, 3
    q = rng.normal(0, 5, (n, K))
    q[rng.uniform(size=(n, K)) < 0.05] *= 1e3
    df = 10.0 ** rng.uniform(-1, 3, n)
    return {"in": OrderedDict(q=In(q.T), df=In(df, "pos"))}


def _pt_call(h, d):
    return {"p": native.pt_dev(h["q"], h["df"], "two_sided")}


def _pt_want(O, d, a):
    from deseq2_amd import student_t as T
    return {"p": T.pt_two_sided(O, a["q"].T, a["df"][:, None])}


# ================================================================================================ the stated synchronisers
def _sfi_build(which):
    from tests import sf_iterate_cases
    # maxit = 4: the true input stops by the tolerance in 3 iterations (flag 0); the decoy starts far from the optimum and is
    # cut off at maxit (flag 1) -- iter, evals and flag all differ
    c = sf_iterate_cases.solve_case(n_rows=97, m=5, seed=400 + which * SEED_DECOY, interleave=False, far=bool(which))
    c["in"] = OrderedDict(y=In.gm(c["counts"], "count"), mu=In.gm(c["mu"], "pos"), sf=In(c["sf"], "pos"), disp=In(c["disp"], "pos"),
                          rows=In(c["rows"], "flag"))
    return c


def _sfi_call(h, d):
    return native.sf_iterate_dev(h["y"], h["mu"], h["sf"], h["disp"], h["rows"], maxit=4, workspace=h["ws"])


SFI_KEYS = ("s", "sf", "F", "iter", "evals", "flag")


def _sfi_want(O, d, a):
    from tests import sf_iterate_spec
    r = sf_iterate_spec.solve(O, counts=a["y"], mu=a["mu"], sf=a["sf"], disp=a["disp"], rows=a["rows"], maxit=4)
    return {k: np.asarray(r[k]).reshape(-1) for k in SFI_KEYS}


def _sfi_got(s, d):
    return {k: _host(s[k]).reshape(-1) for k in SFI_KEYS}


_PRIOR_FACTORS = {"batch": np.arange(24) % 3, "condition": (np.arange(24) >= 12).astype(int)}


def _prior_build(which):
    rng = np.random.default_rng(5 + which * SEED_DECOY)
    n = 337
    cf = native.coef_factor_codes(_PRIOR_FACTORS)
    mle = rng.normal(0, 1.5, (n, cf.size))
    base, fit = np.exp(rng.normal(4, 2, n)), np.exp(rng.normal(-2, 1, n))
    az = (np.arange(n) % 17 == which).astype(np.int32)
    return {"in": OrderedDict(mle=In(mle.T), base=In(base, "pos"), fit=In(fit, "pos"), az=In(az, "flag")), "cf": cf}


def _prior_call(h, d):
    import torch
    got = native.estimateBetaPriorVar_dev(h["mle"], h["base"], h["fit"], h["az"], d["cf"])       # (reads back: a host array)
    return {"var": torch.as_tensor(np.asarray(got, np.float64)).to(h["mle"].device)}


def _prior_want(O, d, a):
    from deseq2_amd import core
    _, names = core.standard_model_matrix(_PRIOR_FACTORS)
    live = a["az"] == 0
    view = type("V", (), {"mcols": {"baseMean": a["base"][live], "dispFit": a["fit"][live]}})()
    want, _ = core.estimateBetaPriorVar(view, a["mle"].T[live], names, modelMatrixType="standard", factors=_PRIOR_FACTORS)
    return {"var": np.asarray(want)}


# ================================================================================================ the table
CASES = [
    # ---- dsq_fit_beta_dev
    Case("fit_beta-cells-p3", "dsq_fit_beta_dev", _beta_build("factor", 3, 37, weights=True), _beta_call, _beta_want, _beta_got),
    Case("fit_beta-wide-p12", "dsq_fit_beta_dev", _beta_build("cont", 12, 60), _beta_call, _beta_want, _beta_got),
    Case("fit_beta-r_layout-p4", "dsq_fit_beta_dev", _beta_r_build(False), _beta_r_call,
         lambda O, d, a: _beta_want(O, d, a, r_layout=True), _beta_r_got),
    Case("fit_beta-f64_counts", "dsq_fit_beta_dev", _beta_r_build(True), _beta_r_call,
         lambda O, d, a: _beta_want(O, d, a, r_layout=True), _beta_r_got, exempt="f64_counts"),
    # ---- dsq_fit_disp_dev / dsq_fit_disp_grid_dev
    Case("fit_disp-p3-m24", "dsq_fit_disp_dev", _disp_build("factor", 3, 24), _disp_call, _disp_want, _keys_got(DISP_KEYS)),
    Case("fit_disp-p4-m300", "dsq_fit_disp_dev", _disp_build("cont", 4, 300), _disp_call, _disp_want, _keys_got(DISP_KEYS)),
    Case("fit_disp-wide-p12", "dsq_fit_disp_dev", _disp_build("cont", 12, 60), _disp_call, _disp_want, _keys_got(DISP_KEYS)),
    Case("fit_disp_grid", "dsq_fit_disp_grid_dev", _disp_build("factor", 3, 24, grid=True), _grid_call, _grid_want, _keys_got(("log_alpha",))),
    # ---- aux and helper entries
    Case("prefit_moments", "dsq_prefit_moments_dev", _prefit_build,
         lambda h, d: native.prefitMoments_dev(h["y"], h["nf"], h["q"], h["a"], h["r"]), _prefit_want, _prefit_got),
    Case("linear_mu", "dsq_linear_mu_dev", _linmu_build, lambda h, d: native.linearMu_dev(h["y"], h["nf"], h["q"], h["a"], d["mu_floor"]),
         _linmu_want, lambda s, d: {"mu": _host(s.view())}),
    Case("nbinom_loglike", "dsq_nbinom_loglike_dev", _loglike_build, lambda h, d: native.nbinomLogLike_dev(h["y"], h["mu"], h["disp"]),
         lambda O, d, a: {"loglike": O.nbinomLogLike(a["y"], a["mu"], a["disp"], d["weights"], False)}, lambda s, d: {"loglike": _host(s)}),
    Case("intercept_fit", "dsq_intercept_fit_dev", _intercept_build,
         lambda h, d: native.interceptFit_dev(h["y"], h["nf"], h["alpha"], None, False, 0.5, True), _intercept_want, _intercept_got),
    Case("parametric_dispersion_fit", "dsq_parametric_dispersion_fit_dev", _paramfit_build, _paramfit_call,
         lambda O, d, a: {"coefs": O.parametricDispersionFit(a["means"], a["disps"])}, _paramfit_got),
    Case("cooks_distance", "dsq_cooks_distance_dev", _cooks_build(0), _cooks_call, _cooks_want, _cooks_got),
    Case("replace_outliers", "dsq_replace_outliers_dev", _replace_build(0), _replace_call, _replace_want, _replace_got),
    Case("weights_prep", "dsq_weights_prep_dev", _wprep_build, _wprep_call, _wprep_want, _wprep_got, constant=("neg",)),
    Case("xim", "dsq_xim_dev", _xim_build, _xim_call, _xim_want, lambda s, d: {"xim": _host(s["xim"])}, workspace=lambda d: 8 * d["m"]),
    Case("layout_converters", "dsq_to_gene_major_f64 / _i32 / dsq_counts_f64_to_gene_major_i32 / dsq_from_gene_major_f64", _conv_build,
         _conv_call, _conv_want, _conv_got, constant=("bad",)),
    # ---- size factors and transforms
    Case("size_factors", "dsq_size_factors_dev", _sf_build, _sf_call, _sf_want, _sf_got,
         workspace=lambda d: int(L.lib().dsq_size_factors_workspace_bytes(997, 48)), constant=("status",)),
    Case("vst-parametric", "dsq_vst_dev", _vst_build("parametric"), _vst_call, _vst_want, lambda s, d: {"out": _host(s["out"].view())}),
    Case("vst-spline", "dsq_vst_dev", _vst_build("spline"), _vst_call, _vst_want, lambda s, d: {"out": _host(s["out"].view())}),
    Case("vst_rowstats", "dsq_vst_rowstats_dev", _vst_build("normalized"), _rowstats_call, _rowstats_want, _rowstats_got),
    Case("rlog", "dsq_rlog_dev", _rlog_build, _rlog_call, _rlog_want, _rlog_got),
    Case("unmix", "dsq_unmix_dev", _unmix_build, _unmix_call, _unmix_want, _keys_got(("p", "loss", "iter", "flag")),
         workspace=lambda d: int(L.lib().dsq_unmix_workspace_bytes(d["n"], d["m"], d["k"]))),
    Case("apeglm", "dsq_apeglm_dev", _apeglm_build, _apeglm_call, _apeglm_want, _apeglm_got),
    # ---- exploration and count helpers
    Case("top_var", "dsq_top_var_dev", _explore_build, _topvar_call, _topvar_want, _topvar_got),
    Case("sample_pairs", "dsq_sample_pairs_dev", _explore_build, _pairs_call, _pairs_want, _keys_got(("gram", "dist"))),
    Case("collapse", "dsq_collapse_dev", _counts_build, _collapse_call, _collapse_want, _collapse_got, constant=("status",)),
    Case("col_sums", "dsq_col_sums_dev", _counts_build, lambda h, d: {"sums": native.col_sums_dev(h["y"])}, _colsums_want, _keys_got(("sums",))),
    Case("fpm", "dsq_fpm_dev", _counts_build, lambda h, d: {"fpm": native.fpm_dev(h["y"], h["lib"])}, _fpm_want,
         lambda s, d: {"fpm": _host(s["fpm"].view())}),
    # ---- dsq_local_fit_dev: fit and evaluate (the evaluation from the resident handle is the GPU test's second held call)
    Case("local_fit", "dsq_local_fit_dev", _local_build, _local_call, _local_want, _local_got),
    # ---- results
    Case("results", "dsq_results_dev", _results_build, _results_call, _results_want, _results_got, constant=("status",)),
    Case("contrasts", "dsq_contrasts_dev", _contrast_build(0), _contrast_call, _contrast_want, _contrast_got),
    Case("pt", "dsq_pt_dev", _pt_build, _pt_call, _pt_want, lambda s, d: {"p": _host(s["p"]).T}),          # ((K, n) = n x K column-major)
    # ---- the entries that state a host synchronisation themselves
    Case("sf_iterate", "dsq_sf_iterate_dev", _sfi_build, _sfi_call, _sfi_want, _sfi_got, exempt="sf_iterate",
         workspace=lambda d: max(8, int(L.lib().dsq_sf_iterate_workspace_bytes(d["counts"].shape[0], 5)))),
    Case("beta_prior_var", "dsq_beta_prior_var_dev", _prior_build, _prior_call, _prior_want, _keys_got(("var",)), exempt="beta_prior_var"),
]

# second data sets (another shape, other host tables) for the back-to-back and the two-stream cases
SECOND = {
    "cooks_distance": Case("cooks_distance-2", "dsq_cooks_distance_dev", _cooks_build(1), _cooks_call, _cooks_want, _cooks_got),
    "replace_outliers": Case("replace_outliers-2", "dsq_replace_outliers_dev", _replace_build(1), _replace_call, _replace_want, _replace_got),
    "fit_beta-cells-p3": Case("fit_beta-cells-p4", "dsq_fit_beta_dev", _beta_build("factor", 4, 24), _beta_call, _beta_want, _beta_got),
    "contrasts": Case("contrasts-2", "dsq_contrasts_dev", _contrast_build(1), _contrast_call, _contrast_want, _contrast_got),
    "results": Case("results-2", "dsq_results_dev",
                    lambda which: _results_build_n(63, which), _results_call, _results_want, _results_got, constant=("status",)),
}


def _results_build_n(n, which):
    from tests.test_gpu_results import _family
    cols, kw = _family(n, "random_na", seed=n * 13 + 9 + which * SEED_DECOY)
    beta, se, stat, pv, bm = cols
    up = lambda v: np.ascontiguousarray(v.T)
    return {"in": OrderedDict(beta=In(up(beta)), betaSE=In(up(se)), stat=In(up(stat)), pvalue=In(up(pv)), baseMean=In(bm, "nonneg"),
                              replace=In(np.zeros(n, np.int32), "flag"), na_mask=In(np.zeros(n, np.int32), "flag"),
                              theta=In(np.linspace(0.0 + 0.01 * which, 0.95, 20), "prob")), "n": n}


BY_NAME = {c.name: c for c in CASES}


# ================================================================================================ the DESeq chain
CHAIN_CONSTANT = ("maxCooks",)      # the call-by-call chain leaves it NA in every row after the refit (compared all the same)


def chain_inputs(which):
    """design "A" of tests/test_gpu_stream_ctx.py (600 x 48, four cells of 12: outliers are replaced and refitted on the side
    stream), and its decoy: the same builder on other seeds"""
    from tests.test_gpu_stream_ctx import _spike
    xa = simulate.design_batch_condition(48)
    s = which * SEED_DECOY
    da = simulate.make_counts(600 + 40 * which, xa, seed=3 + s, size_factors=np.exp(np.random.default_rng(1 + s).normal(0, .2, 48)))
    ca = da["counts"]
    if which:                                        # (make_counts drops its all-zero rows: as many rows as the true input has)
        ca = ca[:chain_inputs(0)[0].shape[0]]
    ca = _spike(ca, 5 + s)
    ca[which::53] = 0
    return ca, (other_coding(xa) if which else xa), da["size_factors"]


def chain_reference(O, counts, x, sf):
    """the oracle chain: the call-by-call DESeq() of core.py on HostEngine(oracle) (__graft_entry__.smoke)"""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    with np.errstate(all="ignore"):
        ref = core.DESeq(core.DESeqDataSet(counts, x, sizeFactors=sf, engine=HostEngine(O)))
    out = {k: np.array(np.asarray(ref.mcols[k], dtype=np.float64)) for k in sorted(ref.mcols) if k != "rowsForOptim"}
    out["trend"] = np.array(np.asarray(ref.dispersionFunction["coefficients"], dtype=np.float64))
    return out
