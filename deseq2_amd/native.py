"""The engine's entry points (include/deseq2_mi355x.h, bound in _lib) as Python functions: each builds the argument and
output blocks of its entry, calls it and raises DsqError on a non-zero status.  The three `.Call` stubs of the reference's
R/RcppExports.R:4,8,12 -- `fitDisp`, `fitBeta`, `fitDispGrid`: same argument names and order, same return-list members and
types (`fitBeta$iter` is double, `fitDisp$iter` integer, `contrast_num/denom` n x 1 matrices; src/DESeq2.cpp:268-276,
458-464, 512) --, the steps R runs around them (prefit moments, linear mu, log-likelihood, intercept fit, optim rows, the
dispersion trend, the beta prior, Cook's distances, outlier replacement), DESeq() behind one call, and what surrounds an
analysis: size factors (type "iterate" too), vst, rlog, unmix, results, contrasts, pt, sample PCA / distances,
collapseReplicates, fpm / fpkm.  Two flavours:
  name      numpy in, numpy out: host pointers in R layout through dsq_<entry> (what the R shim does)
  name_dev  torch CUDA tensors in and out through dsq_<entry>_dev on the current stream, n x m matrices as GeneMajor handles
"""
import ctypes as C

import numpy as np

from . import _lib as L


IGNORES_UNUSED_WEIGHTS = True      # weightsSEXP may be None when useWeightsSEXP is FALSE (HostEngine builds no all-ones matrix)


def _fcol(a, dtype=np.float64):
    """numpy array in R memory order (column-major)"""
    return np.asfortranarray(np.asarray(a, dtype=dtype))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _counts(y):
    y = np.asarray(y)
    if y.dtype.kind in "iu" or y.dtype == np.bool_:
        return np.asfortranarray(y.astype(np.int32, copy=False)), L.DSQ_Y_INT32
    return np.asfortranarray(y.astype(np.float64, copy=False)), L.DSQ_Y_FLOAT64


def _need_matrix(y):
    if y.ndim != 2:
        raise ValueError("counts must be a matrix")
    return y


def _host_nf(nf, n, m):
    """(nf, nf_is_vector) of a host `nf`: the m size factors or an n x m matrix"""
    nf = np.asarray(nf, np.float64)
    vec = nf.ndim == 1
    nf = np.ascontiguousarray(nf) if vec else _fcol(nf)
    if nf.shape != ((m,) if vec else (n, m)):
        raise ValueError("nf must be the m size factors or an n x m matrix")
    return nf, vec


def _cells(cells):
    """the cell_of / ncell pair of an argument block from the host array of design-cell ids (None: not known)"""
    return dict(cell_of=_ptr(cells) if cells is not None else None, ncell=(int(cells.max()) + 1) if cells is not None else 0)


def _scalar_len1(v, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size != 1:
        raise ValueError("%s must be a single value" % name)
    return float(a[0])


def fitBeta(ySEXP, xSEXP, nfSEXP, alpha_hatSEXP, contrastSEXP, beta_matSEXP, lambdaSEXP, weightsSEXP,
            useWeightsSEXP, tolSEXP, maxitSEXP, useQRSEXP, minmuSEXP, want_mu=False, mu_floor=0.0,
            want_hat=True, row_ranges=None):
    """row_ranges: [(lo, cnt), ...] walks the genes range by range through dsq_fit_beta_rows, as the R shim does
    between its R_CheckUserInterrupt() polls (the outputs of rows outside the ranges stay zero)"""
    y, ytype = _counts(ySEXP)
    x = _fcol(xSEXP); nf = _fcol(nfSEXP); b0 = _fcol(beta_matSEXP)
    if y.ndim != 2 or x.ndim != 2:
        raise ValueError("ySEXP and xSEXP must be matrices")
    n, m = y.shape
    p = x.shape[1]
    if x.shape[0] != m or nf.shape != (n, m) or b0.shape != (n, p):
        raise ValueError("non-conformable arguments")
    useW = bool(useWeightsSEXP)
    w = _fcol(weightsSEXP) if useW else None          # unused weights are neither converted nor uploaded
    if w is not None and w.shape != (n, m):
        raise ValueError("weights must be n x m")
    alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha_hatSEXP, np.float64).reshape(-1), (n,)))
    contrast = np.ascontiguousarray(np.asarray(contrastSEXP, np.float64).reshape(-1))
    lam = np.ascontiguousarray(np.asarray(lambdaSEXP, np.float64).reshape(-1))
    if contrast.size != p or lam.size != p:
        raise ValueError("contrast and lambda must have length ncol(x)")
    out = {"beta_mat": np.zeros((n, p), order="F"), "beta_var_mat": np.zeros((n, p), order="F"),
           "iter": np.zeros(n), "hat_diagonals": np.zeros((n, m), order="F") if want_hat else None,
           "contrast_num": np.zeros((n, 1)), "contrast_denom": np.zeros((n, 1)), "deviance": np.zeros(n)}
    mu = np.zeros((n, m), order="F") if want_mu else None
    a = L.DsqFitBetaArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, x=_ptr(x),
                         nf=_ptr(nf), nf_is_vector=0, alpha_hat=_ptr(alpha), contrast=_ptr(contrast),
                         beta_mat=_ptr(b0), lambda_=_ptr(lam), weights=_ptr(w) if useW else None,
                         useWeights=int(useW), tol=_scalar_len1(tolSEXP, "tol"),
                         maxit=int(_scalar_len1(maxitSEXP, "maxit")), useQR=int(bool(useQRSEXP)),
                         minmu=_scalar_len1(minmuSEXP, "minmu"))
    o = L.DsqFitBetaOut(beta_mat=_ptr(out["beta_mat"]), beta_var_mat=_ptr(out["beta_var_mat"]),
                        iter=_ptr(out["iter"]), hat_diagonals=_ptr(out["hat_diagonals"]),
                        contrast_num=_ptr(out["contrast_num"]), contrast_denom=_ptr(out["contrast_denom"]),
                        deviance=_ptr(out["deviance"]), mu=_ptr(mu), mu_floor=float(mu_floor))
    if row_ranges is None:
        L.check(L.lib().dsq_fit_beta(C.byref(a), C.byref(o)))
    else:
        for lo, cnt in row_ranges:
            L.check(L.lib().dsq_fit_beta_rows(C.byref(a), C.byref(o), int(lo), int(cnt)))
    if want_mu:
        out["mu"] = mu
    return out


def fitDisp(ySEXP, xSEXP, mu_hatSEXP, log_alphaSEXP, log_alpha_prior_meanSEXP, log_alpha_prior_sigmasqSEXP,
            min_log_alphaSEXP, kappa_0SEXP, tolSEXP, maxitSEXP, usePriorSEXP, weightsSEXP, useWeightsSEXP,
            weightThresholdSEXP, useCRSEXP):
    y, ytype = _counts(ySEXP)
    x = _fcol(xSEXP); mu = _fcol(mu_hatSEXP)
    n, m = y.shape
    p = x.shape[1]
    if x.shape[0] != m or mu.shape != (n, m):
        raise ValueError("non-conformable arguments")
    useW = bool(useWeightsSEXP)
    w = _fcol(weightsSEXP) if useW else None
    if w is not None and w.shape != (n, m):
        raise ValueError("weights must be n x m")
    la = np.ascontiguousarray(np.broadcast_to(np.asarray(log_alphaSEXP, np.float64).reshape(-1), (n,)))
    pm = np.ascontiguousarray(np.broadcast_to(np.asarray(log_alpha_prior_meanSEXP, np.float64).reshape(-1), (n,)))
    out = {k: np.zeros(n) for k in ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp",
                                     "last_dlp", "last_d2lp")}
    out["iter"] = np.zeros(n, dtype=np.int32)
    out["iter_accept"] = np.zeros(n, dtype=np.int32)
    a = L.DsqFitDispArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, x=_ptr(x),
                         mu_hat=_ptr(mu), log_alpha=_ptr(la), log_alpha_prior_mean=_ptr(pm),
                         log_alpha_prior_sigmasq=_scalar_len1(log_alpha_prior_sigmasqSEXP, "sigmasq"),
                         min_log_alpha=_scalar_len1(min_log_alphaSEXP, "min_log_alpha"),
                         kappa_0=_scalar_len1(kappa_0SEXP, "kappa_0"), tol=_scalar_len1(tolSEXP, "tol"),
                         maxit=int(_scalar_len1(maxitSEXP, "maxit")), usePrior=int(bool(usePriorSEXP)),
                         weights=_ptr(w), useWeights=int(useW),
                         weightThreshold=_scalar_len1(weightThresholdSEXP, "weightThreshold"),
                         useCR=int(bool(useCRSEXP)))
    o = L.DsqFitDispOut(**{k: _ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_fit_disp(C.byref(a), C.byref(o)))
    return out


def fitDispGrid(ySEXP, xSEXP, mu_hatSEXP, disp_gridSEXP, log_alpha_prior_meanSEXP,
                log_alpha_prior_sigmasqSEXP, usePriorSEXP, weightsSEXP, useWeightsSEXP, weightThresholdSEXP,
                useCRSEXP):
    y, ytype = _counts(ySEXP)
    x = _fcol(xSEXP); mu = _fcol(mu_hatSEXP)
    n, m = y.shape
    p = x.shape[1]
    if x.shape[0] != m or mu.shape != (n, m):
        raise ValueError("non-conformable arguments")
    useW = bool(useWeightsSEXP)
    w = _fcol(weightsSEXP) if useW else None
    grid = np.ascontiguousarray(np.asarray(disp_gridSEXP, np.float64).reshape(-1))
    pm = np.ascontiguousarray(np.broadcast_to(np.asarray(log_alpha_prior_meanSEXP, np.float64).reshape(-1), (n,)))
    la = np.zeros(n)
    a = L.DsqFitDispGridArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, x=_ptr(x),
                             mu_hat=_ptr(mu), disp_grid=_ptr(grid), ngrid=grid.size,
                             log_alpha_prior_mean=_ptr(pm),
                             log_alpha_prior_sigmasq=_scalar_len1(log_alpha_prior_sigmasqSEXP, "sigmasq"),
                             usePrior=int(bool(usePriorSEXP)), weights=_ptr(w), useWeights=int(useW),
                             weightThreshold=_scalar_len1(weightThresholdSEXP, "weightThreshold"),
                             useCR=int(bool(useCRSEXP)))
    o = L.DsqFitDispGridOut(log_alpha=_ptr(la))
    L.check(L.lib().dsq_fit_disp_grid(C.byref(a), C.byref(o)))
    return {"log_alpha": la}


_QR_CACHE = {}


def design_qr(x):
    """memoised thin QR of a model matrix (asked for by every prefit / linear_mu call of a DESeq())"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (x.shape, x.tobytes())
    v = _QR_CACHE.get(key)
    if v is None:
        if len(_QR_CACHE) > 64:
            _QR_CACHE.clear()
        v = _QR_CACHE[key] = _design_qr(x)
    return v


def _design_qr(x):
    """thin QR of the model matrix, taken on the host like the reference does with stats::qr
    (R/fitNbinomGLMs.R:139-143, R/core.R:2455-2457): Q (m x p), A = X R^-1 (m x p), R (p x p)"""
    x = np.asarray(x, np.float64)
    q, r = np.linalg.qr(x)
    a = x @ np.linalg.inv(r)
    return np.asfortranarray(q), np.asfortranarray(a), np.asfortranarray(r)


def prefitMoments(counts, nf, x, weights=None, useWeights=False):
    """baseMean / baseVar / allZero (R/core.R:2138-2146), roughDispEstimate (:2422-2437) and the
    QR least-squares start values (R/fitNbinomGLMs.R:139-145) in one kernel launch (dsq_prefit_moments)."""
    y, ytype = _counts(counts)
    nf = _fcol(nf)
    n, m = y.shape
    q, a, r = design_qr(x)
    p = q.shape[1]
    w = _fcol(weights) if useWeights else None
    bm = np.zeros(n); bv = np.zeros(n); az = np.zeros(n, dtype=np.int32); rd = np.zeros(n)
    b0 = np.zeros((n, p), order="F")
    args = L.DsqPrefitArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf),
                           nf_is_vector=0, weights=_ptr(w), useWeights=int(bool(useWeights)), q=_ptr(q), a=_ptr(a),
                           r=_ptr(r))
    out = L.DsqPrefitOut(baseMean=_ptr(bm), baseVar=_ptr(bv), allZero=_ptr(az), roughDisp=_ptr(rd),
                         beta_init=_ptr(b0))
    L.check(L.lib().dsq_prefit_moments(C.byref(args), C.byref(out)))
    return {"baseMean": bm, "baseVar": bv, "allZero": az.astype(bool), "roughDisp": rd, "beta_init": b0}


def linearMu(counts, nf, x, mu_floor=0.0):
    """linearModelMuNormalized (R/core.R:2454-2471) through dsq_linear_mu"""
    y, ytype = _counts(counts)
    nf = _fcol(nf)
    n, m = y.shape
    q, a, r = design_qr(x)
    q, a = _fcol(q), _fcol(a)
    mu = np.zeros((n, m), order="F")
    args = L.DsqPrefitArgs(n=n, m=m, p=q.shape[1], layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf),
                           nf_is_vector=0, weights=None, useWeights=0, q=_ptr(q), a=_ptr(a), r=None)
    L.check(L.lib().dsq_linear_mu(C.byref(args), float(mu_floor), _ptr(mu)))
    return mu


def nbinomLogLike(counts, mu, disp, weights, useWeights):
    """R/core.R:2208-2217 through dsq_nbinom_loglike"""
    y, ytype = _counts(counts)
    mu = _fcol(mu)
    n, m = y.shape
    w = _fcol(weights) if useWeights else None
    d = np.ascontiguousarray(np.broadcast_to(np.asarray(disp, np.float64).reshape(-1), (n,)))
    out = np.zeros(n)
    args = L.DsqLogLikeArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, mu=_ptr(mu),
                            disp=_ptr(d), weights=_ptr(w), useWeights=int(bool(useWeights)))
    L.check(L.lib().dsq_nbinom_loglike(C.byref(args), _ptr(out)))
    return out


def interceptFit(counts, nf, alpha, weights=None, useWeights=False, mu_floor=0.0, want_hat=True):
    """closed form of R/fitNbinomGLMs.R:99-137 (design ~ 1) through dsq_intercept_fit"""
    y, ytype = _counts(counts)
    nf = _fcol(nf)
    n, m = y.shape
    w = _fcol(weights) if useWeights else None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float64).reshape(-1), (n,)))
    b, se = np.zeros(n), np.zeros(n)
    mu = np.zeros((n, m), order="F")
    hat = np.zeros((n, m), order="F") if want_hat else None
    args = L.DsqInterceptArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf),
                              nf_is_vector=0, weights=_ptr(w), useWeights=int(bool(useWeights)), alpha=_ptr(a),
                              mu_floor=float(mu_floor))
    out = L.DsqInterceptOut(beta_log2=_ptr(b), betaSE=_ptr(se), mu=_ptr(mu), hat=_ptr(hat))
    L.check(L.lib().dsq_intercept_fit(C.byref(args), C.byref(out)))
    return {"beta": b, "betaSE": se, "mu": mu, "hat_diagonals": hat}


def optimRows(counts, x, nf, alpha, lam, weights, useWeights, beta_start, minmu=0.5):
    """fitNbinomGLMsOptim (R/fitNbinomGLMs.R:340-407) on the given rows through dsq_optim_rows.  lam: prior
    precisions on the log2 scale; beta_start: log2-scale start values."""
    y, ytype = _counts(counts)
    x = _fcol(x); nf = _fcol(nf)
    n, m = y.shape
    p = x.shape[1]
    w = _fcol(weights) if useWeights else None
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float64).reshape(-1), (n,)))
    lam = np.ascontiguousarray(np.asarray(lam, np.float64).reshape(-1))
    b0 = _fcol(np.asarray(beta_start, np.float64).reshape(n, p))
    beta = np.zeros((n, p), order="F"); se = np.zeros((n, p), order="F")
    conv = np.zeros(n, dtype=np.int32); mu = np.zeros((n, m), order="F"); ll = np.zeros(n)
    args = L.DsqOptimArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, x=_ptr(x), nf=_ptr(nf),
                          nf_is_vector=0, alpha_hat=_ptr(a), lambda_=_ptr(lam), weights=_ptr(w),
                          useWeights=int(bool(useWeights)), beta_start=_ptr(b0), minmu=float(minmu))
    out = L.DsqOptimOut(beta=_ptr(beta), betaSE=_ptr(se), conv=_ptr(conv), mu=_ptr(mu), logLike=_ptr(ll))
    L.check(L.lib().dsq_optim_rows(C.byref(args), C.byref(out)))
    return {"beta": beta, "betaSE": se, "conv": conv.astype(bool), "mu": mu, "logLike": ll}


def coef_factor_codes(factors, expanded=False):
    """the column coding dsq_deseq takes for the beta prior: for model.matrix(~ f1 + f2 + ...) of the design `factors`
    (ordered dict name -> integer level codes, 0 = reference level) 0 for the intercept and f >= 1 for a level
    indicator of the f-th factor; `expanded` = the same for the expanded model matrix (R/expanded.R:1-18: every level)"""
    codes = [0]
    for f, (_, lv) in enumerate(factors.items(), start=1):
        k = int(np.asarray(lv).max())
        codes += [f] * (k + 1 if expanded else k)
    return np.ascontiguousarray(codes, dtype=np.int32)


def estimateBetaPriorVarHost(mle_beta, baseMean, dispFit, allZero, coef_factor, prior_coef_factor=None, prior_coef_src=None):
    """dsq_beta_prior_var: estimateBetaPriorVar (R/core.R:1601-1689) on host arrays, no device work"""
    mle = _fcol(mle_beta)
    n, p = mle.shape
    bm, df = np.ascontiguousarray(baseMean, np.float64), np.ascontiguousarray(dispFit, np.float64)
    az = np.ascontiguousarray(np.asarray(allZero).astype(np.int32))
    cf = np.ascontiguousarray(coef_factor, dtype=np.int32)
    pcf = None if prior_coef_factor is None else np.ascontiguousarray(prior_coef_factor, dtype=np.int32)
    pcs = None if prior_coef_src is None else np.ascontiguousarray(prior_coef_src, dtype=np.int32)
    pp = p if pcf is None else pcf.size
    out = np.zeros(pp)
    args = L.DsqBetaPriorArgs(n=n, p=p, mle_beta=_ptr(mle), baseMean=_ptr(bm), dispFit=_ptr(df), allZero=_ptr(az),
                              coef_factor=_ptr(cf), expanded=int(pcf is not None), p_prior=int(pp),
                              prior_coef_factor=_ptr(pcf), prior_coef_src=_ptr(pcs), upperQuantile=0.05)
    L.check(L.lib().dsq_beta_prior_var(C.byref(args), _ptr(out)))
    return out


def estimateBetaPriorVar_dev(mle_beta, baseMean, dispFit, allZero, coef_factor, prior_coef_factor=None, prior_coef_src=None,
                             workspace=None):
    """dsq_beta_prior_var_dev on resident inputs: mle_beta a (p, n) float64 tensor (= n x p column-major), baseMean /
    dispFit float64 n-vectors, allZero an int32 n-vector, all on the device; the column coding as estimateBetaPriorVarHost
    takes it (host).  Returns the host vector (p values, or one per column of the expanded matrix); the call waits for the
    stream once.  workspace: a uint8 device tensor of dsq_beta_prior_var_workspace_bytes(n, columns) bytes to reuse."""
    import torch
    p, n = (1, mle_beta.numel()) if mle_beta.dim() == 1 else mle_beta.shape
    cf = np.ascontiguousarray(coef_factor, dtype=np.int32)
    pcf = None if prior_coef_factor is None else np.ascontiguousarray(prior_coef_factor, dtype=np.int32)
    pcs = None if prior_coef_src is None else np.ascontiguousarray(prior_coef_src, dtype=np.int32)
    pp = p if pcf is None else pcf.size
    out = np.zeros(pp)
    args = L.DsqBetaPriorArgs(n=n, p=p, mle_beta=_t_ptr(mle_beta), baseMean=_t_ptr(baseMean), dispFit=_t_ptr(dispFit),
                              allZero=_t_ptr(allZero), coef_factor=_ptr(cf), expanded=int(pcf is not None), p_prior=int(pp),
                              prior_coef_factor=_ptr(pcf), prior_coef_src=_ptr(pcs), upperQuantile=0.05)
    if workspace is None:
        wsb = int(L.lib().dsq_beta_prior_var_workspace_bytes(n, L.lib().dsq_beta_prior_var_columns(C.byref(args))))
        workspace = torch.empty(wsb, dtype=torch.uint8, device=mle_beta.device)
    L.check(L.lib().dsq_beta_prior_var_dev(C.byref(args), _ptr(out), _t_ptr(workspace), int(workspace.numel()), _stream()))
    return out


def DESeq(counts, x, sizeFactors=None, test="Wald", reduced=None, normalizationFactors=None, weights=None,
          minReplicatesForReplace=7, betaTol=1e-8, maxit=100, useQR=True,
          minmu=0.5, disp_maxit=100, useCR=True, assays=("mu", "H", "cooks"),
          betaPrior=False, factors=None, modelMatrixType=None, betaPriorVar=None, coef_factor=None,
          fitType="parametric", dispFit=None, geneEstOnly=False, dispPriorVar=None):
    """dsq_deseq: DESeq() behind ONE host-pointer call (what r_shim.c binds as _DESeq2_mi355x_DESeq; the R-side glue is
    in INTEGRATION.md).  counts: n x m integer matrix in R orientation; x: m x p model matrix; sizeFactors: m.  The three
    design-only quantities the R caller computes with qr() / qf() / trigamma() come from numpy / scipy here.  Returns the
    per-gene columns (NA = NaN; integer columns as float64 with NaN), the requested n x m assays, the dispersion
    function and the status counters.  fitType: "parametric" (a trend that does not fit is an error, DSQ_ERR_FIT: the R
    caller then takes the reference's route to locfit), "mean", or "parametric_or_mean" (the mean substituted on the device).
    A trend this entry does not fit (fitType = "local": local_fit below, or R's locfit; dispersionFunction<-): geneEstOnly =
    True returns after estimateDispersionsGeneEst; the caller evaluates its trend at res["baseMean"] and calls again with dispFit = those values
    (count outliers are then flagged but not replaced: the refit is the caller's, R/core.R:2484-2563).  dispPriorVar: the
    argument of estimateDispersionsMAP (R/core.R:989-994); required for m - p <= 3, where R's own estimate is a seeded
    Monte-Carlo match (:1155-1190) the library leaves to the caller."""
    from scipy import special as sps
    if fitType not in L.DSQ_FIT:
        raise ValueError("fitType should be one of %s" % sorted(L.DSQ_FIT))
    from scipy.stats import f as fdist
    y, ytype = _counts(counts)
    x = _fcol(x)
    n, m = y.shape
    p = x.shape[1]
    sf = None if sizeFactors is None or normalizationFactors is not None else np.ascontiguousarray(sizeFactors, dtype=np.float64)
    nfm = None if normalizationFactors is None else _fcol(normalizationFactors)
    wts = None if weights is None else _fcol(weights)
    q, a, r = design_qr(x)
    if m - p > 0:
        cutoff, evld = float(fdist.ppf(.99, p, m - p)), float(sps.polygamma(1, (m - p) / 2.0))
    else:
        cutoff, evld = 1.0, 1.0           # (the library rejects m <= p itself)
    wald = test == "Wald"
    if not wald and test != "LRT":
        raise ValueError("test should be either 'Wald' or 'LRT'")
    grid = np.ascontiguousarray(np.linspace(np.log(1e-8), np.log(max(10, m)), 20))          # R/wrappers.R:70-72
    xr = qr_ = rr_ = None
    p_red = 0
    if not wald and reduced is not None:
        red = _fcol(reduced)
        if not (red.shape[1] == 1 and (red == 1).all()):
            xr, p_red = red, red.shape[1]
            qr_, _, rr_ = design_qr(red)
    # nbinomWaldTest(betaPrior = TRUE): the model matrix of the prior pass and what its columns are (R/core.R:1374-1380)
    pcol, xe, cf, pcf = p, None, None, None
    if betaPrior:
        if not wald:
            raise ValueError("betaPrior: the Wald test only")
        mmt = modelMatrixType or ("expanded" if factors is not None else "standard")
        if factors is not None:
            cf = coef_factor_codes(factors)
        else:
            cf = np.ascontiguousarray(coef_factor if coef_factor is not None else [0] + [-1] * (p - 1), dtype=np.int32)
        if cf.size != p:
            raise ValueError("the design factors do not describe the %d columns of the model matrix" % p)
        if mmt == "expanded":
            if factors is None:
                raise ValueError("an expanded model matrix needs the design factors")
            from . import core
            xe = _fcol(core.makeExpandedModelMatrix(factors)[0])
            pcf = coef_factor_codes(factors, expanded=True)
            pcol = xe.shape[1]
    fit_in = None if dispFit is None else np.ascontiguousarray(dispFit, dtype=np.float64)
    if fit_in is not None and fit_in.shape != (n,):
        raise ValueError("dispFit needs one value per gene")
    bpv_in = None if betaPriorVar is None else np.ascontiguousarray(betaPriorVar, dtype=np.float64)
    if bpv_in is not None and bpv_in.size != pcol:
        raise ValueError("betaPriorVar needs one value per column of the (expanded) model matrix")
    f64 = lambda *sh: np.full(sh, np.nan, order="F")                    # noqa: E731
    i32 = lambda: np.full(n, -1, dtype=np.int32)                         # noqa: E731
    d = {k: f64(n) for k in ("baseMean", "baseVar", "dispGeneEst", "dispFit", "dispMAP", "dispersion", "betaIter",
                             "logLike", "maxCooks")}
    d.update({k: i32() for k in ("allZero", "dispGeneIter", "dispIter", "dispOutlier", "betaConv", "replace", "weightsFail")})
    d.update(beta=f64(n, pcol), betaSE=f64(n, pcol))
    if betaPrior:
        d["mle_beta"] = f64(n, p)
    if wald:
        d.update(stat=f64(n, pcol), pvalue=f64(n, pcol))
    else:
        d["logLikeReduced"] = f64(n)
    for k in assays:
        d[k] = np.zeros((n, m), order="F", dtype=np.int32 if k == "replaceCounts" else np.float64)
    args = L.DsqDeseqHostArgs(
        n=n, m=m, p=p, counts=_ptr(y), y_type=ytype, x=_ptr(x), sizeFactors=_ptr(sf), normalizationFactors=_ptr(nfm),
        weights=_ptr(wts), q=_ptr(q), r=_ptr(r), xrinv=_ptr(a),
        test=0 if wald else 1, x_reduced=_ptr(xr), q_reduced=_ptr(qr_), r_reduced=_ptr(rr_), p_reduced=int(p_red),
        minReplicatesForReplace=float(minReplicatesForReplace), cooksCutoff=cutoff,
        expVarLogDisp=evld, betaTol=float(betaTol), minmu=float(minmu), maxit=int(maxit), useQR=int(bool(useQR)),
        disp_maxit=int(disp_maxit), useCR=int(bool(useCR)), disp_grid=_ptr(grid), ngrid=int(grid.size),
        betaPrior=int(bool(betaPrior)), x_prior=_ptr(xe), p_prior=int(pcol), coef_factor=_ptr(cf),
        prior_coef_factor=_ptr(pcf), prior_coef_src=None, betaPriorVar=_ptr(bpv_in), fitType=L.DSQ_FIT[fitType],
        dispFit=_ptr(fit_in), geneEstOnly=int(bool(geneEstOnly)),
        dispPriorVar=0.0 if dispPriorVar is None else float(dispPriorVar))
    out = L.DsqDeseqHostOut(**{k: _ptr(v) for k, v in d.items()})
    L.check(L.lib().dsq_deseq(C.byref(args), C.byref(out)))
    res = {}
    for k, v in d.items():
        if v.dtype == np.int32 and k != "replaceCounts":
            f = v.astype(np.float64)
            f[v < 0] = np.nan
            res[k] = f
        else:
            res[k] = v
    res["status"] = {k: int(out.status[i]) for k, i in L.DSQ_ST.items()}
    mean_used = out.dispersionFunction[L.DSQ_SC_FIT_USED] == L.DSQ_FIT["mean"]
    given = out.dispersionFunction[L.DSQ_SC_FIT_USED] == L.DSQ_FIT["given"]
    res["dispersionFunction"] = {"fitType": "given" if given else "mean" if mean_used else "parametric",
                                 "coefficients": float(out.dispersionFunction[0]) if mean_used else np.array(out.dispersionFunction[0:2]),
                                 "varLogDispEsts": float(out.dispersionFunction[2]),
                                 "dispPriorVar": float(out.dispersionFunction[3])}
    if betaPrior:
        res["betaPriorVar"] = np.array(out.betaPriorVar[:pcol])
    res["cooksCutoff"] = cutoff
    res["df"] = p - (p_red if p_red else 1)
    return res


_CELL_CACHE = {}


def cell_index(x):
    """design cells (nOrMoreInCell, R/core.R:2366-2371): samples with identical model-matrix rows"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (x.shape, x.tobytes())
    v = _CELL_CACHE.get(key)
    if v is None:
        if len(_CELL_CACHE) > 64:
            _CELL_CACHE.clear()
        _, inv = np.unique(x, axis=0, return_inverse=True)
        v = _CELL_CACHE[key] = np.ascontiguousarray(inv.reshape(-1), dtype=np.int32)
    return v


def cooksDistance(counts, nf, mu, H, x):
    """calculateCooksDistance + recordMaxCooks (R/core.R:2333-2359) through dsq_cooks_distance;
    `x` is the dispersion model matrix."""
    y, ytype = _counts(counts)
    nf, mu, H = _fcol(nf), _fcol(mu), _fcol(H)
    n, m = y.shape
    cells = cell_index(x)
    ck = np.zeros((n, m), order="F")
    mx, rd = np.zeros(n), np.zeros(n)
    args = L.DsqCooksArgs(n=n, m=m, p=np.asarray(x).shape[1], layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype,
                          nf=_ptr(nf), nf_is_vector=0, mu=_ptr(mu), H=_ptr(H), **_cells(cells))
    out = L.DsqCooksOut(cooks=_ptr(ck), maxCooks=_ptr(mx), robustDisp=_ptr(rd))
    L.check(L.lib().dsq_cooks_distance(C.byref(args), C.byref(out)))
    return {"cooks": ck, "maxCooks": mx, "robustDisp": rd}


def replaceOutliers(counts, nf, cooks, cooksCutoff, replaceable, trim=0.2):
    """replaceOutliers (R/core.R:2069-2115) through dsq_replace_outliers"""
    y, ytype = _counts(counts)
    nf, ck = _fcol(nf), _fcol(cooks)
    n, m = y.shape
    rep = np.ascontiguousarray(np.asarray(replaceable).astype(np.int32))
    newc = np.zeros((n, m), dtype=np.int32, order="F")
    flag = np.zeros(n, dtype=np.int32)
    args = L.DsqReplaceArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf),
                            nf_is_vector=0, cooks=_ptr(ck), cooksCutoff=float(cooksCutoff), trim=float(trim),
                            replaceable=_ptr(rep))
    out = L.DsqReplaceOut(newCounts=_ptr(newc), replace=_ptr(flag))
    L.check(L.lib().dsq_replace_outliers(C.byref(args), C.byref(out)))
    return {"counts": newc, "replace": flag.astype(bool)}


def estimateSizeFactorsForMatrix(counts, type="ratio", geoMeans=None, controlGenes=None, normMatrix=None,
                                 want_loggeomeans=False):
    """estimateSizeFactorsForMatrix (R/core.R:535-578) through dsq_size_factors: host arrays in, the m size factors out.
    With normMatrix (estimateNormFactors, R/core.R:2159-2163) the n x m normalization factors are returned instead.
    type "poscounts" as estimateSizeFactors.DESeqDataSet runs it (R/methods.R:377-382).  controlGenes: 0-based indices
    or a logical vector.  A matrix whose every gene has a zero raises DsqError (DSQ_ERR_FIT)."""
    from .engine import control_flags
    if type == "iterate":
        raise NotImplementedError('type = "iterate" belongs to estimateSizeFactors on an object (core.estimateSizeFactors, '
                                  "VERDICT row f4): R's estimateSizeFactorsForMatrix has no such type")
    if type not in L.DSQ_SF:
        raise ValueError("type should be 'ratio' or 'poscounts'")
    y, ytype = _counts(counts)
    n, m = _need_matrix(y).shape
    gm = None
    if geoMeans is not None:
        gm = np.ascontiguousarray(geoMeans, dtype=np.float64).reshape(-1)
        if gm.size != n:
            raise ValueError("geoMeans should be as long as the number of rows of counts")
    ctl = control_flags(controlGenes, n)
    nm = None if normMatrix is None else _fcol(normMatrix)
    if nm is not None and nm.shape != (n, m):
        raise ValueError("normMatrix must have the shape of counts")
    sf = np.zeros(m); lgm = np.zeros(n); st = np.zeros(1, dtype=np.int32)
    nf = np.zeros((n, m), order="F") if nm is not None else None
    a = L.DsqSizeFactorArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, type=L.DSQ_SF[type],
                            geoMeans=_ptr(gm), control=_ptr(ctl), normMatrix=_ptr(nm), workspace=None, workspace_bytes=0)
    o = L.DsqSizeFactorOut(sizeFactors=_ptr(sf), loggeomeans=_ptr(lgm), normalizationFactors=_ptr(nf), status=_ptr(st))
    L.check(L.lib().dsq_size_factors(C.byref(a), C.byref(o)))
    res = nf if nm is not None else sf
    return (res, lgm) if want_loggeomeans else res


def _vst_args(kind, asymptDisp, extraPois, alpha, pc, table, eta, xi):
    """the formula part of DsqVstArgs; the spline table (5 x K: x | y | b | c | d) stays a host array"""
    if kind not in L.DSQ_VST:
        raise ValueError("kind should be one of %s" % ", ".join(L.DSQ_VST))
    tab = None
    if table is not None:
        tab = np.ascontiguousarray(table, dtype=np.float64)
        if tab.ndim != 2 or tab.shape[0] != 5:
            raise ValueError("the spline table is 5 x K: x | y | b | c | d")
    kw = dict(kind=L.DSQ_VST[kind], asymptDisp=float(0.0 if asymptDisp is None else asymptDisp),
              extraPois=float(0.0 if extraPois is None else extraPois), alpha=float(0.0 if alpha is None else alpha),
              pc=float(pc), spline=_ptr(tab), nknots=0 if tab is None else int(tab.shape[1]),
              eta=float(0.0 if eta is None else eta), xi=float(0.0 if xi is None else xi))
    return kw, tab


def vst(counts, nf, kind="parametric", asymptDisp=None, extraPois=None, alpha=None, pc=1.0, table=None, eta=None, xi=None,
        want_out=True, want_stats=False):
    """getVarianceStabilizedData / normTransform / counts(normalized = TRUE) (R/vst.R:146-193, R/helper.R:421-436) through
    dsq_vst: host arrays in R layout in, the n x m matrix out.  nf: the m size factors or an n x m matrix.  want_stats:
    also (rowMeans, row maxima) of the normalized counts."""
    y, ytype = _counts(counts)
    n, m = _need_matrix(y).shape
    nf, vec = _host_nf(nf, n, m)
    kw, tab = _vst_args(kind, asymptDisp, extraPois, alpha, pc, table, eta, xi)
    out = np.zeros((n, m), order="F") if want_out else None
    rmean = np.zeros(n) if want_stats else None
    rmax = np.zeros(n) if want_stats else None
    a = L.DsqVstArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf), nf_is_vector=int(vec), **kw)
    o = L.DsqVstOut(out=_ptr(out), rowMean=_ptr(rmean), rowMax=_ptr(rmax), bad=None)
    L.check(L.lib().dsq_vst(C.byref(a), C.byref(o)))
    if want_out and want_stats:
        return out, rmean, rmax
    return out if want_out else (rmean, rmax)


def rlog(counts, nf, dispFit, betaPriorVar, intercept=None, tol=1e-4, maxit=100, minmu=0.5):
    """the fit of rlogData (R/rlog.R:172-272) through dsq_rlog: host arrays in R layout in; dict(rlog n x m, intercept n
    (form A; None with an intercept given), iter, flag: 0 fitted, 1 row not fitted, 2 a non-finite coefficient).  nf: the
    m size factors or an n x m matrix; betaPriorVar on the log2 scale."""
    y, ytype = _counts(counts)
    n, m = _need_matrix(y).shape
    nf, vec = _host_nf(nf, n, m)
    disp = np.ascontiguousarray(np.broadcast_to(np.asarray(dispFit, np.float64), (n,)))
    icpt = None
    if intercept is not None:
        icpt = np.ascontiguousarray(intercept, dtype=np.float64)
        if icpt.shape != (n,):
            raise ValueError("intercept should be as long as the number of rows of object")
    out = np.zeros((n, m), order="F")
    oi = np.zeros(n) if icpt is None else None
    it = np.zeros(n)
    flag = np.zeros(n, dtype=np.int32)
    a = L.DsqRlogArgs(n=n, m=m, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf), nf_is_vector=int(vec),
                      dispFit=_ptr(disp), betaPriorVar=float(betaPriorVar), intercept=_ptr(icpt), tol=float(tol),
                      minmu=float(minmu), maxit=int(maxit))
    o = L.DsqRlogOut(rlog=_ptr(out), intercept=_ptr(oi), iter=_ptr(it), flag=_ptr(flag), bad=None)
    L.check(L.lib().dsq_rlog(C.byref(a), C.byref(o)))
    return {"rlog": out, "intercept": oi, "iter": it, "flag": flag}


def _apeglm_form(p, coef, no_shrink, prior_scale, prior_df, no_shrink_scale, threshold, tol, maxit):
    mask = 0
    for k, flag in enumerate(np.asarray(no_shrink, bool).reshape(-1)):
        mask |= int(flag) << k
    return dict(coef=int(coef), no_shrink=mask, prior_scale=float(prior_scale), prior_df=float(prior_df),
                no_shrink_scale=float(no_shrink_scale), has_threshold=int(threshold is not None),
                threshold=float(threshold) if threshold is not None else 0.0, tol=float(tol), maxit=int(maxit))


_APEGLM_OUT = (("map", "p"), ("sd", "p"), ("fsr", 1), ("thresh", 1), ("iter", 2), ("conv", 1), ("start", 1), ("objective", 1))


def apeglm(counts, x, nf, disp, coef, no_shrink, prior_scale, prior_df=1.0, no_shrink_scale=15.0, weights=None, init=None,
           threshold=None, tol=1e-8, maxit=100):
    """the apeglm posterior through dsq_apeglm: host arrays in R layout in (counts n x m, x m x p, nf
    the m size factors or an n x m matrix, weights n x m or None, init n x p or None; no_shrink a boolean mask of p);
    dict(map n x p, sd n x p, fsr, thresh, iter n x 2, conv, start, objective) out, NaN on the rows that are not fitted."""
    y, ytype = _counts(counts)
    n, m = _need_matrix(y).shape
    x = _fcol(np.asarray(x, np.float64))
    p = x.shape[1]
    nf, vec = _host_nf(nf, n, m)
    disp = np.ascontiguousarray(np.broadcast_to(np.asarray(disp, np.float64), (n,)))
    w = None if weights is None else _fcol(np.asarray(weights, np.float64))
    b0 = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    if (w is not None and w.shape != (n, m)) or (b0 is not None and b0.shape != (n, p)):
        raise ValueError("weights is n x m and init n x p")
    out = {k: np.zeros((n, p if c == "p" else c) if c != 1 else n) for k, c in _APEGLM_OUT}
    a = L.DsqApeglmArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_R, ld=0, y=_ptr(y), y_type=ytype, nf=_ptr(nf), nf_is_vector=int(vec),
                        x=_ptr(x), weights=_ptr(w), disp=_ptr(disp), init=_ptr(b0),
                        **_apeglm_form(p, coef, no_shrink, prior_scale, prior_df, no_shrink_scale, threshold, tol, maxit))
    o = L.DsqApeglmOut(bad=None, **{k: _ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_apeglm(C.byref(a), C.byref(o)))
    return out


_ASH_ROWS = ("PosteriorMean", "PosteriorSD", "NegativeProb", "PositiveProb", "lfsr", "le_T", "gt_mT")


def _ash_columns(betahat, sebetahat):
    b, s = np.asarray(betahat, np.float64), np.asarray(sebetahat, np.float64)
    if b.shape != s.shape or b.ndim not in (1, 2):
        raise ValueError("betahat and sebetahat are two vectors of one length, or two n x C matrices")
    return (_fcol(b.reshape(b.shape[0], -1)), _fcol(s.reshape(s.shape[0], -1)))


def ash(betahat, sebetahat, threshold=None, maxit=100):
    """adaptive shrinkage through dsq_ash: betahat / sebetahat host vectors of n, or n x C matrices of C
    independent columns; dict(PosteriorMean, PosteriorSD, NegativeProb, PositiveProb, lfsr, le_T, gt_mT: n x C, NaN on the rows
    that are not kept; pi, sd: C x DSQ_ASH_MAX_K; K, iter, flag: int32 of C; loglik: C) out."""
    b, s = _ash_columns(betahat, sebetahat)
    n, c = b.shape
    out = {k: np.zeros((n, c), order="F") for k in _ASH_ROWS}
    out.update(pi=np.zeros((c, L.DSQ_ASH_MAX_K)), sd=np.zeros((c, L.DSQ_ASH_MAX_K)), K=np.zeros(c, np.int32),
               iter=np.zeros(c, np.int32), flag=np.zeros(c, np.int32), loglik=np.zeros(c))
    a = L.DsqAshArgs(n=n, C=c, ld=n, betahat=_ptr(b), sebetahat=_ptr(s), has_threshold=int(threshold is not None),
                     threshold=float(threshold) if threshold is not None else 0.0, maxit=int(maxit))
    o = L.DsqAshOut(**{k: _ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_ash(C.byref(a), C.byref(o)))
    return out


_FIT_ERRORS = {1: "parametric dispersion fit failed", 2: "dispersion fit did not converge"}


def parametricDispersionFit(means, disps):
    """R/core.R:2166-2190 through dsq_parametric_dispersion_fit; raises RuntimeError with the
    reference's messages so the caller can fall back like R/core.R:885-893"""
    means = np.ascontiguousarray(means, dtype=np.float64)
    disps = np.ascontiguousarray(disps, dtype=np.float64)
    coefs = np.zeros(2)
    st = np.zeros(1, dtype=np.int32)
    L.check(L.lib().dsq_parametric_dispersion_fit(_ptr(means), _ptr(disps), means.size, _ptr(coefs), _ptr(st)))
    if st[0] != 0:
        raise RuntimeError(_FIT_ERRORS.get(int(st[0]), "parametric dispersion fit failed"))
    return coefs


def test_math(op, a, b=None, c=None):
    """Evaluate one device-math primitive on the GPU (parity hook, see dsq_test_math)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, np.float64), a.shape))
    c = None if c is None else np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float64), a.shape))
    out = np.empty_like(a)
    L.check(L.lib().dsq_test_math(int(op), _ptr(a), _ptr(b), _ptr(c), _ptr(out), a.size))
    return out


UNARY_OPS = {"exp": 0, "log": 1, "log1p": 2, "lgamma": 3, "digamma": 4, "trigamma": 5, "stirlerr": 6, "pnorm_upper2": 9}
# every op of the hook by name (include/deseq2_mi355x.h: dsq_test_math); 12 and up are the variants the kernels call
MATH_OPS = dict(UNARY_OPS, bd0=7, dnbinom_mu_log=8, pt_upper=10, pt_lower=11, log_full=12, log_pn=13, rcp_n=14, div_n=15,
                stirlerr_n=16, bd0_fast=17, lgamma_pair_lg=18, lgamma_pair_dg=19, pnorm_lower=20, pnorm_upper=21, nb_split=22,
                sf_log=23, sf_exp=24, order_key=25, order_roundtrip=26)


def unary(name, x):
    """n-vector log / exp / ... in the engine's pinned f64 arithmetic (csrc/dsq_math.hpp)"""
    x = np.asarray(x, np.float64)
    return test_math(UNARY_OPS[name], x.reshape(-1)).reshape(x.shape)


# ------------------------------------------------------------------------------------
# device-resident flavour: torch CUDA tensors, current stream, no host round trip
# ------------------------------------------------------------------------------------
def _t_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class GeneMajor:
    """n x m device matrix in the engine's native layout (row-major, leading dim ld)."""

    def __init__(self, tensor, m):
        assert tensor.dim() == 2 and tensor.is_contiguous()
        self.t = tensor
        self.n = tensor.shape[0]
        self.ld = tensor.shape[1]
        self.m = m

    def view(self):
        return self.t[:, : self.m]


def gene_major_ld(m):
    return (m + 7) & ~7


def _y_type(y):
    import torch
    return L.DSQ_Y_FLOAT64 if y.t.dtype == torch.float64 else L.DSQ_Y_INT32


def _f64_like(y):
    """an uninitialised GeneMajor float64 matrix of y's shape, padding columns zero (the kernel writes every sample column
    exactly once: only the padding, which it leaves alone, is cleared)"""
    import torch
    out = GeneMajor(torch.empty((y.n, y.ld), dtype=torch.float64, device=y.t.device), y.m)
    if y.ld > y.m:
        out.t[:, y.m:] = 0.0
    return out


def fitBeta_dev(y, x, nf, alpha_hat, contrast, beta_mat, lambda_, weights, useWeights, tol, maxit, useQR,
                minmu, want_hat=True, want_mu=False, mu_floor=0.0, nf_is_vector=False, cells=None):
    """All array arguments are torch CUDA tensors.  y / nf / weights: GeneMajor (y int32) --
    outputs hat_diagonals / mu are GeneMajor too; x: (m, p) column-major i.e. a (p, m)
    contiguous tensor is passed as `x` (see `design_to_device`)."""
    import torch
    assert isinstance(y, GeneMajor)
    n, m, ld = y.n, y.m, y.ld
    p = x.shape[0]
    dev = y.t.device
    f64 = dict(dtype=torch.float64, device=dev)
    # all per-gene outputs live in ONE buffer so the caller brings them to the host with one copy
    pack = torch.empty((2 * p + 4, n), **f64)
    out = {"beta_mat": pack[:p], "beta_var_mat": pack[p:2 * p], "iter": pack[2 * p], "contrast_num": pack[2 * p + 1],
           "contrast_denom": pack[2 * p + 2], "deviance": pack[2 * p + 3]}
    hat = GeneMajor(torch.empty((n, ld), **f64), m) if want_hat else None
    mu = GeneMajor(torch.empty((n, ld), **f64), m) if want_mu else None
    if nf_is_vector:
        nf_ptr = _t_ptr(nf)
    else:
        assert isinstance(nf, GeneMajor) and nf.ld == ld
        nf_ptr = _t_ptr(nf.t)
    if useWeights:
        assert isinstance(weights, GeneMajor) and weights.ld == ld
    a = L.DsqFitBetaArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                         y_type=L.DSQ_Y_INT32, x=_t_ptr(x), nf=nf_ptr, nf_is_vector=int(nf_is_vector),
                         alpha_hat=_t_ptr(alpha_hat), contrast=_t_ptr(contrast), beta_mat=_t_ptr(beta_mat),
                         lambda_=_t_ptr(lambda_), weights=_t_ptr(weights.t) if useWeights else None,
                         useWeights=int(bool(useWeights)), tol=float(tol), maxit=int(maxit),
                         useQR=int(bool(useQR)), minmu=float(minmu), **_cells(cells))
    o = L.DsqFitBetaOut(beta_mat=_t_ptr(out["beta_mat"]), beta_var_mat=_t_ptr(out["beta_var_mat"]),
                        iter=_t_ptr(out["iter"]), hat_diagonals=_t_ptr(hat.t) if hat else None,
                        contrast_num=_t_ptr(out["contrast_num"]), contrast_denom=_t_ptr(out["contrast_denom"]),
                        deviance=_t_ptr(out["deviance"]), mu=_t_ptr(mu.t) if mu else None,
                        mu_floor=float(mu_floor))
    L.check(L.lib().dsq_fit_beta_dev(C.byref(a), C.byref(o), _stream()))
    out["hat_diagonals"] = hat
    out["mu"] = mu
    out["_pack"] = pack
    return out


def fitDisp_dev(y, x, mu_hat, log_alpha, log_alpha_prior_mean, log_alpha_prior_sigmasq, min_log_alpha,
                kappa_0, tol, maxit, usePrior, weights, useWeights, weightThreshold, useCR, want_d2lp=True, cells=None):
    import torch
    assert isinstance(y, GeneMajor) and isinstance(mu_hat, GeneMajor) and mu_hat.ld == y.ld
    n, m, ld = y.n, y.m, y.ld
    p = x.shape[0]
    dev = y.t.device
    f64 = dict(dtype=torch.float64, device=dev)
    keys = ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp", "last_d2lp")
    pack = torch.empty((len(keys) + 1, n), **f64)       # one buffer, one device-to-host copy for the caller
    out = {k: pack[i] for i, k in enumerate(keys)}
    if not want_d2lp:
        out["last_d2lp"] = None
    ints = pack[len(keys)].view(torch.int32)            # the last row holds the two int32 counters
    out["iter"], out["iter_accept"] = ints[:n], ints[n:]
    a = L.DsqFitDispArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                         y_type=L.DSQ_Y_INT32, x=_t_ptr(x), mu_hat=_t_ptr(mu_hat.t), log_alpha=_t_ptr(log_alpha),
                         log_alpha_prior_mean=_t_ptr(log_alpha_prior_mean),
                         log_alpha_prior_sigmasq=float(log_alpha_prior_sigmasq),
                         min_log_alpha=float(min_log_alpha), kappa_0=float(kappa_0), tol=float(tol),
                         maxit=int(maxit), usePrior=int(bool(usePrior)),
                         weights=_t_ptr(weights.t) if useWeights else None, useWeights=int(bool(useWeights)),
                         weightThreshold=float(weightThreshold), useCR=int(bool(useCR)), **_cells(cells))
    o = L.DsqFitDispOut(**{k: _t_ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_fit_disp_dev(C.byref(a), C.byref(o), _stream()))
    out = {k: v for k, v in out.items() if v is not None}
    out["_pack"] = pack
    return out


def fitDispGrid_dev(y, x, mu_hat, disp_grid, log_alpha_prior_mean, log_alpha_prior_sigmasq, usePrior, weights,
                    useWeights, weightThreshold, useCR, cells=None):
    import torch
    assert isinstance(y, GeneMajor) and isinstance(mu_hat, GeneMajor) and mu_hat.ld == y.ld
    n, m, ld = y.n, y.m, y.ld
    p = x.shape[0]
    la = torch.empty(n, dtype=torch.float64, device=y.t.device)
    a = L.DsqFitDispGridArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                             y_type=L.DSQ_Y_INT32, x=_t_ptr(x), mu_hat=_t_ptr(mu_hat.t),
                             disp_grid=_t_ptr(disp_grid), ngrid=int(disp_grid.numel()),
                             log_alpha_prior_mean=_t_ptr(log_alpha_prior_mean),
                             log_alpha_prior_sigmasq=float(log_alpha_prior_sigmasq), usePrior=int(bool(usePrior)),
                             weights=_t_ptr(weights.t) if useWeights else None, useWeights=int(bool(useWeights)),
                             weightThreshold=float(weightThreshold), useCR=int(bool(useCR)), **_cells(cells))
    o = L.DsqFitDispGridOut(log_alpha=_t_ptr(la))
    L.check(L.lib().dsq_fit_disp_grid_dev(C.byref(a), C.byref(o), _stream()))
    return {"log_alpha": la}


def to_gene_major(t_r, dtype=None):
    """(n, m) torch CUDA tensor holding an R-layout matrix, given as its TRANSPOSE storage:
    pass a contiguous (m, n) tensor (column-major n x m).  Returns GeneMajor."""
    import torch
    m, n = t_r.shape
    ld = gene_major_ld(m)
    if t_r.dtype == torch.int32:
        dst = torch.zeros((n, ld), dtype=torch.int32, device=t_r.device)
        L.check(L.lib().dsq_to_gene_major_i32(_t_ptr(t_r), _t_ptr(dst), n, m, ld, _stream()))
    else:
        assert t_r.dtype == torch.float64
        dst = torch.zeros((n, ld), dtype=torch.float64, device=t_r.device)
        L.check(L.lib().dsq_to_gene_major_f64(_t_ptr(t_r), _t_ptr(dst), n, m, ld, _stream()))
    return GeneMajor(dst, m)


def from_gene_major(gm):
    """GeneMajor f64 -> contiguous (m, n) tensor = column-major n x m (R layout)."""
    import torch
    dst = torch.empty((gm.m, gm.n), dtype=torch.float64, device=gm.t.device)
    L.check(L.lib().dsq_from_gene_major_f64(_t_ptr(gm.t), _t_ptr(dst), gm.n, gm.m, gm.ld, _stream()))
    return dst


def sizeFactors_dev(y, type="ratio", geoMeans=None, control=None, normMatrix=None, workspace=None):
    """dsq_size_factors_dev on resident counts: y GeneMajor (int32 or float64), geoMeans an n-vector on the device,
    control n flags (host or device, int32), normMatrix GeneMajor with y's ld.  Nothing is read back: sizeFactors (m),
    loggeomeans (n) and normalizationFactors (GeneMajor) are device tensors; `_pack` = the m size factors followed by
    the status word (int32 view of its last element), for callers that want both with one copy."""
    import torch
    assert isinstance(y, GeneMajor)
    n, m, ld = y.n, y.m, y.ld
    dev = y.t.device
    pack = torch.zeros(m + 1, dtype=torch.float64, device=dev)
    lgm = torch.empty(n, dtype=torch.float64, device=dev)
    nf = None
    if normMatrix is not None:
        assert isinstance(normMatrix, GeneMajor) and normMatrix.ld == ld and normMatrix.n == n
        nf = GeneMajor(torch.zeros((n, ld), dtype=torch.float64, device=dev), m)
    if control is not None and not torch.is_tensor(control):
        control = torch.as_tensor(np.ascontiguousarray(control, dtype=np.int32), device=dev)
    wsb = int(L.lib().dsq_size_factors_workspace_bytes(n, m))
    ws = workspace if workspace is not None else torch.empty(wsb, dtype=torch.uint8, device=dev)
    a = L.DsqSizeFactorArgs(n=n, m=m, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t), y_type=_y_type(y),
                            type=L.DSQ_SF[type],
                            geoMeans=_t_ptr(geoMeans), control=_t_ptr(control),
                            normMatrix=_t_ptr(normMatrix.t) if normMatrix is not None else None,
                            workspace=_t_ptr(ws), workspace_bytes=int(ws.numel()))
    o = L.DsqSizeFactorOut(sizeFactors=_t_ptr(pack), loggeomeans=_t_ptr(lgm),
                           normalizationFactors=_t_ptr(nf.t) if nf is not None else None,
                           status=C.c_void_p(pack.data_ptr() + 8 * m))
    L.check(L.lib().dsq_size_factors_dev(C.byref(a), C.byref(o), _stream()))
    # (the workspace is stream-ordered scratch: torch's caching allocator hands it out again only to work enqueued later)
    return {"sizeFactors": pack[:m], "loggeomeans": lgm, "normalizationFactors": nf, "_pack": pack}


def _vst_dev_args(y, nf):
    import torch
    assert isinstance(y, GeneMajor)
    vec = torch.is_tensor(nf)
    if not vec:
        assert isinstance(nf, GeneMajor) and nf.ld == y.ld and nf.n == y.n
    else:
        assert nf.dtype == torch.float64 and nf.numel() == y.m and nf.is_contiguous()
    return dict(n=y.n, m=y.m, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=y.ld, y=_t_ptr(y.t), y_type=_y_type(y),
                nf=_t_ptr(nf if vec else nf.t), nf_is_vector=int(vec))


def vst_dev(y, nf, kind="parametric", asymptDisp=None, extraPois=None, alpha=None, pc=1.0, table=None, eta=None, xi=None,
            bad=None, out=None):
    """dsq_vst_dev on resident counts: y GeneMajor (int32 or float64), nf the m size factors (a device tensor) or a
    GeneMajor matrix with y's ld; the spline table is a host array (5 x K).  Returns the transformed matrix as a GeneMajor
    handle (padding columns zero; `out`: a GeneMajor of y's shape to write into); nothing is read back."""
    kw, tab = _vst_args(kind, asymptDisp, extraPois, alpha, pc, table, eta, xi)
    if out is None:
        out = _f64_like(y)
    assert out.n == y.n and out.ld == y.ld and out.m == y.m
    a = L.DsqVstArgs(**_vst_dev_args(y, nf), **kw)
    o = L.DsqVstOut(out=_t_ptr(out.t), rowMean=None, rowMax=None, bad=_t_ptr(bad))
    L.check(L.lib().dsq_vst_dev(C.byref(a), C.byref(o), _stream()))
    return out


def vstRowStats_dev(y, nf):
    """dsq_vst_rowstats_dev: a (2, n) device tensor, row 0 = rowMeans, row 1 = row maxima of counts / nf"""
    import torch
    pack = torch.empty((2, y.n), dtype=torch.float64, device=y.t.device)
    a = L.DsqVstArgs(**_vst_dev_args(y, nf), kind=L.DSQ_VST["normalized"])
    o = L.DsqVstOut(out=None, rowMean=_t_ptr(pack[0]), rowMax=_t_ptr(pack[1]), bad=None)
    L.check(L.lib().dsq_vst_rowstats_dev(C.byref(a), C.byref(o), _stream()))
    return pack


def rlog_dev(y, nf, dispFit, betaPriorVar, intercept=None, tol=1e-4, maxit=100, minmu=0.5, bad=None, out=None):
    """dsq_rlog_dev on resident counts: y GeneMajor (int32 or float64), nf the m size factors (a device tensor) or a
    GeneMajor matrix with y's ld, dispFit / intercept float64 device vectors of n.  Returns dict(rlog: GeneMajor (padding
    columns zero; `out`: a GeneMajor of y's shape to write into), intercept (form A) / iter: float64 tensors, flag: int32
    tensor); nothing is read back."""
    import torch
    dev = y.t.device
    if out is None:
        out = _f64_like(y)
    assert out.n == y.n and out.ld == y.ld and out.m == y.m
    assert dispFit.dtype == torch.float64 and dispFit.numel() == y.n and dispFit.is_contiguous()
    if intercept is not None:
        assert intercept.dtype == torch.float64 and intercept.numel() == y.n and intercept.is_contiguous()
    pack = torch.empty((2, y.n), dtype=torch.float64, device=dev)
    flag = torch.empty(y.n, dtype=torch.int32, device=dev)
    a = L.DsqRlogArgs(**_vst_dev_args(y, nf), dispFit=_t_ptr(dispFit), betaPriorVar=float(betaPriorVar),
                      intercept=_t_ptr(intercept), tol=float(tol), minmu=float(minmu), maxit=int(maxit))
    o = L.DsqRlogOut(rlog=_t_ptr(out.t), intercept=_t_ptr(pack[0]) if intercept is None else None, iter=_t_ptr(pack[1]),
                     flag=_t_ptr(flag), bad=_t_ptr(bad))
    L.check(L.lib().dsq_rlog_dev(C.byref(a), C.byref(o), _stream()))
    return {"rlog": out, "intercept": pack[0] if intercept is None else None, "iter": pack[1], "flag": flag}


def apeglm_dev(y, x, nf, disp, coef, no_shrink, prior_scale, prior_df=1.0, no_shrink_scale=15.0, weights=None, init=None,
               threshold=None, tol=1e-8, maxit=100, bad=None):
    """dsq_apeglm_dev on resident counts: y GeneMajor (int32 or float64), x an (m, p) host array or a device tensor holding
    it column-major, nf the m size factors (a device tensor) or a GeneMajor matrix with y's ld, weights a GeneMajor float64
    matrix with y's ld or None, disp a float64 device vector of n, init an (n, p) contiguous float64 device tensor or None.
    Returns one (n, 2 p + 8) float64 device tensor `pack` and the dict of its column views (map, sd, fsr, thresh, iter,
    conv, start, objective); nothing is read back."""
    import torch
    dev = y.t.device
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).T)).to(dev)      # (p, m) contiguous = m x p column-major
    p = x.shape[0]
    assert x.dtype == torch.float64 and x.is_contiguous() and x.shape[1] == y.m
    assert disp.dtype == torch.float64 and disp.numel() == y.n and disp.is_contiguous()
    if weights is not None:
        assert isinstance(weights, GeneMajor) and weights.ld == y.ld and weights.n == y.n and weights.t.dtype == torch.float64
    if init is not None:
        assert init.dtype == torch.float64 and tuple(init.shape) == (y.n, p) and init.is_contiguous()
    out, at = {}, 0
    pack = torch.empty(y.n * (2 * p + 8), dtype=torch.float64, device=dev)
    for k, c in _APEGLM_OUT:
        c = p if c == "p" else c
        out[k] = pack[at:at + y.n * c].view((y.n, c) if c != 1 else (y.n,))
        at += y.n * c
    a = L.DsqApeglmArgs(**_vst_dev_args(y, nf), p=p, x=_t_ptr(x), weights=_t_ptr(None if weights is None else weights.t),
                        disp=_t_ptr(disp), init=_t_ptr(init),
                        **_apeglm_form(p, coef, no_shrink, prior_scale, prior_df, no_shrink_scale, threshold, tol, maxit))
    o = L.DsqApeglmOut(bad=_t_ptr(bad), **{k: _t_ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_apeglm_dev(C.byref(a), C.byref(o), _stream()))
    out["_pack"] = pack
    return out


def ash_dev(betahat, sebetahat, threshold=None, maxit=100, workspace=None):
    """dsq_ash_dev on resident columns: betahat / sebetahat float64 device tensors of shape (C, n), contiguous (column c of the
    header's n x C at [c * n]).  The call synchronises the current stream (the host decides every step from a record read
    back).  Returns the dict of device tensors: the seven per-row outputs (C, n) as views of `_pack` (7, C, n); pi, sd
    (C, DSQ_ASH_MAX_K) and loglik (C) as views of `_small`; K, iter, flag (C,) int32 as views of `_ints`.  workspace: a uint8
    device tensor of dsq_ash_workspace_bytes(n, C) bytes to reuse."""
    import torch
    assert betahat.dtype == torch.float64 and sebetahat.dtype == torch.float64 and betahat.dim() == 2
    assert betahat.shape == sebetahat.shape and betahat.is_contiguous() and sebetahat.is_contiguous()
    c, n = betahat.shape
    dev = betahat.device
    pack = torch.empty((7, c, n), dtype=torch.float64, device=dev)
    small = torch.empty(c * (2 * L.DSQ_ASH_MAX_K + 1), dtype=torch.float64, device=dev)
    ints = torch.empty((3, c), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(int(L.lib().dsq_ash_workspace_bytes(n, c)), dtype=torch.uint8, device=dev)
    ck = c * L.DSQ_ASH_MAX_K
    out = {k: pack[i] for i, k in enumerate(_ASH_ROWS)}
    out.update(pi=small[:ck].view(c, L.DSQ_ASH_MAX_K), sd=small[ck:2 * ck].view(c, L.DSQ_ASH_MAX_K), loglik=small[2 * ck:],
               K=ints[0], iter=ints[1], flag=ints[2])
    a = L.DsqAshArgs(n=n, C=c, ld=n, betahat=_t_ptr(betahat), sebetahat=_t_ptr(sebetahat), has_threshold=int(threshold is not None),
                     threshold=float(threshold) if threshold is not None else 0.0, maxit=int(maxit))
    o = L.DsqAshOut(**{k: _t_ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_ash_dev(C.byref(a), C.byref(o), _t_ptr(workspace), int(workspace.numel()), _stream()))
    out.update(_pack=pack, _small=small, _ints=ints)
    return out


def _unmix_form(alpha, shift, power, maxit):
    return dict(has_alpha=int(alpha is not None), has_shift=int(shift is not None),
                alpha=float(alpha) if alpha is not None else 0.0, shift=float(shift) if shift is not None else 0.0,
                power=int(power), maxit=int(maxit))


def unmix(x, pure, alpha=None, shift=None, power=1, maxit=200):
    """the fits of unmix() (R/helper.R:96-112) through dsq_unmix: host arrays in R layout in (x n x m, pure n x k);
    dict(p m x k, loss m, iter m, flag m) out.  mix = p / rowSums(p) is the caller's."""
    x, pure = _fcol(x), _fcol(pure)
    if x.ndim != 2 or pure.ndim != 2 or pure.shape[0] != x.shape[0]:
        raise ValueError("x and pure must be matrices with the same number of rows")
    (n, m), k = x.shape, pure.shape[1]
    p, loss = np.zeros((m, k)), np.zeros(m)
    it, flag = np.zeros(m, np.int32), np.zeros(m, np.int32)
    a = L.DsqUnmixArgs(n=n, m=m, k=k, ld=0, x=_ptr(x), pure=_ptr(pure), **_unmix_form(alpha, shift, power, maxit))
    o = L.DsqUnmixOut(p=_ptr(p), loss=_ptr(loss), iter=_ptr(it), flag=_ptr(flag))
    L.check(L.lib().dsq_unmix(C.byref(a), C.byref(o)))
    return {"p": p, "loss": loss, "iter": it, "flag": flag}


def unmix_dev(x, pure, alpha=None, shift=None, power=1, maxit=200, workspace=None):
    """dsq_unmix_dev on resident matrices: x a GeneMajor float64 handle (n x m), pure an (n, k) contiguous float64 device
    tensor.  Returns dict(p: (m, k) float64 tensor, loss: (m,) float64, iter / flag: (m,) int32 tensors); nothing is read
    back.  workspace: a uint8 device tensor of dsq_unmix_workspace_bytes(n, m, k) bytes to reuse."""
    import torch
    assert isinstance(x, GeneMajor) and x.t.dtype == torch.float64
    assert pure.dtype == torch.float64 and pure.dim() == 2 and pure.is_contiguous() and pure.shape[0] == x.n
    dev, m, k = x.t.device, x.m, pure.shape[1]
    p = torch.empty((m, k), dtype=torch.float64, device=dev)
    loss = torch.empty(m, dtype=torch.float64, device=dev)
    ints = torch.empty((2, m), dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(8, int(L.lib().dsq_unmix_workspace_bytes(x.n, m, k))), dtype=torch.uint8, device=dev)
    a = L.DsqUnmixArgs(n=x.n, m=m, k=k, ld=x.ld, x=_t_ptr(x.t), pure=_t_ptr(pure), **_unmix_form(alpha, shift, power, maxit))
    o = L.DsqUnmixOut(p=_t_ptr(p), loss=_t_ptr(loss), iter=_t_ptr(ints[0]), flag=_t_ptr(ints[1]))
    L.check(L.lib().dsq_unmix_dev(C.byref(a), C.byref(o), _t_ptr(workspace), int(workspace.numel()), _stream()))
    # (the workspace is stream-ordered scratch: torch's caching allocator hands it out again only to work enqueued later)
    return {"p": p, "loss": loss, "iter": ints[0], "flag": ints[1]}


def top_var(x, ntop=500):
    """dsq_top_var: host matrix in (n x m, R layout); dict(rowMean n, rowVar n, select: the first min(ntop, n) rows of
    order(rowVar, decreasing = TRUE), 0-based) out"""
    x = _fcol(x)
    if x.ndim != 2:
        raise ValueError("x must be a matrix")
    n, m = x.shape
    k = max(0, min(int(ntop), n))
    mean, var, sel = np.zeros(n), np.zeros(n), np.zeros(max(k, 1), np.int32)
    a = L.sized(L.DsqTopVarArgs, n=n, m=m, ld=0, x=_ptr(x), ntop=int(ntop))
    o = L.sized(L.DsqTopVarOut, rowMean=_ptr(mean), rowVar=_ptr(var), select=_ptr(sel))
    L.check(L.lib().dsq_top_var(C.byref(a), C.byref(o)))
    return {"rowMean": mean, "rowVar": var, "select": sel[:k].astype(np.int64)}


def sample_pairs(x, kind, rows=None, centre=None):
    """dsq_sample_pairs: host matrix in (n x m, R layout), kind "dist2" / "dist" / "gram", rows: 0-based row list or None
    (every row), centre: one value per listed row (gram); the m x m matrix out"""
    x = _fcol(x)
    if x.ndim != 2:
        raise ValueError("x must be a matrix")
    n, m = x.shape
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    centre = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    if centre is not None and centre.size != (n if rows is None else rows.size):
        raise ValueError("centre must have one entry per listed row")
    out = np.zeros((m, m))
    a = L.sized(L.DsqSamplePairsArgs, n=n, m=m, ld=0, x=_ptr(x), kind=L.DSQ_PAIRS[kind], nrows=0 if rows is None else rows.size,
                rows=_ptr(rows), centre=_ptr(centre))
    o = L.sized(L.DsqSamplePairsOut, out=_ptr(out))
    L.check(L.lib().dsq_sample_pairs(C.byref(a), C.byref(o)))
    return out


def top_var_dev(x, ntop=500):
    """dsq_top_var_dev on a resident matrix: x a GeneMajor float64 handle.  Returns dict(rowMean, rowVar: (n,) float64
    tensors (_pack: both as one (2, n) tensor), select: (min(ntop, n),) int32 tensor); nothing is read back."""
    import torch
    assert isinstance(x, GeneMajor) and x.t.dtype == torch.float64
    dev, n = x.t.device, x.n
    k = max(0, min(int(ntop), n))
    pack = torch.empty((2, n), dtype=torch.float64, device=dev)
    sel = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    a = L.sized(L.DsqTopVarArgs, n=n, m=x.m, ld=x.ld, x=_t_ptr(x.t), ntop=int(ntop))
    o = L.sized(L.DsqTopVarOut, rowMean=_t_ptr(pack[0]), rowVar=_t_ptr(pack[1]), select=_t_ptr(sel))
    L.check(L.lib().dsq_top_var_dev(C.byref(a), C.byref(o), _stream()))
    return {"rowMean": pack[0], "rowVar": pack[1], "select": sel[:k], "_pack": pack}


def sample_pairs_dev(x, kind, rows=None, centre=None):
    """dsq_sample_pairs_dev on a resident matrix: x a GeneMajor float64 handle, rows an int32 device tensor or None, centre a
    float64 device tensor with one entry per listed row or None.  Returns the (m, m) float64 tensor; nothing is read back."""
    import torch
    assert isinstance(x, GeneMajor) and x.t.dtype == torch.float64
    if rows is not None:
        assert rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous()
    if centre is not None:
        assert centre.dtype == torch.float64 and centre.is_contiguous() and centre.numel() == (x.n if rows is None else rows.numel())
    out = torch.empty((x.m, x.m), dtype=torch.float64, device=x.t.device)
    a = L.sized(L.DsqSamplePairsArgs, n=x.n, m=x.m, ld=x.ld, x=_t_ptr(x.t), kind=L.DSQ_PAIRS[kind],
                nrows=0 if rows is None else int(rows.numel()), rows=_t_ptr(rows), centre=_t_ptr(centre))
    o = L.sized(L.DsqSamplePairsOut, out=_t_ptr(out))
    L.check(L.lib().dsq_sample_pairs_dev(C.byref(a), C.byref(o), _stream()))
    return out


def _icol(y):
    y = np.asarray(y)
    if y.dtype.kind not in "iu" and y.dtype != np.bool_:
        raise ValueError("counts must be an integer matrix")
    return _need_matrix(np.asfortranarray(y.astype(np.int32, copy=False)))


def _csr(members, offsets):
    return np.ascontiguousarray(members, dtype=np.int32), np.ascontiguousarray(offsets, dtype=np.int32)


def collapse(counts, members, offsets):
    """dsq_collapse: host int matrix in (n x m, R layout) and the groups as a CSR pair (members: the m 0-based sample
    indices group by group, offsets: g + 1); the n x g int32 matrix of group sums out.  A sum that is no int32 raises
    DsqError (DSQ_ERR_VALUE)."""
    y = _icol(counts)
    n, m = y.shape
    members, offsets = _csr(members, offsets)
    g = offsets.size - 1
    if members.size != m:
        raise ValueError("members must list every sample once")
    out = np.zeros((n, max(g, 0)), dtype=np.int32, order="F")
    a = L.sized(L.DsqCollapseArgs, n=n, m=m, g=g, ld=0, y=_ptr(y), members=_ptr(members), offsets=_ptr(offsets))
    o = L.sized(L.DsqCollapseOut, ld=0, out=_ptr(out), status=None)
    L.check(L.lib().dsq_collapse(C.byref(a), C.byref(o)))
    return out


def col_sums(counts):
    """dsq_col_sums: host int matrix in (n x m, R layout); the m column sums out, int64 (exact)"""
    y = _icol(counts)
    n, m = y.shape
    sums = np.zeros(m, dtype=np.int64)
    a = L.sized(L.DsqColSumsArgs, n=n, m=m, ld=0, y=_ptr(y))
    o = L.sized(L.DsqColSumsOut, sums=_ptr(sums))
    L.check(L.lib().dsq_col_sums(C.byref(a), C.byref(o)))
    return sums


def fpm(counts, lib, kind="fpm", basepairs=None, txlen=None):
    """dsq_fpm: host int matrix in (n x m, R layout), lib the m library sizes, kind "fpm" / "fpkm_basepairs" (basepairs: n)
    / "fpkm_txlen" (txlen: n x m); the n x m float64 matrix out"""
    y = _icol(counts)
    n, m = y.shape
    lib = np.ascontiguousarray(lib, dtype=np.float64).reshape(-1)
    if lib.size != m:
        raise ValueError("lib must hold one library size per sample")
    bp = None if basepairs is None else np.ascontiguousarray(basepairs, dtype=np.float64).reshape(-1)
    if bp is not None and bp.size != n:
        raise ValueError("basepairs must hold one length per gene")
    tl = None if txlen is None else _fcol(txlen)
    if tl is not None and tl.shape != (n, m):
        raise ValueError("txlen must have the shape of counts")
    out = np.zeros((n, m), order="F")
    a = L.sized(L.DsqFpmArgs, n=n, m=m, ld=0, y=_ptr(y), kind=L.DSQ_FPM[kind], lib=_ptr(lib), basepairs=_ptr(bp), txlen=_ptr(tl))
    o = L.sized(L.DsqFpmOut, out=_ptr(out))
    L.check(L.lib().dsq_fpm(C.byref(a), C.byref(o)))
    return out


def collapse_dev(y, members, offsets):
    """dsq_collapse_dev on resident counts: y a GeneMajor int32 handle, members / offsets int32 device tensors (m and
    g + 1 entries).  Returns (the n x g GeneMajor int32 handle, padding columns zero; the status word as a (1,) int32
    device tensor: bit 1 a sum that is no int32, bit 2 a member or an offset outside the matrix); nothing is read back."""
    import torch
    assert isinstance(y, GeneMajor) and y.t.dtype == torch.int32
    for v in (members, offsets):
        assert v.dtype == torch.int32 and v.dim() == 1 and v.is_contiguous()
    g = int(offsets.numel()) - 1
    assert int(members.numel()) == y.m
    dev = y.t.device
    out = GeneMajor(torch.zeros((y.n, gene_major_ld(g)), dtype=torch.int32, device=dev), g)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = L.sized(L.DsqCollapseArgs, n=y.n, m=y.m, g=g, ld=y.ld, y=_t_ptr(y.t), members=_t_ptr(members), offsets=_t_ptr(offsets))
    o = L.sized(L.DsqCollapseOut, ld=out.ld, out=_t_ptr(out.t), status=_t_ptr(status))
    L.check(L.lib().dsq_collapse_dev(C.byref(a), C.byref(o), _stream()))
    return out, status


def col_sums_dev(y):
    """dsq_col_sums_dev on resident counts: y a GeneMajor int32 handle.  Returns the (m,) int64 device tensor of column
    sums; nothing is read back."""
    import torch
    assert isinstance(y, GeneMajor) and y.t.dtype == torch.int32
    sums = torch.empty(y.m, dtype=torch.int64, device=y.t.device)
    a = L.sized(L.DsqColSumsArgs, n=y.n, m=y.m, ld=y.ld, y=_t_ptr(y.t))
    o = L.sized(L.DsqColSumsOut, sums=_t_ptr(sums))
    L.check(L.lib().dsq_col_sums_dev(C.byref(a), C.byref(o), _stream()))
    return sums


def fpm_dev(y, lib, kind="fpm", basepairs=None, txlen=None):
    """dsq_fpm_dev on resident counts: y a GeneMajor int32 handle, lib a (m,) float64 device tensor, basepairs a (n,)
    float64 device tensor, txlen a GeneMajor float64 handle with y's ld.  Returns the n x m GeneMajor float64 handle
    (padding columns zero); nothing is read back."""
    import torch
    assert isinstance(y, GeneMajor) and y.t.dtype == torch.int32
    assert lib.dtype == torch.float64 and lib.numel() == y.m and lib.is_contiguous()
    if basepairs is not None:
        assert basepairs.dtype == torch.float64 and basepairs.numel() == y.n and basepairs.is_contiguous()
    if txlen is not None:
        assert isinstance(txlen, GeneMajor) and txlen.t.dtype == torch.float64 and txlen.ld == y.ld and txlen.n == y.n
    out = _f64_like(y)
    a = L.sized(L.DsqFpmArgs, n=y.n, m=y.m, ld=y.ld, y=_t_ptr(y.t), kind=L.DSQ_FPM[kind], lib=_t_ptr(lib),
                basepairs=_t_ptr(basepairs), txlen=None if txlen is None else _t_ptr(txlen.t))
    o = L.sized(L.DsqFpmOut, out=_t_ptr(out.t))
    L.check(L.lib().dsq_fpm_dev(C.byref(a), C.byref(o), _stream()))
    return out


LOCAL_FIT_TOO_FEW = "local dispersion fit: fewer than 3 points in a window"
_LOCAL_FIT_STATUS = ("N", "k", "nSingular", "allBelowFloor")


def local_fit(means=None, disps=None, minDisp=1e-8, eval_means=None, fit=None, evaluate=True):
    """dsq_local_fit (host arrays): the local-regression trend of (means, disps), or -- fit: the block an earlier call
    returned -- of that fit, evaluated at eval_means (None: at means; evaluate = False: the fit alone).  Returns
    dict(dispFit or None, fit: the block, N, k, nSingular, allBelowFloor); raises RuntimeError when a window would hold
    fewer than 3 points."""
    st = np.zeros(4, np.int32)
    ev = None if eval_means is None else np.ascontiguousarray(eval_means, dtype=np.float64).reshape(-1)
    if fit is None:
        means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1)
        disps = np.ascontiguousarray(disps, dtype=np.float64).reshape(-1)
        if means.shape != disps.shape:
            raise ValueError("means and disps must have one entry per gene each")
        n = means.size
        block = np.zeros(int(L.lib().dsq_local_fit_block_doubles(n)) if n else 0)
    else:
        block = np.ascontiguousarray(fit, dtype=np.float64)
        n, means, disps = (block.size - 4) // 3, None, None
    nq = 0 if not evaluate else ev.size if ev is not None else n
    out = np.full(nq, np.nan) if evaluate else None
    a = L.sized(L.DsqLocalFitArgs, n=n, means=_ptr(means), disps=_ptr(disps), minDisp=float(minDisp),
                fit_in=_ptr(block) if fit is not None else None, n_eval=0 if ev is None else ev.size, eval_means=_ptr(ev))
    o = L.sized(L.DsqLocalFitOut, fit=_ptr(block) if fit is None else None, dispFit=_ptr(out), status=_ptr(st))
    try:
        L.check(L.lib().dsq_local_fit(C.byref(a), C.byref(o)))
    except L.DsqError as e:
        if e.code == L.DSQ_ERR_FIT:
            raise RuntimeError(LOCAL_FIT_TOO_FEW) from None
        raise
    return dict(zip(_LOCAL_FIT_STATUS, (int(v) for v in st)), dispFit=out, fit=block)


def local_fit_dev(means=None, disps=None, minDisp=1e-8, eval_means=None, fit=None, evaluate=True, out=None):
    """dsq_local_fit_dev on resident vectors: means / disps / eval_means (n,) float64 device tensors; fit: the block tensor an
    earlier call returned (evaluate only).  out: where dispFit goes (default: a fresh tensor).  Returns dict(dispFit, fit,
    status: (4,) int32 device tensor N, k, nSingular, allBelowFloor); nothing is read back."""
    import torch
    for v in (means, disps, eval_means, fit, out):
        assert v is None or (v.dtype == torch.float64 and v.dim() == 1 and v.is_contiguous())
    src = means if fit is None else fit
    dev = src.device
    if fit is None:
        assert means.numel() == disps.numel()
        n = means.numel()
        block = torch.empty(int(L.lib().dsq_local_fit_block_doubles(n)), dtype=torch.float64, device=dev)
    else:
        block, n = fit, (fit.numel() - 4) // 3
    nq = 0 if not evaluate else eval_means.numel() if eval_means is not None else n
    if evaluate and out is None:
        out = torch.empty(nq, dtype=torch.float64, device=dev)
    assert not evaluate or out.numel() == nq
    status = torch.empty(4, dtype=torch.int32, device=dev)
    a = L.sized(L.DsqLocalFitArgs, n=n, means=_t_ptr(means if fit is None else None), disps=_t_ptr(disps if fit is None else None),
                minDisp=float(minDisp), fit_in=_t_ptr(fit), n_eval=0 if eval_means is None else int(eval_means.numel()),
                eval_means=_t_ptr(eval_means))
    o = L.sized(L.DsqLocalFitOut, fit=_t_ptr(block) if fit is None else None, dispFit=_t_ptr(out) if evaluate else None,
                status=_t_ptr(status))
    L.check(L.lib().dsq_local_fit_dev(C.byref(a), C.byref(o), _stream()))
    return {"dispFit": out if evaluate else None, "fit": block, "status": status}


def sf_iterate_solve(counts, mu, sf, disp, rows, Q=0.05, maxit=100):
    """the solve of one round of estimateSizeFactorsIterate (R/core.R:2600-2611) through dsq_sf_iterate: host arrays in R
    layout in (counts / mu n x m, sf m, disp n, rows n flags); dict(s, sf, F, iter, evals, flag) out."""
    y = np.asfortranarray(counts, dtype=np.int32)
    mu = _fcol(mu)
    if y.ndim != 2 or mu.shape != y.shape:
        raise ValueError("counts and mu must be matrices of the same shape")
    n, m = y.shape
    sf = np.ascontiguousarray(sf, dtype=np.float64)
    disp = np.ascontiguousarray(disp, dtype=np.float64)
    rows = np.ascontiguousarray(np.asarray(rows) != 0, dtype=np.int32)
    if sf.shape != (m,) or disp.shape != (n,) or rows.shape != (n,):
        raise ValueError("sf must have one entry per sample, disp and rows one per gene")
    s, e, F = np.zeros(m), np.zeros(m), np.zeros(1)
    ints = np.zeros(3, np.int32)
    a = L.DsqSfIterateArgs(n=n, m=m, ld=0, y=_ptr(y), mu=_ptr(mu), sf=_ptr(sf), disp=_ptr(disp), rows=_ptr(rows), Q=float(Q),
                           maxit=int(maxit))
    o = L.DsqSfIterateOut(s=_ptr(s), sf=_ptr(e), F=_ptr(F), iter=_ptr(ints[0:1]), evals=_ptr(ints[1:2]), flag=_ptr(ints[2:3]))
    L.check(L.lib().dsq_sf_iterate(C.byref(a), C.byref(o)))
    return {"s": s, "sf": e, "F": float(F[0]), "iter": int(ints[0]), "evals": int(ints[1]), "flag": int(ints[2])}


def sf_iterate_dev(y, mu, sf, disp, rows, Q=0.05, maxit=100, workspace=None):
    """dsq_sf_iterate_dev on resident matrices: y (int32) and mu (float64) GeneMajor handles of one leading dimension, sf (m)
    and disp (n) float64 device tensors, rows (n) an int32 device tensor.  The call synchronises the current stream (the
    host loop reads a record back per evaluation).  Returns dict(s, sf: (m,) float64 tensors, F: (1,), iter / evals / flag:
    (1,) int32 tensors, _pack: all of them as one float64 tensor).  workspace: a uint8 device tensor of
    dsq_sf_iterate_workspace_bytes(n, m) bytes to reuse."""
    import torch
    assert isinstance(y, GeneMajor) and y.t.dtype == torch.int32
    assert isinstance(mu, GeneMajor) and mu.t.dtype == torch.float64 and mu.ld == y.ld and mu.n == y.n and mu.m == y.m
    assert sf.dtype == torch.float64 and sf.numel() == y.m and disp.dtype == torch.float64 and disp.numel() == y.n
    assert rows.dtype == torch.int32 and rows.numel() == y.n
    dev, n, m = y.t.device, y.n, y.m
    pack = torch.empty(2 * m + 1, dtype=torch.float64, device=dev)
    ints = torch.empty(3, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = torch.empty(max(8, int(L.lib().dsq_sf_iterate_workspace_bytes(n, m))), dtype=torch.uint8, device=dev)
    a = L.DsqSfIterateArgs(n=n, m=m, ld=y.ld, y=_t_ptr(y.t), mu=_t_ptr(mu.t), sf=_t_ptr(sf), disp=_t_ptr(disp), rows=_t_ptr(rows),
                           Q=float(Q), maxit=int(maxit))
    o = L.DsqSfIterateOut(s=_t_ptr(pack[:m]), sf=_t_ptr(pack[m:2 * m]), F=_t_ptr(pack[2 * m:]), iter=_t_ptr(ints[0:1]),
                          evals=_t_ptr(ints[1:2]), flag=_t_ptr(ints[2:3]))
    L.check(L.lib().dsq_sf_iterate_dev(C.byref(a), C.byref(o), _t_ptr(workspace), int(workspace.numel()), _stream()))
    return {"s": pack[:m], "sf": pack[m:2 * m], "F": pack[2 * m:], "iter": ints[0:1], "evals": ints[1:2], "flag": ints[2:3],
            "_pack": torch.cat([pack, ints.to(torch.float64)])}


def prefitMoments_dev(y, nf, q, a, r, weights=None, useWeights=False, nf_is_vector=False):
    """device flavour of prefitMoments: y / nf / weights GeneMajor, q / a (p, m) and r (p, p)
    contiguous CUDA tensors (= column-major m x p / p x p)."""
    import torch
    n, m, ld = y.n, y.m, y.ld
    p = q.shape[0]
    dev = y.t.device
    f64 = dict(dtype=torch.float64, device=dev)
    pack = torch.empty((4, n), **f64)
    out = {"baseMean": pack[0], "baseVar": pack[1], "allZero": pack[3].view(torch.int32)[:n], "roughDisp": pack[2],
           "beta_init": torch.empty((p, n), **f64)}
    args = L.DsqPrefitArgs(n=n, m=m, p=p, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                           y_type=L.DSQ_Y_INT32, nf=_t_ptr(nf if nf_is_vector else nf.t),
                           nf_is_vector=int(nf_is_vector), weights=_t_ptr(weights.t) if useWeights else None,
                           useWeights=int(bool(useWeights)), q=_t_ptr(q), a=_t_ptr(a), r=_t_ptr(r))
    o = L.DsqPrefitOut(**{k: _t_ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_prefit_moments_dev(C.byref(args), C.byref(o), _stream()))
    out["_pack"] = pack
    return out


def linearMu_dev(y, nf, q, a, mu_floor=0.0, nf_is_vector=False):
    """y / nf GeneMajor, q / a (p, m) contiguous CUDA tensors; returns GeneMajor mu"""
    import torch
    n, m, ld = y.n, y.m, y.ld
    mu = torch.zeros((n, ld), dtype=torch.float64, device=y.t.device)
    args = L.DsqPrefitArgs(n=n, m=m, p=q.shape[0], layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                           y_type=L.DSQ_Y_INT32, nf=_t_ptr(nf if nf_is_vector else nf.t),
                           nf_is_vector=int(nf_is_vector), weights=None, useWeights=0, q=_t_ptr(q), a=_t_ptr(a), r=None)
    L.check(L.lib().dsq_linear_mu_dev(C.byref(args), float(mu_floor), _t_ptr(mu), _stream()))
    return GeneMajor(mu, m)


def nbinomLogLike_dev(y, mu, disp, weights=None, useWeights=False):
    import torch
    n, m, ld = y.n, y.m, y.ld
    out = torch.empty(n, dtype=torch.float64, device=y.t.device)
    args = L.DsqLogLikeArgs(n=n, m=m, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t), y_type=L.DSQ_Y_INT32,
                            mu=_t_ptr(mu.t), disp=_t_ptr(disp), weights=_t_ptr(weights.t) if useWeights else None,
                            useWeights=int(bool(useWeights)))
    L.check(L.lib().dsq_nbinom_loglike_dev(C.byref(args), _t_ptr(out), _stream()))
    return out


def interceptFit_dev(y, nf, alpha, weights=None, useWeights=False, mu_floor=0.0, want_hat=True, nf_is_vector=False):
    """y / nf / weights GeneMajor, alpha a CUDA vector; mu / hat come back GeneMajor, beta / betaSE in `_pack`"""
    import torch
    n, m, ld = y.n, y.m, y.ld
    dev = y.t.device
    pack = torch.empty((2, n), dtype=torch.float64, device=dev)
    mu = torch.zeros((n, ld), dtype=torch.float64, device=dev)
    hat = torch.zeros((n, ld), dtype=torch.float64, device=dev) if want_hat else None
    args = L.DsqInterceptArgs(n=n, m=m, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t), y_type=L.DSQ_Y_INT32,
                              nf=_t_ptr(nf if nf_is_vector else nf.t), nf_is_vector=int(nf_is_vector),
                              weights=_t_ptr(weights.t) if useWeights else None, useWeights=int(bool(useWeights)),
                              alpha=_t_ptr(alpha), mu_floor=float(mu_floor))
    out = L.DsqInterceptOut(beta_log2=_t_ptr(pack[0]), betaSE=_t_ptr(pack[1]), mu=_t_ptr(mu), hat=_t_ptr(hat))
    L.check(L.lib().dsq_intercept_fit_dev(C.byref(args), C.byref(out), _stream()))
    return {"_pack": pack, "mu": GeneMajor(mu, m), "hat_diagonals": GeneMajor(hat, m) if want_hat else None}


def parametricDispersionFit_dev(means, disps):
    """means / disps: float64 CUDA tensors; returns the two coefficients as a host array"""
    import torch
    out = torch.zeros(3, dtype=torch.float64, device=means.device)      # coefs[2] + status word
    L.check(L.lib().dsq_parametric_dispersion_fit_dev(_t_ptr(means), _t_ptr(disps), means.numel(), _t_ptr(out),
                                                      C.c_void_p(out.data_ptr() + 16), _stream()))
    h = out.cpu()
    st = int(h[2:3].view(torch.int32)[0])
    if st != 0:
        raise RuntimeError(_FIT_ERRORS.get(st, "parametric dispersion fit failed"))
    return h[:2].numpy().copy()


def cooksDistance_dev(y, nf, mu, H, cell_of, p, nf_is_vector=False):
    """y / nf / mu / H GeneMajor; cell_of: host int32 array of design-cell ids.  cooks comes back GeneMajor."""
    import torch
    n, m, ld = y.n, y.m, y.ld
    dev = y.t.device
    cells = np.ascontiguousarray(cell_of, dtype=np.int32)
    ck = torch.zeros((n, ld), dtype=torch.float64, device=dev)
    pack = torch.empty((2, n), dtype=torch.float64, device=dev)
    mx, rd = pack[0], pack[1]
    args = L.DsqCooksArgs(n=n, m=m, p=int(p), layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t),
                          y_type=L.DSQ_Y_INT32, nf=_t_ptr(nf if nf_is_vector else nf.t),
                          nf_is_vector=int(nf_is_vector), mu=_t_ptr(mu.t), H=_t_ptr(H.t), **_cells(cells))
    out = L.DsqCooksOut(cooks=_t_ptr(ck), maxCooks=_t_ptr(mx), robustDisp=_t_ptr(rd))
    L.check(L.lib().dsq_cooks_distance_dev(C.byref(args), C.byref(out), _stream()))
    return {"cooks": GeneMajor(ck, m), "maxCooks": mx, "robustDisp": rd, "_pack": pack}


def replaceOutliers_dev(y, nf, cooks, cooksCutoff, replaceable, trim=0.2, nf_is_vector=False):
    """y / nf / cooks GeneMajor; replaceable: host flags.  The new count matrix comes back GeneMajor int32."""
    import torch
    n, m, ld = y.n, y.m, y.ld
    dev = y.t.device
    rep = np.ascontiguousarray(np.asarray(replaceable).astype(np.int32))
    newc = torch.zeros((n, ld), dtype=torch.int32, device=dev)
    flag = torch.empty(n, dtype=torch.int32, device=dev)
    args = L.DsqReplaceArgs(n=n, m=m, layout=L.DSQ_LAYOUT_GENE_MAJOR, ld=ld, y=_t_ptr(y.t), y_type=L.DSQ_Y_INT32,
                            nf=_t_ptr(nf if nf_is_vector else nf.t), nf_is_vector=int(nf_is_vector),
                            cooks=_t_ptr(cooks.t), cooksCutoff=float(cooksCutoff), trim=float(trim),
                            replaceable=_ptr(rep))
    out = L.DsqReplaceOut(newCounts=_t_ptr(newc), replace=_t_ptr(flag))
    L.check(L.lib().dsq_replace_outliers_dev(C.byref(args), C.byref(out), _stream()))
    return {"counts": GeneMajor(newc, m), "replace": flag}


def _results_scalars(test, lfcThreshold, altHypothesis, theta):
    if test not in L.DSQ_TEST:
        raise ValueError("test should be 'Wald' or 'LRT'")
    if altHypothesis not in L.DSQ_ALT:
        raise ValueError("altHypothesis should be one of %s" % ", ".join(L.DSQ_ALT))
    K = 1 if theta is None else int(len(theta))
    return dict(test=L.DSQ_TEST[test], lfcThreshold=float(lfcThreshold), altHypothesis=L.DSQ_ALT[altHypothesis],
                independentFiltering=int(theta is not None), K=K)


def results(beta, betaSE, stat, pvalue, baseMean, coef, replace=None, na_mask=None, test="Wald", lfcThreshold=0.0,
            altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1, df=None):
    """dsq_results on host arrays: the table of coefficient `coef`, the threshold tests, and the Benjamini-Hochberg
    adjustment over the nested subsets filter >= quantile(filter, theta) (theta None: independentFiltering = FALSE, one
    column).  beta / betaSE: n x p; stat / pvalue: n x p (Wald) or n (LRT); df: n degrees of freedom -- the threshold
    tests then run under Student's t.  Returns the five columns, filtPadj (n x K), numRej, cutoffs."""
    beta, betaSE = _fcol(beta), _fcol(betaSE)
    if beta.ndim == 1:
        beta, betaSE = beta.reshape(-1, 1, order="F"), betaSE.reshape(-1, 1, order="F")
    n, p = beta.shape
    stat, pvalue = _fcol(stat), _fcol(pvalue)
    sc = _results_scalars(test, lfcThreshold, altHypothesis, theta)
    K = sc["K"]
    bm = np.ascontiguousarray(baseMean, dtype=np.float64)
    flags = lambda v: None if v is None else np.ascontiguousarray(np.asarray(v) == 1, dtype=np.int32)
    rep, na = flags(replace), flags(na_mask)
    f = None if filter is None else np.ascontiguousarray(filter, dtype=np.float64)
    th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
    dfa = None if df is None else np.ascontiguousarray(np.broadcast_to(np.asarray(df, np.float64), (n,)))
    cols = {k: np.zeros(n) for k in ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue")}
    fp = np.zeros((n, K), order="F")
    nr, cut, st = np.zeros(K, dtype=np.int32), np.zeros(K), np.zeros(1, dtype=np.int32)
    a = L.DsqResultsArgs(n=n, p=p, c=int(coef), beta=_ptr(beta), betaSE=_ptr(betaSE), stat=_ptr(stat), pvalue=_ptr(pvalue),
                         baseMean=_ptr(bm), replace=_ptr(rep), na_mask=_ptr(na), filter=_ptr(f), theta=_ptr(th),
                         alpha=float(alpha), workspace=None, workspace_bytes=0, df=_ptr(dfa), **sc)
    o = L.DsqResultsOut(filtPadj=_ptr(fp), numRej=_ptr(nr), cutoffs=_ptr(cut), status=_ptr(st),
                        **{k: _ptr(v) for k, v in cols.items()})
    L.check(L.lib().dsq_results(C.byref(a), C.byref(o)))
    cols.update(filtPadj=fp, numRej=nr, cutoffs=cut)
    return cols


def results_dev(beta, betaSE, stat, pvalue, baseMean, coef, replace=None, na_mask=None, test="Wald", lfcThreshold=0.0,
                altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1, df=None):
    """dsq_results_dev on resident columns: beta / betaSE (p, n) tensors (= n x p column-major), stat / pvalue the same or
    n-vectors (LRT), baseMean / filter / df n-vectors (float64), replace / na_mask int32 n-vectors, theta a K-vector -- all
    on the device.  Nothing is read back: the five columns (rows of `table`), filtPadj (K, n): row k is the column of cutoff
    k, and `_small` = cutoffs (K) | numRej (K int32, in ceil(K / 2) doubles) | status, for one copy."""
    import torch
    p, n = (1, beta.numel()) if beta.dim() == 1 else beta.shape
    dev = beta.device
    sc = _results_scalars(test, lfcThreshold, altHypothesis, theta)
    K = sc["K"]
    table = torch.empty((5, n), dtype=torch.float64, device=dev)
    fp = torch.empty((K, n), dtype=torch.float64, device=dev)
    kr = (K + 1) // 2
    small = torch.zeros(K + kr + 1, dtype=torch.float64, device=dev)
    wsb = int(L.lib().dsq_results_workspace_bytes(n, 0))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    a = L.DsqResultsArgs(n=n, p=p, c=int(coef), beta=_t_ptr(beta), betaSE=_t_ptr(betaSE), stat=_t_ptr(stat),
                         pvalue=_t_ptr(pvalue), baseMean=_t_ptr(baseMean), replace=_t_ptr(replace), na_mask=_t_ptr(na_mask),
                         filter=_t_ptr(filter), theta=_t_ptr(theta), alpha=float(alpha), workspace=_t_ptr(ws),
                         workspace_bytes=wsb, df=_t_ptr(df), **sc)
    base = small.data_ptr()
    o = L.DsqResultsOut(baseMean=_t_ptr(table[0]), log2FoldChange=_t_ptr(table[1]), lfcSE=_t_ptr(table[2]),
                        stat=_t_ptr(table[3]), pvalue=_t_ptr(table[4]), filtPadj=_t_ptr(fp), cutoffs=C.c_void_p(base),
                        numRej=C.c_void_p(base + 8 * K), status=C.c_void_p(base + 8 * (K + kr)))
    L.check(L.lib().dsq_results_dev(C.byref(a), C.byref(o), _stream()))
    # (the workspace is stream-ordered scratch: torch's caching allocator hands it out again only to work enqueued later)
    return {"table": table, "filtPadj": fp, "_small": small, "K": K}


def pt(q, df, tail="lower", keep=None, out=None):
    """dsq_pt on host arrays: pt(q[i, k], df[i]) over an n-vector or an n x K matrix q; tail "lower", "upper" or "two_sided"
    (2 * upper(|q|)).  keep: flags shaped as q -- where non-zero the entry of `out` (q when not given) is returned as it is."""
    q = _fcol(q)
    n = q.shape[0] if q.ndim else 1
    K = q.shape[1] if q.ndim == 2 else 1
    dfa = np.ascontiguousarray(np.broadcast_to(np.asarray(df, np.float64), (n,)))
    kp = None if keep is None else np.asfortranarray(np.asarray(keep) != 0, dtype=np.int32)
    res = np.array(q if out is None else _fcol(out), dtype=np.float64, order="F", copy=True)
    L.check(L.lib().dsq_pt(_ptr(q), _ptr(dfa), n, K, L.DSQ_PT[tail], _ptr(kp), _ptr(res)))
    return res


def pt_dev(q, df, tail="lower", keep=None, out=None):
    """dsq_pt_dev on resident tensors: q (n) or (K, n) = n x K column-major, df (n), keep int32 shaped as q or None; out: the
    tensor to write (q itself for in place; a new one when None).  Asynchronous on the current stream."""
    import torch
    n = q.shape[-1]
    K = q.numel() // n if n else 0
    if out is None:
        out = torch.empty_like(q)
    L.check(L.lib().dsq_pt_dev(_t_ptr(q), _t_ptr(df), n, K, L.DSQ_PT[tail], _t_ptr(keep), _t_ptr(out), _stream()))
    return out


def results_small(small, K):
    """(cutoffs, numRej, status) from the host copy of results_dev's `_small`"""
    kr = (K + 1) // 2
    return small[:K].copy(), small[K:K + kr].view(np.int32)[:K].copy(), int(small[K + kr:].view(np.int32)[0])


def _contrast_masks(sample_mask, rule_applies, K, m):
    if sample_mask is None:
        return None, None
    mask = np.ascontiguousarray(np.asarray(sample_mask) != 0, dtype=np.int32).reshape(K, m)
    rule = np.ones(K, dtype=np.int32) if rule_applies is None else np.ascontiguousarray(np.asarray(rule_applies) != 0, dtype=np.int32)
    if rule.shape != (K,):
        raise ValueError("rule_applies must have one flag per contrast")
    return mask, rule


def contrasts(x, nf, alpha_hat, beta, lambda_, contrasts, weights=None, useWeights=False, minmu=0.5, allZero=None,
              counts=None, sample_mask=None, rule_applies=None, K=None, df=None):
    """dsq_contrasts on host arrays: K contrasts from one covariance pass per gene.  x: m x p; nf: n x m (or the m size
    factors); beta: n x p on the natural-log scale; lambda_: p; contrasts: p x K (a column per contrast) or None for the
    all-zero flags alone (then K = the number of masks); counts: the ORIGINAL n x m counts, sample_mask: K x m of 0 / 1,
    rule_applies: K flags; df: n degrees of freedom (pvalue under Student's t).  Returns log2FoldChange, lfcSE, stat, pvalue (n x K) and contrastAllZero (n x K int32)."""
    ct = None if contrasts is None else _fcol(contrasts)
    if ct is not None and ct.ndim == 1:
        ct = ct.reshape(-1, 1, order="F")
    if ct is None:
        if sample_mask is None:
            raise ValueError("neither contrasts nor sample_mask given")
        K = int(np.shape(sample_mask)[0])
        n, m = np.shape(counts)
        p = 1 if x is None else np.shape(x)[1]
    else:
        x = _fcol(x)
        m, p = x.shape
        K = ct.shape[1]
        b = _fcol(beta)
        n = b.shape[0]
        if ct.shape[0] != p or b.shape != (n, p):
            raise ValueError("non-conformable arguments")
    mask, rule = _contrast_masks(sample_mask, rule_applies, K, m)
    y = None if mask is None else np.asfortranarray(np.asarray(counts).astype(np.int32, copy=False))
    if y is not None and y.shape != (n, m):
        raise ValueError("counts must be n x m")
    az = None if allZero is None else np.ascontiguousarray(np.asarray(allZero) == 1, dtype=np.int32)
    out = {k: (np.zeros((n, K), order="F") if ct is not None else None) for k in ("log2FoldChange", "lfcSE", "stat", "pvalue")}
    flags = np.zeros((n, K), dtype=np.int32, order="F")
    a = L.DsqContrastsArgs(n=n, m=m, p=p, K=K, ld=0, minmu=float(minmu), allZero=_ptr(az), counts=_ptr(y),
                           sample_mask=_ptr(mask), rule_applies=_ptr(rule))
    keep = []
    if ct is not None:
        nfa = np.asarray(nf, np.float64)
        is_vec = nfa.ndim == 1
        nfa = np.ascontiguousarray(nfa) if is_vec else _fcol(nfa)
        if nfa.shape != ((m,) if is_vec else (n, m)):
            raise ValueError("nf must be n x m or the m size factors")
        useW = bool(useWeights)
        w = _fcol(weights) if useW else None
        if w is not None and w.shape != (n, m):
            raise ValueError("weights must be n x m")
        alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha_hat, np.float64).reshape(-1), (n,)))
        lam = np.ascontiguousarray(np.asarray(lambda_, np.float64).reshape(-1))
        if lam.size != p:
            raise ValueError("lambda must have length ncol(x)")
        dfa = None if df is None else np.ascontiguousarray(np.broadcast_to(np.asarray(df, np.float64), (n,)))
        keep = [nfa, w, alpha, lam, dfa]
        a.df = _ptr(dfa)
        a.x, a.nf, a.nf_is_vector, a.alpha_hat, a.beta, a.lambda_ = _ptr(x), _ptr(nfa), int(is_vec), _ptr(alpha), _ptr(b), _ptr(lam)
        a.weights, a.useWeights, a.contrasts = _ptr(w), int(useW), _ptr(ct)
    o = L.DsqContrastsOut(contrastAllZero=_ptr(flags), **{k: _ptr(v) for k, v in out.items()})
    L.check(L.lib().dsq_contrasts(C.byref(a), C.byref(o)))
    del keep
    out["contrastAllZero"] = flags
    return out


def contrasts_dev(x, nf, alpha_hat, beta, lambda_, contrasts, weights=None, useWeights=False, minmu=0.5, allZero=None,
                  counts=None, sample_mask=None, rule_applies=None, nf_is_vector=False, cells=None, df=None):
    """dsq_contrasts_dev on resident data: x a (p, m) tensor (= m x p column-major), nf / weights / counts GeneMajor (nf: the
    m size factors with nf_is_vector), alpha_hat (n), beta (p, n) on the natural-log scale, lambda_ (p), contrasts (K, p)
    or None for the flags alone, allZero int32 (n), sample_mask int32 (K, m), rule_applies int32 (K); cells: HOST labels
    (native.cell_index); df float64 (n) or None.  Nothing is read back: `table` (4, K, n) = log2FoldChange | lfcSE | stat | pvalue, each n x K
    column-major, and contrastAllZero (K, n) int32."""
    import torch
    if contrasts is None:
        assert sample_mask is not None and isinstance(counts, GeneMajor)
        K, m = sample_mask.shape
        n, ld, p, dev = counts.n, counts.ld, 1, counts.t.device
    else:
        K, p = contrasts.shape
        n, m, dev = beta.shape[1], x.shape[1], beta.device
        ld = None
        for h in (counts if sample_mask is not None else None, None if nf_is_vector else nf, weights if useWeights else None):
            if h is not None:
                assert isinstance(h, GeneMajor) and h.n == n and h.m == m and (ld is None or h.ld == ld)
                ld = h.ld
        ld = m if ld is None else ld
    table = torch.empty((4, K, n), dtype=torch.float64, device=dev) if contrasts is not None else None
    flags = torch.empty((K, n), dtype=torch.int32, device=dev)
    a = L.DsqContrastsArgs(n=n, m=m, p=p, K=K, ld=ld, minmu=float(minmu), allZero=_t_ptr(allZero),
                           counts=_t_ptr(counts.t) if sample_mask is not None else None, sample_mask=_t_ptr(sample_mask),
                           rule_applies=_t_ptr(rule_applies))
    if contrasts is not None:
        a.x, a.nf, a.nf_is_vector = _t_ptr(x), _t_ptr(nf if nf_is_vector else nf.t), int(bool(nf_is_vector))
        a.alpha_hat, a.beta, a.lambda_, a.contrasts = _t_ptr(alpha_hat), _t_ptr(beta), _t_ptr(lambda_), _t_ptr(contrasts)
        a.weights, a.useWeights = (_t_ptr(weights.t) if useWeights else None), int(bool(useWeights))
        a.df = _t_ptr(df)
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=np.int32)
            a.cell_of, a.ncell = _ptr(cells), int(cells.max()) + 1
    o = L.DsqContrastsOut(contrastAllZero=_t_ptr(flags))
    if table is not None:
        o.log2FoldChange, o.lfcSE, o.stat, o.pvalue = (_t_ptr(table[i]) for i in range(4))
    L.check(L.lib().dsq_contrasts_dev(C.byref(a), C.byref(o), _stream()))
    return {"table": table, "contrastAllZero": flags}
