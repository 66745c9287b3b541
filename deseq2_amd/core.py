"""Host-side mirror of the reference's callers of the native boundary (R/core.R,
R/fitNbinomGLMs.R, R/wrappers.R): same function names, same argument meaning and defaults,
same decision rules, operating on a minimal DESeqDataSet stand-in.  The three native
routines go to the MI355X engine (engine.py); the all-gene "global" steps between them
(dispersion trend, prior variance) stay on the host exactly as in DESeqParallel
(R/parallel.R:27-28) -- they exchange only n-vectors.

Cook's distances, outlier replacement and the refit loop are mirrored too; their
O(n m) parts run in the engine.

Size factors: estimateSizeFactors / estimateSizeFactorsForMatrix ("ratio", "poscounts", geoMeans, controlGenes,
normMatrix) run in the engine too (csrc/size_factors.hip); type = "iterate" (estimateSizeFactorsIterate) alternates the
dispersion steps with the engine's solve of the log size factors (csrc/sf_iterate.hip).

Transformations: vst / varianceStabilizingTransformation / getVarianceStabilizedData (R/vst.R), normTransform and
counts(normalized = TRUE) run in the engine as well (csrc/vst.hip); rlog / rlogTransformation
run there too, for any number of samples (csrc/rlog.hip).

results() / resultsContrasts() (R/results.R) and lfcShrink(type = "normal") (R/lfcShrink.R: the Normal prior; the prior
variance of all columns on the device, csrc/beta_prior.hip) are mirrored at the end of this file.

collapseReplicates, fpm / fpkm (R/helper.R), counts() (R/methods.R) and plotCounts(returnData = TRUE) (R/plots.R) close the
file; their O(n m) parts run in the engine (csrc/count_helpers.hip).

lfcShrinkApeglm / apeglm / svalue serve lfcShrink(type = "apeglm") (R/lfcShrink.R:328-440): the estimator as documented, by
the library's own iteration (csrc/apeglm.hip).

lfcShrinkAshr / ash serve lfcShrink(type = "ashr") (R/lfcShrink.R:442-486), for a coefficient, a contrast or a list of
contrasts: the estimator as its paper and the call state it, by the library's own iteration (csrc/ash.hip, DESIGN.md section
23).  The ashr package's numbers, its optimiser and its treatment of excluded rows are unpinned.

Not mirrored (out of the hot-path scope): the glmGamPoi dispersion fit.
"""
import warnings

import numpy as np
from scipy import special as sps

from .engine import HostEngine, ResultColumns, control_flags

LOG2E = np.log2(np.e)

# facts about a model matrix (rank, design cells) are asked for several times per DESeq(); they depend
# on the m x p matrix only, so they are memoised on its bytes
_DESIGN_CACHE = {}


def _design_fact(kind, x, fn):
    x = np.ascontiguousarray(x, dtype=np.float64)
    key = (kind, x.shape, x.tobytes())
    v = _DESIGN_CACHE.get(key)
    if v is None:
        if len(_DESIGN_CACHE) > 256:
            _DESIGN_CACHE.clear()
        v = _DESIGN_CACHE[key] = fn(x)
    return v


def _rank(x):
    return _design_fact("rank", x, lambda a: int(np.linalg.matrix_rank(a)))


def _cells(x):
    """(cell id per sample, size of that sample's cell): samples with identical model-matrix rows"""
    def f(a):
        _, inv, cnt = np.unique(a, axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        return inv, cnt[inv]
    return _design_fact("cells", x, f)


class DESeqDataSet:
    """counts (n x m int), model matrix x (m x p), size factors (m) or normalization
    factors (n x m), optional observation weights (n x m).  `mcols` holds per-gene vectors
    (R: mcols(object)), `assays` the n x m engine handles (mu, H)."""

    def __init__(self, counts, x, sizeFactors=None, normalizationFactors=None, weights=None, engine=None):
        counts = np.asarray(counts)
        if counts.ndim != 2 or (counts < 0).any():
            raise ValueError("counts must be a non-negative integer matrix")          # R/AllClasses.R:9-20
        self.n, self.m = counts.shape
        self.x = np.asarray(x, dtype=np.float64)
        if self.x.shape[0] != self.m:
            raise ValueError("model matrix rows must match samples")
        self.engine = engine if engine is not None else HostEngine()
        if normalizationFactors is not None:
            nf = np.asarray(normalizationFactors, np.float64)
            self.sizeFactors = None
        else:
            sf = np.ones(self.m) if sizeFactors is None else np.asarray(sizeFactors, np.float64)
            nf = np.broadcast_to(sf[None, :], counts.shape)                          # getSizeOrNormFactors :2221
            self.sizeFactors = sf
        self.counts_host = counts.astype(np.int32)
        self._sf_given = sizeFactors is not None or normalizationFactors is not None
        E = self.engine
        self.y = E.counts(self.counts_host)
        self.nf = E.matrix(nf)
        self.has_weights = weights is not None
        # assays(object)[["weights"]] as given (an engine handle); normalised by getAndCheckWeights
        self.weights_h = None if weights is None else E.matrix(np.asarray(weights, np.float64))
        self.xh = E.design(self.x)
        self.mcols = {}
        self.assays = {}
        self.attrs = {}
        self.dispersionFunction = None

    @classmethod
    def from_device(cls, engine, counts_r, nf_r, x, weights=None, sizeFactors=None, weights_r=None):
        """Build from matrices ALREADY RESIDENT in HBM in R layout: `counts_r` (int32), `nf_r` and the optional
        `weights_r` (float64) are contiguous (m, n) torch tensors, i.e. column-major n x m exactly as
        R holds them.  Converts to the engine's gene-major layout on the device (no host copy).  (`weights`, a
        host array, is uploaded when no `weights_r` is given.)  `sizeFactors`: pass them only when `nf_r` is the matrix
        R builds FROM them (`getSizeOrNormFactors`, R/core.R:2221-2227: no normalizationFactors) -- the chain may
        then read the m-vector instead of the matrix."""
        self = cls.__new__(cls)
        self.m, self.n = counts_r.shape
        self.x = np.asarray(x, dtype=np.float64)
        self.engine = engine
        self.counts_host = None
        self.sizeFactors = None if sizeFactors is None else np.asarray(sizeFactors, np.float64)
        self.y = engine.native.to_gene_major(counts_r)
        # with size factors the chain can run on the m-vector (nf[i, j] = s_j for every gene): the n x m matrix R
        # passes is then converted only if some step asks for it
        if self.sizeFactors is not None:
            self._nf, self._nf_src = None, nf_r
        else:
            self.nf = engine.native.to_gene_major(nf_r)
        self.has_weights = weights is not None or weights_r is not None
        if weights_r is not None:
            self.weights_h = engine.native.to_gene_major(weights_r)
        else:
            self.weights_h = None if weights is None else engine.matrix(np.asarray(weights, np.float64))
        self.xh = engine.design(self.x)
        self.mcols, self.assays, self.attrs = {}, {}, {}
        self.dispersionFunction = None
        return self

    def subset(self, idx, counts_handle=None):
        """object[idx, ] (optionally over another count matrix handle with the same rows as self)"""
        E = self.engine
        sub = DESeqDataSet.__new__(DESeqDataSet)
        idx = np.asarray(idx)
        sub.n, sub.m, sub.x, sub.engine = int(idx.size), self.m, self.x, E
        sub.sizeFactors = self.sizeFactors
        sub.counts_host = None
        sub.y = E.take_rows(self.y if counts_handle is None else counts_handle, idx)
        sub.nf = E.take_rows(self.nf, idx)
        sub.has_weights = self.has_weights
        sub.weights_h = E.take_rows(self.weights_h, idx)
        sub.xh = self.xh
        sub.mcols, sub.assays, sub.attrs = {}, {}, {}
        if "weightsOK" in self.attrs:          # attr(object, "weightsOK"): the rank checks ran on the parent
            sub.attrs["weightsOK"] = True
        sub.dispersionFunction = None if self.dispersionFunction is None else dict(self.dispersionFunction)
        return sub

    @property
    def p(self):
        return self.x.shape[1]

    # False: the object was built without size or normalization factors and none were estimated since (is.null(sizeFactors)
    # & is.null(normalizationFactors), R/vst.R:122,236); the factors of one it carries are a placeholder
    _sf_given = True
    # normalization factors in the engine's gene-major layout; from_device() defers the conversion (see there)
    _nf = None
    _nf_src = None

    @property
    def nf(self):
        if self._nf is None and self._nf_src is not None:
            src = self._nf_src() if callable(self._nf_src) else self._nf_src      # (estimateSizeFactors defers the n x m matrix too)
            self._nf, self._nf_src = self.engine.native.to_gene_major(src), None
        return self._nf

    @nf.setter
    def nf(self, v):
        self._nf, self._nf_src = v, None


# ------------------------------------------------------------------ R/wrappers.R
def _na_guard(fname, **args):
    """R/wrappers.R:31-34,110-113: error naming the arguments that contain NA"""
    bad = [k for k, v in args.items() if v is not None and isinstance(v, np.ndarray) and np.isnan(v).any()]
    if bad:
        raise ValueError("in call to %s, the following arguments contain NA: %s" % (fname, ", ".join(bad)))


def fitDispGridWrapper(E, y, x, mu, logAlphaPriorMean, logAlphaPriorSigmaSq, usePrior, weights, useWeights,
                       weightThreshold, useCR, ncol_y):
    """R/wrappers.R:63-82"""
    _na_guard("fitDispGridWrapper", logAlphaPriorMean=np.asarray(logAlphaPriorMean, float))
    minLogAlpha = np.log(1e-8)
    maxLogAlpha = np.log(max(10, ncol_y))
    dispGrid = np.linspace(minLogAlpha, maxLogAlpha, 20)
    la = E.fit_disp_grid(y, x, mu, dispGrid, logAlphaPriorMean, logAlphaPriorSigmaSq, usePrior, weights,
                         useWeights, weightThreshold, useCR)["log_alpha"]
    return E.vexp(la)


# ------------------------------------------------------------------ weights
def getAndCheckWeights(dds, weightThreshold=1e-2, modelMatrix=None):
    """R/core.R:2697-2751: row-max normalisation; once per analysis the per-gene rank checks, whose failures are
    flagged in mcols weightsFail and treated as all-zero rows (:2736-2747).  Returns (engine handle of the
    normalised weights, useWeights); the handle is cached on the object."""
    E = dds.engine
    if not dds.has_weights:
        return None, False
    w = dds.attrs.get("weights_norm")
    if w is None or dds.attrs.get("weights_norm_of") is not dds.weights_h:
        if E.any_negative(dds.weights_h):
            raise ValueError("all(weights >= 0) is not TRUE")
        w = E.row_max_normalize(dds.weights_h)                                        # :2702
        dds.attrs["weights_norm"], dds.attrs["weights_norm_of"] = w, dds.weights_h
        dds.attrs.pop("weights_floor", None)
    if "weightsOK" not in dds.attrs:
        x = dds.x if modelMatrix is None else np.asarray(modelMatrix, np.float64)
        ok = E.weights_ok(w, x, weightThreshold, _rank(x) == x.shape[1])              # :2706-2734
        if not ok.all():
            dds.mcols["weightsFail"] = ~ok
            if "allZero" in dds.mcols:
                dds.mcols["allZero"] = dds.mcols["allZero"] | ~ok                     # :2737
        dds.attrs["weightsOK"] = True
    return w, True


def _floored_weights(dds, w):
    """weights <- pmax(weights, 1e-6)   (R/core.R:702), cached next to the normalised handle"""
    f = dds.attrs.get("weights_floor")
    if f is None:
        f = dds.attrs["weights_floor"] = dds.engine.clamp_min(w, 1e-6)
    return f


def getBaseMeansAndVariances(dds):
    """R/core.R:2138-2157"""
    E = dds.engine
    # one pass also yields the rough dispersion and the IRLS start values used right after
    # (roughDispEstimate :2422, fitNbinomGLMs.R:139-145); they are cached on the object
    if dds.attrs.get("prefit_for") is dds.y and "prefit" in dds.attrs:   # same count handle: nothing changed
        pf = dds.attrs["prefit"]
    else:
        w = dds.weights_h if dds.has_weights else None
        pf = E.prefit(dds.y, dds.nf, dds.x, w)
        dds.attrs["prefit"], dds.attrs["prefit_for"] = pf, dds.y
    dds.mcols["baseMean"], dds.mcols["baseVar"], dds.mcols["allZero"] = pf["baseMean"], pf["baseVar"], pf["allZero"]
    return dds


def xim_size_factors(sf):
    """momentsDispEstimate's xim = mean(1 / sizeFactors) (R/core.R:2440-2444), summed in sample order (R's mean() is a
    sequential sum too): ONE definition for the call-by-call chain, the fused chain and the library's own host entry
    (csrc/deseq_host.hip), so that all three start the dispersion search from the same bits"""
    sf = np.asarray(sf, np.float64)
    return float(np.cumsum(1.0 / sf)[-1] / sf.size)


# ------------------------------------------------------------------ size factors
def _sf_args(n, type, geoMeans, controlGenes):
    if type == "iterate":
        raise NotImplementedError('type = "iterate" belongs to estimateSizeFactors on an object (R/methods.R:374-375, VERDICT '
                                  "row f4): R's estimateSizeFactorsForMatrix has no such type")
    if type not in ("ratio", "poscounts"):
        raise ValueError("'arg' should be one of 'ratio', 'poscounts', 'iterate'")
    if type == "poscounts":
        geoMeans = None                                    # R/methods.R:381 overwrites the argument
    if geoMeans is not None:
        geoMeans = np.asarray(geoMeans, np.float64).reshape(-1)
        if geoMeans.size != n:
            raise ValueError("geoMeans should be as long as the number of rows of counts")     # R/core.R:552-554
    return geoMeans, control_flags(controlGenes, n)                                            # :565-567


def estimateSizeFactorsForMatrix(E, y, type="ratio", geoMeans=None, controlGenes=None):
    """R/core.R:535-578 on an engine count handle: the m size factors (host).  locfunc is stats::median;
    type = "poscounts" is what estimateSizeFactors.DESeqDataSet makes of it (R/methods.R:377-382: its own geoMeans,
    hence the final division by the geometric mean of the factors); controlGenes: 0-based indices or a logical vector."""
    geoMeans, ctl = _sf_args(E.nrow(y), type, geoMeans, controlGenes)
    return E.size_factors(y, type=type, geoMeans=geoMeans, control=ctl)["sizeFactors"]


def estimateSizeFactors(dds, type="ratio", geoMeans=None, controlGenes=None, normMatrix=None):
    """estimateSizeFactors.DESeqDataSet (R/methods.R:363-406).  Sets dds.sizeFactors and the normalization-factor handle
    R builds from them (getSizeOrNormFactors, R/core.R:2221-2227) -- or, with normMatrix (n x m host array, or an engine
    handle), the matrix of estimateNormFactors (R/core.R:2159-2163) with dds.sizeFactors = None.  Works on the resident
    counts: an object made by from_device() needs no host copy of them."""
    E = dds.engine
    if type == "iterate":                                  # R/methods.R:374-375: geoMeans, controlGenes, normMatrix are not looked at
        info = {}
        sf = estimateSizeFactorsIterate(dds, info=info)
        _install_size_factors(dds, sf)
        dds.attrs["sfIterateRounds"] = info["rounds"]
        return dds
    geoMeans, ctl = _sf_args(dds.n, type, geoMeans, controlGenes)
    nmh = normMatrix
    if normMatrix is not None and isinstance(normMatrix, (np.ndarray, list, tuple)):
        nm = np.asarray(normMatrix, np.float64)
        if nm.shape != (dds.n, dds.m):
            raise ValueError("normMatrix must have the dimensions of the counts")
        nmh = E.matrix(nm)
    r = E.size_factors(dds.y, type=type, geoMeans=geoMeans, control=ctl, normMatrix=nmh)
    if normMatrix is not None:
        for k in ("prefit", "prefit_for"):                 # baseMean / baseVar belong to the old factors
            dds.attrs.pop(k, None)
        dds._sf_given = True
        dds.sizeFactors = None
        dds.nf = r["normalizationFactors"] if E.name == "device" else E.matrix(r["normalizationFactors"])
        return dds
    return _install_size_factors(dds, r["sizeFactors"], r.get("sizeFactors_dev"))


def _install_size_factors(dds, sf, sfd=None):
    """sizeFactors(dds) <- sf: the m-vector, the normalization-factor handle R builds from it (getSizeOrNormFactors,
    R/core.R:2221-2227) and the dropped prefit cache.  sfd: the resident copy of sf on a device engine, if there is one."""
    E = dds.engine
    for k in ("prefit", "prefit_for"):                     # baseMean / baseVar belong to the old factors
        dds.attrs.pop(k, None)
    dds._sf_given = True
    sf = dds.sizeFactors = np.asarray(sf, np.float64)
    if E.name == "device":
        # the chain reads the resident m-vector (fused._Run looks it up by its bytes); the n x m matrix is built from it
        # on the device, and only if a step asks for it
        if sfd is None:
            sfd = E._vec(sf)
        E._cache[("sf", np.ascontiguousarray(sf).tobytes())] = sfd
        n = dds.n
        dds._nf, dds._nf_src = None, (lambda: sfd[:, None].expand(sfd.numel(), n).contiguous())
    else:
        dds.nf = E.matrix(np.broadcast_to(sf[None, :], (dds.n, dds.m)))
    return dds


SF_ITERATE_WITHIN = "iterative size factor normalization did not converge within an iteration"     # R/core.R:2609
SF_ITERATE_OUTER = "iterative size factor normalization did not converge"                          # R/core.R:2617


def estimateSizeFactorsIterate(dds, niter=10, Q=0.05, info=None):
    """R/core.R:2589-2622 on either engine: the m size factors (host).  Each round fits the dispersions of the intercept
    design at the current factors (estimateDispersions(fitType = "mean")) and maximises, over the log size factors, the sum
    of the gene log likelihoods above their Q quantile at q = t(t(mu) / sf) and those dispersions.  R hands that objective
    to optim(L-BFGS-B); here it is the engine's sf_iterate_solve (csrc/sf_iterate.hip on the device): the same objective,
    the library's own deterministic safeguarded Newton iteration.  R's two stop() messages come as
    ValueError.  info: a dict that receives the number of rounds."""
    E = dds.engine
    m = dds.m
    if m - 1 <= 3:
        raise NotImplementedError("estimateSizeFactors(type = \"iterate\") fits the dispersions of the intercept design: with "
                                  "%d samples its residual df is <= 3, where the reference's seeded Monte-Carlo prior "
                                  "variance is not mirrored (VERDICT row f4)" % m)
    work = _shallow(dds, np.ones((m, 1)))                                            # design(object) <- ~ 1, :2590
    sf = np.ones(m)                                                                  # :2591
    _install_size_factors(work, sf)
    allZero = getBaseMeansAndVariances(work).mcols["allZero"]                        # idx <- rowSums(counts(object)) > 0, :2592
    if allZero.any():
        work = work.subset(np.where(~allZero)[0])                                    # (the engine fits the non-zero rows)
    rows = np.ones(work.n, dtype=bool)
    for i in range(1, int(niter) + 1):                                               # :2594
        _install_size_factors(work, sf)                                              # :2595
        work.mcols, work.assays = {}, {}
        estimateDispersions(work, fitType="mean")                                    # :2596
        r = E.sf_iterate_solve(work.y, work.assays["mu"], sf, work.mcols["dispersion"], rows, Q=Q, maxit=100)   # :2597-2607
        if r["flag"] != 0:
            raise ValueError(SF_ITERATE_WITHIN)                                      # :2608-2610
        sf_old, sf = sf, np.asarray(r["sf"], np.float64)                             # :2599, :2611
        dl = E.vlog(sf_old) - E.vlog(sf)
        if i > 1 and np.cumsum(dl * dl)[-1] < 1e-4:                                  # :2613
            break
        if i == niter:
            raise ValueError(SF_ITERATE_OUTER)                                       # :2616-2618
    if info is not None:
        info["rounds"] = i
    return sf


def modelMatrixGroups(x):
    """R/core.R:2450-2452"""
    return _cells(x)[0]


# ------------------------------------------------------------------ R/fitNbinomGLMs.R
def fitNbinomGLMsOptim(E, y, nf, x, lam, rowsForOptim, rowStable, alpha_hat, weights, useWeights, betaMatrix,
                       betaSE, betaConv, beta_mat_init, logLike, minmu=0.5):
    """R/fitNbinomGLMs.R:340-407: the rows the IRLS did not fit are re-fitted by maximising the penalised NB log
    posterior over beta in [-30, 30]^p.  The reference loops over them in R with optim(method = "L-BFGS-B"); the
    engine fits them in one launch (damped Fisher scoring on the same objective and box, E.optim_rows), everything
    after the optimum -- mu, betaSE, logLike -- as :382-400."""
    rows = np.asarray(rowsForOptim)
    large = 30.0
    start = np.empty((rows.size, x.shape[1]))
    for r, row in enumerate(rows):
        if rowStable[row] and (np.abs(betaMatrix[row]) < large).all():
            start[r] = betaMatrix[row]                                             # :351-352
        else:
            start[r] = np.asarray(beta_mat_init[row], float)                       # :354 (the natural-log start, as in R)
    o = E.optim_rows(E.take_rows(y, rows), E.take_rows(nf, rows), x, np.asarray(alpha_hat)[rows], lam,
                     E.take_rows(weights, rows) if useWeights else None, useWeights, start, minmu)
    betaConv[rows[np.asarray(o["conv"], bool)]] = True                             # :378-380
    betaMatrix[rows] = o["beta"]                                                   # :382
    betaSE[rows] = o["betaSE"]                                                     # :397
    logLike[rows] = o["logLike"]                                                   # :398-399
    return betaMatrix, betaSE, betaConv, rows, np.asarray(o["mu"]), logLike


def _host_vector(v):
    """an engine may hand back an n-vector that is still on the device (engine.LaunchedVector)"""
    return v.host() if hasattr(v, "host") else v


class PendingFit:
    """fitNbinomGLMs(defer = TRUE): the fit has been launched; `mu` (and `hat_diagonals`) are engine handles
    usable at once, finish() runs the host half of R/fitNbinomGLMs.R:184-235 (row checks, optim fallback)."""

    def __init__(self, mu, hat_diagonals, finish):
        self.mu, self.hat_diagonals, self.finish = mu, hat_diagonals, finish


def fitNbinomGLMs(dds, rows=None, modelMatrix=None, alpha_hat=None, lam=None, betaTol=1e-8, maxit=100,
                  useOptim=True, useQR=True, minmu=0.5, weights=None, useWeights=False, mu_floor=0.0,
                  want_hat=True, forceOptim=False, want_loglike=False, defer=False):
    """R/fitNbinomGLMs.R:29-236.  Rows the IRLS does not fit (`rowsForOptim`, :203-211) go through the
    reference's L-BFGS-B fallback on the host (fitNbinomGLMsOptim, :213-227), as in R.  logLike
    (:182) is computed only when the caller reads it (want_loglike)."""
    E = dds.engine
    x = dds.x if modelMatrix is None else np.asarray(modelMatrix, np.float64)
    xh = dds.xh if modelMatrix is None else E.design(x)
    y, nf = dds.y, dds.nf
    if rows is not None:
        y, nf = E.take_rows(y, rows), E.take_rows(nf, rows)
        weights = E.take_rows(weights, rows) if weights is not None else None
    n = E.nrow(y)
    p = x.shape[1]
    if alpha_hat is None:
        alpha_hat = dds.mcols["dispersion"] if rows is None else dds.mcols["dispersion"][rows]
    alpha_hat = np.asarray(alpha_hat, np.float64)
    if alpha_hat.shape[0] != n:
        raise ValueError("alpha_hat needs to be the same length as nrows(object)")
    if lam is None:
        lam = np.full(p, 1e-6)                                                     # :73
    lam = np.asarray(lam, np.float64)
    if not (np.abs(x).sum(axis=0) > 0).all():
        raise ValueError("all(colSums(abs(modelMatrix)) > 0) is not TRUE")          # :45
    # intercept-only model with the wide prior: closed form, no native call (:99-137)
    if p == 1 and (x == 1).all() and (lam <= 1e-6).all():
        # one engine pass (the reference does this in vectorised R): beta = log2 of the [weighted] mean normalized
        # count, mu = nf 2^beta, betaSE / hat from w = [weights] / (1/mu + alpha).  The mu handed back is floored at
        # mu_floor (the gene-wise dispersion fit reads fitMu[fitMu < minmu] <- minmu, R/core.R:763); betaSE, hat and
        # logLike are of the unfloored fit, as in R.
        r = E.intercept_fit(y, nf, alpha_hat, weights, useWeights, mu_floor=0.0, want_hat=want_hat)
        mu_h = r["mu"]
        res = {"betaConv": np.ones(n, bool), "betaMatrix": r["beta"][:, None], "betaSE": r["betaSE"][:, None],
                "mu": E.clamp_min(mu_h, mu_floor) if mu_floor > 0 else mu_h, "betaIter": np.ones(n), "modelMatrix": x,
                "nterms": 1, "hat_diagonals": r["hat_diagonals"], "deviance_native": None,
                "rowsForOptim": np.array([], int), "beta_natlog": r["beta"][:, None] / LOG2E, "optimRows": None,
                "logLike": (_host_vector(E.nbinom_loglike(y, mu_h, alpha_hat, weights, useWeights))
                            if want_loglike else None)}
        return PendingFit(res["mu"], res["hat_diagonals"], lambda: res) if defer else res
    # initial betas by QR least squares when full rank (:139-155)
    if _rank(x) == p:
        if rows is None and modelMatrix is None and "prefit" in dds.attrs:
            beta_mat = dds.attrs["prefit"]["beta_init"]
        else:
            beta_mat = E.prefit(y, nf, x)["beta_init"]
    else:
        beta0 = np.zeros((n, p))
        bm = E.prefit(y, nf, np.ones((x.shape[0], 1)))["baseMean"]
        if (x[:, 0] == 1).all():
            beta0[:, 0] = E.vlog(bm)
        else:
            beta0[:] = 1.0
        beta_mat = beta0
    lambdaNatLogScale = lam / np.log(2) ** 2                                       # :162
    contrast = np.r_[1.0, np.zeros(p - 1)]                                         # R/wrappers.R:105-108
    _na_guard("fitBeta", alpha_hatSEXP=alpha_hat, lambdaSEXP=lambdaNatLogScale)
    betaRes = E.fit_beta(y, xh, nf, alpha_hat, contrast, beta_mat, lambdaNatLogScale, weights, useWeights,
                         betaTol, maxit, useQR, minmu, want_mu=True, mu_floor=mu_floor, want_hat=want_hat)
    mu0 = betaRes["mu"]                                                            # :180
    # launched before the host reads anything back, so the row checks below overlap it (:182)
    logLike0 = E.nbinom_loglike(y, mu0, alpha_hat, weights, useWeights) if want_loglike else None

    def finish():
        mu = mu0
        rowStable = ~np.isnan(betaRes["beta_mat"]).any(axis=1)                     # :185
        rowVarPositive = ~(betaRes["beta_var_mat"] <= 0).any(axis=1)               # :188
        betaConv = betaRes["iter"] < maxit                                         # :191
        betaMatrix = LOG2E * betaRes["beta_mat"]                                   # :194
        betaSE = LOG2E * np.sqrt(np.maximum(betaRes["beta_var_mat"], 0))           # :198
        if useOptim:
            rowsForOptim = np.where(~betaConv | ~rowStable | ~rowVarPositive)[0]   # :203-207
        else:
            rowsForOptim = np.where(~rowStable | ~rowVarPositive)[0]
        if forceOptim:
            rowsForOptim = np.arange(n)                                            # :209-211
        logLike = _host_vector(logLike0)
        optimRows = None
        if len(rowsForOptim) > 0:                                                  # :213-227
            ll = np.full(n, np.nan)
            b0 = E.to_numpy_np(beta_mat) if hasattr(E, "to_numpy_np") else beta_mat
            betaMatrix, betaSE, betaConv, optimRows, optimMu, ll = fitNbinomGLMsOptim(
                E, y, nf, x, lam, rowsForOptim, rowStable, alpha_hat, weights, useWeights, betaMatrix.copy(),
                betaSE.copy(), betaConv.copy(), b0, ll, minmu=minmu)
            mu = E.put_rows(mu, optimRows, np.maximum(optimMu, mu_floor))          # mu[row,] <- mu_row  (:386)
            if logLike is not None:
                logLike = np.array(logLike, copy=True)
                logLike[optimRows] = ll[optimRows]                                 # :399
        return {"betaConv": betaConv, "betaMatrix": betaMatrix, "betaSE": betaSE, "mu": mu, "logLike": logLike,
                "optimRows": optimRows,
                "betaIter": betaRes["iter"], "modelMatrix": x, "nterms": p,
                "hat_diagonals": betaRes.get("hat_diagonals"), "deviance_native": betaRes["deviance"],
                "rowsForOptim": rowsForOptim, "beta_natlog": betaRes["beta_mat"]}
    return PendingFit(mu0, betaRes.get("hat_diagonals") if want_hat else None, finish) if defer else finish()


# ------------------------------------------------------------------ dispersions
def estimateDispersionsGeneEst(dds, minDisp=1e-8, kappa_0=1.0, dispTol=1e-6, maxit=100, useCR=True,
                               weightThreshold=1e-2, modelMatrix=None, niter=1, linearMu=None, minmu=0.5,
                               alphaInit=None):
    """R/core.R:657-860"""
    if np.log(minDisp / 10) <= -30:
        raise ValueError("for computational stability, log(minDisp/10) should be above -30")
    E = dds.engine
    x = dds.x if modelMatrix is None else np.asarray(modelMatrix, np.float64)
    if _rank(x) < x.shape[1]:
        raise ValueError("the model matrix is not full rank")                       # checkFullRank :2624
    if x.shape[0] == x.shape[1]:
        raise ValueError("the number of samples and the number of model coefficients are equal")
    if modelMatrix is not None:
        dds.attrs["geneEstModelMatrix"] = x           # attr(object, "dispModelMatrix"): estimateDispersionsMAP's default (R/core.R:850, 1003)
    if not (int(niter) == niter and niter > 0):
        raise ValueError("length(niter) == 1 & niter > 0 is not TRUE")              # :730
    getBaseMeansAndVariances(dds)
    w_norm, useWeights = getAndCheckWeights(dds, weightThreshold, modelMatrix=modelMatrix)   # :698
    weights_glm = w_norm                                            # fitNbinomGLMs re-reads them unfloored (:77)
    weights = _floored_weights(dds, w_norm) if useWeights else None                 # :702
    nz = ~dds.mcols["allZero"]
    if not nz.all():
        raise ValueError("all-zero rows must be removed before fitting (the engine fits objectNZ)")
    m, n = dds.m, dds.n
    xh = dds.xh if modelMatrix is None else E.design(x)
    if alphaInit is None:
        if modelMatrix is None:
            roughDisp = dds.attrs["prefit"]["roughDisp"]                            # :713
        else:
            roughDisp = E.prefit(dds.y, dds.nf, x, dds.weights_h if dds.has_weights else None)["roughDisp"]
        bm, bv = dds.mcols["baseMean"], dds.mcols["baseVar"]
        xim = xim_size_factors(dds.sizeFactors) if dds.sizeFactors is not None else E.xim(dds.nf)
        momentsDisp = (bv - xim * bm) / (bm * bm)                                   # :2439-2448
        alpha_hat = np.minimum(roughDisp, momentsDisp)
    else:
        alpha_hat = np.broadcast_to(np.asarray(alphaInit, float), (n,)).copy()
    maxDisp = max(10, m)
    alpha_hat = alpha_init = np.minimum(np.maximum(minDisp, alpha_hat), maxDisp)    # :727-728
    alpha_hat_new = alpha_hat.copy()
    if linearMu is None:
        linearMu = (len(np.unique(modelMatrixGroups(x))) == x.shape[1]) and not useWeights   # :735-742

    def fit_disp(y, mu, la, w):
        return E.fit_disp(y, xh, mu, la, la, 1.0, np.log(minDisp / 10), kappa_0, dispTol, maxit, False,
                          w, useWeights, weightThreshold, useCR)                    # :771-782

    fitidx = np.ones(n, bool)
    mu = None
    dispIter = np.zeros(n, dtype=np.int32)
    last_lp = initial_lp = None
    for it in range(int(niter)):                                                    # :751
        every = bool(fitidx.all())
        idx = None if every else np.where(fitidx)[0]
        y_f = dds.y if every else E.take_rows(dds.y, idx)
        la_f = E.vlog(alpha_hat if every else alpha_hat[idx])
        # `weightsSEXP = weights` (:778) is NOT subset by fitidx: from the second pass on fitDisp pairs the rows
        # of y[fitidx, ] with the FIRST sum(fitidx) rows of the weight matrix.  Mirrored as written.
        w_f = weights if (every or weights is None) else E.take_rows(weights, np.arange(idx.size))
        if not linearMu:
            # The GLM fit is launched, the dispersion search is launched on its mu right behind it, and only then
            # does the host half of fitNbinomGLMs (row checks, optim fallback) run -- overlapping the search.  Genes
            # are independent: rows whose mu the optim fallback replaces (:386) get their search redone below.
            pend = fitNbinomGLMs(dds, rows=idx, alpha_hat=alpha_hat if every else alpha_hat[idx], modelMatrix=modelMatrix,
                                 weights=weights_glm, useWeights=useWeights, mu_floor=minmu, want_hat=False,
                                 defer=True)                                        # :755-757 (the IRLS keeps ITS default
                                                                                    # minmu = 0.5; `minmu` is the floor of :763)
            dispRes = fit_disp(y_f, pend.mu, la_f, w_f)
            fit = pend.finish()
            fitMu = fit["mu"]                                                       # clamped at minmu (:763)
            if fit["optimRows"] is not None and len(fit["optimRows"]) > 0:
                oi = np.asarray(fit["optimRows"])
                sub = fit_disp(E.take_rows(y_f, oi), E.take_rows(fitMu, oi), la_f[oi], E.take_rows(w_f, oi))
                dispRes = {k: np.array(dispRes[k], copy=True) for k in sub.keys()}
                for k in dispRes:
                    dispRes[k][oi] = sub[k]
        else:
            nf_f = dds.nf if every else E.take_rows(dds.nf, idx)
            fitMu = E.clamp_min(E.linear_mu(y_f, nf_f, xh), minmu)                  # :760,763
            dispRes = fit_disp(y_f, fitMu, la_f, w_f)
        mu = fitMu if every else E.set_rows(mu, idx, fitMu)                         # :764
        new = np.minimum(E.vexp(dispRes["log_alpha"]), maxDisp)                     # :785
        if every:
            dispIter = np.asarray(dispRes["iter"]).copy()
            alpha_hat_new = new
        else:
            dispIter[idx] = dispRes["iter"]
            alpha_hat_new = alpha_hat_new.copy()
            alpha_hat_new[idx] = new
        last_lp, initial_lp = dispRes["last_lp"], dispRes["initial_lp"]
        with np.errstate(invalid="ignore"):
            fitidx = np.abs(E.vlog(alpha_hat_new) - E.vlog(alpha_hat)) > .05        # :822
        fitidx[np.isnan(fitidx)] = False
        alpha_hat = alpha_hat_new
        if fitidx.sum() == 0:
            break
    dispGeneEst = alpha_hat.copy()
    if niter == 1:
        noIncrease = last_lp < initial_lp + np.abs(initial_lp) / 1e6               # :828
        dispGeneEst[noIncrease] = alpha_init[noIncrease]
    dispGeneEstConv = (dispIter < maxit) & ~(dispIter == 1)                         # :832
    refitDisp = ~dispGeneEstConv & (dispGeneEst > minDisp * 10)                     # :835
    if refitDisp.sum() > 0:
        idx = np.where(refitDisp)[0]
        dispGrid = fitDispGridWrapper(E, E.take_rows(dds.y, idx), xh, E.take_rows(mu, idx),
                                      np.zeros(idx.size), 1.0, False, E.take_rows(weights, idx), useWeights,
                                      weightThreshold, useCR, m)                    # :837-846
        dispGeneEst[refitDisp] = dispGrid
    dispGeneEst = np.minimum(np.maximum(dispGeneEst, minDisp), maxDisp)             # :848
    dds.mcols["dispGeneEst"] = dispGeneEst
    dds.mcols["dispGeneIter"] = dispIter
    dds.assays["mu"] = mu
    dds.attrs["disp_weights"] = weights
    dds.attrs["useWeights"] = useWeights
    return dds


def parametricDispersionFit(means, disps):
    """R/core.R:2166-2190 in numpy -- kept as an independent cross-check of the engine's
    `parametric_fit` (tests); the pipeline itself calls the engine.  disp ~ asymptDisp +
    extraPois/mean by a Gamma GLM with identity link (stats::glm's IRLS restated: working weights
    mu^-2, working response = disps)."""
    means = np.asarray(means, np.float64)
    disps = np.asarray(disps, np.float64)
    coefs = np.array([0.1, 1.0])
    it = 0
    while True:
        residuals = disps / (coefs[0] + coefs[1] / means)
        good = (residuals > 1e-4) & (residuals < 15)
        yg, xg = disps[good], 1.0 / means[good]
        b = coefs.copy()
        converged = False
        r0 = yg / (b[0] + b[1] * xg)
        dev_old = -2.0 * (np.log(r0).sum() - (r0 - 1.0).sum())     # glm.fit: devold from the start values
        for _ in range(25):                                   # glm.control(maxit = 25, epsilon = 1e-8)
            mu = b[0] + b[1] * xg
            if mu.min() <= 0:
                raise RuntimeError("parametric dispersion fit failed")
            wgt = 1.0 / (mu * mu)
            wx = wgt * xg
            s0, s1, s2 = wgt.sum(), wx.sum(), (wx * xg).sum()
            t0, t1 = (wgt * yg).sum(), (wx * yg).sum()
            det = s0 * s2 - s1 * s1
            b = np.array([(s2 * t0 - s1 * t1) / det, (s0 * t1 - s1 * t0) / det])
            mu = b[0] + b[1] * xg
            if mu.min() <= 0:
                raise RuntimeError("parametric dispersion fit failed")
            r = yg / mu
            dev = -2.0 * (np.log(r).sum() - (r - 1.0).sum())
            if abs(dev - dev_old) / (abs(dev) + 0.1) < 1e-8:
                converged = True
                break
            dev_old = dev
        oldcoefs = coefs
        coefs = b
        if not (coefs > 0).all():
            raise RuntimeError("parametric dispersion fit failed")
        if np.sum(np.log(coefs / oldcoefs) ** 2) < 1e-6 and converged:
            break
        it += 1
        if it > 10:
            raise RuntimeError("dispersion fit did not converge")
    return coefs


def _mad(v):
    med = np.median(v)
    return 1.4826 * np.median(np.abs(v - med))


def trimmed_mean_fit(dge, minDisp=1e-8, trim=0.001):
    """fitType = "mean" (R/core.R:894-899): mean(dispGeneEst[dispGeneEst > 10 minDisp], na.rm = TRUE, trim = 0.001).
    base::mean.default keeps the order statistics floor(N trim) + 1 ... N - floor(N trim) and takes their long-double
    mean with a correction pass -- to double precision the correctly rounded mean.  The specification shared with the
    chain's kernel (csrc/trend.hip: trend_mean_kernel): every kept value as the integer floor(x 2^128), the exact
    integer sum, the quotient rounded once to nearest-even -- Python integers here."""
    import math
    with np.errstate(invalid="ignore"):
        v = np.sort(dge[dge > 10 * minDisp])
    k = int(np.floor(v.size * trim))
    kept = v[k: v.size - k]
    fr, ex = np.frexp(kept)
    M = np.ldexp(fr, 53).astype(np.int64)
    S = 0
    for mnt, sh in zip(M.tolist(), (ex.astype(np.int64) - 53 + 128).tolist()):
        S += (mnt << sh) if sh >= 0 else (mnt >> -sh)
    Q, rem = divmod(S, int(kept.size))
    h = Q.bit_length() - 1
    if h <= 52:
        return math.ldexp(float(Q), -128)
    shift = h - 52
    mant, rest, half = Q >> shift, Q & ((1 << shift) - 1), 1 << (shift - 1)
    if rest > half or (rest == half and (rem != 0 or (mant & 1))):
        mant += 1
    return math.ldexp(float(mant), shift - 128)


LOCAL_SUBSTITUTED = ("-- note: fitType='parametric', but the dispersion trend was not well captured by the\n"
                     "   function: y = a/x + b, and a local regression fit was automatically substituted.\n"
                     "   specify fitType='local' or 'mean' to avoid this message next time.")


def localDispersionFit(dds_or_engine, means, disps, minDisp=1e-8):
    """R/core.R:2194-2203: the function of the mean that fitType = "local" fits to the genes handed in -- the estimator behind
    locfit(logDisps ~ logMeans, weights = means) at locfit's defaults, evaluated directly at every mean it is called on
    (locfit interpolates between the vertices of a tree, so its values are not pinned).  The
    fit and every evaluation run on the engine (the device engine's on the device).  When all disps are below 10 minDisp
    the constant function minDisp comes back, where R returns a vector that cannot be called."""
    E = getattr(dds_or_engine, "engine", dds_or_engine)
    return E.local_fit(means, disps, minDisp)


def estimateDispersionsFit(dds, fitType="parametric", minDisp=1e-8, engine=None, parametricFallback="mean"):
    """R/core.R:864-939 + `dispersionFunction<-` (R/methods.R:142-190).  parametricFallback: what a parametric trend that
    does not fit is answered with -- "mean" (this library's default) or "local" (the reference's substitution and its
    message, :888-893)."""
    E = engine if engine is not None else dds.engine
    if not callable(fitType) and fitType not in ("parametric", "local", "mean"):
        raise ValueError("fitType should be one of 'parametric', 'local', 'mean'")
    if parametricFallback not in ("mean", "local"):
        raise ValueError("parametricFallback should be 'mean' or 'local'")
    dge, bm = dds.mcols["dispGeneEst"], dds.mcols["baseMean"]
    useForFit = dge > 100 * minDisp
    if useForFit.sum() == 0:
        raise RuntimeError("all gene-wise dispersion estimates are within 2 orders of magnitude from the minimum value")
    if fitType == "parametric":
        try:
            coefs = E.parametric_fit(bm[useForFit], dge[useForFit])
            fn = ("parametric", coefs)
        except RuntimeError:
            fitType = parametricFallback
            if fitType == "local":
                import sys
                print(LOCAL_SUBSTITUTED, file=sys.stderr)
    if fitType == "local":
        fn = ("local", localDispersionFit(E, bm[useForFit], dge[useForFit], minDisp))
    if fitType == "mean":
        fn = ("mean", trimmed_mean_fit(dge, minDisp))                                  # mean(trim = 0.001)
    if callable(fitType):
        # the caller's trend, a function of the normalized mean: what R reaches with fitType = "local" (locfit, :889-893:
        # `dispFunction <- localDispersionFit(means[useForFit], disps[useForFit], minDisp)`) or `dispersionFunction(dds) <- f`
        # (R/methods.R:142-190); it is given the vectors of the genes that enter the fit, returns the function of the mean
        fn = ("custom", fitType(bm[useForFit], dge[useForFit]))
    if fn[0] == "parametric":
        dispFit = fn[1][0] + fn[1][1] / bm
    elif fn[0] in ("custom", "local"):
        with np.errstate(invalid="ignore", divide="ignore"):
            dispFit = np.asarray(fn[1](bm), dtype=np.float64)
    else:
        dispFit = np.full(bm.shape, fn[1])
    dds.mcols["dispFit"] = dispFit
    aboveMinDisp = dge >= minDisp * 100
    varLogDispEsts = None
    if aboveMinDisp.sum() > 0:
        res = E.vlog(dge) - E.vlog(dispFit)
        md = E.mad(res[aboveMinDisp])
        varLogDispEsts = md * md                                                       # mad(...)^2, methods.R:180
    dds.dispersionFunction = {"fitType": fn[0], "coefficients": fn[1], "varLogDispEsts": varLogDispEsts}
    return dds


def estimateDispersionsPriorVar(dds, minDisp=1e-8):
    """R/core.R:1135-1208 (the (m-p) <= 3 Monte-Carlo branch relies on R's RNG stream and is not
    mirrored)"""
    dge = dds.mcols["dispGeneEst"]
    aboveMinDisp = dge >= minDisp * 100
    if aboveMinDisp.sum() == 0:
        raise RuntimeError("no data found which is greater than minDisp")
    varLogDispEsts = dds.dispersionFunction["varLogDispEsts"]
    m, p = dds.x.shape
    if (m - p) <= 3 and m > p:
        raise NotImplementedError("residual df <= 3: the reference's seeded Monte-Carlo matching is not mirrored")
    if m > p:
        expVarLogDisp = sps.polygamma(1, (m - p) / 2.0)
        return float(max(varLogDispEsts - expVarLogDisp, 0.25))                       # :1200
    return float(varLogDispEsts)


def estimateDispersionsMAP(dds, outlierSD=2, dispPriorVar=None, minDisp=1e-8, kappa_0=1.0, dispTol=1e-6,
                           maxit=100, useCR=True, weightThreshold=1e-2, modelMatrix=None):
    """R/core.R:943-1131.  modelMatrix: the caller's design (R/core.R:945, 1003-1005: the Cox-Reid term of the MAP search runs
    on it); default: the one the gene-wise estimate ran on, else the object's"""
    E = dds.engine
    if modelMatrix is None:
        modelMatrix = dds.attrs.get("geneEstModelMatrix")
    xh = dds.xh if modelMatrix is None else E.design(np.asarray(modelMatrix, np.float64))
    if dispPriorVar is None:
        dispPriorVar = estimateDispersionsPriorVar(dds, minDisp)                     # :986
    dds.dispersionFunction["dispPriorVar"] = dispPriorVar
    weights, useWeights = getAndCheckWeights(dds, weightThreshold, modelMatrix=modelMatrix)      # :999 (no 1e-6 floor here)
    dge, dfit = dds.mcols["dispGeneEst"], dds.mcols["dispFit"]
    mu = dds.assays["mu"]
    dispInit = np.where(dge > 0.1 * dfit, dge, dfit)                                 # :1019-1021
    dispInit = np.where(np.isnan(dispInit), dfit, dispInit)
    log_dfit = E.vlog(dfit)
    res = E.fit_disp(dds.y, xh, mu, E.vlog(dispInit), log_dfit, dispPriorVar, np.log(minDisp / 10),
                     kappa_0, dispTol, maxit, True, weights, useWeights, weightThreshold, useCR)   # :1027-1039
    dispMAP = E.vexp(res["log_alpha"])
    dispIter = res["iter"]
    dispConv = dispIter < maxit                                                      # :1048
    refitDisp = ~dispConv
    if refitDisp.sum() > 0:
        idx = np.where(refitDisp)[0]
        dispGrid = fitDispGridWrapper(E, E.take_rows(dds.y, idx), xh, E.take_rows(mu, idx),
                                      log_dfit[idx], dispPriorVar, True, E.take_rows(weights, idx),
                                      useWeights, weightThreshold, True, dds.m)      # :1051-1061
        dispMAP[refitDisp] = dispGrid
    maxDisp = max(10, dds.m)
    dispMAP = np.minimum(np.maximum(dispMAP, minDisp), maxDisp)                      # :1100-1101
    dispersionFinal = dispMAP.copy()
    varLogDispEsts = dds.dispersionFunction["varLogDispEsts"]
    dispOutlier = E.vlog(dge) > log_dfit + outlierSD * np.sqrt(varLogDispEsts)      # :1111-1113
    dispOutlier[np.isnan(dispOutlier)] = False
    dispersionFinal[dispOutlier] = dge[dispOutlier]
    dds.mcols.update(dispersion=dispersionFinal, dispIter=dispIter, dispOutlier=dispOutlier, dispMAP=dispMAP)
    return dds


def estimateDispersions(dds, fitType="parametric", maxit=100, dispPriorVar=None, parametricFallback="mean", **kw):
    """R/methods.R:500-563 (maxit is handed to both dispersion searches, :520,:546).  dispPriorVar: the argument of
    estimateDispersionsMAP (R/core.R:989-994) for callers that run the three steps themselves -- the way an analysis with
    residual df <= 3 gets its prior variance (R's estimate there needs R's RNG, :1155-1190).  parametricFallback: see
    estimateDispersionsFit."""
    estimateDispersionsGeneEst(dds, maxit=maxit, **kw)
    estimateDispersionsFit(dds, fitType=fitType, parametricFallback=parametricFallback)
    estimateDispersionsMAP(dds, maxit=maxit, dispPriorVar=dispPriorVar, modelMatrix=kw.get("modelMatrix"))   # (R/methods.R:546)
    return dds


# ------------------------------------------------------------------ beta prior (R/core.R:1601-1689, R/expanded.R)
def standard_model_matrix(factors):
    """model.matrix(~ f1 + f2 + ...) with treatment contrasts; `factors` is an ordered dict
    name -> integer level codes (0 = reference level).  Returns (x, column names)."""
    m = len(next(iter(factors.values())))
    cols, names = [np.ones(m)], ["Intercept"]
    for f, codes in factors.items():
        codes = np.asarray(codes)
        for lv in range(1, int(codes.max()) + 1):
            cols.append((codes == lv).astype(np.float64)); names.append("%s%d" % (f, lv))
    return np.column_stack(cols), names


def makeExpandedModelMatrix(factors):
    """R/expanded.R:1-18: intercept + one indicator per level of every design factor
    (rank deficient; made solvable by the ridge)."""
    m = len(next(iter(factors.values())))
    cols, names = [np.ones(m)], ["Intercept"]
    for f, codes in factors.items():
        codes = np.asarray(codes)
        for lv in range(0, int(codes.max()) + 1):
            cols.append((codes == lv).astype(np.float64)); names.append("%s%d" % (f, lv))
    return np.column_stack(cols), names


def Hmisc_wtd_quantile(x, weights, prob, normwt=True, sorter=None):
    """R/core.R:2762-2800 (type = 'quantile'), one probability.  `sorter(values)` may supply the stable ascending
    order of `values` (an engine can sort on the device; the stable order of a vector is unique, so nothing changes)."""
    x = np.asarray(x, float); w = np.asarray(weights, float)
    keep = ~(np.isnan(w) | (w == 0))
    x, w = x[keep], w[keep]
    if x.size == 0:                    # (no row with a usable weight: NaN, as csrc/beta_prior.hip returns)
        return np.nan
    if normwt:
        w = w * x.size / np.cumsum(w)[-1]          # (every sum here is sequential: the order csrc/beta_prior.hip follows)
    o = np.argsort(x, kind="stable") if sorter is None else np.asarray(sorter(x))
    x, w = x[o], w[o]
    # the distinct values of the sorted vector and, per value, the sum of its weights in index order (what
    # unique(return_inverse) + bincount give, without sorting a second time)
    head = np.empty(x.size, bool)
    head[:1] = True
    np.not_equal(x[1:], x[:-1], out=head[1:])
    ux = x[head]
    inv = np.cumsum(head) - 1
    wts = np.bincount(inv, weights=w)
    cs = np.cumsum(wts)
    n = cs[-1]
    order = 1 + (n - 1) * prob
    low = max(np.floor(order), 1.0)
    high = min(low + 1, n)
    frac = order % 1

    def stepq(q):                      # approx(cumsum(wts), x, method='constant', f=1, rule=2)
        i = np.searchsorted(cs, q, side="left")
        return ux[min(i, ux.size - 1)]
    return (1 - frac) * stepq(low) + frac * stepq(high)


def matchWeightedUpperQuantileForVariance(x, weights, upperQuantile=0.05, sorter=None):
    """R/core.R:2416-2419"""
    qn = 1.959963984540054 if upperQuantile == 0.05 else sps.ndtri(1 - upperQuantile / 2)       # qnorm(1 - 0.05 / 2)
    sdEst = float(Hmisc_wtd_quantile(np.abs(x), weights, 1 - upperQuantile, normwt=True, sorter=sorter) / qn)
    return sdEst * sdEst


def matchUpperQuantileForVariance(x, upperQuantile=0.05):
    """R/core.R:2411-2414"""
    return float(np.quantile(np.abs(x), 1 - upperQuantile) / sps.ndtri(1 - upperQuantile / 2)) ** 2


def estimateBetaPriorVar(dds, mleBetaMatrix, names, betaPriorMethod="weighted", upperQuantile=0.05,
                         modelMatrixType="standard", factors=None, sorter=None):
    """R/core.R:1601-1689.  `mleBetaMatrix` (log2 scale) are the MLE coefficients of the standard
    design whose column names are `names`."""
    beta = np.asarray(mleBetaMatrix, float)
    names = list(names)
    if modelMatrixType == "expanded":                                  # addAllContrasts, expanded.R:76-98
        pairs = []
        for f, codes in factors.items():
            idx = [i for i, nm in enumerate(names) if nm.startswith(f) and nm != "Intercept"]
            k = len(idx)
            if k > 1:
                for j in range(k - 1):
                    for i in range(j + 1, k):
                        pairs.append((idx[i], idx[j]))
                        names.append(f + "Cntrst")
        if pairs:                                                      # (one allocation for all contrast columns)
            p0 = beta.shape[1]
            wide = np.empty((beta.shape[0], p0 + len(pairs)))
            wide[:, :p0] = beta
            ii, jj = np.array(pairs).T
            np.subtract(beta[:, ii], beta[:, jj], out=wide[:, p0:])
            beta = wide
    dispFit = dds.mcols.get("dispFit")
    if dispFit is None:
        dispFit = np.mean(dds.mcols["dispersion"])
    weights = 1.0 / (1.0 / dds.mcols["baseMean"] + dispFit)            # :1641-1642
    pv = np.empty(beta.shape[1])
    for c in range(beta.shape[1]):
        xcol = beta[:, c]
        if beta.shape[0] == 1:                                         # a one-gene object: (betaMatrix)^2, :1647,1662
            pv[c] = float(xcol[0]) ** 2
            continue
        use = np.abs(xcol) < 10
        if use.sum() == 0:
            pv[c] = 1e6
        elif betaPriorMethod == "quantile":
            pv[c] = matchUpperQuantileForVariance(xcol[use], upperQuantile)
        else:
            pv[c] = matchWeightedUpperQuantileForVariance(xcol[use], weights[use], upperQuantile, sorter=sorter)
    for c, nm in enumerate(names):
        if nm == "Intercept":
            pv[c] = 1e6                                               # :1669-1671
    if modelMatrixType == "expanded":                                  # averagePriorsOverLevels, expanded.R:20-73
        xe, enames = makeExpandedModelMatrix(factors)
        out = np.zeros(len(enames))
        for c, nm in enumerate(names):
            if nm in enames:
                out[enames.index(nm)] = pv[c]
        for f in factors:
            mmset = {nm for nm in enames if nm.startswith(f)} | {f + "Cntrst"}
            vals = [pv[c] for c, nm in enumerate(names) if nm in mmset]
            meanvar = float(np.cumsum(vals)[-1] / len(vals))
            for i, nm in enumerate(enames):
                if nm.startswith(f) and nm != "Intercept":
                    out[i] = meanvar
        if not (out > 0).all():
            raise RuntimeError("beta prior is not greater than 0")
        return out, enames
    return pv, names


def fitGLMsWithPrior(dds, betaTol=1e-8, maxit=100, useOptim=True, useQR=True, betaPriorVar=None,
                     modelMatrixType="standard", factors=None, minmu=0.5, weights=None, useWeights=False):
    """R/fitNbinomGLMs.R:242-337: (1) MLE fit with the wide prior, (2) the all-gene beta prior
    variance, (3) refit with lambda = 1/betaPriorVar on the standard or expanded design."""
    if modelMatrixType == "expanded" and factors is None:
        raise ValueError("an expanded model matrix needs the design factors")
    names = standard_model_matrix(factors)[1] if factors is not None else ["Intercept"] + [
        "V%d" % i for i in range(1, dds.p)]
    fit = fitNbinomGLMs(dds, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR, minmu=minmu,
                        weights=weights, useWeights=useWeights)                       # :256-260
    H, mu, mle = fit["hat_diagonals"], fit["mu"], fit["betaMatrix"]
    if betaPriorVar is None:
        betaPriorVar, pnames = estimateBetaPriorVar(dds, mle, names, modelMatrixType=modelMatrixType,
                                                    factors=factors)                  # :293
    if (np.asarray(betaPriorVar) == 0).any():
        raise ValueError("beta prior variances are equal to zero for some variables")
    lam = 1.0 / np.asarray(betaPriorVar, float)                                       # :311
    if modelMatrixType == "expanded":
        xe, _ = makeExpandedModelMatrix(factors)
        fit2 = fitNbinomGLMs(dds, lam=lam, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR,
                             modelMatrix=xe, minmu=minmu, weights=weights, useWeights=useWeights,
                             want_loglike=True)                                        # :319-325
    else:
        fit2 = fitNbinomGLMs(dds, lam=lam, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR,
                             minmu=minmu, weights=weights, useWeights=useWeights, want_loglike=True)   # :314-317
    return {"fit": fit2, "H": H, "betaPriorVar": np.asarray(betaPriorVar), "mu": mu,
            "modelMatrix": fit2["modelMatrix"], "mleBetaMatrix": mle}


# ------------------------------------------------------------------ tests
def nbinomWaldTest(dds, betaTol=1e-8, maxit=100, useOptim=True, useT=False, df=None, useQR=True, minmu=0.5,
                   modelMatrix=None, betaPrior=False, betaPriorVar=None, modelMatrixType=None, factors=None):
    """R/core.R:1332-1565.  betaPrior = TRUE goes through
    fitGLMsWithPrior (:1416-1432), by default on the expanded model matrix (:1374-1380)."""
    if "dispersion" not in dds.mcols:
        raise RuntimeError("testing requires dispersion estimates, first call estimateDispersions()")
    E = dds.engine
    weights, useWeights = getAndCheckWeights(dds)
    if not betaPrior:
        fit = fitNbinomGLMs(dds, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR, minmu=minmu,
                            modelMatrix=modelMatrix, weights=weights, useWeights=useWeights,
                            want_loglike=True)                                                   # :1403-1408
        H, mu_fit = fit["hat_diagonals"], fit["mu"]
        bpv = np.full(fit["nterms"], 1e6)
    else:
        if modelMatrixType is None:
            modelMatrixType = "expanded" if factors is not None else "standard"
        pf = fitGLMsWithPrior(dds, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR,
                              betaPriorVar=betaPriorVar, modelMatrixType=modelMatrixType, factors=factors,
                              minmu=minmu, weights=weights, useWeights=useWeights)       # :1416-1421
        fit, H, mu_fit, bpv = pf["fit"], pf["H"], pf["mu"], pf["betaPriorVar"]
        dds.mcols["MLE_beta"] = pf["mleBetaMatrix"]
    fit = dict(fit); fit["mu"] = mu_fit; fit["hat_diagonals"] = H
    dds.assays["mu"] = fit["mu"]
    dds.assays["H"] = fit["hat_diagonals"]
    dds.attrs.update(betaPrior=bool(betaPrior), betaPriorVar=bpv, test="Wald",
                     modelMatrixType=modelMatrixType, factors=factors, useT=bool(useT))
    calculateCooksDistance(dds, H, dds.x if modelMatrix is None else np.asarray(modelMatrix, float))   # :1451-1463
    betaMatrix, betaSE = fit["betaMatrix"], fit["betaSE"]
    with np.errstate(divide="ignore", invalid="ignore"):
        WaldStatistic = betaMatrix / betaSE                                         # :1471
    if useT:
        from scipy.stats import t as tdist
        if df is None:
            num = E.to_numpy(weights).sum(axis=1) if useWeights else np.full(dds.n, dds.m)
            df = num - dds.p
        df = np.where(np.asarray(df, float) > 0, df, np.nan)
        WaldPvalue = 2 * tdist.sf(np.abs(WaldStatistic), df=np.asarray(df)[:, None])
        dds.mcols["tDegreesFreedom"] = np.array(np.broadcast_to(np.asarray(df, np.float64), (dds.n,)))   # :1523-1524
    else:
        WaldPvalue = E.two_sided_normal_p(WaldStatistic)                            # :1507
    logLike = fit["logLike"]                                                    # fitNbinomGLMs.R:182,399
    dds.mcols.update(beta=betaMatrix, betaSE=betaSE, WaldStatistic=WaldStatistic, WaldPvalue=WaldPvalue,
                     betaConv=fit["betaConv"], betaIter=fit["betaIter"], deviance=-2 * logLike,
                     rowsForOptim=fit["rowsForOptim"])
    return dds


def pchisq_upper(stat, df):
    """pchisq(stat, df, lower.tail = FALSE) (R/core.R:1878) -- the value scipy.stats.chi2.sf returns (its _sf IS
    scipy.special.chdtrc) without the distribution machinery around it (argument broadcasting / masking: a quarter of
    its 4 ms per 60 000 genes, which shows in a C4 step on the device chain)"""
    stat = np.asarray(stat, np.float64)
    if not (np.ndim(df) == 0 and df > 0):
        from scipy.stats import chi2
        return chi2.sf(stat, df=df)
    from scipy.special import chdtrc
    out = chdtrc(float(df), stat)
    out[np.isnan(stat)] = np.nan
    return out


def nbinomLRT(dds, reduced, betaTol=1e-8, maxit=100, useOptim=True, useQR=True, minmu=0.5):
    """R/core.R:1787-2012: full vs reduced model matrices (betaPrior = FALSE).  `reduced` is a
    model matrix whose column space is nested in dds.x; an intercept-only reduced model takes
    the closed form of R/fitNbinomGLMs.R:99-137."""
    E = dds.engine
    reduced = np.asarray(reduced, np.float64)
    weights, useWeights = getAndCheckWeights(dds)
    disp = dds.mcols["dispersion"]
    full = fitNbinomGLMs(dds, betaTol=betaTol, maxit=maxit, useOptim=useOptim, useQR=useQR, minmu=minmu,
                         weights=weights, useWeights=useWeights, want_loglike=True)
    ll_full = full["logLike"]
    red = fitNbinomGLMs(dds, modelMatrix=reduced, betaTol=betaTol, maxit=maxit, useOptim=useOptim,
                        useQR=useQR, minmu=minmu, weights=weights, useWeights=useWeights, want_hat=False,
                        want_loglike=True)                        # closed form when reduced is ~1 (:99-137)
    ll_red = red["logLike"]
    LRTStatistic = 2 * (ll_full - ll_red)                                            # :1877
    LRTPvalue = pchisq_upper(LRTStatistic, full["nterms"] - red["nterms"])            # :1878
    dds.assays["mu"] = full["mu"]
    dds.assays["H"] = full["hat_diagonals"]
    dds.attrs.update(betaPrior=False, test="LRT", reduced=reduced)
    calculateCooksDistance(dds, full["hat_diagonals"], dds.x)                         # :1886-1891
    dds.mcols.update(beta=full["betaMatrix"], betaSE=full["betaSE"], LRTStatistic=LRTStatistic,
                     LRTPvalue=LRTPvalue, fullBetaConv=full["betaConv"], betaIter=full["betaIter"],
                     deviance=-2 * ll_full)
    return dds


# ------------------------------------------------------------------ count outliers
def nOrMoreInCell(modelMatrix, n):
    """R/core.R:2366-2371: per sample, are there n or more samples with the same model-matrix row"""
    return _cells(modelMatrix)[1] >= n


def calculateCooksDistance(dds, H, modelMatrix):
    """calculateCooksDistance (R/core.R:2333-2340) on the robust method-of-moments dispersion
    (:2277-2331) + recordMaxCooks (:2349-2359); one engine pass over assays mu / H."""
    r = dds.engine.cooks_distance(dds.y, dds.nf, dds.assays["mu"], H, modelMatrix)
    dds.assays["cooks"] = r["cooks"]
    dds.mcols["maxCooks"] = r["maxCooks"]
    dds.attrs["dispModelMatrix"] = np.asarray(modelMatrix, np.float64)
    return dds


def replaceOutliers(dds, trim=.2, cooksCutoff=None, minReplicates=7, whichSamples=None):
    """R/core.R:2069-2115.  The replaced count matrix goes to assays["replaceCounts"] (the handle
    the refit reads); dds.y keeps the original counts, as counts(dds) does at the end of
    refitWithoutOutliers (:2553-2557)."""
    from scipy.stats import f as fdist
    if "cooks" not in dds.assays:
        raise RuntimeError("first run DESeq, nbinomWaldTest, or nbinomLRT to identify outliers")
    if minReplicates < 3:
        raise ValueError("at least 3 replicates are necessary in order to indentify a sample as a count outlier")
    x = dds.attrs["dispModelMatrix"]
    p, m = x.shape[1], dds.m
    if m <= p:
        return dds
    if cooksCutoff is None:
        cooksCutoff = float(fdist.ppf(.99, p, m - p))                                # :2081
    if whichSamples is None:
        whichSamples = nOrMoreInCell(x, minReplicates)                               # :2101
    whichSamples = np.asarray(whichSamples, bool)
    dds.attrs["replaceable"] = whichSamples
    r = dds.engine.replace_outliers(dds.y, dds.nf, dds.assays["cooks"], cooksCutoff, whichSamples, trim)
    dds.mcols["replace"] = r["replace"]
    dds.assays["replaceCounts"] = r["counts"] if whichSamples.any() else dds.y       # :2108-2112
    return dds


_RESULT_COLS = ("beta", "betaSE", "WaldStatistic", "WaldPvalue", "LRTStatistic", "LRTPvalue", "betaConv",
                "fullBetaConv", "betaIter", "deviance", "maxCooks", "tDegreesFreedom")


def _dispersion_function(dds, baseMean):
    fn = dds.dispersionFunction
    if fn["fitType"] == "parametric":
        return fn["coefficients"][0] + fn["coefficients"][1] / baseMean
    if fn["fitType"] in ("custom", "local"):
        return np.asarray(fn["coefficients"](baseMean), dtype=np.float64)
    return np.full(baseMean.shape, fn["coefficients"])


def refitWithoutOutliers(dds, test="Wald", reduced=None, minReplicatesForReplace=7, disp_maxit=100, count_all=None, **kw):
    """R/core.R:2484-2563: replace count outliers by the trimmed mean, then re-estimate the
    dispersion and refit the rows that had a replacement (all through the same engine entry
    points, on the row subset).  `count_all`: when `dds` is one shard of a gene-sharded analysis, a function that adds
    a count up over all shards (called exactly once) -- the closing steps (NA results on the rows that became all zero,
    maxCooks, :2535-2546) run when ANY row of the whole object was refitted (:2496), as on the unsharded object."""
    E = dds.engine
    # the refit runs estimateDispersionsGeneEst / MAP and nbinomWaldTest / nbinomLRT on their DEFAULTS: DESeq()'s betaTol,
    # maxit, useQR, minmu, useT, df are not handed on (:2509-2531) -- refitted rows carry normal-distribution p-values
    # even in a useT analysis
    # ... but the caller's model matrix IS (modelMatrix = modelMatrix in the gene-wise estimate, the MAP estimate and the test of
    # the refit, :2509-2527)
    kw = {k: v for k, v in kw.items() if k == "modelMatrix" and v is not None}
    replaceOutliers(dds, minReplicates=minReplicatesForReplace)
    if "replace" not in dds.mcols:
        if count_all is not None:
            count_all(0)
        return dds
    replace = dds.mcols["replace"]
    nrefit = int(replace.sum())
    newAllZero = np.array([], int)
    refitReplace = np.array([], int)
    whole = None
    if nrefit > 0:
        idx_rep = np.where(replace)[0]
        whole = dds.subset(idx_rep, dds.assays["replaceCounts"])
        getBaseMeansAndVariances(whole)                                               # :2491
        for k in ("baseMean", "baseVar", "allZero"):
            dds.mcols[k] = dds.mcols[k].copy()
            dds.mcols[k][idx_rep] = whole.mcols[k]
        newAllZero = idx_rep[whole.mcols["allZero"]]
        refitReplace = idx_rep[~whole.mcols["allZero"]]
    n_refit_all = refitReplace.size if count_all is None else int(count_all(int(refitReplace.size)))
    if refitReplace.size > 0:                                                         # :2496
        keep = ~whole.mcols["allZero"]
        sub = whole if keep.all() else dds.subset(refitReplace, dds.assays["replaceCounts"])
        estimateDispersionsGeneEst(sub, maxit=disp_maxit, **kw)                       # :2509
        sub.mcols["dispFit"] = _dispersion_function(dds, sub.mcols["baseMean"])       # :2512
        estimateDispersionsMAP(sub, dispPriorVar=dds.dispersionFunction["dispPriorVar"], maxit=disp_maxit, **kw)   # :2518-2519
        if test == "Wald":
            nbinomWaldTest(sub, betaPrior=dds.attrs.get("betaPrior", False), betaPriorVar=(
                dds.attrs["betaPriorVar"] if dds.attrs.get("betaPrior", False) else None),
                modelMatrixType=dds.attrs.get("modelMatrixType"), factors=dds.attrs.get("factors"), **kw)
        else:
            nbinomLRT(sub, reduced)         # (full / reduced are the matrices themselves in this mirror)
        for k, v in sub.mcols.items():                                                # :2533-2534
            if k not in dds.mcols or k == "rowsForOptim" or np.shape(v)[:1] != (sub.n,):
                continue
            dst = np.array(dds.mcols[k], copy=True)
            dst[refitReplace] = v
            dds.mcols[k] = dst
    if n_refit_all > 0:
        for k in _RESULT_COLS:                                                        # :2535
            if k in dds.mcols and newAllZero.size:
                a = dds.mcols[k]
                if a.dtype.kind != "f":
                    a = a.astype(np.float64)
                a[newAllZero] = np.nan
                dds.mcols[k] = a
        replaceable = dds.attrs["replaceable"]
        if replaceable.all():                                                         # :2538-2546
            dds.mcols["maxCooks"] = np.full(dds.n, np.nan)
        else:
            x = dds.attrs["dispModelMatrix"]
            if x.shape[0] > x.shape[1] and nOrMoreInCell(x, 3).any():
                dds.mcols["maxCooks"] = E.masked_row_max(dds.assays["cooks"], nOrMoreInCell(x, 3), replaceable)
            else:
                dds.mcols["maxCooks"] = np.full(dds.n, np.nan)
    if nrefit == 0:
        dds.assays.pop("replaceCounts", None)
        return dds
    dds.assays["replaceCooks"] = dds.assays["cooks"]                                   # :2551
    return dds


def cooksOutlier(dds, cooksCutoff=None):
    """The Cook's-distance filter results() applies to the p-values (R/results.R:520-564): genes whose
    maxCooks exceeds qf(.99, p, m - p); for a two-group design a gene is kept when three or more
    counts are larger than the count with the largest Cook's distance (:541-560).  Returns the flags
    (results() sets pvalue <- NA there)."""
    from scipy.stats import f as fdist
    x = dds.attrs["dispModelMatrix"]
    m, p = x.shape
    if cooksCutoff is None:
        cooksCutoff = float(fdist.ppf(.99, p, m - p))
    mx = dds.mcols["maxCooks"]
    with np.errstate(invalid="ignore"):
        out = np.where(np.isnan(mx), False, mx > cooksCutoff)
    two_group = p == 2 and (x[:, 0] == 1).all() and set(np.unique(x[:, 1])) <= {0.0, 1.0}
    if out.any() and two_group:
        E = dds.engine
        ii = np.where(out)[0]
        cnt = E.to_numpy(E.take_rows(dds.y, ii))
        ck = E.to_numpy(E.take_rows(dds.assays["cooks"], ii))
        outCount = cnt[np.arange(ii.size), np.argmax(ck, axis=1)]
        out[ii[(cnt > outCount[:, None]).sum(axis=1) >= 3]] = False
    return out


def _DESeqNZ(dds, test, fitType, reduced, minReplicatesForReplace, disp_maxit=100, **kw):
    dpv = kw.pop("dispPriorVar", None)      # (not an argument of R's DESeq(): of estimateDispersionsMAP, R/core.R:989-994)
    fallback = kw.pop("parametricFallback", "mean")                  # (nor this one: of estimateDispersionsFit here)
    estimateDispersions(dds, fitType=fitType, maxit=disp_maxit, minmu=kw.get("minmu", 0.5), dispPriorVar=dpv,
                        parametricFallback=fallback)                                                                # R/core.R:393
    if test == "Wald":
        nbinomWaldTest(dds, **kw)
    elif test == "LRT":
        nbinomLRT(dds, reduced, **kw)
    else:
        raise ValueError("test should be either 'Wald' or 'LRT'")
    if np.isfinite(minReplicatesForReplace) and nOrMoreInCell(dds.x, minReplicatesForReplace).any():   # :419-426
        refitWithoutOutliers(dds, test=test, reduced=reduced, minReplicatesForReplace=minReplicatesForReplace,
                             disp_maxit=disp_maxit, **kw)
    return dds


def DESeq(dds, test="Wald", fitType="parametric", reduced=None, minReplicatesForReplace=7, sfType=None, **kw):
    """R/core.R:280-432, serial path.  sfType = None takes the size / normalization factors of the object as given;
    "ratio", "poscounts" or "iterate" estimates them first, as DESeq() does (R/core.R:304,378-389).
    minReplicatesForReplace = np.inf switches the outlier refit off.
    Rows whose counts are all zero are set aside as every step of the reference does (objectNZ,
    e.g. R/core.R:705,1351) and come back as NA (NaN) rows of mcols (buildDataFrameWithNARows);
    the n x m assays then cover the non-zero rows, listed in attrs["nz_rows"]."""
    if sfType is not None:
        estimateSizeFactors(dds, type=sfType)
    getBaseMeansAndVariances(dds)
    if dds.has_weights:
        getAndCheckWeights(dds)       # rows whose weights leave a degenerate design count as all-zero (R/core.R:2737)
    allZero = dds.mcols["allZero"]
    if not allZero.any():
        return _DESeqNZ(dds, test, fitType, reduced, minReplicatesForReplace, **kw)
    nz = np.where(~allZero)[0]
    if nz.size == 0:
        raise ValueError("all genes have zero counts in every sample")
    keep = {k: dds.mcols[k] for k in ("baseMean", "baseVar", "allZero", "weightsFail") if k in dds.mcols}
    sub = _DESeqNZ(dds.subset(nz), test, fitType, reduced, minReplicatesForReplace, **kw)
    out = {}
    for k, v in sub.mcols.items():
        v = np.asarray(v)
        if v.shape[:1] != (nz.size,) or k == "rowsForOptim":
            continue
        full = np.full((dds.n,) + v.shape[1:], np.nan)
        full[nz] = v
        out[k] = full
    for k, v in keep.items():
        # the refit may have updated baseMean / baseVar / allZero of its rows (R/core.R:2491-2494): take the
        # non-zero rows from the sub-analysis, the all-zero rows as first computed
        full = np.array(v, copy=True)
        if k in sub.mcols and np.shape(sub.mcols[k])[:1] == (nz.size,):
            full[nz] = sub.mcols[k]
        out[k] = full
    dds.mcols = out
    dds.assays, dds.attrs = sub.assays, dict(sub.attrs, nz_rows=nz)
    dds.dispersionFunction = sub.dispersionFunction
    return dds


# ------------------------------------------------------------------ R/vst.R, R/helper.R:421-436
class DESeqTransform:
    """What the transformations return: the n x m engine handle of the transformed values (resident in HBM on the device
    engine) next to the object it was computed from.  assay() brings the matrix to the host on request."""

    def __init__(self, dds, handle, kind):
        self.dds, self.handle, self.kind, self.engine = dds, handle, kind, dds.engine
        self.attrs, self.mcols = {}, {}          # attr(dt, .) and mcols(dt) of the transform itself (rlog: betaPriorVar, rlogIntercept)

    def assay(self):
        return np.asarray(self.engine.to_numpy(self.handle))


def _norm_source(dds):
    """what the engine divides by: the m size factors when the object has them, else the normalization-factor handle"""
    if dds.sizeFactors is not None:
        return None, dds.sizeFactors
    return dds.nf, None


def normalized_counts(dds):
    """counts(object, normalized = TRUE) (R/methods.R:58-69)"""
    nf, sf = _norm_source(dds)
    return DESeqTransform(dds, dds.engine.vst_transform(dds.y, nf, "normalized", sizeFactors=sf), "normalized")


def normTransform(dds, pc=1):
    """R/helper.R:421-436 with its default f = log2: log2(counts(object, normalized = TRUE) + pc)"""
    nf, sf = _norm_source(dds)
    return DESeqTransform(dds, dds.engine.vst_transform(dds.y, nf, "log2", sizeFactors=sf, pc=pc), "log2")


def fmm_spline(x, y):
    """The coefficients of splinefun(x, y)'s default method "fmm" (Forsythe, Malcolm & Moler's SPLINE): the cubic spline
    whose third derivative at either end is that of the cubic through the first / the last four points.  Returns the
    5 x K table x | y | b | c | d with S(u) = y_i + dx (b_i + dx (c_i + dx d_i)), dx = u - x_i."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    n = x.size
    if n < 2 or not (np.diff(x) > 0).all():
        raise ValueError("fmm_spline needs at least two strictly ascending knots")
    b, c, d = np.zeros(n), np.zeros(n), np.zeros(n)
    if n < 3:
        b[:] = (y[1] - y[0]) / (x[1] - x[0])
        return np.vstack([x, y, b, c, d])
    last = n - 1
    # tridiagonal system: b = diagonal, d = off-diagonal, c = right-hand side
    d[0] = x[1] - x[0]
    c[1] = (y[1] - y[0]) / d[0]
    for i in range(1, last):
        d[i] = x[i + 1] - x[i]
        b[i] = 2.0 * (d[i - 1] + d[i])
        c[i + 1] = (y[i + 1] - y[i]) / d[i]
        c[i] = c[i + 1] - c[i]
    # end conditions: third derivatives from divided differences
    b[0], b[last] = -d[0], -d[n - 2]
    c[0] = c[last] = 0.0
    if n > 3:
        c[0] = c[2] / (x[3] - x[1]) - c[1] / (x[2] - x[0])
        c[last] = c[n - 2] / (x[last] - x[n - 3]) - c[n - 3] / (x[n - 2] - x[n - 4])
        c[0] = c[0] * d[0] * d[0] / (x[3] - x[0])
        c[last] = -c[last] * d[n - 2] * d[n - 2] / (x[last] - x[n - 4])
    for i in range(1, n):                                  # elimination
        t = d[i - 1] / b[i - 1]
        b[i] = b[i] - t * d[i - 1]
        c[i] = c[i] - t * c[i - 1]
    c[last] = c[last] / b[last]                            # back substitution
    for i in range(n - 2, -1, -1):
        c[i] = (c[i] - d[i] * c[i + 1]) / b[i]
    b[last] = (y[last] - y[n - 2]) / d[n - 2] + d[n - 2] * (c[n - 2] + 2.0 * c[last])
    for i in range(last):
        b[i] = (y[i + 1] - y[i]) / d[i] - d[i] * (c[i + 1] + 2.0 * c[i])
        d[i] = (c[i + 1] - c[i]) / d[i]
        c[i] = 3.0 * c[i]
    c[last] = 3.0 * c[last]
    d[last] = d[n - 2]
    return np.vstack([x, y, b, c, d])


def quantile7(v, p):
    """stats::quantile's default (type 7): (1 - g) x[lo] + g x[hi] at h = (n - 1) p"""
    s = np.sort(np.asarray(v, np.float64))
    h = (s.size - 1) * p
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    g = h - lo
    if g == 0 or s[hi] == s[lo]:
        return float(s[lo])
    return float((1 - g) * s[lo] + g * s[hi])


def vst_spline_table(dispFunction, max_q, xim, ngrid=1000):
    """The numerically integrated transformation of a non-parametric trend (R/vst.R:166-174): the grid
    sinh(seq(0, asinh(max q), length = 1000))[-1], the integrand 1 / sqrt(f(x) x^2 + xim x), its cumulative trapezoid sums,
    and splinefun() through them at asinh of the interval midpoints.  Returns the 5 x 998 table."""
    xg = np.sinh(np.linspace(0.0, np.arcsinh(max_q), ngrid))[1:]
    with np.errstate(all="ignore"):
        base = np.asarray(dispFunction(xg), dtype=np.float64) * xg ** 2 + xim * xg
        integrand = 1.0 / np.sqrt(base)
    knots = np.arcsinh((xg[1:] + xg[:-1]) / 2)
    vals = np.cumsum((xg[1:] - xg[:-1]) * (integrand[1:] + integrand[:-1]) / 2)
    if not np.isfinite(vals).all():
        raise ValueError("the dispersion function gives no finite variance on the integration grid")
    return fmm_spline(knots, vals)


def vst_subset_rows(baseMean, nsub):
    """the rows vst() estimates the trend on (R/vst.R:240-250): among the rows with mean normalized count > 5, ordered by it
    (order(): stable), the nsub positions round(seq(1, L, length = nsub)) (round half to even); 0-based row indices"""
    bm = np.asarray(baseMean, np.float64)
    with np.errstate(invalid="ignore"):
        keep = np.where(bm > 5)[0]
    if keep.size < nsub:
        raise ValueError("less than 'nsub' rows with mean normalized count > 5, \n"
                         "  it is recommended to use varianceStabilizingTransformation directly")
    o = np.argsort(bm[keep], kind="stable")
    L = keep.size
    if nsub == 1:
        pos = np.array([1.0])
    else:
        pos = 1.0 + np.arange(nsub) * ((L - 1) / (nsub - 1))
        pos[-1] = L
    return keep[o[np.rint(pos).astype(np.int64) - 1]]


def getVarianceStabilizedData(dds):
    """R/vst.R:146-193: the transformation that belongs to the object's dispersion function, applied to the normalized
    counts by the engine in one pass.  fitType "local" and "custom" (the caller's trend) take the spline path of :157-183:
    the trend is evaluated at the grid values through the function, i.e. for "local" on the engine.  Returns the n x m
    engine handle."""
    fn = dds.dispersionFunction
    if fn is None or fn.get("fitType") is None:
        raise ValueError("call estimateDispersions before calling getVarianceStabilizedData")
    E = dds.engine
    nf, sf = _norm_source(dds)
    if fn["fitType"] == "parametric":
        a, e = (float(v) for v in fn["coefficients"])                            # asymptDisp, extraPois
        return E.vst_transform(dds.y, nf, "parametric", sizeFactors=sf, asymptDisp=a, extraPois=e)
    if fn["fitType"] == "mean":
        return E.vst_transform(dds.y, nf, "mean", sizeFactors=sf, alpha=float(fn["coefficients"]))
    if fn["fitType"] in ("custom", "local"):
        sfa = sf if sf is not None else E.nf_col_geomeans(nf)                    # :159-165
        xim = float(np.mean(1.0 / np.asarray(sfa, np.float64)))
        rmean, rmax = E.row_stats(dds.y, nf, sizeFactors=sf)
        table = vst_spline_table(fn["coefficients"], float(np.max(rmax)), xim)
        from .engine import spline_eval
        h1, h2 = quantile7(rmean, .95), quantile7(rmean, .999)                   # :175-176
        s1, s2 = (float(spline_eval(table, np.arcsinh(h))) for h in (h1, h2))
        eta = (np.log2(h2) - np.log2(h1)) / (s2 - s1)                            # :177
        xi = np.log2(h1) - eta * s1                                              # :178
        dds.attrs["vst_spline"] = {"table": table, "eta": float(eta), "xi": float(xi), "h1": h1, "h2": h2}
        return E.vst_transform(dds.y, nf, "spline", sizeFactors=sf, table=table, eta=float(eta), xi=float(xi))
    raise ValueError("fitType is not parametric, local or mean")


def _shallow(dds, x=None):
    """the same object (same handles) with fresh mcols / assays / attrs and, optionally, another design"""
    c = DESeqDataSet.__new__(DESeqDataSet)
    c.__dict__.update(dds.__dict__)
    c.mcols, c.assays, c.attrs = {}, {}, {}
    if x is not None:
        c.x = np.asarray(x, np.float64)
        c.xh = dds.engine.design(c.x)
    return c


def _vst_object(obj, engine):
    """a count matrix becomes the `~ 1` object (R/vst.R:116-118, 227-229); an object is copied (same handles, own mcols /
    assays / attrs), so that -- as in R -- the caller's object keeps its factors and its dispersion function"""
    if isinstance(obj, DESeqDataSet):
        c = _shallow(obj)
        c.mcols, c.assays, c.attrs = dict(obj.mcols), dict(obj.assays), dict(obj.attrs)
        if obj.dispersionFunction is not None:
            c.dispersionFunction = dict(obj.dispersionFunction)
        return c, False
    counts = np.asarray(obj)
    return DESeqDataSet(counts, np.ones((counts.shape[1], 1)), engine=engine), True


def _fit_trend(sub, fitType):
    getBaseMeansAndVariances(sub)
    estimateDispersionsGeneEst(sub)
    estimateDispersionsFit(sub, fitType=fitType)
    return sub.dispersionFunction


def varianceStabilizingTransformation(obj, blind=True, fitType="parametric", engine=None, sfType="ratio"):
    """R/vst.R:112-142.  obj: a DESeqDataSet or a count matrix (then `engine` says where it lives).  Size factors are
    estimated (sfType) when the object has neither factors nor a matrix; blind swaps the design for the intercept; with
    blind = False and a dispersion function on the object nothing is fitted (the "frozen" VST).  The dispersion steps run
    on the rows that are not all zero.  Returns a DESeqTransform (for a matrix too: assay() is what R returns) whose `.dds`
    is a copy of the object carrying the factors and the dispersion function used; the argument is left as it was."""
    dds, _ = _vst_object(obj, engine)
    if not dds._sf_given:
        estimateSizeFactors(dds, type=sfType)                                       # :122-124
    fn = dds.dispersionFunction
    if blind or fn is None or fn.get("fitType") is None:                            # :128
        work = _shallow(dds, np.ones((dds.m, 1)) if blind else None)                # :125-127
        getBaseMeansAndVariances(work)
        allZero = work.mcols["allZero"]
        if allZero.all():
            raise ValueError("all genes have zero counts in every sample")
        sub = work if not allZero.any() else work.subset(np.where(~allZero)[0])
        dds.dispersionFunction = _fit_trend(sub, fitType)                           # :129-130
    return DESeqTransform(dds, getVarianceStabilizedData(dds), "vst")


def vst(obj, blind=True, nsub=1000, fitType="parametric", engine=None, sfType="ratio"):
    """R/vst.R:219-267: the trend is estimated on nsub rows spanning the range of the mean normalized count, then the
    transformation is applied to every row.  The argument is left as it was; the DESeqTransform's `.dds` is the copy that
    carries the estimated factors, the dispersion function and attrs["vst_rows"]."""
    dds, matrixIn = _vst_object(obj, engine)
    if dds.n < nsub:
        raise ValueError("less than 'nsub' rows,\n  it is recommended to use varianceStabilizingTransformation directly")
    if not dds._sf_given:
        estimateSizeFactors(dds, type=sfType)                                       # :236-238
    work = _shallow(dds, np.ones((dds.m, 1)) if (blind or matrixIn) else None)      # :231-233
    nf, sf = _norm_source(dds)
    baseMean, _ = dds.engine.row_stats(dds.y, nf, sizeFactors=sf)                   # :239 (unweighted rowMeans)
    idx = vst_subset_rows(baseMean, nsub)                                           # :240-250
    dds.dispersionFunction = _fit_trend(work.subset(idx), fitType)                  # :253-257
    dds.attrs["vst_rows"] = idx
    return DESeqTransform(dds, getVarianceStabilizedData(dds), "vst")               # :261


# ------------------------------------------------------------------ R/rlog.R
SPARSE_WARNING = ("the rlog assumes that data is close to a negative binomial distribution, an assumption\n"
                  "which is sometimes not compatible with datasets where many genes have many zero counts\n"
                  "despite a few very large counts.\n"
                  "In this data, for %s%% of genes with a sum of normalized counts above %s, it was the case\n"
                  "that a single sample's normalized count made up more than %s%% of the sum over all samples.\n"
                  "the threshold for this warning is %s%% of genes.\n"
                  "We recommend instead using the varianceStabilizingTransformation or shifted log.")


def sparseTest(dds, p=.9, t1=100, t2=.1):
    """R/rlog.R:274-287 on the engine's row statistics: rowSums = rowMeans * m, the row maxima"""
    nf, sf = _norm_source(dds)
    rmean, rmx = dds.engine.row_stats(dds.y, nf, sizeFactors=sf)
    rs = np.asarray(rmean, np.float64) * dds.m                                      # :275
    rmx = np.asarray(rmx, np.float64)                                               # :276
    if (rs <= t1).all():                                                            # :277
        return
    big = rs > t1
    total = float(np.mean((rmx[big] / rs[big]) > p))                                # :278-279
    if total > t2:                                                                  # :280
        warnings.warn(SPARSE_WARNING % (round(total, 3) * 100, t1, p * 100, t2 * 100))


def rlogData(dds, intercept=None, betaPriorVar=None):
    """R/rlog.R:172-272.  The fit itself -- fitNbinomGLMs on a design with one coefficient per sample, :249-254 -- is the
    engine's rlog_fit (csrc/rlog.hip on the device, any number of samples); the weighted upper quantile behind the prior
    variance stays the host function.  Returns (n x m engine handle, betaPriorVar, fitted intercept or None)."""
    E = dds.engine
    if dds.mcols.get("dispFit") is None:
        raise ValueError("first estimate dispersion")                               # :173-175
    if dds.has_weights:
        raise NotImplementedError("rlog: observation weights (a weights assay) are not served")
    if intercept is not None:
        intercept = np.asarray(intercept, np.float64).reshape(-1)
        if intercept.size != dds.n:                                                 # :177-181
            raise ValueError("intercept should be as long as the number of rows of object")
    if dds.mcols.get("allZero") is None or dds.mcols.get("baseMean") is None:       # :182-184
        getBaseMeansAndVariances(dds)
    allZero = np.asarray(dds.mcols["allZero"], bool) if intercept is None else ~np.isfinite(intercept)   # :223
    dispFit = np.asarray(dds.mcols["dispFit"], np.float64)
    if np.isnan(dispFit[~allZero]).any():                                           # stopifnot(all(!is.na(dispFit))), :228
        raise ValueError("all(!is.na(mcols(objectNZ)$dispFit)) is not TRUE")
    nf, sf = _norm_source(dds)
    if betaPriorVar is None:                                                        # :233-240
        nz = np.where(~allZero)[0]
        baseMean = np.asarray(dds.mcols["baseMean"], np.float64)[nz]
        logCounts = np.asarray(E.to_numpy(E.vst_transform(dds.y, nf, "log2", sizeFactors=sf, pc=0.5)))[nz]   # :234
        logFoldChangeMatrix = logCounts - np.log2(baseMean + 0.5)[:, None]          # :235
        logFoldChangeVector = np.asarray(logFoldChangeMatrix).flatten(order="F")    # as.numeric(): column-major, :236
        varlogk = 1.0 / baseMean + dispFit[nz]                                      # :237
        betaPriorVar = matchWeightedUpperQuantileForVariance(logFoldChangeVector, np.tile(1.0 / varlogk, dds.m))   # :238-239
    betaPriorVar = float(np.asarray(betaPriorVar, np.float64).reshape(-1)[0]) if np.size(betaPriorVar) == 1 else None
    if betaPriorVar is None:
        raise ValueError("length(betaPriorVar) == 1 is not TRUE")                   # :241
    fit = E.rlog_fit(dds.y, nf, dispFit, betaPriorVar, intercept=intercept, sizeFactors=sf, tol=1e-4, maxit=100, minmu=0.5)
    nbad = int((np.asarray(fit["flag"]) == 2).sum())
    if nbad:
        warnings.warn("%d rows ended the rlog fit with a non-finite coefficient (the rows the reference refits with "
                      "optim, R/fitNbinomGLMs.R:203-207); that refit is not served: the rows are NaN" % nbad)
    dds.mcols["rlogIter"], dds.mcols["rlogConv"] = fit["iter"], np.asarray(fit["iter"]) < 100
    return fit["rlog"], betaPriorVar, (fit["intercept"] if intercept is None else None)


def rlog(obj, blind=True, intercept=None, betaPriorVar=None, fitType="parametric", engine=None, sfType="ratio"):
    """R/rlog.R:108-164.  obj: a DESeqDataSet or a count matrix (then `engine` says where it lives).  Returns a
    DESeqTransform(kind = "rlog") with attrs["betaPriorVar"] and, when no intercept was given, mcols["rlogIntercept"]; the
    argument is left as it was."""
    dds, _ = _vst_object(obj, engine)                                               # :120-125
    if dds.has_weights:
        raise NotImplementedError("rlog: observation weights (a weights assay) are not served")
    if not dds._sf_given:
        estimateSizeFactors(dds, type=sfType)                                       # :126-128
    if intercept is None:
        sparseTest(dds, .9, 100, .1)                                                # :133-135
    if blind or dds.mcols.get("dispFit") is None:                                   # :136
        work = _shallow(dds, np.ones((dds.m, 1)) if blind else None)                # :129-131
        getBaseMeansAndVariances(work)                                              # :138-140
        allZero = np.asarray(work.mcols["allZero"], bool)
        if allZero.all():
            raise ValueError("all genes have zero counts in every sample")
        nz = np.where(~allZero)[0]
        sub = work if nz.size == dds.n else work.subset(nz)                         # the dispersion steps skip all-zero rows
        _fit_trend(sub, fitType)                                                    # :141-142
        dispFit = np.full(dds.n, np.nan)
        dispFit[nz] = np.asarray(sub.mcols["dispFit"], np.float64)
        dds.mcols["dispFit"] = dispFit
        dds.mcols["baseMean"], dds.mcols["allZero"] = work.mcols["baseMean"], allZero
        dds.dispersionFunction = sub.dispersionFunction
    if intercept is not None and np.size(intercept) != dds.n:                       # :144-148
        raise ValueError("intercept should be as long as the number of rows of object")
    handle, bpv, icpt = rlogData(dds, intercept, betaPriorVar)                      # :149
    dt = DESeqTransform(dds, handle, "rlog")
    dt.attrs["betaPriorVar"] = bpv                                                  # :159
    if icpt is not None:
        dt.mcols["rlogIntercept"] = icpt                                            # :160-162
    return dt


rlogTransformation = rlog                                                           # :168


# ------------------------------------------------------------------ R/results.R
class DESeqResults:
    """What results() returns: the six columns baseMean, log2FoldChange, lfcSE, stat, pvalue, padj and metadata(res).  The
    columns stay where the engine made them (HBM on the device engine) until one is asked for: res["padj"]."""
    COLUMNS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue", "padj")
    coef = None                        # results(name = ): the column of the coefficient (what R reads back from the description)
    shown = None                       # lfcShrinkApeglm: the columns R keeps (res[, 1:3] with svalue, res[, c(1:3, 5:6)])

    def __init__(self, tab, priorInfo=None, engine=None):
        self.tab, self.engine = tab, engine
        self.metadata = {}
        self.priorInfo = priorInfo
        self._set = {}                 # columns assigned from the host (padj; `row` of tidy = TRUE)

    @property
    def columns(self):
        if self.shown is not None:
            return list(self.shown)
        return [c for c in ("row",) + self.COLUMNS if c in self._set or (c in self.COLUMNS[:5])]

    @property
    def n(self):
        return int(np.shape(self.tab.resident["baseMean"])[0])

    def __getitem__(self, name):
        if name in self._set:
            v = self._set[name]
            return v() if callable(v) else v
        if name in self.COLUMNS[:5]:
            return self.tab.column(name)
        raise KeyError(name)

    def __setitem__(self, name, value):
        self._set[name] = value if callable(value) else np.asarray(value)

    def __contains__(self, name):
        return name in self.columns

    def to_dict(self):
        return {c: self[c] for c in self.columns}


def _coef_names(dds, ncoef):
    names = dds.attrs.get("coefNames")
    if names is not None and len(names) == ncoef:
        return list(names)
    first_ones = dds.x.shape[1] == ncoef and bool((dds.x[:, 0] == 1).all())
    return ["Intercept" if (k == 0 and first_ones) else "coef%d" % k for k in range(ncoef)]


def resultsNames(dds):
    """resultsNames (R/results.R:619-621): the names of the fitted coefficients -- attrs["coefNames"] when the caller has
    set them (the column names of the model matrix), else Intercept / coef1 / coef2 ..."""
    from .fused import finish
    finish(dds)                      # (an analysis enqueued with wait = False)
    if "beta" not in dds.mcols:
        raise RuntimeError("couldn't find results. you should first run DESeq()")
    return _coef_names(dds, np.shape(dds.mcols["beta"])[1])


def p_adjust(p, method="BH"):
    """stats::p.adjust for the two methods results() is served with: "BH" (NAs left out of n, pmin(1, cummin(n / i * p[o]))[ro])
    and "none"."""
    p0 = np.array(p, np.float64)
    if method == "none":
        return p0
    if method != "BH":
        raise NotImplementedError('p_adjust: method "%s" (served: "BH", "none")' % method)
    nna = ~np.isnan(p0)
    pp = p0[nna]
    n = pp.size
    if n == 0:
        return p0
    o = np.argsort(-pp, kind="stable")
    ro = np.argsort(o, kind="stable")
    i = np.arange(n, 0, -1).astype(np.float64)
    with np.errstate(all="ignore"):
        p0[nna] = np.minimum(1.0, np.minimum.accumulate((n / i) * pp[o]))[ro]
    return p0


def lowess(x, y, f=2.0 / 3.0, iter=3, delta=None):
    """stats::lowess as documented (W. S. Cleveland's algorithm): for every x the ns = clamp(int(f n + 1e-7), 2, n) nearest
    points, tricube weights (1 within 0.001 h, 0 beyond 0.999 h), a weighted local line; `iter` passes of bisquare
    robustness weights from the residuals (6 times their median absolute value); points closer than delta = 0.01
    range(x) to the last fitted one are interpolated linearly.  Returns dict(x, y) sorted by x.  Restated from the
    published algorithm: R's own source is not part of the reference tree, so agreement with R to the last bit is not pinned."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    o = np.argsort(x, kind="stable")
    x, y = x[o], y[o]
    n = x.size
    if n < 2:
        return {"x": x, "y": y.copy()}
    if delta is None:
        delta = 0.01 * (x[-1] - x[0])
    ns = max(2, min(n, int(f * n + 1e-7)))
    ys, rw, res = np.zeros(n), np.ones(n), np.zeros(n)
    rng = x[-1] - x[0]

    def lowest(xs, nleft, nright, userw):
        h = max(xs - x[nleft], x[nright] - xs)
        h9, h1 = 0.999 * h, 0.001 * h
        w = np.zeros(n)
        a = 0.0
        j = nleft
        while j < n:
            r = abs(x[j] - xs)
            if r <= h9:
                w[j] = 1.0 if r <= h1 else (1.0 - (r / h) ** 3) ** 3
                if userw:
                    w[j] *= rw[j]
                a += w[j]
            elif x[j] > xs:
                break
            j += 1
        nrt = j - 1
        if a <= 0.0:
            return False, 0.0
        sl = slice(nleft, nrt + 1)
        w[sl] /= a
        if h > 0.0:
            a = float(np.sum(w[sl] * x[sl]))
            b = xs - a
            c = float(np.sum(w[sl] * (x[sl] - a) ** 2))
            if np.sqrt(c) > 0.001 * rng:
                b /= c
                w[sl] = w[sl] * (b * (x[sl] - a) + 1.0)
        return True, float(np.sum(w[sl] * y[sl]))

    for it in range(iter + 1):
        nleft, nright, last, i = 0, ns - 1, -1, 0
        while True:
            if nright < n - 1:
                d1, d2 = x[i] - x[nleft], x[nright + 1] - x[i]
                if d1 > d2:
                    nleft += 1
                    nright += 1
                    continue
            ok, v = lowest(x[i], nleft, nright, it > 0)
            ys[i] = v if ok else y[i]
            if last < i - 1:
                denom = x[i] - x[last]
                for j in range(last + 1, i):
                    al = (x[j] - x[last]) / denom
                    ys[j] = al * ys[i] + (1.0 - al) * ys[last]
            last = i
            cut = x[last] + delta
            i = last + 1
            while i < n:
                if x[i] > cut:
                    break
                if x[i] == x[last]:
                    ys[i] = ys[last]
                    last = i
                i += 1
            i = max(last + 1, i - 1)
            if last >= n - 1:
                break
        res = y - ys
        if it == iter:
            break
        sc = float(np.sum(np.abs(res))) / n
        ar = np.sort(np.abs(res))
        m1 = n // 2
        cmad = 3.0 * (ar[m1] + ar[n - m1 - 1]) if n % 2 == 0 else 6.0 * ar[m1]
        if cmad < 1e-7 * sc:
            break
        c9, c1 = 0.999 * cmad, 0.001 * cmad
        r = np.abs(res)
        with np.errstate(all="ignore"):         # (cmad = 0: every branch taken is free of the quotient)
            rw = np.where(r <= c1, 1.0, np.where(r <= c9, (1.0 - (r / cmad) ** 2) ** 2, 0.0))
    return {"x": x, "y": ys}


def _seq_length(lo, hi, length):
    """seq(lo, hi, length = length): c(from, from + seq_len(length - 2) * by, to), by = (to - from) / (length - 1)"""
    by = (hi - lo) / (length - 1)
    return np.concatenate([[lo], lo + np.arange(1, length - 1) * by, [hi]])


def pvalueAdjustment(res, independentFiltering=True, filter=None, theta=None, alpha=0.1, pAdjustMethod="BH"):
    """pvalueAdjustment (R/results.R:638-718): independent filtering over a grid of quantiles of the filter statistic, the
    number of rejections per quantile, the choice of the threshold by the lowess rule of :661-692; or the plain adjustment.
    The adjustments run in the engine (csrc/results.hip on the device); the rule over the K counts runs here."""
    E = res.engine
    if pAdjustMethod not in ("BH", "none"):
        raise NotImplementedError('pAdjustMethod "%s": served are "BH" and "none"' % pAdjustMethod)
    if not independentFiltering:
        if pAdjustMethod == "none":
            _realize(res)
            res["padj"] = lambda: np.array(res["pvalue"], copy=True)
        else:
            tab = _run_filtered_p(res, None, None, alpha)                         # :709
            res["padj"] = lambda: tab.padj_column(0)
        return res
    if pAdjustMethod != "BH":
        raise NotImplementedError("independent filtering is served with pAdjustMethod = 'BH' only")
    n = res.n
    if filter is None:
        fvals = res["baseMean"] if theta is None else None                       # (the default theta needs mean(filter == 0))
    else:
        fvals = np.asarray(filter, np.float64)
        if fvals.shape != (n,):
            raise ValueError("length(filter) == nrow(res) is not TRUE")          # :653
    if theta is None:
        lowerQuantile = float(np.mean(fvals == 0))                                # :646-648
        upperQuantile = 0.95 if lowerQuantile < 0.95 else 1.0
        theta = _seq_length(lowerQuantile, upperQuantile, 50)
    theta = np.asarray(theta, np.float64)
    if theta.size <= 1:
        raise ValueError("length(theta) > 1 is not TRUE")                        # :652
    tab = _run_filtered_p(res, None if filter is None else fvals, theta, alpha)   # :654-656, 695
    numRej = np.asarray(tab.numRej, np.float64)
    lo_fit = lowess(theta, numRej, f=1.0 / 5.0)                                   # :661
    if numRej.max() <= 10:
        j = 0
    else:
        pos = numRej > 0
        residual = numRej[pos] - lo_fit["y"][pos]          # (theta ascending: lowess keeps its order)
        maxFit = float(np.max(lo_fit["y"]))
        rmse = float(np.sqrt(np.mean(residual ** 2)))
        thresh = maxFit - rmse
        j = 0
        for bound in (thresh, 0.9 * maxFit, 0.8 * maxFit):                       # :680-691
            hit = np.where(numRej > bound)[0]
            if hit.size:
                j = int(hit[0])
                break
    res["padj"] = lambda: tab.padj_column(j)
    res.metadata.update(filterThreshold=float(tab.cutoffs[j]), filterTheta=float(theta[j]),
                        filterNumRej={"theta": theta, "numRej": np.asarray(tab.numRej).copy()}, alpha=alpha)
    res.metadata["lo.fit"] = lo_fit
    return res


def _cooks_flags(dds, cooksCutoff):
    """cooksOutlier over all n rows, also when the n x m assays cover the non-zero rows only (attrs["nz_rows"])"""
    nz = dds.attrs.get("nz_rows")
    if nz is None or dds.engine.nrow(dds.assays["cooks"]) == dds.n:
        return cooksOutlier(dds, cooksCutoff)
    view = dds.subset(nz)
    view.mcols, view.assays, view.attrs = {"maxCooks": np.asarray(dds.mcols["maxCooks"])[nz]}, dds.assays, dds.attrs
    flags = np.zeros(dds.n, bool)
    flags[nz] = cooksOutlier(view, cooksCutoff)
    return flags


def results(dds, name=None, lfcThreshold=0, altHypothesis="greaterAbs", cooksCutoff=None, independentFiltering=True,
            alpha=0.1, filter=None, theta=None, pAdjustMethod="BH", filterFun=None, test=None, tidy=False, **not_served):
    """results (R/results.R:298-615) for one coefficient: `name` is a name of resultsNames(dds) or a column index and
    defaults to the last coefficient.  cooksCutoff: None = qf(.99, p, m - p), False = no filter, a number = that cutoff.
    The table, the threshold tests and the adjusted p-values of every filter threshold are engine work (one launch chain
    on the device, csrc/results.hip); argument checks, the Cook's flags (core.cooksOutlier) and the choice of the threshold
    stay here.  On a useT analysis (mcols holds tDegreesFreedom, :414) the threshold tests run under Student's t with the
    rows' degrees of freedom.  Not served (NotImplementedError): contrast (see resultsContrasts), addMLE, format, parallel,
    pAdjustMethod other than "BH" / "none"."""
    reasons = {"contrast": "contrasts are served by resultsContrasts(dds, contrasts, ...), one covariance pass for all of them",
               "addMLE": "the MLE column of a beta-prior analysis is not served", "format": "only the table is served",
               "parallel": "the adjustment is global over the genes and runs on one device", "BPPARAM": "see parallel",
               "saveCols": "only the six result columns are served", "listValues": "see contrast", "minmu": "see contrast"}
    for k, v in not_served.items():
        if k not in reasons:
            raise TypeError("results() got an unexpected keyword argument '%s'" % k)
        if not (v is None or v is False or (k == "format" and v == "DataFrame")):
            raise NotImplementedError("results(%s = ): %s" % (k, reasons[k]))
    test, _ = _results_checks(dds, lfcThreshold, altHypothesis, alpha, pAdjustMethod, test)
    beta = np.asarray(dds.mcols["beta"])
    names = _coef_names(dds, beta.shape[1])
    if name is None:
        c = beta.shape[1] - 1                                                    # lastCoefName
    elif isinstance(name, str):
        if name not in names:
            raise ValueError("'%s' is not one of resultsNames(dds): %s" % (name, ", ".join(names)))
        c = names.index(name)
    elif isinstance(name, (int, np.integer)) and 0 <= int(name) < beta.shape[1]:
        c = int(name)
    else:
        raise ValueError("the argument 'name' should be a coefficient name or a column index")   # :403-405
    lfc, se, stat, pvalue = _stored_columns(dds, c, test)
    res = _results_tail(dds, lfc, se, stat, pvalue, lfcThreshold, altHypothesis, cooksCutoff, independentFiltering, alpha,
                        filter, theta, pAdjustMethod, filterFun, tidy)
    res.coef = c
    return res


def _results_checks(dds, lfcThreshold, altHypothesis, alpha, pAdjustMethod, test):
    """the argument checks of results() (R/results.R:326-346, 464-471) that do not depend on the coefficient; returns the
    test that is served and whether a threshold test was asked for"""
    from .fused import finish
    finish(dds)                      # (an analysis enqueued with wait = False)
    if altHypothesis not in ("greaterAbs", "lessAbs", "greater", "less", "greaterAbs2014"):
        raise ValueError("'arg' should be one of greaterAbs, lessAbs, greater, less, greaterAbs2014")
    if np.ndim(lfcThreshold) != 0 or np.ndim(alpha) != 0:
        raise ValueError("lfcThreshold and alpha must have length 1")            # :327-328
    if not lfcThreshold >= 0:
        raise ValueError("lfcThreshold >= 0 is not TRUE")                        # :326
    if not (alpha > 0 and alpha < 1):
        raise ValueError("alpha > 0 & alpha < 1 is not TRUE")                    # :329
    if "beta" not in dds.mcols:
        raise RuntimeError("couldn't find results. you should first run DESeq()")   # :333-335
    if pAdjustMethod not in ("BH", "none"):
        raise NotImplementedError('pAdjustMethod "%s": served are "BH" and "none"' % pAdjustMethod)
    objtest = dds.attrs.get("test")
    if test is None:
        test = objtest                                                           # :336-337
    elif test not in ("Wald", "LRT"):
        raise ValueError("'arg' should be one of Wald, LRT")
    elif test == "LRT" and objtest == "Wald":
        raise ValueError("the LRT requires the user run nbinomLRT or DESeq(dds,test='LRT')")   # :341-343
    if lfcThreshold == 0 and altHypothesis == "lessAbs":
        raise ValueError("when testing altHypothesis='lessAbs', set the argument lfcThreshold to a positive value")   # :344-346
    threshold = not (lfcThreshold == 0 and altHypothesis == "greaterAbs")
    if threshold:
        if test == "LRT":
            raise ValueError("tests of log fold change above or below a theshold must be Wald tests.")   # :465-467
        if altHypothesis == "lessAbs" and dds.attrs.get("betaPrior"):
            raise ValueError("testing altHypothesis='lessAbs' requires setting the DESeq() argument betaPrior=FALSE")   # :469-471
        _student_df(dds)
    return test, threshold


def pt(q, df, lower_tail=True, engine=None):
    """stats::pt(q, df, lower.tail) for real df > 0 in the engine's pinned arithmetic: q an n-vector or
    an n x K matrix, df a number or one value per row.  Accurate in relative terms far into the tail (1e-300 and below); as R's
    pt, NaN for NaN arguments and df <= 0, the normal distribution at df = Inf.  engine: HostEngine() (the default) or a
    DeviceEngine -- the same bits."""
    E = HostEngine() if engine is None else engine
    q = np.asarray(q, np.float64)
    if q.ndim not in (1, 2):
        raise ValueError("q should be a vector or a matrix")
    df = np.ascontiguousarray(np.broadcast_to(np.asarray(df, np.float64), q.shape[:1]))
    r = E.pt(q, df, "lower" if lower_tail else "upper")
    if not isinstance(r, np.ndarray):
        r = E._host(r).numpy()
        r = r.T if r.ndim == 2 else r
    return np.array(r, dtype=np.float64).reshape(q.shape)


def _student_df(dds):
    """the degrees of freedom of a useT analysis, or None: as R/results.R:414, the analysis is on the t distribution when
    mcols holds tDegreesFreedom.  attrs["useT"] without the column is an object from before the column was stored (or a
    hand-made one): there is nothing to evaluate Student's t with"""
    if "tDegreesFreedom" in dds.mcols:
        return np.asarray(dds.mcols["tDegreesFreedom"], np.float64)
    if dds.attrs.get("useT"):
        raise NotImplementedError('attrs["useT"] is set but mcols has no "tDegreesFreedom" column: the Student-t tests need the '
                                  "degrees of freedom nbinomWaldTest(useT = True) stores")
    return None


def _stored_columns(dds, c, test):
    """getCoef / getCoefSE / getStat / getPvalue (R/results.R:1052-1099) of coefficient c"""
    beta, betaSE = np.asarray(dds.mcols["beta"]), np.asarray(dds.mcols["betaSE"])
    lfc, se = beta[:, c], betaSE[:, c]
    if test == "LRT":
        stat, pvalue = dds.mcols["LRTStatistic"], dds.mcols["LRTPvalue"]
    elif "WaldStatistic" in dds.mcols:
        stat, pvalue = np.asarray(dds.mcols["WaldStatistic"])[:, c], np.asarray(dds.mcols["WaldPvalue"])[:, c]
    else:
        with np.errstate(divide="ignore", invalid="ignore"):                     # makeWaldTest (:1101-1118) on an LRT object
            stat = lfc / se
        pvalue = dds.engine.two_sided_normal_p(stat)
    return lfc, se, stat, pvalue


def _results_tail(dds, lfc, se, stat, pvalue, lfcThreshold, altHypothesis, cooksCutoff, independentFiltering, alpha, filter,
                  theta, pAdjustMethod, filterFun, tidy):
    """what results() does with the four columns of a coefficient or of a contrast (R/results.R:520-610): the Cook's mask,
    the replaced rows, the table (launched with the adjustment), pvalueAdjustment, the metadata.  The columns may be host
    arrays or vectors resident in the engine."""
    E = dds.engine
    na_mask = None
    if not (cooksCutoff is False) and "maxCooks" in dds.mcols and "dispModelMatrix" in dds.attrs:
        cut = None if (cooksCutoff is None or cooksCutoff is True) else float(cooksCutoff)     # :524-531
        na_mask = _cooks_flags(dds, cut)                                         # :534-564
    replace = dds.mcols.get("replace")
    if replace is not None:
        with np.errstate(invalid="ignore"):
            replace = np.asarray(replace) == 1                                   # (NA is not TRUE, :568-569)
        if not replace.any():
            replace = None
    if dds.attrs.get("betaPrior"):
        priorInfo = {"type": "normal", "package": "deseq2_amd", "betaPriorVar": dds.attrs.get("betaPriorVar")}   # :579-585
    else:
        priorInfo = {"type": "none", "package": "deseq2_amd"}
    # the table is not launched yet: the adjustment's engine call makes table and adjusted p-values together
    bm = np.asarray(dds.mcols["baseMean"], np.float64)
    threshold = not (lfcThreshold == 0 and altHypothesis == "greaterAbs")
    df = _student_df(dds) if threshold else None                                 # :477-515: pt(., df) for pnorm
    res = DESeqResults(_ResultsPending((lfc, se, stat, pvalue, bm, replace, na_mask, lfcThreshold, altHypothesis), df), priorInfo, E)
    if filterFun is None:
        pvalueAdjustment(res, independentFiltering, filter, theta, alpha, pAdjustMethod)   # :591-593
    else:
        _realize(res)
        res = filterFun(res, filter, alpha, pAdjustMethod)                       # :594-596
    res.metadata["lfcThreshold"] = lfcThreshold                                   # :599
    if tidy:
        res["row"] = np.arange(res.n)                                            # :602-610 (the objects carry no row names)
    return res


class _ResultsPending:
    """the arguments of a table that has not been launched (df: the degrees of freedom of a threshold test under Student's t,
    handed to the engine by keyword)"""

    def __init__(self, args, df=None):
        self.args, self.df = args, df
        self.resident = {"baseMean": args[4]}

    def column(self, name):
        assert name == "baseMean"
        return self.args[4]


def _realize(res):
    if isinstance(res.tab, _ResultsPending):
        res.tab = res.engine.results_table(*res.tab.args, df=res.tab.df)
    return res.tab


def _run_filtered_p(res, filter, theta, alpha):
    """the adjustment over `theta`; for a table not launched yet, table and adjustment in ONE engine call"""
    if isinstance(res.tab, _ResultsPending):
        res.tab = res.engine.results(*res.tab.args, filter=filter, theta=theta, alpha=alpha, df=res.tab.df)
        return res.tab
    return res.engine.filtered_p(res.tab, filter, theta, alpha)


# ------------------------------------------------------------------ contrasts (R/results.R:760-1040, 1146-1201, 1237-1270)
_CONTRAST_FORMS = ("'contrast' vector should be either a character vector of length 3,\n"
                   "a list of length 2 containing character vectors,\n"
                   "or a numeric vector, see the argument description in ?results")


def _contrast_form(contrast):
    """which of R's three forms a contrast is: "character" (a sequence that starts with a str: the factor's name),
    "list" (a sequence of sequences) or "numeric"; anything else is checkContrast's first error (:1147-1151)"""
    if isinstance(contrast, (str, bytes, dict)) or not isinstance(contrast, (list, tuple, np.ndarray)):
        raise ValueError(_CONTRAST_FORMS)
    if len(contrast) > 0 and isinstance(contrast[0], str):
        return "character"
    if len(contrast) > 0 and all(isinstance(e, (list, tuple, np.ndarray)) for e in contrast):
        return "list"
    try:
        np.asarray(contrast, np.float64)
    except (TypeError, ValueError):
        raise ValueError(_CONTRAST_FORMS)
    return "numeric"


def checkContrast(contrast, resNames):
    """checkContrast (R/results.R:1146-1201), every message; returns (form, the contrast as the later steps take it)"""
    form = _contrast_form(contrast)
    if form == "character":
        if len(contrast) != 3:                                                    # :1155-1159
            raise ValueError("'contrast', as a character vector of length 3, should have the form:\n"
                             "contrast = c('factorName','numeratorLevel','denominatorLevel'),\n"
                             "see the manual page of ?results for more information")
        if contrast[1] == contrast[2]:                                            # :1160-1162
            raise ValueError("%s and %s should be different level names" % (contrast[1], contrast[2]))
        return form, tuple(contrast)
    if form == "list":
        contrast = [list(e) for e in contrast]
        if len(contrast) == 1:                                                    # :1167-1169
            contrast = [contrast[0], []]
        if len(contrast) != 2:                                                    # :1170-1174
            raise ValueError("'contrast', as a list, should have length 2, or, if length 1,\n"
                             "an empty vector will be added for the second element.\n"
                             "see the manual page of ?results for more information")
        if not all(isinstance(v, str) for e in contrast for v in e):              # :1175-1178
            raise ValueError("'contrast', as a list of length 2, should have character vectors as elements,\n"
                             "see the manual page of ?results for more information")
        if not all(v in resNames for e in contrast for v in e):                   # :1179-1181
            raise ValueError("all elements of the contrast as a list of length 2 should be elements of 'resultsNames(object)'")
        if set(contrast[0]) & set(contrast[1]):                                   # :1182-1185
            raise ValueError("elements in the contrast list should only appear in the numerator (first element of contrast list)\n"
                             "or the denominator (second element of contrast list), but not both")
        if len(contrast[0]) + len(contrast[1]) == 0:                              # :1186-1188
            raise ValueError("one of the two elements in the list should be a character vector of non-zero length")
        return form, contrast
    c = np.asarray(contrast, np.float64).reshape(-1)
    if c.size != len(resNames):                                                   # :1193-1194
        raise ValueError("numeric contrast vector should have one element for every element of 'resultsNames(object)'")
    if (c == 0).all():                                                            # :1195-1197
        raise ValueError("numeric contrast vector cannot have all elements equal to 0")
    return form, c


def _rnum(v):
    """as.character() of a number as R prints the ones that occur here"""
    v = float(v)
    return "%d" % v if v == int(v) and abs(v) < 1e15 else "%.15g" % v


def _factor_columns(dds, expanded):
    """the columns of the fitted model matrix by (factor, level code): found by position in the matrix
    standard_model_matrix / makeExpandedModelMatrix build from attrs["factors"]"""
    factors = dds.attrs.get("factors")
    numeric = "pass the contrast as a numeric vector over resultsNames(dds) instead"
    if not factors:
        raise ValueError('a character contrast needs dds.attrs["factors"] (the level codes of the design factors): ' + numeric)
    xs, _ = standard_model_matrix(factors)
    if xs.shape != dds.x.shape or not np.array_equal(xs, dds.x):
        raise ValueError('the model matrix of the analysis is not the one attrs["factors"] generates: ' + numeric)
    ncoef = np.shape(dds.mcols["beta"])[1]
    if ncoef != (makeExpandedModelMatrix(factors)[0].shape[1] if expanded else xs.shape[1]):
        raise ValueError('the fitted coefficients are not those of the matrix attrs["factors"] generates: ' + numeric)
    cols, k = {}, 1
    for f, codes in factors.items():
        for lv in range(0 if expanded else 1, int(np.max(codes)) + 1):
            cols[(f, lv)] = k
            k += 1
    return factors, cols


def _contrast_model_matrix(dds):
    """attr(object, "modelMatrix"): the matrix the coefficients were fitted on -- the expanded one on an expanded-matrix
    analysis (R/core.R:1374-1380, R/fitNbinomGLMs.R:319-325)"""
    if dds.attrs.get("betaPrior") and dds.attrs.get("modelMatrixType") == "expanded":
        return makeExpandedModelMatrix(dds.attrs["factors"])[0]
    return np.asarray(dds.x, np.float64)


def resultsContrasts(dds, contrasts, listValues=(1, -1), minmu=0.5, lfcThreshold=0, altHypothesis="greaterAbs", cooksCutoff=None,
                     independentFiltering=True, alpha=0.1, filter=None, theta=None, pAdjustMethod="BH", filterFun=None,
                     test=None, tidy=False, **not_served):
    """results(object, contrast = .) (R/results.R:375-438, 760-1040) for a SEQUENCE of contrasts: a list of DESeqResults,
    one per contrast, in order.  Each contrast is one of R's three forms:
      numeric    a 1-D sequence of numbers, one per element of resultsNames(dds);
      character  (factor, numLevel, denomLevel): factor names a key of dds.attrs["factors"] (the ordered dict of level codes,
                 0 = the reference level, that standard_model_matrix / makeExpandedModelMatrix take), the levels are codes;
      list       one or two sequences of coefficient names, weighted by listValues.
    getContrast re-enters fitBeta once per contrast; here ALL contrasts that need the covariance of the coefficients go
    into ONE engine call (csrc/contrasts.hip on the device: one covariance pass per gene), and a character contrast against
    the reference level is answered from the stored columns (:876-932) with only the all-zero flags from the engine.  Every
    table then takes the tail of results(): Cook's mask, replaced rows, threshold tests, independent filtering, BH.
    metadata["contrast"] is the name R builds (:968-1001).  On a useT analysis the fitted contrasts take
    2 pt(|stat|, tDegreesFreedom, lower.tail = FALSE) (:812-815) and the threshold tests Student's t.  Not served
    (NotImplementedError): addMLE, parallel."""
    reasons = {"addMLE": "the MLE column of a beta-prior analysis is not served",
               "parallel": "all contrasts share one covariance pass per gene on one device", "BPPARAM": "see parallel",
               "format": "only the table is served", "saveCols": "only the six result columns are served"}
    for k, v in not_served.items():
        if k not in reasons:
            raise TypeError("resultsContrasts() got an unexpected keyword argument '%s'" % k)
        if not (v is None or v is False or (k == "format" and v == "DataFrame")):
            raise NotImplementedError("resultsContrasts(%s = ): %s" % (k, reasons[k]))
    test, _ = _results_checks(dds, lfcThreshold, altHypothesis, alpha, pAdjustMethod, test)
    tdf = _student_df(dds)
    lv = np.asarray(listValues, np.float64).reshape(-1)
    if lv.size != 2:
        raise ValueError("length(listValues) == 2 & is.numeric(listValues) is not TRUE")       # :330
    if not (lv[0] > 0 and lv[1] < 0):
        raise ValueError("listValues[1] > 0 & listValues[2] < 0 is not TRUE")                  # :331
    if isinstance(contrasts, (str, bytes, dict)) or not isinstance(contrasts, (list, tuple)):
        raise ValueError("'contrasts' should be a sequence of contrasts")
    E = dds.engine
    resNames = resultsNames(dds)
    expanded = dds.attrs.get("betaPrior") and dds.attrs.get("modelMatrixType") == "expanded"   # isExpanded, :383
    X = _contrast_model_matrix(dds)
    if X.shape[1] != len(resNames):
        raise ValueError("was expecting a model matrix stored as an attribute of the DESeqDataSet")   # :764-766
    m = X.shape[0]
    # cleanContrast for every contrast: `plan` entries are ("pull", column, sign, name, sample mask) or
    # ("fit", numeric contrast, name, sample mask or None)
    plan = []
    for contrast in contrasts:
        form, contrast = checkContrast(contrast, resNames)                        # :420
        if form == "character":
            f, num, den = contrast
            if dds.attrs.get("factors") is not None and f not in dds.attrs["factors"]:
                raise ValueError("%s should be the name of a factor in the colData of the DESeqDataSet" % f)   # :844-846
            factors, cols = _factor_columns(dds, expanded)
            codes = np.asarray(factors[f])
            both = np.isin(codes, [num, den])                                     # contrastAllZeroCharacter, :1237-1243
            name = "%s %s vs %s" % (f, num, den)                                  # :877, :901, :1001
            # (the no-intercept branch, noInterceptPullCoef :861-862, cannot be reached: the matrix `factors` generates always
            #  has its intercept)
            if not expanded:                                                      # case 1, :867-941
                if den == 0:
                    if (f, num) not in cols:
                        raise ValueError("as %s is the reference level, was expecting %s_%s_vs_%s to be present in "
                                         "'resultsNames(object)'" % (den, f, num, den))   # :884-886
                    plan.append(("pull", cols[(f, num)], 1.0, name, both))
                    continue
                if num == 0:
                    if (f, den) not in cols:
                        raise ValueError("as %s is the reference level, was expecting %s_%s_vs_%s to be present in "
                                         "'resultsNames(object)'" % (num, f, den, num))   # :907-909
                    plan.append(("pull", cols[(f, den)], -1.0, name, both))
                    continue
                if (f, num) not in cols or (f, den) not in cols:                  # :937-940
                    raise ValueError("%s and %s should be levels of %s such that %s_%s_vs_0 and %s_%s_vs_0 are contained in "
                                     "'resultsNames(object)'" % (num, den, f, f, num, f, den))
            elif (f, num) not in cols or (f, den) not in cols:                    # case 2, :946-954
                raise ValueError("%s%s and %s%s are expected to be in resultsNames(object)" % (f, num, f, den))
            c = np.zeros(len(resNames))                                           # :997-1000
            c[cols[(f, num)]], c[cols[(f, den)]] = 1.0, -1.0
        elif form == "list":
            l1, l2 = contrast
            n1, n2 = round(float(lv[0]), 3), round(float(lv[1]), 3)               # :978-990
            if l1 and l2:
                n2 = abs(n2)
                name = "%s%s vs %s%s" % ("" if n1 == 1 else _rnum(n1) + " ", "+".join(l1), "" if n2 == 1 else _rnum(n2) + " ",
                                         "+".join(l2))
            elif l1:
                name = "%s%s effect" % ("" if n1 == 1 else _rnum(n1) + " ", "+".join(l1))
            else:
                name = "%s %s effect" % (_rnum(n2), "+".join(l2))
            c = np.zeros(len(resNames))                                           # :991-994
            c[[r in l1 for r in resNames]] = lv[0]
            c[[r in l2 for r in resNames]] = lv[1]
        else:
            c = contrast
            name = ",".join(("+" if v > 0 else "") + _rnum(v) for v in c)         # :969-972
        # contrastAllZeroNumeric (:1245-1270): no rule when all coefficients share a sign; else the samples X binary(c) != 0
        mask = None if ((c >= 0).all() or (c <= 0).all()) else (X @ (c != 0).astype(np.float64)) != 0
        plan.append(("fit", c, name, mask))
    allZero = np.asarray(dds.mcols["allZero"], bool)
    fits = [e for e in plan if e[0] == "fit"]
    pulls = [e for e in plan if e[0] == "pull"]
    fitted = pulled = None
    if fits:                                                                      # getContrast, :760-827, once for all of them
        weights, useWeights = getAndCheckWeights(dds)                             # :787-795
        ln2 = np.log(2.0)
        bpv = np.asarray(dds.attrs.get("betaPriorVar", np.full(len(resNames), 1e6)), np.float64)
        masks = np.array([e[3] if e[3] is not None else np.zeros(m, bool) for e in fits])
        rule = np.array([e[3] is not None for e in fits])
        use_sf = dds.sizeFactors is not None
        fitted = E.contrasts(dds.y, X, None if use_sf else dds.nf, np.asarray(dds.mcols["dispersion"], np.float64),
                             ln2 * np.asarray(dds.mcols["beta"], np.float64), 1.0 / (ln2 ** 2 * bpv),           # :775-777
                             np.column_stack([e[1] for e in fits]), weights, useWeights, minmu, allZero,
                             sample_mask=masks if rule.any() else None, rule_applies=rule if rule.any() else None,
                             sizeFactors=dds.sizeFactors if use_sf else None, df=tdf)
    if pulls:
        pulled = E.contrasts(dds.y, None, None, None, None, None, None, None, False, minmu, allZero,
                             sample_mask=np.array([e[4] for e in pulls]))
    out, kf, kp = [], 0, 0
    for e in plan:
        if e[0] == "fit":
            lfc, se, stat, pvalue = fitted.columns(kf)
            kf += 1
            name = e[2]
        else:
            lfc, se, stat, pvalue = _stored_columns(dds, e[1], test)              # :887-890, :910-913
            if e[2] < 0:
                lfc = -1.0 * lfc                                                  # :916
                if test == "Wald":
                    stat = -1.0 * stat                                            # :917
            lfc, stat, pvalue = E.zero_rule(lfc, stat, pvalue, pulled.flags(kp))  # :1023-1028
            kp += 1
            name = e[3]
        if test == "LRT":                                                         # :1030-1037
            stat, pvalue = dds.mcols["LRTStatistic"], dds.mcols["LRTPvalue"]
        res = _results_tail(dds, lfc, se, stat, pvalue, lfcThreshold, altHypothesis, cooksCutoff, independentFiltering, alpha,
                            filter, theta, pAdjustMethod, filterFun, tidy)
        res.metadata["contrast"] = name
        out.append(res)
    return out


# ------------------------------------------------------------------ lfcShrink (R/lfcShrink.R:145-520)
def _design_from_factors(dds):
    """is(design(dds), "formula") in this mirror: attrs["factors"] is set and dds.x is the matrix standard_model_matrix builds
    from it (the test _factor_columns applies); anything else is a user-supplied matrix"""
    factors = dds.attrs.get("factors")
    if not factors:
        return False
    xs, _ = standard_model_matrix(factors)
    return xs.shape == dds.x.shape and bool(np.array_equal(xs, dds.x))


def _shrink_object(dds, rows):
    """the object nbinomWaldTest(dds, betaPrior = TRUE) works on inside lfcShrink: the rows that are not all zero NOW (objectNZ,
    R/core.R:1351 -- allZero as refitWithoutOutliers left it) over the ORIGINAL counts dds.y, with the dispersions of the
    finished analysis.  The caller's object is not touched."""
    sub = _shallow(dds) if rows is None else dds.subset(rows)
    pick = (lambda v: np.asarray(v)) if rows is None else (lambda v: np.asarray(v)[rows])
    sub.mcols = {k: pick(dds.mcols[k]) for k in ("baseMean", "baseVar", "allZero", "dispersion", "dispFit") if k in dds.mcols}
    sub.attrs = {k: dds.attrs[k] for k in ("weightsOK",) if k in dds.attrs}
    sub.dispersionFunction = dds.dispersionFunction
    return sub


def _shrink_full_rows(dds, sub, rows):
    """buildDataFrameWithNARows: the per-gene columns of the refitted rows back over all n rows (NA elsewhere), next to the
    columns results() reads from the analysis itself (baseMean, allZero, replace, the dispersions)"""
    out = {}
    for k, v in sub.mcols.items():
        v = np.asarray(v)
        if k == "rowsForOptim" or v.shape[:1] != (sub.n,):
            continue
        if rows is None:
            out[k] = v
        else:
            full = np.full((dds.n,) + v.shape[1:], np.nan)
            full[rows] = v
            out[k] = full
    for k in ("baseMean", "baseVar", "allZero", "dispersion", "dispFit", "replace", "weightsFail"):
        if k in dds.mcols:
            out[k] = dds.mcols[k]
    return out


def lfcShrink(dds, coef=None, contrast=None, res=None, type="normal", lfcThreshold=0, quiet=False, **not_served):
    """lfcShrink (R/lfcShrink.R:145-520) with the Normal prior of Love et al. (2014): type = "normal".  NOTE the default: R's is
    type = "apeglm"; "apeglm" and "ashr" delegate to packages whose source is not part of the reference tree and raise
    NotImplementedError here, so "normal" is the default of this mirror.  `coef` is a name of resultsNames(dds) or a column
    index (0-based, as results(name = ) takes it), `contrast` one of the three forms resultsContrasts takes, over the names of
    the EXPANDED model matrix (makeExpandedModelMatrix); one of the two.  Returns `res` (results(dds, name = coef) /
    resultsContrasts(dds, [contrast])[0] when not given) with log2FoldChange and lfcSE -- and, with lfcThreshold > 0, stat,
    pvalue and padj -- replaced by those of the shrunken fit (:318-325); priorInfo carries the prior variance.
    The estimator (:263-316): betaPriorVar = estimateBetaPriorVar over the stored MLE coefficients (the engine's
    beta_prior_var: csrc/beta_prior.hip on the device), standard matrix for `coef`, expanded for `contrast`; then
    nbinomWaldTest(betaPrior = TRUE, betaPriorVar, modelMatrixType) ON ITS DEFAULTS -- no useT, minmu = 0.5, betaTol = 1e-8,
    whatever DESeq() was run with -- on the ORIGINAL counts, also for the rows DESeq() refitted on the replaced counts, over
    the rows that are not all zero as refitWithoutOutliers left that column; then results() on the refitted object.  This is
    what R does (its dds.shr is nbinomWaldTest(dds, ...): counts(dds) are the original counts, mcols(dds)$allZero the updated
    flags), not an oversight of the mirror.
    Two routes, one result: with lfcThreshold == 0 only log2FoldChange and lfcSE of the refit are read, so only the ridge pass
    of fitGLMsWithPrior runs (R/fitNbinomGLMs.R:311-325; the MLE pass, mu, the hat diagonals, Cook's distances, the log
    likelihood and the p-values are skipped) and its coefficients take the tail of results() / resultsContrasts() -- NA on
    the all-zero rows, the nowZero fill, the all-zero rule of a contrast; with lfcThreshold > 0 the whole nbinomWaldTest
    runs and the Cook's mask of the new p-values comes from the refitted object.  The ridge pass does not depend on what is
    skipped: the two give the same log2FoldChange and lfcSE bits.
    A user-supplied matrix (no attrs["factors"], or another matrix than they generate) is served with `coef` only.
    Not served (NotImplementedError): type "apeglm" / "ashr", svalue, returnList, format, saveCols, parallel."""
    import sys
    from .fused import finish
    reasons = {"svalue": "s-values belong to type = 'apeglm' / 'ashr' (see lfcShrinkApeglm)",
               "returnList": "only type = 'apeglm' / 'ashr' return a list (see lfcShrinkApeglm)",
               "format": "only the table is served", "saveCols": "only the six result columns are served",
               "parallel": "the refit runs on one device", "BPPARAM": "see parallel",
               "apeAdapt": "type = 'apeglm' is served by lfcShrinkApeglm", "apeMethod": "type = 'apeglm' is served by lfcShrinkApeglm"}
    for k, v in not_served.items():
        if k not in reasons:
            raise TypeError("lfcShrink() got an unexpected keyword argument '%s'" % k)
        if not (v is None or v is False or (k == "format" and v == "DataFrame") or (k == "apeAdapt" and v is True)
                or (k == "apeMethod" and v == "nbinomCR")):
            raise NotImplementedError("lfcShrink(%s = ): %s" % (k, reasons[k]))
    if not isinstance(dds, DESeqDataSet):
        raise TypeError('is(dds, "DESeqDataSet") is not TRUE')                    # :156
    if res is not None and not isinstance(res, DESeqResults):
        raise ValueError("res should be a DESeqResults object, for GRanges output use 'format'")   # :157-159
    if type not in ("apeglm", "ashr", "normal"):
        raise ValueError("'arg' should be one of apeglm, ashr, normal")          # :160
    finish(dds)                      # (an analysis enqueued with wait = False)
    if "beta" not in dds.mcols:
        raise RuntimeError("first run DESeq() before running lfcShrink()")        # :162-166
    if type != "normal":
        raise NotImplementedError("lfcShrink(type = '%s') delegates to the %s package, whose source is not part of the reference "
                                  "tree: nothing here could pin it.  Served: type = 'normal'%s" % (type, type,
                                  "; the apeglm estimator is served by lfcShrinkApeglm(dds, coef, ...)" if type == "apeglm"
                                  else "; the ashr estimator is served by lfcShrinkAshr(dds, coef / contrast / res, ...)"))
    if dds.attrs.get("betaPrior"):
        raise ValueError("lfcShrink() should be used downstream of DESeq() with betaPrior=FALSE (the default)")   # :170-173
    if np.ndim(lfcThreshold) != 0 or not lfcThreshold >= 0:
        raise ValueError("length(lfcThreshold) == 1 && lfcThreshold >= 0 is not TRUE")   # :174
    names = resultsNames(dds)                                                     # :175
    c = None
    if coef is not None:                                                          # :182-192
        if isinstance(coef, str):
            if coef not in names:
                raise ValueError("coef %in% resultsNamesDDS is not TRUE")
            c = names.index(coef)
        elif isinstance(coef, (int, np.integer)) and not isinstance(coef, bool) and 0 <= int(coef) < len(names):
            c = int(coef)
        else:
            raise ValueError("coef <= length(resultsNamesDDS) is not TRUE")
    if res is None:                                                               # :193-204
        if coef is not None:
            res = results(dds, name=c)
        elif contrast is not None:
            if _contrast_form(contrast) == "numeric":
                raise ValueError("for type='normal' and numeric contrast, user must provide 'res' object")   # :197-199
            res = resultsContrasts(dds, [contrast])[0]
        else:
            raise ValueError("one of coef or contrast required if 'res' is missing")
    if np.isnan(np.asarray(res["lfcSE"], np.float64)).all():
        raise ValueError("lfcShrink requires standard errors, use default fitType")   # :207-208
    if "dispersion" not in dds.mcols:
        raise RuntimeError("type='normal' and 'apeglm' require dispersion estimates, first call estimateDispersions()")   # :211-213
    if res.n != dds.n:
        raise ValueError("all(rownames(dds) == rownames(res)) is not TRUE")      # :214 (the objects carry no row names)
    if coef is None and contrast is None:
        raise ValueError("type='normal' requires either 'coef' or 'contrast' be specified.")   # :223-225
    if not quiet:                                                                 # :231-235
        print("using 'normal' for LFC shrinkage, the Normal prior from Love et al (2014).", file=sys.stderr)
    formula = _design_from_factors(dds)
    if not formula and contrast is not None:
        raise ValueError("user-supplied design matrix supports shrinkage only with 'coef'")   # :243-245, :256-258
    if coef is not None and contrast is not None:
        raise ValueError("missing(coef) | missing(contrast) is not TRUE")        # :262
    factors = dds.attrs.get("factors") if formula else None
    if contrast is None:
        modelMatrixType = "standard"                                              # :269-270
    else:
        modelMatrixType = "expanded"                                              # :273-287
        xe, enames = makeExpandedModelMatrix(factors)
        if _contrast_form(contrast) == "character":
            if len(contrast) != 3:
                raise ValueError("length(contrast) == 3 is not TRUE")
            if contrast[0] not in factors:
                raise ValueError("contrast[1] %in% names(colData(dds)) is not TRUE")
            if not all(lv in set(np.asarray(factors[contrast[0]]).tolist()) for lv in contrast[1:]):
                raise ValueError("all(contrast[2:3] %in% levels(colData(dds)[[contrast[1]]])) is not TRUE")
        checkContrast(contrast, enames)                                           # :286
    # estimateBetaPriorVar (:289) over the stored MLE coefficients of the standard matrix -- on an LRT analysis as well
    E = dds.engine
    from .native import coef_factor_codes
    allZero = np.asarray(dds.mcols["allZero"], bool)
    if factors is not None:
        cf = coef_factor_codes(factors)
    else:
        cf = np.array([0 if nm == "Intercept" else 1 for nm in _coef_names(dds, len(names))], np.int32)
    dispFit = dds.mcols.get("dispFit")
    if dispFit is None:
        dispFit = np.full(dds.n, np.mean(np.asarray(dds.mcols["dispersion"])[~allZero]))   # R/core.R:1637-1640
    betaPriorVar = E.beta_prior_var(np.asarray(dds.mcols["beta"], np.float64), np.asarray(dds.mcols["baseMean"], np.float64),
                                    np.asarray(dispFit, np.float64), allZero, cf,
                                    prior_coef_factor=coef_factor_codes(factors, expanded=True) if contrast is not None else None)
    betaPriorVar = np.asarray(betaPriorVar, np.float64)
    if betaPriorVar.size == 0:
        raise ValueError("length(betaPriorVar) > 0 is not TRUE")                  # :290
    rows = np.where(~allZero)[0] if allZero.any() else None
    sub = _shrink_object(dds, rows)
    if lfcThreshold > 0:                                                          # :293-298
        nbinomWaldTest(sub, betaPrior=True, betaPriorVar=betaPriorVar, modelMatrixType=modelMatrixType, factors=factors)
        sub.mcols.pop("MLE_beta", None)
    else:
        # only the ridge pass of fitGLMsWithPrior (R/fitNbinomGLMs.R:311-325): nothing else of the refit is read below
        if (betaPriorVar == 0).any():
            raise ValueError("beta prior variances are equal to zero for some variables")
        weights, useWeights = getAndCheckWeights(sub)
        fit = fitNbinomGLMs(sub, lam=1.0 / betaPriorVar, modelMatrix=xe if contrast is not None else None,
                            weights=weights, useWeights=useWeights, want_hat=False)
        sub.mcols.update(beta=fit["betaMatrix"], betaSE=fit["betaSE"])
        sub.attrs.update(betaPrior=True, betaPriorVar=betaPriorVar, test="Wald", modelMatrixType=modelMatrixType,
                         factors=factors, useT=False)
    shr = _shallow(dds)
    shr.mcols = _shrink_full_rows(dds, sub, rows)
    shr.assays = sub.assays
    shr.attrs = {k: v for k, v in sub.attrs.items() if k not in ("prefit", "prefit_for")}
    if rows is not None:
        shr.attrs["nz_rows"] = rows
    if contrast is not None:
        shr.attrs["coefNames"] = list(enames)
    elif dds.attrs.get("coefNames") is not None:
        shr.attrs["coefNames"] = dds.attrs["coefNames"]
    shr.dispersionFunction = dds.dispersionFunction
    if contrast is None:                                                          # :309-316
        res_shr = results(shr, name=c, lfcThreshold=lfcThreshold)
    else:
        res_shr = resultsContrasts(shr, [contrast], lfcThreshold=lfcThreshold)[0]
    out = DESeqResults(res.tab, None, res.engine)
    out.metadata = dict(res.metadata)
    out._set = dict(res._set)
    change = ("log2FoldChange", "lfcSE", "stat", "pvalue", "padj") if lfcThreshold > 0 else ("log2FoldChange", "lfcSE")   # :318-322
    for col in change:                                                            # :323-325
        out[col] = (lambda r=res_shr, k=col: r[k])
    out.metadata["lfcThreshold"] = lfcThreshold                                   # :497
    out.priorInfo = {"type": "normal", "package": "deseq2_amd", "betaPriorVar": betaPriorVar}   # :498-505
    return out


# ------------------------------------------------------------------ R/lfcShrink.R:328-440, 489-528: apeglm
APEGLM_CITATION = ("using 'apeglm' for LFC shrinkage. If used in published research, please cite:\n"
                   "    Zhu, A., Ibrahim, J.G., Love, M.I. (2018) Heavy-tailed prior distributions for\n"
                   "    sequence count data: removing the noise and preserving large differences.\n"
                   "    Bioinformatics. https://doi.org/10.1093/bioinformatics/bty895")
QNORM_975 = 1.959963984540054


def svalue(lfsr):
    """apeglm::svalue as R/lfcShrink.R:523-528 restates it: sort with NA last, cumulative mean, rank with ties "first".  On
    the host, in numpy, on both engines (R's cumsum is sequential, and so is numpy.cumsum)."""
    from . import apeglm_host
    return apeglm_host.svalue(lfsr)


_svalue = svalue                       # (lfcShrinkApeglm has an argument of that name)


class _ColumnsTab:
    """the table of a DESeqResults whose columns are host arrays"""

    def __init__(self, cols):
        self.resident = cols

    def column(self, name):
        return self.resident[name]


def apeglm_prior_scale(mle, floor=1e-6):
    """The adaptive scale of the apeglm prior from mle = (estimate, standard error) on the natural-log scale (n x 2), over the
    rows where both are finite: the marginal-likelihood estimate of the variance A of a Normal prior, D_i ~ N(0, A + S_i^2)
    (Efron and Morris), i.e. the root of sum_i (D_i^2 - S_i^2 - A) / (S_i^2 + A)^2 = 0 by the fixed point
    A <- sum w_i (D_i^2 - S_i^2) / sum w_i, w_i = 1 / (S_i^2 + A)^2, sums by math.fsum; S = min(max(sqrt(A), floor), 1).
    The library's own statement of the estimator: agreement with the package's routine is not pinned."""
    from . import apeglm_host
    mle = np.asarray(mle, np.float64)
    if mle.ndim != 2 or mle.shape[1] != 2:
        raise ValueError("mle is an n x 2 matrix: estimate, standard error")
    return apeglm_host.prior_scale(mle[:, 0], mle[:, 1], floor=floor)


def apeglm(Y, x, param, coef, mle=None, threshold=None, weights=None, offset=None, prior_control=None, init=None, engine=None):
    """apeglm::apeglm for the negative binomial likelihood as lfcShrink calls it (R/lfcShrink.R:393-396; DESIGN.md section
    22): Y n x m counts (a matrix or an engine handle), x the m x p design, param the n dispersions, coef the 0-based
    coefficient, mle (n x 2, natural log: estimate and standard error of `coef`) for the adaptive prior scale, threshold on
    the natural-log scale, weights n x m, offset n x m (natural log; None = 0).  prior_control: dict with no_shrink (list
    of columns, [0]), prior_mean 0, prior_scale (from mle when given, else 1), prior_df (1), prior_no_shrink_mean 0,
    prior_no_shrink_scale (15).  init: n x p second start (natural log).  Returns dict(map n x p, sd n x p, fsr n, svalue n,
    thresh n (with a threshold), interval n x 2, diag dict(iter, conv, start, objective), prior_control).
    The estimator is the package's as its paper and lfcShrink's documentation state it; the optimiser, the choice between two
    modes and the prior-scale routine are the library's own, and agreement with the package's numbers is not pinned."""
    x = np.asarray(x, np.float64)
    p = x.shape[1]
    pc = {"no_shrink": [0], "prior_mean": 0.0, "prior_scale": None, "prior_df": 1.0, "prior_no_shrink_mean": 0.0,
          "prior_no_shrink_scale": 15.0}
    for k, v in (prior_control or {}).items():
        if k not in pc:
            raise ValueError("prior_control has no element '%s'" % k)
        pc[k] = v
    if pc["prior_mean"] != 0 or pc["prior_no_shrink_mean"] != 0:
        raise NotImplementedError("apeglm: a prior mean other than 0 is not served")
    if not (isinstance(coef, (int, np.integer)) and 0 <= int(coef) < p):
        raise ValueError("coef is a column of x (0-based)")
    no_shrink = np.zeros(p, bool)
    no_shrink[list(pc["no_shrink"])] = True
    if no_shrink[coef]:
        raise ValueError("coef is among the columns that are not shrunk")
    if pc["prior_scale"] is None:
        pc["prior_scale"] = apeglm_prior_scale(mle) if mle is not None else 1.0
    E = engine if engine is not None else HostEngine()
    nf = 1.0 if offset is None else E.vexp(np.asarray(offset, np.float64))
    n = Y.shape[0] if hasattr(Y, "shape") else Y.n
    if np.ndim(nf) == 0:
        nf = np.ones(x.shape[0])
    fit = E.apeglm_fit(Y, x, nf if np.ndim(nf) == 2 else None, np.broadcast_to(np.asarray(param, np.float64), (n,)), int(coef),
                       no_shrink, float(pc["prior_scale"]), float(pc["prior_df"]), float(pc["prior_no_shrink_scale"]),
                       weights=weights, init=init, threshold=threshold, sizeFactors=nf if np.ndim(nf) == 1 else None)
    return _apeglm_fields(fit, int(coef), threshold, pc)


def _apeglm_fields(fit, coef, threshold, pc):
    mc, sc = fit["map"][:, coef], fit["sd"][:, coef]
    out = {"map": fit["map"], "sd": fit["sd"], "fsr": fit["fsr"], "svalue": svalue(fit["fsr"]),
           "interval": np.stack([mc - QNORM_975 * sc, mc + QNORM_975 * sc], axis=1),
           "diag": {"iter": fit["iter"][np.arange(mc.size), np.nan_to_num(fit["start"]).astype(int)], "iter_by_start": fit["iter"],
                    "conv": fit["conv"], "start": fit["start"], "objective": fit["objective"]},
           "prior_control": dict(pc)}
    if threshold is not None:
        out["thresh"] = fit["thresh"]
    return out


def lfcShrinkApeglm(dds, coef, res=None, lfcThreshold=0, svalue=False, returnList=False, apeAdapt=True, quiet=False, **not_served):
    """lfcShrink(type = "apeglm") (R/lfcShrink.R:156-219, 328-440, 489-518): MAP fold changes under a Cauchy prior with the
    posterior SD of the Laplace approximation, per gene on the engine (csrc/apeglm.hip on the device).
    `coef` is a name of resultsNames(dds) or a column index (0-based, as results(name = ) takes it).  Returns `res`
    (results(dds, name = coef) when not given) with log2FoldChange = log2(e) map and lfcSE = log2(e) sd, columns
    baseMean, log2FoldChange, lfcSE, pvalue, padj -- or, with svalue = TRUE or lfcThreshold > 0, baseMean, log2FoldChange,
    lfcSE, svalue --, metadata["lfcThreshold"], metadata["description"] and priorInfo with prior_control; with
    returnList, (res, fit).  The fit runs on the ORIGINAL counts with the stored dispersions, offsets from sizeFactors or
    normalizationFactors and the weights assay as given; the second start of the search is log(2) times the stored MLE
    coefficients.  apeAdapt = False runs with prior scale 1 and needs only dispersions (:176-180).
    The optimiser, the choice of mode and the prior-scale routine are the library's own: agreement with the apeglm package's
    numbers is not pinned.  Not served (NotImplementedError): apeMethod other than "nbinomCR", format, saveCols, parallel."""
    import sys
    from .fused import finish
    reasons = {"format": "only the table is served", "saveCols": "only the result columns are served",
               "parallel": "the fit runs on one device", "BPPARAM": "see parallel",
               "apeMethod": "only the default, the negative binomial likelihood with the stored dispersions, is served"}
    for k, v in not_served.items():
        if k not in reasons:
            raise TypeError("lfcShrinkApeglm() got an unexpected keyword argument '%s'" % k)
        if not (v is None or v is False or (k == "format" and v == "DataFrame") or (k == "apeMethod" and v == "nbinomCR")):
            raise NotImplementedError("lfcShrinkApeglm(%s = ): %s" % (k, reasons[k]))
    if not isinstance(dds, DESeqDataSet):
        raise TypeError('is(dds, "DESeqDataSet") is not TRUE')                    # :156
    if res is not None and not isinstance(res, DESeqResults):
        raise ValueError("res should be a DESeqResults object, for GRanges output use 'format'")   # :157-159
    finish(dds)                      # (an analysis enqueued with wait = False)
    fitted = "beta" in dds.mcols
    if not fitted and apeAdapt:
        raise RuntimeError("first run DESeq() before running lfcShrink()")        # :162-166
    if dds.attrs.get("betaPrior"):
        raise ValueError("lfcShrink() should be used downstream of DESeq() with betaPrior=FALSE (the default)")   # :170-173
    if np.ndim(lfcThreshold) != 0 or not lfcThreshold >= 0:
        raise ValueError("length(lfcThreshold) == 1 && lfcThreshold >= 0 is not TRUE")   # :174
    names = resultsNames(dds) if fitted else _coef_names(dds, dds.p)             # :175-180
    if coef is None:
        raise ValueError("!missing(coef) is not TRUE")                            # :340
    if isinstance(coef, str):                                                     # :182-192
        if coef not in names:
            raise ValueError("coef %in% resultsNamesDDS is not TRUE")
        c = names.index(coef)
    elif isinstance(coef, (int, np.integer)) and not isinstance(coef, bool) and 0 <= int(coef) < len(names):
        c = int(coef)
    else:
        raise ValueError("coef <= length(resultsNamesDDS) is not TRUE")
    coefAlpha = names[c]
    # (what apeglm itself refuses: the coefficient is among the columns that are not shrunk; and what is served)
    if c == 0:
        raise ValueError("coef is the intercept, which is not shrunk")
    if dds.p > 16:
        raise NotImplementedError("lfcShrinkApeglm: %d design columns (at most 16 are served)" % dds.p)
    if res is None and fitted:                                                    # :193-195
        res = results(dds, name=c)
    elif res is None:
        # :176-180 "we can run apeglm without running nbinomWaldTest()": there are no results to start from, so the table
        # is baseMean and NA columns, which the fit fills
        na = np.full(dds.n, np.nan)
        res = DESeqResults(_ColumnsTab({"baseMean": np.asarray(dds.mcols.get("baseMean", na), np.float64), "log2FoldChange": na,
                                        "lfcSE": na, "stat": na, "pvalue": na}), {"type": "none", "package": "deseq2_amd"}, dds.engine)
        res["padj"] = na
        res.coef = c
    # (:207-208 reads res$lfcSE; on the route without a Wald test the table above has none by construction, and the fit
    # needs none with apeAdapt = FALSE, so the stop is made only where a Wald test ran)
    if fitted and np.isnan(np.asarray(res["lfcSE"], np.float64)).all():
        raise ValueError("lfcShrink requires standard errors, use default fitType")   # :207-208
    if "dispersion" not in dds.mcols:
        raise RuntimeError("type='normal' and 'apeglm' require dispersion estimates, first call estimateDispersions()")   # :211-213
    if res.n != dds.n:
        raise ValueError("all(rownames(dds) == rownames(res)) is not TRUE")      # :214 (the objects carry no row names)
    if apeAdapt and res.coef != c:                                                # :342-347
        raise ValueError("'coef' should specify same coefficient as in results 'res'")
    if not quiet:                                                                 # :349-352
        print(APEGLM_CITATION, file=sys.stderr)
    E = dds.engine
    LN2 = float.fromhex("0x1.62e42fefa39efp-1")                                  # log(2)
    LOG2E = float.fromhex("0x1.71547652b82fep+0")                                # log2(exp(1))
    disps = np.asarray(dds.mcols["dispersion"], np.float64)                       # :361
    mle = None
    if apeAdapt:                                                                  # :373-377
        mle = LN2 * np.stack([np.asarray(res["log2FoldChange"], np.float64), np.asarray(res["lfcSE"], np.float64)], axis=1)
    apeT = None
    if lfcThreshold > 0:                                                          # :383-389
        if not quiet:
            print("computing FSOS 'false sign or small' s-values (T=%s)" % _r_round3(lfcThreshold), file=sys.stderr)
        svalue = True
        apeT = LN2 * lfcThreshold
    pc = {"no_shrink": [0], "prior_mean": 0.0, "prior_scale": apeglm_prior_scale(mle) if mle is not None else 1.0,
          "prior_df": 1.0, "prior_no_shrink_mean": 0.0, "prior_no_shrink_scale": 15.0}
    no_shrink = np.zeros(dds.p, bool)
    no_shrink[0] = True
    init = LN2 * np.asarray(dds.mcols["beta"], np.float64) if fitted else None
    # :354-372, :393-396: the original counts, offsets log(sizeFactors) or log(normalizationFactors), the weights assay
    fit = E.apeglm_fit(dds.y, dds.x, None if dds.sizeFactors is not None else dds.nf, disps, c, no_shrink, pc["prior_scale"],
                       pc["prior_df"], pc["prior_no_shrink_scale"], weights=dds.weights_h if dds.has_weights else None,
                       init=init, threshold=apeT, sizeFactors=dds.sizeFactors)
    fit = _apeglm_fields(fit, c, apeT, pc)
    if fit["map"].shape[0] != dds.n:
        raise RuntimeError("nrow(fit$map) == nrow(dds) is not TRUE")              # :418
    conv = fit["diag"]["conv"]                                                    # :419-422
    if not (conv[~np.isnan(conv)] == 0).all() and not quiet:
        print("some rows did not converge in finding the MAP", file=sys.stderr)
    out = DESeqResults(res.tab, None, res.engine)
    out.metadata = dict(res.metadata)
    out._set = dict(res._set)
    out.coef = c
    out["log2FoldChange"] = LOG2E * fit["map"][:, c]                              # :423
    out["lfcSE"] = LOG2E * fit["sd"][:, c]                                        # :424
    spaces = coefAlpha.replace("_", " ")
    desc = {"baseMean": "mean of normalized counts for all samples",
            "log2FoldChange": "log2 fold change (MAP): " + spaces,                 # :425
            "lfcSE": "posterior SD: " + spaces}                                   # :426
    if svalue:                                                                    # :427-437
        if lfcThreshold > 0:
            out["svalue"] = _svalue(fit["thresh"])
            desc["svalue"] = "FSOS s-value (T=%s): %s" % (_r_round3(lfcThreshold), spaces)
        else:
            out["svalue"] = fit["svalue"]
            desc["svalue"] = "s-value: " + spaces
        out.shown = ("baseMean", "log2FoldChange", "lfcSE", "svalue")
    else:                                                                         # :439
        desc["pvalue"], desc["padj"] = "Wald test p-value: " + spaces, "BH adjusted p-values"
        out.shown = ("baseMean", "log2FoldChange", "lfcSE", "pvalue", "padj")
    out.metadata["description"] = desc
    out.metadata["lfcThreshold"] = lfcThreshold                                   # :497
    out.priorInfo = {"type": "apeglm", "package": "deseq2_amd", "prior_control": fit["prior_control"]}   # :498-507
    return (out, fit) if returnList else out                                      # :514-518


def _r_round3(v):
    """round(v, 3) as paste0 prints it"""
    return "%g" % round(float(v), 3)


# ------------------------------------------------------------------ R/lfcShrink.R:442-486, 489-518: ashr
ASHR_CITATION = ("using 'ashr' for LFC shrinkage. If used in published research, please cite:\n"
                 "    Stephens, M. (2016) False discovery rates: a new deal. Biostatistics, 18:2.\n"
                 "    https://doi.org/10.1093/biostatistics/kxw041")


def _on_host(v):
    """a column where an engine made it -> a float64 host array"""
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    return np.asarray(v, np.float64)


def _fitted_g(fit, c):
    K = int(fit["K"][c])
    return {"pi": np.array(fit["pi"][c, :K]), "mean": np.zeros(K), "sd": np.array(fit["sd"][c, :K])}


def ash(betahat, sebetahat, lfcThreshold=None, engine=None, maxit=100):
    """ashr::ash(betahat, sebetahat, mixcompdist = "normal", method = "shrink") as lfcShrink calls it (R/lfcShrink.R:458-459;
    DESIGN.md section 23): betahat / sebetahat two vectors of n -- or two n x C matrices of C independent columns, fitted in
    one batch.  A row is kept when betahat is finite and sebetahat finite and positive; the others take no part in the fit
    and come back NaN; no kept row: ValueError.  The prior is sum_k pi_k N(0, sd_k^2) on ashr's documented sqrt(2) grid,
    no point mass, uniform prior on the weights.  Returns dict(fitted_g = dict(pi, mean (0), sd) -- a list of C with
    matrices --, result = dict(betahat, sebetahat, NegativeProb, PositiveProb, lfsr, svalue, lfdr (0: no point mass),
    PosteriorMean, PosteriorSD and, with lfcThreshold = T, le_T = P(beta <= T | data) and gt_mT = P(beta > -T | data), each its
    own one-tail sum -- R forms 1 - cdf and loses the small tail, this does not), loglik, iter, flag (0 converged, 1 maxit,
    2 no acceptable step)).
    The estimator is the package's as its paper (Stephens 2017) and the call state it; the optimiser is the library's own
    sequential quadratic programme.  The package's numbers, its optimiser and its treatment of excluded rows are unpinned."""
    E = engine if engine is not None else HostEngine()
    b, s = np.asarray(betahat, np.float64), np.asarray(sebetahat, np.float64)
    if b.shape != s.shape or b.ndim not in (1, 2):
        raise ValueError("betahat and sebetahat are two vectors of one length, or two n x C matrices")
    if lfcThreshold is not None and not (np.ndim(lfcThreshold) == 0 and lfcThreshold >= 0):
        raise ValueError("lfcThreshold is one number that is not negative")
    fit = E.ash_fit(b, s, threshold=None if lfcThreshold is None else float(lfcThreshold), maxit=maxit)
    C = 1 if b.ndim == 1 else b.shape[1]
    shape = (lambda v: _on_host(v)[0]) if b.ndim == 1 else (lambda v: np.ascontiguousarray(_on_host(v).T))
    result = {"betahat": b, "sebetahat": s}
    for k in ("NegativeProb", "PositiveProb", "lfsr", "PosteriorMean", "PosteriorSD") + (("le_T", "gt_mT") if lfcThreshold is not None else ()):
        result[k] = shape(fit[k])
    lf = result["lfsr"]
    result["svalue"] = svalue(lf) if b.ndim == 1 else np.column_stack([svalue(lf[:, c]) for c in range(C)])
    result["lfdr"] = np.where(np.isnan(lf), np.nan, 0.0)
    g = [_fitted_g(fit, c) for c in range(C)]
    one = b.ndim == 1
    return {"fitted_g": g[0] if one else g, "result": result, "loglik": float(fit["loglik"][0]) if one else np.array(fit["loglik"]),
            "iter": int(fit["iter"][0]) if one else np.array(fit["iter"]), "flag": int(fit["flag"][0]) if one else np.array(fit["flag"])}


def _contrast_batch(contrast):
    """a LIST whose elements are contrasts (numeric vectors, (factor, level code, level code), lists of names), as distinct from
    ONE contrast in list form (one or two sequences of names)"""
    if not isinstance(contrast, list) or not contrast:
        return None
    if not all(isinstance(e, (list, tuple, np.ndarray)) for e in contrast):
        return None
    if all(all(isinstance(v, str) for v in e) for e in contrast):
        return None
    return list(contrast)


def _res_handle(res, name):
    """the column of a results table where it lies: an engine handle, or the host array it was assigned from"""
    if name in res._set:
        return res[name]
    return _realize(res).resident[name]


def lfcShrinkAshr(dds, coef=None, contrast=None, res=None, lfcThreshold=0, svalue=False, returnList=False, quiet=False,
                  **not_served):
    """lfcShrink(type = "ashr") (R/lfcShrink.R:156-209, 442-518): adaptive shrinkage of the log2 fold changes and their
    standard errors of a results table -- posterior mean and posterior SD under a scale mixture of zero-mean normals fitted
    to all rows (csrc/ash.hip on the device).  Both columns are on the log2 scale and nothing is converted.
    `res` is results(dds, name = coef) for `coef` (a name of resultsNames(dds) or a 0-based column), resultsContrasts(dds,
    [contrast])[0] for `contrast` (one of its three forms), or as given -- with `res`, coef and contrast are ignored.  A LIST
    of contrasts (or of results tables) is served in one batch and returns a list, equal to one call each.
    Returns `res` with log2FoldChange = PosteriorMean and lfcSE = PosteriorSD (engine handles until one is asked for), columns
    baseMean, log2FoldChange, lfcSE, pvalue, padj -- or, with svalue = TRUE or lfcThreshold > 0, baseMean, log2FoldChange,
    lfcSE, svalue (the s-values of lfsr; with lfcThreshold = T > 0 of P(beta <= T) where the posterior mean is positive and
    P(beta > -T) elsewhere, :478-485, each tail summed on its own) --, metadata["lfcThreshold"], metadata["description"] and
    priorInfo with fitted_g; with returnList, (res, fit), fit as core.ash returns it.  Rows whose estimate or standard error is
    NA (all-zero genes) take no part in the fit and come back NaN.
    The ashr package's numbers, its optimiser and its treatment of excluded rows are unpinned.  Not served
    (NotImplementedError): format, saveCols, parallel, and the arguments R passes on to ashr::ash (mixcompdist, method,
    pointmass, df, ...)."""
    import sys
    from .fused import finish
    reasons = {"format": "only the table is served", "saveCols": "only the result columns are served",
               "parallel": "the fit runs on one device", "BPPARAM": "see parallel",
               "mixcompdist": "only the normal mixture is served", "method": "only method = 'shrink' is served",
               "pointmass": "no point mass is served", "df": "only the normal likelihood is served",
               "prior": "only the uniform prior on the weights is served", "mode": "only mode 0 is served",
               "gridmult": "only gridmult = sqrt(2) is served", "mixsd": "only the documented grid is served",
               "optmethod": "the optimiser is the library's own", "outputlevel": "the outputs are fixed"}
    for k, v in not_served.items():
        if k not in reasons:
            raise TypeError("lfcShrinkAshr() got an unexpected keyword argument '%s'" % k)
        if not (v is None or v is False or (k == "format" and v == "DataFrame") or (k == "mixcompdist" and v == "normal")
                or (k == "method" and v == "shrink")):
            raise NotImplementedError("lfcShrinkAshr(%s = ): %s" % (k, reasons[k]))
    if not isinstance(dds, DESeqDataSet):
        raise TypeError('is(dds, "DESeqDataSet") is not TRUE')                    # :156
    many = isinstance(res, list) or (res is None and _contrast_batch(contrast) is not None)
    for r in (res if isinstance(res, list) else [res]):
        if r is not None and not isinstance(r, DESeqResults):
            raise ValueError("res should be a DESeqResults object, for GRanges output use 'format'")   # :157-159
    finish(dds)                      # (an analysis enqueued with wait = False)
    if "beta" not in dds.mcols:
        raise RuntimeError("first run DESeq() before running lfcShrink()")        # :162-166
    if dds.attrs.get("betaPrior"):
        raise ValueError("lfcShrink() should be used downstream of DESeq() with betaPrior=FALSE (the default)")   # :170-173
    if np.ndim(lfcThreshold) != 0 or not lfcThreshold >= 0:
        raise ValueError("length(lfcThreshold) == 1 && lfcThreshold >= 0 is not TRUE")   # :174
    names = resultsNames(dds)                                                     # :175
    c = None
    if coef is not None:                                                          # :182-192
        if isinstance(coef, str):
            if coef not in names:
                raise ValueError("coef %in% resultsNamesDDS is not TRUE")
            c = names.index(coef)
        elif isinstance(coef, (int, np.integer)) and not isinstance(coef, bool) and 0 <= int(coef) < len(names):
            c = int(coef)
        else:
            raise ValueError("coef <= length(resultsNamesDDS) is not TRUE")
    if res is None:                                                               # :193-204
        if coef is not None:
            tabs = [results(dds, name=c)]
        elif contrast is not None:
            tabs = resultsContrasts(dds, _contrast_batch(contrast) or [contrast])
        else:
            raise ValueError("one of coef or contrast required if 'res' is missing")
    else:
        tabs = list(res) if many else [res]
        if not tabs:
            raise ValueError("one of coef or contrast required if 'res' is missing")
    E = dds.engine
    cols = []
    for r in tabs:
        if r.n != dds.n:
            raise ValueError("all(rownames(dds) == rownames(res)) is not TRUE")  # (the objects carry no row names)
        b, s = _res_handle(r, "log2FoldChange"), _res_handle(r, "lfcSE")
        if np.isnan(_on_host(s)).all():
            raise ValueError("lfcShrink requires standard errors, use default fitType")   # :207-208
        cols.append((b, s))
    if not quiet:                                                                 # :452-454
        print(ASHR_CITATION, file=sys.stderr)
    T = float(lfcThreshold)
    fit = E.ash_fit([b for b, _ in cols], [s for _, s in cols], threshold=T if T > 0 else None)   # :456-459, :480-483
    if (np.asarray(fit["flag"]) != 0).any() and not quiet:
        print("ash: the iteration for the mixture weights did not converge in some column", file=sys.stderr)
    if T > 0:                                                                     # :477
        if not quiet:
            print("computing FSOS 'false sign or small' s-values (T=%s)" % _r_round3(lfcThreshold), file=sys.stderr)
        svalue = True
    outs = []
    for j, r in enumerate(tabs):
        tab = _realize(r)
        resident = dict(tab.resident)
        for k in ("log2FoldChange", "lfcSE", "pvalue"):          # (columns assigned from the host go where the others lie)
            if k in r._set:
                resident[k] = r._set[k]
        resident["log2FoldChange"], resident["lfcSE"] = fit["PosteriorMean"][j], fit["PosteriorSD"][j]   # :460-461
        out = DESeqResults(ResultColumns(resident, _on_host), None, r.engine)
        out.metadata = dict(r.metadata)
        out._set = {k: v for k, v in r._set.items() if k not in ("log2FoldChange", "lfcSE", "pvalue")}
        out.coef = r.coef
        words = r.metadata["contrast"] if "contrast" in r.metadata else (names[r.coef].replace("_", " ") if r.coef is not None else "")
        desc = {"baseMean": "mean of normalized counts for all samples",
                "log2FoldChange": "log2 fold change (MMSE): " + words,           # :462
                "lfcSE": "posterior SD: " + words}                                # :463
        if svalue:                                                                # :469-486, :490-494
            if T > 0:
                def sv(j=j):
                    pm = _on_host(fit["PosteriorMean"][j])
                    with np.errstate(invalid="ignore"):
                        return _svalue(np.where(pm > 0, _on_host(fit["le_T"][j]), _on_host(fit["gt_mT"][j])))   # :484-485
            else:
                def sv(j=j):
                    return _svalue(_on_host(fit["lfsr"][j]))                      # :472
            out["svalue"] = _Once(sv)
            desc["svalue"] = "s-value: " + words
            out.shown = ("baseMean", "log2FoldChange", "lfcSE", "svalue")
        else:                                                                     # :474
            desc["pvalue"], desc["padj"] = "Wald test p-value: " + words, "BH adjusted p-values"
            out.shown = ("baseMean", "log2FoldChange", "lfcSE", "pvalue", "padj")
        out.metadata["description"] = desc
        out.metadata["lfcThreshold"] = lfcThreshold                               # :497
        g = _fitted_g(fit, j)
        out.priorInfo = {"type": "ashr", "package": "deseq2_amd", "fitted_g": g}   # :498-509
        if returnList:                                                            # :514-518
            result = {k: _on_host(fit[k][j]) for k in ("NegativeProb", "PositiveProb", "lfsr", "PosteriorMean", "PosteriorSD")
                      + (("le_T", "gt_mT") if T > 0 else ())}
            result["svalue"] = _svalue(result["lfsr"])
            result["lfdr"] = np.where(np.isnan(result["lfsr"]), np.nan, 0.0)
            outs.append((out, {"fitted_g": g, "result": result, "loglik": float(fit["loglik"][j]), "iter": int(fit["iter"][j]),
                               "flag": int(fit["flag"][j])}))
        else:
            outs.append(out)
    return outs if many else outs[0]


class _Once:
    """a column made on the first request and kept"""

    def __init__(self, make):
        self.make, self.value = make, None

    def __call__(self):
        if self.value is None:
            self.value = self.make()
        return self.value


# ------------------------------------------------------------------ R/helper.R:70-132
UNMIX_COR_WARNING = ("some columns of 'pure' are highly correlated (>.99 after VST),\n"
                     "  may result in instabilty of unmix(). visually inspect correlations of 'pure'")


class NamedMatrix(np.ndarray):
    """a host matrix that carries dimnames: rownames / colnames are lists of names or None"""
    rownames = colnames = None

    def __array_finalize__(self, obj):
        self.rownames, self.colnames = getattr(obj, "rownames", None), getattr(obj, "colnames", None)


def _named(a, rownames=None, colnames=None):
    out = np.asarray(a, np.float64).view(NamedMatrix)
    out.rownames, out.colnames = rownames, colnames
    return out


def _colnames_of(a):
    names = getattr(a, "colnames", None)
    if names is None:
        names = getattr(a, "columns", None)
    return None if names is None else [str(v) for v in names]


def _r_stopifnot(ok, expr):
    if not ok:
        raise ValueError("%s is not TRUE" % expr)


def unmix(x, pure, alpha=None, shift=None, power=1, format="matrix", quiet=False, engine=None):
    """R/helper.R:70-132.  x: the n x m samples to unmix -- normalized counts or TPMs as a host matrix, an engine handle, or the
    DESeqTransform that normalized_counts() returns (it stays resident on a device engine); pure: the n x k pure components, a
    host matrix.  alpha: the dispersion of a negative binomial fit (the asymptotic or mean value of the trend); shift: for TPMs;
    exactly one of them.  Returns mix, m x k with rows summing to 1 (format = "matrix"), or dict(mix, cor, fitted)
    (format = "list").  Column names of pure and x (attributes colnames or columns) carry through.  `quiet` is accepted: there is
    no progress bar.  The fits are the engine's unmix_fit (csrc/unmix.hip on the device): R's objective, box and start, the
    library's own deterministic optimiser in place of optim's L-BFGS-B."""
    if format not in ("matrix", "list"):                                             # :72
        raise ValueError("'arg' should be one of 'matrix', 'list'")
    if alpha is None:
        _r_stopifnot(shift is not None, "!missing(shift)")                           # :73
    if shift is None:
        _r_stopifnot(alpha is not None, "!missing(alpha)")                           # :74
    _r_stopifnot(shift is None or alpha is None, "missing(shift) | missing(alpha)")  # :75
    _r_stopifnot(power in (1, 2), "power %in% 1:2")                                  # :76
    xnames = _colnames_of(x)
    if isinstance(x, DESeqTransform):
        E = x.engine if engine is None else engine
        handle = x.handle
    else:
        E = HostEngine() if engine is None else engine
        handle = x if hasattr(x, "ld") else np.asarray(x, np.float64)
        if isinstance(handle, np.ndarray) and handle.ndim != 2:
            raise ValueError("x should be a matrix")
    pnames = _colnames_of(pure)
    pure = np.asarray(pure, np.float64)
    if pure.ndim != 2:
        raise ValueError("pure should be a matrix")
    nrow_x = handle.shape[0] if isinstance(handle, np.ndarray) else E.nrow(handle)
    _r_stopifnot(nrow_x == pure.shape[0], "nrow(x) == nrow(pure)")                   # :77
    _r_stopifnot(pure.shape[1] > 1, "ncol(pure) > 1")                                # :78
    if shift is None:
        _r_stopifnot(alpha > 0, "alpha > 0")                                         # :88
        al = float(alpha)
        v = lambda q: (2 * np.arcsinh(np.sqrt(al * q)) - np.log(al) - np.log(4)) / np.log(2)    # :90
    else:
        _r_stopifnot(shift > 0, "shift > 0")                                         # :101
        sh = float(shift)
        v = lambda q: np.log(q + sh)                                                 # :103
    with np.errstate(all="ignore"):
        pure_cor = np.corrcoef(v(pure), rowvar=False)                                # :91, :104
        np.fill_diagonal(pure_cor, 0.0)
        if (pure_cor > .99).any():                                                   # :92, :105
            warnings.warn(UNMIX_COR_WARNING)
    if pure.shape[1] > 16:
        raise NotImplementedError("unmix: %d pure components (at most 16 are served)" % pure.shape[1])
    fit = E.unmix_fit(handle, pure, alpha=None if alpha is None else float(alpha), shift=None if shift is None else float(shift),
                      power=int(power), maxit=200)                                   # :96-99, :109-112
    from . import unmix_host
    mix = _named(unmix_host.mix_from_p(fit["p"]), xnames, pnames)                    # :115-118
    if format == "matrix":
        return mix
    fitted = pure @ np.asarray(mix).T                                                # :123
    xh = np.asarray(E.to_numpy(handle), np.float64) if not isinstance(handle, np.ndarray) else handle
    cor = np.empty(xh.shape[1])
    with np.errstate(all="ignore"):
        for i in range(xh.shape[1]):                                                 # diag(cor(., .)), :124-129
            cor[i] = np.corrcoef(v(xh[:, i]), v(fitted[:, i]))[0, 1]
    return {"mix": mix, "cor": cor, "fitted": _named(fitted, None, xnames)}


# ------------------------------------------------------------------ R/plots.R:239-291, dist(t(assay(vsd)))
PLOTPCA_INTGROUP_STOP = "the argument 'intgroup' should specify columns of colData(dds)"


class PCAData(dict):
    """plotPCA(returnData = TRUE): the columns of R's data frame in its order, by name -- "PC<a>", "PC<b>", "group", the
    intgroup columns, "name" --; attrs["percentVar"] is attr(d, "percentVar")"""

    def __init__(self, columns, percentVar):
        super().__init__(columns)
        self.attrs = {"percentVar": percentVar}


def _transform_of(obj, what):
    if not isinstance(obj, DESeqTransform):
        raise TypeError("%s takes what vst(), rlog(), normTransform() or normalized_counts() return" % what)
    return obj.engine, obj.handle


def rowVars(obj):
    """matrixStats::rowVars(assay(obj)) of a transform (R/plots.R:245): the n variances on the host; the matrix stays where
    the engine keeps it (csrc/explore.hip on the device)"""
    E, h = _transform_of(obj, "rowVars")
    return E.row_vars(h)[1]


def sampleDists(obj):
    """as.matrix(dist(t(assay(obj)))), method "euclidean": the m x m sample-to-sample distances on the host, from the
    engine's all-pairs sums over every gene (csrc/explore.hip on the device).  dist's rescaling of
    sums with NA terms is not mirrored: a NaN in a sample gives NaN against every other sample."""
    E, h = _transform_of(obj, "sampleDists")
    return E.pair_sums(h, "dist")


def pca(obj, ntop=500):
    """prcomp(t(assay(obj)[select, ])) with select = order(rowVars, decreasing = TRUE)[seq_len(min(ntop, n))]
    (R/plots.R:245-254): dict(select (0-based), sdev, x (m x min(m, k) scores), percentVar).  The variances, the order and
    the m x m Gram matrix of the centred selection are the engine's; LAPACK's symmetric eigen-solver on the host turns the
    Gram matrix into the components, on the sample side whatever k is.  The sign of a component (arbitrary in R) is fixed:
    its score of largest magnitude is positive.  A selected row with a non-finite variance stops as prcomp does."""
    from . import explore_host
    E, h = _transform_of(obj, "pca")
    if int(ntop) < 1:
        raise ValueError("ntop should be at least 1")
    tv = E.top_var(h, int(ntop))
    if not np.isfinite(tv["selVar"]).all():
        raise ValueError(explore_host.PRCOMP_STOP)
    G = E.pair_sums(h, "gram", rows=tv["rows"], centre=tv["centre"])
    out = {"select": tv["select"]}
    out.update(explore_host.pca_from_gram(G, len(tv["select"])))
    return out


def plotPCA(obj, intgroup="condition", ntop=500, returnData=True, pcsToUse=(1, 2)):
    """R/plots.R:239-291 with returnData = TRUE: the data frame behind the plot as a PCAData.  intgroup names entries of
    attrs["factors"] of the transform or of the object it came from (level codes per sample); group is the factor itself,
    or the levels pasted with ":" when more than one is given; name: attrs["colnames"] when present, else "sample1" ...
    There is no plotting layer: returnData = False is not served."""
    import sys
    print("using ntop=%s top features by variance" % _rnum(ntop), file=sys.stderr)                    # :242
    E, h = _transform_of(obj, "plotPCA")
    pcs = [int(v) for v in np.atleast_1d(pcsToUse)]
    if len(pcs) != 2:
        raise ValueError("pcsToUse should name two components")
    p = pca(obj, ntop=ntop)                                                                          # :245-254
    intgroup = [intgroup] if isinstance(intgroup, str) else list(intgroup)
    factors = obj.attrs.get("factors") or obj.dds.attrs.get("factors") or {}
    if not all(g in factors for g in intgroup):                                                      # :256-258
        raise ValueError(PLOTPCA_INTGROUP_STOP)
    r = p["x"].shape[1]
    if min(pcs) < 1 or max(pcs) > r:
        raise ValueError("pcsToUse should lie within 1 .. %d" % r)
    m = p["x"].shape[0]
    cols = {g: np.asarray(factors[g]) for g in intgroup}                                             # :260
    if len(intgroup) > 1:                                                                            # :263-267
        group = np.array([":".join(str(cols[g][j]) for g in intgroup) for j in range(m)])
    else:
        group = cols[intgroup[0]]
    names = obj.attrs.get("colnames") or obj.dds.attrs.get("colnames") or ["sample%d" % (j + 1) for j in range(m)]
    d = {"PC%d" % pcs[0]: p["x"][:, pcs[0] - 1].copy(), "PC%d" % pcs[1]: p["x"][:, pcs[1] - 1].copy(), "group": group}
    d.update(cols)
    d["name"] = list(names)
    out = PCAData(d, p["percentVar"][[pcs[0] - 1, pcs[1] - 1]])                                      # :270-278
    if not returnData:
        raise NotImplementedError("plotPCA: there is no plotting layer; returnData = True returns the data frame")
    return out


# ------------------------------------------------------------------ R/helper.R:187-216, 291-391; R/methods.R:1-29; R/plots.R:365-411
COLLAPSE_WARNING = ("\n\n  Warning! collapseReplicates only sums columns of the 'counts' assay.\n"
                    "  Other assays are dropped from output, and must be manually combined,\n"
                    "  as it is not unambiguous how to combine non-count assays.\n")
COUNTS_REPLACED_WARNING = ("there are no assays named 'replaceCounts', using original.\n"
                           "calling DESeq() will replace outliers if they are detected and store this assay.")
COUNTS_NORMALIZED_STOP = "first calculate size factors, add normalizationFactors, or set normalized=FALSE"
PLOTCOUNTS_INTGROUP_STOP = "all variables in 'intgroup' must be columns of colData"
FPKM_NO_LENGTH_STOP = ('fpkm needs feature lengths: an n x m handle assays["avgTxLength"] or the n-vector mcols["basepairs"] '
                       "(there are no rowRanges in this mirror)")


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def _factor_levels(labels, levels=None):
    """factor(labels) followed by droplevels(): (level names, code per label).  Without `levels` they are sort(unique(labels))
    as factor() orders them: numerically when every label is a number (bool excluded), else every label is taken as
    as.character() of itself (numbers as R prints them) and the strings sort by code point (R's sort follows the session's
    collation; the C locale's is used here).  With `levels` (levels(groupby) of an existing factor) that order is kept and
    the levels without a label are dropped."""
    labels = list(labels)
    if levels is None:
        if all(_is_number(v) for v in labels):
            keys = labels
            lev = sorted(set(float(v) for v in labels))
            names = [_rnum(v) for v in lev]
            index = {v: c for c, v in enumerate(lev)}
            codes = [index[float(v)] for v in keys]
        else:
            keys = [_rnum(v) if _is_number(v) else str(v) for v in labels]
            names = sorted(set(keys))
            index = {v: c for c, v in enumerate(names)}
            codes = [index[v] for v in keys]
        return names, np.asarray(codes, np.int64)
    names = [_rnum(v) if _is_number(v) else str(v) for v in levels]
    index = {v: c for c, v in enumerate(names)}
    keys = [_rnum(v) if _is_number(v) else str(v) for v in labels]
    if any(k not in index for k in keys):
        raise ValueError("groupby holds a label that is not among its levels (NA in R)")
    codes = np.asarray([index[k] for k in keys], np.int64)
    used = sorted(set(codes.tolist()))                                               # droplevels, :198
    remap = {c: i for i, c in enumerate(used)}
    return [names[c] for c in used], np.asarray([remap[c] for c in codes.tolist()], np.int64)


def collapseReplicates(dds, groupby, run=None, renameCols=True, levels=None):
    """R/helper.R:187-216 on either engine: the object with one column per level of groupby, its counts the sums of the
    level's columns (the engine's collapse_columns: csrc/count_helpers.hip on the device, where the matrix stays).
    groupby: m labels; levels: see _factor_levels, which also states how mixed numeric and string labels are ordered.
    The result is object[, colsToKeep] for the first column of each level: the rows of x, every attrs["factors"] code vector
    and the size factors (when the object carries real ones) are subset to them; mcols and dispersionFunction are kept as R
    keeps rowData; attrs["colnames"] are the levels (renameCols) or the kept columns' names; attrs["runsCollapsed"] pastes
    `run` per level.  A normalization-factor matrix, weights and every entry of assays are dropped with R's warning (after
    the length check on groupby).  An object without a size-factor vector counts as carrying the matrix: from_device
    called without sizeFactors= holds only its nf_r and so warns, whatever that matrix was built from.  `levels` is beyond
    R's signature: R carries them inside the factor groupby, here they come beside the labels.  R's stopifnot()s come as
    ValueError; a level whose sum exceeds the largest integer raises ValueError naming it (R: NA from
    mode<-, then the closing stopifnot fails)."""
    E = dds.engine
    groupby = list(groupby)
    _r_stopifnot(len(groupby) == dds.m, "length(groupby) == ncol(object)")           # :199, ahead of the warning: a refused call says one thing
    if dds.sizeFactors is None or dds.has_weights or dds.assays:                      # :190-197
        warnings.warn(COLLAPSE_WARNING)
    names, codes = _factor_levels(groupby, levels)                                   # :188, :198
    g = len(names)
    order = np.argsort(codes, kind="stable")                                         # sp <- split(seq(along = groupby), groupby), :200
    members = order.astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=g))]).astype(np.int32)
    y, status = E.collapse_columns(dds.y, members, offsets)                          # :201-202
    if status:
        c = E.collapse_overflow_group(dds.y, members, offsets)
        raise ValueError("collapseReplicates: the sum of the columns of level '%s' exceeds the largest integer (%d): "
                         "NA in R" % (names[c if c is not None else 0], 2 ** 31 - 1))
    keep = members[offsets[:-1]].astype(np.int64)                                    # colsToKeep, :203
    out = DESeqDataSet.__new__(DESeqDataSet)                                         # object[, colsToKeep], :204-206
    out.n, out.m, out.engine = dds.n, g, E
    out.x = np.ascontiguousarray(dds.x[keep])
    out.counts_host = None
    out.y = y
    out.has_weights, out.weights_h = False, None
    out.xh = E.design(out.x)
    out.mcols, out.assays, out.attrs = dict(dds.mcols), {}, {}
    out.dispersionFunction = None if dds.dispersionFunction is None else dict(dds.dispersionFunction)
    real = dds._sf_given and dds.sizeFactors is not None
    _install_size_factors(out, np.asarray(dds.sizeFactors, np.float64)[keep] if real else np.ones(g))
    out._sf_given = bool(real)
    if dds.attrs.get("factors") is not None:
        out.attrs["factors"] = type(dds.attrs["factors"])((k, np.asarray(v)[keep]) for k, v in dds.attrs["factors"].items())
    if run is not None:                                                              # :207-210
        run = list(run)
        _r_stopifnot(len(groupby) == len(run), "length(groupby) == length(run)")
        out.attrs["runsCollapsed"] = [",".join(str(run[j]) for j in members[offsets[c]:offsets[c + 1]]) for c in range(g)]
    if renameCols:                                                                   # :211-213
        out.attrs["colnames"] = list(names)
    elif dds.attrs.get("colnames") is not None:
        out.attrs["colnames"] = [dds.attrs["colnames"][j] for j in keep]
    before = sum(int(v) for v in E.col_sums(dds.y))                                  # :214, on the engine's exact column sums
    after = sum(int(v) for v in E.col_sums(out.y))
    _r_stopifnot(before == after, "sum(as.numeric(assay(object))) == sum(as.numeric(assay(collapsed)))")
    return out


def _library_sizes(dds, robust):
    """library.sizes of fpm (R/helper.R:385-389): colSums(k) -- the engine's exact int64 sums, each rounded once to double
    --, or sizeFactors * exp(mean(log(colSums(k)))) in the library's log / exp with the mean as the sequential sum in sample
    order over m (as xim_size_factors states its mean): host arithmetic over m numbers"""
    E = dds.engine
    cs = np.asarray(E.col_sums(dds.y), np.int64).astype(np.float64)
    if not robust:
        return cs
    lg = E.vlog(cs)
    mean = np.cumsum(lg)[-1] / cs.size
    return np.asarray(dds.sizeFactors, np.float64) * E.vexp(np.array([mean]))[0]


def fpm(dds, robust=True):
    """R/helper.R:378-391 on either engine: 1e6 * sweep(k, 2, library.sizes, "/") as a DESeqTransform of kind "fpm" (the
    matrix stays where the engine keeps it).  robust: the library sizes are sizeFactors * exp(mean(log(colSums(k)))),
    estimated on a copy when the object has no size factors; not used when assays["avgTxLength"] is present."""
    noAvgTxLen = "avgTxLength" not in dds.assays                                     # :380
    work = dds
    if robust and noAvgTxLen and not (dds._sf_given and dds.sizeFactors is not None):         # :381-383, on a copy
        work = estimateSizeFactors(_shallow(dds))
    lib = _library_sizes(work, bool(robust and noAvgTxLen))                          # :385-389
    return DESeqTransform(dds, dds.engine.fpm_transform(dds.y, lib, "fpm"), "fpm")   # :390


def fpkm(dds, robust=True):
    """R/helper.R:291-323 on either engine, as a DESeqTransform of kind "fpkm".  assays["avgTxLength"] (an n x m engine
    handle) takes precedence: 1e3 * fpm / avgTxLength over the plain column sums, then -- robust -- divided by the
    median-ratio size factors of that matrix (estimateSizeFactorsForMatrix); else mcols["basepairs"]: 1e3 * sweep(fpm, 1,
    basepairs, "/").  There are no rowRanges in this mirror: with neither, ValueError."""
    E = dds.engine
    if "avgTxLength" in dds.assays:                                                  # :293-302
        lib = _library_sizes(dds, False)
        ex = E.fpm_transform(dds.y, lib, "fpkm_txlen", txlen=dds.assays["avgTxLength"])
        if robust:
            sf = E.size_factors(ex, type="ratio")                                    # :296
            ex = E.vst_transform(ex, None, "normalized", sizeFactors=sf["sizeFactors"])      # :297
        return DESeqTransform(dds, ex, "fpkm")
    if dds.mcols.get("basepairs") is None:                                           # :303
        raise ValueError(FPKM_NO_LENGTH_STOP)
    bp = np.asarray(dds.mcols["basepairs"], np.float64).reshape(-1)
    if bp.size != dds.n:
        raise ValueError('mcols["basepairs"] should hold one length per row')
    work = dds
    if robust and not (dds._sf_given and dds.sizeFactors is not None):               # fpm(object, robust), :292
        work = estimateSizeFactors(_shallow(dds))
    lib = _library_sizes(work, bool(robust))
    return DESeqTransform(dds, E.fpm_transform(dds.y, lib, "fpkm_basepairs", basepairs=bp), "fpkm")    # :322


def counts(dds, normalized=False, replaced=False):
    """counts.DESeqDataSet (R/methods.R:1-29): a DESeqTransform over the count handle (kind "counts": assay() gives the
    integer matrix) or, normalized, what normalized_counts returns -- of assays["replaceCounts"] when replaced and DESeq()
    stored it, else with R's warning of the original counts."""
    src = dds
    if replaced:                                                                     # :7-14
        if "replaceCounts" in dds.assays:
            src = _shallow(dds)
            src.mcols, src.assays, src.attrs = dds.mcols, dds.assays, dds.attrs
            src.y = dds.assays["replaceCounts"]
        else:
            warnings.warn(COUNTS_REPLACED_WARNING)
    if not normalized:                                                               # :18-19
        return DESeqTransform(dds, src.y, "counts")
    if dds.sizeFactors is None:                                                      # :21-22 (normalization factors)
        return normalized_counts(src)
    if not dds._sf_given or np.isnan(np.asarray(dds.sizeFactors, np.float64)).any():          # :23-24
        raise ValueError(COUNTS_NORMALIZED_STOP)
    return normalized_counts(src)                                                    # :26


def plotCounts(dds, gene, intgroup="condition", normalized=True, transform=True, returnData=True, replaced=False, pc=None):
    """R/plots.R:365-411 with returnData = TRUE: dict(count = counts(dds, normalized, replaced)[gene, ] + pc, then the
    intgroup columns from attrs["factors"]).  gene: a 0-based row index; pc: 0.5 when transform else 0 unless given.  Only
    the one row is computed (take_rows first).  There is no plotting layer: returnData = False is not served."""
    ok = isinstance(gene, (int, np.integer)) and not isinstance(gene, (bool, np.bool_)) and 0 <= int(gene) < dds.n
    _r_stopifnot(ok, "length(gene) == 1 & (is.numeric(gene) & (gene >= 1 & gene <= nrow(dds)))")     # :372
    intgroup = [intgroup] if isinstance(intgroup, str) else list(intgroup)
    factors = dds.attrs.get("factors") or {}
    if not all(v in factors for v in intgroup):                                      # :373
        raise ValueError(PLOTCOUNTS_INTGROUP_STOP)
    if not returnData:
        raise NotImplementedError("plotCounts: there is no plotting layer; returnData = True returns the data frame")
    if pc is None:                                                                   # :381-383
        pc = 0.5 if transform else 0
    work = dds
    if not dds._sf_given:                                                            # :385-387
        work = estimateSizeFactors(_shallow(dds))
        work.attrs, work.assays = dds.attrs, dds.assays
    row = _shallow(work)                                                             # counts(...)[gene, ], :388
    row.n = 1
    E = dds.engine
    src = work.assays["replaceCounts"] if replaced and "replaceCounts" in work.assays else work.y
    row.y = E.take_rows(src, np.array([int(gene)]))
    row.assays = {"replaceCounts": row.y} if replaced and "replaceCounts" in work.assays else {}
    if work.sizeFactors is None:
        row.nf = E.take_rows(work.nf, np.array([int(gene)]))
    cnts = np.asarray(counts(row, normalized=normalized, replaced=replaced).assay(), np.float64).reshape(-1)
    out = {"count": cnts + pc}                                                       # :401, :411
    out.update((v, np.asarray(factors[v])) for v in intgroup)
    return out
