"""Engines: where the n x m matrices of one analysis live and who runs the three native
routines on them.

The host-side mirror of the reference's R callers (core.py, fit_nbinom_glms.py) is written
once against this small interface.  n-vectors and n x p matrices are always host numpy
arrays (they are what R keeps in mcols()); n x m matrices are opaque handles:

  HostEngine    handles are numpy arrays in R orientation (genes x samples); every call
                goes through the host-pointer C ABI (dsq_fit_*), i.e. exactly what the
                .Call shim does -- upload, kernels, download.  Constructed with the module
                providing fitBeta/fitDisp/fitDispGrid, so the parity tests can run the very
                same host code over the CPU oracle.
  DeviceEngine  handles are gene-major torch CUDA tensors resident in HBM; calls go through
                dsq_fit_*_dev on the current stream.  Y / nf / weights are uploaded and
                transposed once, mu-hat produced by fitBeta is consumed in place by fitDisp
                (SURVEY 8f-2).  torch is used for memory, streams and the O(n*m)
                elementwise glue (row gathers, clamps); the fits are the HIP kernels.
"""
import threading

import numpy as np

_PROF_LOCK = threading.Lock()


class Launched(dict):
    """Results of a kernel that has been LAUNCHED: n x m device handles are in the dict at once; the per-gene
    host arrays arrive (one device-to-host copy + stream sync) the first time one of them is read.  A caller
    that launches its next kernel before touching the host arrays overlaps its own host code with the GPU."""

    def __init__(self, ready, fetch):
        super().__init__(ready)
        self._fetch = fetch

    def _materialize(self):
        if self._fetch is not None:
            f, self._fetch = self._fetch, None
            super().update(f())

    def __getitem__(self, k):
        if not super().__contains__(k):
            self._materialize()
        return super().__getitem__(k)

    def get(self, k, default=None):
        if not super().__contains__(k):
            self._materialize()
        return super().get(k, default)

    def __contains__(self, k):
        self._materialize()
        return super().__contains__(k)

    def items(self):
        self._materialize()
        return super().items()

    def keys(self):
        self._materialize()
        return super().keys()


class LaunchedVector:
    """an n-vector still on the device; .host() copies it (once)"""

    def __init__(self, fetch):
        self._fetch, self._v = fetch, None

    def host(self):
        if self._fetch is not None:
            self._v, self._fetch = self._fetch(), None
        return self._v


def _gram_rank(G, tol=1e-7):
    """qr()$rank of the matrices A whose Gram matrices A'A are stacked in G (n, p, p), as R computes it: LINPACK
    dqrdc2's limited column pivoting -- going through the columns in order, a column counts when the norm of its part
    orthogonal to the columns already counted is at least tol (1e-7, qr()'s default) times ITS OWN original norm (so
    rescaling a column never changes its decision), and an exactly zero column never counts.  Evaluated on the Gram
    matrix (a Cholesky factorisation that skips the rejected columns); the squared threshold 1e-14 is a hundred
    roundings of a Gram entry."""
    G = np.asarray(G, np.float64)
    n, p, _ = G.shape
    d0 = np.einsum("nii->ni", G)
    C = np.zeros((n, p, p))                      # row k: <q_k, a_j> for every column j; zero when column k was rejected
    rank = np.zeros(n, dtype=np.int64)
    for j in range(p):
        r = d0[:, j] - (C[:, :, j] ** 2).sum(axis=1)
        ok = (d0[:, j] > 0) & (r >= (tol * tol) * d0[:, j])
        num = G[:, j, :] - np.einsum("nk,nkj->nj", C[:, :, j], C)
        C[:, j, :] = np.where(ok[:, None], num / np.sqrt(np.where(ok, r, 1.0))[:, None], 0.0)
        rank += ok
    return rank


def _weights_ok_host(w, x, thr, full_rank):
    """the per-gene checks of getAndCheckWeights (R/core.R:2711-2734), all genes at once: test1 = rank(w_i * X) == p;
    test2 = the rows with w_i > thr, minus their all-zero columns, have full column rank.  Not full rank (expanded
    designs): no design column may be weighted out entirely."""
    n, m = w.shape
    p = x.shape[1]
    ok = np.ones(n, bool)
    if full_rank:
        w2 = w * w
        G1 = np.einsum("nm,ma,mb->nab", w2, x, x)
        t1 = _gram_rank(G1) == p
        keep = (w > thr).astype(np.float64)
        G2 = np.einsum("nm,ma,mb->nab", keep, x, x)
        ncol = (np.einsum("nm,ma->na", keep, np.abs(x)) > 0).sum(axis=1)
        t2 = _gram_rank(G2) == ncol
        ok = t1 & t2
    else:
        for j in range(p):
            allzero = ((w * x[None, :, j]) == 0).all(axis=1)
            ok &= ~allzero
    return ok


SF_ALL_ZERO = "every gene contains at least one zero, cannot compute log geometric means"       # R/core.R:558


def control_flags(controlGenes, n):
    """controlGenes (R/core.R:564-568: an index vector -- 0-based here -- or a logical vector over the genes) as n int32
    flags, the form the engine takes; None = every gene.  R's `counts[controlGenes, ]` would repeat a row listed twice:
    a repeated index is refused instead of silently counted once."""
    if controlGenes is None:
        return None
    c = np.asarray(controlGenes)
    if c.dtype == np.bool_:
        if c.shape != (n,):
            raise ValueError("a logical controlGenes must have one entry per gene")
        return np.ascontiguousarray(c, dtype=np.int32)
    if c.dtype.kind not in "iuf":
        raise ValueError("controlGenes should be either a numeric or logical vector")
    idx = c.astype(np.int64).reshape(-1)
    if (idx != c.reshape(-1)).any() or (idx < 0).any() or (idx >= n).any():
        raise IndexError("controlGenes: indices must be integers in [0, n)")
    if np.unique(idx).size != idx.size:
        raise ValueError("controlGenes: an index is listed twice")
    f = np.zeros(n, dtype=np.int32)
    f[idx] = 1
    return f


def spline_eval(table, u):
    """the piecewise cubic of a table x | y | b | c | d (5 x K) as R's splinefun() evaluates its "fmm" fit: interval = the
    largest i with x_i <= u (the first knot left of all), y + dx (b + dx (c + dx d)), cubic extrapolation on both sides"""
    x, y, b, c, d = np.asarray(table, np.float64).reshape(5, -1)
    u = np.asarray(u, np.float64)
    i = np.clip(np.searchsorted(x, u, side="right") - 1, 0, x.size - 1)
    dx = u - x[i]
    return y[i] + dx * (b[i] + dx * (c[i] + dx * d[i]))


class ResultColumns:
    """The columns of a results table where the engine made them (numpy arrays on the host engine, device vectors on the
    device engine): column(name) brings one to the host when it is asked for.  After filtered_p: numRej, cutoffs (host,
    K values each) and padj_column(j)."""
    numRej = cutoffs = _padj = None

    def __init__(self, cols, fetch=None):
        self.resident, self._fetch, self._hostcols = cols, fetch, {}

    def column(self, name):
        if name not in self._hostcols:
            v = self.resident[name]
            self._hostcols[name] = np.asarray(v) if self._fetch is None else self._fetch(v)
        return self._hostcols[name]

    def padj_column(self, j):
        return np.array(self._padj(int(j)), copy=True)


class ContrastColumns:
    """What an engine's contrasts() returns: the four n x K columns log2FoldChange, lfcSE, stat, pvalue (None in flags-only
    mode) and the n x K contrastAllZero flags, where the engine made them -- numpy arrays (n, K) on the host engine, device
    tensors (K, n) on the device engine.  columns(k) / flags(k): the n-vectors of contrast k, still resident."""
    NAMES = ("log2FoldChange", "lfcSE", "stat", "pvalue")

    def __init__(self, table, flag_matrix, pick):
        self.table, self.flag_matrix, self._pick = table, flag_matrix, pick

    def columns(self, k):
        return tuple(self._pick(t, k) for t in self.table)

    def flags(self, k):
        return self._pick(self.flag_matrix, k)


class DeviceLocalFit:
    """The local-regression dispersion trend on the device (DeviceEngine.local_fit): the resident fit handle, N, k and the
    all-below-floor flag.  Calling it on a host array of means evaluates on the device and returns a host array (the values
    and the status come down in one copy); on a resident vector it returns a resident vector and nothing comes down.
    nSingular: the singular points of the last evaluation that came to the host."""

    def __init__(self, E, means, disps, minDisp=1e-8):
        t = E.torch
        self.E, self.minDisp = E, float(minDisp)
        md = means if t.is_tensor(means) else E._vec(np.asarray(means, np.float64).reshape(-1))
        dd = disps if t.is_tensor(disps) else E._vec(np.asarray(disps, np.float64).reshape(-1))
        if md.shape != dd.shape:
            raise ValueError("means and disps must have one entry per gene each")
        r = E._timed("local_fit", int(md.numel()), lambda: E.native.local_fit_dev(md, dd, self.minDisp, evaluate=False))
        self.fit = r["fit"]
        st = E._host(r["status"]).numpy()
        self.N, self.k, self.nSingular, self.allBelowFloor = int(st[0]), int(st[1]), 0, bool(st[3])
        if self.N and self.k < 3:
            raise RuntimeError(E.native.LOCAL_FIT_TOO_FEW)

    def eval_dev(self, q, out=None):
        """dispFit at the resident means q (a contiguous float64 vector): (values, status), both resident"""
        r = self.E._timed("local_fit", int(q.numel()), lambda: self.E.native.local_fit_dev(
            eval_means=q, fit=self.fit, minDisp=self.minDisp, out=out))
        return r["dispFit"], r["status"]

    def __call__(self, q):
        E = self.E
        t = E.torch
        if t.is_tensor(q):
            return self.eval_dev(q.contiguous())[0]
        q = np.asarray(q, np.float64)
        if q.size == 0:
            return np.zeros(q.shape)
        v, st = self.eval_dev(E._vec(np.ascontiguousarray(q).reshape(-1)))
        h = E._host(t.cat([v, st.to(t.float64)])).numpy()
        self.nSingular = int(h[-2])
        return h[:-4].reshape(q.shape).copy()


class HostEngine:
    name = "host"

    def __init__(self, fns=None):
        if fns is None:
            from . import native as fns
        self.fns = fns

    # ---- handles
    # n x m handles are held column-major, as R holds them: the C ABI then takes them without a layout copy
    def counts(self, K):
        return np.asfortranarray(K, dtype=np.int32)

    def matrix(self, A):
        return None if A is None else np.asfortranarray(A, dtype=np.float64)

    def design(self, x):
        return np.ascontiguousarray(x, dtype=np.float64)

    def to_numpy(self, h):
        return h

    def take_rows(self, h, idx):
        return None if h is None else h[idx]

    def clamp_min(self, h, v):
        return np.maximum(h, v)

    def put_rows(self, h, idx, values):
        """h[idx, ] <- values (a few rows patched from the host, R/fitNbinomGLMs.R:386)"""
        h = np.array(h, copy=True)
        h[np.asarray(idx)] = values
        return h

    def set_rows(self, h, idx, sub):
        """h[idx, ] <- sub, both handles (mu[fitidx, ] <- fitMu, R/core.R:764)"""
        h = np.array(h, copy=True, order="F")
        h[np.asarray(idx)] = sub
        return h

    def nrow(self, h):
        return h.shape[0]

    # ---- n-vector log / exp in the engine's pinned arithmetic (csrc/dsq_math.hpp; the test suite's CPU checker restates it), so that
    # the host-side decision rules give the same bits whichever engine runs them and whether they run here or in
    # the fused device pipeline (R: log(), exp())
    def vlog(self, v):
        return self.fns.unary("log", np.asarray(v, np.float64))

    def vexp(self, v):
        return self.fns.unary("exp", np.asarray(v, np.float64))

    # ---- observation weights (getAndCheckWeights, R/core.R:2697-2751)
    def any_negative(self, h):
        return bool((h < 0).any())

    def row_max_normalize(self, h):
        """weights / apply(weights, 1, max)"""
        return np.asfortranarray(h / h.max(axis=1, keepdims=True))

    def weights_ok(self, w, x, thr, full_rank):
        return _weights_ok_host(np.asarray(w), x, thr, full_rank)

    # ---- O(n*m) steps the reference does in R around the native calls
    def prefit(self, y, nf, x, weights=None):
        """baseMean / baseVar / allZero, roughDispEstimate and the QR start values in one pass
        (R/core.R:2138-2146, 2422-2437; R/fitNbinomGLMs.R:139-145)"""
        return self.fns.prefitMoments(y, nf, x, weights, weights is not None)

    def xim(self, nf):
        """momentsDispEstimate's xim, R/core.R:2440-2444: mean over the samples of 1 / colMeans(nf) -- every column summed
        down the genes in gene order, the m reciprocals in sample order (the order contract of csrc/aux.hip xim_kernel
        and of the library's host entry; numpy's own mean() sums pairwise)"""
        nf = np.asarray(nf, np.float64)
        n, m = nf.shape
        rec = np.empty(m)
        for j0 in range(0, m, 64):
            rec[j0:j0 + 64] = 1.0 / (np.cumsum(nf[:, j0:j0 + 64], axis=0)[-1] / n)
        return float(np.cumsum(rec)[-1] / m)

    def size_factors(self, y, type="ratio", geoMeans=None, control=None, normMatrix=None):
        """estimateSizeFactorsForMatrix / estimateNormFactors (R/core.R:535-578, 2159-2163; "poscounts" as
        estimateSizeFactors.DESeqDataSet runs it, R/methods.R:377-382) in plain numpy: the host statement of what
        csrc/size_factors.hip computes on the device (libm log / exp and numpy's sums here, so equal to rounding, not
        to the bit).  control: int32 flags (control_flags) or None.  Returns sizeFactors (m), loggeomeans (n) and, with
        normMatrix, normalizationFactors (n x m)."""
        K = np.asarray(y, np.float64)
        n, m = K.shape
        V = K if normMatrix is None else K / np.asarray(normMatrix, np.float64)
        with np.errstate(all="ignore"):
            if type == "poscounts":
                pos = K > 0
                s = np.where(pos, np.log(np.where(pos, K, 1.0)), 0.0).sum(axis=1)
                lgm = np.log(np.where(pos.any(axis=1), np.exp(s / m), 0.0))
            elif geoMeans is not None:
                lgm = np.log(np.asarray(geoMeans, np.float64))
            else:
                lgm = np.log(V).sum(axis=1) / m
            if np.isinf(lgm).all():
                raise ValueError(SF_ALL_ZERO)
            use = np.isfinite(lgm)
            if control is not None:
                use &= np.asarray(control) != 0
            sf = np.full(m, np.nan)
            for j in range(m):
                sel = use & (V[:, j] > 0)
                if sel.any():
                    sf[j] = np.exp(np.median(np.log(V[sel, j]) - lgm[sel]))
            if type == "poscounts" or geoMeans is not None:
                sf = sf / np.exp(np.mean(np.log(sf)))                                   # R/core.R:573-576
            out = {"sizeFactors": sf, "loggeomeans": lgm}
            if normMatrix is not None:
                nf = np.asarray(normMatrix, np.float64) * sf[None, :]
                out["normalizationFactors"] = np.asfortranarray(nf / np.exp(np.log(nf).sum(axis=1) / m)[:, None])
        return out

    def vst_transform(self, y, nf, kind, sizeFactors=None, asymptDisp=None, extraPois=None, alpha=None, pc=1.0,
                      table=None, eta=None, xi=None):
        """getVarianceStabilizedData's formulas (R/vst.R:151-189), normTransform (R/helper.R:421-436) and
        counts(normalized = TRUE) in plain numpy + libm: the host statement of what csrc/vst.hip computes on the device
        (equal to rounding, not to the bit).  sizeFactors (m) take precedence over the nf handle.  Returns an n x m handle."""
        K = np.asarray(y, np.float64)
        with np.errstate(all="ignore"):
            q = K / (np.asarray(sizeFactors, np.float64)[None, :] if sizeFactors is not None else np.asarray(nf, np.float64))
            if kind == "parametric":
                a, e = float(asymptDisp), float(extraPois)
                r = np.log((1 + e + 2 * a * q + 2 * np.sqrt(a * q * (1 + e + a * q))) / (4 * a)) / np.log(2)
            elif kind == "mean":
                al = float(alpha)
                r = (2 * np.arcsinh(np.sqrt(al * q)) - np.log(al) - np.log(4)) / np.log(2)
            elif kind == "spline":
                r = float(eta) * spline_eval(table, np.arcsinh(q)) + float(xi)
            elif kind == "log2":
                r = np.log2(q + float(pc))
            elif kind == "normalized":
                r = q
            else:
                raise ValueError("kind should be parametric, mean, spline, log2 or normalized")
        return np.asfortranarray(r)

    def row_stats(self, y, nf, sizeFactors=None):
        """(rowMeans, row maxima) of the normalized counts (R/vst.R:166,175-176,239), host n-vectors"""
        K = np.asarray(y, np.float64)
        with np.errstate(all="ignore"):
            q = K / (np.asarray(sizeFactors, np.float64)[None, :] if sizeFactors is not None else np.asarray(nf, np.float64))
            return q.mean(axis=1), q.max(axis=1)

    def rlog_fit(self, y, nf, dispFit, betaPriorVar, intercept=None, sizeFactors=None, tol=1e-4, maxit=100, minmu=0.5):
        """The fit of rlogData the way the reference runs it (R/rlog.R:186-254): the dense model matrix [1 | I_m] (no
        intercept given) or I_m (the caller's intercept folded into the factors, :208-219), the start values of
        R/fitNbinomGLMs.R:139-155, lambda / log(2)^2 (:162), then the fit module's fitBeta with useQR = TRUE on the rows
        that are fitted.  The independent host statement of what csrc/rlog.hip computes with two sums per step; it stops
        where the dense fit stops (DSQ_MAX_P = 64 columns).  Returns dict(rlog: n x m handle, intercept (form A), iter,
        flag: 0 fitted, 1 row not fitted, 2 a non-finite coefficient)."""
        K = np.asarray(y, np.float64)
        n, m = K.shape
        NF = np.broadcast_to(np.asarray(sizeFactors, np.float64)[None, :], (n, m)) if sizeFactors is not None else np.asarray(nf, np.float64)
        disp = np.broadcast_to(np.asarray(dispFit, np.float64), (n,))
        formA = intercept is None
        p = m + 1 if formA else m
        if p > 64:
            raise NotImplementedError("the dense rlog fit of the host engine stops at 64 design columns (m = %d)" % m)
        if formA:
            x = np.hstack([np.ones((m, 1)), np.eye(m)])                              # model.matrix(~samples)[-1, ], :192-194
            fitted = (K != 0).any(axis=1)                                            # !allZero, :227
            lam = np.r_[1e-6, np.full(m, 1.0 / float(betaPriorVar))]                 # :243-247
        else:
            x = np.eye(m)                                                            # model.matrix(~ 0 + samples), :202
            icpt = np.asarray(intercept, np.float64)
            fitted = np.isfinite(icpt)                                               # allZero <- infiniteIntercept, :223
            NF = NF * np.exp2(np.where(fitted, icpt, -10.0))[:, None]                # :216-219
            lam = np.full(m, 1.0 / float(betaPriorVar))
        out = np.zeros((n, m), order="F")
        oi = np.full(n, -np.inf) if formA else None
        it = np.zeros(n)
        flag = np.where(fitted, 0, 1).astype(np.int32)
        idx = np.where(fitted)[0]
        if idx.size:
            Ks, NFs = K[idx], np.asfortranarray(NF[idx])
            q = Ks / NFs
            if formA:                                                                # not of full rank: R/fitNbinomGLMs.R:147-151
                b0 = np.zeros((idx.size, p))
                b0[:, 0] = np.log(q.mean(axis=1))
            else:                                                                    # Q and R of an identity: :142-145
                b0 = np.log(q + 0.1)
            r = self.fit_beta(self.counts(Ks), x, NFs, np.ascontiguousarray(disp[idx]), np.r_[1.0, np.zeros(p - 1)],
                              np.asfortranarray(b0), lam / np.log(2) ** 2, None, False, tol, maxit, True, minmu,
                              want_mu=False, want_hat=False)
            beta = np.log2(np.e) * np.asarray(r["beta_mat"])                         # :194
            vals = beta @ x.T                                                        # t(modelMatrix %*% t(betaMatrix)), R/rlog.R:254
            if not formA:
                vals = vals + icpt[idx][:, None]                                     # :260
            bad = ~np.isfinite(beta).all(axis=1)
            vals[bad] = np.nan
            out[idx] = vals
            it[idx] = np.asarray(r["iter"]).reshape(-1)
            flag[idx[bad]] = 2
            if formA:
                oi[idx] = np.where(bad, np.nan, beta[:, 0])
        return {"rlog": out, "intercept": oi, "iter": it, "flag": flag}

    def unmix_fit(self, x, pure, alpha=None, shift=None, power=1, maxit=200):
        """the fits of unmix() (R/helper.R:96-112): x an n x m handle (or array) of normalized counts / TPMs, pure an n x k
        array.  The iteration of csrc/unmix.hip stated in numpy over this engine's log (unmix_host.py), the same bits.
        Returns dict(p m x k, loss m, iter m, flag m) on the host."""
        from . import unmix_host
        return unmix_host.unmix_fit(self.vlog, np.asarray(x, np.float64), pure, alpha=alpha, shift=shift, power=power, maxit=maxit)

    def apeglm_fit(self, y, x, nf, disp, coef, no_shrink, prior_scale, prior_df=1.0, no_shrink_scale=15.0, weights=None,
                   init=None, threshold=None, tol=1e-8, maxit=100, sizeFactors=None):
        """the apeglm posterior per gene: y / nf / weights n x m handles (or arrays), x m x p,
        no_shrink a boolean mask of p, init n x p or None.  The iteration of csrc/apeglm.hip stated in numpy over this
        engine's exp / log / log1p (apeglm_host.py), the same bits.  Returns dict(map n x p, sd n x p, fsr, thresh,
        iter n x 2, conv, start, objective) on the host, NaN on the rows that are not fitted."""
        from . import apeglm_host
        if np.asarray(x).shape[1] > apeglm_host.MAX_P:
            raise NotImplementedError("apeglm: %d design columns (at most %d are served)" % (np.asarray(x).shape[1], apeglm_host.MAX_P))
        return apeglm_host.fit(self.fns.unary, np.asarray(y, np.float64), x, sizeFactors if sizeFactors is not None else nf,
                               np.asarray(disp, np.float64), coef, no_shrink, prior_scale, prior_df, no_shrink_scale,
                               weights=None if weights is None else np.asarray(weights, np.float64),
                               init=None if init is None else np.asarray(init, np.float64), threshold=threshold, tol=tol,
                               maxit=maxit)

    def ash_fit(self, betahat, sebetahat, threshold=None, maxit=100):
        """adaptive shrinkage of C independent columns: betahat / sebetahat vectors of n or n x C
        matrices (or this engine's columns).  The iteration of csrc/ash.hip and of its host loop stated in numpy over this
        engine's exp / log (ash_host.py), the same bits.  Returns dict(PosteriorMean, PosteriorSD, NegativeProb,
        PositiveProb, lfsr, le_T, gt_mT: n x C on the host, NaN on the rows that are not kept; pi, sd: C x 64; K, iter,
        flag: C; loglik: C).  ValueError: a column without a kept row; NotImplementedError: a grid beyond 64 components."""
        from . import ash_host
        b, s = np.asarray(betahat, np.float64), np.asarray(sebetahat, np.float64)
        if isinstance(betahat, (list, tuple)):          # (a list of C columns, as the device engine takes them)
            b, s = b.T, s.T
        out = ash_host.fit(self.fns.unary, b.reshape(b.shape[0], -1), s.reshape(s.shape[0], -1), threshold=threshold, maxit=maxit)
        for k in ash_host.ROW_KEYS:                     # (C, n), column c contiguous: what the device engine returns
            out[k] = np.ascontiguousarray(out[k].T)
        return out

    def row_vars(self, x):
        """(rowMean, rowVar) of an n x m handle (matrixStats::rowVars as documented): the two wave-order sums of
        csrc/explore.hip stated in numpy (explore_host.py), the same bits"""
        from . import explore_host
        return explore_host.row_vars(np.asarray(x, np.float64))

    def top_var(self, x, ntop):
        """the first min(ntop, n) rows of order(rowVars, decreasing = TRUE) (R/plots.R:245-248).  dict(select: the 0-based
        rows on the host, selVar: their variances on the host, rows / centre: the list and the means of the listed rows in
        the form this engine's pair_sums takes)"""
        from . import explore_host
        mean, var = self.row_vars(x)
        sel = explore_host.top_var(var, ntop)
        return {"select": sel, "selVar": var[sel], "rows": sel, "centre": mean[sel]}

    def pair_sums(self, x, kind, rows=None, centre=None):
        """the m x m all-pairs sums over the listed rows (all rows when None) of an n x m handle on the host: kind "dist2",
        "dist" or "gram" (rows less centre, one value per listed row), in the order of csrc/explore.hip (explore_host.py)"""
        from . import explore_host
        return explore_host.pair_sums(np.asarray(x, np.float64), kind, rows=rows, centre=centre)

    # ---- collapseReplicates / colSums / fpm / fpkm (R/helper.R:187-216, 291-391): plain numpy, the host statement of
    # csrc/count_helpers.hip (integer sums exact, every quotient and product one IEEE operation in R's order: the same bits)
    def collapse_columns(self, y, members, offsets):
        """the n x g count handle of group sums (group c = members[offsets[c] .. offsets[c + 1]), 0-based samples) and the
        status: 1 when a sum is no int32 (R: NA from mode<-), the handle then being of no use"""
        K = np.asarray(y)
        members = np.asarray(members, np.int64)
        cols = [K[:, members[offsets[c]:offsets[c + 1]]].sum(axis=1, dtype=np.int64) for c in range(len(offsets) - 1)]
        S = np.stack(cols, axis=1)
        status = int((S > np.iinfo(np.int32).max).any() or (S < np.iinfo(np.int32).min).any())
        return self.counts(S.astype(np.int32)), status

    def collapse_overflow_group(self, y, members, offsets):
        """the first group one of whose sums is no int32 (the error path of collapse_columns), or None"""
        K = np.asarray(y)
        for c in range(len(offsets) - 1):
            s = K[:, np.asarray(members[offsets[c]:offsets[c + 1]], np.int64)].sum(axis=1, dtype=np.int64)
            if (s > np.iinfo(np.int32).max).any() or (s < np.iinfo(np.int32).min).any():
                return c
        return None

    def col_sums(self, y):
        """colSums of a count handle before the conversion to double: m exact int64 sums on the host"""
        return np.asarray(y).sum(axis=0, dtype=np.int64)

    def fpm_transform(self, y, lib, kind, basepairs=None, txlen=None):
        """fpm / fpkm of a count handle (R/helper.R:390, 322, 294) for m library sizes: kind "fpm", "fpkm_basepairs"
        (basepairs: n) or "fpkm_txlen" (txlen: an n x m handle).  Returns an n x m handle."""
        K = np.asarray(y).astype(np.float64)
        with np.errstate(all="ignore"):
            f = 1e6 * (K / np.asarray(lib, np.float64)[None, :])
            if kind == "fpkm_basepairs":
                f = 1e3 * (f / np.asarray(basepairs, np.float64)[:, None])
            elif kind == "fpkm_txlen":
                f = (1e3 * f) / np.asarray(txlen, np.float64)
            elif kind != "fpm":
                raise ValueError("kind should be fpm, fpkm_basepairs or fpkm_txlen")
        return np.asfortranarray(f)

    def sf_iterate_solve(self, y, mu, sf, disp, rows, Q=0.05, maxit=100):
        """the solve of one round of estimateSizeFactorsIterate (R/core.R:2600-2611): y / mu n x m handles, sf the m size
        factors mu was fitted with, disp n, rows n flags (rowSums > 0).  The iteration of csrc/sf_iterate.hip stated in numpy
        over this engine's nbinomLogLike, log and exp (sf_iterate_host.py), the same bits.  Returns dict(s, sf, F, iter,
        evals, flag) on the host."""
        from . import sf_iterate_host
        loglike = lambda K, mu_, a: self.fns.nbinomLogLike(K, mu_, a, None, False)
        return sf_iterate_host.solve(loglike, self.vexp, self.vlog, y, mu, sf, disp, rows, float(Q), int(maxit),
                                     sf_iterate_host.SLICE_GENES)

    def nf_col_geomeans(self, nf):
        """exp(colMeans(log(normalizationFactors))): the approximate size factors of R/vst.R:162"""
        return np.exp(np.log(np.asarray(nf, np.float64)).mean(axis=0))

    def linear_mu(self, y, nf, x):
        """linearModelMuNormalized, R/core.R:2465-2471 (engine kernel: a BLAS product on the host would make
        a gene's value depend on how many rows are in the call)"""
        return self.fns.linearMu(y, nf, x)

    def nbinom_loglike(self, y, mu, disp, weights, useWeights):
        """nbinomLogLike, R/core.R:2208-2217"""
        return self.fns.nbinomLogLike(y, mu, disp, weights if useWeights else None, useWeights)

    def optim_rows(self, y, nf, x, alpha, lam, weights, useWeights, beta_start, minmu):
        """fitNbinomGLMsOptim on the rows handed over (R/fitNbinomGLMs.R:340-407); mu comes back as a host array"""
        return self.fns.optimRows(y, x, nf, alpha, lam, weights if useWeights else None, useWeights, beta_start, minmu)

    def intercept_fit(self, y, nf, alpha, weights, useWeights, mu_floor=0.0, want_hat=True):
        """closed form of the intercept-only model, R/fitNbinomGLMs.R:99-137"""
        return self.fns.interceptFit(y, nf, alpha, weights if useWeights else None, useWeights, mu_floor, want_hat)

    def parametric_fit(self, means, disps):
        """parametricDispersionFit, R/core.R:2166-2190"""
        return self.fns.parametricDispersionFit(means, disps)

    def local_fit(self, means, disps, minDisp=1e-8):
        """localDispersionFit, R/core.R:2194-2203: the function of the mean, local_fit_host.py on this
        engine's log / exp"""
        from . import local_fit_host
        return local_fit_host.LocalFit(self.vlog, self.vexp, means, disps, minDisp)

    def mad(self, v):
        """stats::mad (R/methods.R:180)"""
        v = np.asarray(v, np.float64)
        med = np.median(v)
        return 1.4826 * np.median(np.abs(v - med))

    def two_sided_normal_p(self, z):
        """2 * pnorm(abs(z), lower.tail = FALSE), R/core.R:1507 (Cody's algorithm as in R's pnorm, engine arithmetic)"""
        return self.fns.unary("pnorm_upper2", np.asarray(z, np.float64))

    # ---- Student's t: student_t.py on this engine's exp / log / log1p / stirlerr
    def pt(self, q, df, tail="lower", keep=None, out=None):
        """pt over an n x K column (or an n-vector) q with row i's df: tail "lower", "upper" or "two_sided" (2 * upper(|q|));
        where keep is non-zero the entry of `out` (q when not given) stays.  The statement of csrc/student.hip."""
        from . import student_t as S
        q = np.asarray(q, np.float64)
        d = np.asarray(df, np.float64).reshape((-1,) + (1,) * (q.ndim - 1))
        r = {"lower": S.pt_lower, "upper": S.pt_upper, "two_sided": S.pt_two_sided}[tail](self.fns, q, d)
        if keep is not None:
            r = np.where(np.asarray(keep) != 0, q if out is None else out, r)
        return r

    def _pt_pair(self, df):
        if df is None:
            return None
        from . import student_t as S
        df = np.asarray(df, np.float64)
        return (lambda q: S.pt_lower(self.fns, q, df)), (lambda q: S.pt_upper(self.fns, q, df))

    # ---- the beta prior variance of all columns (R/core.R:1601-1689)
    def beta_prior_var(self, mle_beta, baseMean, dispFit, allZero, coef_factor, prior_coef_factor=None, prior_coef_src=None):
        """estimateBetaPriorVar over the n x p MLE coefficients (log2 scale), rows flagged allZero left out; the column coding
        of native.coef_factor_codes; prior_coef_factor given = the expanded model matrix.  The library's host function
        (dsq_beta_prior_var: the definition core.estimateBetaPriorVar follows, the same bits)."""
        from . import native
        return native.estimateBetaPriorVarHost(mle_beta, baseMean, dispFit, allZero, coef_factor,
                                               prior_coef_factor=prior_coef_factor, prior_coef_src=prior_coef_src)

    # ---- results() (R/results.R:443-575, 638-740): the numpy statement of csrc/results.hip
    def results_table(self, lfc, se, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
                      altHypothesis="greaterAbs", df=None):
        """the five columns of one coefficient (n-vectors in): threshold tests (under Student's t with the n degrees of
        freedom df when given), pvalue NA where na_mask, the nowZero fill"""
        from . import results_host as R
        return ResultColumns(R.results_table(self.vexp, lfc, se, stat, pvalue, baseMean, replace, na_mask, lfcThreshold,
                                             altHypothesis, self._pt_pair(df)))

    def filtered_p(self, tab, filter=None, theta=None, alpha=0.1):
        """BH-adjusted p-values of `tab` over filter >= quantile(filter, theta), one column per theta (theta None: one
        column, no filtering); sets filtPadj / numRej / cutoffs on tab and returns it"""
        from . import results_host as R
        f = tab.column("baseMean") if filter is None else filter
        fp, tab.numRej, tab.cutoffs = R.filtered_p(f, tab.column("pvalue"), theta, alpha)
        tab._padj = lambda j: fp[:, j]
        return tab

    def results(self, lfc, se, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
                altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1, df=None):
        return self.filtered_p(self.results_table(lfc, se, stat, pvalue, baseMean, replace, na_mask, lfcThreshold,
                                                  altHypothesis, df=df), filter, theta, alpha)

    # ---- contrasts (R/results.R:760-827, 1021-1028, 1237-1270): the statement csrc/contrasts.hip equals
    def contrasts(self, y, x, nf, alpha_hat, beta, lam, contrasts, weights, useWeights, minmu, allZero, sample_mask=None,
                  rule_applies=None, sizeFactors=None, df=None):
        """K contrasts of the fitted coefficients.  y: the ORIGINAL counts handle (read by the masks only), x: the model
        matrix the coefficients were fitted on (m x p), nf: the normalization-factor handle (or None with sizeFactors),
        alpha_hat (n), beta (n x p, natural-log scale), lam (p, natural-log scale), contrasts (p x K, or None: flags
        only), weights: the normalised handle, allZero (n flags), sample_mask (K x m of 0 / 1) with rule_applies (K).
        getContrast per contrast -- fitBeta(maxit = 0) on the rows that are not all zero --, log2(exp(1)) on both members,
        the quotient, the two-sided normal p-value (df, n degrees of freedom, given: 2 pt(|stat|, df, lower.tail = FALSE),
        :812-815), NA rows, then the all-zero rule.  Returns ContrastColumns."""
        allZero = np.asarray(allZero, bool)
        n, live = allZero.size, ~np.asarray(allZero, bool)
        K = np.shape(contrasts)[1] if contrasts is not None else np.shape(sample_mask)[0]
        flags = np.zeros((n, K), bool)
        if sample_mask is not None:
            cnt = np.asarray(y)
            rule = np.ones(K, bool) if rule_applies is None else np.asarray(rule_applies, bool)
            for k in range(K):
                if rule[k]:
                    sel = np.asarray(sample_mask[k]) != 0
                    flags[:, k] = live & ~(cnt[:, sel] != 0).any(axis=1)                  # :1242, :1268-1269, :1023
        pick = lambda a, k: a[:, k]
        if contrasts is None:
            return ContrastColumns(None, flags, pick)
        contrasts = np.asarray(contrasts, np.float64)
        x = np.asarray(x, np.float64)
        nz = np.where(live)[0]
        m = x.shape[0]
        nfm = np.asarray(nf) if nf is not None else np.broadcast_to(np.asarray(sizeFactors, np.float64)[None, :], (n, m))
        ynz = np.asfortranarray(np.asarray(y)[nz])
        nfnz = np.asfortranarray(nfm[nz])
        wnz = np.asfortranarray(np.asarray(weights)[nz]) if useWeights else None
        anz, bnz = np.asarray(alpha_hat, np.float64)[nz], np.asfortranarray(np.asarray(beta, np.float64)[nz])
        LOG2E = np.log2(np.e)                                                            # log2(exp(1)), :809-810
        table = [np.full((n, K), np.nan) for _ in range(4)]
        for k in range(K):
            if nz.size == 0:
                break
            r = self.fit_beta(ynz, x, nfnz, anz, contrasts[:, k], bnz, lam, wnz, useWeights, 1e-8, 0, False, minmu,
                              want_mu=False, want_hat=False)                              # :797-807
            lfc = LOG2E * np.asarray(r["contrast_num"]).reshape(-1)
            se = LOG2E * np.asarray(r["contrast_denom"]).reshape(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                stat = lfc / se
            pv = self.two_sided_normal_p(stat)                                           # :817
            if df is not None:
                pv = self.pt(stat, np.asarray(df, np.float64)[nz], "two_sided")          # :812-815
            for t, v in zip(table, (lfc, se, stat, pv)):
                t[nz, k] = v                                                             # buildDataFrameWithNARows, :823
            z = flags[:, k]
            table[0][z, k], table[2][z, k], table[3][z, k] = 0.0, 0.0, 1.0               # :1024-1028
        return ContrastColumns(table, flags, pick)

    def zero_rule(self, lfc, stat, pvalue, flag):
        """res$log2FoldChange[contrastAllZero] <- 0, stat <- 0, pvalue <- 1 (R/results.R:1024-1028) on columns of the host"""
        flag = np.asarray(flag, bool)
        return (np.where(flag, 0.0, lfc), np.where(flag, 0.0, stat), np.where(flag, 1.0, pvalue))

    # ---- count outliers (R/core.R:2333-2359, 2069-2115)
    def cooks_distance(self, y, nf, mu, H, x):
        """calculateCooksDistance + recordMaxCooks; x = the dispersion model matrix"""
        return self.fns.cooksDistance(y, nf, mu, H, x)

    def replace_outliers(self, y, nf, cooks, cooksCutoff, replaceable, trim=0.2):
        """replaceOutliers: new counts handle + per-gene `replace` flag"""
        r = self.fns.replaceOutliers(y, nf, cooks, cooksCutoff, replaceable, trim)
        return {"counts": np.asfortranarray(r["counts"], dtype=np.int32), "replace": r["replace"]}     # (stays column-major)

    def masked_row_max(self, h, use, zero):
        """apply(h[, use], 1, max) after h[, zero] <- 0   (refitWithoutOutliers, R/core.R:2542-2545)"""
        a = np.where(np.asarray(zero, bool)[None, :], 0.0, h)
        return a[:, np.asarray(use, bool)].max(axis=1)

    def _ones(self, n, m):
        """the all-ones weight matrix R passes when there are no weights (R/fitNbinomGLMs.R:85): one per shape.  The
        engine library never reads unused weights (useWeights = FALSE), so for it no matrix is built at all."""
        if getattr(self.fns, "IGNORES_UNUSED_WEIGHTS", False):
            return None
        if getattr(self, "_ones_cache", None) is None or self._ones_cache.shape != (n, m):
            self._ones_cache = np.ones((n, m), order="F")
        return self._ones_cache

    # ---- the three native routines
    def fit_beta(self, y, x, nf, alpha_hat, contrast, beta_mat, lam, weights, useWeights, tol, maxit, useQR,
                 minmu, want_mu=True, mu_floor=0.0, want_hat=True):
        n, m = y.shape
        w = weights if weights is not None else self._ones(n, m)
        # mu = nf * exp(x beta) comes back from the engine (extension of the fitBeta entry point)
        # instead of being recomputed on the host as R/fitNbinomGLMs.R:180 does
        return self.fns.fitBeta(y, x, nf, alpha_hat, contrast, beta_mat, lam, w, useWeights, tol, maxit, useQR, minmu,
                                want_mu=want_mu, mu_floor=mu_floor, want_hat=want_hat)

    def fit_disp(self, y, x, mu_hat, log_alpha, prior_mean, prior_sigmasq, min_log_alpha, kappa_0, tol, maxit,
                 usePrior, weights, useWeights, weightThreshold, useCR):
        n, m = y.shape
        w = weights if weights is not None else self._ones(n, m)
        return self.fns.fitDisp(y, x, mu_hat, log_alpha, prior_mean, prior_sigmasq, min_log_alpha, kappa_0, tol,
                                maxit, usePrior, w, useWeights, weightThreshold, useCR)

    def fit_disp_grid(self, y, x, mu_hat, disp_grid, prior_mean, prior_sigmasq, usePrior, weights, useWeights,
                      weightThreshold, useCR):
        n, m = y.shape
        w = weights if weights is not None else self._ones(n, m)
        return self.fns.fitDispGrid(y, x, mu_hat, disp_grid, prior_mean, prior_sigmasq, usePrior, w, useWeights,
                                    weightThreshold, useCR)


class DeviceEngine:
    name = "device"

    def __init__(self, device="cuda:0"):
        import torch
        from . import native
        self.torch = torch
        self.native = native
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceEngine needs a CUDA/HIP device; deseq2_amd has no CPU compute path")
        torch.cuda.set_device(self.device)
        from . import _lib
        _lib.check(_lib.lib().dsq_set_device(self.device.index or 0))
        self._cache = {}
        self._cells = {}
        self._tls = threading.local()
        self.record = None          # set to a list to collect (name, n, ms) per fit kernel
        self.want_d2lp = False      # estimateDispersions* never read fitDisp$last_d2lp (R/core.R:784-787,1042)

    def _timed(self, name, n, fn):
        """profiling pass only: the C library brackets the fit kernel with HIP events on the
        launch stream (dsq_profile_enable); read the duration back after the call."""
        if self.record is None:
            return fn()
        from . import _lib
        L = _lib.lib()
        with _PROF_LOCK:            # the library keeps ONE pair of events: chunk threads take turns here
            L.dsq_profile_enable(1)
            r = fn()
            ms = L.dsq_profile_last_ms()
            L.dsq_profile_enable(0)
        self.record.append((name, n, ms))
        return r

    def _host(self, t):
        """device tensor -> host tensor through PINNED memory (torch's caching host allocator recycles
        the blocks, so this is an async DMA + one stream sync instead of a staged pageable copy)"""
        h = self.torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        # cooperative chunk pipeline (parallel.Pipeline): this is the point where the host would block on the
        # GPU, so the chunk hands the interpreter to the next chunk first and synchronises when it is back
        wait = getattr(self._tls, "before_sync", None)
        if wait is not None:
            wait()
        self.torch.cuda.current_stream().synchronize()
        return h

    def _vec(self, a):
        """host vector -> device, through pinned memory and WITHOUT blocking the host: a pageable copy on the
        (null) stream would wait for every kernel launched before it, i.e. serialise launch and host code"""
        t = self.torch
        a = np.ascontiguousarray(a, dtype=np.float64)
        h = t.empty(a.shape, dtype=t.float64, pin_memory=True)
        h.numpy()[...] = a
        return h.to(self.device, non_blocking=True)

    # ---- handles
    def counts(self, K):
        t = self.torch.as_tensor(np.ascontiguousarray(np.asarray(K, dtype=np.int32).T), device=self.device)
        return self.native.to_gene_major(t)

    def matrix(self, A):
        if A is None:
            return None
        t = self.torch.as_tensor(np.ascontiguousarray(np.asarray(A, dtype=np.float64).T), device=self.device)
        return self.native.to_gene_major(t)

    def design(self, x):
        """(p, m) device copy of the model matrix, memoised on its bytes (asked for by every fit of a DESeq())"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = ("x", x.shape, x.tobytes())
        v = self._cache.get(key)
        if v is None:
            v = self._cache[key] = self.torch.as_tensor(np.ascontiguousarray(x.T), device=self.device)
            self._cells[v.data_ptr()] = self.native.cell_index(x)       # design cells, for the cell-collapsed fitBeta
        return v

    def _design_qr_dev(self, x):
        """device copies of Q, X R^-1, R of the (memoised) thin QR of the model matrix"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        key = ("qr", x.shape, x.tobytes())
        v = self._cache.get(key)
        if v is None:
            t = self.torch
            q, a, r = self.native.design_qr(x)
            v = self._cache[key] = tuple(t.as_tensor(np.ascontiguousarray(z.T), device=self.device) for z in (q, a, r))
        return v

    def to_numpy(self, h):
        return self._host(h.view()).numpy()

    def to_numpy_np(self, b):
        """n x p host matrix from either a host array or the (p, n) device tensor of start values"""
        return self._host(b.t()).numpy() if self.torch.is_tensor(b) else np.asarray(b)

    def take_rows(self, h, idx):
        if h is None:
            return None
        ii = self.torch.as_tensor(np.asarray(idx), device=self.device)
        if ii.dtype == self.torch.bool:
            ii = ii.nonzero().squeeze(1)
        return self.native.GeneMajor(h.t.index_select(0, ii).contiguous(), h.m)

    def clamp_min(self, h, v):
        return self.native.GeneMajor(self.torch.clamp_min(h.t, v), h.m)

    def put_rows(self, h, idx, values):
        t = self.torch
        ii = t.as_tensor(np.asarray(idx), device=self.device)
        out = h.t.clone()
        out[ii, : h.m] = t.as_tensor(np.ascontiguousarray(values, dtype=np.float64), device=self.device)
        return self.native.GeneMajor(out, h.m)

    def set_rows(self, h, idx, sub):
        t = self.torch
        ii = t.as_tensor(np.asarray(idx), device=self.device)
        out = h.t.clone()
        out[ii] = sub.t
        return self.native.GeneMajor(out, h.m)

    def nrow(self, h):
        return h.n

    def vlog(self, v):
        return self.native.unary("log", np.asarray(v, np.float64))

    def vexp(self, v):
        return self.native.unary("exp", np.asarray(v, np.float64))

    # ---- observation weights: elementwise / flag work on the resident handle
    def any_negative(self, h):
        return bool((h.view() < 0).any())

    def row_max_normalize(self, h):
        t = self.torch
        out = t.zeros_like(h.t)
        out[:, : h.m] = h.view() / h.view().max(dim=1, keepdim=True).values
        return self.native.GeneMajor(out, h.m)

    def _prof_lock(self):
        return _PROF_LOCK

    def weights_ok(self, w, x, thr, full_rank):
        return self._host(self.weights_ok_dev(w, x, thr, full_rank)).numpy()

    def weights_ok_dev(self, w, x, thr, full_rank):
        """the flags of weights_ok as a device tensor (no host round trip)"""
        t = self.torch
        xd = t.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=self.device)
        wv = w.view()
        p = xd.shape[1]
        if not full_rank:
            ok = t.ones(w.n, dtype=t.bool, device=self.device)
            for j in range(p):
                ok &= ~((wv * xd[None, :, j]) == 0).all(dim=1)
            return ok

        def rank(G, tol=1e-7):               # _gram_rank (dqrdc2's column-relative test) on the device
            d0 = t.diagonal(G, dim1=1, dim2=2)
            C = t.zeros_like(G)
            rk = t.zeros(G.shape[0], dtype=t.int64, device=self.device)
            for j in range(p):
                r = d0[:, j] - (C[:, :, j] ** 2).sum(dim=1)
                ok = (d0[:, j] > 0) & (r >= (tol * tol) * d0[:, j])
                num = G[:, j, :] - t.einsum("nk,nkj->nj", C[:, :, j], C)
                den = t.sqrt(t.where(ok, r, t.ones_like(r)))[:, None]
                C[:, j, :] = t.where(ok[:, None], num / den, t.zeros_like(num))
                rk += ok
            return rk
        xx = (xd[:, :, None] * xd[:, None, :]).reshape(xd.shape[0], p * p)          # m x p^2
        G1 = ((wv * wv) @ xx).reshape(-1, p, p)
        keep = (wv > thr).to(t.float64)
        G2 = (keep @ xx).reshape(-1, p, p)
        ncol = ((keep @ xd.abs()) > 0).sum(dim=1)
        return (rank(G1) == p) & (rank(G2) == ncol)

    # ---- O(n*m) steps around the fits: HIP kernels too (csrc/aux.hip)
    def prefit(self, y, nf, x, weights=None):
        t = self.torch
        dq, da, dr = self._design_qr_dev(x)          # m x p design: thin QR on the host, like stats::qr
        o = self._timed("prefit_moments", y.n, lambda: self.native.prefitMoments_dev(
            y, nf, dq, da, dr, weights, weights is not None))
        h = self._host(o["_pack"])                        # one copy for the four n-vectors
        n = y.n
        return {"baseMean": h[0].numpy(), "baseVar": h[1].numpy(),
                "allZero": h[3].view(t.int32)[:n].numpy().astype(bool), "roughDisp": h[2].numpy(),
                "beta_init": o["beta_init"]}        # (p, n) device tensor, consumed by fit_beta in place

    def xim(self, nf):
        """momentsDispEstimate's xim (R/core.R:2440-2444) by the library's kernel: columns summed down the genes in gene
        order, the same definition the one-call host entry uses"""
        from . import _lib
        import ctypes as C
        t = self.torch
        buf = t.empty(nf.m + 1, dtype=t.float64, device=self.device)
        st = C.c_void_p(t.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().dsq_xim_dev(C.c_void_p(nf.t.data_ptr()), nf.n, nf.m, nf.ld, C.c_void_p(buf.data_ptr()),
                                          C.c_void_p(buf[nf.m:].data_ptr()), st))
        return float(self._host(buf[nf.m:])[0])

    def size_factors(self, y, type="ratio", geoMeans=None, control=None, normMatrix=None):
        """estimateSizeFactors on the resident counts (csrc/size_factors.hip): the loggeomeans, the per-sample medians by
        radix selection and, with a normMatrix handle, the normalization-factor matrix, all on the current stream.  The ONE
        host look is the m size factors with the status word (the caller needs them for xim, and R's error for a matrix
        whose every gene has a zero has to surface).  sizeFactors_dev / normalizationFactors stay resident."""
        r = self.native.sizeFactors_dev(y, type=type, geoMeans=None if geoMeans is None else self._vec(geoMeans),
                                        control=control, normMatrix=normMatrix)
        h = self._host(r["_pack"])
        if int(h[y.m:].view(self.torch.int32)[0]) == 1:
            raise ValueError(SF_ALL_ZERO)
        out = {"sizeFactors": h[: y.m].numpy().copy(), "sizeFactors_dev": r["sizeFactors"], "loggeomeans_dev": r["loggeomeans"]}
        if normMatrix is not None:
            out["normalizationFactors"] = r["normalizationFactors"]
        return out

    def _sf_dev(self, sizeFactors):
        """the m size factors as a device vector (the one estimateSizeFactors left resident, if these are its bytes)"""
        sf = np.ascontiguousarray(sizeFactors, dtype=np.float64)
        v = self._cache.get(("sf", sf.tobytes()))
        return v if v is not None else self._vec(sf)

    def vst_transform(self, y, nf, kind, sizeFactors=None, asymptDisp=None, extraPois=None, alpha=None, pc=1.0,
                      table=None, eta=None, xi=None):
        """the transformation of the resident counts in one pass (csrc/vst.hip, dsq_vst_dev) on the current stream; the
        n x m result is a handle and stays in HBM.  What goes up: the scalars of the formula (kernel arguments) and, for
        the spline formula, the 40 KB table.  Nothing comes down."""
        f = self._sf_dev(sizeFactors) if sizeFactors is not None else nf
        return self._timed("vst_transform", y.n, lambda: self.native.vst_dev(
            y, f, kind, asymptDisp=asymptDisp, extraPois=extraPois, alpha=alpha, pc=pc, table=table, eta=eta, xi=xi))

    def row_stats(self, y, nf, sizeFactors=None):
        """(rowMeans, row maxima) of the normalized counts by dsq_vst_rowstats_dev; the two n-vectors come to the host in one
        copy (vst()'s subset rule and the spline path's quantiles are host decisions over n-vectors)"""
        f = self._sf_dev(sizeFactors) if sizeFactors is not None else nf
        pack = self._timed("vst_rowstats", y.n, lambda: self.native.vstRowStats_dev(y, f))
        h = self._host(pack).numpy()
        return h[0], h[1]

    def rlog_fit(self, y, nf, dispFit, betaPriorVar, intercept=None, sizeFactors=None, tol=1e-4, maxit=100, minmu=0.5):
        """the fit of rlogData on the resident counts (csrc/rlog.hip, dsq_rlog_dev) on the current stream, any number of
        samples; the n x m result is a handle and stays in HBM.  What goes up: dispFit (and the intercept); what comes down:
        the fitted intercept, the iteration counts and the row flags (n-vectors) and the bad-count word."""
        t = self.torch
        f = self._sf_dev(sizeFactors) if sizeFactors is not None else nf
        bad = t.zeros(2, dtype=t.int32, device=self.device) if y.t.dtype == t.float64 else None
        r = self._timed("rlog", y.n, lambda: self.native.rlog_dev(
            y, f, self._vec(dispFit), betaPriorVar, intercept=None if intercept is None else self._vec(intercept),
            tol=tol, maxit=maxit, minmu=minmu, bad=bad))
        if bad is not None and int(self._host(bad)[0]) != 0:
            raise ValueError("count matrix holds negative, non-finite or non-integer values")
        pack = self._host(t.stack([r["iter"] if r["intercept"] is None else r["intercept"], r["iter"],
                                   r["flag"].to(t.float64)])).numpy()
        return {"rlog": r["rlog"], "intercept": None if intercept is not None else pack[0].copy(), "iter": pack[1].copy(),
                "flag": pack[2].astype(np.int32)}

    def unmix_fit(self, x, pure, alpha=None, shift=None, power=1, maxit=200):
        """the fits of unmix() on the device (csrc/unmix.hip, dsq_unmix_dev) on the current stream: x a resident n x m float64
        handle (what normalized_counts returns) or a host matrix, which goes up once; pure (n x k) goes up; p, loss, iter and
        flag (m x k and three m-vectors) come down in one copy."""
        t = self.torch
        if not isinstance(x, self.native.GeneMajor):
            x = self.matrix(x)
        pure = np.ascontiguousarray(pure, dtype=np.float64)
        k = pure.shape[1]
        r = self._timed("unmix", x.m, lambda: self.native.unmix_dev(
            x, self._vec(pure), alpha=alpha, shift=shift, power=power, maxit=maxit))
        pack = self._host(t.cat([r["p"], r["loss"][:, None], r["iter"].to(t.float64)[:, None],
                                 r["flag"].to(t.float64)[:, None]], dim=1)).numpy()
        return {"p": pack[:, :k].copy(), "loss": pack[:, k].copy(), "iter": pack[:, k + 1].astype(np.int32),
                "flag": pack[:, k + 2].astype(np.int32)}

    def apeglm_fit(self, y, x, nf, disp, coef, no_shrink, prior_scale, prior_df=1.0, no_shrink_scale=15.0, weights=None,
                   init=None, threshold=None, tol=1e-8, maxit=100, sizeFactors=None):
        """the apeglm posterior per gene on the device (csrc/apeglm.hip, dsq_apeglm_dev) on the current stream: y the
        resident counts (or a host matrix, which goes up once), nf a resident matrix or -- with sizeFactors -- the m-vector,
        weights a resident matrix (or host) or None.  What goes up: the design, the dispersions and init; what comes down,
        in one copy: map, sd (n x p) and the six per-gene columns."""
        t = self.torch
        p = np.asarray(x).shape[1]
        if not isinstance(y, self.native.GeneMajor):
            y = self.counts(y) if np.issubdtype(np.asarray(y).dtype, np.integer) else self.matrix(y)
        f = self._sf_dev(sizeFactors) if sizeFactors is not None else (nf if isinstance(nf, self.native.GeneMajor) else self.matrix(nf))
        if weights is not None and not isinstance(weights, self.native.GeneMajor):
            weights = self.matrix(weights)
        bad = t.zeros(2, dtype=t.int32, device=self.device) if y.t.dtype == t.float64 else None
        r = self._timed("apeglm", y.n, lambda: self.native.apeglm_dev(
            y, self.design(x), f, self._vec(disp), coef, no_shrink, prior_scale, prior_df, no_shrink_scale, weights=weights,
            init=None if init is None else self._vec(np.ascontiguousarray(init, dtype=np.float64)), threshold=threshold,
            tol=tol, maxit=maxit, bad=bad))
        if bad is not None and int(self._host(bad)[0]) != 0:
            raise ValueError("count matrix holds negative, non-finite or non-integer values")
        h = self._host(r["_pack"]).numpy()
        out, at, n = {}, 0, y.n
        for k, c in self.native._APEGLM_OUT:
            c = p if c == "p" else c
            out[k] = h[at:at + n * c].reshape((n, c) if c != 1 else (n,)).copy()
            at += n * c
        return out

    def ash_fit(self, betahat, sebetahat, threshold=None, maxit=100):
        """adaptive shrinkage of C independent columns on the device (csrc/ash.hip, dsq_ash_dev) on the current stream:
        betahat / sebetahat resident columns -- a list of C device vectors of n, or one (C, n) device tensor -- or host arrays
        (n or n x C), which go up once.  The call synchronises the stream a few dozen times (the host decides every step of
        the iteration from a small record).  The per-row outputs stay on the device: dict of (C, n) device tensors
        PosteriorMean, PosteriorSD, NegativeProb, PositiveProb, lfsr, le_T, gt_mT, and on the host pi, sd (C x 64), K, iter,
        flag, loglik.  ValueError: a column without a kept row; NotImplementedError: a grid beyond 64 components."""
        t = self.torch
        from . import _lib

        def up(v):
            if isinstance(v, (list, tuple)):
                return t.stack([(e if t.is_tensor(e) else self._vec(np.asarray(e, np.float64))).to(t.float64).reshape(-1)
                                for e in v]).contiguous()
            if t.is_tensor(v):
                return v.to(t.float64).reshape(-1, v.shape[-1]).contiguous()
            a = np.asarray(v, np.float64)
            return self._vec(np.ascontiguousarray(a.reshape(a.shape[0], -1).T))
        b, s = up(betahat), up(sebetahat)
        try:
            r = self._timed("ash", int(b.shape[1]), lambda: self.native.ash_dev(b, s, threshold=threshold, maxit=maxit))
        except _lib.DsqError as e:
            if e.code == _lib.DSQ_ERR_VALUE:
                raise ValueError("ash: no row with a finite estimate and a finite, positive standard error") from e
            if e.code == _lib.DSQ_ERR_UNSUPPORTED:
                raise NotImplementedError(str(e)) from e
            raise
        c = b.shape[0]
        small, ints = self._host(r["_small"]).numpy(), self._host(r["_ints"]).numpy()
        ck = c * _lib.DSQ_ASH_MAX_K
        out = {k: r[k] for k in self.native._ASH_ROWS}
        out.update(pi=small[:ck].reshape(c, -1).copy(), sd=small[ck:2 * ck].reshape(c, -1).copy(), loglik=small[2 * ck:].copy(),
                   K=ints[0].copy(), iter=ints[1].copy(), flag=ints[2].copy())
        return out

    def _resident(self, x):
        return x if isinstance(x, self.native.GeneMajor) else self.matrix(x)

    def row_vars(self, x):
        """(rowMean, rowVar) of a resident n x m float64 handle by row_vars_kernel (csrc/explore.hip, dsq_top_var_dev); the
        two n-vectors come to the host in one copy"""
        x = self._resident(x)
        r = self._timed("top_var", x.n, lambda: self.native.top_var_dev(x, 0))
        h = self._host(r["_pack"]).numpy()
        return h[0].copy(), h[1].copy()

    def top_var(self, x, ntop):
        """the row variances and their top-ntop order on the device (dsq_top_var_dev): the means and variances stay resident;
        the selection and the variances of the selected rows come to the host in one copy"""
        t = self.torch
        x = self._resident(x)
        r = self._timed("top_var", x.n, lambda: self.native.top_var_dev(x, ntop))
        sel = r["select"]
        idx = sel.to(t.int64)
        pack = self._host(t.stack([idx.to(t.float64), r["rowVar"].index_select(0, idx)])).numpy()
        return {"select": pack[0].astype(np.int64), "selVar": pack[1].copy(), "rows": sel,
                "centre": r["rowMean"].index_select(0, idx)}

    def pair_sums(self, x, kind, rows=None, centre=None):
        """the m x m all-pairs sums of a resident n x m float64 handle by pair_sums_kernel (csrc/explore.hip,
        dsq_sample_pairs_dev); rows / centre: device tensors as top_var returns them, or host arrays, which go up; the m x m
        result comes to the host"""
        t = self.torch
        x = self._resident(x)
        if rows is not None and not t.is_tensor(rows):
            rows = t.as_tensor(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
        if centre is not None and not t.is_tensor(centre):
            centre = self._vec(centre)
        out = self._timed("sample_pairs", x.m, lambda: self.native.sample_pairs_dev(x, kind, rows=rows, centre=centre))
        return self._host(out).numpy().copy()

    # ---- collapseReplicates / colSums / fpm / fpkm on the resident counts (csrc/count_helpers.hip): no n x m matrix leaves HBM
    def _csr_dev(self, members, offsets):
        t = self.torch
        return (t.as_tensor(np.ascontiguousarray(members, dtype=np.int32)).to(self.device),
                t.as_tensor(np.ascontiguousarray(offsets, dtype=np.int32)).to(self.device))

    def collapse_columns(self, y, members, offsets):
        """the grouped column sums by collapse_kernel (dsq_collapse_dev): the m + g + 1 indices go up, the n x g count handle
        stays resident, the status word (4 bytes) comes to the host"""
        mt, ot = self._csr_dev(members, offsets)
        out, status = self._timed("collapse", y.n, lambda: self.native.collapse_dev(y, mt, ot))
        return out, int(self._host(status)[0]) & 1

    def collapse_overflow_group(self, y, members, offsets):
        """the first group one of whose sums is no int32, or None: the error path of collapse_columns, in stock tensor
        operations on the resident counts (one flag per group comes to the host)"""
        t = self.torch
        for c in range(len(offsets) - 1):
            idx = t.as_tensor(np.asarray(members[offsets[c]:offsets[c + 1]], np.int64), device=self.device)
            s = y.view().index_select(1, idx).sum(dim=1, dtype=t.int64)
            if bool(((s > 2 ** 31 - 1) | (s < -2 ** 31)).any()):
                return c
        return None

    def col_sums(self, y):
        """colSums of the resident counts by col_sums_kernel (dsq_col_sums_dev): the m int64 sums come to the host"""
        s = self._timed("col_sums", y.n, lambda: self.native.col_sums_dev(y))
        return self._host(s).numpy().copy()

    def fpm_transform(self, y, lib, kind, basepairs=None, txlen=None):
        """fpm / fpkm of the resident counts in one pass (fpm_kernel, dsq_fpm_dev): the m library sizes (and the n feature
        lengths) go up, the n x m result is a handle and stays in HBM.  txlen: a resident n x m handle."""
        bp = None if basepairs is None else self._vec(basepairs)
        tl = None if txlen is None else self._resident(txlen)
        libd = self._vec(lib)
        return self._timed("fpm", y.n, lambda: self.native.fpm_dev(y, libd, kind, basepairs=bp, txlen=tl))

    def sf_iterate_solve(self, y, mu, sf, disp, rows, Q=0.05, maxit=100):
        """the solve of one round of estimateSizeFactorsIterate on the device (csrc/sf_iterate.hip, dsq_sf_iterate_dev) on
        the current stream: y / mu resident handles; sf, disp and the row flags go up; s, sf, F and the three counters come
        down in one copy."""
        t = self.torch
        rv = t.as_tensor(np.ascontiguousarray(np.asarray(rows) != 0, dtype=np.int32)).to(self.device)
        r = self._timed("sf_iterate", y.n, lambda: self.native.sf_iterate_dev(
            y, mu, self._vec(sf), self._vec(np.where(np.asarray(rows) != 0, disp, np.nan)), rv, Q=Q, maxit=maxit))
        m = y.m
        pack = self._host(r["_pack"]).numpy()
        return {"s": pack[:m].copy(), "sf": pack[m:2 * m].copy(), "F": float(pack[2 * m]), "iter": int(pack[2 * m + 1]),
                "evals": int(pack[2 * m + 2]), "flag": int(pack[2 * m + 3])}

    def nf_col_geomeans(self, nf):
        t = self.torch
        return self._host(t.exp(t.log(nf.view()).mean(dim=0))).numpy()

    def weights_prep(self, w, x, thr=1e-2):
        """getAndCheckWeights (R/core.R:2697-2751) in ONE kernel on the resident weights: (w / rowmax, its 1e-6 floor,
        weightsFail flags (int32 device tensor), any-negative flag (int32 device tensor of one element))"""
        from . import _lib
        import ctypes as C
        t = self.torch
        xd = self.design(x)
        wn, wf = t.zeros_like(w.t), t.zeros_like(w.t)
        fz = t.empty(w.n, dtype=t.int32, device=self.device)
        neg = t.zeros(1, dtype=t.int32, device=self.device)
        st = C.c_void_p(t.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().dsq_weights_prep_dev(C.c_void_p(w.t.data_ptr()), C.c_void_p(xd.data_ptr()), w.n, w.m,
                                                   int(np.asarray(x).shape[1]), w.ld, float(thr), C.c_void_p(wn.data_ptr()),
                                                   C.c_void_p(wf.data_ptr()), C.c_void_p(fz.data_ptr()),
                                                   C.c_void_p(neg.data_ptr()), st))
        GM = self.native.GeneMajor
        return GM(wn, w.m), GM(wf, w.m), fz, neg

    def linear_mu(self, y, nf, x_dev):
        dq, da, _ = self._design_qr_dev(x_dev.t().cpu().numpy())
        return self._timed("linear_mu", y.n, lambda: self.native.linearMu_dev(y, nf, dq, da))

    def nbinom_loglike(self, y, mu, disp, weights, useWeights):
        dv = self._vec(disp)
        o = self._timed("nbinom_loglike", y.n, lambda: self.native.nbinomLogLike_dev(y, mu, dv, weights, useWeights))
        return LaunchedVector(lambda: self._host(o).numpy())

    def optim_rows(self, y, nf, x, alpha, lam, weights, useWeights, beta_start, minmu):
        """the handful of rows the IRLS left: gathered rows go through the host-pointer entry point"""
        return self.native.optimRows(self.to_numpy(y), x, self.to_numpy(nf), alpha, lam,
                                     self.to_numpy(weights) if useWeights else None, useWeights, beta_start, minmu)

    def intercept_fit(self, y, nf, alpha, weights, useWeights, mu_floor=0.0, want_hat=True):
        av = self._vec(np.broadcast_to(np.asarray(alpha, float), (y.n,)))
        o = self._timed("intercept_fit", y.n, lambda: self.native.interceptFit_dev(
            y, nf, av, weights, useWeights, mu_floor, want_hat))
        h = self._host(o["_pack"]).numpy()
        return {"beta": h[0], "betaSE": h[1], "mu": o["mu"], "hat_diagonals": o["hat_diagonals"]}

    def parametric_fit(self, means, disps):
        dm, dd = self._vec(means), self._vec(disps)
        return self._timed("trend_fit", int(dm.numel()), lambda: self.native.parametricDispersionFit_dev(dm, dd))

    def local_fit(self, means, disps, minDisp=1e-8):
        """localDispersionFit on the device (csrc/local_fit.hip, dsq_local_fit_dev): means / disps host vectors, which go up,
        or resident ones.  The fit handle stays resident; the status words (16 bytes) come to the host."""
        return DeviceLocalFit(self, means, disps, minDisp)

    def mad(self, v):
        """stats::mad on the device (a sort; selecting order statistics is exact, so the value equals numpy's)"""
        t = self.torch
        x = self._vec(v)

        def med(z):
            s, _ = t.sort(z)
            k = s.numel()
            return s[k // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) * 0.5
        m0 = med(x)
        return float(1.4826 * med((x - m0).abs()))

    def two_sided_normal_p(self, z):
        return self.native.unary("pnorm_upper2", np.asarray(z, np.float64))

    # ---- the beta prior variance: HIP kernels (csrc/beta_prior.hip); one upload, `columns` values back
    def beta_prior_var(self, mle_beta, baseMean, dispFit, allZero, coef_factor, prior_coef_factor=None, prior_coef_src=None):
        """HostEngine.beta_prior_var through dsq_beta_prior_var_dev: the n x p coefficients, baseMean and dispFit go up in
        one copy, the all-zero flags in another; the contrast columns of the expanded matrix are formed on the device"""
        t = self.torch
        mle = np.asarray(mle_beta, np.float64)
        n, p = mle.shape
        dv = self._vec(np.concatenate([mle.T.reshape(-1), np.asarray(baseMean, np.float64).reshape(-1),
                                       np.asarray(dispFit, np.float64).reshape(-1)]))
        az = t.as_tensor(np.ascontiguousarray(np.asarray(allZero) != 0, dtype=np.int32), device=self.device)
        return self.native.estimateBetaPriorVar_dev(dv[:n * p].view(p, n), dv[n * p:n * p + n], dv[n * p + n:], az, coef_factor,
                                                    prior_coef_factor=prior_coef_factor, prior_coef_src=prior_coef_src)

    # ---- results(): HIP kernels (csrc/results.hip) on resident columns; nothing but K cutoffs and counts comes back
    def pt(self, q, df, tail="lower", keep=None, out=None):
        """HostEngine.pt through dsq_pt_dev: q (n, or K x n = n x K column-major), df (n) and keep host arrays or resident
        tensors; returns a resident tensor shaped as q (q itself is not overwritten)"""
        t = self.torch
        col = lambda v: v if t.is_tensor(v) else self._vec(v)
        qd = col(np.asarray(q, np.float64).T if not t.is_tensor(q) and np.ndim(q) == 2 else q)
        kd = None
        if keep is not None:
            kd = keep if t.is_tensor(keep) else t.as_tensor(np.ascontiguousarray((np.asarray(keep) != 0).T, dtype=np.int32), device=self.device)
        od = None
        if keep is not None:
            od = (qd if out is None else col(np.asarray(out, np.float64).T if not t.is_tensor(out) and np.ndim(out) == 2 else out)).clone()
        return self.native.pt_dev(qd, col(df), tail, keep=kd, out=od)

    def results(self, lfc, se, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
                altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1, df=None):
        t = self.torch
        col = lambda v: v if t.is_tensor(v) else self._vec(v)
        flag = lambda v: None if v is None else t.as_tensor(np.ascontiguousarray(np.asarray(v) == 1, dtype=np.int32), device=self.device)
        n = int(np.shape(baseMean)[0])
        r = self._timed("results", n, lambda: self.native.results_dev(
            col(lfc), col(se), col(stat), col(pvalue), col(baseMean), 0, replace=flag(replace), na_mask=flag(na_mask),
            test="Wald", lfcThreshold=lfcThreshold, altHypothesis=altHypothesis, filter=None if filter is None else col(filter),
            theta=None if theta is None else self._vec(theta), alpha=alpha, df=None if df is None else col(df)))
        cutoffs, numRej, status = self.native.results_small(self._host(r["_small"]).numpy(), r["K"])
        if status & 1:
            raise ValueError("filter holds NA")
        if status & 2:
            raise ValueError("theta must lie in [0, 1]")
        tab = ResultColumns({k: r["table"][i] for i, k in enumerate(("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue"))},
                            fetch=lambda v: self._host(v).numpy())
        tab.numRej, tab.cutoffs = numRej, cutoffs
        tab._padj = lambda j: self._host(r["filtPadj"][j]).numpy()
        return tab

    def results_table(self, lfc, se, stat, pvalue, baseMean, replace=None, na_mask=None, lfcThreshold=0.0,
                      altHypothesis="greaterAbs", df=None):
        """(the same launch with one unfiltered column: the table comes with p.adjust(pvalue, "BH"))"""
        return self.results(lfc, se, stat, pvalue, baseMean, replace, na_mask, lfcThreshold, altHypothesis, df=df)

    def filtered_p(self, tab, filter=None, theta=None, alpha=0.1):
        c = tab.resident
        new = self.results(c["log2FoldChange"], c["lfcSE"], c["stat"], c["pvalue"], c["baseMean"], filter=filter, theta=theta,
                           alpha=alpha)
        tab.numRej, tab.cutoffs, tab._padj = new.numRej, new.cutoffs, new._padj
        return tab

    # ---- contrasts: ONE launch of csrc/contrasts.hip on the resident data; the n x K columns stay in HBM
    def contrasts(self, y, x, nf, alpha_hat, beta, lam, contrasts, weights, useWeights, minmu, allZero, sample_mask=None,
                  rule_applies=None, sizeFactors=None, df=None):
        """HostEngine.contrasts through dsq_contrasts_dev.  What goes up: the n-vectors, the n x p coefficients, the
        contrasts and the masks; nothing comes down -- ContrastColumns holds (K, n) device tensors."""
        t = self.torch
        i32 = lambda v: t.as_tensor(np.ascontiguousarray(np.asarray(v) != 0, dtype=np.int32), device=self.device)
        az = i32(allZero)
        mask = rule = None
        if sample_mask is not None:
            K = int(np.shape(sample_mask)[0])
            mask = i32(sample_mask)
            rule = i32(np.ones(K) if rule_applies is None else rule_applies)
        pick = lambda a, k: a[k]
        if contrasts is None:
            r = self._timed("contrasts", y.n, lambda: self.native.contrasts_dev(
                None, None, None, None, None, None, allZero=az, counts=y, sample_mask=mask, rule_applies=rule))
            return ContrastColumns(None, r["contrastAllZero"], pick)
        x = np.ascontiguousarray(x, dtype=np.float64)
        xd = self.design(x)
        n, p = y.n, x.shape[1]
        with np.errstate(invalid="ignore"):
            dv = self._vec(np.concatenate([np.asarray(alpha_hat, np.float64).reshape(-1), np.asarray(lam, np.float64).reshape(-1),
                                           np.asarray(beta, np.float64).T.reshape(-1),
                                           np.asarray(contrasts, np.float64).T.reshape(-1)]))        # one upload
        K = int(np.shape(contrasts)[1])
        av, lv, bv, cv = dv[:n], dv[n:n + p], dv[n + p:n + p + n * p].view(p, n), dv[n + p + n * p:].view(K, p)
        nfh, is_vec = (self._sf_dev(sizeFactors), True) if sizeFactors is not None else (nf, False)
        r = self._timed("contrasts", n, lambda: self.native.contrasts_dev(
            xd, nfh, av, bv, lv, cv, weights=weights, useWeights=useWeights, minmu=minmu, allZero=az, counts=y,
            sample_mask=mask, rule_applies=rule, nf_is_vector=is_vec, cells=self._cells.get(xd.data_ptr()),
            df=None if df is None else self._vec(df)))
        return ContrastColumns(list(r["table"]), r["contrastAllZero"], pick)

    def zero_rule(self, lfc, stat, pvalue, flag):
        t = self.torch
        col = lambda v: v if t.is_tensor(v) else self._vec(v)
        f = flag != 0
        zero, one = t.zeros((), dtype=t.float64, device=self.device), t.ones((), dtype=t.float64, device=self.device)
        return (t.where(f, zero, col(lfc)), t.where(f, zero, col(stat)), t.where(f, one, col(pvalue)))

    # ---- count outliers: HIP kernels (csrc/outlier.hip)
    def cooks_distance(self, y, nf, mu, H, x):
        cells = self.native.cell_index(x)
        p = np.asarray(x).shape[1]
        r = self._timed("cooks_distance", y.n, lambda: self.native.cooksDistance_dev(y, nf, mu, H, cells, p))
        h = self._host(r["_pack"]).numpy()
        return {"cooks": r["cooks"], "maxCooks": h[0], "robustDisp": h[1]}

    def replace_outliers(self, y, nf, cooks, cooksCutoff, replaceable, trim=0.2):
        r = self._timed("replace_outliers", y.n, lambda: self.native.replaceOutliers_dev(
            y, nf, cooks, cooksCutoff, replaceable, trim))
        return {"counts": r["counts"], "replace": self._host(r["replace"]).numpy().astype(bool)}

    def masked_row_max(self, h, use, zero):
        t = self.torch
        z = t.as_tensor(np.asarray(zero, bool), device=self.device)
        u = t.as_tensor(np.asarray(use, bool), device=self.device)
        a = t.where(z[None, :], t.zeros((), dtype=t.float64, device=self.device), h.view())
        return self._host(a[:, u].max(dim=1).values).numpy()      # max is exact: glue, not arithmetic

    # ---- the three native routines
    def fit_beta(self, y, x, nf, alpha_hat, contrast, beta_mat, lam, weights, useWeights, tol, maxit, useQR,
                 minmu, want_mu=True, mu_floor=0.0, want_hat=True):
        t = self.torch
        b0 = beta_mat if t.is_tensor(beta_mat) else self._vec(np.asarray(beta_mat).T)
        n, pp = y.n, len(lam)
        dv = self._vec(np.concatenate([np.broadcast_to(np.asarray(alpha_hat, float), (n,)), contrast, lam]))   # one upload
        av, cv, lv = dv[:n], dv[n:n + pp], dv[n + pp:]
        r = self._timed("fit_beta", y.n, lambda: self.native.fitBeta_dev(
            y, x, nf, av, cv, b0, lv, weights, useWeights, tol, maxit, useQR, minmu, want_hat=want_hat,
            want_mu=want_mu, mu_floor=mu_floor, cells=self._cells.get(x.data_ptr())))
        def fetch():
            h = self._host(r["_pack"]).numpy()           # one device-to-host copy for all per-gene outputs
            p = (h.shape[0] - 4) // 2
            # n x p matrices as column-major VIEWS of the host buffer (what R holds): no transpose copy, and the
            # row scans of fitNbinomGLMs (is.na / <= 0 per row) run along contiguous memory
            return {"beta_mat": h[:p].T, "beta_var_mat": h[p:2 * p].T, "iter": h[2 * p], "deviance": h[2 * p + 3],
                    "contrast_num": h[2 * p + 1].reshape(-1, 1), "contrast_denom": h[2 * p + 2].reshape(-1, 1)}
        return Launched({"hat_diagonals": r["hat_diagonals"], "mu": r["mu"]}, fetch)

    def fit_disp(self, y, x, mu_hat, log_alpha, prior_mean, prior_sigmasq, min_log_alpha, kappa_0, tol, maxit,
                 usePrior, weights, useWeights, weightThreshold, useCR):
        n = y.n
        dv = self._vec(np.concatenate([np.broadcast_to(np.asarray(log_alpha, float), (n,)),
                                       np.broadcast_to(np.asarray(prior_mean, float), (n,))]))    # one upload
        la, pm = dv[:n], dv[n:]
        r = self._timed("fit_disp", n, lambda: self.native.fitDisp_dev(
            y, x, mu_hat, la, pm, prior_sigmasq, min_log_alpha, kappa_0, tol, maxit, usePrior, weights, useWeights,
            weightThreshold, useCR, want_d2lp=self.want_d2lp, cells=self._cells.get(x.data_ptr())))
        def fetch():
            h = self._host(r.pop("_pack"))               # one copy; the views below index the host buffer
            keys = ("log_alpha", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp", "last_d2lp")
            out = {k: h[i].numpy() for i, k in enumerate(keys) if k in r}
            ints = h[len(keys)].view(self.torch.int32)
            out["iter"], out["iter_accept"] = ints[:n].numpy(), ints[n:].numpy()
            return out
        return Launched({}, fetch)

    def fit_disp_grid(self, y, x, mu_hat, disp_grid, prior_mean, prior_sigmasq, usePrior, weights, useWeights,
                      weightThreshold, useCR):
        n = y.n
        pm = self._vec(np.broadcast_to(np.asarray(prior_mean, float), (n,)))
        gv = self._vec(disp_grid)
        r = self._timed("fit_disp_grid", n, lambda: self.native.fitDispGrid_dev(
            y, x, mu_hat, gv, pm, prior_sigmasq, usePrior, weights, useWeights, weightThreshold, useCR,
            cells=self._cells.get(x.data_ptr())))
        return {"log_alpha": self._host(r["log_alpha"]).numpy()}
