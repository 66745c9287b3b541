"""The arithmetic specification of the rlog fit stated in numpy: the reference for the rlog tests.
Not a test itself.  exp / log and the negative binomial log density are the oracle's (oracle.unary, oracle.dnbinom_mu_log:
bit-equal to the device's dexp / dlog / dnbinom_mu_log, tests/test_gpu_math.py); +, -, *, / and max are IEEE, every
operation rounded once, in the order written here; every sum over the samples is a wave-order sum (sf_spec.wave_sum).
Shares no code with the product (deseq2_amd/csrc/rlog.hip, deseq2_amd.engine.HostEngine.rlog_fit, core.rlogData).

rlogData (R/rlog.R:172-272) fits one coefficient per sample under a ridge.  Form A (no intercept given): the design is
[1 | I_m], the normal equations of an IRLS step are an arrow matrix and the step is its Schur complement.  Form B (the
caller's intercept): the design is I_m and the step is elementwise."""
import numpy as np

from tests.sf_spec import wave_sum, _exp, _log

LN2 = float.fromhex("0x1.62e42fefa39efp-1")          # the double nearest to ln 2: R's log(2)
LOG2E = float.fromhex("0x1.71547652b82fep+0")        # R's log2(exp(1))
LARGE = 30.0


def _wsum1(v):
    return float(wave_sum(np.asarray(v, np.float64)[None, :])[0])


def fit_gene(O, y, nf, alpha, lam, lam0, c, tol, maxit, minmu):
    """one gene: counts y (m), factors nf (m), dispersion alpha, the ridges on the natural-log scale; c = None (form A)
    or the intercept of the gene on the log2 scale (form B).  Returns (rlog row, intercept, iter, flag)."""
    m = y.size
    formA = c is None
    with np.errstate(all="ignore"):
        if formA:
            if not (y != 0).any():
                return np.zeros(m), -np.inf, 0.0, 1
            nfe = nf
            beta0 = float(_log(O, np.array([_wsum1(y / nfe) / m]))[0])           # R/fitNbinomGLMs.R:146-151
            beta = np.zeros(m)
        else:
            if not np.isfinite(c):
                return np.zeros(m), np.nan, 0.0, 1
            nfe = nf * float(_exp(O, np.array([c * LN2]))[0])                    # nf * 2^c, R/rlog.R:219
            beta0 = 0.0
            beta = _log(O, y / nfe + 0.1)                                       # R/fitNbinomGLMs.R:144-145, Q = R = I
        size = 1.0 / alpha
        it = 0.0
        dev_old = 0.0
        for t in range(int(maxit)):
            it += 1.0
            eta = beta0 + beta if formA else beta
            mu = np.fmax(nfe * _exp(O, eta), minmu)
            w = mu / (1.0 + alpha * mu)
            z = _log(O, mu / nfe) + (y - mu) / mu
            u = w / (w + lam)
            if formA:
                h = lam * u
                s1 = _wsum1(h)
                s2 = _wsum1(h * z)
                beta0 = s2 / (lam0 + s1)
                beta = u * (z - beta0)
                large = abs(beta0) > LARGE or bool((np.abs(beta) > LARGE).any())
            else:
                beta = u * z
                large = bool((np.abs(beta) > LARGE).any())
            if large:
                it = float(maxit)
                break
            eta = beta0 + beta if formA else beta
            mu = np.fmax(nfe * _exp(O, eta), minmu)
            dev = -2.0 * _wsum1(O.dnbinom_mu_log(y, np.full(m, size), mu))
            conv = abs(dev - dev_old) / (abs(dev) + 0.1)
            if conv != conv:
                it = float(maxit)
                break
            if t > 0 and conv < tol:
                break
            dev_old = dev
        if not (np.isfinite(beta).all() and np.isfinite(beta0)):
            return np.full(m, np.nan), np.nan, it, 2
        if formA:
            return beta0 * LOG2E + beta * LOG2E, beta0 * LOG2E, it, 0
        return beta * LOG2E + c, np.nan, it, 0


def rlog_fit(O, counts, nf, dispFit, betaPriorVar, intercept=None, tol=1e-4, maxit=100, minmu=0.5):
    """dict(rlog n x m, intercept n (form A; NaN in form B), iter n, flag n int32: 0 fitted, 1 all-zero row, 2 a
    non-finite coefficient).  nf: m size factors or an n x m matrix.  betaPriorVar on the log2 scale."""
    K = np.asarray(counts, np.float64)
    n, m = K.shape
    nf = np.asarray(nf, np.float64)
    NF = np.broadcast_to(nf[None, :], (n, m)) if nf.ndim == 1 else nf
    alpha = np.broadcast_to(np.asarray(dispFit, np.float64), (n,))
    ln2sq = LN2 * LN2
    lam = (1.0 / float(betaPriorVar)) / ln2sq                                  # R/rlog.R:243, R/fitNbinomGLMs.R:162
    lam0 = 1e-6 / ln2sq                                                        # R/rlog.R:246
    out = np.zeros((n, m))
    icpt = np.full(n, np.nan)
    it = np.zeros(n)
    flag = np.zeros(n, dtype=np.int32)
    for i in range(n):
        c = None if intercept is None else float(np.asarray(intercept, np.float64)[i])
        if c is not None and not np.isfinite(c):
            c = np.nan                                                          # the all-zero rows of form B
        out[i], icpt[i], it[i], flag[i] = fit_gene(O, np.ascontiguousarray(K[i]), np.ascontiguousarray(NF[i]), float(alpha[i]),
                                                   lam, lam0, c, float(tol), int(maxit), float(minmu))
    return {"rlog": out, "intercept": icpt, "iter": it, "flag": flag}
