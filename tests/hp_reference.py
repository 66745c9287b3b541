"""HIGH-PRECISION REFERENCE -- test infrastructure only.

The per-gene functions of the three native routines at 50 significant digits, written straight from the formulas of
src/DESeq2.cpp (log_posterior :31-64, dlog_posterior :68-107, d2log_posterior :111-158, fitDisp :164-277, fitBeta
:283-465, fitDispGrid :469-513) and of R/core.R (nbinomLogLike :2208-2217, linearModelMuNormalized :2454-2471,
baseMean / baseVar :2138-2146, roughDispEstimate :2422-2437, calculateCooksDistance :2277-2359) and the start values
of R/fitNbinomGLMs.R:139-145.  It shares nothing with the library or with
the oracles: no import from oracle/ or deseq2_amd/, no lgamma restatement, no summation order, no pivoting rule, no
design cells.  Special functions are mpmath's (loggamma / digamma / polygamma at mp.dps = 50); the dense linear algebra
runs in `decimal` at 60 digits (the same precision class, an order of magnitude faster than mpmath's matrices, which
is what lets a 64-column Cox-Reid matrix be factorised at every grid point within a test's seconds).

With maxit = 0 (fitDisp, fitBeta) or maxit = 1 (fitBeta) the routines are closed-form functions of their inputs, so
every output can be compared with the values below at a few units of rounding error -- on every gene, with no
"well-conditioned" mask.  Inputs are the doubles the kernels receive, converted exactly.

Every value comes with the MAGNITUDE M its error budget is built from; a double-precision implementation is held to
    |double - mp| <= K * u * M,    u = 2^-53,
with one constant K per output (BUDGETS below).
  * Sums: M is the sum of the absolute values of every addend of the formula as the reference writes it (each of the
    lgamma / log terms of a sample separately, times its weight), including the alpha^-2, alpha^-3 and final * alpha
    scalings.  A sum of doubles carries an error of a few u per addend magnitude whatever its order; M is its condition.
  * Linear solves: M is the 2-norm condition number kappa of the solved matrix times the magnitude of the result
    (the classical forward bound of a backward-stable solve).  The Cox-Reid terms are functions of b^-1 and det b, so
    their addends enter M times kappa(b) (log det b: an error of kappa u in det b's relative value is kappa u in its log).
    kappa is a magnitude, one digit of it suffices: numpy's SVD of the 60-digit matrix rounded to double.
    (profiles/hp_parity.md derives why these two magnitudes exceed the plain sum of addends.)
  * deviance after one IRLS step is evaluated at mu(beta_1), and beta_1 itself is only known to kappa u |beta_1|: M adds
    |d deviance / d eta_j| * |x_j| * M_beta over the samples (first-order propagation) to the sum of its addends.
"""
import decimal
from decimal import Decimal as D

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
_CTX = decimal.Context(prec=60, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)

# K per output: 4 x the largest ratio |double - mp| / (u M) that the independent numpy restatement (oracle/lapack_oracle.py)
# shows on the cases below (tests/test_hp_reference_cpu.py prints and asserts them), rounded up to a power of
# two.  Why 4 x: the two sides use different lgamma / digamma and different summation orders, each addend carries an ulp
# or two on either side; a missing, doubled or mis-weighted term is off by many orders of magnitude more.
# Measured against lapack_oracle only -- never against the HIP library or the C oracle.
BUDGETS = {
    #                       K        largest lapack_oracle ratio (CPU, every case of DISP_SHAPES / BETA_SHAPES)
    "lp":                   16.0,    # 3.85   (cont-p4-m500)
    "dlp":                  32.0,    # 4.21   (factor-p3-m24-w with useCR off; 4.16 at factor-p10-m255)
    "d2lp":                 8.0,     # 1.46   (cont-p7-m256)
    "beta_step":            32.0,    # 4.71   (cont-p4-m1500)
    "deviance":             4.0,     # 0.998  (cont-p4-m1500)
    "beta_var_mat":         16.0,    # 2.32   (factor-p2-m6)
    "hat_diagonals":        16.0,    # 3.66   (factor-p10-m2000)
    "contrast_num":         4.0,     # 0.988  (cont-p10-m503)
    "contrast_denom":       8.0,     # 1.42   (factor-p10-m2000)
    # the aux routines: against the plain numpy restatement of each in tests/test_hp_reference_cpu.py (np_aux), AUX_SHAPES
    "nbinomLogLike":        8.0,     # 1.06   (m = 7; the direct gammaln form)
    "linearMu":             32.0,    # 6.56   (p = 10, m = 130)
    "baseMean":             16.0,    # 2.27   (p = 3, m = 500, weights)
    "baseVar":              16.0,    # 2.17   (p = 3, m = 500, weights)
    "roughDisp":            8.0,     # 1.61   (p = 3, m = 500, weights)
    "beta_init":            32.0,    # 4.13   (p = 3, m = 500, weights)
    "cooks":                32.0,    # 5.72   (p = 2, m = 1000)
    "maxCooks":             32.0,    # 4.49   (p = 2, m = 1000)
    "robustDisp":           4.0,     # 0.598  (p = 3, m = 12)
}


class Singular(ArithmeticError):
    pass


def _mp(d):
    """Decimal -> mpf (60 -> 50 digits)"""
    return mp.mpf(str(d))


def _dec(v):
    """double -> Decimal, exactly"""
    return D(float(v))


# ---- dense linear algebra at 60 digits -------------------------------------------------------------------------------
def _logdet_spd(a):
    """log det of a symmetric positive definite matrix (list of lists of Decimal) by symmetric elimination.  Any pivot
    order is stable on such a matrix; the sparsest rows go first so that factor-level indicator columns (mutually
    orthogonal) cause no fill-in -- a choice of cost, not of value."""
    q = len(a)
    order = sorted(range(q), key=lambda i: sum(1 for v in a[i] if v != 0))
    A = [[a[i][j] for j in order] for i in order]
    s = D(0)
    for i in range(q):
        piv = A[i][i]
        if not piv > 0:
            raise Singular("pivot %d is %s" % (i, piv))
        s += _CTX.ln(piv)
        row = A[i]
        nz = [r for r in range(i + 1, q) if row[r] != 0]
        for r in nz:
            f = row[r] / piv
            Ar = A[r]
            for c in nz:
                if c >= r:
                    Ar[c] -= f * row[c]
                    A[c][r] = Ar[c]
    return s


def _inverse_spd(a):
    """inverse by Gauss-Jordan on [a | I] (numpy object arrays of Decimal; no pivoting: symmetric positive definite)"""
    q = len(a)
    A = np.empty((q, 2 * q), dtype=object)
    A[:, :] = D(0)
    for i in range(q):
        for j in range(q):
            A[i, j] = a[i][j]
        A[i, q + i] = D(1)
    for i in range(q):
        piv = A[i, i]
        if not piv > 0:
            raise Singular("pivot %d is %s" % (i, piv))
        A[i] = A[i] / piv
        col = A[:, i].copy()
        col[i] = D(0)
        nz = np.flatnonzero(col != 0)
        if nz.size:
            A[nz] = A[nz] - np.outer(col[nz], A[i])
    return [[A[i, q + j] for j in range(q)] for i in range(q)]


def _cond2(a):
    """2-norm condition number as a magnitude (double SVD of the 60-digit matrix)"""
    if len(a) == 0:
        return 1.0
    return float(np.linalg.cond(np.array([[float(v) for v in r] for r in a])))


def _gram_q(rows, d, q):
    """sum_j d_j x_j x_j' (q x q) over sparse rows [(k, x_jk), ...]"""
    g = [[D(0)] * q for _ in range(q)]
    for r, dj in zip(rows, d):
        for a_, xa in r:
            t = xa * dj
            ga = g[a_]
            for b_, xb in r:
                ga[b_] += t * xb
    return g


def _sparse_rows(x, keep, cols):
    idx = {k: i for i, k in enumerate(cols)}
    return [[(idx[k], _dec(x[j, k])) for k in cols if x[j, k] != 0.0] for j in keep]


# ---- the negative binomial log density --------------------------------------------------------------------------------
def nb_logpmf_parts(y, mu, size):
    """addends of log dnbinom(y; mu, size) in the direct form (exact enough at 50 digits even at size 1e9):
    lgamma(y + size) - lgamma(size) - lgamma(y + 1) + size log(size / (size + mu)) + y log(mu / (size + mu))"""
    y = mp.mpf(float(y)); mu = mp.mpf(mu)
    parts = [mp.loggamma(y + size), -mp.loggamma(size), -mp.loggamma(y + 1), size * mp.log(size / (size + mu))]
    if y != 0:
        parts.append(y * mp.log(mu / (size + mu)))
    return parts


def pois_logpmf_parts(y, mu):
    """the Poisson limit (size -> infinity): y log mu - mu - lgamma(y + 1)"""
    y = mp.mpf(float(y)); mu = mp.mpf(mu)
    return ([y * mp.log(mu)] if y != 0 else []) + [-mu, -mp.loggamma(y + 1)]


def nbinomLogLike(y, mu, disp, wts, useWeights):
    """R/core.R:2208-2217: sum_j [w_j] log dnbinom(y_j; mu_j, size = 1 / disp) -> (value, M)"""
    size = 1 / mp.mpf(float(disp))
    val = M = mp.mpf(0)
    for j in range(len(y)):
        w = mp.mpf(float(wts[j])) if useWeights else mp.mpf(1)
        parts = nb_logpmf_parts(y[j], float(mu[j]), size)
        val += w * mp.fsum(parts)
        M += abs(w) * mp.fsum(parts, absolute=True)
    return val, M


# ---- log_posterior and its derivatives ---------------------------------------------------------------------------------
def _cr_setup(log_alpha, mu, x, wts, useWeights, thr):
    """src/DESeq2.cpp:36-45: alpha, the kept samples (w > weightThreshold), the kept (not all-zero) columns, 1/mu + alpha"""
    m, p = x.shape
    alpha = _CTX.exp(_dec(log_alpha))
    if useWeights:
        keep = [j for j in range(m) if float(wts[j]) > thr]
        cols = [k for k in range(p) if any(x[j, k] != 0.0 for j in keep)]
    else:
        keep, cols = list(range(m)), list(range(p))
    rows = _sparse_rows(x, keep, cols)
    base = [1 / _dec(mu[j]) + alpha for j in keep]
    return rows, base, len(cols)


def cr_terms(log_alpha, mu, x, wts, useWeights, thr, order):
    """Cox-Reid term of log_posterior (order 0), dlog_posterior (1) or d2log_posterior (2), each as the reference
    writes it, -> (value, M) with M = kappa(b) * sum |addends|"""
    with decimal.localcontext(_CTX):
        rows, base, q = _cr_setup(log_alpha, mu, x, wts, useWeights, thr)
        if q == 0:
            return mp.mpf(0), mp.mpf(0)              # arma::det of a 0 x 0 matrix is 1; the derivative terms stay 0
        b = _gram_q(rows, [1 / v for v in base], q)
        kap = _cond2(b)
        if order == 0:
            ld = _logdet_spd(b)
            return _mp(-ld / 2), (abs(_mp(ld)) + kap) / 2
        db = _gram_q(rows, [-1 / (v * v) for v in base], q)
        bi = _inverse_spd(b)
        t1 = sum(bi[i][j] * db[j][i] for i in range(q) for j in range(q))
        t1a = sum(abs(bi[i][j] * db[j][i]) for i in range(q) for j in range(q))
        if order == 1:
            return _mp(-t1 / 2), kap * _mp(t1a) / 2                      # -0.5 ddetb / detb, ddetb = detb tr(b^-1 db)
        d2b = _gram_q(rows, [2 / (v * v * v) for v in base], q)
        B, DB = np.array(bi, dtype=object), np.array(db, dtype=object)
        C = B.dot(DB)
        t2 = sum(C[i, j] * C[j, i] for i in range(q) for j in range(q))
        t2a = sum(abs(C[i, j] * C[j, i]) for i in range(q) for j in range(q))
        t3 = sum(bi[i][j] * d2b[j][i] for i in range(q) for j in range(q))
        t3a = sum(abs(bi[i][j] * d2b[j][i]) for i in range(q) for j in range(q))
        # 0.5 (ddetb/detb)^2 - 0.5 d2detb/detb, d2detb = detb (tr^2 - tr(b^-1 db b^-1 db) + tr(b^-1 d2b))
        val = t1 * t1 / 2 - (t1 * t1 - t2 + t3) / 2
        return _mp(val), kap * _mp(t1a * t1a + t2a / 2 + t3a / 2)


class _Memo:
    """function values by double argument: samples that share a count (or a mean) share the evaluation"""
    def __init__(self, fn):
        self.fn, self.d = fn, {}

    def __call__(self, v):
        r = self.d.get(v)
        if r is None:
            r = self.d[v] = self.fn(v)
        return r


def _ll_sum(log_alpha, y, mu, wts, useWeights, order, want_M=True):
    """the likelihood sums of :47-58 (order 0), :88-98 (1: sum w t1) and :136-147 (2: sum w t2) -> (value, M)"""
    alpha = mp.exp(mp.mpf(float(log_alpha)))
    an1 = 1 / alpha
    if order == 0:
        lg0 = mp.loggamma(an1)
        fy = _Memo(lambda yv: mp.loggamma(yv + an1))
        fm = _Memo(lambda mv: (mp.log(mv + an1), an1 * mp.log(1 + mv * alpha)))
    elif order == 1:
        dg0 = mp.digamma(an1)
        fy = _Memo(lambda yv: mp.digamma(yv + an1))
        fm = _Memo(lambda mv: (mp.log(1 + mv * alpha), mv * alpha / (1 + mv * alpha), mv + an1))
    else:
        an2 = alpha ** -2
        tg0 = an2 * mp.polygamma(1, an1)
        fy = _Memo(lambda yv: an2 * mp.polygamma(1, yv + an1))
        fm = _Memo(lambda mv: (mv ** 2 * alpha * (1 + mv * alpha) ** -2, (mv + an1) ** -2))
    val = M = mp.mpf(0)
    for j in range(len(y)):
        yj, mj = float(y[j]), float(mu[j])
        w = mp.mpf(float(wts[j])) if useWeights else mp.mpf(1)
        if order == 0:
            l1, l2 = fm(mj)
            parts = (fy(yj), -lg0, -yj * l1, -l2)
        elif order == 1:
            l1, r1, den = fm(mj)
            parts = (dg0, l1, -r1, -fy(yj), yj / den)
        else:
            r2, den2 = fm(mj)
            parts = (-tg0, r2, fy(yj), an2 * yj * den2)
        t = parts[0] + parts[1] + parts[2] + parts[3]
        if order == 1:
            t += parts[4]
        val += w * t
        if want_M:
            M += abs(w) * mp.fsum(parts, absolute=True)
    return val, M


def log_posterior(log_alpha, y, mu, x, prior_mean, prior_sigmasq, usePrior, wts, useWeights, weightThreshold, useCR,
                  want_M=True):
    """src/DESeq2.cpp:31-64 -> (value, M)"""
    val, M = _ll_sum(log_alpha, y, mu, wts, useWeights, 0, want_M)
    if usePrior:
        pp = -(mp.mpf(float(log_alpha)) - mp.mpf(float(prior_mean))) ** 2 / (2 * mp.mpf(float(prior_sigmasq)))
        val += pp; M += abs(pp)
    if useCR:
        c, Mc = cr_terms(log_alpha, mu, x, wts, useWeights, weightThreshold, 0)
        val += c; M += Mc
    return val, M


def dlog_posterior(log_alpha, y, mu, x, prior_mean, prior_sigmasq, usePrior, wts, useWeights, weightThreshold, useCR):
    """src/DESeq2.cpp:68-107: (alpha^-2 sum w t + cr_term) * alpha + prior_part -> (value, M)"""
    alpha = mp.exp(mp.mpf(float(log_alpha)))
    s, Ms = _ll_sum(log_alpha, y, mu, wts, useWeights, 1)
    val, M = alpha ** -2 * s, alpha ** -2 * Ms
    if useCR:
        c, Mc = cr_terms(log_alpha, mu, x, wts, useWeights, weightThreshold, 1)
        val += c; M += Mc
    val, M = val * alpha, M * alpha
    if usePrior:
        pp = -(mp.mpf(float(log_alpha)) - mp.mpf(float(prior_mean))) / mp.mpf(float(prior_sigmasq))
        val += pp; M += abs(pp)
    return val, M


def d2log_posterior(log_alpha, y, mu, x, prior_mean, prior_sigmasq, usePrior, wts, useWeights, weightThreshold, useCR,
                    inner=None):
    """src/DESeq2.cpp:111-158: (ll_part + cr_term) alpha^2 + dlog_posterior(usePrior = false) [:156] + prior_part
    (inner: that dlog_posterior value and its M, where the caller already has them)"""
    alpha = mp.exp(mp.mpf(float(log_alpha)))
    s1, M1 = _ll_sum(log_alpha, y, mu, wts, useWeights, 1)
    s2, M2 = _ll_sum(log_alpha, y, mu, wts, useWeights, 2)
    val = -2 * alpha ** -3 * s1 + alpha ** -2 * s2
    M = 2 * alpha ** -3 * M1 + alpha ** -2 * M2
    if useCR:
        c, Mc = cr_terms(log_alpha, mu, x, wts, useWeights, weightThreshold, 2)
        val += c; M += Mc
    val, M = val * alpha ** 2, M * alpha ** 2
    inner, Mi = inner or dlog_posterior(log_alpha, y, mu, x, prior_mean, prior_sigmasq, False, wts, useWeights,
                                        weightThreshold, useCR)
    val += inner; M += Mi
    if usePrior:
        pp = -1 / mp.mpf(float(prior_sigmasq))
        val += pp; M += abs(pp)
    return val, M


def fit_disp_frozen(log_alpha, y, mu, x, prior_mean, prior_sigmasq, wts, useWeights, weightThreshold, useCR):
    """fitDisp at maxit = 0 (src/DESeq2.cpp:164-277) for the prior off and on, sharing the evaluations (the prior is an
    additive term): {usePrior: {"lp": (v, M), "dlp": (v, M), "d2lp": (v, M)}}"""
    rest = (y, mu, x, prior_mean, prior_sigmasq, False, wts, useWeights, weightThreshold, useCR)
    off = {"lp": log_posterior(log_alpha, *rest), "dlp": dlog_posterior(log_alpha, *rest)}
    off["d2lp"] = d2log_posterior(log_alpha, *rest, inner=off["dlp"])
    la, pm, sg = mp.mpf(float(log_alpha)), mp.mpf(float(prior_mean)), mp.mpf(float(prior_sigmasq))
    pri = {"lp": -(la - pm) ** 2 / (2 * sg), "dlp": -(la - pm) / sg, "d2lp": -1 / sg}
    on = {k: (off[k][0] + pri[k], off[k][1] + abs(pri[k])) for k in off}
    return {False: off, True: on}


def fit_disp_grid(y, mu, x, grid, prior_mean, prior_sigmasq, wts, useWeights, weightThreshold, useCR):
    """fitDispGrid (src/DESeq2.cpp:469-513) for the prior off and on: the argmax of log_posterior over the coarse grid,
    then over the fine grid around it.  {usePrior: (log_alpha, [(gap, M) per stage])} with gap = the difference between
    the best and the second-best log_posterior of the stage and M the magnitude of the best one.  The grid points are
    the doubles the routine forms: grid[k], and a_hat - delta + k * (2 delta / (ngrid - 1)) in double arithmetic."""
    grid = np.asarray(grid, float)
    delta = grid[1] - grid[0]
    ll = _Memo(lambda a: _grid_point(a, y, mu, x, wts, useWeights, weightThreshold, useCR))
    out = {}
    for usePrior in (False, True):
        def lp(a):
            v, M = ll(float(a))
            if usePrior:
                pp = -(mp.mpf(float(a)) - mp.mpf(float(prior_mean))) ** 2 / (2 * mp.mpf(float(prior_sigmasq)))
                v, M = v + pp, M + abs(pp)
            return v, M
        stages, pts = [], grid
        for _stage in range(2):
            vals = [lp(a) for a in pts]
            order = sorted(range(len(pts)), key=lambda k: vals[k][0], reverse=True)
            best = order[0]
            M = _grid_point(float(pts[best]), y, mu, x, wts, useWeights, weightThreshold, useCR, True)[1]
            if usePrior:                                  # (lp() ran without magnitudes: M is taken once, here)
                M += abs((mp.mpf(float(pts[best])) - mp.mpf(float(prior_mean))) ** 2 / (2 * mp.mpf(float(prior_sigmasq))))
            stages.append((vals[best][0] - vals[order[1]][0], M))
            a_hat = pts[best]
            pts = fine_grid(a_hat, delta, grid.size)
        out[usePrior] = (float(a_hat), stages)
    return out


def fine_grid(a_hat, delta, ngrid):
    """the fine grid of :503 as doubles (arma::linspace: start + k * step, the last point the end itself)"""
    lo, hi = a_hat - delta, a_hat + delta
    step = (hi - lo) / (ngrid - 1.0)
    return np.array([lo + k * step for k in range(ngrid - 1)] + [hi])


def _grid_point(a, y, mu, x, wts, useWeights, weightThreshold, useCR, want_M=False):
    return log_posterior(a, y, mu, x, 0.0, 1.0, False, wts, useWeights, weightThreshold, useCR, want_M)


# ---- fitBeta -------------------------------------------------------------------------------------------------------------
def _mu_of(beta, x, nf, minmu):
    """mu = max(nf exp(x beta), minmu), Decimal"""
    m, p = x.shape
    out = []
    for j in range(m):
        eta = sum((_dec(x[j, k]) * beta[k] for k in range(p) if x[j, k] != 0.0), D(0))
        out.append(max(_dec(nf[j]) * _CTX.exp(eta), _dec(minmu)))
    return out


def _wvec(mu, alpha, wts, useWeights):
    a = _dec(alpha)
    return [(_dec(wts[j]) * v if useWeights else v) / (1 + a * v) for j, v in enumerate(mu)]


def irls_step(y, x, nf, alpha, beta0, lam, wts, useWeights, minmu):
    """one IRLS step of src/DESeq2.cpp:318-353 as the exact solution of (X'WX + Lambda) beta = X'W z, mu floored at minmu
    (QR of [sqrt(W) X; sqrt(Lambda)] and the normal equations are the same mathematical solution)
    -> (beta_1 [mp], M_beta = kappa(A) * max |beta_1|, mu(beta_1) [Decimal], beta_1 [Decimal])"""
    m, p = x.shape
    with decimal.localcontext(_CTX):
        b0 = [_dec(v) for v in beta0]
        mu = _mu_of(b0, x, nf, minmu)
        w = _wvec(mu, alpha, wts, useWeights)
        z = [_CTX.ln(mu[j] / _dec(nf[j])) + (_dec(y[j]) - mu[j]) / mu[j] for j in range(m)]
        rows = _sparse_rows(x, range(m), range(p))
        A = _gram_q(rows, w, p)
        for k in range(p):
            A[k][k] += _dec(lam[k])
        rhs = [D(0)] * p
        for r, wj, zj in zip(rows, w, z):
            for k, xv in r:
                rhs[k] += xv * wj * zj
        Ai = _inverse_spd(A)
        b1 = [sum(Ai[k][l] * rhs[l] for l in range(p)) for k in range(p)]
        kap = _cond2(A)
        mu1 = _mu_of(b1, x, nf, minmu)
        return [_mp(v) for v in b1], kap * max(abs(float(v)) for v in b1), mu1, b1


def deviance_after_step(y, x, nf, alpha, wts, useWeights, minmu, mu1, M_beta):
    """-2 sum [w] log dnbinom(y; mu(beta_1), 1/alpha) (src/DESeq2.cpp:362-373) -> (value, M): the sum of the addends'
    magnitudes plus the first-order effect of beta_1's own uncertainty M_beta (module docstring)"""
    size = 1 / mp.mpf(float(alpha))
    val = M = mp.mpf(0)
    a = float(alpha)
    for j in range(len(y)):
        w = mp.mpf(float(wts[j])) if useWeights else mp.mpf(1)
        mj = _mp(mu1[j])
        parts = nb_logpmf_parts(y[j], mj, size)
        val += -2 * w * mp.fsum(parts)
        M += 2 * abs(w) * mp.fsum(parts, absolute=True)
        if mu1[j] > _dec(minmu):                      # d/d eta of -2 w log f = -2 w (y - mu) / (1 + alpha mu)
            g = 2 * float(w) * abs(float(y[j]) - float(mj)) / (1 + a * float(mj))
            M += g * float(np.abs(x[j]).sum()) * M_beta
    return val, M


def fit_beta_post(y, x, nf, alpha, contrast, beta, lam, wts, useWeights, minmu):
    """the post-fit quantities of src/DESeq2.cpp:376-465 at the given beta (what fitBeta returns at maxit = 0):
    Sigma = A^-1 X'WX A^-1 with A = X'WX + Lambda, its diagonal, the hat diagonals w_j x_j' A^-1 x_j, c'beta and
    sqrt(c' Sigma c).  {name: (values, M)}; M = kappa(A) * |value| for what passes through A^-1 (for the diagonal of
    Sigma: times its largest entry), the sum of |c_k beta_k| for contrast_num."""
    m, p = x.shape
    with decimal.localcontext(_CTX):
        b = [_dec(v) for v in beta]
        mu = _mu_of(b, x, nf, minmu)
        w = _wvec(mu, alpha, wts, useWeights)
        rows = _sparse_rows(x, range(m), range(p))
        G = _gram_q(rows, w, p)
        A = [r[:] for r in G]
        for k in range(p):
            A[k][k] += _dec(lam[k])
        kap = _cond2(A)
        Ai = np.array(_inverse_spd(A), dtype=object)
        S = Ai.dot(np.array(G, dtype=object)).dot(Ai)
        hat = []
        for r, wj in zip(rows, w):
            hat.append(wj * sum(xa * Ai[a_, b_] * xb for a_, xa in r for b_, xb in r))
        c = [_dec(v) for v in contrast]
        num = sum(c[k] * b[k] for k in range(p))
        num_M = sum(abs(c[k] * b[k]) for k in range(p))
        den = _CTX.sqrt(sum(c[k] * S[k, l] * c[l] for k in range(p) for l in range(p)))
        var = [S[k, k] for k in range(p)]
        vmax = max(abs(float(v)) for v in var)
        return {"beta_var_mat": ([_mp(v) for v in var], [kap * vmax] * p),
                "hat_diagonals": ([_mp(v) for v in hat], [kap * abs(float(v)) for v in hat]),
                "contrast_num": ([_mp(num)], [float(num_M)]),
                "contrast_denom": ([_mp(den)], [kap * float(den)]),
                "mu": mu}


# ---- the cases -------------------------------------------------------------------------------------------------------------
LOG_ALPHAS = np.log([1e-8, 1e-6, 1e-4, 0.05, 1.0, 10.0])
WEIGHT_THRESHOLD = 1e-2


def n_genes(m):
    return 4 if m >= 2000 else 8 if m > 1000 else 16


def design(kind, p, m, seed):
    if kind == "factor":                                  # one factor of p levels: p design cells
        grp = (np.arange(m) * p) // m
        return np.column_stack([np.ones(m)] + [(grp == g).astype(float) for g in range(1, p)])
    if kind == "cont":                                    # a (p - 1)-level factor and one continuous covariate: no cells
        grp = (np.arange(m) * (p - 1)) // m
        z = np.random.default_rng(seed).normal(0.0, 0.5, m)
        return np.column_stack([np.ones(m)] + [(grp == g).astype(float) for g in range(1, p - 1)] + [z])
    if kind == "paired":                                  # ~ patient + treatment: p - 1 patients, 2 (p - 1) cells
        assert m == 2 * (p - 1)
        pat = np.repeat(np.arange(p - 1), 2)
        return np.column_stack([np.ones(m)] + [(pat == k).astype(float) for k in range(1, p - 1)]
                               + [np.tile([0.0, 1.0], p - 1)])
    raise ValueError(kind)


def make_case(kind, p, m, weights=False, seed=None, big_every=1):
    """one case of the frozen-iteration tests: NB draws with means spread over exp(N(4, 1.5)); in every gene one block
    of all-zero samples and one count >= 2^20; log_alpha cycling from the 1e-8 floor to 10.  With weights: whole
    samples at zero, a weight equal to weightThreshold in every gene, and in every second gene a whole (non-reference)
    level below the threshold, so that a column of the Cox-Reid matrix is dropped and the matrix stays non-singular.
    big_every = 2 (the fitBeta cases): the 2^20 count in every second gene only -- one IRLS step from the least-squares
    start values throws such a row out of the |beta| <= 30 box, where the routine returns before it takes the deviance
    (src/DESeq2.cpp:355-358): those rows pin beta_1 and the exit (iter = maxit, deviance = 0), the others the deviance."""
    seed = 1000 * p + m if seed is None else seed
    rng = np.random.default_rng(seed)
    n = n_genes(m)
    x = design(kind, p, m, seed)
    beta = np.column_stack([rng.normal(4.0, 1.5, n)] + [rng.normal(0.0, 0.5, n) for _ in range(p - 1)])
    nf = np.exp(rng.normal(0.0, 0.2, (n, m))) if m <= 600 else np.ones((n, m))
    mu_true = nf * np.exp(beta @ x.T)
    size = 1.0 / 0.2
    y = rng.negative_binomial(size, size / (size + mu_true)).astype(np.int32)
    blk = max(1, m // 8)
    for i in range(n):
        lo = int(rng.integers(0, m - blk + 1))
        y[i, lo:lo + blk] = 0
        free = np.setdiff1d(np.arange(m), np.arange(lo, lo + blk))
        big = rng.choice(free)
        if i % big_every == 0:
            y[i, big] = 2 ** 20 + int(rng.integers(0, 1000))
    la = LOG_ALPHAS[np.arange(n) % LOG_ALPHAS.size].copy()
    w = np.ones((n, m))
    if weights:
        w = rng.uniform(0.05, 1.0, (n, m))
        w[:, rng.choice(m, max(1, m // 12), replace=False)] = 0.0                  # whole samples at zero
        w = w / w.max(axis=1, keepdims=True)                                        # R/core.R:2702
        for i in range(n):
            live = np.flatnonzero(w[i] > 0.5)
            w[i, rng.choice(live)] = WEIGHT_THRESHOLD                               # a weight EQUAL to the threshold
            if kind == "factor" and i % 2 == 1:
                w[i, x[:, 1] == 1.0] = 0.005                                        # level 1 below the threshold
        w[:, 0] = 1.0
    mu = np.maximum(mu_true, 0.5)
    # start values of R/fitNbinomGLMs.R:139-145 (inputs, not results: plain numpy)
    q, r = np.linalg.qr(x)
    beta_start = np.linalg.solve(r, q.T @ np.log(y / nf + 0.1).T).T.copy()
    beta_drawn = beta_start + rng.normal(0.0, 0.1, beta_start.shape)
    lam = np.where(np.arange(p) % 2 == 0, 1e-6 / np.log(2) ** 2, 0.5)            # both ridge values in one call
    contrast = np.zeros(p); contrast[0] = 1.0; contrast[p - 1] = -1.0
    return dict(kind=kind, p=p, m=m, n=n, x=x, y=y, nf=nf, mu=mu, log_alpha=la, prior_mean=la - 0.1, sigmasq=0.8,
                weights=w, useWeights=bool(weights), beta_start=beta_start, beta_drawn=beta_drawn, lam=lam,
                contrast=contrast, grid=np.linspace(np.log(1e-8), np.log(max(10, m)), 12), minmu=0.5)


# (kind, p, m, weights) -- the shapes of the issue's tables; test_gpu_hp.py's docstring says which kernel each reaches
DISP_SHAPES = [
    ("factor", 2, 6, False), ("factor", 3, 64, False), ("factor", 3, 65, False), ("factor", 10, 130, False),
    ("factor", 10, 255, False), ("factor", 10, 256, False), ("factor", 10, 2560, False), ("factor", 10, 2561, False),
    ("factor", 10, 2000, False), ("factor", 3, 1500, True),
    ("factor", 3, 24, True), ("factor", 2, 16, True),
    ("cont", 5, 40, False), ("cont", 4, 500, False),
    ("cont", 7, 256, False), ("cont", 7, 257, False), ("cont", 10, 1024, False), ("cont", 10, 1025, False),
    ("cont", 12, 60, False), ("paired", 31, 60, False), ("factor", 48, 96, False), ("factor", 64, 130, True),
]
BETA_SHAPES = [
    ("factor", 2, 6, False), ("factor", 3, 500, False), ("factor", 10, 2000, False), ("factor", 3, 37, True),
    ("cont", 4, 100, False), ("cont", 4, 1500, False),
    ("cont", 7, 249, False), ("cont", 7, 250, False), ("cont", 10, 502, False), ("cont", 10, 503, False),
    ("cont", 10, 600, False), ("cont", 10, 2000, False),
    ("cont", 12, 60, False), ("paired", 31, 60, False), ("factor", 48, 96, False), ("factor", 64, 130, False),
]


def shape_id(s):
    return "%s-p%d-m%d%s" % (s[0], s[1], s[2], "-w" if s[3] else "")


_REF_CACHE = {}


def disp_reference(shape, useCR=True):
    """the mp side of one fitDisp / fitDispGrid case, computed once per process: (case, frozen[i][usePrior][key],
    grid[i][usePrior])"""
    key = ("disp", shape, useCR)
    if key not in _REF_CACHE:
        c = make_case(*shape)
        fro, grd = [], []
        for i in range(c["n"]):
            a = (c["y"][i], c["mu"][i], c["x"], c["prior_mean"][i], c["sigmasq"], c["weights"][i], c["useWeights"],
                 WEIGHT_THRESHOLD, useCR)
            fro.append(fit_disp_frozen(c["log_alpha"][i], *a))
            grd.append(fit_disp_grid(c["y"][i], c["mu"][i], c["x"], c["grid"], *a[3:]))
        _REF_CACHE[key] = (c, fro, grd)
    return _REF_CACHE[key]


def beta_reference(shape):
    """the mp side of one fitBeta case: (case, post[i] at beta_drawn (maxit = 0), step[i] = (beta_1, M_beta, (dev, M_dev))
    from beta_start (maxit = 1); no deviance (None) where beta_1 leaves the box)"""
    key = ("beta", shape)
    if key not in _REF_CACHE:
        c = make_case(*shape, big_every=2)
        post, step = [], []
        for i in range(c["n"]):
            alpha = float(np.exp(c["log_alpha"][i]))
            a = (c["y"][i], c["x"], c["nf"][i], alpha)
            post.append(fit_beta_post(*a, c["contrast"], c["beta_drawn"][i], c["lam"], c["weights"][i], c["useWeights"],
                                      c["minmu"]))
            b1, Mb, mu1, _ = irls_step(*a, c["beta_start"][i], c["lam"], c["weights"][i], c["useWeights"], c["minmu"])
            large = any(abs(v) > 30 for v in b1)                  # :355-358: iter = maxit and out, deviance still 0
            dev = None if large else deviance_after_step(c["y"][i], c["x"], c["nf"][i], alpha, c["weights"][i],
                                                         c["useWeights"], c["minmu"], mu1, Mb)
            step.append((b1, Mb, dev))
        _REF_CACHE[key] = (c, post, step)
    return _REF_CACHE[key]


# ---- the O(n m) steps around the fits --------------------------------------------------------------------------------------
# The kernels take Q, A = X R^-1 and R of the thin QR of the model matrix as INPUTS (stats::qr on the host, as in the
# reference): the statements below are functions of those doubles, like every other input converted exactly.
def _f(v):
    return mp.mpf(float(v))


def linear_mu(y, nf, q, a, mu_floor=0.0, yn=None):
    """linearModelMuNormalized (R/core.R:2454-2471): mu_j = nf_j * sum_k (sum_l (y_l / nf_l) Q_lk) A_jk, floored at
    mu_floor when > 0 (:763).  -> (values, M): M_j = nf_j * sum_k (sum_l |y_l / nf_l Q_lk|) |A_jk|, the addends' magnitudes"""
    m, p = q.shape
    yn = [_f(y[j]) / _f(nf[j]) for j in range(m)] if yn is None else yn
    t = [mp.fsum(yn[l] * _f(q[l, k]) for l in range(m)) for k in range(p)]
    ta = [mp.fsum(abs(yn[l] * _f(q[l, k])) for l in range(m)) for k in range(p)]
    vals, Ms = [], []
    for j in range(m):
        v = _f(nf[j]) * mp.fsum(t[k] * _f(a[j, k]) for k in range(p))
        M = _f(nf[j]) * mp.fsum(ta[k] * abs(_f(a[j, k])) for k in range(p))
        if mu_floor > 0 and v < mu_floor:
            v = mp.mpf(mu_floor)
        vals.append(v); Ms.append(max(M, abs(v)))
    return vals, Ms


def _mean_var(v):
    """row mean and row variance of the mp values v -> ((mean, M), (var, M)), the magnitudes of prefit_moments' docstring"""
    m = len(v)
    mean = mp.fsum(v) / m
    sq = mp.fsum((t - mean) ** 2 for t in v)
    Mvar = (sq + 2 * mp.fsum(abs(t - mean) * (abs(t) + abs(mean)) for t in v)) / (m - 1)
    return (mean, mp.fsum(abs(t) for t in v) / m), (sq / (m - 1), Mvar)


def prefit_moments(y, nf, q, a, r, wts, useWeights):
    """baseMean, baseVar, allZero (R/core.R:2138-2146: row mean and row variance of the [weighted] normalized counts),
    roughDispEstimate (:2422-2437, on the normalized counts, mu = pmax(1, linearModelMu)) and the start values
    solve(R, Q' log(yn + 0.1)) (R/fitNbinomGLMs.R:139-145).  {name: (values, M)}.
    M: baseMean sum |v| / m; baseVar the squares plus what the rounding of each v - mean moves them by,
    [sum (v - mean)^2 + 2 sum |v - mean| (|v| + |mean|)] / (m - 1); roughDisp the addends' magnitudes plus
    |d addend / d mu_j| M_mu_j for the unfloored mu_j; beta_init kappa_2(R) max |beta| + |R^-1| (|Q|' |log(yn + 0.1)|)."""
    m, p = q.shape
    yn = [_f(y[j]) / _f(nf[j]) for j in range(m)]
    v = [_f(wts[j]) * yn[j] for j in range(m)] if useWeights else yn
    (mean, Mmean), (var, Mvar) = _mean_var(v)
    mu, Mmu = linear_mu(None, np.ones(m), q, a, yn=yn)
    est = Mest = mp.mpf(0)
    for j in range(m):
        floored = mu[j] < 1
        mj = mp.mpf(1) if floored else mu[j]
        d = yn[j] - mj
        est += (d * d - mj) / mj ** 2
        Mest += (d * d + mj) / mj ** 2
        if not floored:
            Mest += abs((-2 * d * mj + mj - 2 * d * d) / mj ** 3) * Mmu[j]
    est, Mest = est / (m - p), Mest / (m - p)
    ly = [mp.log(t + mp.mpf("0.1")) for t in yn]
    u = [mp.fsum(ly[j] * _f(q[j, k]) for j in range(m)) for k in range(p)]
    ua = [mp.fsum(abs(ly[j] * _f(q[j, k])) for j in range(m)) for k in range(p)]
    R = mp.matrix([[_f(r[i, k]) for k in range(p)] for i in range(p)])
    Ri = mp.inverse(R)
    beta = [mp.fsum(Ri[k, l] * u[l] for l in range(p)) for k in range(p)]
    kap = float(np.linalg.cond(np.asarray(r, float)))
    bmax = max(abs(b) for b in beta)
    Mb = [kap * bmax + mp.fsum(abs(Ri[k, l]) * ua[l] for l in range(p)) for k in range(p)]
    return {"baseMean": ([mean], [Mmean]), "baseVar": ([var], [Mvar]),
            "roughDisp": ([max(est, mp.mpf(0))], [Mest]), "beta_init": (beta, Mb),
            "allZero": all(float(t) == 0.0 for t in y)}


def _trimmed_mean(vals, trim):
    """R's mean(x, trim): the mean of sort(x)[lo:hi], lo = floor(n trim) + 1, hi = n + 1 - lo -> (value, sum |.| / k)"""
    n = len(vals)
    lo = int(mp.floor(n * trim))
    s = sorted(vals)[lo:n - lo]
    return mp.fsum(s) / len(s), mp.fsum(abs(t) for t in s) / len(s), s


def cooks_distance(y, nf, mu, H, x):
    """calculateCooksDistance (R/core.R:2333-2340) with robustMethodOfMomentsDisp (:2277-2299), trimmedCellVariance
    (:2301-2324), trimmedVariance (:2326-2331) and recordMaxCooks (:2349-2359).  {name: (values, M)}.
    M of cooks_j: the value itself (a product of well-conditioned factors: a few u relative) plus what the robust
    dispersion's own magnitude M_alpha moves it by, cooks_j * mu_j^2 / V_j * M_alpha; M_alpha from the two sums it
    is the difference of, (M_v + M_mean (1 + 2 |v - mean| / mean)) / mean^2, zero where alpha sits on its 0.04 floor."""
    m, p = x.shape
    cn = [_f(y[j]) / _f(nf[j]) for j in range(m)]
    _, cell = np.unique(np.asarray(x, float), axis=0, return_inverse=True)
    cell = cell.reshape(-1)
    sizes = np.bincount(cell)
    big = [c for c in range(sizes.size) if sizes[c] >= 3]
    trimratio, scale = [mp.mpf(1) / 3, mp.mpf(1) / 4, mp.mpf(1) / 8], [mp.mpf("2.04"), mp.mpf("1.86"), mp.mpf("1.51")]

    def tvar(vals, k):
        cm, cma, _ = _trimmed_mean(vals, trimratio[k])
        sq = [(t - cm) ** 2 for t in vals]
        ve, _, kept = _trimmed_mean(sq, trimratio[k])
        # the kept squares, and the rounding of each difference under them: 2 |d| (|t| + |cm|) >= 2 sqrt(sq) cma
        Mv = scale[k] * (ve + 2 * mp.fsum(mp.sqrt(t) for t in kept) / len(kept) * 2 * max(cma, mp.mpf(0)))
        return scale[k] * ve, Mv
    if big:
        cands = []
        for c in big:
            nc = int(sizes[c])
            k = 0 if nc <= 3.5 else 1 if nc <= 23.5 else 2
            cands.append(tvar([cn[j] for j in range(m) if cell[j] == c], k))
        v, Mv = max(cands, key=lambda t: t[0])
    else:
        v, Mv = tvar(cn, 2)
    mean = mp.fsum(cn) / m
    raw = (v - mean) / mean ** 2
    floor = mp.mpf("0.04")
    if raw > floor:
        alpha, Ma = raw, (Mv + mean * (1 + 2 * abs(v - mean) / mean)) / mean ** 2
    else:
        alpha, Ma = floor, mp.mpf(0)
    cooks, Mc = [], []
    for j in range(m):
        mj, hj = _f(mu[j]), _f(H[j])
        V = mj + alpha * mj ** 2
        c = (_f(y[j]) - mj) ** 2 / V / p * hj / (1 - hj) ** 2
        cooks.append(c); Mc.append(abs(c) * (1 + mj ** 2 / V * Ma))
    keep = [j for j in range(m) if sizes[cell[j]] >= 3]
    if m > p and keep:
        jm = max(keep, key=lambda j: cooks[j])
        mx = ([cooks[jm]], [Mc[jm]])
    else:
        mx = None                                           # NA
    return {"cooks": (cooks, Mc), "maxCooks": mx, "robustDisp": ([alpha], [max(Ma, alpha)])}


def design_qr(x):
    """thin QR of the model matrix as doubles (inputs of the aux kernels): Q, A = X R^-1, R"""
    q, r = np.linalg.qr(np.asarray(x, float))
    return q, np.asarray(x, float) @ np.linalg.inv(r), r


# (name, kind, p, m, weights): the aux cases of the issue; genes as n_genes(m)
AUX_SHAPES = [("nbinomLogLike", "factor", 2, 7, False), ("nbinomLogLike", "factor", 2, 1500, True),
              ("linearMu", "factor", 3, 24, False), ("linearMu", "factor", 10, 130, False), ("linearMu", "factor", 3, 500, False),
              ("prefitMoments", "factor", 2, 6, False), ("prefitMoments", "factor", 3, 500, True),
              ("cooksDistance", "factor", 3, 12, False), ("cooksDistance", "factor", 2, 1000, False)]


def aux_id(s):
    return "%s-p%d-m%d%s" % (s[0], s[2], s[3], "-w" if s[4] else "")


def aux_reference(shape):
    """(case, per-gene mp results) of one aux case.  cooksDistance: mu and H are the doubles nearest the mp statement of
    a maxit = 0 fit at beta_drawn (fit_beta_post), not an oracle's."""
    key = ("aux", shape)
    if key not in _REF_CACHE:
        name, kind, p, m, w = shape
        # (cooksDistance: the 2^20 count in every second gene -- with it the row mean exceeds the trimmed variance and the
        #  robust dispersion sits on its 0.04 floor; the other genes exercise the moments estimate itself)
        c = make_case(kind, p, m, weights=w, big_every=2 if name == "cooksDistance" else 1)
        c["q"], c["a"], c["r"] = design_qr(c["x"])
        c["mu_floor"] = 0.5 if m == 24 else 0.0                     # (the floor of R/core.R:763 on one case)
        ref = []
        if name == "cooksDistance":
            c["mu_fit"], c["H"] = np.zeros((c["n"], m)), np.zeros((c["n"], m))
        for i in range(c["n"]):
            if name == "nbinomLogLike":
                ref.append(nbinomLogLike(c["y"][i], c["mu"][i], np.exp(c["log_alpha"][i]), c["weights"][i], w))
            elif name == "linearMu":
                ref.append(linear_mu(c["y"][i], c["nf"][i], c["q"], c["a"], c["mu_floor"]))
            elif name == "prefitMoments":
                ref.append(prefit_moments(c["y"][i], c["nf"][i], c["q"], c["a"], c["r"], c["weights"][i], w))
            else:
                post = fit_beta_post(c["y"][i], c["x"], c["nf"][i], float(np.exp(c["log_alpha"][i])), c["contrast"],
                                     c["beta_drawn"][i], c["lam"], c["weights"][i], False, c["minmu"])
                c["mu_fit"][i] = [float(v) for v in post["mu"]]
                c["H"][i] = [float(v) for v in post["hat_diagonals"][0]]
                ref.append(cooks_distance(c["y"][i], c["nf"][i], c["mu_fit"][i], c["H"][i], c["x"]))
        _REF_CACHE[key] = (c, ref)
    return _REF_CACHE[key]


def aux_items(shape, c, ref, got):
    """(budget family, gene, double, mp value, M) for every output of an aux case; `got`: the routine's arrays under its
    own names (a bare array for nbinomLogLike / linearMu).  Exact outputs (allZero, an NA maxCooks) are asserted here."""
    name = shape[0]
    for i in range(c["n"]):
        if name == "nbinomLogLike":
            yield name, i, got[i], ref[i][0], ref[i][1]
        elif name == "linearMu":
            for j in range(c["m"]):
                yield name, i, got[i, j], ref[i][0][j], ref[i][1][j]
        elif name == "prefitMoments":
            assert bool(got["allZero"][i]) == ref[i]["allZero"], "allZero of gene %d" % i
            for k in ("baseMean", "baseVar", "roughDisp"):
                yield k, i, got[k][i], ref[i][k][0][0], ref[i][k][1][0]
            for k in range(c["p"]):
                yield "beta_init", i, got["beta_init"][i, k], ref[i]["beta_init"][0][k], ref[i]["beta_init"][1][k]
        else:
            for j in range(c["m"]):
                yield "cooks", i, got["cooks"][i, j], ref[i]["cooks"][0][j], ref[i]["cooks"][1][j]
            if ref[i]["maxCooks"] is None:
                assert np.isnan(got["maxCooks"][i])
            else:
                yield "maxCooks", i, got["maxCooks"][i], ref[i]["maxCooks"][0][0], ref[i]["maxCooks"][1][0]
            yield "robustDisp", i, got["robustDisp"][i], ref[i]["robustDisp"][0][0], ref[i]["robustDisp"][1][0]


def ratio(value, ref, M):
    """|double - mp| / (u M)"""
    err = abs(mp.mpf(float(value)) - ref)
    if M == 0:                                   # (a hat diagonal under a zero weight: exactly zero on both sides)
        return 0.0 if err == 0 else float("inf")
    return float(err / (U * mp.mpf(M)))


# ---- the columns between and after the fits: chain_audit -------------------------------------------------------------------
# One DESeq() call returns every column below together with the columns it is a closed-form function of.  chain_audit
# recomputes each derived column at 50 digits from the upstream columns THE SAME CALL returned (no search is re-run, no
# control flow is followed), written from R/core.R, R/fitNbinomGLMs.R and R/expanded.R:
#   baseMean, baseVar      R/core.R:2138-2146  row mean / variance of counts / nf [* weights]; refitted rows from replaceCounts (:2491)
#   dispFit                :2166-2190, 894-899, 2512   asymptDisp + extraPois / baseMean, or the coefficient itself ("mean")
#   trend coefficients     :871   the fit on exactly the rows with dispGeneEst > 100 minDisp
#   varLogDispEsts         :1137-1150, R/methods.R:180   (1.4826 median |r - median r|)^2, r = log dispGeneEst - log dispFit
#   dispPriorVar           :1197-1200   max(varLogDispEsts - trigamma((m - p) / 2), 0.25)
#   dispMAP                :1099-1101   within [minDisp, max(10, m)]
#   dispOutlier            :1111-1114   log dispGeneEst > log dispFit + 2 sqrt(varLogDispEsts)
#   dispersion             :1115        dispGeneEst on flagged rows, dispMAP elsewhere
#   mu                     R/fitNbinomGLMs.R:180   nf exp(x beta), beta = the returned log2 beta / log2(e) (the assay is NOT floored
#                          at minmu: the floor of src/DESeq2.cpp:359-361 acts inside the fit, on betaSE and H)
#   betaSE, H              src/DESeq2.cpp:376-465, R/fitNbinomGLMs.R:198   sqrt(diag Sigma) log2(e); the hat diagonals
#   stat                   R/core.R:1471   beta / betaSE
#   pvalue                 :1507   2 pnorm(|stat|, lower.tail = FALSE) = erfc(|stat| / sqrt 2)
#   logLike                :2208-2217, R/fitNbinomGLMs.R:182
#   logLikeReduced, LRT    :1877-1878, R/fitNbinomGLMs.R:99-137   the closed-form fit of ~ 1; pchisq(2 (logLike - logLikeReduced), df)
#   cooks, maxCooks        :2333-2359; after a refit :2538-2546 (the replaceable samples do not count)
#   replace, replaceCounts :2079-2110   any cooks > qf(.99, p, m - p); as.integer(trimmed mean (trim .2) * nf) where above it
#   betaPriorVar           :1601-1689, 2416-2419, 2762-2800; R/expanded.R:20-98
# Budgets (BUDGETS below, the file's convention |double - mp| <= K u M): measured on the CPU against the oracle chain
# (tests/test_chain_audit_cpu.py prints them), K the next power of two at or above twice the worst ratio seen.
#
# mu, betaSE, H and a logLike that is taken at mu(beta) carry a CONDITIONING term, derived here from the count of roundings
# (as tests/vst_spec.py: spec_bound does), not measured.  The returned log2 coefficient is fl(beta_fit * fl(log2 e)): two
# roundings, so the beta the audit recovers (returned / log2 e, exact at 50 digits) is beta_fit (1 + d), |d| <= 2u.  The
# fit's own eta_j = sum_k x_jk beta_k is a sum of nnz_j products: |error| <= nnz_j u S_j with S_j = sum_k |x_jk beta_k|
# (the classical bound of a dot product; an fma only lowers it).  Together |eta_fit - eta_mp| <= (2 + nnz_j) u S_j.  exp()
# of the engine is within 2 ulp = 4u (tests/test_oracle_math.py holds it to 1.5), the product with nf adds u:
#     |mu_fit - mu_mp| <= u mu (5 + (2 + nnz_j) S_j) =: u M_mu_j.
# w_j = mu_j / (1 + alpha mu_j) has d log w / d eta = 1 / (1 + alpha mu) <= 1, so every entry of X'WX moves by at most that
# relative amount and what passes through A^-1 moves by kappa(A) times it: the M of fit_beta_post's outputs is multiplied
# by C = max_j (5 + (2 + nnz_j) S_j) / 5 >= 1 -- in units of the five roundings a mu costs anyway.
BUDGETS.update({
    #                       K        largest ratio of the oracle chain (CPU, every case of tests/chain_cases.py)
    "stat":                 1.0,     # derived, not measured: one correctly rounded division is within u |value| (0.995 seen)
    "dispFit":              4.0,     # 1.71   (paired12)
    "varLogDispEsts":       0.5,     # 0.154  (bc_weights)
    "dispPriorVar":         1.0,     # 0.300  (factor4_mean; on the 0.25 floor elsewhere)
    "pvalue":               16.0,    # 6.63   (bc_4200)
    "mu":                   1.0,     # 0.363  (paired12; M carries the derived term)
    "betaSE":               2.0,     # 0.883  (factor4_prior_expanded; M carries the derived term)
    "H":                    1.0,     # 0.349  (bc_weights; M carries the derived term)
    "logLike_at_beta":      8.0,     # 2.17   (bc_4200: at mu(beta), refitted rows and the beta-prior fit; M carries the derived term)
    "logLikeReduced":       4.0,     # 1.89   (bc_weights under LRT; M carries the derived term of the closed-form mu)
    "LRTStatistic":         4.0,     # 1.05   (bc_weights under LRT)
    "betaPriorVar":         0.0625,  # 0.021  (factor4_prior_standard_no_refit)
})
MIN_DISP = 1e-8
OUTLIER_TIE_UNITS = 8.0            # see _disp_outlier
LOG2E = mp.log(2) ** -1


def _col(result, k, n):
    v = result.get(k)
    return None if v is None else np.asarray(v, np.float64).reshape(n, -1)


def cooks_cutoff_mp(p, m):
    """qf(.99, p, m - p) (R/core.R:2081) by inverting the regularised incomplete beta function: the F distribution
    function at x is I_{p x / (p x + d2)}(p / 2, d2 / 2)"""
    from scipy.stats import f as fdist
    d1, d2 = mp.mpf(p), mp.mpf(m - p)
    cdf = lambda t: mp.betainc(d1 / 2, d2 / 2, 0, d1 * t / (d1 * t + d2), regularized=True) - mp.mpf("0.99")
    return mp.findroot(cdf, float(fdist.ppf(.99, p, m - p)), tol=mp.mpf(10) ** -40)


def _cells_of(x):
    _, cell = np.unique(np.asarray(x, float), axis=0, return_inverse=True)
    cell = cell.reshape(-1)
    return cell, np.bincount(cell)[cell]


def _mp_median(vals):
    s = sorted(vals)
    k = len(s)
    return s[k // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) / 2


def var_log_disp_ests(dge, dfit):
    """(mad(r))^2 over r = log dispGeneEst - log dispFit on the rows with dispGeneEst >= 100 minDisp (R/core.R:1137-1150,
    R/methods.R:180; stats::mad = 1.4826 median |r - median r|, both medians exact selections) -> (value, M).
    M: the double side takes its logs in double, each within an ulp or two of a value up to L = max (|log dispGeneEst| +
    |log dispFit| + |r|) in magnitude; the MAD moves by as much, its square by 2 mad times that: M = v + 2 * 1.4826 sqrt(v) L"""
    rows = [i for i in range(len(dge)) if dge[i] >= 100 * MIN_DISP]
    la, lf = [mp.log(_f(dge[i])) for i in rows], [mp.log(_f(dfit[i])) for i in rows]
    r = [a - b for a, b in zip(la, lf)]
    med = _mp_median(r)
    mad = mp.mpf("1.4826") * _mp_median([abs(t - med) for t in r])
    L = max(abs(a) + abs(b) + abs(t) for a, b, t in zip(la, lf, r))
    return mad * mad, mad * mad + 2 * mp.mpf("1.4826") * mad * L


def _disp_outlier(dge, dfit, vlde, outlierSD=2):
    """R/core.R:1111-1113 at 50 digits -> (flag, tie).  The double evaluation takes two logs (each within 1.5 ulp = 3u of its
    value), a square root (u), a product by 2 (exact) and a sum (u): with L = |log dispGeneEst| and R = |log dispFit| + 2 sd
    its two sides are off by at most 3u L + (3 + 1 + 1) u R <= 8u max(L, R).  A row whose margin is within OUTLIER_TIE_UNITS =
    8 units of u = 2^-53 of the larger side is a tie."""
    a, b = mp.log(_f(dge)), mp.log(_f(dfit))
    sd = outlierSD * mp.sqrt(_f(vlde))
    margin = a - (b + sd)
    return bool(margin > 0), abs(margin) <= OUTLIER_TIE_UNITS * U * max(abs(a), abs(b) + sd)


def _wtd_quantile(x, w, prob):
    """Hmisc.wtd.quantile(x, weights, prob, normwt = TRUE), type = "quantile" (R/core.R:2762-2800) -> (value, M).  With
    normwt the weights sum to N exactly; the double side's sum is off by up to N u N, its order statistic `order` with it:
    M = |value| + N^2 |x_high - x_low| / 2 (a continuous function of `order`); a cumulated weight that close to `low` or
    `high` is a tie (value None)."""
    keep = [i for i in range(len(x)) if w[i] != 0]
    x, w = [x[i] for i in keep], [w[i] for i in keep]
    N = len(x)
    tot = mp.fsum(w)
    pairs = sorted(zip(x, [t * N / tot for t in w]), key=lambda t: t[0])
    ux, cs = [], []
    for xv, wv in pairs:
        if ux and ux[-1] == xv:
            cs[-1] += wv
        else:
            ux.append(xv); cs.append((cs[-1] if cs else mp.mpf(0)) + wv)
    order = 1 + (N - 1) * _f(prob)
    low = max(mp.floor(order), 1)
    high = min(low + 1, N)
    frac = order - mp.floor(order)

    def stepq(q):                                   # approx(cumsum(wts), x, method = "constant", f = 1, rule = 2)
        for xv, c in zip(ux, cs):
            if c != q and abs(c - q) <= N * N * U and q < N:
                return None
            if c >= q:
                return xv
        return ux[-1]
    ql, qh = stepq(low), stepq(high)
    if ql is None or qh is None:
        return None, None
    val = (1 - frac) * ql + frac * qh
    return val, abs(val) + N * N * abs(qh - ql) / 2


def beta_prior_var(mle_beta, baseMean, dispFit, x_names, factors=None, expanded=False, weighted=True, upperQuantile=0.05):
    """estimateBetaPriorVar (R/core.R:1601-1689) with matchWeightedUpperQuantileForVariance (:2416-2419); expanded model
    matrices: addAllContrasts (R/expanded.R:76-98) and averagePriorsOverLevels (:20-73).  mle_beta: the rows that are not all
    zero.  x_names: one name per column of the standard matrix, "<factor><level>" for the level indicators.
    -> [(value, M) or (None, None) on a tie] per column of the (expanded) matrix"""
    n, p = mle_beta.shape
    cols = [[_f(v) for v in mle_beta[:, c]] for c in range(p)]
    names = list(x_names)
    if expanded:
        for f in factors:
            idx = [i for i, nm in enumerate(x_names) if nm.startswith(f) and nm != "Intercept"]
            for j in range(len(idx) - 1):
                for i in range(j + 1, len(idx)):
                    cols.append([a - b for a, b in zip(cols[idx[i]], cols[idx[j]])]); names.append(f + "Cntrst")
    wts = [1 / (1 / _f(baseMean[i]) + _f(dispFit[i])) for i in range(n)]                       # :1641-1642
    qn = mp.sqrt(2) * mp.erfinv(1 - mp.mpf(upperQuantile))                                    # qnorm(1 - upperQuantile / 2)
    pv = []
    for c, col in enumerate(cols):
        if names[c] == "Intercept":
            pv.append((mp.mpf(10) ** 6, mp.mpf(10) ** 6)); continue                          # :1669-1671
        use = [i for i in range(n) if abs(col[i]) < 10]
        if not use:
            pv.append((mp.mpf(10) ** 6, mp.mpf(10) ** 6)); continue
        q, Mq = _wtd_quantile([abs(col[i]) for i in use], [wts[i] if weighted else mp.mpf(1) for i in use], 1 - upperQuantile)
        pv.append((None, None) if q is None else ((q / qn) ** 2, 2 * q * Mq / qn ** 2))
    if not expanded:
        return pv
    enames = ["Intercept"] + ["%s%d" % (f, lv) for f, codes in factors.items() for lv in range(int(np.max(codes)) + 1)]
    out = [(mp.mpf(0), mp.mpf(0))] * len(enames)
    for c, nm in enumerate(names):
        if nm in enames:
            out[enames.index(nm)] = pv[c]
    for f, codes in factors.items():
        mm = {"%s%d" % (f, lv) for lv in range(int(np.max(codes)) + 1)} | {f + "Cntrst"}
        vals = [pv[c] for c, nm in enumerate(names) if nm in mm]
        mean = (None, None) if any(v[0] is None for v in vals) else (mp.fsum(v[0] for v in vals) / len(vals),
                                                                      mp.fsum(v[1] for v in vals) / len(vals))
        for i, nm in enumerate(enames):
            if nm in mm:
                out[i] = mean
    return out


def heavy_rows(result, n_max=64):
    """the rows the mp-heavy relations run on, chosen from the result alone: every replaced row, every dispOutlier row, the rows
    whose searches ended at their iteration limit (what N_OPTIM_* / N_GRID_* count), the neighbours of the all-zero rows, then
    the others evenly by baseMean rank"""
    n = len(result["baseMean"])
    live = np.nan_to_num(np.asarray(result["allZero"], float), nan=1.0) == 0
    picked, special = [], True

    def add(rows):
        for i in rows:
            if 0 <= i < n and live[i] and i not in picked and (special or len(picked) < n_max):
                picked.append(int(i))
    add(np.flatnonzero(np.nan_to_num(np.asarray(result["replace"], float)) == 1))
    add(np.flatnonzero(np.nan_to_num(np.asarray(result["dispOutlier"], float)) == 1))
    for k in ("betaIter", "dispIter", "dispGeneIter"):
        add(np.flatnonzero(np.nan_to_num(np.asarray(result[k], float)) >= 100))
    n_max = max(n_max, len(picked) + 16)         # (the rows singled out above all count; at least 16 ordinary ones beside them)
    special = False
    for i in np.flatnonzero(~live)[:8]:
        add([i - 1, i + 1])
    rank = [i for i in np.argsort(np.nan_to_num(np.asarray(result["baseMean"], float)), kind="stable") if live[i]]
    if rank and len(picked) < n_max:
        add([rank[int(round(t))] for t in np.linspace(0, len(rank) - 1, n_max - len(picked))])
    return picked


_BUDGET_OF = {"logLike": "nbinomLogLike"}        # (a family held to a budget of another name)


class AuditReport:
    def __init__(self):
        self.ratios, self.where, self.ties, self.failures, self.counts = {}, {}, {}, [], {}

    def item(self, fam, row, value, ref, M):
        r = ratio(value, ref, M) if np.isfinite(value) else float("inf")
        self.counts[fam] = self.counts.get(fam, 0) + 1
        if r > self.ratios.get(fam, -1.0):
            self.ratios[fam], self.where[fam] = r, row

    def exact(self, ok, what):
        self.counts[what.split(":")[0]] = self.counts.get(what.split(":")[0], 0) + 1
        if not ok:
            self.failures.append(what)

    def tie(self, fam):
        self.ties[fam] = self.ties.get(fam, 0) + 1

    def excess(self):
        """the worst ratio in units of its budget; infinite when an exact relation is broken"""
        if self.failures:
            return float("inf")
        return max([v / BUDGETS[_BUDGET_OF.get(k, k)] for k, v in self.ratios.items()] + [0.0])

    def summary(self):
        return {k: float("%.3g" % v) for k, v in sorted(self.ratios.items())}


def chain_audit(inputs, result, n_heavy=64, scalars=True, trend_fits=None, rows=None):
    """inputs: counts (n x m), x, sizeFactors or normalizationFactors, weights, minReplicatesForReplace, minmu, fitType, betaPrior,
    factors, modelMatrixType, x_names -- what the call was given.  result: what it returned (native.DESeq's names: the
    per-gene columns, the assays mu / H / cooks [/ replaceCounts], dispersionFunction, status [, betaPriorVar, mle_beta]).
    scalars = False: the all-gene scalars (trend, varLogDispEsts, betaPriorVar) are not rebuilt -- after a refit the rows
    they came from are overwritten (R/core.R:2533-2534); the caller compares them with the run without a refit instead.
    trend_fits: {"exact": f, "restated": (f, rtol)}, f(means, disps) -> the two coefficients.  -> AuditReport"""
    R = AuditReport()
    y = np.asarray(inputs["counts"])
    n, m = y.shape
    x = np.asarray(inputs["x"], np.float64)
    p = x.shape[1]
    nf = (np.broadcast_to(np.asarray(inputs["sizeFactors"], np.float64)[None, :], y.shape)
          if inputs.get("normalizationFactors") is None else np.asarray(inputs["normalizationFactors"], np.float64))
    wraw = None if inputs.get("weights") is None else np.asarray(inputs["weights"], np.float64)
    useW = wraw is not None
    wnorm = wraw / wraw.max(axis=1, keepdims=True) if useW else np.ones(y.shape)          # R/core.R:2702
    minmu = float(inputs.get("minmu", 0.5))
    minrep = float(inputs.get("minReplicatesForReplace", 7))
    col = lambda k: None if result.get(k) is None else np.asarray(result[k], np.float64)          # (_col: the same as n x k)
    allZero = np.nan_to_num(col("allZero"), nan=1.0) == 1
    replace = np.nan_to_num(col("replace")) == 1
    yrep = None if result.get("replaceCounts") is None else np.asarray(result["replaceCounts"])
    yfit = np.where(replace[:, None], yrep, y) if (replace.any() and yrep is not None) else y
    live = ~allZero
    bm, bv, dge, dfit = col("baseMean"), col("baseVar"), col("dispGeneEst"), col("dispFit")
    dmap, disp, dout = col("dispMAP"), col("dispersion"), col("dispOutlier")
    fn = result["dispersionFunction"]
    vlde = fn["varLogDispEsts"]
    cell, cellsize = _cells_of(x)
    replaceable = cellsize >= minrep
    refit_ran = bool(replace.any() and (replace & live).any() and replaceable.any())

    beta, se, stat, pval = (_col(result, k, n) for k in ("beta", "betaSE", "stat", "pvalue"))

    # ---- every row: the cheap relations
    for i in (range(n) if rows is None else rows):
        src = yfit[i] if (replace[i] and yrep is not None) else y[i]
        v = [_f(src[j]) / _f(nf[i, j]) * (_f(wraw[i, j]) if useW else 1) for j in range(m)]
        (mean, Mm), (var, Mv) = _mean_var(v)
        R.item("baseMean", i, bm[i], mean, Mm)
        R.item("baseVar", i, bv[i], var, Mv)
        if not live[i]:
            continue
        if fn["fitType"] == "parametric":
            a, e = (_f(t) for t in fn["coefficients"])
            R.item("dispFit", i, dfit[i], a + e / _f(bm[i]), abs(a) + abs(e / _f(bm[i])))
        elif fn["fitType"] == "mean":
            R.exact(dfit[i] == float(fn["coefficients"]), "dispFit: row %d is not the trimmed mean" % i)
        R.exact(MIN_DISP <= dmap[i] <= max(10, m), "dispMAP: row %d outside [minDisp, max(10, m)]" % i)
        flag, tie = _disp_outlier(dge[i], dfit[i], vlde)
        if tie:
            R.tie("dispOutlier")
        else:
            R.exact(bool(dout[i]) == flag, "dispOutlier: row %d" % i)
        R.exact(disp[i] == (dge[i] if dout[i] else dmap[i]), "dispersion: row %d is not %s" % (i, "dispGeneEst" if dout[i] else "dispMAP"))
        if stat is not None:
            for c in range(beta.shape[1]):
                if not (np.isfinite(beta[i, c]) and se[i, c] > 0):
                    continue
                q = _f(beta[i, c]) / _f(se[i, c])
                R.item("stat", i, stat[i, c], q, abs(q))
                pv = mp.erfc(abs(_f(stat[i, c])) / mp.sqrt(2))
                if pv < mp.mpf(2) ** -1022:                   # a subnormal result: one denormal step from the nearest double
                    R.exact(abs(pval[i, c] - float(pv)) <= 2.0 ** -1074, "pvalue: row %d (subnormal)" % i)
                else:
                    R.item("pvalue", i, pval[i, c], pv, pv)

    # ---- the all-gene scalars
    if scalars:
        use = live & (np.nan_to_num(dge) > 100 * MIN_DISP)                                   # R/core.R:871
        if fn["fitType"] == "parametric" and trend_fits:
            got = np.asarray(fn["coefficients"], np.float64)
            if "exact" in trend_fits:
                R.exact(np.array_equal(np.asarray(trend_fits["exact"](bm[use], dge[use])), got),
                        "trend: not the fit on the rows with dispGeneEst > 100 minDisp")
            if "restated" in trend_fits:
                f, rtol = trend_fits["restated"]
                R.exact(np.allclose(np.asarray(f(bm[use], dge[use])), got, rtol=rtol, atol=0), "trend: restatement")
        if fn["fitType"] == "mean":
            from fractions import Fraction
            s = np.sort(dge[live & (np.nan_to_num(dge) > 10 * MIN_DISP)])                   # :894-899
            k = int(np.floor(s.size * 0.001))
            kept = s[k: s.size - k]
            R.exact(float(sum(Fraction(t) for t in kept.tolist()) / kept.size) == float(fn["coefficients"]), "trend: trimmed mean")
        v, Mv = var_log_disp_ests(dge[live], dfit[live])
        R.item("varLogDispEsts", -1, vlde, v, Mv)
    if m > p:
        tg = mp.psi(1, mp.mpf(m - p) / 2)
        R.item("dispPriorVar", -1, fn["dispPriorVar"], max(_f(vlde) - tg, mp.mpf("0.25")), _f(vlde) + tg)

    # ---- Cook's cutoff, maxCooks, replace: exact selections on the returned distances, every row
    ck = col("cooks")
    cutoff = float(result["cooksCutoff"])
    cm = cooks_cutoff_mp(p, m)
    R.exact(abs(_f(cutoff) - cm) <= mp.mpf(10) ** -12 * cm, "cooksCutoff: not qf(.99, p, m - p)")
    if ck is not None:
        for3 = cellsize >= 3
        ckm = np.where(replaceable[None, :], 0.0, ck) if refit_ran else ck                  # :2538-2546: replaceCooks[, replaceable] <- 0
        if refit_ran and replaceable.all():
            for3 = np.zeros(m, bool)                                                         # :2539: NA
        mx = col("maxCooks")
        for i in np.flatnonzero(live):
            want = ckm[i, for3].max() if (m > p and for3.any()) else np.nan
            R.exact((np.isnan(want) and np.isnan(mx[i])) or mx[i] == want, "maxCooks: row %d" % i)
            if np.isfinite(minrep) and replaceable.any():
                R.exact(bool(replace[i]) == bool((ck[i] > cutoff).any()), "replace: row %d" % i)   # :2086

    # ---- at most n_heavy rows: the relations that need the model
    heavy = heavy_rows(result, n_heavy) if rows is None else [i for i in rows if live[i]]
    prior = bool(inputs.get("betaPrior"))
    mle = _col(result, "mle_beta", n) if prior else beta
    xp = x
    lam_mle = np.full(p, 1e-6) / np.log(2) ** 2                                              # R/fitNbinomGLMs.R:73,162
    lam_fit = lam_mle
    if prior:
        if inputs.get("modelMatrixType", "expanded" if inputs.get("factors") else "standard") == "expanded":
            f = inputs["factors"]
            xp = np.column_stack([np.ones(m)] + [(np.asarray(c) == lv).astype(float) for c in f.values()
                                                 for lv in range(int(np.max(c)) + 1)])     # R/expanded.R:1-18
        lam_fit = 1.0 / np.asarray(result["betaPriorVar"], np.float64) / np.log(2) ** 2     # :311, :162
    mu_r, H_r = col("mu"), col("H")
    iters = np.nan_to_num(col("betaIter"))

    def mu_at(xm, b, i):                             # R/fitNbinomGLMs.R:180: nf * exp(x beta), NOT floored at minmu
        return [_f(nf[i, j]) * mp.exp(mp.fsum(_f(xm[j, k]) * b[k] for k in range(xm.shape[1]) if xm[j, k] != 0)) for j in range(m)]

    def eta_terms(xm, b):
        S = [sum(abs(xm[j, k] * b[k]) for k in range(xm.shape[1])) for j in range(m)]
        return [5 + (2 + int(np.count_nonzero(xm[j]))) * S[j] for j in range(m)]
    for i in heavy:
        alpha = disp[i]
        zero = np.zeros(xp.shape[1])
        opt = iters[i] >= 100                      # (rows of the optim fallback: mu, betaSE as R/fitNbinomGLMs.R:382-397, H the IRLS's)
        b_mp = [_f(v) / LOG2E for v in beta[i]]
        b_fit = [float(v) for v in b_mp]
        post = fit_beta_post(yfit[i], xp, nf[i], alpha, zero, b_mp, lam_fit, wnorm[i], useW, minmu)
        T = eta_terms(xp, b_fit)
        C = max(T) / 5
        if not opt:
            for k in range(xp.shape[1]):
                s = mp.sqrt(post["beta_var_mat"][0][k]) * LOG2E
                Mk = LOG2E * post["beta_var_mat"][1][k] / (2 * mp.sqrt(post["beta_var_mat"][0][k])) * C
                R.item("betaSE", i, se[i, k], s, Mk)
        # mu and H belong to the fit without the prior (R/fitNbinomGLMs.R:256-260, 293), and to the FIRST fit on refitted rows
        m_mp = [_f(v) / LOG2E for v in mle[i]]
        own = post if not prior else fit_beta_post(yfit[i], x, nf[i], alpha, np.zeros(p), m_mp, lam_mle, wnorm[i], useW, minmu)
        Tm = T if not prior else eta_terms(x, [float(_f(v) / LOG2E) for v in mle[i]])
        if mu_r is not None and not replace[i] and not opt:
            mus = mu_at(x, m_mp, i)
            for j in range(m):
                R.item("mu", i, mu_r[i, j], mus[j], mus[j] * Tm[j])
                if H_r is not None and not prior:   # (the beta-prior run returns no iteration count of its first fit: the rows
                    #                                  that left its IRLS -- their H is the last iterate's -- cannot be told apart)
                    R.item("H", i, H_r[i, j], own["hat_diagonals"][0][j], own["hat_diagonals"][1][j] * max(Tm) / 5)
        ll = col("logLike")
        if ll is not None and mu_r is not None:
            if replace[i] or prior:
                if not opt:
                    size = 1 / _f(alpha)
                    val = M = mp.mpf(0)
                    mus = mu_at(xp, b_mp, i)
                    for j in range(m):
                        w = _f(wnorm[i, j]) if useW else mp.mpf(1)
                        mj = mus[j]
                        parts = nb_logpmf_parts(yfit[i][j], mj, size)
                        val += w * mp.fsum(parts)
                        g = abs(_f(yfit[i][j]) - mj) / (1 + _f(alpha) * mj)           # |d log f / d eta|
                        M += abs(w) * (mp.fsum(parts, absolute=True) + g * T[j])
                    R.item("logLike_at_beta", i, ll[i], val, M)
            else:                                      # (a row of the optim fallback: at the floored mu, R/fitNbinomGLMs.R:386-399)
                R.item("logLike", i, ll[i], *nbinomLogLike(y[i], np.maximum(mu_r[i], minmu) if opt else mu_r[i], alpha, wnorm[i], useW))
        llr, lrt = col("logLikeReduced"), col("LRTStatistic")
        if (llr is not None or lrt is not None) and ll is not None:
            # nbinomLRT against ~ 1 (R/core.R:1877): the reduced fit is closed-form (R/fitNbinomGLMs.R:99-137), mu = nf 2^beta with
            # beta = log2 of the [weighted] mean normalized count.  Derived term of its mu: the mean is m [2m] roundings, log2 within
            # 2 ulp of beta is 4u |ln mean| in 2^beta, 2^beta 4u, the product u: T = [2] m + 5 + 4 |ln mean|
            yn = [_f(yfit[i][j]) / _f(nf[i, j]) for j in range(m)]
            ws = [_f(wnorm[i, j]) if useW else mp.mpf(1) for j in range(m)]
            mean = mp.fsum(w * t for w, t in zip(ws, yn)) / mp.fsum(ws)
            Tr = (2 if useW else 1) * m + 5 + 4 * abs(mp.log(mean))
            size = 1 / _f(alpha)
            vr = Mr = mp.mpf(0)
            for j in range(m):
                mj = _f(nf[i, j]) * mean
                parts = nb_logpmf_parts(yfit[i][j], mj, size)
                vr += ws[j] * mp.fsum(parts)
                Mr += ws[j] * (mp.fsum(parts, absolute=True) + abs(_f(yfit[i][j]) - mj) / (1 + _f(alpha) * mj) * Tr)
            if llr is not None:
                R.item("logLikeReduced", i, llr[i], vr, Mr)
            if lrt is not None and not opt:
                # the statistic at the returned logLike (audited above): 2 (logLike - logLikeReduced), the reduced side at 50 digits
                R.item("LRTStatistic", i, lrt[i], 2 * (_f(ll[i]) - vr), 2 * (abs(_f(ll[i])) + Mr))
                pv = mp.gammainc(mp.mpf(int(result["df"])) / 2, max(_f(lrt[i]), 0) / 2, mp.inf, regularized=True)   # :1878
                R.exact(abs(_f(col("LRTPvalue")[i]) - pv) <= mp.mpf(10) ** -12 * pv + mp.mpf(2) ** -1074, "LRTPvalue: row %d" % i)
        if ck is not None and mu_r is not None and H_r is not None:
            cd = cooks_distance(y[i], nf[i], mu_r[i], H_r[i], x)
            for j in range(m):
                if float(H_r[i, j]) < 1.0:
                    R.item("cooks", i, ck[i, j], cd["cooks"][0][j], cd["cooks"][1][j])
        if replace[i] and yrep is not None:                                                   # :2088-2098
            cn = [_f(y[i, j]) / _f(nf[i, j]) for j in range(m)]
            tm, Mt, _ = _trimmed_mean(cn, mp.mpf("0.2"))
            for j in range(m):
                if ck[i, j] > cutoff and replaceable[j]:
                    t = tm * _f(nf[i, j])
                    if abs(t - mp.nint(t)) <= 8 * U * Mt * _f(nf[i, j]):
                        R.tie("replaceCounts")
                    else:
                        R.exact(int(yrep[i, j]) == int(mp.floor(t)), "replaceCounts: row %d sample %d is not as.integer(trimmed mean * nf)" % (i, j))
                else:
                    R.exact(int(yrep[i, j]) == int(y[i, j]), "replaceCounts: row %d sample %d was not to be replaced" % (i, j))

    # ---- the beta prior variance
    if prior and scalars and inputs.get("betaPriorVar") is None:
        names = inputs.get("x_names") or ["Intercept"] + ["V%d" % k for k in range(1, p)]
        expd = xp.shape[1] != p
        ref = beta_prior_var(mle[live], bm[live], dfit[live], names, inputs.get("factors"), expd)
        for k, (v, M) in enumerate(ref):
            if v is None:
                R.tie("betaPriorVar")
            else:
                R.item("betaPriorVar", k, result["betaPriorVar"][k], v, M)
    return R
