"""R's unmix() call restated through scipy (R/helper.R:93-112) -- TEST helper: the reference optimiser on the reference
objective, the cross-check of the library's own optimiser.  optim(par = rep(1, k), fn, gr = NULL,
method = "L-BFGS-B", lower = lo, upper = 100): factr = 1e7, pgtol = 0, maxit = 100, 5 corrections, and optim's numerical
gradient -- central differences of step ndeps = 1e-3, clipped at the bounds as optim clips them.  It is NOT R's iterates:
scipy's L-BFGS-B is a later revision of the code R ships, and libm's log / asinh stand in for R's.  Not part of the product."""
import numpy as np


def vst(q, alpha):
    return (2 * np.arcsinh(np.sqrt(alpha * q)) - np.log(alpha) - np.log(4)) / np.log(2)           # R/helper.R:90


def vstSL(q, shift):
    return np.log(q + shift)                                                                      # R/helper.R:103


def sum_loss(p, x_col, pure, alpha=None, shift=None, power=1):
    """sumLossVST / sumLossSL (R/helper.R:93-95, :106-108)"""
    with np.errstate(all="ignore"):
        if alpha is not None:
            return float(np.sum(np.abs(vst(x_col, alpha) - vst(pure @ p, alpha)) ** power))
        return float(np.sum(np.abs(vstSL(x_col, shift) - vstSL(pure @ p, shift)) ** power))


def unmix_lbfgsb(x, pure, alpha=None, shift=None, power=1):
    """dict(p m x k, loss m, mix m x k): the minimiser optim would be asked for, per sample"""
    from scipy.optimize import minimize
    x, pure = np.asarray(x, np.float64), np.asarray(pure, np.float64)
    m, k = x.shape[1], pure.shape[1]
    lo, hi = (1e-6 if alpha is not None else 0.0), 100.0
    P, Ls = np.zeros((m, k)), np.zeros(m)
    for i in range(m):
        fn = lambda p: sum_loss(p, x[:, i], pure, alpha, shift, power)

        def gr(p):
            g = np.empty(k)
            for j in range(k):
                up, dn = p.copy(), p.copy()
                up[j], dn[j] = min(p[j] + 1e-3, hi), max(p[j] - 1e-3, lo)
                g[j] = (fn(up) - fn(dn)) / (up[j] - dn[j])
            return g
        o = minimize(fn, np.ones(k), jac=gr, method="L-BFGS-B", bounds=[(lo, hi)] * k,
                     options=dict(maxcor=5, ftol=1e7 * np.finfo(float).eps, gtol=0.0, maxiter=100))
        P[i], Ls[i] = o.x, fn(o.x)
    with np.errstate(all="ignore"):
        return {"p": P, "loss": Ls, "mix": P / P.sum(axis=1, keepdims=True)}
