"""R's optim call of estimateSizeFactorsIterate restated through scipy (R/core.R:2600-2607) -- TEST helper: the reference
optimiser on the reference objective, the cross-check of the library's own iteration.
optim(log(sf.old), fn, control = list(fnscale = -1), method = "L-BFGS-B"): no bounds, factr = 1e7, pgtol = 0, maxit = 100,
5 corrections, and optim's numerical gradient -- central differences of step ndeps = 1e-3.  It is NOT R's iterates: scipy's
L-BFGS-B is a later revision of the code R ships, and scipy's / libm's functions stand in for R's.  Not part of the product."""
import numpy as np


def fn_of(counts, mu, sf, disp, rows, Q=0.05):
    """R's fn on the rows idx: p -> sum(gene.ll[gene.ll > quantile(gene.ll, Q)])"""
    from scipy.stats import nbinom
    r = np.asarray(rows) != 0
    cts = np.asarray(counts, np.float64)[r]
    q = (np.asarray(mu, np.float64) / np.asarray(sf, np.float64)[None, :])[r]        # t(t(mu) / sf)[idx, ]
    size = 1.0 / np.asarray(disp, np.float64)[r][:, None]

    def fn(p):
        p = np.asarray(p, np.float64)
        s = np.exp(p - p.mean())
        mu_new = q * s[None, :]
        ll = nbinom.logpmf(cts, size, size / (size + mu_new))
        gene_ll = ll.sum(axis=1)
        return float(gene_ll[gene_ll > np.quantile(gene_ll, Q)].sum())
    return fn


def sf_iterate_lbfgsb(counts, mu, sf, disp, rows, Q=0.05):
    """dict(par, s = par - mean(par), F, nfev, convergence): the maximiser optim would be asked for"""
    from scipy.optimize import minimize
    fn = fn_of(counts, mu, sf, disp, rows, Q)
    m = np.asarray(sf).size
    calls = [0]

    def neg(p):                       # fnscale = -1
        calls[0] += 1
        return -fn(p)

    def gr(p):
        g = np.empty(m)
        for j in range(m):
            up, dn = p.copy(), p.copy()
            up[j], dn[j] = p[j] + 1e-3, p[j] - 1e-3
            g[j] = (neg(up) - neg(dn)) / 2e-3
        return g
    o = minimize(neg, np.log(np.asarray(sf, np.float64)), jac=gr, method="L-BFGS-B",
                 options=dict(maxcor=5, ftol=1e7 * np.finfo(float).eps, gtol=0.0, maxiter=100))
    return {"par": o.x, "s": o.x - o.x.mean(), "F": fn(o.x), "nfev": calls[0], "convergence": 0 if o.success else 1}
