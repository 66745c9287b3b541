"""Student's t distribution function in plain numpy: THE statement of dpt_upper / dpt_lower of csrc/dsq_math.hpp (DESIGN.md
section 15).  `O.unary(name, v)` supplies exp / log / log1p / stirlerr in the engine's pinned arithmetic (the oracle's or
the device's: the same bits); every other operation is IEEE, rounded once, in the order written -- no fused multiply-add
anywhere -- and each loop below runs per element exactly as a lane of the kernel runs it, so the device equals this
module bit for bit.

    upper(q, df) = P(T > q),  lower(q, df) = upper(-q, df)

With a = df / 2, t = q^2 / df, x = 1 / (1 + t), y = t / (1 + t) the two-sided area is P2 = I_x(a, 1/2) and
    E = Gamma(a + 1/2) / (Gamma(a) sqrt(pi)) x^a,     log of the Gamma quotient through stirlerr (no lgamma difference):
        a log1p(1 / (2a)) - 1/2 + log(a) / 2 + stirlerr(a + 1/2) - stirlerr(a)
four ranges of |q|:
    far     t > 1e100 (q^2 may overflow)   P2 = E / a with log x = -(2 log|q| - log df)
    tail    t >= 1                         P2 = E sqrt(y) / a  sum_k  prod_{j<k} x (a + 1/2 + j) / (a + 1 + j)
    centre  t < 1, |q| <= 2                D  = E sqrt(y)      sum_k  prod_{j<k} y (a + 1/2 + j) / (3/2 + j);  0.5 -+ D
    frac    t < 1, |q| > 2                 P2 = E sqrt(y) r,  r the continued fraction of I_x(a, 1/2) in the form that
                                           is written in y and lambda = (a + 1/2) y - 1/2 (Didonato & Morris, ACM TOMS 18
                                           (1992), section 6): stable as x -> 1, the count of its steps falls with |q| and
                                           does not grow with df
and upper = P2 / 2 for q > 0, 1 - P2 / 2 for q < 0.  Every loop stops at CAP steps whatever the input.
"""
import numpy as np

from .results_host import pnorm_both

CAP = 300                                   # kPtCap of dsq_math.hpp
FRAC_EPS = 1e-15
HALF_LN_PI = 0.572364942924700087071713675677


def _un(O, name, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return O.unary(name, v) if v.size else v


def _series(z, a, den0):
    """sum_k prod_{j<k} z (a + 1/2 + j) / (den0 + j), each element until a term no longer changes its sum; den0 is a + 1 in
    the tail (z = x) and 3/2 near the centre (z = y).  Returns the sums and the largest step count."""
    s, c = np.ones_like(z), np.ones_like(z)
    live = np.ones(z.shape, bool)
    trips = 0
    for k in range(CAP):
        if not live.any():
            break
        trips = k + 1
        kk = float(k)
        c = c * (z * ((a + 0.5) + kk) / (den0 + kk))
        s1 = s + c
        done = s1 == s
        s = np.where(live, s1, s)
        live = live & ~done
    return s, trips


def _frac(x, y, a):
    lam = (a + 0.5) * y - 0.5
    c = 1.0 + lam
    c0 = 0.5 / a
    c1 = 1.0 + 1.0 / a
    yp1 = y + 1.0
    p = np.ones_like(x)
    s = a + 1.0
    an, bn, anp1 = np.zeros_like(x), np.ones_like(x), np.ones_like(x)
    bnp1 = c / c1
    r = c1 / c
    live = np.ones(x.shape, bool)
    trips = 0
    for k in range(1, CAP + 1):
        if not live.any():
            break
        trips = k
        n = float(k)
        tt = n / a
        w = (n * (0.5 - n)) * x
        e = a / s
        alpha = p * (p + c0) * e * e * (w * x)
        e2 = (tt + 1.0) / (c1 + tt + tt)
        beta = n + w / s + e2 * (c + n * yp1)
        p = tt + 1.0
        s = s + 2.0
        t1 = alpha * an + beta * anp1
        t2 = alpha * bn + beta * bnp1
        r1 = t1 / t2
        done = np.abs(r1 - r) <= FRAC_EPS * r1
        r = np.where(live, r1, r)
        an, bn = anp1 / t2, bnp1 / t2
        anp1, bnp1 = r1, np.ones_like(x)
        live = live & ~done
    return r, trips


def _finite(O, q, df):
    """upper tail for finite q and finite df > 0, and the largest step count of each range"""
    out = np.empty(q.shape)
    trips = {"tail": 0, "centre": 0, "frac": 0}
    with np.errstate(all="ignore"):
        aq = np.abs(q)
        a = 0.5 * df
        t = (aq / df) * aq
        la = _un(O, "log", a)
        base = a * _un(O, "log1p", 0.5 / a) - 0.5 - HALF_LN_PI + (_un(O, "stirlerr", a + 0.5) - _un(O, "stirlerr", a))
        far = t > 1e100
        tail = ~far & (t >= 1.0)
        centre = (t < 1.0) & (aq <= 2.0)
        frac = (t < 1.0) & (aq > 2.0)
        x = 1.0 / (1.0 + t)
        y = t / (1.0 + t)
        sy = np.sqrt(y)
        L = _un(O, "log1p", np.where(far, 0.0, t))
        if far.any():
            L[far] = 2.0 * _un(O, "log", aq[far]) - _un(O, "log", df[far])
        outer = far | tail
        E = _un(O, "exp", np.where(outer, base - 0.5 * la, base + 0.5 * la) - a * L)
        p2 = np.zeros(q.shape)
        p2[far] = E[far]
        if tail.any():
            s, trips["tail"] = _series(x[tail], a[tail], a[tail] + 1.0)
            p2[tail] = (E[tail] * sy[tail]) * s
        if frac.any():
            r, trips["frac"] = _frac(x[frac], y[frac], a[frac])
            p2[frac] = (E[frac] * sy[frac]) * r
        half = 0.5 * p2
        out = np.where(q > 0, half, 1.0 - half)
        if centre.any():
            s, trips["centre"] = _series(y[centre], a[centre], 1.5)
            d = (E[centre] * sy[centre]) * s
            out[centre] = np.where(q[centre] > 0, 0.5 - d, 0.5 + d)
    return out, trips


def pt_upper_steps(O, q, df):
    """pt_upper and, per range of the method, the largest loop count any element took (what DESIGN.md section 15 quotes and
    the tests hold below CAP)"""
    q, df = np.broadcast_arrays(np.asarray(q, np.float64), np.asarray(df, np.float64))
    shape = q.shape
    q, df = q.ravel(), df.ravel()
    trips = {"tail": 0, "centre": 0, "frac": 0}
    out = np.full(q.shape, np.nan)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(q) & ~np.isnan(df) & (df > 0)
    qinf = ok & np.isinf(q)
    out[qinf] = np.where(q[qinf] > 0, 0.0, 1.0)
    normal = ok & ~qinf & np.isinf(df)
    if normal.any():
        out[normal] = pnorm_both(lambda v: _un(O, "exp", v), q[normal])[1]
    fin = ok & ~qinf & ~normal
    if fin.any():
        out[fin], trips = _finite(O, q[fin], df[fin])
    return out.reshape(shape), trips


def pt_upper(O, q, df):
    """pt(q, df, lower.tail = FALSE), elementwise over the broadcast of q and df.  NaN in either, df <= 0: NaN; q = -Inf /
    +Inf: 1 / 0; df = +Inf: the normal tail (results_host.pnorm_both)"""
    return pt_upper_steps(O, q, df)[0]


def pt_lower(O, q, df):
    """pt(q, df): the upper tail of -q, bit for bit"""
    return pt_upper(O, -np.asarray(q, np.float64), df)


def pt_two_sided(O, q, df):
    """2 * pt(abs(q), df, lower.tail = FALSE), getContrast's p-value (R/results.R:812-815)"""
    return 2.0 * pt_upper(O, np.abs(np.asarray(q, np.float64)), df)
