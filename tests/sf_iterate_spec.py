"""The arithmetic specification of the solve of estimateSizeFactors(type = "iterate") stated in
numpy: the reference for the sf_iterate tests.  Not a test itself.  exp / log / log1p / stirlerr and the negative binomial
log density are the oracle's (oracle.unary, oracle.dnbinom_mu_log: bit-equal to the device's, tests/test_gpu_math.py); +, -,
*, / are IEEE, every operation rounded once, in the order written here; every sum has the order written here.  Shares no code
with the product (deseq2_amd/csrc/sf_iterate.hip, deseq2_amd/sf_iterate_host.py).

One round of estimateSizeFactorsIterate (R/core.R:2597-2611) fixes the counts k, q_ij = mu_ij / sf_j and the dispersions
a_i over the rows whose flag is set and maximises, over s with sum s = 0,
    F(s) = sum of L_i over { i : L_i > quantile(L, Q) (type 7) },   L_i = sum_j log NB(k_ij; mu = q_ij exp(s_j), size = 1 / a_i)
by Newton's step under the gauge on the kept set, safeguarded by an Armijo test on the true F.

Orders.  L_i = K'_i + W, both wave-order sums over the samples (sf_spec.wave_sum) of the two parts of the closed split of
the density.  F: thread t of T = 1024 adds the kept rows t, t + T, ... (positions in the FULL row
range) from 0.0; the 64 threads of a wave combine by the butterfly; the 16 wave sums add in wave order.  g_j, h_j: the kept
genes of a slice of G consecutive genes add in gene order from 0.0; the slices add in slice order from 0.0.  Every sum over
the samples other than a row sum (means, lambda, g.d) is serial in sample order from 0.0."""
import numpy as np

from tests.sf_spec import wave_sum, _exp, _log

LN2PI = 1.837877066409345483560659472811
T = 1024                 # the threads that add F
G = 64                   # dsq_sf_iterate_slice_genes()
MAX_TRIALS = 30
ARMIJO = 1e-4
RELTOL = 1e-10


def serial_sum(v):
    s = 0.0
    for x in np.asarray(v, np.float64):
        s = s + x
    return s


def _split(K, a):
    """the cells inside the closed split (cell_dev_closed of csrc/dsq_math.hpp) and the gene's `fast` flag"""
    with np.errstate(all="ignore"):
        size = 1.0 / a
        fast = (a > 0) & np.isfinite(a) & np.isfinite(size) & (size > 0)
        sz = size[:, None]
        nn = K + sz
        gen = (K > 0) & np.isfinite(K) & ~(K < 1e-10 * sz) & (nn != sz) & np.isfinite(nn)
    return fast, fast[:, None] & ((K == 0) | gen)


def row_constants(O, K, a):
    """K'_i: the mu-independent part of the row sums of the split, in wave order; 0 for a gene that is not `fast`"""
    n, m = K.shape
    fast, closed = _split(K, a)
    kj = np.zeros((n, m))
    sel = closed & (K != 0)
    if sel.any():
        y = K[sel]
        al = np.broadcast_to(a[:, None], (n, m))[sel]
        size = 1.0 / al
        nn = y + size
        L = O.unary("log1p", al * y)
        ly = O.unary("log", y)
        c0 = O.unary("stirlerr", nn) - O.unary("stirlerr", size) - O.unary("stirlerr", nn - size)
        base = -L + (c0 - 0.5 * (LN2PI + ly - L))
        t = nn * L - y * ly
        kj[sel] = base + t
    return np.where(fast, wave_sum(kj), 0.0)


def row_loglike(O, K, mu, a, Kc):
    """L_i = K'_i + the wave-order sum of the mu-dependent part (the whole density for a cell outside the split)"""
    n, m = K.shape
    _, closed = _split(K, a)
    with np.errstate(all="ignore"):
        al = np.broadcast_to(a[:, None], (n, m))
        size = 1.0 / al
        d = np.empty((n, m))
        c = closed
        am = al[c] * mu[c]
        opm = 1.0 + am
        rcp = 1.0 / opm
        l1p = O.unary("log", opm) + (am - (opm - 1.0)) * rcp
        y = K[c]
        pos = y != 0
        lm = np.zeros(y.shape)
        lm[pos] = O.unary("log", np.ascontiguousarray(mu[c][pos]))
        d[c] = np.where(pos, y * lm - (y + size[c]) * l1p, -(size[c] * l1p))
        if (~c).any():
            d[~c] = O.dnbinom_mu_log(K[~c], size[~c], mu[~c])
        return Kc + wave_sum(d)


def cut_of(L, rows, Q):
    """quantile(L[rows], Q), type 7, as tests/results_spec.py states it: h = (n' - 1) Q, g = h - floor(h),
    (1 - g) s[lo] + g s[hi] with both products rounded; s[lo] itself when g == 0 or s[hi] == s[lo]"""
    s = np.sort(L[rows])
    h = (s.size - 1) * Q
    lo, hi = int(np.floor(h)), int(np.ceil(h))
    g = h - lo
    with np.errstate(all="ignore"):
        return s[lo] if (g == 0 or s[hi] == s[lo]) else (1.0 - g) * s[lo] + g * s[hi]


def kept_sum(L, kept):
    n = L.size
    part = np.zeros(T)
    for t in range(min(T, n)):
        acc = 0.0
        for i in range(t, n, T):
            if kept[i]:
                acc = acc + L[i]
        part[t] = acc
    w = wave_sum(part.reshape(T // 64, 64))
    F = w[0]
    for x in w[1:]:
        F = F + x
    return float(F)


class Problem:
    """the fixed part of one solve"""

    def __init__(self, O, counts, mu, sf, disp, rows, Q=0.05):
        self.O = O
        self.K = np.asarray(counts, np.float64)
        self.n, self.m = self.K.shape
        self.rows = np.asarray(rows) != 0
        self.sf = np.asarray(sf, np.float64)
        self.a = np.asarray(disp, np.float64)
        self.Q = float(Q)
        with np.errstate(all="ignore"):
            self.q = np.asarray(mu, np.float64) / self.sf[None, :]
        r = self.rows
        self.Kc = row_constants(O, self.K[r], self.a[r])

    def start(self):
        ls = _log(self.O, self.sf)
        return ls - serial_sum(ls) / self.m

    def evaluate(self, e):
        """at the point whose exponentials are e: (L over all rows -- NaN outside the flagged ones --, cut, kept, F)"""
        r = self.rows
        L = np.full(self.n, np.nan)
        if r.any():
            L[r] = row_loglike(self.O, self.K[r], self.q[r] * e[None, :], self.a[r], self.Kc)
        if not r.any():
            return L, np.nan, np.zeros(self.n, bool), 0.0
        if np.isnan(L[r]).any():
            return L, np.nan, np.zeros(self.n, bool), np.nan
        cut = cut_of(L, r, self.Q)
        with np.errstate(all="ignore"):
            kept = r & (L > cut)
        return L, cut, kept, kept_sum(L, kept)

    def gradient(self, kept, e):
        """g_j, h_j over the kept genes: slices of G consecutive genes, each in gene order, then the slices in order"""
        g, h = np.zeros(self.m), np.zeros(self.m)
        with np.errstate(all="ignore"):
            for b in range(0, self.n, G):
                pg, ph = np.zeros(self.m), np.zeros(self.m)
                for i in range(b, min(b + G, self.n)):
                    if not kept[i]:
                        continue
                    k, a = self.K[i], self.a[i]
                    mu = self.q[i] * e
                    opm = 1.0 + a * mu
                    pg = pg + (k - mu) / opm
                    ph = ph + (mu * (1.0 + a * k)) / (opm * opm)
                g = g + pg
                h = h + ph
        return g, h

    @staticmethod
    def step(g, h):
        """lambda, d and g.d"""
        with np.errstate(all="ignore"):
            lam = serial_sum(g / h) / serial_sum(1.0 / h)
            d = (g - lam) / h
            return d, serial_sum(g * d)


def solve(O, counts, mu, sf, disp, rows, Q=0.05, maxit=100):
    """dict(s, sf, F, iter, evals, flag); flag 0 converged (or an empty kept set), 1 maxit reached or no acceptable step,
    2 F at the start is not finite"""
    P = Problem(O, counts, mu, sf, disp, rows, Q)
    m = P.m
    s = P.start()
    e = _exp(O, s)
    L, cut, kept, F = P.evaluate(e)
    it, evals = 0, 1
    if not np.isfinite(F):
        flag = 2
    elif not kept.any():
        flag = 0
    else:
        while True:
            if it >= maxit:
                flag = 1
                break
            it += 1
            d, gd = P.step(*P.gradient(kept, e))
            t, accepted = 1.0, False
            for _ in range(MAX_TRIALS):
                with np.errstate(all="ignore"):
                    u = s + t * d
                    st = u - serial_sum(u) / m
                et = _exp(O, st)
                Lt, cutt, keptt, Ft = P.evaluate(et)
                evals += 1
                if Ft >= F + (ARMIJO * t) * gd:
                    accepted = True
                    break
                t = 0.5 * t
            if not accepted:
                flag = 0 if gd <= RELTOL * abs(F) else 1
                break
            gain = Ft - F
            s, e, L, cut, kept, F = st, et, Lt, cutt, keptt, Ft
            if gain <= RELTOL * abs(F):
                flag = 0
                break
    return {"s": s, "sf": e, "F": float(F), "iter": it, "evals": evals, "flag": flag}


def objective(O, counts, mu, sf, disp, rows, Q=0.05):
    """R's fn (R/core.R:2600-2606) as a function of p, on the specification's arithmetic: F at p - mean(p)"""
    P = Problem(O, counts, mu, sf, disp, rows, Q)

    def fn(p):
        p = np.asarray(p, np.float64)
        return P.evaluate(_exp(O, p - serial_sum(p) / P.m))[3]
    return fn
