"""The local-regression dispersion trend (fitType = "local") in numpy: csrc/local_fit.hip's operations
in the same order, so that HostEngine.local_fit and dsq_local_fit_dev give the same bits (tests/local_fit_spec.py states
the arithmetic one evaluation point at a time; here the points go in batches and the fit set is swept once per batch).

vlog / vexp: the engine's pinned log / exp (csrc/dsq_math.hpp).  LANES: the partial sums of every moment (dsq_local_fit_lanes
of the C ABI): partial (j mod LANES) takes the window's points in ascending j, then the butterfly of dsq_wave.hpp."""
import numpy as np

LANES = 64
TOO_FEW = "local dispersion fit: fewer than 3 points in a window"
_BATCH = 2048


def bandwidth(N):
    return (7 * int(N)) // 10


class LocalFit:
    """x | y | w of the fit set in sorted order (the fit handle), N, k; calling it evaluates dispFit at the given means"""

    def __init__(self, vlog, vexp, means, disps, minDisp=1e-8):
        means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1)
        disps = np.ascontiguousarray(disps, dtype=np.float64).reshape(-1)
        if means.shape != disps.shape:
            raise ValueError("means and disps must have one entry per gene each")
        self.vlog, self.vexp, self.minDisp = vlog, vexp, float(minDisp)
        with np.errstate(invalid="ignore"):
            keep = np.flatnonzero((disps >= 10 * self.minDisp) & (disps < np.inf) & (means > 0) & (means < np.inf))
        x = vlog(means[keep]) if keep.size else np.zeros(0)
        o = np.argsort(x, kind="stable")
        rows = keep[o]
        self.x, self.y, self.w = x[o], (vlog(disps[rows]) if rows.size else np.zeros(0)), means[rows].copy()
        self.N, self.k = int(rows.size), bandwidth(rows.size)
        self.allBelowFloor = self.N == 0
        self.nSingular = 0
        if self.N and self.k < 3:
            raise RuntimeError(TOO_FEW)

    def _window(self, z):
        x, k = self.x, self.k
        lo = np.zeros(z.size, np.int64)
        hi = np.full(z.size, self.N - k, np.int64)
        while True:
            live = lo < hi
            if not live.any():
                break
            mid = (lo + hi) // 2
            up = np.zeros(z.size, bool)
            up[live] = x[mid[live] + k] - z[live] < z[live] - x[mid[live]]
            lo = np.where(live & up, mid + 1, lo)
            hi = np.where(live & ~up, mid, hi)
        return lo, np.maximum(z - x[lo], x[lo + k - 1] - z)

    def _solve(self, S, T, distinct):
        S0, S1, S2, S3, S4 = S
        T0, T1, T2 = T
        with np.errstate(all="ignore"):
            m1 = S1 / S0
            m2 = S2 / S0
            A11 = S2 - m1 * S1
            A12 = S3 - m1 * S2
            A22 = S4 - m2 * S2
            b1 = T1 - m1 * T0
            b2 = T2 - m2 * T0
            m3 = A12 / A11
            p2 = A22 - m3 * A12
            c2 = b2 - m3 * b1
            a2 = c2 / p2
            a1 = (b1 - A12 * a2) / A11
            a0 = ((T0 - S1 * a1) - S2 * a2) / S0
            ok = (distinct >= 3) & (S0 > 0) & (A11 > 0) & (p2 > 0)
        return np.where(ok, a0, np.nan)

    def _batch(self, z):
        x, y, w, k = self.x, self.y, self.w, self.k
        l, h = self._window(z)
        part = np.zeros((8, z.size, LANES))
        distinct = np.zeros(z.size, np.int64)
        lanes = np.arange(LANES)
        with np.errstate(all="ignore"):
            for c in range(int(l.min()) // LANES, (int(l.max()) + k - 1) // LANES + 1):
                j = c * LANES + lanes
                jc = np.minimum(j, self.N - 1)
                xj, yj = x[jc], y[jc]
                t = (xj[None, :] - z[:, None]) / h[:, None]
                a = np.abs(t)
                live = (j[None, :] >= l[:, None]) & (j[None, :] < (l + k)[:, None]) & (a < 1)
                u = 1 - (a * a) * a
                c0 = w[jc][None, :] * ((u * u) * u)
                c1 = c0 * t
                c2 = c1 * t
                c3 = c2 * t
                c4 = c3 * t
                for r, v in enumerate((c0, c1, c2, c3, c4, c0 * yj, c1 * yj, c2 * yj)):
                    part[r] = part[r] + np.where(live, v, 0.0)
                prev = x[np.maximum(jc - 1, 0)]
                distinct += (live & (c0 > 0) & ((j[None, :] == l[:, None]) | (xj != prev)[None, :])).sum(axis=1)
            for off in (1, 2, 4, 8, 16, 32):
                part = part + part[..., lanes ^ off]
        m = part[..., 0]
        return self._solve(m[:5], m[5:], distinct)

    def __call__(self, q):
        q = np.asarray(q, np.float64)
        flat = np.ascontiguousarray(q).reshape(-1)
        if self.allBelowFloor:
            return np.full(q.shape, self.minDisp)
        out = np.full(flat.shape, np.nan)
        with np.errstate(invalid="ignore"):
            ok = np.flatnonzero((flat > 0) & (flat < np.inf))
        z = self.vlog(flat[ok]) if ok.size else np.zeros(0)
        a0 = np.concatenate([self._batch(z[b:b + _BATCH]) for b in range(0, z.size, _BATCH)]) if ok.size else np.zeros(0)
        fin = np.isfinite(a0)
        val = np.where(a0 == -np.inf, 0.0, a0)                       # sf_exp: NaN and +Inf stay, exp(-Inf) = 0
        if fin.any():
            val[fin] = self.vexp(np.ascontiguousarray(a0[fin]))
        out[ok] = val
        self.nSingular = int(np.isnan(val).sum())
        return out.reshape(q.shape)
