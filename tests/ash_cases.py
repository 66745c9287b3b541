"""The cases of the ash tests (tests/test_ash_cpu.py, tests/test_gpu_ash.py): seeded (betahat, sebetahat) columns on the
smallest shapes at which the kernels of csrc/ash.hip can go wrong.  Not a test itself."""
import numpy as np

SLICE = 128                    # dsq_ash_slice_rows()


def column(n, seed, m=12, null=0.8, wide=1.5):
    """fold changes of a two-group experiment with m samples: 80 % near zero, 20 % spread; standard errors from a gamma"""
    r = np.random.default_rng(seed)
    s = np.sqrt(r.gamma(4.0, 1.5 / m, n)) + 0.05
    beta = np.where(r.random(n) < null, r.normal(0.0, 0.05, n), r.normal(0.0, wide, n))
    return beta + s * r.normal(size=n), s


def null_column(n, seed):
    """no row with b^2 > s^2: the grid falls back to 8 smin, K = 7"""
    r = np.random.default_rng(seed)
    s = r.uniform(0.2, 1.0, n)
    return s * r.uniform(-0.9, 0.9, n), s


def wide_column(n, seed, top=127.7):
    """max / min of the grid near 2^31.25: K = 64 (top = 127.7); beyond 2^31.5: K = 65 (top = 170)"""
    b, s = column(n, seed)
    s[0], b[0] = 1e-6, 2e-6
    s[1 % n], b[1 % n] = 1.0, top
    return b, s


def exclude(b, s, rows):
    """rows of each kind that are not kept: NaN estimate, NaN / zero / negative / infinite standard error"""
    b, s = b.copy(), s.copy()
    kinds = ((np.nan, None), (None, np.nan), (None, 0.0), (None, -1.0), (None, np.inf), (np.inf, None))
    for j, i in enumerate(rows):
        vb, vs = kinds[j % len(kinds)]
        if vb is not None:
            b[i] = vb
        if vs is not None:
            s[i] = vs
    return b, s


def _stack(cols):
    return np.column_stack([c[0] for c in cols]), np.column_stack([c[1] for c in cols])


def gpu_cases():
    """name -> dict(b, s: n x C; threshold)"""
    out = {}
    for n in (1, 63, 64, 65, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1):
        b, s = column(n, 100 + n)
        out["n%d" % n] = dict(b=b[:, None], s=s[:, None], threshold=None if n % 2 else 0.5)
    b, s = null_column(150, 3)
    out["K7"] = dict(b=b[:, None], s=s[:, None], threshold=1.0)
    b, s = column(200, 5, m=6, wide=2.5)
    out["K_odd"] = dict(b=b[:, None], s=s[:, None], threshold=None)
    b, s = wide_column(70, 7)
    out["K64"] = dict(b=b[:, None], s=s[:, None], threshold=0.25)
    b, s = exclude(*column(2 * SLICE + 9, 9), (0, 63, 64, SLICE - 1, SLICE, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 8))
    out["excluded"] = dict(b=b[:, None], s=s[:, None], threshold=0.5)
    b, s = _stack([null_column(300, 11), column(300, 12), exclude(*column(300, 13, m=6, wide=3.0), (5, 127, 128, 299))])
    out["C3"] = dict(b=b, s=s, threshold=None)
    out["C3_T"] = dict(b=b, s=s, threshold=1.0)
    return out


def seeded(n, m, seed=1):
    return column(n, seed, m=m)
