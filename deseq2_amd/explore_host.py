"""Sample PCA and sample distances on the host: the sums of csrc/explore.hip in numpy, the same
operations in the same order, so that HostEngine.row_vars / top_var / pair_sums and dsq_top_var_dev / dsq_sample_pairs_dev
agree to the bit; and the small decomposition both engines share (LAPACK's symmetric eigen-solver on the m x m Gram matrix).
tests/explore_spec.py states the same arithmetic independently."""
import numpy as np

TILE = 64                          # kPairTile of csrc/dsq_internal.hpp
MIN_SLICE = 64                     # kPairMinSlice
WORK = 2048                        # kPairWork
KINDS = ("dist2", "dist", "gram")
PRCOMP_STOP = "infinite or missing values in 'x'"


def _wave_sum(T):
    """the wave-order sum along the last axis (dsq_wave.hpp wave_allreduce after the lanes' strided partial sums)"""
    m = T.shape[-1]
    part = np.zeros(T.shape[:-1] + (64,))
    for j0 in range(0, m, 64):
        w = min(64, m - j0)
        part[..., :w] = part[..., :w] + T[..., j0:j0 + w]
    lanes = np.arange(64)
    for off in (1, 2, 4, 8, 16, 32):
        part = part + part[..., lanes ^ off]
    return part[..., 0]


def row_vars(A):
    """(rowMean, rowVar) of an n x m matrix, m >= 2: row_vars_kernel's two wave-order sums"""
    A = np.asarray(A, np.float64)
    if A.ndim != 2 or A.shape[1] < 2:
        raise ValueError("row variances need a matrix of at least two columns")
    m = A.shape[1]
    with np.errstate(all="ignore"):
        mean = _wave_sum(A) / float(m)
        d = A - mean[:, None]
        var = _wave_sum(d * d) / float(m - 1)
    return mean, var


def top_var(rv, ntop):
    """order(rv, decreasing = TRUE)[seq_len(min(ntop, n))], 0-based: the stable sort of the inverted keys, NaN last"""
    rv = np.asarray(rv, np.float64)
    nan = np.isnan(rv)
    with np.errstate(all="ignore"):
        order = np.lexsort((np.arange(rv.size), np.where(nan, 0.0, -rv), nan))
    return order[:max(0, min(int(ntop), rv.size))].astype(np.int64)


def slice_rows(R, m):
    """the L of the summation order: a function of (rows summed, m) alone (pair_slices of csrc/explore.hip)"""
    nb = (m + TILE - 1) // TILE
    tiles = nb * (nb + 1) // 2
    cap = max(1, WORK // tiles)
    return max(MIN_SLICE, -(-int(R) // cap))


def pair_sums(A, kind, rows=None, centre=None):
    """the m x m all-pairs sums over the listed rows of A (all rows in order when rows is None): "dist2", its square root
    "dist", or the "gram" of the rows less centre (one value per listed row)"""
    if kind not in KINDS:
        raise ValueError("kind should be one of %s" % (KINDS,))
    A = np.asarray(A, np.float64)
    n, m = A.shape
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    if rows.size < 1 or m < 2:
        raise ValueError("pair sums need at least one row and two samples")
    if rows.min() < 0 or rows.max() >= n:
        raise ValueError("a row index is outside the matrix")
    R = rows.size
    L = slice_rows(R, m)
    total = None
    with np.errstate(all="ignore"):
        for r0 in range(0, R, L):
            acc = np.zeros((m, m))
            for t in range(r0, min(r0 + L, R)):
                a = A[rows[t]]
                if kind == "gram":
                    if centre is not None:
                        a = a - float(centre[t])
                    acc = acc + a[:, None] * a[None, :]
                else:
                    d = a[:, None] - a[None, :]
                    acc = acc + d * d
            total = acc if total is None else total + acc
        if kind != "gram":
            np.fill_diagonal(total, 0.0)
        if kind == "dist":
            total = np.sqrt(total)
    return total


def pca_from_gram(G, k):
    """prcomp from the m x m Gram matrix of the centred selection (k rows): dict(sdev, x, percentVar) of the first
    min(m, k) components.  The sign of a component is this library's rule: its entry of largest magnitude is positive
    (the lowest index on a tie)."""
    G = np.asarray(G, np.float64)
    m = G.shape[0]
    if not np.isfinite(G).all():
        raise ValueError(PRCOMP_STOP)
    lam, U = np.linalg.eigh(G)
    lam, U = np.maximum(lam[::-1], 0.0), U[:, ::-1]
    r = min(m, int(k))
    root = np.sqrt(lam[:r])
    sdev = np.sqrt(lam[:r] / float(max(1, m - 1)))
    x = U[:, :r] * root[None, :]
    top = np.argmax(np.abs(x), axis=0)
    x = np.where(x[top, np.arange(r)] < 0, -x, x)
    var = sdev * sdev
    with np.errstate(all="ignore"):
        return {"sdev": sdev, "x": np.ascontiguousarray(x), "percentVar": var / var.sum()}
