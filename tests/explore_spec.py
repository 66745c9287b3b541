"""The arithmetic specification of sample PCA and sample distances on a transform stated in numpy,
one operation per line: the reference for the exploration tests.  Not a test itself.  +, -, *, /, sqrt are IEEE, every
operation rounded once (the library is built with -ffp-contract=off).  Shares no code with the product
(deseq2_amd.explore_host, csrc/explore.hip).

What is restated, and from where:
  row_vars       matrixStats::rowVars as documented (the unbiased sample variance of each row); its source is not in the
                 reference tree, so the order of the two sums is this library's: the wave-order sum of DESIGN.md section 11.
  top_var        order(rv, decreasing = TRUE)[seq_len(min(ntop, length(rv)))]                            R/plots.R:248
  pair_sums      the sums behind prcomp's cross-product and dist(); the slice rule is this library's
  sample_dists   as.matrix(dist(t(A))), method "euclidean".  Base R's dist source is not in the reference tree.  Its
                 rescaling of sums with NA terms is NOT mirrored: a NaN in a sample gives NaN in every pair that sample
                 forms with another one (the diagonal stays 0, as as.matrix(dist) shows it).
  pca            prcomp(t(A[select, ])) with percentVar                                                 R/plots.R:245-254
                 The sign of a component is arbitrary in LAPACK and in R; the rule here (largest-magnitude score
                 positive, lowest index on a tie) is this library's."""
import numpy as np

from tests.sf_spec import wave_sum

# the constants of the slice rule
TILE = 64            # samples per side of a tile of pairs
LMIN = 64            # the shortest slice
WORK = 2048          # (tile, slice) pairs aimed at: a single tile is cut into up to WORK slices, and the partial sums of
#                      all slices take at most max(WORK, tiles) tiles of 64 x 64 doubles (64 MiB while tiles <= WORK)


def row_vars(A):
    """(mean, variance) per row of the n x m matrix A, m >= 2"""
    A = np.asarray(A, np.float64)
    n, m = A.shape
    assert m >= 2
    with np.errstate(all="ignore"):
        s = wave_sum(A)
        mean = s / m
        d = A - mean[:, None]
        q = d * d
        ss = wave_sum(q)
        var = ss / (m - 1)
    return mean, var


def top_var(rv, ntop):
    """variance descending, ties by ascending row index, NaN after every number by ascending index"""
    rv = [float(v) for v in np.asarray(rv, np.float64)]
    numbers = [i for i in range(len(rv)) if rv[i] == rv[i]]
    nans = [i for i in range(len(rv)) if rv[i] != rv[i]]
    numbers.sort(key=lambda i: (-rv[i], i))
    return np.array((numbers + nans)[:min(int(ntop), len(rv))], dtype=np.int64)


def slice_length(R, m):
    """L: the rows of one slice, a function of (rows summed, m) only"""
    nb = -(-m // TILE)
    tiles = nb * (nb + 1) // 2
    most_slices = max(1, WORK // tiles)
    return max(LMIN, -(-R // most_slices))


def pair_sums(A, kind, rows=None, centre=None, _skip_last_slice=False):
    """m x m.  kind "dist2": D2[i,j] = sum_g (A[g,i] - A[g,j]) (A[g,i] - A[g,j]); kind "gram": G[i,j] = sum_g c[g,i] c[g,j],
    c[g,.] = A[g,.] - centre[g] (centre aligned with the rows summed).  g runs over `rows` in list order, else over all rows.
    The rows summed are cut into slices of slice_length(R, m) consecutive entries; each slice is summed in order from +0.0;
    the slice partials are added in slice order.  Only j >= i is computed, then mirrored; the diagonal of dist2 is +0."""
    assert kind in ("dist2", "gram")
    A = np.asarray(A, np.float64)
    n, m = A.shape
    rows = list(range(n)) if rows is None else [int(g) for g in rows]
    R = len(rows)
    L = slice_length(R, m)
    starts = list(range(0, R, L))
    if _skip_last_slice:                     # (a mutation for the tests: never set otherwise)
        starts = starts[:-1] if len(starts) > 1 else starts
    iu = np.triu_indices(m)
    out = None
    with np.errstate(all="ignore"):
        for s0 in starts:
            part = np.zeros(len(iu[0]))
            for t in range(s0, min(s0 + L, R)):
                a = A[rows[t]]
                if kind == "gram" and centre is not None:
                    a = a - centre[t]
                if kind == "gram":
                    term = a[iu[0]] * a[iu[1]]
                else:
                    d = a[iu[0]] - a[iu[1]]
                    term = d * d
                part = part + term
            out = part if out is None else out + part
    full = np.zeros((m, m))
    full[iu] = out
    full.T[iu] = out
    if kind == "dist2":
        full[np.arange(m), np.arange(m)] = 0.0
    return full


def sample_dists(A):
    with np.errstate(all="ignore"):
        return np.sqrt(pair_sums(A, "dist2"))


def pca(A, ntop):
    """dict(select, sdev, x, percentVar, mean, var).  Raises ValueError where prcomp stops ("infinite or missing values in
    'x'"): a selected row with a non-finite variance."""
    A = np.asarray(A, np.float64)
    n, m = A.shape
    mean, var = row_vars(A)
    select = top_var(var, ntop)
    k = len(select)
    if not np.isfinite(var[select]).all():
        raise ValueError("infinite or missing values in 'x'")
    G = pair_sums(A, "gram", rows=select, centre=mean[select])
    lam, U = np.linalg.eigh(G)
    lam = lam[::-1]
    U = U[:, ::-1]
    lam = np.maximum(lam, 0.0)
    r = min(m, k)
    lam = lam[:r]
    sdev = np.sqrt(lam / max(1, m - 1))
    x = U[:, :r] * np.sqrt(lam)
    for c in range(r):
        mag = np.abs(x[:, c])
        top = int(np.flatnonzero(mag == mag.max())[0])
        if x[top, c] < 0:
            x[:, c] = -x[:, c]
    v = sdev * sdev
    with np.errstate(all="ignore"):
        pv = v / v.sum()
    return {"select": select, "sdev": sdev, "x": x, "percentVar": pv, "mean": mean, "var": var, "G": G}
