"""Inputs and tolerances shared by tests/test_explore_cpu.py and tests/test_gpu_explore.py (sample PCA and sample
distances).  Not a test itself.  Every reference is computed once and cached."""
import functools

import numpy as np

from tests import explore_spec as S

L = S.LMIN                                                  # the slice length at the shapes below (one or few tiles)
M_LIST = (2, 3, 63, 64, 65, 129, 200)
ROWS_SUMMED = (1, 2, L - 1, L, L + 1, 3 * L + 7)
U = 2.0 ** -53


def matrix(n, m, seed, scale=3.0, shift=8.0):
    """transform-like values: positive, of one sign, rows of different spread"""
    rng = np.random.Generator(np.random.PCG64(seed))
    spread = rng.uniform(0.05, 1.0, size=(n, 1)) * scale
    return shift + spread * rng.normal(size=(n, m)).clip(-2.5, 2.5)


def row_lists(n, seed):
    """a single row, all rows, a permutation, repeated indices"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return {"single": np.array([n // 2]), "all": np.arange(n), "permutation": rng.permutation(n),
            "repeated": rng.integers(0, n, size=n + 9)}


def selection_matrix(n=40, m=6, seed=5):
    """rows with duplicate rows (tied variances), constant rows (variance 0, tied), NaN rows in the middle and at the end"""
    A = matrix(n, m, seed)
    A[7] = A[3]
    A[21] = A[3]
    A[10] = 4.0
    A[11] = 9.5
    A[30] = A[2]
    A[15, 2] = np.nan
    A[16] = np.nan
    A[n - 1, 0] = np.nan
    return A


def lexsort_order(rv):
    """numpy.lexsort on (index, -variance with NaN last)"""
    rv = np.asarray(rv, np.float64)
    nan = np.isnan(rv)
    with np.errstate(all="ignore"):
        return np.lexsort((np.arange(rv.size), np.where(nan, np.inf, -rv), nan))


# ---------------------------------------------------------------------------------------------- independent statements
def var_longdouble(A):
    return np.var(np.asarray(A, np.longdouble), axis=1, ddof=1)


def var_bound(m):
    """|var - exact| <= (m + 4) 2^-53 |exact| for the two-pass form on rows of one sign, bounded away from constant.
    Derivation, u = 2^-53.  (1) The computed mean differs from the exact one by e with |e| <= c u |mean|, c <= m / 64 + 8 (the
    lane sums, six butterfly steps, the division).  Shifting every deviation by e changes sum d^2 by m e^2 only, because the
    exact deviations sum to 0: a second-order term, below u |exact| as soon as the row's coefficient of variation exceeds
    c sqrt(u) ~ 1e-7 -- "bounded away from constant"; the cases keep it above 1e-3.  (2) Each term is d = fl(a - mean), one
    rounding, squared with one more: d^2 (1 + u)^3, i.e. 3 u.  (3) A sum of m NON-NEGATIVE terms in any order adds at most
    (m - 1) u relative (a term passes through at most m - 1 additions that round; adding 0.0 is exact).  (4) The division by
    m - 1 rounds once.  Together (3 + (m - 1) + 1) u = (m + 3) u to first order, and one more u covers (1) and the
    second-order terms: (m + 4) u.  Rows of one sign make the mean's relative error meaningful; a constant row gives d = 0
    exactly and is compared for 0."""
    return (m + 4) * U


def dist_bound(R):
    """|d - exact| <= ((R + 3) / 2 + 1) 2^-53 d for R rows summed.  Each term (a_i - a_j)^2 carries 3 u (the difference
    rounded once and squared, the square rounded); a sum of R non-negative terms in any order adds at most (R - 1) u ...
    R u: the squared distance is within (R + 3) u of exact.  The square root halves a relative error and rounds once."""
    return ((R + 3) / 2.0 + 1.0) * U


def dist_longdouble(A):
    A = np.asarray(A, np.longdouble)
    d = A[:, :, None] - A[:, None, :]
    return np.sqrt((d * d).sum(axis=0))


def gram_longdouble(C):
    """exact Gram of the f64 centred values C (k x m) and the sum of |c_gi| |c_gj| its bound scales with"""
    C = np.asarray(C, np.longdouble)
    return C.T @ C, np.abs(C).T @ np.abs(C)


def gram_bound(k):
    """|G_ij - exact| <= (k + 2) 2^-53 sum_g |c_gi| |c_gj| over the SAME f64 centred values: each product rounds once, a sum
    of k terms in any order adds at most (k - 1) u times the sum of the terms' magnitudes; two u of room for second order"""
    return (k + 2) * U


def prcomp_svd(A, select):
    """prcomp(t(A[select, ])) over LAPACK's SVD: centre each selected gene, svd, sdev = d / sqrt(m - 1), x = Xc V, signs by
    the library's rule; and d itself (for the choice of the components compared)"""
    X = np.asarray(A, np.float64)[np.asarray(select)].T                 # m x k
    m = X.shape[0]
    Xc = X - X.mean(axis=0, keepdims=True)
    u, d, vt = np.linalg.svd(Xc, full_matrices=False)
    x = Xc @ vt.T
    for c in range(x.shape[1]):
        top = int(np.argmax(np.abs(x[:, c])))
        if x[top, c] < 0:
            x[:, c] = -x[:, c]
    sdev = d / np.sqrt(m - 1.0)
    return {"sdev": sdev, "x": x, "percentVar": sdev ** 2 / (sdev ** 2).sum(), "d": d}


def comparable(d):
    """the components held to the SVD statement: eigenvalue (d^2) at least 1e-6 of the largest, relative gap of the
    eigenvalue to both neighbours at least 1e-3"""
    lam = np.asarray(d, np.float64) ** 2
    keep = []
    for i in range(lam.size):
        if lam[i] < 1e-6 * lam[0]:
            continue
        gaps = [abs(lam[i] - lam[j]) / lam[i] for j in (i - 1, i + 1) if 0 <= j < lam.size]
        if all(g >= 1e-3 for g in gaps):
            keep.append(i)
    return keep


# The largest deviation HostEngine's pca shows against prcomp_svd on the two inputs below, over the comparable components
# (tests/test_explore_cpu.py pca_deviation, which prints it): |sdev - sdev_svd| / sdev_svd and |percentVar - percentVar_svd| /
# percentVar_svd per component, max |x - x_svd| / max |x_svd| per component.  Measured on the host engine only -- never against
# the device.  The tolerance is ten times that: a Gram route's error grows with (d_1 / d_i)^2.  On both inputs 11 of the 12
# components are compared (the twelfth is the null direction of the centring), PC1 and PC2 among them.
PCA_MEASURED = {"planted": 4.24e-13, "example": 5.38e-14}
PCA_TOL = {k: 10 * v for k, v in PCA_MEASURED.items()}
PCA_COMPARED = {"planted": 11, "example": 11}


@functools.lru_cache(maxsize=None)
def pca_input(which):
    """(A, factors): the transformed matrix (host) and the design factors.
    planted: simulate.make_counts with three planted groups of four samples, through vst on HostEngine(oracle);
    example: makeExampleDESeqDataSet's defaults (n = 1000, m = 12, two conditions, betaSD = 0, dispersion 4 / mu + 0.1;
    tests/testthat/test_plots.R:16-18 runs plotPCA on such an object) through varianceStabilizingTransformation."""
    from oracle import oracle as O
    from deseq2_amd import core, simulate
    from deseq2_amd.engine import HostEngine
    E = HostEngine(O)
    if which == "planted":
        m = 12
        x = simulate.design_factor(m, 3)
        d = simulate.make_counts(1500, x, seed=23, beta_sd=np.array([2.0, 2.0]))
        dds = core.DESeqDataSet(d["counts"], x, sizeFactors=np.ones(m), engine=E)
        vsd = core.vst(dds, blind=True, nsub=500)
        factors = {"condition": (np.arange(m) * 3) // m, "batch": np.arange(m) % 2}
    elif which == "example":
        n, m = 1000, 12
        rng = np.random.default_rng(7)
        b0 = rng.normal(4, 2, n)
        mu = np.broadcast_to(2.0 ** b0[:, None], (n, m))
        size = 1.0 / (4.0 / 2.0 ** b0 + 0.1)[:, None]
        counts = rng.negative_binomial(np.broadcast_to(size, mu.shape), size / (size + mu)).astype(np.int32)
        x = simulate.design_two_group(m)
        dds = core.DESeqDataSet(counts, x, sizeFactors=np.ones(m), engine=E)
        vsd = core.varianceStabilizingTransformation(dds, blind=True)
        factors = {"condition": (np.arange(m) >= m // 2).astype(int)}
    else:
        raise ValueError(which)
    A = np.array(vsd.assay(), dtype=np.float64, order="C")
    A.setflags(write=False)
    return A, factors
