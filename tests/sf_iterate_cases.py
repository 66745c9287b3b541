"""Seeded inputs for the sf_iterate tests (numpy PCG64).  Not a test itself.

solve_case: the inputs of ONE solve with synthetic dispersions (the kernel apart from the chain): negative binomial counts
around q_i * true_sf_j, a planted zero per gene, mu = the intercept fit at the given current factors (floored at 0.5, as
the chain floors it).  testthat_case: the data of tests/testthat/test_size_factor.R:20-29 with numpy's generator."""
import numpy as np


def solve_case(n_rows, m, seed, interleave=False, dup=1, outlier=True, disp_edges=False, far=False):
    """n_rows rows that take part (each distinct row repeated `dup` times, adjacent: ties in L), with interleave two excluded
    rows (all-zero counts, NaN dispersion, flag 0) after every third one.  far: the current factors are far from the optimum.
    Returns dict(counts int32 n x m, mu n x m, sf m, disp n, rows n int32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nd = -(-n_rows // dup)
    true_sf = np.exp(rng.normal(0.0, 0.5, m))
    q = np.exp(rng.normal(4.0, 1.5, (nd, 1)))
    a = rng.uniform(0.01, 0.5, nd)
    mean = q * true_sf[None, :]
    k = rng.negative_binomial(1.0 / a[:, None], 1.0 / (1.0 + mean * a[:, None])).astype(np.int64)
    k[np.arange(nd), rng.integers(0, m, nd)] = 0
    if outlier:
        k[0, 0] = 10 ** 6
    k[k.sum(axis=1) == 0, 0] = 1                      # (a row that takes part has a positive sum)
    if disp_edges:
        a[1::5] = 1e-8                                # the dispersion floor
        a[2::5] = 1e-12                               # counts below 1e-10 size: cells outside the closed split
        a[3::5] = max(10.0, m)                        # the ceiling
    k, a = np.repeat(k, dup, axis=0)[:n_rows], np.repeat(a, dup)[:n_rows]
    sf = np.exp(rng.normal(0.0, 1.5, m)) if far else np.exp(rng.normal(0.0, 0.1, m)) * true_sf
    mu = np.maximum((k / sf[None, :]).mean(axis=1, keepdims=True) * sf[None, :], 0.5)
    rows = np.ones(n_rows, np.int32)
    if interleave:
        pos = np.repeat(np.arange(3, n_rows + 1, 3), 2)             # two excluded rows after every third row
        k = np.insert(k, pos, 0, axis=0)
        mu = np.insert(mu, pos, 0.5, axis=0)
        a = np.insert(a, pos, np.nan)
        rows = np.insert(rows, pos, 0)
    return {"counts": np.ascontiguousarray(k, dtype=np.int32), "mu": np.ascontiguousarray(mu), "sf": sf, "disp": a, "rows": rows}


def testthat_case(n, seed=1):
    """(counts n x 12, true.sf): true.sf = 2^(rep(c(-2,-1,0,0,1,2), each = 2)), makeExampleDESeqDataSet's means 2^N(4, 2),
    dispersion 0.01, one planted zero per gene, cts[1, 1] = 1000000"""
    rng = np.random.default_rng(seed)
    true_sf = 2.0 ** np.repeat([-2, -1, 0, 0, 1, 2], 2)
    m = 12
    mean = 2.0 ** rng.normal(4, 2, (n, 1)) * true_sf[None, :]
    disp = 0.01
    cts = rng.negative_binomial(1.0 / disp, 1.0 / (1.0 + mean * disp)).astype(np.int64)
    cts[np.arange(n), rng.integers(0, m, n)] = 0
    cts[0, 0] = 1000000
    return cts, true_sf
