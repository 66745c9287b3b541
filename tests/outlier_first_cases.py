"""Inputs shared by tests/test_outlier_bound_cpu.py and tests/test_gpu_outlier_first.py, and a numpy restatement of the bound
the cell kernel of csrc/fit_beta.hip evaluates per sample (cooks_can_exceed), operation by operation.

The outlier phase of the fused chain first handles the rows that CAN hold a count outlier: a sample's Cook's distance,
    V = mu + alpha (mu mu);  d = y - mu;  pr = (d d) / V;  ck = pr / p * h / ((1 - h)(1 - h)),
is largest at the floor of the robust dispersion, alpha = 0.04, so the distance at 0.04 bounds the real one from above."""
import numpy as np

from deseq2_amd import simulate

ALPHA_FLOOR = 0.04


def cooks_expr(y, mu, h, p, alpha):
    """cooks_kernel's expression (csrc/outlier.hip), IEEE double, in its operation order"""
    with np.errstate(all="ignore"):
        y, mu, h = np.asarray(y, np.float64), np.asarray(mu, np.float64), np.asarray(h, np.float64)
        V = mu + alpha * (mu * mu)
        d = y - mu
        pr = (d * d) / V
        omh = 1.0 - h
        return pr / float(p) * h / (omh * omh)


def sample_flag(y, mu, h, p, cutoff):
    """cooks_can_exceed: the sample makes its row a candidate"""
    with np.errstate(all="ignore"):
        B = cooks_expr(y, mu, h, p, ALPHA_FLOOR)
        return ~(B <= cutoff) | ~(np.asarray(h, np.float64) >= 0.0)


def sample_flag_divfree(y, mu, h, p, cutoff):
    """the -DDSQ_CAND_DIVFREE build of cooks_can_exceed: the same decision without a division, with a margin"""
    with np.errstate(all="ignore"):
        y, mu, h = np.asarray(y, np.float64), np.asarray(mu, np.float64), np.asarray(h, np.float64)
        V = mu + ALPHA_FLOOR * (mu * mu)
        d = y - mu
        omh = 1.0 - h
        L = (d * d) * h
        R = ((cutoff * float(p)) * V) * (omh * omh)
        below = (L * (1.0 + 2.0 ** -40) <= R) & (R >= 1e-280) & (R < np.inf) & (h >= 0.0) & (h < 1.0) & (cutoff * float(p) >= 1e-100)
        return ~below


def plant(counts, seed, rows=12):
    """single counts multiplied by factors from 3 to 1000 (some land on either side of the cutoff), and one row that is zero
    except for its outlier"""
    rng = np.random.default_rng(seed)
    c = counts.copy()
    n, m = c.shape
    pick = rng.choice(n, rows + 1, replace=False)
    factors = np.exp(rng.uniform(np.log(3.0), np.log(1000.0), rows))
    factors[:4] = (3.0, 10.0, 100.0, 1000.0)
    for r, f in zip(pick[:rows], factors):
        j = int(rng.integers(m))
        c[r, j] = int(max(c[r, j], 1) * f)
    c[pick[rows]] = 0
    c[pick[rows], int(rng.integers(m))] = 5000
    return c


def _counts(n, x, seed):
    m = x.shape[0]
    sf = np.exp(np.random.default_rng(seed + 1000).normal(0, 0.2, m))
    d = simulate.make_counts(n, x, seed=seed, size_factors=sf)
    c = d["counts"]
    if c.shape[0] < n:
        c = np.vstack([c, c[: n - c.shape[0]]])
    return c, sf


def chain_inputs():
    """the two shapes of both test files: name -> counts, x, sizeFactors"""
    out = {}
    for name, x, seed in (("two_group_28", simulate.design_two_group(28), 21),
                          ("batch_condition_48", simulate.design_batch_condition(48), 22)):
        c, sf = _counts(300, x, seed)
        out[name] = {"counts": plant(c, seed), "x": x, "sizeFactors": sf}
    return out


def variant_inputs():
    """the further cases of the GPU test"""
    out = {}
    c, sf = _counts(300, simulate.design_two_group(28), 23)
    out["no_outlier"] = {"counts": np.minimum(c, np.maximum(np.median(c, axis=1, keepdims=True).astype(c.dtype) * 2, 4)),
                         "x": simulate.design_two_group(28), "sizeFactors": sf}
    out["cutoff_zero"] = dict(chain_inputs()["two_group_28"], cutoff_zero=True)
    x2 = simulate.design_factor(16, 8)                                        # cells of two samples: no row replaceable
    c, sf = _counts(300, x2, 24)
    out["cells_of_two"] = {"counts": plant(c, 24), "x": x2, "sizeFactors": sf}
    xc = np.column_stack([simulate.design_two_group(28),                      # a continuous covariate: one cell per sample
                          np.random.default_rng(25).normal(0.0, 0.5, 28)])
    c, sf = _counts(300, xc, 25)
    out["continuous"] = {"counts": plant(c, 25), "x": xc, "sizeFactors": sf}
    return out
