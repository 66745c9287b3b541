"""Seeded inputs shared by the rlog tests (tests/test_rlog_cpu.py, tests/test_gpu_rlog.py).  Not a test itself."""
import numpy as np

RTOL = 1e-11          # rlog values against the dense fit, relative to max(|v|, 1)
TIE_CAP = 0.01        # share of a case's rows whose iteration count may differ by a last-bit tie of the convergence test


def inputs(n, m, seed, nf_matrix=False, zero_row=True):
    """negative binomial counts around exp(N(3, 2.5)) with log fold changes of sd 1 between the samples, size factors
    (or a normalization-factor matrix), a dispersion trend at the gene's mean and a prior variance in [0.05, 2]"""
    rng = np.random.default_rng(1000 * m + seed)
    base = np.exp(rng.normal(3.0, 2.5, n))
    sf = np.exp(rng.normal(0.0, 0.3, m))
    nf = sf[None, :] * np.exp(rng.normal(0.0, 0.2, (n, m))) if nf_matrix else sf
    NF = nf if nf_matrix else np.broadcast_to(sf[None, :], (n, m))
    disp = 0.05 + 1.0 / np.maximum(base, 0.5)
    mu = base[:, None] * np.exp(rng.normal(0.0, 1.0, (n, m))) * NF
    k = rng.poisson(rng.gamma(1.0 / disp[:, None], mu * disp[:, None]))
    k = np.minimum(k, 2 ** 31 - 1).astype(np.int32)
    if zero_row and n > 3:
        k[3] = 0
    return {"counts": k, "nf": nf, "dispFit": disp, "betaPriorVar": float(rng.uniform(0.05, 2.0))}


def compare(got, want, what, it_got=None, it_want=None, rtol=RTOL):
    """iteration counts equal but for at most TIE_CAP of the rows (left out of the value check), values within rtol
    relative to max(|v|, 1); returns (rows with another iteration count, largest relative difference)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    keep = np.ones(got.shape[0], bool)
    ties = 0
    if it_got is not None:
        keep = np.asarray(it_got) == np.asarray(it_want)
        ties = int((~keep).sum())
        assert ties <= TIE_CAP * keep.size, "%s: %d of %d rows differ in their iteration count" % (what, ties, keep.size)
    g, w = got[keep], want[keep]
    assert (np.isnan(g) == np.isnan(w)).all(), "%s: NaN pattern" % what
    same = (g == w) | (np.isnan(g) & np.isnan(w))
    with np.errstate(all="ignore"):
        rel = np.where(same, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1.0))
    worst = float(rel.max()) if rel.size else 0.0
    print("%s: rows with another iteration count %d / %d, largest relative difference %.3g" % (what, ties, keep.size, worst))
    assert worst <= rtol, "%s: relative difference %.3g > %.3g" % (what, worst, rtol)
    return ties, worst
