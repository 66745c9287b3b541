"""Seeded inputs shared by the rlog tests (tests/test_rlog_cpu.py, tests/test_gpu_rlog.py).  Not a test itself."""
import numpy as np

RTOL = 1e-11          # rlog values against the dense fit, relative to max(|v|, 1)
TIE_CAP = 0.01        # share of a case's rows whose iteration count may differ by a last-bit tie of the convergence test
LN2 = np.log(2.0)


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


def dense_design(k, nf, disp, bpv, intercept=None):
    """what rlogData (R/rlog.R:172-272) hands fitBeta for the rows that are fitted: the dense design [1 | I_m] (form A) or
    I_m with the intercept folded into the factors (form B), its ridge, start values and fixed arguments.  Returns
    (rows, x, args): args is the positional argument list of a fitBeta (the C oracle's or the LAPACK restatement's)."""
    k = np.asarray(k, np.float64)
    n, m = k.shape
    NF = np.broadcast_to(nf[None, :], (n, m)) if np.ndim(nf) == 1 else np.asarray(nf, np.float64)
    if intercept is None:
        rows = np.where((k != 0).any(axis=1))[0]
        x = np.hstack([np.ones((m, 1)), np.eye(m)])
        lam = np.r_[1e-6, np.full(m, 1.0 / bpv)]
        NFs = NF[rows]
        b0 = np.zeros((rows.size, m + 1))
        b0[:, 0] = np.log((k[rows] / NFs).mean(axis=1))
    else:
        rows = np.where(np.isfinite(intercept))[0]
        x = np.eye(m)
        lam = np.full(m, 1.0 / bpv)
        NFs = NF[rows] * (2.0 ** intercept[rows])[:, None]
        b0 = np.log(k[rows] / NFs + 0.1)
    p = x.shape[1]
    args = (k[rows], x, NFs, disp[rows], np.r_[1.0, np.zeros(p - 1)], b0, lam / LN2 ** 2, np.ones((rows.size, m)), False,
            1e-4, 100, True, 0.5)
    return rows, x, args


def dense_values(x, r, rows, intercept=None):
    """the rlog values of a dense fit r = fitBeta(*args): log2(e) beta X' (+ the frozen intercept)"""
    v = (np.log2(np.e) * r["beta_mat"]) @ x.T
    if intercept is not None:
        v = v + np.asarray(intercept)[rows][:, None]
    return v


def dense_lapack(k, nf, disp, bpv, intercept=None):
    """the reference's route on the rows that are fitted, over the LAPACK restatement (oracle/lapack_oracle.py: numpy's QR
    and solve, no width limit): returns (rows, rlog values, iter)"""
    from oracle import lapack_oracle
    rows, x, args = dense_design(k, nf, disp, bpv, intercept)
    r = lapack_oracle.fitBeta(*args)
    return rows, dense_values(x, r, rows, intercept), r["iter"]


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


_LAPACK = {}


def lapack_case(O, n, m):
    """inputs(n, m, seed=2) with both forms of the specification and of the LAPACK route on them, computed once per shape
    and left unchanged: form A, then form B on the intercepts form A returned with one made non-finite (row 5) and one
    finite intercept on all-zero counts (row 7)"""
    from tests import rlog_spec
    if (n, m) not in _LAPACK:
        d = inputs(n, m, seed=2)
        k, nf, disp, bpv = d["counts"], d["nf"], d["dispFit"], d["betaPriorVar"]
        sa = rlog_spec.rlog_fit(O, k, nf, disp, bpv)
        c = np.array(sa["intercept"])
        c[5] = np.nan
        k2 = k.copy()
        k2[7] = 0
        sb = rlog_spec.rlog_fit(O, k2, nf, disp, bpv, intercept=c)
        _LAPACK[(n, m)] = dict(d=d, k2=k2, c=c, specA=sa, specB=sb, lapackA=dense_lapack(k, nf, disp, bpv),
                               lapackB=dense_lapack(k2, nf, disp, bpv, intercept=c))
    return _LAPACK[(n, m)]


def mutants(rlog, it, rows):
    """two copies of a result the comparison must refuse: one value of a fitted row moved by 3e-11 relative (an element of
    magnitude >= 1, so that the move is 3e-11 of max(|v|, 1) too), one iteration count off by one"""
    v = np.array(rlog)
    sub = np.abs(v[rows])
    a, b = np.unravel_index(np.argmax(np.where(np.isfinite(sub), sub, 0.0)), sub.shape)
    assert sub[a, b] >= 1.0
    v[rows[a], b] *= 1.0 + 3e-11
    i2 = np.array(it)
    i2[rows[len(rows) // 2]] += 1.0
    return (v, np.array(it)), (np.array(rlog), i2)
