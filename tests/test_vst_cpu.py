"""The variance stabilizing transformation without a GPU: the host statement (HostEngine.vst_transform / row_stats, core.vst)
against the numpy specification of tests/vst_spec.py; the specification itself against mpmath; the spline table by its
properties (no output of R's splinefun exists here); vst()'s subset rule."""

import numpy as np
import pytest

from tests import vst_spec

U = 2.0 ** -52


spec_bound, spline_bound, ASINH_ULPS = vst_spec.spec_bound, vst_spec.spline_bound, vst_spec.ASINH_ULPS


def _counts(n, m, seed, zeros=0.1):
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.normal(6, 2.5, (n, 1)) * np.exp(rng.normal(0, 0.4, m))[None, :]
    k = rng.poisson(mu).astype(np.int64)
    k[rng.uniform(size=k.shape) < zeros] = 0
    k[3] = 0
    k[0, :] = 2 ** 31 - 1
    return np.minimum(k, 2 ** 31 - 1).astype(np.int32)


def _trend(mu):
    return 0.05 + 2.0 / mu


PARAMS = {"parametric": [dict(asymptDisp=a, extraPois=e) for a, e in ((1e-4, 1e-2), (1e-2, 1e3), (0.1, 1.0), (10.0, 30.0))],
          "mean": [dict(alpha=a) for a in (1e-4, 0.07, 10.0)], "log2": [dict(pc=1.0), dict(pc=0.5)], "normalized": [{}]}


@pytest.mark.parametrize("nfkind", ["size_factors", "norm_matrix"])
@pytest.mark.parametrize("kind", ["parametric", "mean", "log2", "normalized", "spline"])
def test_host_statement_matches_the_specification(oracle, kind, nfkind):
    """Both sides are within spec_bound / spline_bound of the exact value at the same q (q = k / nf is one IEEE division on
    both sides): they are at most twice that apart."""
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine, spline_eval
    n, m = 400, 9
    k = _counts(n, m, 3)
    rng = np.random.default_rng(8)
    nf = np.exp(rng.normal(0, 0.3, m)) if nfkind == "size_factors" else np.exp(rng.normal(0, 0.3, (n, m)))
    E = HostEngine(oracle)
    y = E.counts(k)
    hkw = dict(sizeFactors=nf, nf=None) if nf.ndim == 1 else dict(nf=E.matrix(nf))
    q = vst_spec.normalized(k, nf)
    if kind == "spline":
        table = core.vst_spline_table(_trend, float(q.max()), 1.0)
        plist = [dict(table=table, eta=1.3, xi=-2.0)]
    else:
        plist = PARAMS[kind]
    for params in plist:
        ref = vst_spec.transform(oracle, k, nf, kind, **params)
        got = np.asarray(E.vst_transform(y, hkw.get("nf"), kind, sizeFactors=hkw.get("sizeFactors"), **params))
        assert np.isfinite(ref).all()
        if kind == "normalized":
            np.testing.assert_array_equal(got, ref)
            continue
        if kind == "spline":
            bound = 2 * spline_bound(table, 1.3, -2.0, np.arcsinh(q), ref)
        elif kind == "mean":
            bound = 2 * spec_bound("mean", ref, A=np.arcsinh(np.sqrt(params["alpha"] * q)), la=np.log(params["alpha"]))
        else:
            bound = 2 * spec_bound(kind, ref)
        err = np.abs(got - ref)
        print("%s %s %r: max |host - spec| = %.3g, smallest bound %.3g" % (kind, nfkind, {k_: v for k_, v in params.items() if k_ != "table"},
                                                                           err.max(), bound.min()))
        assert (err <= bound).all()
    mean, mx = E.row_stats(y, hkw.get("nf"), sizeFactors=hkw.get("sizeFactors"))
    rmean, rmx = vst_spec.row_stats(k, nf)
    np.testing.assert_array_equal(mx, rmx)
    # an m-term sum in another order: (m - 1) roundings at the size of the sum of non-negative terms
    np.testing.assert_allclose(mean, rmean, rtol=m * U, atol=0)


def test_asinh_definition_against_mpmath(oracle):
    """the three-range asinh of the specification from 0 through 2^60; mid range: the argument of log1p is built by six
    operations of which the quotient's three count at most half (t / (1 + r) <= x / 2 ... x): < 5 ulps of an argument the
    logarithm does not amplify (w / ((1 + w) log1p(w)) <= 1), one for log1p, and a binade step between argument and
    result may double the figure in ulps of the RESULT: <= ASINH_ULPS = 8 asserted; the figure seen is printed."""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(1)
    x = np.concatenate([[0.0, 2.0 ** -28, np.nextafter(2.0 ** -28, 0), 2.0, np.nextafter(2.0, 3), 2.0 ** 28,
                         np.nextafter(2.0 ** 28, np.inf), 2.0 ** 60], 2.0 ** rng.uniform(-40, 60, 4000), rng.uniform(0, 4, 1000)])
    got = vst_spec.asinh(oracle, x)
    worst = 0.0
    for xi, gi in zip(x.tolist(), got.tolist()):
        ex = mp.asinh(mp.mpf(xi))
        if xi == 0.0:
            assert gi == 0.0
            continue
        ulp = np.spacing(abs(float(ex)))
        worst = max(worst, float(abs(mp.mpf(gi) - ex) / mp.mpf(ulp)))
    print("asinh: largest error %.3f ulps over %d arguments in [0, 2^60]" % (worst, x.size))
    assert worst <= ASINH_ULPS
    assert np.isnan(vst_spec.asinh(oracle, np.array([np.nan]))[0]) and vst_spec.asinh(oracle, np.array([np.inf]))[0] == np.inf


def _exact(kind, q, p):
    import mpmath as mp
    q = mp.mpf(q)
    if kind == "parametric":
        a, e = mp.mpf(p["asymptDisp"]), mp.mpf(p["extraPois"])
        return mp.log((1 + e + 2 * a * q + 2 * mp.sqrt(a * q * (1 + e + a * q))) / (4 * a)) / mp.log(2)
    if kind == "mean":
        al = mp.mpf(p["alpha"])
        return (2 * mp.asinh(mp.sqrt(al * q)) - mp.log(al) - mp.log(4)) / mp.log(2)
    return mp.log(q + mp.mpf(p["pc"])) / mp.log(2)


@pytest.mark.parametrize("kind", ["parametric", "mean", "log2"])
def test_specification_against_mpmath(oracle, kind):
    """the expressions as tests/vst_spec.py evaluates them against 50-digit arithmetic, q from 0 to 2^31 (exact q: size
    factors of one), the coefficient ranges of the GPU test; the bound is spec_bound's (derived there)"""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(2)
    q = np.unique(np.concatenate([[0, 1, 2, 3, 2 ** 31 - 1], np.floor(2.0 ** rng.uniform(0, 31, 600))])).astype(np.float64)
    worst = 0.0
    for params in PARAMS[kind]:
        got = vst_spec.transform(oracle, q[None, :], np.ones(q.size), kind, **params)[0]
        ex = [_exact(kind, v, params) for v in q.tolist()]
        err = np.array([float(abs(mp.mpf(g) - e)) for g, e in zip(got.tolist(), ex)])
        exf = np.array([float(e) for e in ex])
        if kind == "mean":
            bound = spec_bound("mean", exf, A=np.arcsinh(np.sqrt(params["alpha"] * q)), la=np.log(params["alpha"]))
        else:
            bound = spec_bound(kind, exf)
        worst = max(worst, float((err / bound).max()))
        print("%s %r: largest error %.3g (%.3g ulps of the result)" % (kind, params, err.max(), (err / np.spacing(np.abs(exf) + 1e-300)).max()))
        assert (err <= bound).all()
    print("%s: largest error / bound = %.3f" % (kind, worst))


def test_asymptote_to_log2(oracle):
    """R/vst.R:65-67: for large q the transformation approaches log2(q).  Expanding the expressions: parametric
    log2(q) + log2(1 + (1 + e) / (2 a q) + ...) with a distance below (1 + e) / (a q ln 2), mean below 1 / (alpha q ln 2).
    At q = 2^30, 2^40, 2^50 the distance shrinks from one to the next and is below that figure -- asserted where the figure
    at 2^50 is well above the rounding of the double-precision evaluation (spec_bound); coefficient pairs whose distance
    has sunk below that rounding by 2^50 are held to figure + spec_bound.  The spline path: measured and printed."""
    from deseq2_amd import core
    qs = np.array([2.0 ** 30, 2.0 ** 40, 2.0 ** 50])
    lg = np.array([30.0, 40.0, 50.0])
    one = np.ones(3)
    for a, e in ((1e-4, 1e-2), (1e-4, 1e3), (1e-2, 1e3), (0.1, 1.0), (10.0, 30.0)):
        r = vst_spec.transform(oracle, qs[None, :], one, "parametric", asymptDisp=a, extraPois=e)[0]
        dist, fig, rnd = np.abs(r - lg), (1 + e) / (a * qs * np.log(2)), spec_bound("parametric", lg)
        print("parametric a=%g e=%g: distance %s, figure %s" % (a, e, dist, fig))
        if fig[2] > 100 * rnd[2]:
            assert dist[0] > dist[1] > dist[2] and (dist < fig).all()
        else:
            assert (dist <= fig + rnd).all() and dist[0] + rnd[0] >= dist[1] - rnd[1]
    for al in (1e-4, 0.07, 10.0):
        r = vst_spec.transform(oracle, qs[None, :], one, "mean", alpha=al)[0]
        dist, fig = np.abs(r - lg), 1 / (al * qs * np.log(2))
        rnd = spec_bound("mean", lg, A=np.arcsinh(np.sqrt(al * qs)), la=np.log(al))
        print("mean alpha=%g: distance %s, figure %s" % (al, dist, fig))
        if fig[2] > 100 * rnd[2]:
            assert dist[0] > dist[1] > dist[2] and (dist < fig).all()
        else:
            assert (dist <= fig + rnd).all()
    # spline: a trend with a closed form, rescaled through h1 = 2^20, h2 = 2^25 as R/vst.R:175-178 does
    from deseq2_amd.engine import spline_eval
    table = core.vst_spline_table(lambda mu: np.full(np.shape(mu), 0.07), 2.0 ** 50, 0.0)
    s1, s2 = (float(spline_eval(table, np.arcsinh(h))) for h in (2.0 ** 20, 2.0 ** 25))
    eta = 5.0 / (s2 - s1)
    r = vst_spec.transform(oracle, qs[None, :], one, "spline", table=table, eta=eta, xi=20.0 - eta * s1)[0]
    print("spline (f = 0.07): distance to log2(q) at 2^30, 2^40, 2^50: %s" % np.abs(r - lg))


# ---------------------------------------------------------------------------------------------------------- the spline table
def test_fmm_spline_properties():
    """splinefun's "fmm" coefficients pinned by what defines them: the pieces meet with equal value, first and second
    derivative at the inner knots; the third derivative of the first / last piece is that of the cubic through the first /
    last four points (third divided difference times 3!); a cubic is reproduced."""
    from deseq2_amd import core
    rng = np.random.default_rng(3)
    x = np.cumsum(rng.uniform(0.05, 1.0, 40))
    y = np.sin(x) + 0.1 * x ** 2
    t = core.fmm_spline(x, y)
    X, Y, B, C_, D = t
    np.testing.assert_array_equal(X, x)
    np.testing.assert_array_equal(Y, y)
    h = np.diff(x)
    scale = np.abs(y).max()
    np.testing.assert_allclose(Y[:-1] + h * (B[:-1] + h * (C_[:-1] + h * D[:-1])), Y[1:], atol=1e-12 * scale, rtol=0)
    np.testing.assert_allclose(B[:-1] + h * (2 * C_[:-1] + 3 * h * D[:-1]), B[1:], atol=1e-10 * scale, rtol=0)
    np.testing.assert_allclose(2 * C_[:-1] + 6 * h * D[:-1], 2 * C_[1:], atol=1e-9 * scale, rtol=0)

    def dd3(xx, yy):
        d1 = np.diff(yy) / np.diff(xx)
        d2 = (d1[1:] - d1[:-1]) / (xx[2:] - xx[:-2])
        return (d2[1] - d2[0]) / (xx[3] - xx[0])
    np.testing.assert_allclose(D[0], dd3(x[:4], y[:4]), rtol=1e-8)
    np.testing.assert_allclose(D[-2], dd3(x[-4:], y[-4:]), rtol=1e-8)
    assert D[-1] == D[-2]
    cub = 0.3 * x ** 3 - x ** 2 + 2 * x - 1
    tc = core.fmm_spline(x, cub)
    xx = np.linspace(x[0] - 1, x[-1] + 1, 500)
    from deseq2_amd.engine import spline_eval
    np.testing.assert_allclose(spline_eval(tc, xx), 0.3 * xx ** 3 - xx ** 2 + 2 * xx - 1, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(spline_eval(tc, xx), vst_spec.spline_eval(tc, xx))
    two = core.fmm_spline([1.0, 3.0], [2.0, 6.0])
    np.testing.assert_array_equal(two[2:], [[2.0, 2.0], [0, 0], [0, 0]])
    with pytest.raises(ValueError):
        core.fmm_spline([1.0, 1.0, 2.0], [0, 1, 2])


def test_spline_path_agrees_with_the_closed_form():
    """f(mu) = alpha has the integral in closed form: int dx / sqrt(alpha x^2 + xim x) = 2 asinh(sqrt(alpha x / xim)) / sqrt(alpha),
    the "mean" formula up to an affine map, which the rescaling through h1, h2 removes.  The reference's construction is
    itself approximate: the cumulative sum up to grid point i + 1 is attached to the knot at the MIDPOINT of interval i
    (R/vst.R:170-174), half a grid step delta / 2 = asinh(max q) / 999 / 2 to the left in u = asinh(q).  The rescaled closed form has
    the slope sqrt(1 + q^2) sqrt(alpha) / (ln 2 sqrt(alpha q^2 + xim q)) <= sqrt(2) / ln 2 in u for q >= 1, so the shift moves the curve by
    at most (sqrt(2) / ln 2) delta / 2 there, and fixing it at the two anchors h1, h2 can add as much again: asserted is
    2 (sqrt(2) / ln 2) delta / 2 for q >= 1 (the trapezoid rule's own error on 999 points is far below it).  The figure seen is printed."""
    from deseq2_amd import core
    from deseq2_amd.engine import spline_eval
    alpha, xim = 0.07, 1.1
    table = core.vst_spline_table(lambda mu: np.full(np.shape(mu), alpha), 1e6, xim)
    assert table.shape == (5, 998) and (np.diff(table[0]) > 0).all()
    h1, h2 = 300.0, 5000.0
    closed = lambda q: 2 * np.arcsinh(np.sqrt(alpha * q / xim)) / np.sqrt(alpha)
    s1, s2 = (float(spline_eval(table, np.arcsinh(h))) for h in (h1, h2))
    eta = (np.log2(h2) - np.log2(h1)) / (s2 - s1)
    xi = np.log2(h1) - eta * s1
    eta_c = (np.log2(h2) - np.log2(h1)) / (closed(h2) - closed(h1))
    xi_c = np.log2(h1) - eta_c * closed(h1)
    q = np.concatenate([[0.0], 2.0 ** np.linspace(-3, np.log2(1e6), 400)])
    got = eta * spline_eval(table, np.arcsinh(q)) + xi
    ref = eta_c * closed(q) + xi_c
    d = np.abs(got - ref)
    print("spline vs closed form: max |difference| %.3g for q >= 1, %.3g for q < 1 (log2 units)" % (d[q >= 1].max(), d[q < 1].max()))
    assert d[q >= 1].max() <= 2 * (np.sqrt(2) / np.log(2)) * np.arcsinh(1e6) / 999 / 2


# ------------------------------------------------------------------------------------------------------------- vst()'s rule
def test_vst_subset_rule_with_ties_and_exact_nsub():
    from deseq2_amd import core
    bm = np.array([7.0, 3.0, 9.0, 7.0, 5.0, 100.0, 7.0, 6.0, 5.0000001, np.nan, 8.0])
    # rows > 5: 0 2 3 5 6 7 8 10; ordered (stable): 8(5.0000001) 7(6) 0(7) 3(7) 6(7) 10(8) 2(9) 5(100)
    order = np.array([8, 7, 0, 3, 6, 10, 2, 5])
    np.testing.assert_array_equal(core.vst_subset_rows(bm, 8), order)                 # exactly nsub qualifying rows: all of them
    np.testing.assert_array_equal(vst_spec.vst_subset(bm, 8), order)
    # nsub = 3: seq(1, 8, length = 3) = 1, 4.5, 8 -> round half even: 1, 4, 8
    np.testing.assert_array_equal(core.vst_subset_rows(bm, 3), order[[0, 3, 7]])
    # nsub = 5: 1, 2.75, 4.5, 6.25, 8 -> 1, 3, 4, 6, 8
    np.testing.assert_array_equal(core.vst_subset_rows(bm, 5), order[[0, 2, 3, 5, 7]])
    # nsub = 2 of L = 4 rows: 1, 4; L = 6, nsub = 3: 1, 3.5 -> 4, 6
    np.testing.assert_array_equal(core.vst_subset_rows(np.array([6.0, 9, 8, 7, 1]), 2), [0, 1])
    np.testing.assert_array_equal(core.vst_subset_rows(np.array([10.0, 11, 12, 13, 14, 15]), 3), [0, 3, 5])
    rng = np.random.default_rng(4)
    big = np.round(rng.gamma(1.0, 20.0, 5000), 1)                                       # many ties
    for nsub in (1, 2, 10, 999, 1000):
        np.testing.assert_array_equal(core.vst_subset_rows(big, nsub), vst_spec.vst_subset(big, nsub))
    with pytest.raises(ValueError, match="less than 'nsub' rows with mean normalized count > 5"):
        core.vst_subset_rows(bm, 9)


def test_vst_stop_conditions_and_host_pipeline(oracle):
    from deseq2_amd import core
    from deseq2_amd.engine import HostEngine
    from tests.helpers import make_case
    E = HostEngine(oracle)
    d = make_case(600, 8, "two_group", seed=3, sf_random=True, drop_all_zero=False)
    dds = core.DESeqDataSet(d["counts"], d["x"], sizeFactors=d["size_factors"], engine=E)
    with pytest.raises(ValueError, match="less than 'nsub' rows,"):
        core.vst(dds, nsub=601)
    with pytest.raises(ValueError, match="less than 'nsub' rows with mean normalized count > 5"):
        core.vst(dds, nsub=600)
    with pytest.raises(ValueError, match="call estimateDispersions before calling getVarianceStabilizedData"):
        core.getVarianceStabilizedData(dds)
    t = core.vst(dds, nsub=200)
    assert dds.dispersionFunction is None and "vst_rows" not in dds.attrs      # the argument is left as it was
    dds = t.dds
    fn = dds.dispersionFunction
    assert fn["fitType"] in ("parametric", "mean")
    rm, _ = vst_spec.row_stats(d["counts"], d["size_factors"])
    np.testing.assert_array_equal(dds.attrs["vst_rows"], vst_spec.vst_subset(E.row_stats(dds.y, None, sizeFactors=d["size_factors"])[0], 200))
    assert np.abs(E.row_stats(dds.y, None, sizeFactors=d["size_factors"])[0] - rm).max() <= 8 * U * rm.max()
    kind = fn["fitType"]
    kw = dict(asymptDisp=fn["coefficients"][0], extraPois=fn["coefficients"][1]) if kind == "parametric" else dict(alpha=fn["coefficients"])
    ref = vst_spec.transform(oracle, d["counts"], d["size_factors"], kind, **kw)
    assert t.assay().shape == d["counts"].shape and np.abs(t.assay() - ref).max() < 1e-12
    # the frozen VST: blind = False with a dispersion function on the object fits nothing
    calls = []

    class Spy(HostEngine):
        def fit_disp(self, *a, **k):
            calls.append("fit_disp")
            return super().fit_disp(*a, **k)
    dds2 = core.DESeqDataSet(d["counts"], d["x"], sizeFactors=d["size_factors"], engine=Spy(oracle))
    dds2.dispersionFunction = dict(fn)
    t2 = core.varianceStabilizingTransformation(dds2, blind=False)
    assert calls == []
    np.testing.assert_array_equal(t2.assay(), t.assay())
    core.varianceStabilizingTransformation(dds2, blind=True)
    assert calls
    # matrix input: the ~ 1 object with estimated size factors; a callable trend takes the spline path
    t3 = core.vst(d["counts"], nsub=200, engine=E, fitType=lambda means, disps: (lambda mu: 0.1 + 1.0 / np.asarray(mu)))
    assert t3.dds.p == 1 and not np.all(t3.dds.sizeFactors == 1.0) and t3.dds.dispersionFunction["fitType"] == "custom"
    assert np.isfinite(t3.assay()).all() and "vst_spline" in t3.dds.attrs
    lg = core.normTransform(dds).assay()
    np.testing.assert_allclose(lg, np.log2(d["counts"] / d["size_factors"][None, :] + 1), rtol=4 * U, atol=4 * U)
    np.testing.assert_array_equal(core.normalized_counts(dds).assay(), d["counts"] / d["size_factors"][None, :])


def test_vst_kinds_and_entries():
    """the specification's kinds in the binding's numbering (the layout of DsqVstArgs / DsqVstOut and the DSQ_VST_* values
    themselves: test_capi_cpu.test_struct_layout_matches_header, test_constants_match_header)"""
    from deseq2_amd import _lib
    assert [_lib.DSQ_VST[k] for k in vst_spec.KINDS if k != "spline"][:2] == [_lib.DSQ_VST["parametric"], _lib.DSQ_VST["mean"]]
    for s in ("dsq_vst", "dsq_vst_dev", "dsq_vst_rowstats_dev"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), s)
