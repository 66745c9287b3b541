"""The case table of the stream-order tests (tests/stream_cases.py) held to the conditions that let
tests/test_gpu_stream_order.py FAIL -- on the oracle and the specifications alone, no device:

  * the decoy of every device input has the shape and dtype of the true input;
  * every array that carries indices, counts or lengths is in range and every value in its domain, in both builds: a kernel
    that runs too early computes a wrong finite answer from a valid input and never forms an address from garbage;
  * the reference's outputs on the decoy differ from its outputs on the true input in EVERY output array the GPU test compares
    (the host tables and scalars being the true call's): a stale read of the whole input set cannot go unseen in any of them.
"""
import numpy as np
import pytest

from tests import stream_cases as SC
from tests.stream_hold import BASE_MS, MARGIN

ALL = SC.CASES + list(SC.SECOND.values())


def _in_domain(a, dom, what):
    a = np.asarray(a)
    if dom is None:
        return
    if dom == "count":
        assert np.isfinite(a.astype(np.float64)).all() and (a >= 0).all() and (a == np.floor(a)).all() and (a <= 2 ** 31 - 1).all(), what
    elif dom == "pos":
        assert np.isfinite(a).all() and (a > 0).all(), what
    elif dom == "nonneg":
        assert np.isfinite(a).all() and (a >= 0).all(), what
    elif dom == "weight":
        assert np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all() and (a.max(axis=1) > 0).all(), what
    elif dom == "prob":
        assert np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all(), what
    elif dom == "flag":
        assert a.dtype.kind in "iu" and set(np.unique(a)) <= {0, 1}, what
    elif isinstance(dom, tuple) and dom[0] == "index":
        assert a.dtype.kind in "iu" and (a >= 0).all() and (a < dom[1]).all(), what
    elif isinstance(dom, tuple) and dom[0] == "offsets":
        assert a.dtype.kind in "iu" and a[0] == 0 and a[-1] == dom[1] and (np.diff(a) >= 0).all(), what
    else:
        raise AssertionError("%s: unknown domain %r" % (what, dom))


def _differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return True
    same = (a == b) | (np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)))
    return not bool(same.all())


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_decoy_is_a_valid_input_and_every_output_sees_it(oracle, case):
    t, u = case.data(0)["in"], case.data(1)["in"]
    assert list(t) == list(u)
    for k in t:
        what = "%s: input %s" % (case.name, k)
        assert t[k].a.shape == u[k].a.shape and t[k].a.dtype == u[k].a.dtype and t[k].m == u[k].m, what
        assert t[k].dom == u[k].dom, what
        for which, v in (("true", t[k]), ("decoy", u[k])):
            _in_domain(v.logical(), v.dom, "%s (%s) is outside its domain %r" % (what, which, v.dom))
            if v.m is not None:
                assert (v.a[:, v.m:] == 0).all(), what + ": padding columns"
        if t[k].dom != "flag":            # (a short vector of flags may well be the same under both seeds)
            assert _differs(t[k].a, u[k].a), what + ": the decoy equals the true input"
    want, stale = case.expected(oracle, 0), case.expected(oracle, 1)
    assert sorted(want) == sorted(stale) and want
    assert set(case.constant) <= set(want)
    for k in want:
        if k in case.constant:            # a status word: 0 on every valid input, by definition
            assert not _differs(want[k], stale[k]) and not np.asarray(want[k]).any(), "%s: %s is no constant" % (case.name, k)
            continue
        assert _differs(want[k], stale[k]), "%s: output %s is the same on the decoy: a stale read would go unseen" % (case.name, k)


def test_the_chain_decoy(oracle):
    """dsq_deseq_dev: counts, size factors and design of the decoy are valid, of the true shapes, and move every compared column"""
    (c0, x0, s0), (c1, x1, s1) = SC.chain_inputs(0), SC.chain_inputs(1)
    assert c0.shape == c1.shape and c0.dtype == c1.dtype and x0.shape == x1.shape and s0.shape == s1.shape
    for c, x, s in ((c0, x0, s0), (c1, x1, s1)):
        _in_domain(c, "count", "chain counts")
        _in_domain(s, "pos", "chain size factors")
        assert np.linalg.matrix_rank(x) == x.shape[1]
    # the same design cells under both codings (the host tables of the call are the true design's)
    from deseq2_amd import native
    a, b = native.cell_index(x0), native.cell_index(x1)
    assert len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))
    want, stale = SC.chain_reference(oracle, c0, x0, s0), SC.chain_reference(oracle, c1, x1, s1)
    assert sorted(want) == sorted(stale)
    for k in want:
        if k in SC.CHAIN_CONSTANT:       # NA in every row once outliers were replaced and refitted: no input moves it
            assert np.isnan(want[k]).all() and np.isnan(stale[k]).all(), k
            continue
        assert _differs(want[k], stale[k]), "chain: column %s is the same on the decoy" % k


def test_the_exempt_set_is_exactly_the_stated_synchronisers():
    used = sorted({c.exempt for c in SC.CASES if c.exempt})
    assert used == sorted(SC.EXEMPT) == ["beta_prior_var", "f64_counts", "sf_iterate"]
    assert not any(c.exempt for c in SC.SECOND.values())
    # the header grants each: its block of the entry says so
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "deseq2_mi355x.h")).read()
    flat = " ".join(hdr.replace("\n *", " ").split())
    for entry, words in SC.EXEMPT.values():
        assert words in flat, "%s: the header does not say %r" % (entry, words)


def test_every_listed_entry_has_a_case():
    entries = " ".join(c.entry for c in SC.CASES)
    for e in ("dsq_fit_beta_dev", "dsq_fit_disp_dev", "dsq_fit_disp_grid_dev", "dsq_prefit_moments_dev", "dsq_linear_mu_dev",
              "dsq_nbinom_loglike_dev", "dsq_intercept_fit_dev", "dsq_parametric_dispersion_fit_dev", "dsq_cooks_distance_dev",
              "dsq_replace_outliers_dev", "dsq_weights_prep_dev", "dsq_xim_dev", "dsq_to_gene_major_f64", "dsq_from_gene_major_f64",
              "dsq_counts_f64_to_gene_major_i32", "dsq_size_factors_dev", "dsq_vst_dev", "dsq_vst_rowstats_dev", "dsq_rlog_dev",
              "dsq_unmix_dev", "dsq_apeglm_dev", "dsq_top_var_dev", "dsq_sample_pairs_dev", "dsq_collapse_dev", "dsq_col_sums_dev",
              "dsq_fpm_dev", "dsq_local_fit_dev", "dsq_results_dev", "dsq_contrasts_dev", "dsq_pt_dev", "dsq_sf_iterate_dev",
              "dsq_beta_prior_var_dev"):
        assert e in entries, e
    assert sum(c.entry == "dsq_fit_beta_dev" for c in SC.CASES) == 4 and sum(c.entry == "dsq_fit_disp_dev" for c in SC.CASES) == 3
    assert sum(c.entry == "dsq_vst_dev" for c in SC.CASES) == 2


def test_the_hold_margin():
    assert MARGIN >= 20.0 and BASE_MS >= 100.0
