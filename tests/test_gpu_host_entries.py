"""-m gpu: the host-pointer entry points (csrc/capi_host.hip) as staging code: what goes up into which workspace slot at
which offset, what comes down from where.  Every host entry against its `_dev` twin on device copies of the same arrays
(R layout on both sides, same flags), the `_rows` entries over uneven ranges, `nf_is_vector`, NULL optional outputs, the
padded optim width, and the two failures that are reported after the stream has been synchronised.  Bit for bit.

n = 203 (more than 64, no multiple of 2, 3 or 7: uneven ranges), m = 70 (past the 64 lanes and the 64-wide transpose tile,
ld = 72 != m) and m = 40 (ld = m), the batch + condition design: the smallest shapes at which a wrong offset, `lo` or ld / m mix-up shows."""
import ctypes as C

import numpy as np
import pytest

from deseq2_amd import _lib as L
from tests import capi_blocks as cb
from tests.helpers import assert_same, make_case

pytestmark = pytest.mark.gpu

N = 203
_CASES = {}


def case(m, n=N, design="batch_condition"):
    """make_case cut to exactly n genes (it drops all-zero rows), with weights and random size factors; built once"""
    key = (m, n, design)
    if key not in _CASES:
        d = make_case(n + 60, m, design, seed=m, weights=True, sf_random=True)
        n0 = d["counts"].shape[0]
        assert n0 >= n
        _CASES[key] = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (n0,) else v) for k, v in d.items()}
    return _CASES[key]


def same_outputs(got, want, what, keys=None):
    for k in (keys if keys is not None else want):
        assert_same(got[k], want[k], "%s$%s" % (what, k))


@pytest.mark.parametrize("float_counts", [False, True], ids=["int32", "float64"])
@pytest.mark.parametrize("m", [40, 70])
def test_host_entry_equals_dev_twin(oracle, m, float_counts):
    """the twelve host entries that have a `_dev` twin, the twin run on device copies in R layout with the same flags
    (weights on); dsq_optim_rows and dsq_test_math have no twin: against the oracle"""
    d = case(m)
    B = cb.blocks(d, float_counts=float_counts, weights=True)
    for key, b in B.items():
        if not b.dev:
            continue
        same_outputs(cb.run_host(b), cb.run_twin(b), "%s (m=%d)" % (b.name, m))
    # the trend fit takes plain vectors
    import torch
    rng = np.random.default_rng(m)
    means = np.exp(rng.uniform(0, 8, N))
    disps = (0.05 + 3.0 / means) * np.exp(rng.normal(0, 0.3, N))
    coefs, st = np.zeros(2), np.zeros(1, np.int32)
    L.check(L.lib().dsq_parametric_dispersion_fit(cb.ptr(means), cb.ptr(disps), N, cb.ptr(coefs), cb.ptr(st)))
    tm, td = torch.from_numpy(means).cuda(), torch.from_numpy(disps).cuda()
    tc, ts = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L.check(L.lib().dsq_parametric_dispersion_fit_dev(C.c_void_p(tm.data_ptr()), C.c_void_p(td.data_ptr()), N,
                                                      C.c_void_p(tc.data_ptr()), C.c_void_p(ts.data_ptr()), None))
    torch.cuda.synchronize()
    assert_same(coefs, tc.cpu().numpy(), "dsq_parametric_dispersion_fit$coefs")
    assert st[0] == int(ts.cpu()[0]) == 0
    o = B["optim_rows"]
    got = cb.run_host(o)
    want = oracle.optimRows(d["counts"], d["x"], d["nf"], d["alpha_init"], o.inputs["lambda_"], d["weights"], True,
                            o.inputs["beta_start"], 0.5)
    for k, kw in (("beta", "beta"), ("betaSE", "betaSE"), ("conv", "conv"), ("mu", "mu"), ("logLike", "logLike")):
        assert_same(np.asarray(got[k], float), np.asarray(want[kw], float), "dsq_optim_rows$" + k)
    if not float_counts:
        from deseq2_amd import native
        xs = rng.poisson(30.0, N).astype(float)
        size, mu = rng.uniform(0.5, 50, N), rng.uniform(1.0, 60, N)
        assert_same(native.test_math(8, xs, size, mu), oracle.dnbinom_mu_log(xs, size, mu), "dsq_test_math(8)")


RANGES = [(0, 64), (64, 1), (65, N - 65)]


@pytest.mark.parametrize("shards", [None, "3"])
@pytest.mark.parametrize("m", [40, 70])
def test_row_ranges_equal_the_whole_call(monkeypatch, m, shards):
    """dsq_fit_disp_rows, dsq_fit_disp_grid_rows and dsq_fit_beta_rows (weights, mu asked for) over (0, 64), (64, 1),
    (65, n - 65), with the library's own split of a range off and forced to 3: the same bits as one call over [0, n)"""
    monkeypatch.delenv("DSQ_HOST_SHARDS", raising=False)
    B = cb.blocks(case(m), weights=True)
    whole = {k: cb.run_host(B[k]) for k in ("fit_beta", "fit_disp", "fit_disp_grid")}
    if shards:
        monkeypatch.setenv("DSQ_HOST_SHARDS", shards)
    for k, want in whole.items():
        same_outputs(cb.run_host(B[k], rows=RANGES), want, "%s_rows (m=%d, shards %s)" % (B[k].name, m, shards))


@pytest.mark.parametrize("m", [40, 70])
def test_size_factor_vector_through_the_host_entries(m):
    """nf_is_vector = 1 (no Python caller sets it): the m size factors give what the n x m matrix of them gives"""
    d = case(m)
    B = cb.blocks(d, weights=True)
    sf = np.ascontiguousarray(d["nf"][0])
    assert (d["nf"] == sf[None, :]).all()
    for key in ("fit_beta", "prefit_moments", "linear_mu", "intercept_fit", "optim_rows", "cooks_distance",
                "replace_outliers", "vst"):
        b = B[key]
        same_outputs(cb.run_host(b.but(nf=sf, nf_is_vector=1)), cb.run_host(b), "%s with nf_is_vector (m=%d)" % (b.name, m))


@pytest.mark.parametrize("m", [40, 70])
def test_optional_outputs_left_null(m):
    """hat_diagonals / mu (fitBeta, intercept), robustDisp, loggeomeans, vst with the matrix only and with the row statistics
    only: what is still asked for equals the all-outputs call"""
    B = cb.blocks(case(m), weights=True)
    for key, drops in (("fit_beta", (["hat_diagonals"], ["mu"], ["hat_diagonals", "mu"])),
                       ("intercept_fit", (["hat"], ["mu"], ["hat", "mu"])),
                       ("cooks_distance", (["robustDisp"],)),
                       ("size_factors", (["loggeomeans"],)),
                       ("vst", (["rowMean", "rowMax"], ["out"]))):
        full = cb.run_host(B[key])
        for drop in drops:
            got = cb.run_host(B[key].but(drop_out=drop))
            assert not set(drop) & set(got)
            same_outputs(got, full, "%s without %s (m=%d)" % (B[key].name, "+".join(drop), m), keys=list(got))


def test_optim_rows_at_the_padded_width(oracle):
    """p = 11 runs at the padded width 16 (the memset of the packed inputs, beta / betaSE read back at stride n x 16):
    tests/test_gpu_wide.py's construction at n = 37, m = 40, against the oracle at the true p"""
    from deseq2_amd import native
    levels, m, n = 11, 40, 37
    d = case(m, n=n, design=("factor", levels))
    y = d["counts"].copy()
    y[3] = 0; y[3, 5:9] = 1000                      # rows the IRLS cannot fit
    y[11] = 0; y[11, -1] = 7
    y[20, : m // 2] = 0
    lam = np.full(levels, 1e-6)
    lam[-1] = 0.5
    start = np.random.default_rng(3).normal(0, 1.0, (n, levels))
    args = (y, d["x"], d["nf"], d["alpha_init"], lam, d["weights"], True, start, 0.5)
    got, want = native.optimRows(*args), oracle.optimRows(*args)
    for k in ("beta", "betaSE", "conv", "mu", "logLike"):
        assert_same(np.asarray(got[k], float), np.asarray(want[k], float), "optimRows p=11$" + k)
    assert want["conv"].mean() > 0.8


def test_failures_reported_after_the_synchronisation():
    """a float64 count matrix with one 0.5 in the last gene: DSQ_ERR_VALUE from dsq_nbinom_loglike and dsq_vst; a zero in
    every gene: DSQ_ERR_FIT from dsq_size_factors.  Ordinary error returns, and the library serves the next call"""
    d = case(70)
    bad = d["counts"].astype(np.float64)
    bad[-1, -1] = 0.5
    B = cb.blocks(dict(d, counts=bad), float_counts=True)
    for key in ("nbinom_loglike", "vst"):
        assert cb.run_host(B[key], check=False) == L.DSQ_ERR_VALUE, key
        assert b"non-integer" in L.lib().dsq_last_error()
    z = d["counts"].copy()
    z[np.arange(N), np.arange(N) % 70] = 0
    S = cb.blocks(dict(d, counts=z))["size_factors"]
    assert cb.run_host(S, check=False) == L.DSQ_ERR_FIT
    assert b"zero" in L.lib().dsq_last_error()
    good = cb.blocks(d)["nbinom_loglike"]
    same_outputs(cb.run_host(good), cb.run_twin(good), "dsq_nbinom_loglike after the failures")
