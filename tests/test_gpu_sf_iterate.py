"""The solve of estimateSizeFactors(type = "iterate") on the device (csrc/sf_iterate.hip) against the numpy specification of
tests/sf_iterate_spec.py, BIT FOR BIT (s, sf, F, iter, evals, flag): the device's log / exp / log1p / stirlerr / density
equal the oracle's, the four operations are IEEE, every sum has the order the specification states.  Dispersions are
synthetic, so the kernels are tested apart from the chain: dsq_sf_iterate_dev on the smallest shapes at which they can go
wrong, then the host entry (native.sf_iterate_solve), core.estimateSizeFactors(type = "iterate") on a DeviceEngine against
the same call on HostEngine(oracle), and fused.DESeq(sfType = "iterate")."""
import ctypes as C

import numpy as np
import pytest

from tests import sf_iterate_cases as CS
from tests import sf_iterate_spec as S
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

G = S.G
KEYS = ("s", "sf", "F", "iter", "evals", "flag")


def _dev(c, pad=0, stream=None, short=0, Q=0.05, maxit=100):
    """dsq_sf_iterate_dev through ctypes: counts and mu gene-major with ld = round8(m) + pad, the padding of mu NaN, of the
    counts garbage; outputs prefilled with garbage; a guard region behind the workspace.  Returns the host results and the
    two buffers as they are afterwards."""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    n, m = c["counts"].shape
    ld = ((m + 7) & ~7) + pad
    yb = np.full((n, ld), -123456, np.int32)
    yb[:, :m] = c["counts"]
    mb = np.full((n, ld), np.nan)
    mb[:, :m] = c["mu"]
    yt, mt = torch.as_tensor(yb, device=dev), torch.as_tensor(mb, device=dev)
    sf = torch.as_tensor(np.ascontiguousarray(c["sf"], np.float64), device=dev)
    disp = torch.as_tensor(np.ascontiguousarray(c["disp"], np.float64), device=dev)
    rows = torch.as_tensor(np.ascontiguousarray(c["rows"], np.int32), device=dev)
    s = torch.full((m,), -777.0, dtype=torch.float64, device=dev)
    e = torch.full((m,), -777.0, dtype=torch.float64, device=dev)
    F = torch.full((1,), -777.0, dtype=torch.float64, device=dev)
    ints = torch.full((3,), -5, dtype=torch.int32, device=dev)
    need = int(L.lib().dsq_sf_iterate_workspace_bytes(n, m))
    assert need == 8 * (3 * n + 2 * (-(-n // G)) * m + 7 * m) + 64
    ws = torch.empty(need + 64, dtype=torch.uint8, device=dev)
    ws[need:] = 171
    a = L.DsqSfIterateArgs(n=n, m=m, ld=ld, y=yt.data_ptr(), mu=mt.data_ptr(), sf=sf.data_ptr(), disp=disp.data_ptr(),
                           rows=rows.data_ptr(), Q=Q, maxit=maxit)
    o = L.DsqSfIterateOut(s=s.data_ptr(), sf=e.data_ptr(), F=F.data_ptr(), iter=ints[0:1].data_ptr(), evals=ints[1:2].data_ptr(),
                          flag=ints[2:3].data_ptr())
    st = torch.cuda.current_stream() if stream is None else stream
    torch.cuda.synchronize()
    rc = L.lib().dsq_sf_iterate_dev(C.byref(a), C.byref(o), C.c_void_p(ws.data_ptr()), need - short, C.c_void_p(st.cuda_stream))
    st.synchronize()
    if short:
        return rc
    L.check(rc)
    assert (ws[need:].cpu().numpy() == 171).all()                       # nothing written past the workspace
    ih = ints.cpu().numpy()
    assert_same(yt.cpu().numpy(), yb, "the counts are not written")
    assert_same(mt.cpu().numpy(), mb, "mu is not written")
    return {"s": s.cpu().numpy(), "sf": e.cpu().numpy(), "F": float(F.cpu().numpy()[0]), "iter": int(ih[0]), "evals": int(ih[1]),
            "flag": int(ih[2])}


def _same(got, want, what):
    for key in KEYS:
        assert_same(got[key], want[key], "%s: %s" % (what, key))


@pytest.mark.parametrize("n_rows", [1, 2, 19, 20, 21, G - 1, G, G + 1, 2 * G + 3])
def test_row_counts_around_the_cut_and_the_slice(oracle, n_rows):
    """n' = 1, 2: an empty kept set, a single kept row; 19 | 20 | 21: (n' - 1) Q crosses 1; G - 1 | G | G + 1 | 2 G + 3: the
    slices of the column pass (G = 64: the wave's 63 | 64 | 65 too).  Every case once with all rows taking part and once
    with excluded rows (NaN dispersion, all-zero counts) in between, which moves the slice boundaries."""
    for interleave in (False, True):
        c = CS.solve_case(n_rows=n_rows, m=6, seed=100 + n_rows, interleave=interleave)
        want = S.solve(oracle, **c)
        _same(_dev(c), want, "n' = %d, interleave %r" % (n_rows, interleave))
        if n_rows == 1:
            assert (want["flag"], want["iter"], want["evals"], want["F"]) == (0, 0, 1, 0.0)
        else:
            assert want["flag"] == 0 and want["iter"] >= 1


@pytest.mark.parametrize("m", [5, 63, 64, 65, 129, 257])
def test_sample_counts(oracle, m):
    """63 | 64 | 65 and 129: the 64 lanes of the row pass and the 64-sample tiles of the column pass; 257: one past the 256
    threads of the per-sample kernels (few genes there)"""
    c = CS.solve_case(n_rows=30 if m > 129 else 70, m=m, seed=200 + m, interleave=True)
    want = S.solve(oracle, **c)
    _same(_dev(c), want, "m = %d" % m)
    assert want["flag"] == 0 and want["iter"] >= 1


def test_more_rows_than_one_grid_round(oracle):
    """the row pass is capped at four workgroups (16 waves, one per gene) per CU; the sum of F goes past its 1024 threads.
    Two iterations are enough to run every kernel at this size."""
    import torch
    n_rows = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    c = CS.solve_case(n_rows=n_rows, m=5, seed=300, interleave=True)
    want = S.solve(oracle, maxit=2, **c)
    _same(_dev(c, maxit=2), want, "n' = %d" % n_rows)
    assert want["iter"] == 2


@pytest.mark.parametrize("name,kw", [
    ("pairs of equal rows", dict(n_rows=42, m=6, seed=5, dup=2)),
    ("four equal rows at the cut", dict(n_rows=20, m=6, seed=8, dup=4)),
    ("every row tied", dict(n_rows=4, m=6, seed=8, dup=4)),
    ("dispersion edges", dict(n_rows=131, m=65, seed=3, disp_edges=True, interleave=True)),
    ("no outlier", dict(n_rows=50, m=7, seed=12, outlier=False)),
    ("far start", dict(n_rows=60, m=8, seed=33, far=True)),
    ("far start, many halvings", dict(n_rows=60, m=8, seed=37, far=True)),
])
def test_content(oracle, name, kw):
    """ties that straddle the cut (the strict ">"), dispersions at 1e-8, at 1e-12 (cells outside the closed split of the
    density) and at max(10, m), the 1e6 outlier (every other case has it), starts far from the optimum"""
    c = CS.solve_case(**kw)
    want = S.solve(oracle, **c)
    _same(_dev(c), want, name)
    assert want["flag"] == 0
    if name.startswith("far start"):
        assert want["evals"] > want["iter"] + 1                  # the Armijo test rejected at least once
    if name == "every row tied":
        assert want["iter"] == 0 and want["F"] == 0.0
    if name == "dispersion edges":
        assert (c["disp"][c["rows"] != 0] == 1e-12).any() and (c["disp"][c["rows"] != 0] == 65.0).any()


SEL_DIRECT = 1024        # kSelDirect of csrc/dsq_select.hpp: that many candidates or fewer are ranked by direct counting
SEL_SHIFTS = (53, 42, 31, 20, 9, 0)      # what is left below the digits of 11, 11, 11, 11, 11, 9 bits


def _selection_regime(oracle, c, Q):
    """What the cut's selection meets at the start point, from the specification's L: the number of rows that take part and
    equal the lower order statistic s[lo]; whether rank lo + 1 is one of them; and the candidates left after each radix digit
    (the entries -- a row that does not take part is +inf -- whose key agrees with s[lo]'s above the digit's shift; the L
    are negative, so agreeing bits of the doubles are agreeing bits of the keys)."""
    P = S.Problem(oracle, Q=Q, **c)
    L = P.evaluate(S._exp(oracle, P.start()))[0]
    s = np.sort(L[P.rows])
    h = (s.size - 1) * Q
    lo = int(np.floor(h))
    assert h != lo and lo + 1 < s.size and s[-1] < 0.0            # the upper statistic is needed
    bits = np.where(P.rows, L, np.inf).view(np.uint64)
    want = s[lo:lo + 1].view(np.uint64)[0]
    left = [int(((bits >> np.uint64(sh)) == (want >> np.uint64(sh))).sum()) for sh in SEL_SHIFTS]
    return int((s == s[lo]).sum()), bool(s[lo + 1] == s[lo]), left


@pytest.mark.parametrize("name,kw,Q", [
    ("radix passes, then direct ranking", dict(n_rows=3000, m=5, seed=41), 0.05),
    ("the same with excluded rows", dict(n_rows=3000, m=5, seed=42, interleave=True), 0.05),
    ("exactly 1024 candidates", dict(n_rows=4096, m=5, seed=43, dup=1024), 0.05),
    ("1025 tied candidates", dict(n_rows=4100, m=5, seed=43, dup=1025), 0.05),
    ("the upper statistic tied", dict(n_rows=2200, m=5, seed=44, dup=1100), 0.05),
    ("the upper statistic the smallest above", dict(n_rows=6000, m=5, seed=45, dup=1500), 0.25),
])
def test_the_shared_selection_past_one_pass_and_at_large_ties(oracle, name, kw, Q):
    """sfi_cut_kernel's order statistics come from radix_select / next_order_stat (csrc/dsq_select.hpp): the smallest shapes at
    which those take paths the cases above do not -- a real histogram pass in front of the direct ranking, with and without
    sentinel entries; a tie block of exactly kSelDirect candidates (ranked directly) and of one more (never: every digit
    runs, the result is the prefix); the next order statistic inside a block of more than kSelDirect ties and just above one.
    Each case first proves from the specification that it is in its regime."""
    c = CS.solve_case(**kw)
    if name == "the same with excluded rows":
        assert c["rows"].size == 5000
    ties, next_tied, left = _selection_regime(oracle, c, Q)
    direct = [k for k, v in enumerate(left[:-1]) if v <= SEL_DIRECT]           # (the last digit never hands over)
    if name in ("radix passes, then direct ranking", "the same with excluded rows"):
        assert left[0] > SEL_DIRECT and direct and ties <= 2
    elif name == "exactly 1024 candidates":
        assert ties == 1024 and direct and left[direct[0]] == 1024
    elif name == "1025 tied candidates":
        assert ties == 1025 and not direct
    elif name == "the upper statistic tied":
        assert ties == 1100 and next_tied
    else:
        assert ties == 1500 and not next_tied
    want = S.solve(oracle, maxit=3, Q=Q, **c)
    _same(_dev(c, Q=Q, maxit=3), want, name)


def test_a_second_stream_padding_maxit_and_q(oracle):
    import torch
    c = CS.solve_case(n_rows=97, m=5, seed=400, interleave=True)
    want = S.solve(oracle, **c)
    _same(_dev(c, stream=torch.cuda.Stream()), want, "side stream")
    _same(_dev(c, pad=16), want, "ld = m + padding")
    for maxit in (0, 1):
        w = S.solve(oracle, maxit=maxit, **c)
        _same(_dev(c, maxit=maxit), w, "maxit = %d" % maxit)
        assert w["flag"] == 1 and w["iter"] == maxit
    for Q in (0.0, 0.5):
        _same(_dev(c, Q=Q), S.solve(oracle, Q=Q, **c), "Q = %g" % Q)


def test_a_workspace_one_byte_short_is_refused():
    from deseq2_amd import _lib as L
    c = CS.solve_case(n_rows=65, m=5, seed=401)
    assert _dev(c, short=1) == 1 and "workspace" in L.lib().dsq_last_error().decode()


def test_host_entry(oracle):
    from deseq2_amd import native
    for kw in (dict(n_rows=131, m=65, seed=3, disp_edges=True, interleave=True), dict(n_rows=60, m=8, seed=33, far=True)):
        c = CS.solve_case(**kw)
        _same(native.sf_iterate_solve(c["counts"], c["mu"], c["sf"], c["disp"], c["rows"]), S.solve(oracle, **c), "dsq_sf_iterate %r" % kw)
    bad = dict(c, counts=c["counts"].copy())
    bad["counts"][3, 1] = -1
    with pytest.raises(Exception, match="negative"):
        native.sf_iterate_solve(bad["counts"], bad["mu"], bad["sf"], bad["disp"], bad["rows"])
    sf = c["sf"].copy()
    sf[2] = 0.0
    with pytest.raises(Exception, match="not positive"):
        native.sf_iterate_solve(c["counts"], c["mu"], sf, c["disp"], c["rows"])


def test_core_on_the_device_engine_equals_the_host_engine(oracle):
    """core.estimateSizeFactors(type = "iterate"): every round's dispersions and solve on the device, against the same call
    on HostEngine(oracle): the factors bit for bit, and the number of outer rounds"""
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    cts, true_sf = CS.testthat_case(100)
    cts[7] = 0                                                    # an all-zero row: outside idx
    res = {}
    for label, E in (("host", HostEngine(oracle)), ("device", DeviceEngine())):
        dds = core.estimateSizeFactors(core.DESeqDataSet(cts, np.ones((12, 1)), engine=E), type="iterate")
        res[label] = (dds.sizeFactors, dds.attrs["sfIterateRounds"])
        assert_same(np.asarray(E.to_numpy(dds.nf)), np.broadcast_to(dds.sizeFactors[None, :], cts.shape), label + ": nf")
    assert res["host"][1] == res["device"][1] == 4
    assert_same(res["device"][0], res["host"][0], "sizeFactors")
    slope, icpt = np.polyfit(true_sf, res["device"][0], 1)
    assert abs(icpt) < .1 and abs(slope - 1) < .1


def test_fused_deseq_with_sftype_iterate():
    from deseq2_amd import core, fused, simulate
    from deseq2_amd.engine import DeviceEngine
    x = simulate.design_two_group(8)
    k = simulate.make_counts(200, x, seed=41)["counts"]
    E = DeviceEngine()
    one = fused.DESeq(core.DESeqDataSet(k, x, engine=E), sfType="iterate")
    two = fused.DESeq(core.estimateSizeFactors(core.DESeqDataSet(k, x, engine=E), type="iterate"))
    assert_same(one.sizeFactors, two.sizeFactors, "sizeFactors")
    assert not np.array_equal(one.sizeFactors, np.ones(8))
    for key in ("dispersion", "dispMAP", "baseMean"):
        assert_same(one.mcols[key], two.mcols[key], key)
