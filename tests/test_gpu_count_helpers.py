"""collapseReplicates, colSums, fpm and fpkm on the device (csrc/count_helpers.hip) against the numpy specification of
tests/counts_spec.py, BIT FOR BIT: dsq_collapse_dev / dsq_col_sums_dev / dsq_fpm_dev through ctypes on the smallest shapes
at which the kernels can go wrong (inputs padded to ld = m + 3 with garbage in the padding, outputs prefilled, one spare
element behind them checked untouched, the input checked unchanged), the robust avgTxLength route end to end, the host
entries, and core.collapseReplicates / fpm / fpkm / counts / plotCounts on a DeviceEngine against the same calls on
HostEngine, on an object made by from_device."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests import counts_spec as S
from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu

PAD = 3
GARBAGE = -123456789          # what the padding of an int32 input holds: a read past m shows in every sum
FILL = -777
I32MAX = 2 ** 31 - 1
M_LIST = [1, 2, 63, 64, 65, 129]


def _cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _round_items():
    """items of one grid round of collapse_kernel and fpm_kernel: 8 workgroups of 256 threads per CU (launch_collapse,
    launch_fpm_kind, csrc/count_helpers.hip)"""
    return 8 * _cu() * 256


def _counts(n, m, seed, hi=200000):
    rng = np.random.Generator(np.random.PCG64(seed))
    y = rng.integers(0, hi, size=(n, m), dtype=np.int32)
    y[rng.random((n, m)) < 0.2] = 0
    return y


def _resident_i32(y, pad=PAD):
    import torch
    n, m = y.shape
    buf = np.full((n, m + pad), GARBAGE, dtype=np.int32)
    buf[:, :m] = y
    return torch.as_tensor(buf, device="cuda:0"), m + pad


def _resident_f64(A, pad=PAD):
    import torch
    n, m = A.shape
    buf = np.full((n, m + pad), np.nan)
    buf[:, :m] = A
    return torch.as_tensor(buf, device="cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream()


def _collapse_dev(y, members, offsets, pad=PAD):
    """dsq_collapse_dev through ctypes: (out n x g, status)"""
    import torch
    from deseq2_amd import _lib as L
    n, m = y.shape
    g = len(offsets) - 1
    yt, ld = _resident_i32(y, pad)
    mt = torch.as_tensor(np.ascontiguousarray(members, np.int32), device="cuda:0")
    ot = torch.as_tensor(np.ascontiguousarray(offsets, np.int32), device="cuda:0")
    ldo = g + pad
    out = torch.full((n * ldo + 1,), FILL, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    status[1] = FILL
    a = L.sized(L.DsqCollapseArgs, n=n, m=m, g=g, ld=ld, y=yt.data_ptr(), members=mt.data_ptr(), offsets=ot.data_ptr())
    o = L.sized(L.DsqCollapseOut, ld=ldo, out=out.data_ptr(), status=status.data_ptr())
    st = _stream()
    L.check(L.lib().dsq_collapse_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    h, s = out.cpu().numpy(), status.cpu().numpy()
    assert h[n * ldo] == FILL and s[1] == FILL                          # nothing written past the outputs
    h = h[:n * ldo].reshape(n, ldo)
    assert (h[:, g:] == FILL).all()                                     # the padding of the output is not written
    assert np.array_equal(yt.cpu().numpy()[:, :m], y)                   # the input is left alone
    return h[:, :g].copy(), int(s[0])


def _col_sums_dev(y, pad=PAD):
    import torch
    from deseq2_amd import _lib as L
    n, m = y.shape
    yt, ld = _resident_i32(y, pad)
    sums = torch.full((m + 1,), FILL, dtype=torch.int64, device="cuda:0")
    a = L.sized(L.DsqColSumsArgs, n=n, m=m, ld=ld, y=yt.data_ptr())
    o = L.sized(L.DsqColSumsOut, sums=sums.data_ptr())
    st = _stream()
    L.check(L.lib().dsq_col_sums_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    h = sums.cpu().numpy()
    assert h[m] == FILL
    assert np.array_equal(yt.cpu().numpy()[:, :m], y)
    return h[:m].copy()


def _fpm_dev(y, lib, kind, basepairs=None, txlen=None, pad=PAD):
    import torch
    from deseq2_amd import _lib as L
    n, m = y.shape
    yt, ld = _resident_i32(y, pad)
    lt = torch.as_tensor(np.ascontiguousarray(lib, np.float64), device="cuda:0")
    bt = None if basepairs is None else torch.as_tensor(np.ascontiguousarray(basepairs, np.float64), device="cuda:0")
    tt = None if txlen is None else _resident_f64(txlen, pad)
    out = torch.full((n * ld + 1,), float(FILL), dtype=torch.float64, device="cuda:0")
    a = L.sized(L.DsqFpmArgs, n=n, m=m, ld=ld, y=yt.data_ptr(), kind=L.DSQ_FPM[kind], lib=lt.data_ptr(),
                basepairs=None if bt is None else bt.data_ptr(), txlen=None if tt is None else tt.data_ptr())
    o = L.sized(L.DsqFpmOut, out=out.data_ptr())
    st = _stream()
    L.check(L.lib().dsq_fpm_dev(C.byref(a), C.byref(o), C.c_void_p(st.cuda_stream)))
    st.synchronize()
    h = out.cpu().numpy()
    assert h[n * ld] == FILL
    h = h[:n * ld].reshape(n, ld)
    assert (h[:, m:] == FILL).all()
    assert np.array_equal(yt.cpu().numpy()[:, :m], y)
    return h[:, :m].copy()


# ---------------------------------------------------------------------------------------------- collapse
def _groups(m, which):
    """(members, offsets): "one" g = 1; "identity" g = m; "mixed" interleaved groups of sizes 1, 2 and 5 (repeating, the
    last group takes what is left), the samples dealt to the groups round robin so that no group is contiguous"""
    if which == "one":
        return np.arange(m), np.array([0, m])
    if which == "identity":
        return np.arange(m), np.arange(m + 1)
    sizes, left = [], m
    while left > 0:
        s = min((1, 2, 5)[len(sizes) % 3], left)
        sizes.append(s)
        left -= s
    g = len(sizes)
    code, room, c = np.empty(m, np.int64), list(sizes), 0
    for j in range(m):
        while room[c % g] == 0:
            c += 1
        code[j] = c % g
        room[c % g] -= 1
        c += 1
    members = np.argsort(code, kind="stable")
    return members, np.concatenate([[0], np.cumsum(sizes)])


def _n_list(g):
    return [1, 67, _round_items() // g + 1]


@pytest.mark.parametrize("which", ["one", "identity", "mixed"])
@pytest.mark.parametrize("m", M_LIST)
def test_collapse(m, which):
    members, offsets = _groups(m, which)
    g = len(offsets) - 1
    for n in _n_list(g):
        assert n == 1 or n == 67 or n * g > _round_items()
        y = _counts(n, m, seed=1000 * m + n % 997, hi=I32MAX // m)
        y[0, 0] = 0
        y[n - 1, m - 1] = I32MAX // m
        if which == "identity":
            y[n // 2, m // 2] = I32MAX
        got, status = _collapse_dev(y, members, offsets)
        want, wstatus = S.collapse(y, members, offsets)
        assert wstatus == 0 and status == 0
        assert np.array_equal(got, want), "m = %d, %s, n = %d" % (m, which, n)


def test_collapse_overflow_status():
    """the status word: set by exactly one element summing to 2^31, not set at 2^31 - 1"""
    members, offsets = _groups(7, "mixed")
    y = _counts(67, 7, seed=5, hi=1000)
    grp = members[offsets[1]:offsets[2]]
    assert grp.size == 2
    y[40, grp] = [I32MAX - 5, 5]
    got, status = _collapse_dev(y, members, offsets)
    want, wstatus = S.collapse(y, members, offsets)
    assert (status, wstatus) == (0, 0) and np.array_equal(got, want) and got[40, 1] == I32MAX
    y[40, grp] = [I32MAX - 5, 6]
    got, status = _collapse_dev(y, members, offsets)
    want, wstatus = S.collapse(y, members, offsets)
    assert (status, wstatus) == (1, 1)
    keep = np.ones(got.shape, bool)
    keep[40, 1] = False
    assert np.array_equal(got[keep], want[keep])                        # every other element is still its sum


def test_collapse_members_outside_the_matrix_are_not_read():
    """dsq_collapse_dev cannot look at resident indices before the launch: a member outside [0, m) is not read and an offset
    outside [0, m] is clipped; either sets bit 2 of the status (the host entry refuses such a pair)"""
    y = _counts(5, 4, seed=6)
    got, status = _collapse_dev(y, [0, 4, -1, 3], [0, 2, 4])
    assert status == 2
    assert np.array_equal(got, np.stack([y[:, 0], y[:, 3]], axis=1))
    got, status = _collapse_dev(y, [0, 1, 2, 3], [-3, 2, 9])
    assert status == 2
    assert np.array_equal(got, np.stack([y[:, 0] + y[:, 1], y[:, 2] + y[:, 3]], axis=1))


# ---------------------------------------------------------------------------------------------- col_sums
@pytest.mark.parametrize("m", M_LIST)
def test_col_sums(m):
    for n in (1, 67, _round_items() // m + 1):
        y = _counts(n, m, seed=2000 * m + n % 997, hi=I32MAX)
        y[0, 0] = 0
        y[n - 1, m - 1] = I32MAX
        assert np.array_equal(_col_sums_dev(y), S.col_sums(y)), "m = %d, n = %d" % (m, n)


def test_col_sums_of_one_sample_past_a_round_of_workgroups():
    """m = 1: 256 genes per step of a workgroup, every slice 16 steps: one gene more than 8 workgroups per CU hold"""
    n = 8 * _cu() * 16 * 256 + 1
    y = _counts(n, 1, seed=3, hi=I32MAX)
    assert np.array_equal(_col_sums_dev(y), S.col_sums(y))


def test_col_sums_above_2_to_the_53():
    """n = 2^22 + 3 genes of 2^31 - 1: the sum is odd and above 2^53, so the int64 has to be exact and the host double is its
    single rounding (to nearest even), which differs from it"""
    n = 2 ** 22 + 3
    y = np.full((n, 1), I32MAX, dtype=np.int32)
    got = _col_sums_dev(y, pad=1)
    exact = n * I32MAX
    assert exact % 2 == 1 and exact > 2 ** 53
    assert int(got[0]) == exact
    from fractions import Fraction
    d = S.as_double(got)[0]
    assert d == float(Fraction(exact)) and int(d) != exact


# ---------------------------------------------------------------------------------------------- fpm / fpkm
def _fpm_inputs(n, m, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    y = _counts(n, m, seed)
    lib = rng.uniform(1e5, 5e7, size=m)
    bp = rng.integers(1, 20000, size=n).astype(np.float64)
    tl = rng.uniform(50.0, 9000.0, size=(n, m))
    return y, lib, bp, tl


def _fpm_all_kinds(y, lib, bp, tl, what, pad=PAD):
    with np.errstate(all="ignore"):
        assert_bits(_fpm_dev(y, lib, "fpm", pad=pad), S.fpm(y, lib, "fpm"), what + ": fpm")
        assert_bits(_fpm_dev(y, lib, "fpkm_basepairs", basepairs=bp, pad=pad), S.fpm(y, lib, "fpkm_basepairs", basepairs=bp),
                    what + ": fpkm_basepairs")
        assert_bits(_fpm_dev(y, lib, "fpkm_txlen", txlen=tl, pad=pad), S.fpm(y, lib, "fpkm_txlen", txlen=tl),
                    what + ": fpkm_txlen")


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
def test_fpm_kinds(m, pad):
    """pad 3: ld = m + 3; pad 4: ld = m + 4 -- between them every m runs both the paired (even ld) and the single walk"""
    per_thread = 2 if (m + pad) % 2 == 0 and m >= 2 else 1
    inner = (m + 1) // 2 if per_thread == 2 else m
    for n in (1, 67, _round_items() // inner + 1):
        y, lib, bp, tl = _fpm_inputs(n, m, seed=3000 * m + n % 997)
        _fpm_all_kinds(y, lib, bp, tl, "m = %d, ld = %d, n = %d" % (m, m + pad, n), pad=pad)


@pytest.mark.parametrize("pad", [3, 4])
def test_fpm_edge_values(pad):
    """a zero library size (0/0 NaN, k/0 Inf), a NaN size factor, basepairs 0, an L entry 0; counts 0 and 2^31 - 1"""
    y, lib, bp, tl = _fpm_inputs(67, 6, seed=9)
    y[:, 1] = _counts(67, 1, seed=10)[:, 0]
    y[3, 1], y[4, 1], y[5, 2], y[6, 2] = 0, 7, 0, I32MAX
    lib[1], lib[4] = 0.0, np.nan
    bp[5], bp[8] = 0.0, 0.0
    tl[6, 2], tl[9, 0], tl[3, 1] = 0.0, 0.0, 0.0
    y[9, 0] = 0
    _fpm_all_kinds(y, lib, bp, tl, "edges, ld = %d" % (6 + pad), pad=pad)
    with np.errstate(all="ignore"):
        f = _fpm_dev(y, lib, "fpm", pad=pad)
    assert np.isnan(f[3, 1]) and np.isposinf(f[4, 1]) and np.isnan(f[:, 4]).all()


def test_fpkm_txlen_robust_route():
    """fpkm(robust = TRUE) with avgTxLength, end to end on resident data: dsq_fpm_dev (DSQ_FPKM_TXLEN over the plain column
    sums), dsq_size_factors_dev on the float64 result, the division by the DSQ_VST_NORMALIZED launch -- against the
    specification composed with sf_spec"""
    from deseq2_amd.engine import DeviceEngine
    from oracle import oracle as O
    D = DeviceEngine("cuda:0")
    y, _, _, tl = _fpm_inputs(300, 7, seed=11)
    y = y + 1
    yh, th = D.counts(y), D.matrix(tl)
    sums = D.col_sums(yh)
    assert np.array_equal(sums, S.col_sums(y))
    ex = D.fpm_transform(yh, S.as_double(sums), "fpkm_txlen", txlen=th)
    sf = D.size_factors(ex, type="ratio")["sizeFactors"]
    got = D.to_numpy(D.vst_transform(ex, None, "normalized", sizeFactors=sf))
    want, wsf = S.fpkm_txlen_robust(O, y, tl)
    assert_bits(sf, wsf, "size factors of the fpkm matrix")
    assert_bits(got, want, "fpkm, robust, avgTxLength")


# ---------------------------------------------------------------------------------------------- host entries
def test_host_entries():
    """dsq_collapse / dsq_col_sums / dsq_fpm: host pointers in R layout, staged through the library's own buffers"""
    from deseq2_amd import _lib as L
    from deseq2_amd import native
    y, lib, bp, tl = _fpm_inputs(150, 67, seed=21)
    members, offsets = _groups(67, "mixed")
    got = native.collapse(y, members, offsets)
    assert got.dtype == np.int32 and np.array_equal(got, S.collapse(y, members, offsets)[0])
    assert np.array_equal(native.col_sums(y), S.col_sums(y))
    for kind, kw in (("fpm", {}), ("fpkm_basepairs", {"basepairs": bp}), ("fpkm_txlen", {"txlen": tl})):
        assert_bits(native.fpm(y, lib, kind, **kw), S.fpm(y, lib, kind, **kw), kind)
    big = y.copy()
    big[7, members[offsets[1]:offsets[2]]] = [I32MAX, 1]
    with pytest.raises(L.DsqError) as e:
        native.collapse(big, members, offsets)
    assert e.value.code == L.DSQ_ERR_VALUE
    for bad_members, bad_offsets in (([0, 1, 1], [0, 1, 3]), ([0, 1, 3], [0, 1, 3]), ([1, 0, 2], [0, 2, 3]), ([0, 1, 2], [0, 1, 2]),
                                     ([0, 1, 2], [0, 0, 3])):
        with pytest.raises(L.DsqError) as e:
            native.collapse(y[:, :3], bad_members, bad_offsets)
        assert e.value.code == L.DSQ_ERR_ARG


# ---------------------------------------------------------------------------------------------- the engine and core
def _objects(counts, x, sizeFactors=None, txlen=None, basepairs=None, factors=None):
    """the same data as an object made by from_device on a DeviceEngine and as a host-engine object"""
    import torch
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    D, H = DeviceEngine("cuda:0"), HostEngine()
    n, m = counts.shape
    sf = np.ones(m) if sizeFactors is None else sizeFactors
    cr = torch.as_tensor(np.ascontiguousarray(counts.T.astype(np.int32)), device="cuda:0")
    nr = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(sf[:, None], (m, n))), device="cuda:0")
    dev = core.DESeqDataSet.from_device(D, cr, nr, x, sizeFactors=sf)
    dev._sf_given = sizeFactors is not None
    host = core.DESeqDataSet(counts, x, sizeFactors=sizeFactors, engine=H)
    for o in (dev, host):
        if txlen is not None:
            o.assays["avgTxLength"] = o.engine.matrix(txlen)
        if basepairs is not None:
            o.mcols["basepairs"] = basepairs
        if factors is not None:
            o.attrs["factors"] = dict(factors)
    return dev, host


def _example(m=12, n=400, seed=5):
    from deseq2_amd import simulate
    x = simulate.design_factor(m, 2)
    d = simulate.make_counts(n, x, seed=seed, beta_sd=np.array([2.0, 1.0]))
    return d["counts"], x, d["size_factors"]


def test_collapse_replicates_on_the_device_engine():
    from deseq2_amd import core
    counts, x, sf = _example()
    groupby = ["s%d" % v for v in (3, 1, 1, 2, 9, 4, 4, 5, 3, 6, 7, 8)]
    run = ["run%d" % (j + 1) for j in range(12)]
    factors = {"condition": np.arange(12) % 2}
    dev, host = _objects(counts, x, sizeFactors=sf, factors=factors)
    cd, ch = (core.collapseReplicates(o, groupby, run) for o in (dev, host))
    assert cd.m == ch.m == 9 and cd.attrs["colnames"] == ch.attrs["colnames"] == sorted(set(groupby))
    assert cd.attrs["runsCollapsed"] == ch.attrs["runsCollapsed"] and cd.attrs["runsCollapsed"][0] == "run2,run3"
    got = cd.engine.to_numpy(cd.y)
    assert np.array_equal(got, np.asarray(ch.y))
    lv = cd.attrs["colnames"]
    for c, name in enumerate(lv):
        cols = [j for j in range(12) if groupby[j] == name]
        assert np.array_equal(got[:, c], counts[:, cols].sum(axis=1))
    assert_bits(cd.sizeFactors, ch.sizeFactors, "size factors of the kept columns")
    assert np.array_equal(cd.attrs["factors"]["condition"], ch.attrs["factors"]["condition"])
    # ... and the collapsed object goes on through the workflow where it is
    for o in (cd, ch):
        core.estimateSizeFactors(o)
    from oracle import oracle as O
    from tests import sf_spec
    assert_bits(cd.sizeFactors, sf_spec.size_factors(O, got, type="ratio")["sizeFactors"], "estimateSizeFactors on the collapsed object")
    np.testing.assert_allclose(cd.sizeFactors, ch.sizeFactors, rtol=1e-12)      # (HostEngine.size_factors: libm, equal to rounding)


def test_collapse_replicates_overflow_names_the_level():
    from deseq2_amd import core
    counts = np.full((5, 4), 10, dtype=np.int64)
    counts[2, 1], counts[2, 3] = I32MAX, 1
    x = np.ones((4, 1))
    groupby = ["a", "b", "a", "b"]
    for o in _objects(counts, x):
        with pytest.raises(ValueError, match="level 'b' exceeds the largest integer"):
            core.collapseReplicates(o, groupby)
    counts[2, 3] = 0
    dev, host = _objects(counts, x)
    assert int(dev.engine.to_numpy(core.collapseReplicates(dev, groupby).y)[2, 1]) == I32MAX


def test_fpm_fpkm_counts_plotcounts_on_the_device_engine():
    from deseq2_amd import core
    from oracle import oracle as O
    counts, x, sf = _example()
    rng = np.random.Generator(np.random.PCG64(12))
    bp = rng.integers(200, 9000, size=counts.shape[0]).astype(np.float64)
    factors = {"condition": np.arange(12) % 2, "batch": np.arange(12) % 3}
    dev, host = _objects(counts, x, sizeFactors=sf, basepairs=bp, factors=factors)
    sums = S.col_sums(counts)
    for robust in (True, False):
        lib = S.library_sizes(O, sf, sums) if robust else S.as_double(sums)
        fd, fh = (core.fpm(o, robust=robust) for o in (dev, host))
        assert fd.kind == "fpm" and not isinstance(fd.handle, np.ndarray)              # the result stays resident
        assert_bits(fd.assay(), S.fpm(counts, lib, "fpm"), "fpm against the specification, robust = %s" % robust)
        assert_bits(fd.assay(), fh.assay(), "fpm: device vs host engine")
        kd, kh = (core.fpkm(o, robust=robust) for o in (dev, host))
        assert_bits(kd.assay(), S.fpm(counts, lib, "fpkm_basepairs", basepairs=bp), "fpkm against the specification")
        assert_bits(kd.assay(), kh.assay(), "fpkm: device vs host engine")
    assert_bits(core.sampleDists(core.fpm(dev)), core.sampleDists(core.fpm(host)), "the transform feeds sampleDists")
    # no size factors: estimated on a copy, the caller's object unchanged
    dev0, host0 = _objects(counts, x, basepairs=bp)
    f0 = core.fpm(dev0)
    assert not dev0._sf_given and np.array_equal(dev0.sizeFactors, np.ones(12))
    from tests import sf_spec
    est = sf_spec.size_factors(O, counts, type="ratio")["sizeFactors"]
    assert_bits(f0.assay(), S.fpm(counts, S.library_sizes(O, est, sums), "fpm"), "fpm with estimated size factors")
    # avgTxLength takes precedence
    tl = rng.uniform(100.0, 5000.0, size=counts.shape)
    devt, hostt = _objects(counts + 1, x, sizeFactors=sf, txlen=tl, basepairs=bp)
    want, _ = S.fpkm_txlen_robust(O, counts + 1, tl)
    assert_bits(core.fpkm(devt).assay(), want, "fpkm, robust, avgTxLength")
    np.testing.assert_allclose(core.fpkm(hostt).assay(), want, rtol=1e-12)              # (HostEngine.size_factors: libm)
    plain = S.fpm(counts + 1, S.as_double(S.col_sums(counts + 1)), "fpkm_txlen", txlen=tl)
    for o in (devt, hostt):
        assert_bits(core.fpkm(o, robust=False).assay(), plain, "fpkm, robust = FALSE, avgTxLength")
    # counts() and plotCounts()
    assert np.array_equal(core.counts(dev).assay(), counts)
    with np.errstate(all="ignore"):
        assert_bits(core.counts(dev, normalized=True).assay(), counts / sf[None, :], "counts(normalized = TRUE)")
    with pytest.warns(UserWarning, match="there are no assays named 'replaceCounts'"):
        assert np.array_equal(core.counts(dev, replaced=True).assay(), counts)
    with pytest.raises(ValueError, match="first calculate size factors"):
        core.counts(dev0, normalized=True)
    for gene in (0, 17, counts.shape[0] - 1):
        pd, ph = (core.plotCounts(o, gene, intgroup=["condition", "batch"]) for o in (dev, host))
        assert list(pd) == list(ph) == ["count", "condition", "batch"]
        assert_bits(pd["count"], counts[gene] / sf + 0.5, "plotCounts$count")
        assert_bits(pd["count"], ph["count"], "plotCounts: device vs host engine")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert_bits(core.plotCounts(dev, 3, normalized=False, transform=False)["count"], counts[3].astype(float), "raw row")
