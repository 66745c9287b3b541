"""CPU: the argument checks of dsq_contrasts / dsq_contrasts_dev (include/deseq2_mi355x.h), in the manner of
tests/test_capi_cpu.py: every check is decided from the argument block before a device is asked for, so the codes hold with
and without a GPU (1 = DSQ_ERR_ARG, 2 = DSQ_ERR_UNSUPPORTED)."""
import ctypes

import numpy as np
import pytest

P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _blocks(n=3, m=6, p=2, K=2):
    """a valid pair of argument blocks over host arrays (kept alive in `keep`)"""
    from deseq2_amd import _lib
    keep = dict(x=np.asfortranarray(np.column_stack([np.ones(m), np.arange(m) % 2.0])[:, :p]), nf=np.ones((n, m), order="F"),
                alpha=np.full(n, 0.1), beta=np.zeros((n, p), order="F"), lam=np.full(p, 1e-6), w=np.ones((n, m), order="F"),
                c=np.asfortranarray(np.ones((p, K))), y=np.ones((n, m), dtype=np.int32, order="F"),
                mask=np.ones((K, m), dtype=np.int32), rule=np.ones(K, dtype=np.int32),
                out=[np.zeros((n, K), order="F") for _ in range(4)], flags=np.zeros((n, K), dtype=np.int32, order="F"))
    a = _lib.DsqContrastsArgs(n=n, m=m, p=p, K=K, ld=m, x=P(keep["x"]), nf=P(keep["nf"]), nf_is_vector=0, alpha_hat=P(keep["alpha"]),
                              beta=P(keep["beta"]), lambda_=P(keep["lam"]), weights=None, useWeights=0, minmu=0.5,
                              contrasts=P(keep["c"]), allZero=None, counts=P(keep["y"]), sample_mask=P(keep["mask"]),
                              rule_applies=P(keep["rule"]), cell_of=None, ncell=0)
    o = _lib.DsqContrastsOut(log2FoldChange=P(keep["out"][0]), lfcSE=P(keep["out"][1]), stat=P(keep["out"][2]),
                             pvalue=P(keep["out"][3]), contrastAllZero=P(keep["flags"]))
    return a, o, keep


_CASES = [
    # (name, field block, field, value, code, message)
    ("K < 1", "a", "K", 0, 1, "at least one contrast"),
    ("n < 0", "a", "n", -1, 1, "bad dimensions"),
    ("m < 1", "a", "m", 0, 1, "bad dimensions"),
    ("p < 1", "a", "p", 0, 1, "bad dimensions"),
    ("p > 64", "a", "p", 65, 2, "design columns"),
    ("NULL x", "a", "x", None, 1, "NULL input"),
    ("NULL nf", "a", "nf", None, 1, "NULL input"),
    ("NULL alpha_hat", "a", "alpha_hat", None, 1, "NULL input"),
    ("NULL beta", "a", "beta", None, 1, "NULL input"),
    ("NULL lambda", "a", "lambda_", None, 1, "NULL input"),
    ("weights", "a", "useWeights", 1, 1, "weights is NULL"),
    ("masks without counts", "a", "counts", None, 1, "without counts"),
    ("masks without rule_applies", "a", "rule_applies", None, 1, "without rule_applies"),
    ("NULL log2FoldChange", "o", "log2FoldChange", None, 1, "NULL output"),
    ("NULL lfcSE", "o", "lfcSE", None, 1, "NULL output"),
    ("NULL stat", "o", "stat", None, 1, "NULL output"),
    ("NULL pvalue", "o", "pvalue", None, 1, "NULL output"),
    ("masks without flags", "o", "contrastAllZero", None, 1, "contrastAllZero is NULL"),
]


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
@pytest.mark.parametrize("entry", ["dsq_contrasts", "dsq_contrasts_dev"])
def test_argument_errors(entry, case):
    from deseq2_amd import _lib
    L = _lib.lib()
    _, blk, field, value, code, msg = case
    a, o, keep = _blocks()
    setattr(a if blk == "a" else o, field, value)
    call = (lambda: L.dsq_contrasts(ctypes.byref(a), ctypes.byref(o))) if entry == "dsq_contrasts" else (
        lambda: L.dsq_contrasts_dev(ctypes.byref(a), ctypes.byref(o), None))
    assert call() == code
    assert msg in L.dsq_last_error().decode()


@pytest.mark.parametrize("entry", ["dsq_contrasts", "dsq_contrasts_dev"])
def test_null_blocks_and_neither_mode(entry):
    from deseq2_amd import _lib
    L = _lib.lib()
    a, o, keep = _blocks()
    fn = getattr(L, entry)
    tail = () if entry == "dsq_contrasts" else (None,)
    assert fn(None, ctypes.byref(o), *tail) == 1 and fn(ctypes.byref(a), None, *tail) == 1
    a.contrasts, a.sample_mask = None, None
    assert fn(ctypes.byref(a), ctypes.byref(o), *tail) == 1
    assert "neither contrasts nor sample_mask" in L.dsq_last_error().decode()


def test_device_entry_checks_ld():
    from deseq2_amd import _lib
    L = _lib.lib()
    a, o, keep = _blocks()
    a.ld = a.m - 1
    assert L.dsq_contrasts_dev(ctypes.byref(a), ctypes.byref(o), None) == 1
    assert "ld" in L.dsq_last_error().decode()


def test_flags_only_mode_needs_no_table_outputs():
    """contrasts == NULL with masks: the four table outputs may be NULL -- whatever comes back is not an argument error"""
    import torch
    from deseq2_amd import _lib
    L = _lib.lib()
    a, o, keep = _blocks()
    a.contrasts = None
    a.x = a.nf = a.alpha_hat = a.beta = a.lambda_ = None
    o.log2FoldChange = o.lfcSE = o.stat = o.pvalue = None
    rc = L.dsq_contrasts(ctypes.byref(a), ctypes.byref(o))
    assert rc == (0 if torch.cuda.is_available() else 3)


def test_max_m_follows_the_lds():
    """the longest row of the per-sample path: what is left of a CU's 160 KiB next to three p x p matrices, falling with p"""
    from deseq2_amd import _lib
    L = _lib.lib()
    assert L.dsq_contrasts_max_m(0) == 0 and L.dsq_contrasts_max_m(65) == 0
    v = [L.dsq_contrasts_max_m(p) for p in (1, 16, 32, 64)]
    assert v == sorted(v, reverse=True) and v[-1] >= 1024
    for p, got in zip((1, 16, 32, 64), v):
        assert 8 * (3 * p * p + got) <= 160 * 1024 < 8 * (3 * p * p + got) + 8 * (4 * p + 300)
