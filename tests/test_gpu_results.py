"""results() on the device (csrc/results.hip) against the numpy specification of tests/results_spec.py, BIT FOR BIT: dexp
equals the oracle's exp, the threshold tests run the specification's operations in its order, and the Benjamini-Hochberg
adjustment over all thresholds from one sort is exact integer counting and minima."""
import ctypes as C

import numpy as np
import pytest

from tests import results_spec as S
from tests.helpers import assert_same, make_case

pytestmark = pytest.mark.gpu

COLS = ("baseMean", "log2FoldChange", "lfcSE", "stat", "pvalue")


def _dev(beta, betaSE, stat, pvalue, baseMean, c=0, replace=None, na_mask=None, test="Wald", T=0.0, alt="greaterAbs",
         filter=None, theta=None, alpha=0.1, padj_in_workspace=False):
    """dsq_results_dev through ctypes on poisoned output buffers; returns the host copies"""
    import torch
    from deseq2_amd import _lib as L
    dev = torch.device("cuda:0")
    beta, betaSE = np.asarray(beta, np.float64), np.asarray(betaSE, np.float64)
    n, p = beta.shape
    K = 1 if theta is None else len(theta)
    up = lambda a, dt=np.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dt).T), device=dev)
    ins = dict(beta=up(beta), betaSE=up(betaSE), stat=up(stat), pvalue=up(pvalue), baseMean=up(baseMean),
               replace=up(replace, np.int32), na_mask=up(na_mask, np.int32), filter=up(filter), theta=up(theta))
    table = torch.full((5, n), -7.0, dtype=torch.float64, device=dev)
    fp = torch.full((K, n), -3.0, dtype=torch.float64, device=dev)
    nr = torch.full((K,), -9, dtype=torch.int32, device=dev)
    cut = torch.full((K,), -5.0, dtype=torch.float64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    wsb = int(L.lib().dsq_results_workspace_bytes(n, K if padj_in_workspace else 0))
    ws = torch.full((wsb,), 0xAB, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = L.DsqResultsArgs(n=n, p=p, c=c, test=L.DSQ_TEST[test], lfcThreshold=T, altHypothesis=L.DSQ_ALT[alt],
                         independentFiltering=int(theta is not None), K=K, alpha=alpha, workspace=ptr(ws), workspace_bytes=wsb,
                         **{k: ptr(v) for k, v in ins.items()})
    o = L.DsqResultsOut(baseMean=ptr(table[0]), log2FoldChange=ptr(table[1]), lfcSE=ptr(table[2]), stat=ptr(table[3]),
                        pvalue=ptr(table[4]), filtPadj=None if padj_in_workspace else ptr(fp), numRej=ptr(nr), cutoffs=ptr(cut),
                        status=ptr(st))
    L.check(L.lib().dsq_results_dev(C.byref(a), C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    if padj_in_workspace:
        off = int(L.lib().dsq_results_workspace_bytes(n, 0))
        fp = ws[off:off + 8 * n * K].view(torch.float64).reshape(K, n)
    out = {k: table[i].cpu().numpy() for i, k in enumerate(COLS)}
    out.update(filtPadj=fp.cpu().numpy().T, numRej=nr.cpu().numpy(), cutoffs=cut.cpu().numpy(), status=int(st.cpu()[0]))
    return out


def _compare(got, ref, what):
    assert got["status"] == 0, what
    for k in COLS + ("filtPadj", "cutoffs", "numRej"):
        assert_same(got[k], ref[k], "%s %s" % (what, k))


FAMILIES = ["random_na", "ties", "all_na", "all_equal", "zero_one", "filter_zeros", "filter_equal", "filter_negative", "masks"]


def _family(n, family, seed):
    """columns of a p = 3 Wald analysis (column 1 is read) with the p-values / filter of the family"""
    rng = np.random.default_rng(seed)
    p = 3
    beta = rng.normal(0, 2, (n, p))
    se = np.exp(rng.normal(-1, 0.5, (n, p)))
    stat = beta / se
    pv = rng.uniform(size=(n, p)) ** 3
    bm = np.exp(rng.normal(4, 2, n))
    kw = {}
    if family == "random_na":
        pv[rng.uniform(size=n) < 0.1, 1] = np.nan
    elif family == "ties":
        pv[:, 1] = np.round(pv[:, 1], 2)
    elif family == "all_na":
        pv[:, 1] = np.nan
    elif family == "all_equal":
        pv[:, 1] = 0.03
    elif family == "zero_one":
        pv[::3, 1] = 0.0
        pv[1::4, 1] = 1.0
    elif family == "filter_zeros":
        bm[rng.uniform(size=n) < 0.3] = 0.0
    elif family == "filter_equal":
        kw["filter"] = np.full(n, 2.5)
    elif family == "filter_negative":
        kw["filter"] = rng.normal(0, 3, n)
    elif family == "masks":
        kw["na_mask"] = (rng.uniform(size=n) < 0.15).astype(np.int32)
        rep = (rng.uniform(size=n) < 0.3).astype(np.int32)
        rep[::7] = -1                                   # NA in `replace`: not TRUE
        bm[rng.uniform(size=n) < 0.3] = 0.0
        kw["replace"] = rep
    return (beta, se, stat, pv, bm), kw


def _theta(K, f):
    if K == 1:
        return None
    lo = float(np.mean(f == 0))
    return np.linspace(lo, 0.95 if lo < 0.95 else 1.0, K)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1025, 5000])
def test_results_dev_equals_spec(oracle, n, family):
    cols, kw = _family(n, family, seed=n * 13 + len(family))
    f = kw.get("filter", cols[4])
    for K in (1, 2, 50):
        theta = _theta(K, f)
        ref = S.results(oracle, cols[0][:, 1], cols[1][:, 1], cols[2][:, 1], cols[3][:, 1], cols[4],
                        replace=None if "replace" not in kw else kw["replace"] == 1, theta=theta, **{k: v for k, v in kw.items() if k != "replace"})
        got = _dev(*cols, c=1, theta=theta, padj_in_workspace=(K == 2), **kw)
        _compare(got, ref, "%s n=%d K=%d" % (family, n, K))


@pytest.mark.parametrize("alt,T", [("greaterAbs", 0.5), ("lessAbs", 0.5), ("greater", 0.5), ("less", 0.5), ("greaterAbs2014", 0.5),
                                   ("greaterAbs", 0.0)])
def test_threshold_tests_equal_spec(oracle, alt, T):
    n = 1500
    (beta, se, stat, pv, bm), _ = _family(n, "random_na", seed=77)
    lfc, s = beta[:, 2], se[:, 2]
    lfc[:60] = np.random.default_rng(1).normal(0, 0.05, 60)           # the central range of pnorm
    s[100:110] = 0.0                                                  # SE = 0
    lfc[105] = 0.0
    s[110:115] = np.nan                                               # SE NA
    lfc[115:118] = np.nan
    lfc[120:130] = np.array([40, -40, 60, -60, 400, -400, 39, -39, 1e6, -1e6]) * s[120:130]   # |LFC / SE| > 38
    with np.errstate(all="ignore"):
        stat[:, 2] = lfc / s
    theta = _theta(50, bm)
    ref = S.results(oracle, lfc, s, stat[:, 2], pv[:, 2], bm, lfcThreshold=T, altHypothesis=alt, theta=theta)
    got = _dev(beta, se, stat, pv, bm, c=2, T=T, alt=alt, theta=theta)
    _compare(got, ref, "%s T=%g" % (alt, T))
    if T > 0:
        assert not np.array_equal(got["pvalue"], pv[:, 2], equal_nan=True)


def test_lrt_columns(oracle):
    n = 700
    (beta, se, _, _, bm), _ = _family(n, "random_na", seed=5)
    rng = np.random.default_rng(6)
    stat, pv = rng.chisquare(1, n), rng.uniform(size=n)
    pv[::9] = np.nan
    theta = _theta(50, bm)
    _compare(_dev(beta, se, stat, pv, bm, c=1, test="LRT", theta=theta), S.results(oracle, beta[:, 1], se[:, 1], stat, pv, bm, theta=theta), "LRT")


def test_host_entry_equals_dev(oracle):
    from deseq2_amd import native
    for n, K in ((1, 1), (65, 2), (3000, 50)):
        cols, kw = _family(n, "masks", seed=n)
        theta = _theta(K, cols[4])
        d = _dev(*cols, c=1, theta=theta, T=0.5, alt="greater", **kw)
        h = native.results(*cols, coef=1, theta=theta, lfcThreshold=0.5, altHypothesis="greater", **kw)
        for k in COLS + ("filtPadj", "cutoffs", "numRej"):
            assert_same(h[k], d[k], "host entry n=%d %s" % (n, k))


def _analysis(E, test):
    from deseq2_amd import core
    d = make_case(600, 14, "two_group", seed=31)
    k = d["counts"].copy()
    k[3] = [90000] + [12] * 13
    k[5] = [70000] + [0] * 13
    k[9, 8] = 50000
    kw = {"reduced": np.ones((14, 1))} if test == "LRT" else {}
    a = core.DESeq(core.DESeqDataSet(k, d["x"], engine=E), test=test, **kw)
    b = core.DESeq(core.DESeqDataSet(k, d["x"], engine=E), test=test, minReplicatesForReplace=np.inf, **kw)
    return a, b


@pytest.mark.parametrize("test", ["Wald", "LRT"])
def test_core_results_device_equals_host(oracle, test):
    """core.results after a DESeq on each engine: replaced rows (one of them all zero afterwards) and Cook's outliers"""
    from deseq2_amd import core
    from deseq2_amd.engine import DeviceEngine, HostEngine
    dev, host = _analysis(DeviceEngine(), test), _analysis(HostEngine(oracle), test)
    assert (np.asarray(host[0].mcols["replace"]) == 1).sum() >= 2 and core.cooksOutlier(host[1]).any()
    calls = [dict(), dict(independentFiltering=False), dict(alpha=0.05, theta=np.linspace(0.1, 0.9, 7)), dict(cooksCutoff=False)]
    if test == "Wald":
        calls += [dict(lfcThreshold=0.5), dict(lfcThreshold=1.0, altHypothesis="lessAbs"), dict(name=0, altHypothesis="greater")]
    for dd, hh in zip(dev, host):
        for kw in calls:
            rd, rh = core.results(dd, **kw), core.results(hh, **kw)
            for c in core.DESeqResults.COLUMNS:
                assert_same(rd[c], rh[c], "%s %r %s" % (test, kw, c))
            assert set(rd.metadata) == set(rh.metadata)
            if "filterNumRej" in rh.metadata:
                assert_same(rd.metadata["filterNumRej"]["numRej"], rh.metadata["filterNumRej"]["numRej"], "numRej")
                assert rd.metadata["filterThreshold"] == rh.metadata["filterThreshold"]
                assert rd.metadata["filterTheta"] == rh.metadata["filterTheta"]


def _block(n=8, K=2):
    """a valid host argument block of dsq_results (arrays kept alive by the caller)"""
    from deseq2_amd import _lib as L
    keep = dict(beta=np.zeros((n, 2), order="F"), se=np.ones((n, 2), order="F"), stat=np.zeros((n, 2), order="F"),
                pv=np.full((n, 2), 0.5, order="F"), bm=np.arange(1.0, n + 1), theta=np.linspace(0, 0.9, K),
                out=[np.zeros(n) for _ in range(5)], fp=np.zeros((n, K), order="F"), nr=np.zeros(K, np.int32), cut=np.zeros(K),
                st=np.zeros(1, np.int32))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    a = L.DsqResultsArgs(n=n, p=2, c=1, test=0, beta=ptr(keep["beta"]), betaSE=ptr(keep["se"]), stat=ptr(keep["stat"]),
                         pvalue=ptr(keep["pv"]), baseMean=ptr(keep["bm"]), lfcThreshold=0.0, altHypothesis=0, independentFiltering=1,
                         theta=ptr(keep["theta"]), K=K, alpha=0.1)
    o = L.DsqResultsOut(baseMean=ptr(keep["out"][0]), log2FoldChange=ptr(keep["out"][1]), lfcSE=ptr(keep["out"][2]),
                        stat=ptr(keep["out"][3]), pvalue=ptr(keep["out"][4]), filtPadj=ptr(keep["fp"]), numRej=ptr(keep["nr"]),
                        cutoffs=ptr(keep["cut"]), status=ptr(keep["st"]))
    return a, o, keep


ERRORS = [
    ("n", 0, "at least one gene"), ("c", 2, "outside 0 .. p - 1"), ("c", -1, "outside 0 .. p - 1"), ("alpha", 0.0, "must lie in (0, 1)"),
    ("alpha", 1.0, "must lie in (0, 1)"), ("lfcThreshold", -0.5, "must be >= 0"), ("altHypothesis", 1, "lessAbs needs a positive"),
    ("test+T", None, "must be Wald tests"), ("nan_filter", None, "is NaN"), ("K", 1, "thresholds: 2"), ("K", 5000, "thresholds: 2"),
    ("K_nofilter", None, "takes K = 1"), ("beta", None, "NULL beta"), ("theta", None, "NULL theta"), ("numRej", None, "NULL output"),
]


@pytest.mark.parametrize("field,value,text", ERRORS)
def test_argument_errors(field, value, text):
    from deseq2_amd import _lib as L
    a, o, keep = _block()
    if field == "test+T":
        a.test, a.lfcThreshold = 1, 1.0
    elif field == "nan_filter":
        keep["bm"][3] = np.nan
    elif field == "K_nofilter":
        a.independentFiltering = 0
    elif field == "numRej":
        o.numRej = None
    else:
        setattr(a, field, value)
    assert L.lib().dsq_results(C.byref(a), C.byref(o)) == 1                          # DSQ_ERR_ARG
    assert text in L.lib().dsq_last_error().decode()
    assert L.lib().dsq_results(None, C.byref(o)) == 1 and "NULL args" in L.lib().dsq_last_error().decode()


def test_dev_status_and_workspace():
    """what the device entry cannot see without reading device memory comes back in status; a short workspace is refused"""
    import torch
    from deseq2_amd import _lib as L
    (beta, se, stat, pv, bm), _ = _family(100, "random_na", seed=3)
    f = bm.copy()
    f[7] = np.nan
    assert _dev(beta, se, stat, pv, bm, c=1, filter=f, theta=np.linspace(0, 0.9, 5))["status"] & 1
    assert _dev(beta, se, stat, pv, bm, c=1, theta=np.array([0.1, 1.5, 0.3]))["status"] & 2
    a, o, keep = _block()
    a.workspace, a.workspace_bytes = C.c_void_p(torch.zeros(8, device="cuda:0").data_ptr()), 64
    assert L.lib().dsq_results_dev(C.byref(a), C.byref(o), None) == 1 and "workspace" in L.lib().dsq_last_error().decode()
