"""The arithmetic specification of collapseReplicates, colSums, fpm and fpkm on the count matrix
stated in numpy, one operation per line: the reference for the count-helper tests.  Not a test itself.  Integer sums are
exact (int64); /, * are IEEE double, every operation rounded once, in R's order.  log / exp are the oracle's
(oracle.unary, bit-equal to the device's dlog / dexp).  Shares no code with the product (deseq2_amd.engine,
csrc/count_helpers.hip).

What is restated, and from where:
  collapse        sapply(sp, function(i) rowSums(assay(object)[, i, drop = FALSE])); mode(.) <- "integer"   R/helper.R:200-202
                  sp = split(seq(along = groupby), groupby) as a CSR pair (members, offsets), 0-based.  A sum that is no
                  int32 (R: NA) sets status 1; that element is unspecified (here: the low 32 bits).
  col_sums        colSums(counts) before its conversion to double: int64, exact                            R/helper.R:386,388
  library_sizes   sizeFactors * exp(mean(log(colSums(k))))                                                 R/helper.R:386
                  colSums as double is ONE rounding of the exact sum (to nearest even); the mean is the sequential sum in
                  sample order from 0.0, divided by m (R's mean() over m numbers; core.xim_size_factors states its mean
                  the same way).
  fpm             "fpm"             1e6 * (k / lib)                                                        R/helper.R:390
                  "fpkm_basepairs"  1e3 * ((1e6 * (k / lib)) / basepairs)                                  R/helper.R:322
                  "fpkm_txlen"      (1e3 * (1e6 * (k / lib))) / L                                          R/helper.R:294
  fpkm_txlen_robust   estimateSizeFactorsForMatrix(exprs); t(t(exprs) / sf)                                R/helper.R:296-297"""
import numpy as np

INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31


def collapse(y, members, offsets):
    """(out n x g int32, status)"""
    y = np.asarray(y, dtype=np.int64)
    n, m = y.shape
    g = len(offsets) - 1
    out = np.zeros((n, g), dtype=np.int64)
    for c in range(g):
        for k in range(offsets[c], offsets[c + 1]):
            out[:, c] = out[:, c] + y[:, members[k]]
    status = 1 if ((out > INT32_MAX) | (out < INT32_MIN)).any() else 0
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32), status


def col_sums(y):
    y = np.asarray(y, dtype=np.int64)
    s = np.zeros(y.shape[1], dtype=np.int64)
    for i0 in range(0, y.shape[0], 1 << 20):
        s = s + y[i0:i0 + (1 << 20)].sum(axis=0, dtype=np.int64)
    return s


def as_double(sums):
    """the int64 sums as R holds them: one rounding to nearest even (numpy's int64 -> float64 conversion is that rounding)"""
    return np.asarray(sums, dtype=np.int64).astype(np.float64)


def library_sizes(O, sizeFactors, sums):
    from tests.sf_spec import _exp, _log
    cs = as_double(sums)
    lg = _log(O, cs)
    s = 0.0
    with np.errstate(all="ignore"):
        for j in range(cs.size):
            s = s + lg[j]
        mean = s / cs.size
        return np.asarray(sizeFactors, np.float64) * _exp(O, np.array([mean]))[0]


def fpm(y, lib, kind="fpm", basepairs=None, txlen=None):
    k = np.asarray(y).astype(np.float64)
    lib = np.asarray(lib, np.float64)
    with np.errstate(all="ignore"):
        q = k / lib[None, :]
        f = 1e6 * q
        if kind == "fpm":
            return f
        if kind == "fpkm_basepairs":
            r = f / np.asarray(basepairs, np.float64)[:, None]
            return 1e3 * r
        if kind == "fpkm_txlen":
            t = 1e3 * f
            return t / np.asarray(txlen, np.float64)
    raise ValueError(kind)


def fpkm_txlen_robust(O, y, txlen):
    """fpkm(robust = TRUE) with avgTxLength: the library sizes are the plain column sums (R/helper.R:385-389: robust
    normalization is not used when average transcript lengths are present), then the median-ratio factors of the result"""
    from tests import sf_spec
    ex = fpm(y, as_double(col_sums(y)), "fpkm_txlen", txlen=txlen)
    sf = sf_spec.size_factors(O, ex, type="ratio")["sizeFactors"]
    with np.errstate(all="ignore"):
        return ex / sf[None, :], sf
