"""The numpy statement of ONE contrast table, written from the R text (R/results.R:760-827 getContrast,
:1021-1037 the tail of cleanContrast, :1237-1270 contrastAllZero*) and from the oracle's fitBeta(maxit = 0), its
pnorm_upper2 and tests/results_spec.results.  Nothing of deseq2_amd.core or deseq2_amd.engine is used: this is what
resultsContrasts and csrc/contrasts.hip are held to, bit for bit."""
import numpy as np

from tests import results_spec

LOG2E = float.fromhex("0x1.71547652b82fep+0")        # R's log2(exp(1))
LN2 = float.fromhex("0x1.62e42fefa39efp-1")          # R's log(2)


def mask_numeric(x, c):
    """contrastAllZeroNumeric (:1262-1267): None when all coefficients share a sign (the rule does not apply), else the
    samples with modelMatrix %*% ifelse(contrast == 0, 0, 1) != 0"""
    c = np.asarray(c, np.float64)
    if (c >= 0).all() or (c <= 0).all():
        return None
    return (np.asarray(x, np.float64) @ np.where(c == 0, 0.0, 1.0)) != 0


def mask_character(codes, num, den):
    """contrastAllZeroCharacter (:1240-1241): the samples of the two levels"""
    return np.isin(np.asarray(codes), [num, den])


def all_zero(counts, mask, allZero):
    """rowSums(cts.sub == 0) == ncol(cts.sub) / counts %*% whichSamples == 0, and not a row that is all zero (:1023)"""
    if mask is None:
        return np.zeros(np.shape(counts)[0], bool)
    return ~(np.asarray(counts)[:, np.asarray(mask, bool)] != 0).any(axis=1) & ~np.asarray(allZero, bool)


def get_contrast(O, x, nf, dispersion, beta_log2, betaPriorVar, c, allZero, weights=None, minmu=0.5, counts=None):
    """getContrast (:760-827): the four columns of the numeric contrast c, NA on the all-zero rows.  `weights`: as they sit in
    the assay (normalised by the row maximum here, :791).  counts: any counts -- at maxit = 0 fitBeta reads none."""
    x = np.asarray(x, np.float64)
    n, m = np.shape(nf)
    nz = ~np.asarray(allZero, bool)                                              # :770
    beta_mat = LN2 * np.asarray(beta_log2, np.float64)[nz]                        # :775
    lam = 1.0 / (LN2 ** 2 * np.asarray(betaPriorVar, np.float64))                 # :777
    y = np.zeros((int(nz.sum()), m)) if counts is None else np.asarray(counts, np.float64)[nz]
    if weights is not None:
        w = np.asarray(weights, np.float64)
        w = (w / w.max(axis=1, keepdims=True))[nz]                                # :791
    else:
        w = np.ones((int(nz.sum()), m))                                           # :794
    r = O.fitBeta(y, x, np.asarray(nf, np.float64)[nz], np.asarray(dispersion, np.float64)[nz], np.asarray(c, np.float64),
                  beta_mat, lam, w, weights is not None, 1e-8, 0, False, minmu)   # :797-807
    est = LOG2E * r["contrast_num"].reshape(-1)                                   # :809
    se = LOG2E * r["contrast_denom"].reshape(-1)                                  # :810
    with np.errstate(divide="ignore", invalid="ignore"):
        stat = est / se                                                           # :811
    pv = O.unary("pnorm_upper2", stat)                                            # :817
    out = {}
    for k, v in (("log2FoldChange", est), ("lfcSE", se), ("stat", stat), ("pvalue", pv)):
        full = np.full(n, np.nan)                                                 # buildDataFrameWithNARows, :823
        full[nz] = v
        out[k] = full
    return out


def zero_rule(cols, flag):
    """:1024-1028: LFC and statistic 0, p-value 1; lfcSE keeps its value"""
    out = {k: np.array(v, copy=True) for k, v in cols.items()}
    out["log2FoldChange"][flag] = 0.0
    out["stat"][flag] = 0.0
    out["pvalue"][flag] = 1.0
    return out


def contrast_table(O, cols, baseMean, mask, counts, allZero, lrt=None, replace=None, na_mask=None, lfcThreshold=0.0,
                   altHypothesis="greaterAbs", filter=None, theta=None, alpha=0.1):
    """cleanContrast's tail on the four columns `cols` (from get_contrast, or pulled from the stored coefficient), then what
    results() does with them (results_spec.results).  lrt: (LRTStatistic, LRTPvalue) overwrites stat and pvalue (:1030-1037)"""
    cols = zero_rule(cols, all_zero(counts, mask, allZero))
    if lrt is not None:
        cols["stat"], cols["pvalue"] = np.asarray(lrt[0], np.float64), np.asarray(lrt[1], np.float64)
    return results_spec.results(O, cols["log2FoldChange"], cols["lfcSE"], cols["stat"], cols["pvalue"], baseMean, replace=replace,
                                na_mask=na_mask, lfcThreshold=lfcThreshold, altHypothesis=altHypothesis, filter=filter,
                                theta=theta, alpha=alpha)
