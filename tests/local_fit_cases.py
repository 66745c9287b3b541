"""Shared builders for the local-regression trend tests (tests/test_local_fit_cpu.py, tests/test_gpu_local_fit.py): the fit
sets, the evaluation lists, and the specification's values for each pair, computed once per session and never changed."""
import numpy as np

from tests import local_fit_spec as S

MIN_DISP = 1e-8
LANES = S.LANES
BLOCK_POINTS = 4                      # evaluation points per workgroup of the device kernel (one wave each)
GRID_ROUND = 8 * 256 * BLOCK_POINTS   # ... and per round of its largest grid (8 workgroups per CU, 256 CUs)


def _trend(n, seed, lo=1.0, hi=1e4):
    rng = np.random.Generator(np.random.PCG64(seed))
    means = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    disps = (0.05 + 3.0 / means) * np.exp(rng.normal(0.0, 0.3, n))
    return means, disps


def _ties(n_distinct, reps, seed):
    means, disps = _trend(n_distinct * reps, seed)
    means = np.repeat(means[:n_distinct], reps)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    p = rng.permutation(means.size)
    return means[p], disps[p]


def _mixed(seed):
    means, disps = _trend(90, seed)
    disps[::3] = 5e-8                     # below 10 minDisp: left out
    disps[4] = np.nan
    disps[7] = 10 * MIN_DISP              # exactly at the floor: kept
    means[10] = 0.0                       # no logarithm: left out
    return means, disps


# name -> (means, disps); N = the size of the fit set
FIT_SETS = {
    "n5": _trend(5, 1),                              # k = 3, the smallest legal case
    "n20": _trend(20, 2),
    "n63": _trend(LANES - 1, 3),                     # one below the summation parameter
    "n64": _trend(64, 4),
    "n65": _trend(LANES + 1, 5),                     # one above it
    "n129": _trend(129, 6),
    "n300": _trend(300, 7),                          # past one workgroup's 4 x 64 points; windows over several aligned chunks
    "n1000": _trend(1000, 8),
    "ties": _ties(11, 3, 9),                         # N = 33, k = 23 (no multiple of 3): a window edge cuts a run of equal x
    "mixed": _mixed(10),                             # rows below the floor, a NaN, a zero mean among the rest
    "weights": _trend(200, 11, lo=1.0, hi=1e6),      # prior weights over six decades
    "all_equal": (np.full(20, 37.5), _trend(20, 12)[1]),            # one distinct x: singular everywhere
    "all_below": (_trend(12, 13)[0], np.full(12, 5e-8)),            # the constant minDisp
}
TOO_FEW = {"n4": _trend(4, 14), "n1": _trend(1, 15)}                # k < 3: raises


def eval_list(fit_name, which):
    means = FIT_SETS[fit_name][0]
    pos = means[means > 0]
    rng = np.random.Generator(np.random.PCG64(len(fit_name) * 131 + len(which)))
    lo, hi = np.log(pos.min()), np.log(pos.max())
    if which == "one":
        return np.exp(rng.uniform(lo, hi, 1))
    if which == "n65":
        return np.exp(rng.uniform(lo, hi, 65))
    if which == "n203":                              # no multiple of the points per workgroup
        return np.exp(rng.uniform(lo - 0.5, hi + 0.5, 203))
    if which == "rounds":                            # more points than one round of the largest grid
        return np.exp(rng.uniform(lo, hi, GRID_ROUND + 5))
    if which == "special":                           # fit points, outside the range on both sides, and what has no logarithm
        return np.array([pos[0], pos[pos.size // 2], np.sort(pos)[0], np.sort(pos)[-1], pos.min() / 7.0, pos.min() * (1 - 2.0 ** -52),
                         pos.max() * 9.0, 1e-300, 1e300, np.nan, 0.0, -1.0, np.inf, -np.inf])
    raise KeyError(which)


# every (fit set, evaluation list) pair the tests run
PAIRS = ([(f, "n65") for f in FIT_SETS] + [(f, "special") for f in FIT_SETS] +
         [("n5", "one"), ("n300", "one"), ("n129", "n203"), ("n1000", "n203"), ("n20", "rounds")])

_REFERENCE = {}


def reference(fns, fit_name, which):
    """(dispFit, nSingular, the fit tuple) by the specification; computed once"""
    key = (fit_name, which)
    if key not in _REFERENCE:
        means, disps = FIT_SETS[fit_name]
        fit = S.local_fit(fns, means, disps, MIN_DISP)
        out, nsing = S.evaluate(fns, fit, eval_list(fit_name, which))
        out.setflags(write=False)
        _REFERENCE[key] = (out, nsing, fit)
    return _REFERENCE[key]
