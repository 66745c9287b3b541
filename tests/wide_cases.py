"""Designs of 11 to 64 columns for the comparisons with the LAPACK restatement (oracle/lapack_oracle.py): shared by
tests/test_oracle_vs_lapack.py and tests/test_floor_regime.py (CPU: the C oracle) and tests/test_gpu_vs_lapack.py (the HIP
path), and the home of the paired design tests/test_gpu_wide.py uses.  Every case is the dict run_all() of
tests/test_oracle_vs_lapack.py takes; a case is built when it is asked for (wide_case(name)), not at import.

Each entry of WIDE names the kernel variant it is there for, read off launch_fit_beta_p / fit_beta_on_cells /
wide_geometry (csrc/fit_beta*.hip, dsq_internal.hpp) and launch_fit_disp_p / fit_disp_rolled_applies / launch_dispw
(csrc/fit_disp*.hip); profiles/wide_parity.md holds the DSQ_VERBOSE=1 line each case printed on the device.  The gene counts
are what the numpy side finishes in seconds; m is the smallest that still takes the path."""
import numpy as np

from deseq2_amd import simulate
from tests.helpers import beta_init_qr, rough_alpha

MIN_WELL = 0.9          # cap on the well-conditioned share of the wide cases (a property of the inputs: measured 0.92 .. 1.0)


def paired(patients, reps=1):
    """~ patient + treatment: every patient measured `reps` times under both treatments (2 * reps * patients samples,
    p = patients + 1, 2 * patients design cells -- beyond 16 patients more than the 32 the cell-collapsed paths take: the
    general per-sample kernels)"""
    m = 2 * reps * patients
    pat = np.repeat(np.arange(patients), 2 * reps)
    trt = np.tile(np.repeat([0.0, 1.0], reps), patients)
    x = np.column_stack([np.ones(m)] + [(pat == k).astype(float) for k in range(1, patients)] + [trt])
    assert np.linalg.matrix_rank(x) == patients + 1
    return x


def factor_cont(m, levels):
    """a factor and ONE continuous covariate (p = levels + 1): one design cell per sample"""
    x = np.column_stack([simulate.design_factor(m, levels),
                         np.random.Generator(np.random.PCG64(m + levels + 77)).normal(0.0, 0.5, m)])
    assert np.linalg.matrix_rank(x) == levels + 1
    return x


def case(n, x, weights=False, zero_w=False, useQR=True, useCR=True, lam=1e-6, seed=None):
    """counts on the design x with log-normal size factors; weights, zero_w, useQR, useCR and lam as in
    test_oracle_vs_lapack._case"""
    m, p = x.shape
    seed = m + p if seed is None else seed
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    sf = np.exp(rng.normal(0, 0.25, m))
    d = simulate.make_counts(n, x, seed=seed, size_factors=sf, beta_sd=np.array([0.4] * (p - 2) + [1.0]))
    counts = d["counts"]
    nn = counts.shape[0]
    nf = np.broadcast_to(sf[None, :], (nn, m)).copy()
    w = np.ones((nn, m))
    if weights:
        w = rng.uniform(0.05, 1.0, (nn, m))
        w[rng.uniform(size=(nn, m)) < 0.02] = 0.0
        w = w / w.max(axis=1, keepdims=True)      # R/core.R:2702
    if zero_w:
        w[:, ::5] = 0.0                           # whole samples dropped
    with np.errstate(all="ignore"):
        b0 = beta_init_qr(counts.astype(float), nf, x)
        a0 = rough_alpha(counts.astype(float), nf, x)
    d.update(x=x, nf=nf, weights=w, beta_init=b0, alpha_init=a0, useWeights=weights, useQR=useQR, useCR=useCR,
             lam=np.full(p, lam) / np.log(2) ** 2)
    return d


def _factor(levels, m):
    return lambda: simulate.design_factor(m, levels)


def _paired(patients, reps=1):
    return lambda: paired(patients, reps)


def _cont(p, m):
    return lambda: factor_cont(m, p - 1)


# name -> (genes, design, options).  The comment of a case: B = the fitBeta launch, D = the fitDisp launches (search /
# second-derivative pass / grid) as the DSQ_VERBOSE=1 lines of the device run name them (profiles/wide_parity.md); "rolled k w"
# = the rolled kernel with k waves per gene, "LDS" / "global" = where fitBeta keeps the gene's slab
WIDE = {
    # ---- factors: cell-collapsed fits up to 32 levels, and their end
    "factor12_m60": (100, _factor(12, 60), {}),                                # B fit_beta_cells<16>; D fit_disp<16> on 12 cells (4 padding columns)
    "factor16_m96_weights": (100, _factor(16, 96), dict(weights=True)),        # B fit_beta_cells<16> with weights, no padding; D fit_disp<16>
    "factor24_m120_ne": (100, _factor(24, 120), dict(useQR=False)),            # B fit_beta_cells<24>, normal equations; D fit_disp<24>
    "factor32_m132": (80, _factor(32, 132), {}),                               # B fit_beta_cells<32>: 32 cells + 32 columns = the 64 lanes, DSQ_SPEC_BETA_CELL_MAXP; D fit_disp<32>
    "factor33_m132": (80, _factor(33, 132), {}),                               # one past it: B rolled 4 w LDS; D rolled 2 / 4 / 1 w
    "factor48_m192": (60, _factor(48, 192), {}),                               # B rolled 8 w LDS at the 48-column build's own width; D rolled 4 / 8 / 2 w
    "factor64_m256": (40, _factor(64, 256), {}),                               # DSQ_MAX_P: B rolled 4 w global; D rolled 8 / 8 / 4 w, 148 KB of LDS
    "factor64_m130_weights": (40, _factor(64, 130), dict(weights=True)),       # B rolled<weights> 8 w LDS (143 KB); D rolled<weights> 8 / 8 / 4 w
    "factor11_m44_ridge": (100, _factor(11, 44), dict(lam=0.5)),               # narrowest wide width, a ridge that matters: B fit_beta_cells<16>; D fit_disp<16>
    # ---- paired designs: more than 32 cells, the general per-sample path
    "paired12x2_weights": (100, _paired(12, 2), dict(weights=True)),           # 24 cells, p = 13: B fit_beta_cells<16>; D fit_disp<16>, with weights
    "paired30_qr": (100, _paired(30), {}),                                     # p = 31: B rolled 2 w LDS, Householder QR; D rolled 2 / 2 / 1 w
    "paired30_ne": (100, _paired(30), dict(useQR=False)),                      # B rolled 2 w LDS, normal equations (Gram + LU)
    "paired30_ridge": (100, _paired(30), dict(lam=0.5)),                       # B rolled 2 w LDS, ridge rows that matter
    "paired26_weights": (100, _paired(26), dict(weights=True)),                # p = 27 of the 32-column build: B rolled<weights> 2 w LDS; D rolled<weights> 2 / 2 / 1 w
    "paired45": (100, _paired(45), {}),                                        # p = 46: B rolled 4 w LDS; D rolled 4 / 4 / 2 w
    "paired55_noCR": (50, _paired(55), dict(useCR=False)),                     # p = 56 of the 64-column build: B rolled 8 w LDS; D rolled 8 / 8 / 2 w without the Cox-Reid term
    "paired63_weights": (40, _paired(63), dict(weights=True)),                 # p = 64: B rolled<weights> 8 w LDS; D rolled<weights> 8 / 8 / 4 w
    # ---- a factor plus a continuous covariate: the summation-order boundaries of dsq_arith_spec.h and the long-row paths
    "cont_p11_m257_ne_noCR": (100, _cont(11, 257), dict(useQR=False, useCR=False)),   # narrowest rolled width: B rolled 2 w LDS, normal equations; D rolled 1 w
    "cont_p12_m1024": (60, _cont(12, 1024), {}),                               # DSQ_SPEC_SERIAL_GRAM_MAXM, the last row of the serial Gram sums: B rolled 8 w LDS; D rolled 4 w
    "cont_p12_m1025": (60, _cont(12, 1025), {}),                               # one past it, wave-order sums: B rolled 8 w LDS; D fit_disp<16>, the per-width kernel
    "cont_p16_m1500_weights": (50, _cont(16, 1500), dict(weights=True)),       # long weighted rows: B rolled<weights> 4 w global; D fit_disp<16>
    "cont_p31_m124": (80, _cont(31, 124), {}),                                 # one padding column: B rolled 4 w LDS; D rolled 2 / 2 / 1 w
    "cont_p40_m700": (50, _cont(40, 700), {}),                                 # B rolled 4 w global (slab beyond the LDS); D rolled 8 / 8 / 4 w
    "cont_p48_m1024_weights": (40, _cont(48, 1024), dict(weights=True)),       # B rolled<weights> 4 w global; D rolled<weights> 8 w at the serial-sum limit
    "cont_p49_m1024": (40, _cont(49, 1024), {}),                               # the longest row fitDisp takes from 49 columns: B rolled 4 w global; D rolled 8 w, 140 KB of LDS
    "cont_p64_m260_zero_weights": (40, _cont(64, 260), dict(weights=True, zero_w=True)),   # DSQ_MAX_P, whole samples at zero weight: B rolled 4 w global; D rolled 8 / 8 / 4 w
    # ---- long factor rows
    "factor24_m1200": (60, _factor(24, 1200), {}),                             # B fit_beta_cells<24>; D fit_disp<24> on rows beyond 1024 samples
}

# betaPrior pass 2 on a wide factor: levels -> (genes, samples, weights)
EXPANDED_LEVELS = {12: (100, 48, False), 20: (100, 80, True), 47: (50, 188, False), 63: (40, 252, False)}
EXPANDED = tuple("expanded%d_%s" % (k, s) for k in EXPANDED_LEVELS for s in ("qr", "ne"))


def wide_case(name):
    n, design, kw = WIDE[name]
    return case(n, design(), **kw)


def expanded_case(name):
    """fitGLMsWithPrior's second pass (R/fitNbinomGLMs.R:319-325) on the expanded model matrix of a factor
    (R/expanded.R:1-18): intercept plus one column per level (rank deficient), lambda = (1e-6, 1, ..., 1) / ln(2)^2, the
    contrast of the last level against the first; the first pass runs on the standard design of the same factor"""
    levels, solver = name[len("expanded"):].split("_")
    levels = int(levels)
    n, m, weights = EXPANDED_LEVELS[levels]
    x = simulate.design_factor(m, levels)
    d = case(n, x, weights=weights, useQR=solver == "qr")
    grp = (np.arange(m) * levels) // m
    d["x_expanded"] = np.column_stack([np.ones(m)] + [(grp == g).astype(float) for g in range(levels)])
    d["lam_expanded"] = np.r_[1e-6, np.ones(levels)] / np.log(2) ** 2
    c = np.zeros(levels + 1)
    c[1], c[levels] = -1.0, 1.0
    d["contrast_expanded"] = c
    return d


# the dispersion-floor regime (tests/floor_regime.py) at wide widths: name -> (seed, design)
FLOOR = {
    "floor_paired20x2": (21, _paired(20, 2)),        # p = 21, m = 80: B rolled 2 w LDS; D rolled 1 w
    "floor_factor16_m64": (16, _factor(16, 64)),     # p = 16, m = 64: B fit_beta_cells<16>; D fit_disp<16>
}


def floor_wide_case(name):
    from tests.floor_regime import floor_case
    seed, design = FLOOR[name]
    x = design()
    return floor_case(seed, n=300, m=x.shape[0], frac_pois=0.6, design=x)


def take_rows(d, rows):
    """the case restricted to the genes `rows`: the fits are per gene, every per-gene input is a row of a matrix or an entry of
    a vector"""
    per_gene = ("counts", "nf", "weights", "beta_init", "alpha_init", "beta", "alpha")
    return {k: (v[rows] if k in per_gene else v) for k, v in d.items()}
