"""Seeded inputs shared by the apeglm tests (tests/test_apeglm_cpu.py, tests/test_gpu_apeglm.py).  Not a test itself."""
import numpy as np

from deseq2_amd import simulate

SPEC_KEYS = ("map", "sd", "fsr", "thresh", "iter", "conv", "start", "objective")
LDS_DOUBLES = 4096             # dsq_apeglm_lds_doubles(): the design is staged in LDS while m * p <= this
WAVES = 4                      # genes of a workgroup
GRID_GENES = 8 * 256 * WAVES   # the genes of one grid round on 256 compute units


def prototype_designs():
    """the four designs of the comparison with scipy"""
    return {"two_group_6": simulate.design_two_group(6), "two_group_20": simulate.design_two_group(20),
            "batch_condition_12": simulate.design_batch_condition(12), "factor_16_4": simulate.design_factor(16, 4)}


def design(m, p, seed=3):
    """intercept, a 50/50 factor column, then factor and continuous columns by turns: full rank for m > p"""
    rng = np.random.default_rng(seed)
    cols = [np.ones(m), (np.arange(m) % 2).astype(np.float64)]
    for k in range(2, p):
        cols.append(((np.arange(m) // (k + 1)) % 2).astype(np.float64) if k % 2 == 0 else np.round(rng.normal(size=m), 3))
    return np.column_stack(cols[:p])


def make(n, m, p, seed, x=None, matrix_nf=False, weights=False, init=True, big_effects=True):
    """dict(Y int32 n x m, x, nf (m or n x m), disp n, weights (n x m or None), init (n x p or None), coef)"""
    rng = np.random.default_rng(seed)
    x = design(m, p) if x is None else x
    p = x.shape[1]
    sf = np.exp(rng.normal(0.0, 0.3, m))
    beta = np.zeros((n, p))
    beta[:, 0] = rng.normal(4.0, 1.5, n)
    beta[:, 1:] = rng.normal(0.0, 0.5, (n, p - 1))
    if big_effects:
        beta[::5, p - 1] = rng.choice([-3.0, 3.0], beta[::5].shape[0])          # the rows the second start is for
    disp = np.exp(rng.uniform(np.log(0.01), np.log(1.0), n))
    mu = sf * np.exp(np.clip(beta @ x.T, -20, 12))
    Y = rng.negative_binomial(1.0 / disp[:, None], 1.0 / (1.0 + disp[:, None] * mu)).astype(np.int32)
    nf = sf
    if matrix_nf:
        nf = sf * np.exp(rng.normal(0.0, 0.1, (n, m)))
    w = None
    if weights:
        w = np.round(rng.uniform(0.2, 1.0, (n, m)), 3)
        w[0, 0] = 0.0                                     # an exact zero
        w[:, m - 1] = 0.0                                 # a sample of all-zero weights
    b0 = None
    if init:
        b0 = beta + rng.normal(0.0, 0.05, beta.shape)     # stands for the maximum-likelihood coefficients
    return {"Y": Y, "x": x, "nf": nf, "disp": disp, "weights": w, "init": b0, "coef": p - 1}


def special_rows(c):
    """overwrite the first rows of a case with the rows the issue lists; needs n >= 8 and a two-level column 1"""
    Y, disp = c["Y"], c["disp"]
    m = Y.shape[1]
    Y[0] = 0                                              # all-zero
    disp[1] = np.nan                                      # NaN dispersion
    Y[2, c["x"][:, 1] != 0] = 0                           # one whole group zero: the MLE start sits at the clip
    if c["init"] is not None:
        c["init"][2, 1] = -40.0
    Y[3, 0] = 2 ** 31 - 1                                 # the largest count
    disp[4] = 1e-8
    disp[5] = 1e2
    disp[6] = 0.0                                         # not positive
    disp[7] = np.inf
    return c


def scipy_rows(seed, x, n=94):
    """one of the sixteen (design, seed) sets of the comparison with scipy: make_counts, log-normal size factors, true dispersions"""
    rng = np.random.default_rng(100 + seed)
    m = x.shape[0]
    sf = np.exp(rng.normal(0.0, 0.3, m))
    d = simulate.make_counts(n, x, seed=seed, size_factors=sf)
    return {"Y": d["counts"], "x": x, "nf": d["size_factors"], "disp": d["alpha"], "coef": x.shape[1] - 1}


def on_optimum_rows():
    """six rows of a 20 000 x 48 two-group simulation (dispersions near 1, prior scale 0.83) on which the search sat on the
    optimum -- gradient 3e-14, Newton step 3e-16 -- and ran to maxit while the resolution of F was taken relative to |F|:
    F cancels to less than 1 there while its terms sum to 1e4.  tests/golden/apeglm_on_optimum_rows.npz: Y, disp, init, x, sf"""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apeglm_on_optimum_rows.npz"))
    mask = np.array([True, False])
    return {"name": "on_optimum", "Y": d["Y"].astype(np.int32), "x": d["x"], "nf": d["sf"], "disp": d["disp"], "weights": None,
            "init": d["init"], "coef": 1, "S": 0.83, "threshold": None, "no_shrink": mask, "maxit": 100, "y_f64": False, "pad": 0,
            "layout_r": False, "stream": False, "tile": None}


def _case(name, n, m, p, seed, S=0.3, threshold=None, no_shrink=(0,), coef=None, maxit=100, special=True, y_f64=False, pad=0,
          layout_r=False, stream=False, tile=None, **kw):
    c = make(n, m, p, seed, **kw)
    if special and n >= 8:
        special_rows(c)
    if coef is not None:
        c["coef"] = coef
    mask = np.zeros(c["x"].shape[1], bool)
    mask[list(no_shrink)] = True
    c.update(name=name, S=S, threshold=threshold, no_shrink=mask, maxit=maxit, y_f64=y_f64, pad=pad, layout_r=layout_r,
             stream=stream, tile=tile)
    return c


def gpu_cases():
    """the shapes and options of tests/test_gpu_apeglm.py; tests/test_apeglm_cpu.py holds the host engine to the
    specification on every one of them.  tile: the device run repeats the rows up to that many genes"""
    out = []
    for m in (3, 63, 64, 65, 128, 129, 257):
        out.append(_case("m%d" % m, 37, m, 2, seed=m, threshold=0.4 if m % 2 else None, weights=m in (65, 257),
                         matrix_nf=m in (64, 129)))
    for m in (LDS_DOUBLES // 2, LDS_DOUBLES // 2 + 1):          # the design in LDS, and read through L2
        out.append(_case("m%d" % m, 9, m, 2, seed=m))
    for p in (2, 3, 4, 5, 8, 9, 16):
        out.append(_case("p%d" % p, 37, 40, p, seed=50 + p, S=0.05 if p in (2, 5) else 0.3, threshold=0.2, weights=p in (4, 9, 16),
                         matrix_nf=p in (3, 16)))
    for n in (1, WAVES - 1, WAVES, WAVES + 1):
        out.append(_case("n%d" % n, n, 12, 2, seed=80 + n))
    out.append(_case("grid_rounds", 37, 6, 2, seed=90, tile=GRID_GENES + 5))
    out.append(_case("long_rows", 8, 2000, 4, seed=91, weights=True, threshold=0.3))
    out.append(_case("f64_counts", 20, 13, 3, seed=92, y_f64=True, weights=True, matrix_nf=True, pad=16, threshold=0.5))
    out.append(_case("ld_padding", 20, 13, 3, seed=93, pad=24, matrix_nf=True))
    out.append(_case("r_layout", 20, 13, 3, seed=94, layout_r=True, matrix_nf=True, weights=True))
    out.append(_case("no_shrink_01", 20, 14, 3, seed=95, no_shrink=(0, 1), coef=2))
    out.append(_case("no_init", 20, 14, 3, seed=96, init=False, threshold=0.1))
    out.append(_case("maxit0", 20, 14, 3, seed=97, maxit=0))
    out.append(_case("maxit1", 20, 14, 3, seed=98, maxit=1))
    out.append(_case("stream", 20, 14, 3, seed=99, stream=True))
    out.append(_case("small_scale", 60, 10, 2, seed=100, S=0.05))
    out.append(on_optimum_rows())
    # every instantiation of the kernel (padded width 4 / 8 / 16 x int32 / float64 counts x design in LDS / through L2) that
    # the cases above leave out
    for p, m_l2 in ((4, 1100), (8, 600), (16, 300)):
        for f64 in (False, True):
            if not (p == 4 and not f64):
                out.append(_case("p%d_%s_l2" % (p, "f64" if f64 else "i32"), 12, m_l2, p, seed=110 + p + f64, y_f64=f64,
                                 weights=p == 16, threshold=0.2))
        if p > 4:
            out.append(_case("p%d_f64_lds" % p, 12, 40, p, seed=120 + p, y_f64=True, matrix_nf=True))
    return out
