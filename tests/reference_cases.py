"""The recorded outputs of the reference build (oracle/_ref, see oracle/Makefile `ref`): which cases are recorded, how a
result is packed into tests/golden/reference/<case>.npz and read back, and the comparison each kind of case is held to.
Shared by tests/golden/make_reference_golden.py (writes the files), tests/test_oracle_vs_reference.py (CPU: the C oracle and
the LAPACK restatement against them), tests/test_gpu_reference.py (the HIP path against them) and tools/parity_report.py.

The inputs are rebuilt from their seeds by the case builders that already exist (golden_cases of
tests/test_oracle_vs_lapack.py, tests/wide_cases.py, tests/floor_regime.py); only the reference's OUTPUTS are stored.

What a file holds.  Every per-gene vector in full (fitBeta: iter, deviance, contrast_num, contrast_denom; fitDisp: all nine
outputs of both searches; fitDispGrid: log_alpha; the floor cases: every entry of visible_chain()).  The matrices --
beta_mat, beta_var_mat, hat_diagonals -- for the first G_HEAD genes only: hat_diagonals is genes x samples, and at 1500
samples a full one would alone be larger than any file this directory may hold.  complete() fills the rows that are not
recorded from the result under test, so that compare() can be called as it stands: its matrix assertions then say nothing
about the genes from G_HEAD on, whose fit is still held by the vectors (iter and deviance of fitBeta; every fitDisp output
downstream of their fitted means)."""
import os

import numpy as np

from tests import wide_cases
from tests.floor_regime import SEEDS, assert_visible_parity, floor_case, visible_chain

G_HEAD = 16                    # genes whose rows of beta_mat, beta_var_mat and hat_diagonals are recorded; same for every case
MATRICES = ("beta_mat", "beta_var_mat", "hat_diagonals")
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
MAX_FILE_BYTES = 239394        # tests/golden/nmath_golden.json, the largest fixture there was before these

# Budgets of a single case.  Everything is held to compare() / assert_visible_parity() as they stand, except where a case
# misses one of their SHARE budgets against the reference build and the LAPACK restatement -- which is not the code under test
# either -- misses it against the reference build as well: the miss is then a property of the input (its genes at the
# dispersion floor), and that case alone is held to the LAPACK-vs-reference measurement less one gene (shares are quantised in
# genes, and one last-bit decision can flip on either side).  Measured (profiles/reference_parity.md):
#   paired45 (100 genes)           fitDispGrid identical: oracle 94, LAPACK 94 (budget 0.95 -> 95): 93.  The six genes are the
#                                  same for both -- oracle and LAPACK agree on all 100 -- and end on neighbouring points of the
#                                  fine grid at 0.94e-8 / 1.07e-8, below minDisp: there lgamma(y + 1e8) - lgamma(1e8) in
#                                  double carries ulp(1.7e9) = 2.4e-7 per term, more than the posterior differs between the two
#                                  points; the binary128 stand-in rounds once, both double implementations do not
#   floor_paired20x2 (300 genes)   clamped dispGeneEst beyond 1e-6 relative: oracle 10, LAPACK 15 (budget 0.03 n = 9): 16;
#                                  all of them floor genes, dge_abs_max 4.5e-11 (budget 1e-7, unchanged)
CASE_BUDGETS = {
    "paired45": dict(min_grid=0.93),
    "floor_paired20x2": dict(max_dge_rel=16),
}
# ... and where ONLY the LAPACK restatement misses (cephes' special functions in double against binary128, again on floor
# genes alone; the oracle is within the unchanged budget there and stays held to it), its own comparison with the reference
# build is held to what it measured less one gene -- a pin on that figure, not a claim about the code under test:
#   c1_two_group_m6 (118 genes)    fitDispGrid identical: LAPACK 100 (budget 0.85 -> 101; oracle 103): 99
#   floor_factor16_m64 (300 genes) dispGeneEstConv differs: LAPACK 29 (budget 0.08 n = 24; oracle 24): 30
LAPACK_ONLY_BUDGETS = {
    "c1_two_group_m6": dict(min_grid=99 / 118),
    "floor_factor16_m64": dict(max_conv_differs=30),
}

NARROW = ("c1_two_group_m6", "bc_m12", "bc_m24_weights", "two_m10_normal_eq", "factor5_m20_ridge",
          "two_m16_zero_weights_noCR")
FLOOR_SEEDS = tuple("floor_seed%d" % s for s in SEEDS)


def kinds():
    """name -> kind of every recorded case, in the order the generator runs them"""
    k = {n: "narrow" for n in NARROW}
    k.update({n: "wide" for n in wide_cases.WIDE})
    k.update({n: "expanded" for n in wide_cases.EXPANDED})
    k.update({n: "floor" for n in wide_cases.FLOOR})
    k.update({n: "floor" for n in FLOOR_SEEDS})
    return k


_narrow = {}


def build(name):
    """the inputs of a recorded case, from its seed"""
    kind = kinds()[name]
    if kind == "narrow":
        if not _narrow:
            from tests.test_oracle_vs_lapack import golden_cases
            _narrow.update(golden_cases())
            assert tuple(_narrow) == NARROW
        return _narrow[name]
    if kind == "wide":
        return wide_cases.wide_case(name)
    if kind == "expanded":
        return wide_cases.expanded_case(name)
    if name in wide_cases.FLOOR:
        return wide_cases.floor_wide_case(name)
    return floor_case(int(name[len("floor_seed"):]))


def run(F, name, d):
    """the call sequence a case is recorded under: run_all(), or visible_chain() for the floor regime"""
    if kinds()[name] == "floor":
        return visible_chain(F, d)
    from tests.test_oracle_vs_lapack import run_all
    return run_all(F, d)


def pack(name, res):
    """a result as the flat {key: array} a fixture file holds"""
    if kinds()[name] == "floor":
        return {k: np.asarray(v) for k, v in res.items()}
    out = {}
    for fn, dd in res.items():
        if fn == "aux":
            continue
        for k, v in dd.items():
            if v is not None:
                a = np.asarray(v)
                out["%s/%s" % (fn, k)] = a[:G_HEAD] if k in MATRICES else a
    return out


def path(name):
    return os.path.join(DIR, name + ".npz")


def load(name):
    """the recorded reference result of a case: {routine: {key: array}}, flat for the floor cases"""
    with np.load(path(name)) as z:
        flat = {k: z[k] for k in z.files}
    if kinds()[name] == "floor":
        return flat
    ref = {}
    for key, v in flat.items():
        fn, k = key.split("/")
        ref.setdefault(fn, {})[k] = v
    return ref


def complete(ref, got):
    """the recorded result with the rows of its matrices that are not recorded (genes from G_HEAD on) taken from `got`"""
    full = {fn: dict(dd) for fn, dd in ref.items()}
    for fn, dd in full.items():
        for k in MATRICES:
            if k in dd:
                g = np.asarray(got[fn][k], dtype=np.float64)
                if dd[k].shape == g.shape:         # a live result: nothing is missing
                    continue
                assert dd[k].shape == (min(G_HEAD, g.shape[0]),) + g.shape[1:], "%s$%s: recorded %r, computed %r" % (
                    fn, k, dd[k].shape, g.shape)
                dd[k] = np.concatenate([dd[k], g[G_HEAD:]], axis=0)
    return full


def check(got, ref, name, d, label, lapack=False):
    """`got` against the recorded (or live) reference result `ref` of the case `name` under the budgets of its kind: compare()
    as it stands -- min_well = wide_cases.MIN_WELL for the wide cases, the second pass of the expanded designs at scale 1 --
    or assert_visible_parity() for the floor regime; CASE_BUDGETS where the case has one (lapack: `got` is the LAPACK
    restatement's result, LAPACK_ONLY_BUDGETS too).  Returns the measured rates."""
    kind = kinds()[name]
    own = dict(CASE_BUDGETS.get(name, {}), **(LAPACK_ONLY_BUDGETS.get(name, {}) if lapack else {}))
    if kind == "floor":
        return assert_visible_parity(got, ref, label, **own)
    from tests.test_oracle_vs_lapack import _fit_beta_compare, compare
    ref = complete(ref, got)
    if kind == "narrow":
        return compare(got, ref, d, label, **own)
    st = compare(got, ref, d, label, min_well=wide_cases.MIN_WELL, **own)
    if kind == "expanded":
        _fit_beta_compare(got["fitBetaPrior"], ref["fitBetaPrior"], label, "fitBetaPrior", 1.0)
    return st
