"""-m gpu: the HIP path (host-pointer C ABI) against the reference's own compiled source -- the comparison the C oracle is
held to in tests/test_oracle_vs_reference.py, with the same calls and budgets (tests/reference_cases.py).

  recorded   every case of tests/golden/reference/: the six narrow cases, wide_cases.WIDE / EXPANDED / FLOOR and the floor
             seeds.  Needs only the committed files, never skips.  The wide cases are the smallest shapes at which each kernel
             variant is selected, and the test asserts that variant from the DSQ_VERBOSE launch lines, so that a change of the
             launch geometry cannot move a case onto another kernel unnoticed.
  live       when oracle/_ref/libdeseq2_ref.so travelled with the tree and loads: four inputs that are not recorded, the
             reference running on the host for a second or so each.

Nothing here reads the reference tree."""
import re

import pytest

from deseq2_amd import native
from oracle import reference
from tests import reference_cases as RC
from tests import test_oracle_vs_lapack as T

pytestmark = pytest.mark.gpu

# ---- the kernel variant of each wide case, as the comments of wide_cases.WIDE / FLOOR name it (profiles/wide_parity.md) ------
# fitBeta:  ("cells", P) = fit_beta_cells<P>;  ("rolled", waves per gene, "LDS" | "global") = the rolled kernel and where it
#           keeps the gene's slab.  The expanded designs have two entries: the first pass (p) and the prior pass (p + 1).
# fitDisp:  ("width", P) = fit_disp<P>, the per-width kernel;  ("rolled", w0, w2, w1) = the rolled kernel's waves per gene in
#           the search (mode 0), the second-derivative pass (mode 2) and the grid (mode 1; None where the case has no grid)
VARIANT = {
    "factor12_m60": ([("cells", 16)], ("width", 16)),
    "factor16_m96_weights": ([("cells", 16)], ("width", 16)),
    "factor24_m120_ne": ([("cells", 24)], ("width", 24)),
    "factor32_m132": ([("cells", 32)], ("width", 32)),
    "factor33_m132": ([("rolled", 4, "LDS")], ("rolled", 2, 4, 1)),
    "factor48_m192": ([("rolled", 8, "LDS")], ("rolled", 4, 8, 2)),
    "factor64_m256": ([("rolled", 4, "global")], ("rolled", 8, 8, 4)),
    "factor64_m130_weights": ([("rolled", 8, "LDS")], ("rolled", 8, 8, 4)),
    "factor11_m44_ridge": ([("cells", 16)], ("width", 16)),
    "paired12x2_weights": ([("cells", 16)], ("width", 16)),
    "paired30_qr": ([("rolled", 2, "LDS")], ("rolled", 2, 2, 1)),
    "paired30_ne": ([("rolled", 2, "LDS")], ("rolled", 2, 2, 1)),
    "paired30_ridge": ([("rolled", 2, "LDS")], ("rolled", 2, 2, 1)),
    "paired26_weights": ([("rolled", 2, "LDS")], ("rolled", 2, 2, 1)),
    "paired45": ([("rolled", 4, "LDS")], ("rolled", 4, 4, 2)),
    "paired55_noCR": ([("rolled", 8, "LDS")], ("rolled", 8, 8, 2)),
    "paired63_weights": ([("rolled", 8, "LDS")], ("rolled", 8, 8, 4)),
    "cont_p11_m257_ne_noCR": ([("rolled", 2, "LDS")], ("rolled", 1, 1, 1)),
    "cont_p12_m1024": ([("rolled", 8, "LDS")], ("rolled", 4, 4, 4)),
    "cont_p12_m1025": ([("rolled", 8, "LDS")], ("width", 16)),
    "cont_p16_m1500_weights": ([("rolled", 4, "global")], ("width", 16)),
    "cont_p31_m124": ([("rolled", 4, "LDS")], ("rolled", 2, 2, 1)),
    "cont_p40_m700": ([("rolled", 4, "global")], ("rolled", 8, 8, 4)),
    "cont_p48_m1024_weights": ([("rolled", 4, "global")], ("rolled", 8, 8, 8)),
    "cont_p49_m1024": ([("rolled", 4, "global")], ("rolled", 8, 8, 8)),
    "cont_p64_m260_zero_weights": ([("rolled", 4, "global")], ("rolled", 8, 8, 4)),
    "factor24_m1200": ([("cells", 24)], ("width", 24)),
    "expanded12_qr": ([("cells", 16), ("cells", 16)], ("width", 16)),
    "expanded12_ne": ([("cells", 16), ("cells", 16)], ("width", 16)),
    "expanded20_qr": ([("cells", 24), ("cells", 24)], ("width", 24)),
    "expanded20_ne": ([("cells", 24), ("cells", 24)], ("width", 24)),
    "expanded47_qr": ([("rolled", 8, "LDS"), ("rolled", 8, "LDS")], ("rolled", 4, 8, 2)),
    "expanded47_ne": ([("rolled", 8, "LDS"), ("rolled", 8, "LDS")], ("rolled", 4, 8, 2)),
    "expanded63_qr": ([("rolled", 4, "global"), ("rolled", 4, "global")], ("rolled", 8, 8, 4)),
    "expanded63_ne": ([("rolled", 4, "global"), ("rolled", 4, "global")], ("rolled", 8, 8, 4)),
    "floor_paired20x2": ([("rolled", 2, "LDS")], ("rolled", 1, 1, None)),
    "floor_factor16_m64": ([("cells", 16)], ("width", 16)),
}

BETA_ROLLED = re.compile(r"\[dsq\] fit_beta_rolled p=(\d+) m=(\d+): slab in (LDS|global) ?(?:memory)?,(?: lds=\d+,)? (\d+) waves per gene")
BETA_WIDTH = re.compile(r"\[dsq\] (fit_beta_cells|fit_beta)<P=(\d+)>")
DISP_ROLLED = re.compile(r"\[dsq\] fit_disp_rolled p=(\d+) m=(\d+) mode=(\d): lds=\d+, (\d+) waves per gene")
DISP_WIDTH = re.compile(r"\[dsq\] fit_disp<P=(\d+),mode=(\d)>")


def _build_width(p):
    """the width of the library build a design of p columns runs on (zero-padded; csrc/capi.hip, "wide designs")"""
    return next(P for P in (16, 24, 32, 48, 64) if p <= P)


def assert_variant(name, d, err):
    """the launch lines of one run of the case against VARIANT.

    fitBeta.  Every call prints one fit_beta_rolled line at the build width P when it sizes its scratch
    (fit_beta_scratch_doubles), whichever kernel then runs.  launch_fit_beta_rolled prints a second one at P, and a third at the
    design's own width p < P, at which it launches when the slab then fits the LDS (csrc/fit_beta_wide.hip); fit_beta_cells<P>
    prints no rolled line, and its own only when its geometry changes -- it may be missing after an earlier test with the same
    geometry.  So the lines at P count 2 per rolled call and 1 per call on cells, the geometry of a rolled launch is the last
    line at its p, and a per-width line, where there is one, names fit_beta_cells<P>.
    fitDisp.  The rolled launches print their line every time, the per-width ones when their geometry changes."""
    beta, disp = VARIANT[name]
    m = d["counts"].shape[1]
    widths = [d["x"].shape[1]] + ([d["x_expanded"].shape[1]] if "x_expanded" in d else [])
    assert len(beta) == len(widths)
    P = _build_width(widths[0])
    assert all(_build_width(p) == P for p in widths)
    lines_b = [(int(p), ("rolled", int(nw), slab)) for p, mm, slab, nw in BETA_ROLLED.findall(err) if int(mm) == m]
    at_P = sum(1 for p, _ in lines_b if p == P)
    assert at_P == sum(2 if w[0] == "rolled" else 1 for w in beta), "%s: %d fit_beta_rolled lines at the build width %d\n%s" % (
        name, at_P, P, err)
    width_b = {(k, int(Pw)) for k, Pw in BETA_WIDTH.findall(err)}
    for p, want in zip(widths, beta):
        if want[0] == "rolled":
            last = [g for q, g in lines_b if q == p][-1]
            assert last == want, "%s: fitBeta at p = %d ran %r, not %r\n%s" % (name, p, last, want, err)
        else:
            assert _build_width(p) == want[1]
            assert p == P or not [g for q, g in lines_b if q == p], "%s: a rolled fitBeta launch at p = %d\n%s" % (name, p, err)
    assert width_b <= {("fit_beta_cells", w[1]) for w in beta if w[0] == "cells"}, "%s: fitBeta launches %r\n%s" % (name, width_b, err)
    rolled_d = {}
    for p, mm, mode, nw in DISP_ROLLED.findall(err):
        assert (int(p), int(mm)) == (widths[0], m), err
        rolled_d.setdefault(int(mode), set()).add(int(nw))
    width_d = {int(P) for P, _ in DISP_WIDTH.findall(err)}
    if disp[0] == "rolled":
        want = {mode: {nw} for mode, nw in zip((0, 2, 1), disp[1:]) if nw is not None}
        assert rolled_d == want, "%s: rolled fitDisp launches (mode -> waves per gene) %r, not %r\n%s" % (name, rolled_d, want, err)
        assert not width_d, "%s: a per-width fitDisp launch\n%s" % (name, err)
    else:
        assert not rolled_d, "%s: fitDisp ran the rolled kernel, not fit_disp<%d>\n%s" % (name, disp[1], err)
        assert width_d <= {disp[1]}, "%s: fitDisp launches fit_disp<%r>\n%s" % (name, width_d, err)


def test_every_wide_case_names_its_variant():
    kinds = RC.kinds()
    assert set(VARIANT) == {n for n, k in kinds.items() if k in ("wide", "expanded")} | set(RC.wide_cases.FLOOR)


@pytest.mark.parametrize("name", list(RC.kinds()))
def test_hip_reproduces_recorded_reference(monkeypatch, capfd, name):
    """the HIP path on a recorded case: compare() / assert_visible_parity() against the reference's recorded outputs, and, for
    the designs of 11 to 64 columns, the kernel variant the launch took"""
    d, ref = RC.build(name), RC.load(name)
    monkeypatch.setenv("DSQ_VERBOSE", "1")
    capfd.readouterr()
    got = RC.run(native, name, d)
    err = capfd.readouterr().err
    monkeypatch.delenv("DSQ_VERBOSE")
    print("\n".join(line for line in err.splitlines() if line.startswith("[dsq] fit_")))
    RC.check(got, ref, name, d, "hip " + name)
    if name in VARIANT:
        assert_variant(name, d, err)


@pytest.mark.skipif(not reference.available(), reason=reference.why_not() or "-")
@pytest.mark.parametrize("n,m,design,seed,kw", [
    (300, 50, "batch_condition", 7301, {}),
    (200, 120, ("factor", 8), 7302, {}),
    (200, 30, "two_group", 7303, {"weights": True}),
    (100, 64, "batch_condition", 7304, {"weights": True, "zero_w": True, "useQR": False}),
])
def test_hip_vs_reference_live(n, m, design, seed, kw):
    """inputs that are not recorded, the reference build running on the host beside the device"""
    d = T._case(n, m, design, seed=seed, **kw)
    T.compare(T.run_all(native, d), T.run_all(reference, d), d, "live %dx%d" % (n, m))
