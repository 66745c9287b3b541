#!/usr/bin/env python
"""Measured agreement rates against the LAPACK restatement (oracle/lapack_oracle.py): `python tools/parity_report.py hip`
on the GPU box (HIP path through the host-pointer C ABI), `python tools/parity_report.py oracle` anywhere (the C oracle).
A second argument `wide` reports the designs of 11 to 64 columns (tests/wide_cases.py) instead: the cases, the expanded
prior designs and the wide floor cases (profiles/wide_parity.md); with DSQ_VERBOSE=1 the launch lines of the HIP path
precede each row on stderr.

A second argument `reference` changes the comparison target to the reference build (oracle/_ref: the reference's own
src/DESeq2.cpp over stand-in linear algebra and binary128 special functions) on every recorded case of
tests/reference_cases.py: `python tools/parity_report.py <oracle|lapack|hip> reference` against the recorded outputs
(tests/golden/reference/), `... reference live` against the library itself.  A case that misses a budget is printed with the
assertion's text instead of ending the report (profiles/reference_parity.md)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tests.test_oracle_vs_lapack as T   # noqa: E402
from oracle import lapack_oracle          # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "oracle"
wide = len(sys.argv) > 2 and sys.argv[2] == "wide"
if which == "hip":
    from deseq2_amd import native as F
elif which == "lapack":
    F = lapack_oracle
else:
    from oracle import oracle as F


def row(name, d, st, prior="-"):
    n, m = d["counts"].shape
    fb = st["fitBeta"]
    return "| %s | %d x %d, p=%d | %d / %d | %.3f | %s | %.3f / %.3f | %d / %d | %.1e / %.1e | %.3f |" % (
        name, n, m, d["x"].shape[1], fb["iter_mismatch"], fb["n"], fb["converged"], prior,
        st["fitDispMLE"]["well"], st["fitDispMAP"]["well"], st["fitDispMLE"]["ties"], st["fitDispMAP"]["ties"],
        st["fitDispMLE"]["max_rel_log_alpha"], st["fitDispMAP"]["max_rel_log_alpha"], st["fitDispGrid"]["same"])


FLOOR_HEAD = ("| floor case | shape | floor_start | beta_iter_mismatch | iter_equal_rest | conv_differs | refit_differs | "
              "map_conv_differs | dge_abs_max | beyond 1e-6 relative |\n|---|---|---|---|---|---|---|---|---|---|")


def floor_row(name, d, s):
    return "| %s | %d x %d, p=%d | %d | %d | %.3f | %d | %d | %d | %.1e | %d |" % (
        name, d["counts"].shape[0], d["counts"].shape[1], d["x"].shape[1], s["floor_start"], s["beta_iter_mismatch"],
        s["iter_equal_rest"], s["conv_differs"], s["refit_differs"], s["map_conv_differs"], s["dge_abs_max"], s["dge_rel_gt_1e6"])


if len(sys.argv) > 2 and sys.argv[2] == "reference":
    from tests import reference_cases as RC   # noqa: E402
    live = len(sys.argv) > 3 and sys.argv[3] == "live"
    if live:
        from oracle import reference          # noqa: E402
        if not reference.available():
            sys.exit(reference.why_not())
    print("# Agreement of the %s path with the reference build, %s\n" % (
        which.upper(), "run live (oracle/_ref)" if live else "as recorded (tests/golden/reference/)"))
    print("Budgets asserted by the tests (compare(), unchanged): fitBeta$iter equal on every gene; fitDisp iter / iter_accept "
          "equal outside ulp-level ties, ties <= 1 %; well-conditioned share >= 0.9 (wide cases), 0.95 (narrow), 0.8 (m <= 12); "
          "grid agreement >= 0.95 (0.85 at m <= 12); values within 1e-7 (beta, log_alpha) / 1e-8 (lp, H, deviance).\n")
    print("| case | shape | fitBeta$iter mismatches | converged | betaPrior pass (iterations) | well (MLE / MAP) | ties (MLE / MAP) | max rel log alpha | grid same |")
    print("|---|---|---|---|---|---|---|---|---|")
    floors = []
    for name, kind in RC.kinds().items():
        d = RC.build(name)
        got = RC.run(F, name, d)
        ref = RC.run(reference, name, d) if live else RC.load(name)
        try:
            st = RC.check(got, ref, name, d, name, lapack=which == "lapack")
        except AssertionError as e:
            print("| %s | %d x %d, p=%d | MISSES: %s |" % (name, d["counts"].shape[0], d["counts"].shape[1], d["x"].shape[1],
                                                           " ".join(str(e).split())[:300]), flush=True)
            continue
        if kind == "floor":
            floors.append(floor_row(name, d, st))
            continue
        prior = "-"
        if "fitBetaPrior" in st:
            it = ref["fitBetaPrior"]["iter"]
            prior = "%d / %d (%d .. %d)" % (st["fitBetaPrior"]["iter_mismatch"], st["fitBetaPrior"]["n"], it.min(), it.max())
        print(row(name, d, st, prior), flush=True)
    print("\n" + FLOOR_HEAD)
    print("\n".join(floors))
    sys.exit(0)
print("# Agreement of the %s path with the LAPACK restatement (oracle/lapack_oracle.py)\n" % which.upper())
print("Budgets asserted by the tests: fitBeta$iter equal on every gene; fitDisp iter / iter_accept equal outside "
      "ulp-level ties, ties <= 1 %%; well-conditioned share >= %s; grid agreement >= 0.95; values within "
      "1e-7 (beta, log_alpha) / 1e-8 (lp, H, deviance).\n" % ("0.9 (wide cases)" if wide else "0.95 (m > 12)"))
print("| case | shape | fitBeta$iter mismatches | converged | betaPrior pass (iterations) | well (MLE / MAP) | ties (MLE / MAP) | max rel log alpha | grid same |")
print("|---|---|---|---|---|---|---|---|---|")
if wide:
    from tests import wide_cases as W     # noqa: E402
    cases = [(n, (lambda n=n: W.wide_case(n)), W.MIN_WELL) for n in W.WIDE]
    cases += [(n, (lambda n=n: W.expanded_case(n)), W.MIN_WELL) for n in W.EXPANDED]
else:
    cases = [(n, (lambda n=n: T.shape_case(n)), None) for n in T.SHAPE_NAMES]
    cases += [(n, (lambda d=d: d), None) for n, d in T.live_cases().items()]
for name, build, min_well in cases:
    d = build()
    got, ref = T.run_all(F, d), T.run_all(lapack_oracle, d)
    st = T.compare(got, ref, d, name, min_well=min_well)
    prior = "-"
    if "fitBetaPrior" in st:
        if wide:                          # the wide expanded designs are held at scale 1
            T._fit_beta_compare(got["fitBetaPrior"], ref["fitBetaPrior"], name, "fitBetaPrior", 1.0)
        it = ref["fitBetaPrior"]["iter"]
        prior = "%d / %d (%d .. %d)" % (st["fitBetaPrior"]["iter_mismatch"], st["fitBetaPrior"]["n"], it.min(), it.max())
    n, m = d["counts"].shape
    fb = st["fitBeta"]
    print("| %s | %d x %d, p=%d | %d / %d | %.3f | %s | %.3f / %.3f | %d / %d | %.1e / %.1e | %.3f |" % (
        name, n, m, d["x"].shape[1], fb["iter_mismatch"], fb["n"], fb["converged"], prior,
        st["fitDispMLE"]["well"], st["fitDispMAP"]["well"], st["fitDispMLE"]["ties"], st["fitDispMAP"]["ties"],
        st["fitDispMLE"]["max_rel_log_alpha"], st["fitDispMAP"]["max_rel_log_alpha"], st["fitDispGrid"]["same"]), flush=True)
if wide:
    from tests import floor_regime as FR  # noqa: E402
    print("\n" + FLOOR_HEAD)
    for name in W.FLOOR:
        d = W.floor_wide_case(name)
        s = FR.assert_visible_parity(FR.visible_chain(F, d), FR.visible_chain(lapack_oracle, d), name)
        print(floor_row(name, d, s), flush=True)
