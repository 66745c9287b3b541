#!/usr/bin/env python
"""Write tests/golden/reference/<case>.npz: the outputs of the REFERENCE'S OWN src/DESeq2.cpp, compiled by oracle/Makefile
(target `ref`) against the stand-in headers of oracle/shim/, on the seeded cases of tests/reference_cases.py -- the six
narrow golden cases, every case of wide_cases.WIDE / EXPANDED / FLOOR and the floor regime at seeds 5, 6, 7.

    make -C oracle ref && python tests/golden/make_reference_golden.py [case ...]

A one-off of a few minutes on the CPU, no part of any test; it needs oracle/_ref/libdeseq2_ref.so (made where the reference
tree exists).  Only outputs are stored -- the inputs are rebuilt from their seeds -- and of the matrices (beta_mat,
beta_var_mat, hat_diagonals) the first G_HEAD = 16 genes; see tests/reference_cases.py.
tests/test_oracle_vs_reference.py::test_fixture_is_current fails when a file no longer is what this script writes."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference                       # noqa: E402
from tests import reference_cases as RC            # noqa: E402


def main(names):
    if not reference.available():
        sys.exit(reference.why_not())
    os.makedirs(RC.DIR, exist_ok=True)
    total_bytes, t_all = 0, time.time()
    for name in names:
        d = RC.build(name)
        t0 = time.time()
        res = RC.run(reference, name, d)
        dt = time.time() - t0
        np.savez_compressed(RC.path(name), **RC.pack(name, res))
        size = os.path.getsize(RC.path(name))
        assert size <= RC.MAX_FILE_BYTES, "%s: %d bytes" % (name, size)
        total_bytes += size
        print("%-28s %4d x %-4d p=%-2d  reference %6.1f s  %7d bytes" % (
            name, d["counts"].shape[0], d["counts"].shape[1], d["x"].shape[1], dt, size), flush=True)
    print("%d files, %d bytes, %.0f s" % (len(names), total_bytes, time.time() - t_all))


if __name__ == "__main__":
    main(sys.argv[1:] or list(RC.kinds()))
