"""-m gpu: the outlier phase in candidates-first order (csrc/pipeline.hip: phase_outlier_first) changes no bit.  The fused
chain runs each case in this process (DSQ_OUTLIER_FIRST unset: the new order where it applies) and is held, bit for bit --
every per-gene column, the status counters, the dispersion function, the assays mu / H / cooks / replaceCounts -- against
  * the call-by-call chain of core.py on the device engine (serial by construction), and
  * the same fused calls with DSQ_OUTLIER_FIRST=0, made by ONE fresh child process (the knob is read once per process).
Cases: the two shapes of tests/test_outlier_bound_cpu.py with planted outliers; no outlier at all (empty refit);
cooksCutoff = 0 (every row a candidate, nothing left for the bulk pass); cells of two samples (no row replaceable); a
continuous covariate (no design cells: no flag, the old order).
That the new order is really the one taken is observed too: under DSQ_VERBOSE the library says so on stderr, once per call
(a second child process; test_the_new_order_is_taken)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import outlier_first_cases as OC
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["two_group_28", "batch_condition_48", "no_outlier", "cutoff_zero", "cells_of_two", "continuous"]


def _inputs():
    return {**OC.chain_inputs(), **OC.variant_inputs()}


class _zero_cutoff:
    """qf(.99, p, m - p) = 0 for both chains (each evaluates scipy's F quantile where it needs the cutoff)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from scipy import stats
        from deseq2_amd import fused
        fused._FACTS.clear()
        if self.on:
            self.saved = stats.f.ppf
            stats.f.ppf = lambda *a, **k: 0.0

    def __exit__(self, *exc):
        from scipy import stats
        from deseq2_amd import fused
        if self.on:
            stats.f.ppf = self.saved
        fused._FACTS.clear()


def _run(E, c, which):
    from deseq2_amd import core, fused
    from tests.chain_cases import result_of
    with _zero_cutoff(bool(c.get("cutoff_zero"))):
        dds = core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], engine=E)
        if which == "fused":
            assert fused.supported(dds)
            fused.DESeq(dds)
            assert dds.attrs.get("fused")
        else:
            core.DESeq(dds)
        res = result_of(dds)
    res.pop("cooksCutoff", None)
    fn = res.pop("dispersionFunction")
    res["trend_coefficients"] = np.asarray(fn["coefficients"], np.float64)
    res["trend_scalars"] = np.array([fn["varLogDispEsts"], fn["dispPriorVar"]], np.float64)
    if which == "fused":
        st = dds.attrs["status"]
        res["status"] = np.array([float(st[k]) for k in sorted(st)], np.float64)
        res["status_N_REPLACE_N_REFIT"] = np.array([st["N_REPLACE"], st["N_REFIT"]], np.float64)
    nz = dds.attrs.get("nz_rows")
    res["nz_rows"] = np.arange(dds.n) if nz is None else np.asarray(nz)
    return {k: np.asarray(v, np.float64) for k, v in res.items() if not isinstance(v, dict)}


def _child(path):
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine("cuda:0")
    out = {}
    for name, c in _inputs().items():
        for k, v in _run(E, c, "fused").items():
            out[name + "/" + k] = v
    np.savez(path, **out)


def _child_verbose(names):
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine("cuda:0")
    ins = _inputs()
    for name in names:
        sys.stderr.write("CASE %s\n" % name)
        sys.stderr.flush()
        _run(E, ins[name], "fused")


def test_the_new_order_is_taken():
    names = ["two_group_28", "batch_condition_48", "cutoff_zero", "no_outlier", "cells_of_two", "continuous"]
    env = {k: v for k, v in os.environ.items() if k != "DSQ_OUTLIER_FIRST"}
    env.update(DSQ_VERBOSE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_outlier_first import _child_verbose; _child_verbose(%r)" % names],
                       cwd=ROOT, env=env, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    taken, case = {n: 0 for n in names}, None
    for line in r.stderr.splitlines():
        if line.startswith("CASE "):
            case = line[5:].strip()
        elif "outlier phase: candidates first" in line and case:
            taken[case] += 1
    # one call each; cells of two samples have nothing replaceable and a continuous covariate has no design cells: serial order
    assert taken == {"two_group_28": 1, "batch_condition_48": 1, "cutoff_zero": 1, "no_outlier": 1, "cells_of_two": 0, "continuous": 0}, taken


@pytest.fixture(scope="module")
def E():
    from deseq2_amd.engine import DeviceEngine
    return DeviceEngine("cuda:0")


@pytest.fixture(scope="module")
def old_order(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("outlier_first") / "old_order.npz")
    env = dict(os.environ, DSQ_OUTLIER_FIRST="0")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_outlier_first import _child; _child(%r)" % path],
                       cwd=ROOT, env=env, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def new_order(E):
    assert os.environ.get("DSQ_OUTLIER_FIRST", "1") != "0", "this process is to run the new order"
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(E, _inputs()[name], "fused")
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_the_old_order(new_order, old_order, name):
    new = new_order(name)
    keys = [k[len(name) + 1:] for k in old_order if k.startswith(name + "/")]
    assert sorted(keys) == sorted(new), (sorted(keys), sorted(new))
    for k in keys:
        assert_same(new[k], old_order[name + "/" + k], "%s: %s against DSQ_OUTLIER_FIRST=0" % (name, k))


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_the_call_by_call_chain(E, new_order, name):
    new = new_order(name)
    ref = _run(E, _inputs()[name], "core")
    nz = new["nz_rows"].astype(int)
    assert (ref["nz_rows"] == new["nz_rows"]).all()
    rep = np.nan_to_num(ref["replace"]).astype(bool)
    for k, v in ref.items():
        if k == "nz_rows":
            continue
        a, b = v, new[k]
        if k in ("mu", "H", "cooks"):                  # (the call-by-call chain keeps the assays of the non-zero rows)
            a, b = a[nz], b[nz]
        elif k == "replaceCounts":                     # (... and replacement counts that matter at the replaced rows)
            a, b = a[rep], b[rep]
        assert_same(a, b, "%s: %s against the call-by-call chain" % (name, k))
    if name in ("two_group_28", "batch_condition_48"):
        assert new["status_N_REPLACE_N_REFIT"][0] >= 4 and new["status_N_REPLACE_N_REFIT"][1] >= 3
        assert new["status_N_REPLACE_N_REFIT"][0] == rep.sum()
    if name == "no_outlier":
        assert new["status_N_REPLACE_N_REFIT"][0] == 0
    if name == "cutoff_zero":            # (the cutoff really is 0: every row with a non-zero distance is replaced)
        assert new["status_N_REPLACE_N_REFIT"][0] >= 0.9 * len(nz), (new["status_N_REPLACE_N_REFIT"], len(nz))
        assert new["status_N_REPLACE_N_REFIT"][0] > 10 * new_order("two_group_28")["status_N_REPLACE_N_REFIT"][0]
