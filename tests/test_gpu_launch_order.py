"""-m gpu: the launch orders of the fused chain's full-size fit launches (csrc/pipeline.hip: lpt_scatter_kernel) change no
bit.  The fused chain runs each case in this process with the orders on (DSQ_LPT unset) and is held, bit for bit -- every
per-gene column, the status counters, the trend's scalars, the assays -- against
  * the same fused calls with DSQ_LPT=0, made by ONE fresh child process (the knobs are read once per process), and
  * the call-by-call chain of core.py on the device engine (which has no row lists at all).
The default keys order launches from 256 samples (below that an order recovers less than it costs), so with these small
inputs the process itself runs whatever the defaults order, and the same calls are also made by child processes that force
every launch into an order whatever the shape, one per key of the MAP search (FORCED: DSQ_LPT=2 and the keys), and held
against the DSQ_LPT=0 child in the same way.
Cases: the two 300-gene inputs of tests/outlier_first_cases.py; 1 500 genes x 28 samples, ~ batch + condition (six blocks of
the order's two passes, the last one partly filled) with all-zero rows and rows whose gene-wise IRLS runs to its 100
iterations; and 1, 63, 64 and 65 non-zero rows cut from that input (one wave of a block: empty but for one row, one short,
full, one over).
That the orders are really built is observed too: under DSQ_VERBOSE the library checks each list it has built on the host
and says so on stderr, one line per ordered launch (child processes: the default keys, every launch ordered, none)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import outlier_first_cases as OC
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = (1, 63, 64, 65)
CASES = ["two_group_28", "batch_condition_48", "wide_1500"] + ["edge_%d" % k for k in EDGE]
KNOBS = ("DSQ_LPT", "DSQ_LPT_MAXN", "DSQ_LPT_KEY1", "DSQ_LPT_KEYD", "DSQ_LPT_KEYM", "DSQ_LPT_KEY2")
LAUNCHES = ("gene-wise fit_beta", "gene-wise fit_disp", "MAP fit_disp", "test fit_beta")
# every launch in an order, whatever the shape: gene-wise search backwards through the list, no size limit for the MAP search,
# each of its four keys once, both keys of the test's fit
FORCED = {"mean_down": dict(DSQ_LPT="2", DSQ_LPT_KEYD="2", DSQ_LPT_MAXN="0", DSQ_LPT_KEYM="2", DSQ_LPT_KEY2="0"),
          "iterations": dict(DSQ_LPT="2", DSQ_LPT_KEYD="2", DSQ_LPT_MAXN="0", DSQ_LPT_KEYM="3", DSQ_LPT_KEY2="1"),
          "iterations_x_mean": dict(DSQ_LPT="2", DSQ_LPT_KEYD="2", DSQ_LPT_MAXN="0", DSQ_LPT_KEYM="5", DSQ_LPT_KEY2="0"),
          "distance": dict(DSQ_LPT="2", DSQ_LPT_KEYD="2", DSQ_LPT_MAXN="0", DSQ_LPT_KEYM="6", DSQ_LPT_KEY2="1")}


def default_ordered(c, lpt=1):
    """the launches the default keys order for this input (csrc/pipeline.hip, "launch orders, host half";
    profiles/launch_order.md says why): none below 256 samples unless DSQ_LPT=2; then the gene-wise fit_beta when the gene-wise
    means come from an IRLS (a design that is not one indicator per group), the gene-wise search for 256 .. 1024 samples, the
    MAP search up to 16 384 genes, the test's fit always"""
    x = c["x"]
    if x.shape[0] < 256 and lpt < 2:
        return []
    irls = len(np.unique(x, axis=0)) != x.shape[1]
    out = ["gene-wise fit_beta"] if irls else []
    if 256 <= x.shape[0] <= 1024:
        out.append("gene-wise fit_disp")
    if c["counts"].shape[0] <= 16384:
        out.append("MAP fit_disp")
    return out + ["test fit_beta"]


def wide_counts():
    """1 500 x 28, ~ batch + condition (p = 4, six cells): planted outliers, twenty all-zero rows, and rows with one condition at
    zero and the other at large, widely spread counts (SLOW_ROWS: the gene-wise IRLS of rows 7 and 700 is still moving after its
    100 iterations -- the oracle's fitBeta$iter on this input --, so the fit hands them to the optim fallback: N_OPTIM_GENEEST)"""
    x = OC.simulate.design_batch_condition(28)
    c, sf = OC._counts(1500, x, 31)
    c = OC.plant(c, 31)
    c[np.arange(40, 1500, 73)[:20]] = 0
    rng = np.random.default_rng(32)
    for r in SLOW_ROWS:
        c[r] = 0
        c[r, x[:, -1] == 1] = np.exp(rng.uniform(0.0, np.log(2.0e5), int((x[:, -1] == 1).sum()))).astype(c.dtype)
    return c, x, sf


SLOW_ROWS = (7, 700, 1499)


def _inputs():
    out = dict(OC.chain_inputs())
    c, x, sf = wide_counts()
    out["wide_1500"] = {"counts": c, "x": x, "sizeFactors": sf}
    nzr = np.flatnonzero(c.sum(axis=1) > 0)
    for k in EDGE:
        # the first k non-zero rows with the all-zero rows among them (the list is shorter than the matrix), row 7 included
        out["edge_%d" % k] = {"counts": c[: nzr[k - 1] + 1] if k > 1 else c[7:8], "x": x, "sizeFactors": sf}
    return out


def _run(E, c, which):
    from deseq2_amd import core, fused
    from tests.chain_cases import result_of
    fused._FACTS.clear()
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
    res["trend_fitType"] = np.array([float(len(str(fn["fitType"])))])
    res["trend_coefficients"] = np.atleast_1d(np.asarray(fn["coefficients"], np.float64))
    res["trend_scalars"] = np.array([fn["varLogDispEsts"], fn["dispPriorVar"]], np.float64)
    if which == "fused":
        st = dds.attrs["status"]
        res["status"] = np.array([float(st[k]) for k in sorted(st)], np.float64)
        res["status_N_OPTIM_GENEEST"] = np.array([st["N_OPTIM_GENEEST"]], np.float64)
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


def _env(**knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS and k != "DSQ_VERBOSE"}
    env.update(knobs)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")
    return env


def _lines(names, **knobs):
    """case -> the launches the library reports as ordered, in the chain's order"""
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_launch_order import _child_verbose; _child_verbose(%r)" % (names,)],
                       cwd=ROOT, env=_env(DSQ_VERBOSE="1", **knobs), timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    seen, case = {n: [] for n in names}, None
    for line in r.stderr.splitlines():
        if line.startswith("CASE "):
            case = line[5:].strip()
        elif "[dsq] launch order:" in line and case:
            assert line.rstrip().endswith("permutation ok"), line
            what = line.split("launch order:")[1].split(" by ")[0].strip()
            rows = int(line.split(",")[-2].split()[0])
            seen[case].append((what, rows))
    return seen


def test_default_keys_say_permutation_ok_for_every_ordered_launch():
    ins = _inputs()
    names = ["two_group_28", "batch_condition_48", "wide_1500", "edge_1"]
    seen = _lines(names)
    for n in names:
        nnz = int((ins[n]["counts"].sum(axis=1) > 0).sum())
        assert seen[n] == [(w, nnz) for w in LAUNCHES if w in default_ordered(ins[n])], (n, seen[n])
    # ... and the default keys whatever the row length
    seen = _lines(names, DSQ_LPT="2")
    for n in names:
        nnz = int((ins[n]["counts"].sum(axis=1) > 0).sum())
        assert seen[n] == [(w, nnz) for w in LAUNCHES if w in default_ordered(ins[n], 2)], (n, seen[n])
    assert "gene-wise fit_beta" in default_ordered(ins["wide_1500"], 2) and "gene-wise fit_beta" not in default_ordered(ins["two_group_28"], 2)


def test_every_launch_ordered_and_none():
    ins = _inputs()
    nnz = int((ins["wide_1500"]["counts"].sum(axis=1) > 0).sum())
    seen = _lines(["wide_1500"], **FORCED["iterations"])
    assert seen["wide_1500"] == [(w, nnz) for w in LAUNCHES], seen
    seen = _lines(["wide_1500"], DSQ_LPT_KEY1="0", DSQ_LPT_KEYD="0", DSQ_LPT_KEYM="0", DSQ_LPT_KEY2="2")
    assert seen["wide_1500"] == [], seen
    seen = _lines(["wide_1500"], DSQ_LPT="0")
    assert seen["wide_1500"] == [], seen


@pytest.fixture(scope="module")
def E():
    from deseq2_amd.engine import DeviceEngine
    return DeviceEngine("cuda:0")


@pytest.fixture(scope="module")
def list_order(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("launch_order") / "list_order.npz")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_launch_order import _child; _child(%r)" % path],
                       cwd=ROOT, env=_env(DSQ_LPT="0"), timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module", params=sorted(FORCED))
def forced(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("launch_order") / ("forced_%s.npz" % request.param))
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_launch_order import _child; _child(%r)" % path],
                       cwd=ROOT, env=_env(**FORCED[request.param]), timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(path))


def test_every_launch_ordered_same_bits_as_list_order(forced, list_order):
    assert sorted(forced) == sorted(list_order)
    for k in sorted(list_order):
        assert_same(forced[k], list_order[k], "%s: every launch ordered against DSQ_LPT=0" % k)


@pytest.fixture(scope="module")
def ordered(E):
    for k in KNOBS:
        assert k not in os.environ, "this process is to run the default launch orders (%s is set)" % k
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(E, _inputs()[name], "fused")
        return cache[name]
    return get


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_list_order(ordered, list_order, name):
    new = ordered(name)
    keys = [k[len(name) + 1:] for k in list_order if k.startswith(name + "/")]
    assert sorted(keys) == sorted(new), (sorted(keys), sorted(new))
    for k in keys:
        assert_same(new[k], list_order[name + "/" + k], "%s: %s against DSQ_LPT=0" % (name, k))


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_the_call_by_call_chain(E, ordered, name):
    new = ordered(name)
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
    c = _inputs()[name]["counts"]
    assert len(nz) == int((c.sum(axis=1) > 0).sum())
    if name == "wide_1500":
        assert len(nz) == 1480 and len(nz) % 256 != 0
        # rows whose gene-wise IRLS ran to maxit went to the optim fallback (7 and 700 at least)
        assert new["status_N_OPTIM_GENEEST"][0] >= 2, new["status_N_OPTIM_GENEEST"]
    if name.startswith("edge_"):
        assert len(nz) == int(name[5:])
