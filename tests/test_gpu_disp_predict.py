"""-m gpu: the evaluator policy of the fitDisp line search (csrc/fit_disp.hip, DSQ_DISP_PREDICT) changes no bit.
Policy 0 evaluates log_posterior and dlog_posterior fused at every proposal, policy 1 (the default but for one gated shape)
the likelihood alone where it predicts a rejection, policy 2 the likelihood alone at every proposal -- with a fused
evaluation at the same point after every acceptance that continues, so 2 drives every accepted proposal through the
fallback that 1 takes on a misprediction.
The knob is read once per process: ONE fresh child process per policy makes every call of this file.  Every case asserts
  * the eight outputs of the search bit-equal under policies 0, 1 and 2, and
  * bit-equal to the oracle's fitDisp.
Shapes (the smallest that reach each path of the per-width kernel):
  p2_m8       p = 2, 8 samples: distinct counts by register sort, no cells
  p4_m48      ~ batch + condition, 48 samples: design cells, parked closes, LaneLU
  p4_m300     the same design, 300 samples: distinct counts by histogram (from 256 samples)
  p4_m48_w    48 samples with weights, one sample's weights zero in every row (USE_W)
  p3_cont_m40 a factor and one continuous covariate, 40 samples: the general mode, no cells
each with and without the prior and with and without the Cox-Reid term.  Starts:
  rough       the usual rough start: the long run of rejections at the head of the search
  converged   the log alpha a previous call converged to: the first proposal is accepted or ends the search (the fallback and
              the exits that compute no derivative, under policy 1: last_dlp)
  far         -35 and +12, inside the accepted [-40, 40] and outside the proposals' [-30, 10]: kappa re-derived from the bound
  maxit3      the search stops inside the run of rejections
  nonfinite   one row with a mu-hat of 1e150 (mu_ok false), one all-zero row and one row with a mu-hat of 1e308, whose lp is
              not finite at the proposals above log alpha = 0.6: kstar has to survive it
  floor       min_log_alpha above every start: the a < min_log_alpha exit at the first acceptance
One chain-level case: fused.DESeq on ~ batch + condition, 300 x 48, every per-gene column under policies 0 and 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import assert_bits, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("log_alpha", "iter", "iter_accept", "last_change", "initial_lp", "initial_dlp", "last_lp", "last_dlp")
SHAPES = {"p2_m8": (96, 8, "two_group", False), "p4_m48": (128, 48, "batch_condition", False),
          "p4_m300": (64, 300, "batch_condition", False), "p4_m48_w": (128, 48, "batch_condition", True),
          "p3_cont_m40": (96, 40, ("factor_cont", 2), False)}
STARTS = ("rough", "converged", "far", "maxit3", "nonfinite", "floor")
CASES = ["%s-%s-%s" % (s, pr, cr) for s in SHAPES for pr in ("prior", "noprior") for cr in ("cr", "nocr")]
POLICIES = ("0", "1", "2")
MIN_LA = np.log(1e-8 / 10)


def _oracle():
    from oracle import oracle
    return oracle


def _shape_inputs(shape):
    n, m, design, useW = SHAPES[shape]
    d = make_case(n, m, design, seed=8, weights=useW, sf_random=True)
    x = d["x"]; p = x.shape[1]
    w = np.maximum(d["weights"], 1e-6)                                     # R/core.R:702
    if useW:
        w[:, 5] = 0.0
    lam = np.full(p, 1e-6) / np.log(2) ** 2
    fb = _oracle().fitBeta(d["counts"], x, d["nf"], d["alpha_init"], np.r_[1.0, np.zeros(p - 1)], d["beta_init"], lam, w, useW,
                           1e-8, 100, True, 0.5)
    mu = np.maximum(d["nf"] * np.exp(fb["beta_mat"] @ x.T), 0.5)
    return d["counts"], x, mu, w, useW, np.log(d["alpha_init"])


def _case_args(case, inputs, converged=None):
    """start -> the fifteen arguments of fitDisp; `converged` = the log alpha of the rough start's call (None: left out)"""
    shape, pr, cr = case.split("-")
    y, x, mu, w, useW, la0 = inputs[shape]
    usePrior, useCR = pr == "prior", cr == "cr"
    pm = la0 + 0.3 if usePrior else la0
    sig = 0.7 if usePrior else 1.0

    def args(y=y, mu=mu, la=la0, min_la=MIN_LA, maxit=100):
        return (y, x, mu, la, pm, sig, min_la, 1.0, 1e-6, maxit, usePrior, w, useW, 1e-2, useCR)
    out = {"rough": args()}
    if converged is not None:
        out["converged"] = args(la=converged)
    far = np.where(np.arange(len(la0)) % 2 == 0, -35.0, 12.0)
    out["far"] = args(la=far)
    out["maxit3"] = args(maxit=3)
    y2 = y.copy(); mu2 = mu.copy()
    mu2[0, 1] = 1e150
    y2[1] = 0
    mu2[2, 1] = 1e308                      # (1 + mu alpha overflows from log alpha = 0.6: lp is not finite there)
    out["nonfinite"] = args(y=y2, mu=mu2)
    out["floor"] = args(min_la=11.0)
    return out


def _all_inputs():
    return {s: _shape_inputs(s) for s in SHAPES}


def _chain(E):
    """fused.DESeq on the 300 x 48 ~ batch + condition input of tests/outlier_first_cases.py -> its per-gene columns and assays"""
    from deseq2_amd import core, fused
    from tests import outlier_first_cases as OC
    from tests.chain_cases import result_of
    c = OC.chain_inputs()["batch_condition_48"]
    fused._FACTS.clear()
    dds = core.DESeqDataSet(c["counts"], c["x"], sizeFactors=c["sizeFactors"], engine=E)
    assert fused.supported(dds)
    fused.DESeq(dds)
    assert dds.attrs.get("fused")
    return {k: np.asarray(v, np.float64) for k, v in result_of(dds).items() if isinstance(v, np.ndarray)}


def _child(path):
    """every call of this file under the policy of this process"""
    from deseq2_amd import native
    from deseq2_amd.engine import DeviceEngine
    inputs = _all_inputs()
    out = {}
    for case in CASES:
        rough = native.fitDisp(*_case_args(case, inputs)["rough"])
        for start, a in _case_args(case, inputs, rough["log_alpha"]).items():
            r = rough if start == "rough" else native.fitDisp(*a)
            for k in KEYS:
                out["%s/%s/%s" % (case, start, k)] = np.asarray(r[k], np.float64)
    for k, v in _chain(DeviceEngine("cuda:0")).items():
        out["chain/" + k] = v
    np.savez(path, **out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """policy -> the child's arrays; each child says on stderr (DSQ_VERBOSE) which policy its launches carried"""
    d = tmp_path_factory.mktemp("disp_predict")
    out = {}
    for pol in POLICIES:
        path = str(d / ("policy_%s.npz" % pol))
        env = {k: v for k, v in os.environ.items() if k not in ("DSQ_DISP_PREDICT", "DSQ_FORCE_ITERS", "DSQ_VERBOSE")}
        env.update(DSQ_DISP_PREDICT=pol, DSQ_VERBOSE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_disp_predict import _child; _child(%r)" % path],
                           cwd=ROOT, env=env, timeout=240, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        said = [ln for ln in r.stderr.splitlines() if "fit_disp<P=" in ln and "mode=0" in ln]
        assert said and all(ln.rstrip().endswith("predict=%s" % pol) for ln in said), said[:3]
        out[pol] = dict(np.load(path))
    return out


@pytest.fixture(scope="module")
def inputs():
    return _all_inputs()


def _child_default():
    """no knob set: five calls, a marker on stderr in front of each"""
    from deseq2_amd import native

    def call(tag, m, p, useW):
        sys.stderr.write("CALL %s\n" % tag)
        sys.stderr.flush()
        x = np.column_stack([np.ones(m), np.arange(m) % 2.0, (np.arange(m) // 2) % 2.0, (np.arange(m) // 4) % 2.0])[:, :p]
        native.fitDisp(np.full((4, m), 3), x, np.full((4, m), 3.0), np.zeros(4), np.zeros(4), 1.0, -20.0, 1.0, 1e-6, 100, False,
                       np.ones((4, m)), useW, 1e-2, True)
    call("p2_short", 100, 2, False)
    call("p2_short_weights", 99, 2, True)
    call("p2_longer", 101, 2, False)
    call("p1_short", 98, 1, False)
    call("p4_short", 48, 4, False)


def test_default_policy_by_shape():
    """no knob set: policy 1, but policy 0 for unweighted rows of a two-column design with up to 100 samples (the gate of
    launch_disp_p: the one shape measured to lose under policy 1)"""
    env = {k: v for k, v in os.environ.items() if k not in ("DSQ_DISP_PREDICT", "DSQ_FORCE_ITERS", "DSQ_VERBOSE")}
    env.update(DSQ_VERBOSE="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_disp_predict import _child_default; _child_default()"],
                       cwd=ROOT, env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    said, tag = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("CALL "):
            tag = ln[5:].strip()
        elif "fit_disp<P=" in ln and "mode=0" in ln and tag:
            said.setdefault(tag, []).append(ln.rstrip().rsplit("predict=", 1)[1])
    assert said == {"p2_short": ["0"], "p2_short_weights": ["1"], "p2_longer": ["1"], "p1_short": ["1"], "p4_short": ["1"]}, said


@pytest.mark.parametrize("case", CASES)
def test_same_bits_under_every_policy_and_as_the_oracle(runs, inputs, case):
    O = _oracle()
    rough = O.fitDisp(*_case_args(case, inputs)["rough"])
    for start, a in _case_args(case, inputs, rough["log_alpha"]).items():
        want = rough if start == "rough" else O.fitDisp(*a)
        for k in KEYS:
            name = "%s/%s/%s" % (case, start, k)
            for pol in ("1", "2"):
                assert_bits(runs[pol][name], runs["0"][name], "%s: policy %s against policy 0" % (name, pol))
            assert_bits(runs["0"][name], np.asarray(want[k], np.float64), "%s against the oracle" % name)
        # the start does what it is there for
        it, acc = np.asarray(want["iter"]), np.asarray(want["iter_accept"])
        if start == "rough":
            assert (it > acc).any()
        elif start == "converged":
            assert (acc >= 1).mean() > 0.9, "the first proposal accepted in nearly every row"
        elif start == "maxit3":
            assert (it == 3).mean() > 0.9 and (acc < 3).any()
        elif start == "floor":
            assert ((acc == 1) | (it == 100)).all() and (acc == 1).mean() > 0.5
        elif start == "far":
            assert np.isfinite(want["log_alpha"]).all()


def test_chain_same_bits_under_policies_0_and_1(runs):
    keys = sorted(k for k in runs["0"] if k.startswith("chain/"))
    assert len(keys) > 10 and keys == sorted(k for k in runs["1"] if k.startswith("chain/"))
    for k in keys:
        assert_bits(runs["1"][k], runs["0"][k], "%s: policy 1 against policy 0" % k)
