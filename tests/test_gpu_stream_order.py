"""-m gpu: the stream-order contract of the `_dev` entry points (include/deseq2_mi355x.h: "asynchronous on `stream`, no host
synchronisation") on a stream that is HELD busy, with inputs that arrive late and buffers that are recycled early
(tests/stream_hold.py says how; tests/stream_cases.py holds the cases, tests/test_stream_cases_cpu.py their conditions).

Every other GPU test calls on an idle stream with finished inputs, or on the null stream, and synchronises before it looks:
a launch, memset or copy that goes to the wrong stream, a fork that does not wait for the caller's stream or is not joined
back, a host synchronisation inside an entry that promises none, and a host table whose copy is still pending when its source
is rewritten all pass there.  Here each shows by value.  Per case, in this order:

  * a plain call on the same non-default stream S, synchronised (the warm-up: the slots of (device, S) grown, code objects
    loaded, torch's allocator holding the blocks of S), its host time taken;
  * the held call: hold S, true inputs copied in behind the hold, the call, `held` still pending when it returned (else
    INCONCLUSIVE: a failure), outputs cloned, inputs overwritten with the decoy and outputs / workspaces with 0xFF on S, then
    the first synchronisation;
  * the snapshot against what the entry's own GPU test compares with -- the oracle, the numpy specification, or the
    line-cited mirror -- bit for bit.  Never against another run of the library.

Then: two or three calls of one entry behind ONE hold with different host tables; the same entry on a held stream and on an
idle one at the same time; the evaluation of a resident local-fit handle; the whole DESeq chain with its fork to the side
stream; and the control -- a call issued on the WRONG stream must be seen.
"""
from collections import OrderedDict

import numpy as np
import pytest

from tests import stream_cases as SC
from tests import stream_hold as SH
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class _Rig:
    def __init__(self):
        import torch
        self.holder = SH.Holder(DEV)
        self.S = torch.cuda.Stream(device=DEV)          # the stream that is held
        self.B = torch.cuda.Stream(device=DEV)          # the idle one of the two-stream and control cases
        self.report = []


@pytest.fixture(scope="module")
def rig():
    r = _Rig()
    yield r
    h = r.holder
    print("\n[stream_order] hold operation: %s, %.3g ms per unit; %d holds, the shortest %.1f ms; largest host time of a warm-up call "
          "%.3f ms, of a call under a hold %.3f ms" % ("torch.cuda._sleep" if h.sleep else "8192^2 float32 matmul", h.unit_ms, h.holds,
                                                        h.min_hold_ms or 0.0, h.max_host_s * 1e3, h.max_issue_s * 1e3))
    for line in r.report:
        print("[stream_order] " + line)


def _lates(case):
    t, u = case.data(0)["in"], case.data(1)["in"]
    return OrderedDict((k, SH.Late(t[k].a, u[k].a, DEV, m=t[k].m)) for k in t)


def _step(case, lates=None):
    import torch
    lates = _lates(case) if lates is None else lates
    d = case.data(0)
    h = {k: l.handle for k, l in lates.items()}
    scratch = []
    if case.workspace is not None:
        h["ws"] = torch.empty(int(case.workspace(d)), dtype=torch.uint8, device=DEV)       # exactly its _workspace_bytes
        scratch.append(h["ws"])
    return SH.Step(lates.values(), lambda: case.call(h, d), scratch, what=case.name)


def _check(case, snap, oracle, what):
    want = case.expected(oracle)
    got = case.got(snap, case.data(0))
    assert sorted(got) == sorted(want), what
    for k in sorted(want):
        assert_same(np.asarray(got[k]), np.asarray(want[k]), "%s: %s" % (what, k))


def _recycled(steps, what):
    """after the run every input buffer holds its decoy again: nothing of the call wrote it, nothing ran behind the recycling"""
    import torch
    for s in steps:
        for l in s.lates:
            assert torch.equal(l.buf.view(torch.uint8), l.decoy.view(torch.uint8)), what + ": an input buffer is not its decoy"


def _note(rig, what, info):
    rig.report.append("%-34s hold %6.1f ms, host time of the call(s) %s ms, held pending after: %s"
                      % (what, info["hold_ms"], " / ".join("%.3f" % (1e3 * v) for v in info["issue_s"]), info["pending"]))


def _conclusive(info, what):
    assert all(info["pending"]), ("%s: INCONCLUSIVE -- the hold of %.1f ms had run out after a call (host times %s ms)"
                                  % (what, info["hold_ms"], ["%.3f" % (1e3 * v) for v in info["issue_s"]]))


# ---- the chain: counts, size factors and the design arrive late; the outlier refit forks to the side stream and joins ---------
# (first in the file: its call has by far the longest host time, so every later hold is sized by it)
def test_deseq_chain_on_a_held_stream(rig, oracle):
    import time
    import torch
    from deseq2_amd import core, fused
    from deseq2_amd.engine import DeviceEngine
    E = DeviceEngine(DEV)
    counts, x, sf = SC.chain_inputs(0)
    dcounts, dx, dsf = SC.chain_inputs(1)
    want = SC.chain_reference(oracle, counts, x, sf)

    def compare(b, what):
        assert b.attrs.get("fused") and b.attrs["status"]["N_REFIT"] >= 3, (what, b.attrs.get("status"))      # the fork really ran
        for k in sorted(want):
            got = b.dispersionFunction["coefficients"] if k == "trend" else b.mcols[k]
            assert_same(np.asarray(got, dtype=np.float64), want[k], "%s: %s" % (what, k))

    for timed in (False, True):                          # (the first pass loads, grows and caches; the second is timed)
        with torch.cuda.stream(rig.S):
            b = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
            assert fused.supported(b)
            t0 = time.perf_counter()
            fused.DESeq(b, wait=False)
            if timed:
                rig.holder.note_host_time(time.perf_counter() - t0)
            fused.finish(b)
        rig.S.synchronize()
        compare(b, "chain, warm-up")
        del b
    with torch.cuda.stream(rig.S):
        b = core.DESeqDataSet(counts, x, sizeFactors=sf, engine=E)
    torch.cuda.synchronize()
    sf_dev = E._cache[("sf", np.ascontiguousarray(sf, np.float64).tobytes())]              # the resident m-vector the chain reads
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    lates = [SH.Late.around(b.y.t, up(SC.In.gm(dcounts.astype(np.int32)).a)), SH.Late.around(b.xh, up(dx.T)),
             SH.Late.around(sf_dev, up(dsf))]
    # (no output is poisoned here: the result block is read by the copy that finish() enqueues behind the chain)
    step = SH.Step(lates, lambda: fused.DESeq(b, wait=False) and None, what="dsq_deseq_dev")
    try:
        _, info = SH.held(rig.holder, rig.S, [step], sync=False)
        with torch.cuda.stream(rig.S):
            fused.finish(b)
        rig.S.synchronize()
        _note(rig, "dsq_deseq_dev (fused.DESeq, wait=False)", info)
        compare(b, "chain, held")
        _recycled([step], "chain")
        _conclusive(info, "dsq_deseq_dev")
    finally:
        torch.cuda.synchronize()
        for l in lates:                                  # (the design and the size factors are memoised by the engine)
            l.buf.copy_(l.true)
        torch.cuda.synchronize()


# ---- every entry, one case per host-side path -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_entry_on_a_held_stream(rig, oracle, case):
    step = _step(case)
    warm = SH.plain(rig.holder, rig.S, [step])
    _check(case, warm[0], oracle, case.name + ", warm-up")
    snaps, info = SH.held(rig.holder, rig.S, [step], expect_async=case.exempt is None)
    _note(rig, case.name + (" (exempt: %s)" % case.exempt if case.exempt else ""), info)
    _check(case, snaps[0], oracle, case.name + ", held")
    _recycled([step], case.name)
    if case.exempt is None:
        _conclusive(info, case.name)
    else:
        assert case.exempt in SC.EXEMPT


def test_local_fit_evaluates_a_resident_handle(rig, oracle):
    """dsq_local_fit_dev: the fit (the case above), then the evaluation from the resident handle in a second held call -- the
    handle and the evaluation points arrive late; the decoy handle is the fit of the decoy inputs (N, k and the order in range)"""
    import torch
    from deseq2_amd import native
    case = SC.BY_NAME["local_fit"]
    blocks = []
    for which in (0, 1):
        a = case.arrays(which)
        up = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=DEV)
        r = native.local_fit_dev(up(a["means"]), up(a["disps"]), case.data(0)["minDisp"], evaluate=False)
        torch.cuda.synchronize()
        blocks.append(r["fit"].cpu().numpy())
    ins = case.data(0)["in"], case.data(1)["in"]
    lates = OrderedDict(fit=SH.Late(blocks[0], blocks[1], DEV), q=SH.Late(ins[0]["q"].a, ins[1]["q"].a, DEV))
    fn = lambda: native.local_fit_dev(fit=lates["fit"].buf, eval_means=lates["q"].buf, minDisp=case.data(0)["minDisp"])
    step = SH.Step(lates.values(), lambda: {k: v for k, v in fn().items() if k != "fit"}, what="local_fit, resident handle")
    want = case.expected(oracle)
    for name, run in (("warm-up", lambda: (SH.plain(rig.holder, rig.S, [step]), None)), ("held", lambda: SH.held(rig.holder, rig.S, [step]))):
        snaps, info = run()
        assert_same(snaps[0]["dispFit"].cpu().numpy(), want["dispFit"], "resident handle, %s: dispFit" % name)
        assert_same(snaps[0]["status"].cpu().numpy(), want["status"], "resident handle, %s: status" % name)
    _note(rig, "local_fit, resident handle", info)
    _conclusive(info, "local_fit, resident handle")
    _recycled([step], "local_fit, resident handle")


# ---- back to back behind one hold: different host tables, different data ----------------------------------------------------
BACK_TO_BACK = {"cooks_distance": "AB", "replace_outliers": "AB", "fit_beta-cells-p3": "ABA", "contrasts": "AB"}


@pytest.mark.parametrize("name", sorted(BACK_TO_BACK))
def test_back_to_back_behind_one_hold(rig, oracle, name):
    """two (fitBeta: three -- cells A, B, A; the warm-up ends on A, so the first held call takes the skip-if-unchanged branch
    of the table upload) calls of one entry: each host table is rewritten by the next call while the copy of the one before is
    still behind the hold.  At most four table uploads per hold (the pinned ring has eight buffers)."""
    cases = {"A": SC.BY_NAME[name], "B": SC.SECOND[name]}
    order = BACK_TO_BACK[name]
    steps = [_step(cases[k]) for k in order]
    warm = SH.plain(rig.holder, rig.S, steps)
    snaps, info = SH.held(rig.holder, rig.S, steps)
    _note(rig, "%s x %s" % (name, order), info)
    for i, k in enumerate(order):
        _check(cases[k], warm[i], oracle, "%s, call %d (%s), warm-up" % (name, i, k))
        _check(cases[k], snaps[i], oracle, "%s, call %d (%s) behind one hold" % (name, i, k))
    _recycled(steps, name)
    _conclusive(info, name)


# ---- two streams: what is shared across the per-(device, stream) contexts or kept in thread-local host buffers ------------------
@pytest.mark.parametrize("name", ["cooks_distance", "fit_beta-cells-p3", "results"])
def test_a_held_stream_and_an_idle_one(rig, oracle, name):
    """data set 1 on the held stream S, then data set 2 (another shape, other host tables) on the idle stream B: B's result is
    complete and right while S is still held; then S's"""
    import torch
    one, two = SC.BY_NAME[name], SC.SECOND[name]
    s1, s2 = _step(one), _step(two)
    SH.plain(rig.holder, rig.S, [s1])
    SH.plain(rig.holder, rig.B, [s2])
    for l in s2.lates:                                   # stream B: nothing late, nothing held
        l.buf.copy_(l.true)
    snaps1, info = SH.held(rig.holder, rig.S, [s1], sync=False)
    with torch.cuda.stream(rig.B):
        snap2 = SH.snapshot(s2.fn())
    rig.B.synchronize()
    still = not info["event"].query()
    _check(two, snap2, oracle, name + ": data set 2 on the idle stream")
    rig.S.synchronize()
    _note(rig, name + ", two streams", info)
    assert still, "%s: INCONCLUSIVE -- the held stream had drained before the idle stream's result was complete (hold %.1f ms)" % (name, info["hold_ms"])
    _check(one, snaps1[0], oracle, name + ": data set 1 on the held stream")
    _recycled([s1], name)
    _conclusive(info, name)


# ---- the control: the instrument sees a call on the wrong stream -------------------------------------------------------------
@pytest.mark.parametrize("name", ["pt", "fpm"])
def test_control_a_call_on_the_wrong_stream_is_seen(rig, oracle, name):
    """the true input arrives late on the held stream S, the call is issued on the idle stream B: it reads the decoy, and the
    result DIFFERS from the expected bits (it is the decoy's answer).  Elementwise kernels over valid decoys: nothing can go out
    of range.  No other control, and none that misorders anything carrying an index."""
    import torch
    case = SC.BY_NAME[name]
    step = _step(case)
    SH.plain(rig.holder, rig.B, [step])
    for l in step.lates:
        l.buf.copy_(l.decoy)
    torch.cuda.synchronize()
    ev, hold_ms = rig.holder.hold(rig.S)
    with torch.cuda.stream(rig.S):
        for l in step.lates:
            l.buf.copy_(l.true, non_blocking=True)
    with torch.cuda.stream(rig.B):
        snap = SH.snapshot(step.fn())
    rig.B.synchronize()
    still = not ev.query()
    rig.S.synchronize()
    assert still, "control %s: INCONCLUSIVE -- the hold of %.1f ms had run out before the misordered call was complete" % (name, hold_ms)
    got, want, stale = case.got(snap, case.data(0)), case.expected(oracle, 0), case.expected(oracle, 1)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        differ = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert differ.any(), "control %s: the misordered call was NOT seen in %s" % (name, k)
        assert_same(a, np.asarray(stale[k]), "control %s: %s is the decoy's answer" % (name, k))
    rig.report.append("control %-26s hold %6.1f ms: %d of %d elements differ from the expected bits"
                      % (name, hold_ms, int(differ.sum()), differ.size))


def test_zz_the_hold_was_long_enough(rig):
    """every hold of this file against the largest host time of a call in it (warm-up calls and calls under a hold)"""
    h = rig.holder
    assert h.holds > 0 and h.min_hold_ms >= SH.BASE_MS
    rig.report.append("margin: shortest hold %.1f ms; largest host time %.3f ms (warm-up) / %.3f ms (under a hold)"
                      % (h.min_hold_ms, h.max_host_s * 1e3, h.max_issue_s * 1e3))
    assert h.max_host_s > 0.0 and h.min_hold_ms >= SH.MARGIN * h.max_host_s * 1e3, (h.min_hold_ms, h.max_host_s)
