"""A held stream for the tests of the library's stream-order contract (tests/test_gpu_stream_order.py; the case table
is tests/stream_cases.py, held to its conditions on the CPU by tests/test_stream_cases_cpu.py).

Every `_dev` entry promises "asynchronous on `stream`, no host synchronisation" (include/deseq2_mi355x.h).  On an idle
stream with finished inputs, and on the null stream, a launch on the wrong stream, a fork that does not wait, a host
synchronisation or a host table whose copy is still pending when its source is rewritten are all invisible.  Here they show
BY VALUE, as a stale read does in tests/poison.py:

  hold          the stream is kept busy by stock torch work (torch.cuda._sleep, else a few large matrix products), an event
                `held` recorded behind it;
  late inputs   every device input lives in a buffer that holds a DECOY -- a valid input of the same entry, same shapes and
                dtypes, other seed, every index / count / length in range -- and is synchronised.  Behind the hold, on the same
                stream, the true input is copied in device-to-device; then the call is made on that stream.  Work of the
                entry that does not wait for the stream reads the decoy: a wrong FINITE answer, never an address from garbage
                (no NaN, 0xFF or random-word decoy: the rule of poison.py's LEFT state);
  recycling     straight after the call returns, on the same stream and without touching the host: every output is cloned
                into a snapshot, every input overwritten with its decoy again, every output and caller-provided workspace
                with 0xFF bytes.  Only then is the stream synchronised; the snapshot is what is compared;
  asynchrony    right after the call returns `held.query()` must still be false: the entry returned while the stream was
                held, so it did not synchronise the host, and the true inputs had not arrived when it was issued.  A hold
                that has run out is INCONCLUSIVE and fails.

The hold's length: at least 20 times the largest host time of a warm-up call seen so far (time.perf_counter around the call),
never under BASE_MS; the hold operation is timed once per Holder with events.  The module is a helper: no fixture, no pytest
setting.
"""
import time

BASE_MS = 100.0            # the shortest hold
MARGIN = 20.0              # hold >= MARGIN x the largest host time of a call
_SLEEP_PROBE = 20_000_000  # cycles of the calibration run of torch.cuda._sleep


def _torch():
    import torch
    return torch


class Inconclusive(AssertionError):
    """the hold ran out before the call returned: nothing was shown either way"""


class Late:
    """one device input: `buf` is what the library is handed; it holds `decoy` except between the late copy of `true` and the
    recycling.  host arrays in, any shape and dtype; m: the matrix is a GeneMajor handle of m sample columns"""

    def __init__(self, true, decoy, device, m=None):
        t = _torch()
        import numpy as np
        true, decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert true.shape == decoy.shape and true.dtype == decoy.dtype, "a decoy has the shape and dtype of the input"
        self.true = t.as_tensor(true).to(device)
        self.decoy = t.as_tensor(decoy).to(device)
        self.buf = self.decoy.clone()
        self.m = m

    @classmethod
    def around(cls, buf, decoy, m=None):
        """a buffer the product already holds (its content is the true input) and a device tensor of the decoy"""
        assert buf.shape == decoy.shape and buf.dtype == decoy.dtype, "a decoy has the shape and dtype of the input"
        self = cls.__new__(cls)
        self.true, self.decoy, self.buf, self.m = buf.clone(), decoy.to(buf.device), buf, m
        return self

    @property
    def handle(self):
        if self.m is None:
            return self.buf
        from deseq2_amd.native import GeneMajor
        return GeneMajor(self.buf, self.m)


class Holder:
    """times the hold operation once (events), remembers the host times of the warm-up calls, sizes every hold"""

    def __init__(self, device="cuda:0"):
        t = _torch()
        self.device = t.device(device)
        self.max_host_s = 0.0          # the largest host time of a warm-up call
        self.min_hold_ms = None        # the shortest hold asked for
        self.max_issue_s = 0.0         # the largest host time of a call under a hold
        self.holds = 0
        self.sleep = hasattr(t.cuda, "_sleep")
        self._mat = None
        self.unit_ms = self._calibrate()

    def _op(self, units):
        t = _torch()
        if self.sleep:
            t.cuda._sleep(int(units))
        else:
            for _ in range(int(units)):
                t.mm(self._mat, self._mat, out=self._out)

    def _calibrate(self):
        """milliseconds per unit of the hold operation (a cycle of _sleep, or one 8192^2 float32 product)"""
        t = _torch()
        if not self.sleep:
            self._mat = t.ones((8192, 8192), dtype=t.float32, device=self.device)
            self._out = t.empty_like(self._mat)
        probe = _SLEEP_PROBE if self.sleep else 2
        s = t.cuda.Stream(device=self.device)
        with t.cuda.stream(s):
            self._op(probe if self.sleep else 1)       # (code object loaded, clocks up)
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record(s)
            self._op(probe)
            e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.0, "the hold operation took no measurable time"
        return ms / probe

    def note_host_time(self, seconds):
        self.max_host_s = max(self.max_host_s, float(seconds))

    def target_ms(self):
        return max(BASE_MS, MARGIN * self.max_host_s * 1e3)

    def hold(self, stream):
        """keep `stream` busy for target_ms(); returns (held: the event behind the hold, the hold's length in ms)"""
        t = _torch()
        ms = self.target_ms()
        units = max(1, int(ms / self.unit_ms + 0.5))
        if not self.sleep:
            units = min(units, 64)                     # (a few large operations, never a long train)
        with t.cuda.stream(stream):
            self._op(units)
            held = t.cuda.Event()
            held.record(stream)
        self.min_hold_ms = ms if self.min_hold_ms is None else min(self.min_hold_ms, ms)
        self.holds += 1
        return held, ms


# ---- the outputs of a call: tensors, GeneMajor handles, and dicts / tuples / lists of them ----------------------------------
def _is_gm(o):
    return hasattr(o, "t") and hasattr(o, "ld") and hasattr(o, "m")


def leaves(o):
    """every tensor of an output structure"""
    t = _torch()
    if t.is_tensor(o):
        yield o
    elif _is_gm(o):
        yield o.t
    elif isinstance(o, dict):
        for v in o.values():
            yield from leaves(v)
    elif isinstance(o, (tuple, list)):
        for v in o:
            yield from leaves(v)


def snapshot(o):
    """the same structure, every tensor cloned (on the current stream)"""
    t = _torch()
    if t.is_tensor(o):
        return o.clone()
    if _is_gm(o):
        return type(o)(o.t.clone(), o.m)
    if isinstance(o, dict):
        return {k: snapshot(v) for k, v in o.items()}
    if isinstance(o, (tuple, list)):
        return type(o)(snapshot(v) for v in o)
    return o


def fill_ff(o):
    """every byte of the storage behind every tensor of `o` becomes 0xFF (on the current stream)"""
    t = _torch()
    seen = set()
    for v in leaves(o):
        st = v.untyped_storage()
        if st.data_ptr() in seen or st.nbytes() == 0:
            continue
        seen.add(st.data_ptr())
        t.empty(0, dtype=t.uint8, device=v.device).set_(st).fill_(0xFF)


class Step:
    """one call behind a hold: the inputs that arrive late for it, the call, the caller-provided workspaces it uses"""

    def __init__(self, lates, fn, scratch=(), what=""):
        self.lates, self.fn, self.scratch, self.what = list(lates), fn, list(scratch), what


def _arrive(lates):
    for l in lates:
        l.buf.copy_(l.true, non_blocking=True)


def _recycle(step, out):
    snap = snapshot(out)
    for l in step.lates:
        l.buf.copy_(l.decoy, non_blocking=True)
    fill_ff(out)
    fill_ff(step.scratch)
    return snap


def plain(holder, stream, steps):
    """the warm-up: the same sequence on `stream` without a hold, synchronised, TWICE -- the first pass grows the workspace
    slots of (device, stream), loads the code objects and leaves torch's allocator holding the blocks the held run will ask
    for; the host time of every call of the second pass (what a call costs in the steady state) goes to the holder.
    Returns the snapshots of the second pass."""
    t = _torch()
    for timed in (False, True):
        snaps = []
        t.cuda.synchronize()
        with t.cuda.stream(stream):
            for s in steps:
                _arrive(s.lates)
            for s in steps:
                t0 = time.perf_counter()
                out = s.fn()
                if timed:
                    holder.note_host_time(time.perf_counter() - t0)
                snaps.append(_recycle(s, out))
        stream.synchronize()
    return snaps


def held(holder, stream, steps, expect_async=True, sync=True):
    """Hold `stream`; behind the hold the true inputs of every step arrive; then, step by step: the call, the asynchrony
    check, snapshot and recycling.  Only then the stream is synchronised.  Returns (snapshots, info) -- info: hold_ms, the
    host time of every call, whether `held` was still pending after each.  expect_async = False (an entry that states a host
    synchronisation itself): the asynchrony check is not made; sync = False: the caller synchronises `stream` (after work on another stream, say)."""
    t = _torch()
    for s in steps:
        for l in s.lates:
            l.buf.copy_(l.decoy)
    t.cuda.synchronize()                       # decoys in place, nothing pending anywhere
    snaps, issue, pending = [], [], []
    ev, hold_ms = holder.hold(stream)
    with t.cuda.stream(stream):
        for s in steps:
            _arrive(s.lates)
        for s in steps:
            t0 = time.perf_counter()
            out = s.fn()
            dt = time.perf_counter() - t0
            still = not ev.query()
            issue.append(dt)
            pending.append(still)
            holder.max_issue_s = max(holder.max_issue_s, dt)
            if expect_async and not still:
                stream.synchronize()
                raise Inconclusive("%s: INCONCLUSIVE -- the hold of %.1f ms had run out when the call returned after %.3f ms of "
                                   "host time: the entry synchronised the host, or the hold is too short"
                                   % (s.what, hold_ms, dt * 1e3))
            snaps.append(_recycle(s, out))
    if sync:
        stream.synchronize()
    info = dict(hold_ms=hold_ms, issue_s=issue, pending=pending, event=ev)
    return snaps, info
