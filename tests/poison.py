"""Poisoned memory for the tests of the library's memory contract (tests/test_gpu_chain_memory.py,
tests/test_gpu_entry_memory.py; tests/test_poison_cpu.py tests this module on a numpy array).

One uint8 buffer is the ARENA.  A test carves from it every device buffer it hands to the library: each block starts on a
256-byte boundary and has at least MARGIN = 64 KiB of guard bytes (0xA5) in front of it and behind it.  `check()` then says
what the library did to memory it had no business with:

  * a guard byte that is no longer 0xA5             -> a write outside a buffer (an overrun of the workspace included: the
                                                       tests give it exactly its `_workspace_bytes`);
  * a watched view that is no longer what it was    -> an input that was written, or the padding columns m .. ld-1 of a
                                                       gene-major output that were.

What the library READS before it has written it shows in the values instead: the tests run the same call on buffers in
different prefill states and ask for the same bits.  There are exactly three states:

  FF     every byte 0xFF: NaN in a double, -1 in an int32;
  ZERO   every byte 0x00: what Python's wrappers hand over anyway (torch.zeros), the state the suite had before;
  LEFT   left by another analysis: the bytes a run of the same shape and options on OTHER data left in the same buffers --
         finite, plausible, in range: what a caching allocator produces in real use.

No other byte pattern is used, and that is deliberate.  The library keeps row lists and counters in the chain's workspace.
A stale int32 that a kernel takes for a row number or a length reads as -1 or 0 in the first two states and as a row
number below n in the third: the access it leads to lies at most one row in front of a buffer -- ld * 8 bytes, 16 KiB or
less at the shapes of these tests -- or inside it, i.e. inside the arena's margins.  A large stale value (0xA5A5A5A5, a random
word) would index far outside the arena, into memory of other processes' making: a fault on a shared machine instead of a
failed assertion.  These tests find stale reads BY VALUE, never by faulting.  (The guard pattern 0xA5 is never inside a buffer
the library is handed: the margins are not the library's to read.)

`standing_in()` puts the arena behind `torch.empty` for CUDA devices (pinned and host requests pass through), which reaches
the allocations of native.py, engine.py and fused.py without touching product code; with zeros = True also behind
`torch.zeros`, for the wrappers that hand the library a cleared output (the call under test is then the ONLY code running
inside the context).  The module is a helper: no fixture, no pytest setting.
"""
import contextlib

import numpy as np

GUARD = 0xA5
MARGIN = 64 * 1024
ALIGN = 256
FF, ZERO, LEFT = "FF", "ZERO", "LEFT"
BYTE = {FF: 0xFF, ZERO: 0x00}


def round8(m):
    return (int(m) + 7) & ~7


def padded_ld(m):
    """the leading dimension of the tests' gene-major handles: padding in every case, m a multiple of 8 included"""
    return round8(m) + 8


def _is_numpy(a):
    return isinstance(a, np.ndarray)


def _snapshot(view):
    return view.copy() if _is_numpy(view) else view.clone()


def _differs(view, other):
    """number of elements of `view` whose bits differ from `other` (an array of the same shape, or one byte value)"""
    if _is_numpy(view):
        a = np.ascontiguousarray(view).view(np.uint8)
        b = other if isinstance(other, int) else np.ascontiguousarray(other).view(np.uint8)
        return int(np.count_nonzero(a != b))
    a = view.contiguous().view(-1).view(_torch().uint8)
    b = other if isinstance(other, int) else other.contiguous().view(-1).view(_torch().uint8)
    return int((a != b).sum().item())


def _torch():
    import torch
    return torch


class Arena:
    """the arena over `buf`, a one-dimensional uint8 numpy array or torch tensor; `margin` >= 64 KiB"""

    def __init__(self, buf, margin=MARGIN):
        assert buf.ndim == 1 and margin >= MARGIN
        assert buf.dtype == (np.uint8 if _is_numpy(buf) else _torch().uint8)
        self.buf = buf
        self.margin = int(margin)
        self.addr = int(buf.ctypes.data) if _is_numpy(buf) else int(buf.data_ptr())
        self.size = int(buf.shape[0])
        self.blocks = []               # (offset, bytes, name), in address order
        self.watched = []              # (view, snapshot or byte value, what)
        self.cursor = 0
        buf[:] = GUARD

    @classmethod
    def on_device(cls, nbytes, device="cuda:0", margin=MARGIN):
        t = _torch()
        return cls(t.empty(int(nbytes), dtype=t.uint8, device=device), margin)

    # ---- carving
    def carve(self, nbytes, prefill=None, name=None):
        """a uint8 view of `nbytes` bytes, 256-byte aligned, `margin` guard bytes on both sides; filled with the byte
        `prefill` (None: left at the guard pattern for the caller to fill whole)"""
        nbytes = int(nbytes)
        off = self.cursor + self.margin
        off += -(self.addr + off) % ALIGN
        if off + nbytes + self.margin > self.size:
            raise MemoryError("arena of %d bytes is full (%d blocks, %d more bytes asked for)" % (self.size, len(self.blocks), nbytes))
        self.blocks.append((off, nbytes, name or "block %d" % len(self.blocks)))
        self.cursor = off + nbytes
        view = self.buf[off: off + nbytes]
        if prefill is not None and nbytes:
            view[:] = int(prefill)
        return view

    def empty(self, shape, dtype, prefill, name=None):
        """torch: a contiguous tensor of `shape` / `dtype` carved from the arena, every byte `prefill`"""
        t = _torch()
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, t.Size)) else (shape,)))
        count = int(np.prod(shape, dtype=np.int64)) if shape else 1
        item = t.empty((), dtype=dtype).element_size()
        return self.carve(count * item, prefill, name).view(dtype).view(shape)

    def put(self, host, name=None):
        """torch: a watched device copy of a host array (an INPUT of the library: bytewise as it was at check())"""
        t = _torch()
        h = t.as_tensor(np.ascontiguousarray(host))
        d = self.empty(h.shape, h.dtype, 0, name)
        d.copy_(h)
        self.unchanged(d, "input %s" % (name or len(self.blocks)))
        return d

    def gene_major(self, host, pad, name=None):
        """torch: an n x m host matrix as a watched GeneMajor input with ld = round8(m) + 8, the padding columns m .. ld-1
        holding `pad` (-7 for int32 counts, NaN for doubles)"""
        from deseq2_amd.native import GeneMajor
        t = _torch()
        h = t.as_tensor(np.ascontiguousarray(host))
        n, m = h.shape
        d = self.empty((n, padded_ld(m)), h.dtype, 0, name)
        d[:, :m] = h.to(d.device)
        g = GeneMajor(d, m)
        poison_padding(g, pad)
        self.unchanged(d, "input %s" % (name or len(self.blocks)))
        return g

    def owns(self, t):
        """whether the tensor / array starts inside a carved block of this arena"""
        at = (int(t.ctypes.data) if _is_numpy(t) else int(t.data_ptr())) - self.addr
        return any(off <= at < off + max(nbytes, 1) for off, nbytes, _ in self.blocks)

    # ---- what check() looks at
    def unchanged(self, view, what):
        """`view` (any strided view of a carved buffer) must hold at check() the bits it holds now"""
        self.watched.append((view, _snapshot(view), what))

    def holds(self, view, byte, what):
        """every byte of `view` must be `byte` at check(): the padding of an output that was allocated prefilled"""
        self.watched.append((view, int(byte), what))

    def padding(self, handle, what, byte=None):
        """watch the padding columns m .. ld-1 of a GeneMajor output: as they are now, or every byte `byte`"""
        pad = handle.t[:, handle.m:]
        if byte is None:
            self.unchanged(pad, "padding of " + what)
        else:
            self.holds(pad, byte, "padding of " + what)

    def _gaps(self):
        at = 0
        for off, nbytes, name in self.blocks:
            yield at, off, "in front of " + name
            at = off + nbytes
        yield at, self.size, "behind " + (self.blocks[-1][2] if self.blocks else "the start")

    def problems(self):
        """what check() would complain about, as a list of strings"""
        out = []
        for lo, hi, where in self._gaps():
            if hi > lo:
                bad = _differs(self.buf[lo:hi], GUARD)
                if bad:
                    g = self.buf[lo:hi]
                    g = g if _is_numpy(g) else g.cpu().numpy()
                    first = int(np.flatnonzero(g != GUARD)[0])
                    out.append("guard: %d bytes written %s, the first at offset %d (%d bytes into the gap of %d)"
                               % (bad, where, lo + first, first, hi - lo))
        for view, want, what in self.watched:
            bad = _differs(view, want)
            if bad:
                out.append("%s: %d bytes %s" % (what, bad, "are not 0x%02X" % want if isinstance(want, int) else "changed"))
        return out

    def check(self):
        """every guard byte intact, every watched input as it was, the padding of every watched output as prefilled"""
        if not _is_numpy(self.buf):
            _torch().cuda.synchronize()
        bad = self.problems()
        assert not bad, "memory contract broken:\n  " + "\n  ".join(bad)

    # ---- behind torch.empty
    @contextlib.contextmanager
    def standing_in(self, monkeypatch, prefill, zeros=False):
        """while active, torch.empty (and with zeros = True torch.zeros) for a CUDA device returns a carved tensor with every
        byte `prefill`; pinned-memory and host requests, and forms this stand-in does not know, go to the real function"""
        t = _torch()
        real_empty, real_zeros = t.empty, t.zeros
        arena = self

        def stand_in(real):
            def fn(*size, dtype=None, device=None, pin_memory=False, **kw):
                cuda = device is not None and t.device(device).type == "cuda"
                if kw or pin_memory or not cuda:
                    return real(*size, dtype=dtype, device=device, pin_memory=pin_memory, **kw)
                shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, t.Size)) else size
                return arena.empty(tuple(shape), dtype or t.get_default_dtype(), prefill, "torch." + real.__name__)
            return fn
        with monkeypatch.context() as mp:
            mp.setattr(t, "empty", stand_in(real_empty))
            if zeros:
                mp.setattr(t, "zeros", stand_in(real_zeros))
            yield self


def poison_padding(handle, value):
    """write `value` into the padding columns m .. ld-1 of a GeneMajor handle"""
    if handle.ld > handle.m:
        handle.t[:, handle.m:] = value
    return handle
