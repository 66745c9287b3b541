"""tests/poison.py on a numpy array standing in for the arena: carving, alignment, margins, and a check() that reports a
flipped guard byte, a flipped input byte and a written padding element -- each by itself."""
import numpy as np
import pytest

from tests import poison
from tests.poison import Arena


class _Handle:
    """what poison_padding / Arena.padding need of native.GeneMajor"""

    def __init__(self, t, m):
        self.t, self.m, self.n, self.ld = t, m, t.shape[0], t.shape[1]


def _arena(nbytes=1 << 20):
    # (an odd start address: the alignment is of the ADDRESS, not of the offset)
    return Arena(np.zeros(nbytes + 3, np.uint8)[3:])


def test_leading_dimension_always_has_padding():
    for m, ld in ((1, 16), (6, 16), (8, 16), (9, 24), (48, 56), (130, 144)):
        assert poison.padded_ld(m) == ld and ld % 8 == 0 and ld - m >= 8


def test_carving_alignment_and_margins():
    a = _arena()
    assert (a.buf == poison.GUARD).all()
    views = [a.carve(k, prefill=0xFF, name="b%d" % k) for k in (1, 255, 256, 4097, 0, 100000)]
    end = 0
    for v, (off, nbytes, name) in zip(views, a.blocks):
        assert v.shape == (nbytes,) and (v == 0xFF).all()
        assert (a.addr + off) % poison.ALIGN == 0, name
        assert off - end >= poison.MARGIN, name                       # guard in front, counted from the previous block's end
        if nbytes:
            assert v.ctypes.data == a.addr + off
        end = off + nbytes
    assert a.size - end >= poison.MARGIN                              # ... and behind the last one
    assert poison.MARGIN >= 64 * 1024
    a.check()
    with pytest.raises(MemoryError):
        a.carve(a.size)
    with pytest.raises(AssertionError):
        Arena(np.zeros(1 << 20, np.uint8), margin=1024)


def test_prefill_none_leaves_the_block_to_the_caller():
    a = _arena()
    v = a.carve(64)
    v[:] = 7
    a.check()                                                         # the block itself is not guard


@pytest.mark.parametrize("where", ["front", "behind", "tail"])
def test_a_flipped_guard_byte_is_reported(where):
    a = _arena()
    a.carve(1000, 0, "first")
    off, nbytes, _ = a.blocks[0]
    a.carve(1000, 0, "second")
    at = {"front": off - 1, "behind": off + nbytes, "tail": a.size - 1}[where]
    a.check()
    a.buf[at] ^= 0x01
    bad = a.problems()
    assert len(bad) == 1 and bad[0].startswith("guard: 1 bytes written") and "offset %d " % at in bad[0]
    with pytest.raises(AssertionError, match="memory contract broken"):
        a.check()


def test_a_flipped_input_byte_is_reported():
    a = _arena()
    x = a.carve(8 * 40, 0, "x").view(np.float64).reshape(5, 8)
    x[...] = np.arange(40.0).reshape(5, 8)
    a.unchanged(x, "input x")
    a.check()
    x.view(np.uint8)[3, 17] ^= 0x80
    bad = a.problems()
    assert bad == ["input x: 1 bytes changed"]
    with pytest.raises(AssertionError, match="input x"):
        a.check()


@pytest.mark.parametrize("byte", [None, 0xFF, 0x00])
def test_a_written_padding_element_is_reported(byte):
    a = _arena()
    m, ld = 6, poison.padded_ld(6)
    out = _Handle(a.carve(8 * 4 * ld, 0xFF if byte is None else byte, "mu").view(np.float64).reshape(4, ld), m)
    a.padding(out, "mu", byte)
    out.t[:, :m] = 1.5                                                # the sample columns are the library's to write
    a.check()
    out.t[2, m] = 1.5                                                 # ... the first padding column is not
    bad = a.problems()
    assert len(bad) == 1 and bad[0].startswith("padding of mu: ")
    with pytest.raises(AssertionError, match="padding of mu"):
        a.check()


def test_poison_padding_writes_the_padding_only():
    a = _arena()
    m, ld = 8, poison.padded_ld(8)
    h = _Handle(a.carve(4 * 3 * ld, 0, "y").view(np.int32).reshape(3, ld), m)
    h.t[:, :m] = 5
    poison.poison_padding(h, -7)
    assert (h.t[:, :m] == 5).all() and (h.t[:, m:] == -7).all() and ld - m == 8
    a.check()
