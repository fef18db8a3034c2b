"""tests/guarded.py itself, on numpy buffers (no GPU): planted writes around
and inside the view are caught, the base residue asked for is obtained, and
typed data round-trips."""
from __future__ import annotations

import numpy as np
import pytest

from tests import guarded as G

DTYPES = [np.uint8, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
BASES = [0, 16, 48, 112]


@pytest.mark.parametrize("poison", [0xA5, 0x5A])
def test_fresh_frame_is_clean(poison):
    f = G.frame(37, np.uint32, poison=poison)
    assert f.buf.size == 4096 + 128 + 37 * 4 + 4096 and (f.buf == poison).all()
    f.check()
    f.untouched()


def test_write_one_byte_before_is_caught():
    f = G.frame(10, np.uint8)
    f.buf[f.off - 1] ^= 0xFF
    with pytest.raises(AssertionError, match=r"-1 bytes before the start"):
        f.check()
    with pytest.raises(AssertionError):
        f.untouched()


def test_write_one_byte_after_is_caught():
    f = G.frame(10, np.uint16)
    f.buf[f.off + f.nbytes] = 0
    with pytest.raises(AssertionError, match=r"first \+1 bytes past the end.*last \+1 bytes"):
        f.check()
    f = G.frame(10, np.uint16)
    f.buf[f.off + f.nbytes + 2] = 0
    with pytest.raises(AssertionError, match=r"\+3 bytes past the end"):
        f.check()


def test_write_at_far_ends_of_the_guards_is_caught():
    f = G.frame(10, np.uint8)
    f.buf[-1] = 0
    with pytest.raises(AssertionError, match="past the end"):
        f.check()
    f = G.frame(10, np.uint8)
    f.buf[0] = 0
    with pytest.raises(AssertionError, match=rf"-{f.off} bytes before the start"):
        f.check()
    # first and last offender are both reported
    f = G.frame(10, np.uint8)
    f.buf[f.off - 5] = 0
    f.buf[f.off + f.nbytes + 15] = 0
    with pytest.raises(AssertionError, match=r"first -5 bytes before.*last \+16 bytes past"):
        f.check()


def test_a_write_of_the_poison_value_is_seen_under_the_other_poison():
    """Why every GPU case runs under two poisons: a stray byte that happens to
    equal one of them differs from the other."""
    stray = 0xA5
    hits = 0
    for poison in (0xA5, 0x5A):
        f = G.frame(4, np.uint8, poison=poison)
        f.buf[f.off + f.nbytes] = stray
        try:
            f.check()
        except AssertionError:
            hits += 1
    assert hits == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("base_mod", BASES)
def test_base_mod_obtained(dtype, base_mod):
    for n in (0, 1, 65):
        f = G.frame(n, dtype, base_mod=base_mod)
        assert f.ptr % 128 == base_mod
        assert f.off >= f.guard and f.buf.size - (f.off + f.nbytes) >= f.guard
        assert f.view.dtype == np.dtype(dtype) and f.view.size == n
        if n:
            assert f.view.ctypes.data == f.ptr
        assert f.buf.ctypes.data + f.off == f.ptr


def test_base_mod_must_be_a_multiple_of_16():
    with pytest.raises(AssertionError):
        G.frame(4, np.uint8, base_mod=8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_length_view(dtype):
    f = G.frame(0, dtype, base_mod=48)
    assert f.view.size == 0 and f.nbytes == 0 and f.host().size == 0
    f.check()
    f.untouched()
    f.buf[f.off] = 0  # the first byte "of" an empty view is guard
    with pytest.raises(AssertionError, match=r"\+1 bytes past the end"):
        f.check()


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip_typed(dtype):
    rng = np.random.default_rng(5)
    data = rng.integers(0, 200, 77).astype(dtype)
    f = G.frame(77, dtype, base_mod=112, poison=0x5A)
    f.view[:] = data
    assert np.array_equal(f.host(), data) and f.host().dtype == np.dtype(dtype)
    f.check()
    g = G.frame_input(data, dtype, base_mod=0)
    assert np.array_equal(g.view, data) and g.ptr % 128 == 0
    g.check()
    h = G.frame_input(data.tobytes(), base_mod=16)
    assert h.view.dtype == np.uint8 and h.view.tobytes() == data.tobytes()
    assert (h.buf[:h.off] == 0xA5).all() and (h.buf[h.off + h.nbytes:] == 0xA5).all()


def test_untouched_fails_after_any_write_into_the_view():
    for at in (0, 5, 9):
        f = G.frame(10, np.uint8)
        f.untouched()
        f.view[at] = 0
        f.check()  # the guards are still intact
        with pytest.raises(AssertionError, match=rf"first at \+{at}"):
            f.untouched()
    f = G.frame(3, np.uint64)
    f.view[2] = 1
    with pytest.raises(AssertionError, match=r"first at \+16"):
        f.untouched()
