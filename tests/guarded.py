"""Framed buffers for the caller-buffer tests: every buffer handed to the
library sits inside one larger allocation that is filled with a poison byte,
with a guard band on each side of it.

A store outside the view lands in the guard (memory the test owns) and
check() reports it; a byte the library promised to leave alone still holds
the poison (untouched()); a byte the library promised to write cannot equal
the reference under two different poisons unless it really was written.

The view's address can be placed at any 16-byte residue of a 128-byte line
(base_mod), so a kernel that assumes line-aligned bases is seen.  Works on
numpy arrays (host mode; needs no GPU) and on torch tensors (device mode)."""
from __future__ import annotations

import numpy as np

GUARD = 4096   # several times the widest store of any kernel: 64 lanes x 16 bytes
LINE = 128

# torch has no unsigned 16/32/64-bit arithmetic types everywhere; the device
# view of an unsigned array is its signed twin, host() gives the numpy dtype back
_TORCH_NAME = {"uint8": "uint8", "int8": "int8", "uint16": "int16", "int16": "int16",
               "uint32": "int32", "int32": "int32", "uint64": "int64", "int64": "int64"}


def _where(idx, lo, hi):
    """'-3 bytes before the start' / '+3 bytes past the end' for allocation offset idx."""
    return f"-{lo - idx} bytes before the start" if idx < lo else f"+{idx - hi + 1} bytes past the end"


class Frame:
    """One framed buffer.  view: the typed array / tensor the library gets;
    ptr: its address (valid inside the allocation even when the view is empty);
    nbytes: its size; buf: the whole uint8 allocation; off: the view's offset."""

    def __init__(self, n_items, dtype, base_mod, poison, guard, device):
        self.dtype = np.dtype(dtype)
        assert base_mod % 16 == 0 and 0 <= base_mod < LINE, base_mod
        assert 0 <= poison <= 255 and guard >= 0 and n_items >= 0
        self.n_items, self.poison, self.guard = int(n_items), int(poison), int(guard)
        self.nbytes = self.n_items * self.dtype.itemsize
        total = guard + LINE + self.nbytes + guard
        self.device = device
        if device is None:
            self.buf = np.full(total, poison, np.uint8)
            addr = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.full((total,), poison, dtype=torch.uint8, device=device)
            addr = self.buf.data_ptr()
        self.off = guard + (base_mod - (addr + guard)) % LINE
        self.ptr = addr + self.off
        assert self.ptr % LINE == base_mod and self.off + self.nbytes + guard <= total
        raw = self.buf[self.off:self.off + self.nbytes]
        if device is None:
            self.view = raw.view(self.dtype)
        else:
            import torch
            self.view = raw.view(getattr(torch, _TORCH_NAME[self.dtype.name]))
            torch.cuda.synchronize(device)  # the library's stream is not torch's

    # -- access ---------------------------------------------------------------
    def _all(self) -> np.ndarray:
        """The whole allocation as a host uint8 array (a copy in device mode)."""
        return self.buf if self.device is None else self.buf.cpu().numpy()

    def host(self) -> np.ndarray:
        """The view's contents as a numpy array of the frame's dtype (a copy)."""
        return self._all()[self.off:self.off + self.nbytes].copy().view(self.dtype)

    def fill(self, data) -> None:
        """Copy bytes-like / array data (exactly nbytes) into the view."""
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert a.size == self.nbytes, (a.size, self.nbytes)
        if not a.size:
            return
        if self.device is None:
            self.buf[self.off:self.off + self.nbytes] = a
        else:
            import torch
            self.buf[self.off:self.off + self.nbytes] = torch.from_numpy(a.copy()).to(self.device)
            torch.cuda.synchronize(self.device)

    # -- assertions -----------------------------------------------------------
    def check(self, what="buffer") -> None:
        """Every byte of the allocation outside the view still holds the poison."""
        a = self._all()
        lo, hi = self.off, self.off + self.nbytes
        bad = np.concatenate([np.flatnonzero(a[:lo] != self.poison),
                              hi + np.flatnonzero(a[hi:] != self.poison)])
        if bad.size:
            first, last = int(bad[0]), int(bad[-1])
            raise AssertionError(
                f"{what}: {bad.size} guard byte(s) written, first {_where(first, lo, hi)} "
                f"(value 0x{int(a[first]):02x}), last {_where(last, lo, hi)} "
                f"(view of {self.nbytes} bytes, poison 0x{self.poison:02x})")

    def untouched(self, what="buffer") -> None:
        """Every byte of the view still holds the poison (and so do the guards)."""
        self.check(what)
        a = self._all()[self.off:self.off + self.nbytes]
        bad = np.flatnonzero(a != self.poison)
        if bad.size:
            raise AssertionError(
                f"{what}: {bad.size} byte(s) of the view written, first at +{int(bad[0])}, "
                f"last at +{int(bad[-1])} of {self.nbytes} (poison 0x{self.poison:02x})")


def frame(n_items, dtype, *, base_mod=16, poison=0xA5, guard=GUARD, device=None) -> Frame:
    """A poisoned allocation of guard + 128 + nbytes + guard bytes and a view of
    n_items x dtype in it whose address is base_mod mod 128."""
    return Frame(n_items, dtype, base_mod, poison, guard, device)


def frame_input(data, dtype=np.uint8, *, base_mod=16, poison=0xA5, guard=GUARD,
                device=None) -> Frame:
    """frame() with the payload copied in: both sides of it hold the poison."""
    a = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    dt = np.dtype(dtype)
    assert a.size % dt.itemsize == 0
    f = Frame(a.size // dt.itemsize, dt, base_mod, poison, guard, device)
    f.fill(a)
    return f
