"""bloom.BloomFilter resident on the device (okv_bloom_*, include/okv_sst.h).

``DeviceBloom`` mirrors the filter the reference's default writer options carry
(segment_writer_option.go:20): ``add_rows`` is WriteRow's ``Add`` per row
(segment_writer.go:133-136) over rows in host or device memory, ``to_bytes`` /
``write_to_device`` are ``WriteTo`` (:295-300), ``test_rows`` is the batched
``Test``.  ``Encoder.encode`` / ``encode_device`` / ``GpuSegmentWriter`` take one
as ``bloom=``: the rows of the call are added on the device and the bytes go to
the encoder in device memory (OKV_F_BLOOM_DEVICE).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (BLOOM_FORCE_GLOBAL, BLOOM_FORCE_LDS, BLOOM_PATH_GLOBAL,  # noqa: F401
                   BLOOM_PATH_LDS, F_ASYNC, F_DEVICE_PTRS, lib)
from .sst import OkvError, _ptr, pack_rows


def estimate(n: int, p: float):
    """bloom.EstimateParameters -> (m, k)."""
    m, k = C.c_uint64(), C.c_uint64()
    lib().okv_bloom_estimate(n, p, C.byref(m), C.byref(k))
    return m.value, k.value


def pack_keys(keys):
    """[key, ...] -> the key arrays of the okv_rows layout (numpy)."""
    r = pack_rows([(k, b"") for k in keys])
    return dict(key_arena=r["key_arena"], key_off=r["key_off"], key_len=r["key_len"])


def key_rows(rows, n_rows, key_arena_bytes):
    """The key arrays of rows -- the pack_rows() dict, a list of keys or (key, value) pairs,
    or a dict of device tensors -- as an okv_rows -> (okv_rows, device?, the arrays kept alive)"""
    if not isinstance(rows, dict):
        rows = list(rows)
        rows = pack_rows(rows) if rows and isinstance(rows[0], tuple) else pack_keys(rows)
    host = isinstance(rows["key_len"], np.ndarray)
    n = int(rows["key_len"].size if host else rows["key_len"].numel()) \
        if n_rows is None else int(n_rows)
    if key_arena_bytes is None:
        ka = rows.get("key_arena")
        key_arena_bytes = 0 if ka is None else int(ka.size if host else ka.numel())
    R = _lib.Rows(_ptr(rows.get("key_arena")), _ptr(rows["key_off"]), _ptr(rows["key_len"]),
                  None, None, None, n, int(key_arena_bytes), 0)
    return R, not host, rows


class Values:
    """value(i) of a result that holds val_len, val_pos and val_arena."""

    def value(self, i):
        """Row i's value from val_arena (host arrays): bytes, or None for Go's nil."""
        n = int(self.val_len[i])
        if not n:
            return None
        p = int(self.val_pos[i])
        return self.val_arena[p:p + n].tobytes()


def rows_call(owner, name, cols, call, result, keys, n_rows, key_arena_bytes, values, val_cap,
              out, sync, flags=0):
    """What get_rows and snap_get_rows share.  cols: the (name, dtype) per-key arrays of the
    out struct; call(R, [pointer per column], arena pointer, cap, flags) -> (rc, out struct);
    result(arrays, arena, out struct) -> the result.  Device mode takes the tensors of
    ``out``; host mode makes the arrays, sizes the arena by an index-only call when val_cap
    is None, and raises OkvError with .result.  flags: further OKV_F_* bits of every call."""
    R, dev, keep = key_rows(keys, n_rows, key_arena_bytes)

    def go(arrays, arena, cap, flags):
        return call(R, [_ptr(arrays.get(k)) for k, _ in cols], _ptr(arena), cap, flags)

    if dev:
        arena = out.get("val_arena")
        cap = int(arena.numel()) if arena is not None and val_cap is None else int(val_cap or 0)
        rc, o = go(out, arena, cap, flags | F_DEVICE_PTRS | (0 if sync else F_ASYNC))
        arrays = {k: out.get(k) for k, _ in cols}
    else:
        arrays = {k: np.zeros(int(R.n_rows), t) for k, t in cols}
        arena, cap = None, 0
        if values:
            if val_cap is None:  # size query: index only, then the arena
                rc, o = go(arrays, None, 0, flags)
                owner._check(rc, name)
                val_cap = int(o.val_bytes)
            cap = int(val_cap)
            arena = np.zeros(max(cap, 1), np.uint8)
        rc, o = go(arrays, arena, cap, flags)
    res = result(arrays, arena, o)
    if rc:
        e = OkvError(rc, f"{name}: {owner.error()}")
        e.result = res
        raise e
    return res


class DeviceBloom:
    """One okv_bloom on the context of an existing Decoder / Encoder."""

    def __init__(self, owner, m: int = 0, k: int = 0, _handle=None):
        self._owner = owner
        self._h = _handle
        self._wt = None  # device buffer of write_to_device()
        if self._h is None:
            h = C.c_void_p()
            owner._check(lib().okv_bloom_new(owner._ctx, m, k, C.byref(h)), "okv_bloom_new")
            self._h = h.value

    @classmethod
    def with_estimates(cls, owner, n: int, p: float) -> "DeviceBloom":
        """bloom.NewWithEstimates(n, p)."""
        return cls(owner, *estimate(n, p))

    @classmethod
    def from_bytes(cls, owner, data) -> "DeviceBloom":
        """BloomFilter.ReadFrom of WriteTo bytes (raises OkvError(OKV_E_ARG) where Go errors)."""
        a = np.frombuffer(bytes(data), np.uint8)
        h = C.c_void_p()
        owner._check(lib().okv_bloom_read_from(owner._ctx, _ptr(a), a.size, C.byref(h)),
                     "okv_bloom_read_from")
        return cls(owner, _handle=h.value)

    # -- properties ----------------------------------------------------------------
    def info(self):
        """-> (m, k, bitset length, WriteTo bytes)"""
        v = [C.c_uint64() for _ in range(4)]
        lib().okv_bloom_info(self._h, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    m = property(lambda self: self.info()[0])
    k = property(lambda self: self.info()[1])
    length = property(lambda self: self.info()[2])
    write_to_bytes = property(lambda self: self.info()[3])

    def last_path(self) -> int:
        """BLOOM_PATH_LDS / BLOOM_PATH_GLOBAL: the form the last add_rows took (0: no launch)."""
        return int(lib().okv_bloom_last_path(self._h))

    # -- rows ----------------------------------------------------------------------
    def add_rows(self, rows, n_rows=None, key_arena_bytes=None, form: int = 0, sync=True):
        """Add(key) for every row.  rows: the pack_rows() dict, a list of keys or
        (key, value) pairs (host mode), or a dict of device tensors key_arena,
        key_off, key_len.  form: BLOOM_FORCE_LDS / BLOOM_FORCE_GLOBAL; sync=False
        only enqueues (device tensors)."""
        R, dev, keep = key_rows(rows, n_rows, key_arena_bytes)
        flags = form | ((F_DEVICE_PTRS | (0 if sync else F_ASYNC)) if dev else 0)
        self._owner._check(lib().okv_bloom_add_rows(self._owner._ctx, self._h, C.byref(R), flags),
                           "okv_bloom_add_rows")
        return self

    def test_rows(self, rows, n_rows=None, key_arena_bytes=None, out=None, sync=True):
        """Test(key) for every row -> uint8 per key (1 maybe, 0 absent): a numpy
        array (host rows) or `out`, a device uint8 tensor (device rows)."""
        R, dev, keep = key_rows(rows, n_rows, key_arena_bytes)
        if dev:
            if out is None:
                raise ValueError("test_rows on device rows needs out=")
            flags = F_DEVICE_PTRS | (0 if sync else F_ASYNC)
        else:
            out = np.zeros(int(R.n_rows), np.uint8)
            flags = 0
        self._owner._check(lib().okv_bloom_test_rows(self._owner._ctx, self._h, C.byref(R),
                                                     _ptr(out), flags), "okv_bloom_test_rows")
        return out

    # -- WriteTo / ClearAll --------------------------------------------------------
    def to_bytes(self) -> bytes:
        """WriteTo's bytes on the host."""
        b = np.zeros(self.write_to_bytes, np.uint8)
        self._owner._check(lib().okv_bloom_write_to(self._owner._ctx, self._h, _ptr(b), b.size, 0),
                           "okv_bloom_write_to")
        return b.tobytes()

    def write_to_device(self, dst=None, sync=True):
        """WriteTo into device memory -> (device pointer, bytes).  dst: a uint8
        device tensor (8-byte aligned), or None for a buffer the filter owns
        (valid until the next call without dst, or close())."""
        need = self.write_to_bytes
        if dst is None:
            if self._wt is None or self._wt[1] < need:
                self._free_wt()
                p = lib().okv_device_alloc(self._owner._ctx, need)
                if not p:
                    raise OkvError(_lib.OKV_E_HIP, "okv_device_alloc")
                self._wt = (p, need)
            ptr, cap = self._wt
        else:
            ptr, cap = _ptr(dst), int(dst.numel())
        flags = F_DEVICE_PTRS | (0 if sync else F_ASYNC)
        self._owner._check(lib().okv_bloom_write_to(self._owner._ctx, self._h, ptr, cap, flags),
                           "okv_bloom_write_to(device)")
        return ptr, need

    def clear(self):
        """ClearAll."""
        self._owner._check(lib().okv_bloom_clear(self._owner._ctx, self._h), "okv_bloom_clear")
        return self

    def _free_wt(self):
        if self._wt is not None and getattr(self._owner, "_ctx", None):
            self._owner.sync()
            lib().okv_device_free(self._owner._ctx, self._wt[0])
        self._wt = None

    def close(self):
        L = _lib._lib
        if getattr(self, "_h", None) and L is not None:
            self._free_wt()
            L.okv_bloom_free(self._h)
            self._h = None

    __del__ = close
