"""Batched GetRow on the device (okv_index_*, okv_get_rows, include/okv_sst.h).

``DeviceIndex`` is SegmentMetadata.BlockIndex resident on the device (google/btree
built by ReplaceOrInsert in meta-block order: of equal first keys the last entry
stays).  ``get_rows`` is SegmentReader.GetRow (segment_reader.go:362-404) for many
keys against a segment in device memory in one call: bloom probe, floor block,
ReadBlockWithStat of each touched block once, the first row with an equal key.
Key and output arrays are numpy arrays (host mode, staged) or torch tensors on the
device, as for ``DeviceBloom``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (F_ASYNC, F_DEVICE_PTRS, F_GET_ZSTD, GET_BLOCK_ERROR, GET_BLOOM_NEGATIVE,  # noqa: F401
                   GET_FALLBACK, GET_FOUND, GET_NO_BLOCK, GET_NOT_IN_BLOCK, lib)
from .bloom import DeviceBloom, Values, pack_keys, rows_call
from .sst import _ptr

_OUT = (("state", np.int32), ("blk_status", np.int32), ("entry", np.uint32),
        ("val_off", np.uint64), ("val_len", np.uint32), ("val_pos", np.uint64))


class DeviceIndex:
    """One okv_index on the context of an existing Decoder / Encoder."""

    def __init__(self, owner, descs, first_keys):
        """descs: [n, 4] uint64 (Offset, BlockSize, OriginalSize, CompressedSize) and
        first_keys: n byte strings, both in meta-block order."""
        self._owner = owner
        self._h = None
        d = np.ascontiguousarray(descs, np.uint64).reshape(-1, 4)
        fk = [bytes(k) for k in first_keys]
        if d.shape[0] != len(fk):
            raise ValueError("descs and first_keys differ in length")
        k = pack_keys(fk)
        h = C.c_void_p()
        owner._check(lib().okv_index_new(owner._ctx, _ptr(d), _ptr(k["key_arena"]),
                                         _ptr(k["key_off"]), _ptr(k["key_len"]), len(fk),
                                         C.byref(h)), "okv_index_new")
        self._h = h.value

    @classmethod
    def from_metadata(cls, owner, md) -> "DeviceIndex":
        """The block index of a parsed meta block (sst.Metadata)."""
        return cls(owner, md.descs, md.first_keys)

    def info(self):
        """-> (entries in the tree, entries given)"""
        a, b = C.c_uint64(), C.c_uint64()
        lib().okv_index_info(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def close(self):
        L = _lib._lib
        if getattr(self, "_h", None) and L is not None:
            L.okv_index_free(self._h)
            self._h = None

    __del__ = close


class GetResult(Values):
    """The arrays of okv_get_out and its totals."""

    def __init__(self, arrays, val_arena, o):
        self.__dict__.update(arrays)
        self.val_arena = val_arena
        self.n_found, self.n_fallback = int(o.n_found), int(o.n_fallback)
        self.val_bytes, self.blocks_searched = int(o.val_bytes), int(o.blocks_searched)


def get_rows(owner, seg, seg_bytes, index: DeviceIndex, keys, bloom: DeviceBloom = None,
             compression=_lib.COMP_NONE, values=True, val_cap=None, out=None, sync=True,
             n_rows=None, key_arena_bytes=None, zstd=False) -> GetResult:
    """okv_get_rows.  seg: a device pointer (int) or a device uint8 tensor holding the
    segment's seg_bytes bytes.  keys: a list of keys or a dict of numpy arrays key_arena /
    key_off / key_len (host mode), or a dict of device tensors (device mode; then
    ``out`` must hold device tensors state, blk_status, entry, val_off, val_len and
    optionally val_pos and val_arena, and sync=False only enqueues: totals()).
    Host mode: values=False is the index-only call; val_cap defaults to room for every
    value (two calls: the first sizes the arena).  zstd=True sets OKV_F_GET_ZSTD: the
    touched blocks of a COMP_ZSTD segment are inflated on the device and searched, and
    val_off counts inside the inflated block ``entry`` names.  Raises OkvError
    (OKV_E_CAPACITY with .result holding the totals)."""
    segp = seg if isinstance(seg, int) or seg is None else _ptr(seg)
    bh = bloom._h if bloom is not None else None

    def call(R, ptrs, arena, cap, flags):
        o = _lib.GetOut(*ptrs, arena, cap, 0, 0, 0, 0)
        return lib().okv_get_rows(owner._ctx, segp, seg_bytes, index._h, bh, C.byref(R),
                                  compression, C.byref(o), flags), o

    return rows_call(owner, "okv_get_rows", _OUT, call, GetResult, keys, n_rows, key_arena_bytes,
                     values, val_cap, out, sync, F_GET_ZSTD if zstd else 0)


def totals(owner) -> dict:
    """okv_get_totals after a sync=False get_rows and owner.sync()."""
    o = _lib.GetOut()
    owner._check(lib().okv_get_totals(owner._ctx, C.byref(o)), "okv_get_totals")
    return {"n_found": int(o.n_found), "n_fallback": int(o.n_fallback),
            "val_bytes": int(o.val_bytes), "blocks_searched": int(o.blocks_searched)}


__all__ = ["DeviceIndex", "GetResult", "get_rows", "totals"]
