"""Snapshot GetRows on the device (okv_snap_*, include/okv_sst.h).

``DeviceSnapshot`` is snapshot_reader.Reader's blockRangeTree resident on the device:
segments already in device memory, each with its ``DeviceIndex`` and optional
``DeviceBloom``, in the tree's order (blockRangeLessFunc, snapshot_reader.go:28-60)
and ranked in GetRow's order (Level ascending, then ID descending, :109-116).
``snap_get_rows`` is Reader.GetRow (:104-149) for many keys in one call: the candidate
segments of every key, each probed and searched as ``get_rows`` does, the newest
answer per key.  Key and output arrays are numpy arrays (host mode, staged) or torch
tensors on the device, as for ``get_rows``.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import (F_ASYNC, F_DEVICE_PTRS, F_GET_ZSTD, SNAP_DELETED, SNAP_FALLBACK, SNAP_FOUND,  # noqa: F401
                   SNAP_NO_ROWS, SNAP_SEG_ERROR, lib)
from .bloom import Values, rows_call
from .sst import _ptr

_OUT = (("state", np.int32), ("seg", np.uint32), ("blk_status", np.int32), ("entry", np.uint32),
        ("val_off", np.uint64), ("val_len", np.uint32), ("val_pos", np.uint64))
_TOTALS = ("n_found", "n_deleted", "n_fallback", "val_bytes", "pairs_probed", "blocks_searched")


def _b(x) -> bytes:
    return b"" if x is None else bytes(x)


class _Rec:
    def __init__(self, at, ID, Level, FirstKey, LastKey):
        self.at, self.ID, self.Level = at, ID, Level
        self.FirstKey, self.LastKey = _b(FirstKey), _b(LastKey)


def _priority_less(x, y):  # snapshot_reader.go:109-116
    if x.Level != y.Level:
        return x.Level < y.Level
    return x.ID > y.ID


class DeviceSnapshot:
    """One okv_snap on the context of an existing Decoder / Encoder.  It keeps the
    segments, indexes and filters it is given alive; it does not own them."""

    def __init__(self, owner, segments):
        """segments: (seg, seg_bytes, DeviceIndex, DeviceBloom | None, compression, level,
        ID, first_key, last_key) each, in any order; seg is a device uint8 tensor or a
        device pointer.  ``order[t]`` is the position in ``segments`` of tree position t
        (what ``SnapResult.seg`` counts in) and ``ids[t]`` its ID.  Segments that are
        equal under blockRangeLessFunc replace each other as in ReplaceOrInsert: the
        last one given stays."""
        from .snapshot import _Tree, _block_range_less
        self._owner = owner
        self._h = None
        self._keep = list(segments)
        tree = _Tree(_block_range_less)
        for at, s in enumerate(self._keep):
            tree.replace_or_insert(_Rec(at, s[6], int(s[5]), s[7], s[8]))
        recs = tree.items
        ranked = sorted(recs, key=functools.cmp_to_key(
            lambda a, b: -1 if _priority_less(a, b) else (1 if _priority_less(b, a) else 0)))
        prio = {r.at: p for p, r in enumerate(ranked)}
        self.order = [r.at for r in recs]
        self.ids = [r.ID for r in recs]
        self.levels = [r.Level for r in recs]
        arr = (_lib.SnapSeg * max(len(recs), 1))()
        self._keys = []
        for t, r in enumerate(recs):
            seg, nbytes, index, bloom, comp = self._keep[r.at][:5]
            fk = np.frombuffer(r.FirstKey, np.uint8)
            lk = np.frombuffer(r.LastKey, np.uint8)
            self._keys += [fk, lk]
            arr[t] = _lib.SnapSeg(
                seg if isinstance(seg, int) or seg is None else _ptr(seg), int(nbytes), index._h,
                bloom._h if bloom is not None else None, _ptr(fk) if fk.size else None,
                _ptr(lk) if lk.size else None, fk.size, lk.size, int(comp), r.Level, prio[r.at])
        h = C.c_void_p()
        owner._check(lib().okv_snap_new(owner._ctx, arr, len(recs), C.byref(h)), "okv_snap_new")
        self._h = h.value

    def __len__(self):
        return len(self.order)

    def close(self):
        L = _lib._lib
        if getattr(self, "_h", None) and L is not None:
            L.okv_snap_free(self._h)
            self._h = None

    __del__ = close


class SnapResult(Values):
    """The arrays of okv_snap_out and its totals."""

    def __init__(self, arrays, val_arena, o):
        self.__dict__.update(arrays)
        self.val_arena = val_arena
        for k in _TOTALS:
            setattr(self, k, int(getattr(o, k)))


def snap_get_rows(owner, snap: DeviceSnapshot, keys, values=True, val_cap=None, out=None,
                  sync=True, n_rows=None, key_arena_bytes=None, zstd=False) -> SnapResult:
    """okv_snap_get_rows.  keys: a list of keys or a dict of numpy arrays key_arena /
    key_off / key_len (host mode), or a dict of device tensors (device mode; then ``out``
    must hold device tensors state, seg, blk_status, entry, val_off, val_len and
    optionally val_pos and val_arena, and sync=False only enqueues: totals()).
    Host mode: values=False is the index-only call; val_cap defaults to room for every
    value (two calls: the first sizes the arena).  zstd=True sets OKV_F_GET_ZSTD: zstd
    candidates answer like any other (val_off then counts inside the inflated block).
    Raises OkvError (OKV_E_CAPACITY with .result holding the totals)."""
    def call(R, ptrs, arena, cap, flags):
        o = _lib.SnapOut(*ptrs, arena, cap, 0, 0, 0, 0, 0, 0)
        return lib().okv_snap_get_rows(owner._ctx, snap._h, C.byref(R), C.byref(o), flags), o

    return rows_call(owner, "okv_snap_get_rows", _OUT, call, SnapResult, keys, n_rows,
                     key_arena_bytes, values, val_cap, out, sync, F_GET_ZSTD if zstd else 0)


def totals(owner) -> dict:
    """okv_snap_totals after a sync=False snap_get_rows and owner.sync()."""
    o = _lib.SnapOut()
    owner._check(lib().okv_snap_totals(owner._ctx, C.byref(o)), "okv_snap_totals")
    return {k: int(getattr(o, k)) for k in _TOTALS}


__all__ = ["DeviceSnapshot", "SnapResult", "snap_get_rows", "totals"]
