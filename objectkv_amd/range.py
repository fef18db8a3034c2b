"""Range reads from resident segments (okv_seek_rows, okv_gather_rows, include/okv_sst.h).

``ResidentRows`` is a segment's decoded rows on the device with no host copy: for an
uncompressed segment the raw bytes plus an index-only decode (row_start, key_off, key_len,
val_off, val_len: offsets into the segment), for a zstd segment the decode's arenas.
``seek_rows`` is RowIter(direction).Seek(key) followed by Next() to the end
(segment_row_iter.go:102-207) for a batch of (segment, key, direction) triples: the row
range each iterator yields, which is an ``okv_merge_rows`` input.  ``gather_rows`` packs
the rows a merge picked (its ``src`` / ``row`` outputs, still on the device) into two
arenas.  Key and output arrays are numpy arrays (host mode, staged) or torch tensors on
the device, as for ``get_rows``.  ``pack_pages`` lays the merges of a batch out as the pages
of one ``okv_merge_pages`` call (``Decoder.merge_pages_device``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import F_ASYNC, F_DEVICE_PTRS, lib
from .bloom import Values, key_rows
from .sst import COMP_NONE, OkvError, _ptr

_GATHER = (("key_pos", np.uint64), ("key_len", np.uint16), ("val_pos", np.uint64),
           ("val_len", np.uint32))
ARENA_SPARE = 32  # bytes kept readable past an arena: the merge and the gather read the
#                   aligned 16-byte lines around a key or value


class ResidentRows:
    """The rows of one segment on the device.  ``t`` holds key_arena / key_off / key_len /
    val_arena / val_off / val_len (an ``okv_merge_src``'s pointers) and ``row_start``
    (the first row of every block, then ``n``); ``status`` is the only host array."""

    def __init__(self, decoder, seg_t, seg_bytes, md):
        """seg_t: the segment's bytes in a device uint8 tensor with ARENA_SPARE bytes of
        room after them; md: its parsed meta block (sst.Metadata)."""
        import torch
        dev = seg_t.device
        descs = np.ascontiguousarray(md.descs, np.uint64).reshape(-1, 4)
        nb = descs.shape[0]
        self.n_blocks, self.compression = nb, md.compression
        d_t = torch.from_numpy(descs.view(np.int64).copy()).to(dev) if nb else \
            torch.zeros((1, 4), dtype=torch.int64, device=dev)
        index_only = md.compression == COMP_NONE
        rows, kb, vb = decoder.plan_device(seg_t, seg_bytes, d_t, nb, md.compression, index_only)

        def z(n, dt):
            return torch.zeros(max(int(n), 1), dtype=dt, device=dev)
        out = {"row_start": z(nb + 1, torch.int64), "status": z(nb, torch.int32),
               "key_off": z(rows, torch.int64), "key_len": z(rows, torch.int16),
               "val_off": z(rows, torch.int64), "val_len": z(rows, torch.int32)}
        if not index_only:
            out.update(key_base=z(nb, torch.int64), val_base=z(nb, torch.int64),
                       key_arena=z(kb + ARENA_SPARE, torch.uint8),
                       val_arena=z(vb + ARENA_SPARE, torch.uint8))
        torch.cuda.current_stream(dev).synchronize()  # (the decoder has its own stream)
        if nb:
            decoder.decode_device(seg_t, seg_bytes, d_t, nb, out, md.compression,
                                  index_only=index_only)
        self.n = int(out["row_start"][nb].item())
        self.status = out["status"][:nb].cpu().numpy()
        ka = seg_t if index_only else out["key_arena"]
        va = seg_t if index_only else out["val_arena"]
        self.t = {"key_arena": ka, "key_off": out["key_off"], "key_len": out["key_len"],
                  "val_arena": va, "val_off": out["val_off"], "val_len": out["val_len"],
                  "row_start": out["row_start"]}
        self.index_only = index_only

    def resident_bytes(self) -> int:
        """Device bytes this object adds (the raw segment is not counted for an
        index-only decode: GetRows keeps it anyway)."""
        skip = ("key_arena", "val_arena") if self.index_only else ()
        return sum(int(v.numel()) * v.element_size() for k, v in self.t.items() if k not in skip)

    def seek_src(self) -> _lib.SeekSrc:
        t = self.t
        return _lib.SeekSrc(_ptr(t["key_arena"]), _ptr(t["key_off"]), _ptr(t["key_len"]),
                            _ptr(t["row_start"]), self.n, self.n_blocks)


def _seek_srcs(sources):
    arr = (_lib.SeekSrc * max(1, len(sources)))()
    for i, s in enumerate(sources):
        arr[i] = s.seek_src() if hasattr(s, "seek_src") else s
    return arr


def seek_rows(owner, sources, keys, src_of, direction, out=None, sync=True, n_rows=None,
              key_arena_bytes=None):
    """okv_seek_rows.  sources: ResidentRows (or _lib.SeekSrc) in the order src_of counts
    in.  Host mode: keys is a list of keys (None is UnboundStart) or a dict of numpy arrays
    key_arena / key_off / key_len, src_of and direction are sequences -> (row_lo, row_hi)
    numpy uint64 arrays.  Device mode: keys is a dict of device tensors, src_of (int32) and
    direction (uint8) are device tensors and ``out`` holds device tensors row_lo / row_hi
    (int64); sync=False only enqueues."""
    if not isinstance(keys, dict):
        keys = [b"" if k is None else bytes(k) for k in keys]
    R, dev, keep = key_rows(keys, n_rows, key_arena_bytes)
    n = int(R.n_rows)
    arr = _seek_srcs(sources)
    if dev:
        lo, hi = out["row_lo"], out["row_hi"]
        flags = F_DEVICE_PTRS | (0 if sync else F_ASYNC)
        so, di = src_of, direction
    else:
        so = np.ascontiguousarray(src_of, np.uint32)
        di = np.ascontiguousarray(direction, np.uint8)
        if so.size != n or di.size != n:
            raise ValueError("src_of and direction must have one entry per key")
        lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        flags = 0
    owner._check(lib().okv_seek_rows(owner._ctx, arr, len(sources), C.byref(R), _ptr(so),
                                     _ptr(di), _ptr(lo), _ptr(hi), flags), "okv_seek_rows")
    return lo, hi


def merge_srcs(sources):
    """(_lib.MergeSrc array, count) of the gather's sources: ResidentRows, dicts of the six
    device tensors, or merge_device's (dict, row_lo, row_hi, level) tuples."""
    arr = (_lib.MergeSrc * max(1, len(sources)))()
    for i, s in enumerate(sources):
        t = s.t if hasattr(s, "t") else (s[0] if isinstance(s, tuple) else s)
        arr[i] = _lib.MergeSrc(_ptr(t["key_arena"]), _ptr(t["key_off"]), _ptr(t["key_len"]),
                               _ptr(t["val_arena"]), _ptr(t["val_off"]), _ptr(t["val_len"]),
                               0, 0, 0, 0)
    return arr, len(sources)


PAGE_MAX_STREAMS = 64  # okv_page.nsrc


def pack_pages(jobs, first_slot=0):
    """The okv_merge_pages arguments of one batch of GetRange merges (no GPU).

    jobs: dicts with ``ranges`` [(row_lo, row_hi)] per stream, ``lim`` (> 0), ``direction``,
    ``bound`` (bytes), ``base`` (the index of the job's first stream in the call's srcs: its
    gather base) and ``cap`` (slots of its slice).  The slices lie one after the other from
    ``first_slot`` on, every job's (the old path's too) at the sum of the earlier caps.
    -> (pages: a _lib.Page array, bounds: the bounds back to back, at: each job's slice
    start, old: the indices of the jobs that are no page -- more than PAGE_MAX_ROWS rows
    or more than 64 streams -- and stay with okv_merge_rows)."""
    at, old, fit, blob = [], [], [], bytearray()
    slot = int(first_slot)
    for i, j in enumerate(jobs):
        at.append(slot)
        slot += int(j["cap"])
        rows = sum(int(b) - int(a) for a, b in j["ranges"])
        if rows > _lib.PAGE_MAX_ROWS or len(j["ranges"]) > PAGE_MAX_STREAMS:
            old.append(i)
            continue
        bound = bytes(j["bound"])
        fit.append(_lib.Page(int(j["lim"]), at[i], int(j["cap"]), int(j["base"]),
                             len(j["ranges"]), len(blob), len(bound), int(j["direction"]), 0))
        blob += bound
    return (_lib.Page * len(fit))(*fit), bytes(blob), at, old


class GatherResult(Values):
    """The arrays of okv_gather_out and its totals."""

    def __init__(self, arrays, key_arena, val_arena, o):
        self.__dict__.update(arrays)
        self.key_arena, self.val_arena = key_arena, val_arena
        self.key_bytes, self.val_bytes = int(o.key_bytes), int(o.val_bytes)

    def pairs(self, lo, hi):
        """Rows [lo, hi) as (key, value or None) tuples (host arrays); the arenas are turned
        into bytes once, so a row costs two slices."""
        if getattr(self, "_flat", None) is None:
            self._flat = (self.key_arena.tobytes(), self.val_arena.tobytes(),
                          self.key_pos.tolist(), self.key_len.tolist(), self.val_pos.tolist(),
                          self.val_len.tolist())
        kb, vb, kp, kl, vp, vl = self._flat
        return [(kb[kp[i]:kp[i] + kl[i]], vb[vp[i]:vp[i] + vl[i]] if vl[i] else None)
                for i in range(lo, hi)]

    def key(self, i) -> bytes:
        """Row i's key (host arrays)."""
        p = int(self.key_pos[i])
        return self.key_arena[p:p + int(self.key_len[i])].tobytes()


def gather_rows(owner, sources, src, row, n=None, out=None, arenas=True, key_cap=None,
                val_cap=None) -> GatherResult:
    """okv_gather_rows.  src (int32) and row (int64) are device tensors: a merge's
    outputs; n defaults to their length.  Host mode (out is None): numpy outputs, sized by
    a first call unless key_cap and val_cap are given; arenas=False is that size query
    alone.  Device mode: ``out`` holds device tensors key_pos, key_len, val_pos, val_len
    and optionally key_arena and val_arena (their sizes are the capacities).  Raises
    OkvError (OKV_E_CAPACITY with .result holding the totals)."""
    arr, nsrc = sources if isinstance(sources, tuple) else merge_srcs(sources)
    n = int(src.numel()) if n is None else int(n)
    L = lib()

    def call(arrays, ka, va, kc, vc, flags):
        o = _lib.GatherOut(*[_ptr(arrays.get(k)) for k, _ in _GATHER], _ptr(ka), _ptr(va),
                           int(kc), int(vc), 0, 0)
        rc = L.okv_gather_rows(owner._ctx, arr, nsrc, _ptr(src), _ptr(row), n, C.byref(o), flags)
        return rc, o

    if out is not None:
        ka, va = out.get("key_arena"), out.get("val_arena")
        rc, o = call(out, ka, va, ka.numel() if ka is not None else 0,
                     va.numel() if va is not None else 0, F_DEVICE_PTRS)
        arrays = {k: out.get(k) for k, _ in _GATHER}
    else:
        arrays = {k: np.zeros(n, t) for k, t in _GATHER}
        ka = va = None
        if arenas and (key_cap is None or val_cap is None):
            rc, o = call(arrays, None, None, 0, 0, 0)
            owner._check(rc, "okv_gather_rows")
            key_cap, val_cap = int(o.key_bytes), int(o.val_bytes)
        if arenas:
            ka, va = np.zeros(max(int(key_cap), 1), np.uint8), np.zeros(max(int(val_cap), 1), np.uint8)
            rc, o = call(arrays, ka, va, key_cap, val_cap, 0)
        else:
            rc, o = call(arrays, None, None, 0, 0, 0)
    res = GatherResult(arrays, ka, va, o)
    if rc:
        e = OkvError(rc, f"okv_gather_rows: {owner.error()}")
        e.result = res
        raise e
    return res


__all__ = ["ARENA_SPARE", "GatherResult", "PAGE_MAX_STREAMS", "ResidentRows", "gather_rows",
           "merge_srcs", "pack_pages", "seek_rows"]
