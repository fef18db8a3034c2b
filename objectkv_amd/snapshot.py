"""Go-shaped snapshot reader over device-resident segments and the device merge.

Mirrors /root/reference/snapshot_reader/snapshot_reader.go and
snapshot_iter.go: Reader (NewReader, UpdateSegments, GetRow, GetRange,
RowIter) and Iter (Next, Peek); GetRows is GetRow for a batch of keys in one device
call (okv_snap_get_rows, objectkv_amd/snap.py) over the segments' raw bytes.  The segment index (the two btrees and their
quirky descend-and-stop search, :149-193) and the per-segment Seek positions
are host control logic, restated statement by statement; every block read is
the batched GPU decode and every GetRange merge is okv_merge_rows
(objectkv_amd/csrc/okv_merge.hip).  There is no CPU merge path.  GetRanges is GetRange
for a batch of queries served from the resident segments (objectkv_amd/range.py): the seek
on the device, the merge over windows of limit + slack rows (cut_windows / accept_window),
the result rows gathered on the device.

Segments must be written in key order (the Go writer's stated precondition,
segment_writer.go:78): the merge reads each segment as one sorted row array.
``compact()`` runs decode -> merge -> encode on the device: the compactor the
reference leaves as a stub (sst/compactor.go:3-6), with GetRange's newest-wins
rule as its merge semantics.
"""
from __future__ import annotations

import functools

import numpy as np

from . import _lib
from .sst import COMP_NONE, Decoder, Encoder, OkvError, fetch_metadata

DirectionAscending, DirectionDescending = 0, 1  # segment_row_iter.go:22-25
_RANGE_STATS = ("seeks", "seek_calls", "gather_calls", "rows_merged", "windows_accepted",
                "reruns", "rows_gathered", "merge_calls", "pages_merged")
_GATHER_SOURCES = 60000  # streams of one okv_gather_rows call (it takes 65535 sources)
UnboundStart = None  # segment_reader.go:60
UnboundEnd = b"\xff"  # :62


class SnapshotError(Exception):
    """A Go error value; .kind is the sentinel name (ErrInvalidRange, EOF,
    ErrNoRows, ErrNoNextIndexFound)."""

    def __init__(self, kind, msg=""):
        self.kind = kind
        super().__init__(f"{kind}: {msg}" if msg else kind)


class SnapshotPanic(Exception):
    """Where the Go code panics."""


def _b(x) -> bytes:
    return b"" if x is None else bytes(x)


def _cmp(a, b) -> int:  # bytes.Compare (nil == empty)
    a, b = _b(a), _b(b)
    return (a > b) - (a < b)


class KVPair:
    """sst.KVPair (segment_reader.go:285-288); None is a Go nil slice."""

    __slots__ = ("Key", "Value")

    def __init__(self, Key, Value):
        self.Key, self.Value = Key, Value

    def __repr__(self):
        return f"KVPair({self.Key!r}, {self.Value!r})"


class SegmentRecord:
    """segment_record.go:5-12: ID, Level and the segment's first / last key."""

    def __init__(self, ID: str, Level: int, FirstKey, LastKey):
        self.ID, self.Level, self.FirstKey, self.LastKey = ID, Level, FirstKey, LastKey

    def __repr__(self):
        return f"SegmentRecord({self.ID!r}, L{self.Level})"


# ---- one segment, decoded on the GPU and kept resident ------------------------------


class DeviceSegment:
    """A segment's rows as device SoA (torch tensors) plus the host copy the
    Go-shaped results are built from.  Decoded once with the batched GPU
    decode (okv_decode_blocks)."""

    def __init__(self, decoder: Decoder, data, file_len: int):
        import torch
        seg = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data
        self.md = fetch_metadata(seg, file_len)
        descs = self.md.descs
        d = decoder.decode(seg, descs, self.md.compression)
        if d.status.size and int(np.abs(d.status).max()) != 0:
            raise OkvError(-309, f"segment blocks failed to decode: {np.unique(d.status)}")
        self.h = d
        self.n = int(d.row_start[-1])
        first = [int(d.row_start[b]) for b in range(descs.shape[0])]
        self.block_first_row = np.array(first + [self.n], np.int64)
        self.block_first_key = [self.key(r) if self.block_first_row[b] < self.block_first_row[b + 1]
                                else b"" for b, r in enumerate(first)]
        for a, b in zip(self.block_first_key, self.block_first_key[1:]):
            if _cmp(a, b) >= 0:
                raise NotImplementedError("segment not written in key order (segment_writer.go:78)")
        dev = torch.device("cuda", decoder.device)

        def up(a, dt):
            if a is None or a.size == 0:
                return torch.zeros(16, dtype=dt, device=dev)
            return torch.from_numpy(np.ascontiguousarray(a).view(dt_np[dt])).to(dev)
        dt_np = {torch.uint8: np.uint8, torch.int64: np.int64, torch.int16: np.int16,
                 torch.int32: np.int32}
        self.t = {"key_arena": up(d.key_arena, torch.uint8), "key_off": up(d.key_off, torch.int64),
                  "key_len": up(d.key_len, torch.int16), "val_arena": up(d.val_arena, torch.uint8),
                  "val_off": up(d.val_off, torch.int64), "val_len": up(d.val_len, torch.int32)}

    def key(self, r: int) -> bytes:
        o, l_ = int(self.h.key_off[r]), int(self.h.key_len[r])
        return self.h.key_arena[o:o + l_].tobytes()

    def value(self, r: int):
        o, l_ = int(self.h.val_off[r]), int(self.h.val_len[r])
        return self.h.val_arena[o:o + l_].tobytes() if l_ else None  # Q4: nil

    def _lower(self, key) -> int:  # first row with key >= key
        lo, hi = 0, self.n
        while lo < hi:
            m = (lo + hi) // 2
            if _cmp(self.key(m), key) < 0:
                lo = m + 1
            else:
                hi = m
        return lo

    def _upper(self, key) -> int:  # first row with key > key
        lo, hi = 0, self.n
        while lo < hi:
            m = (lo + hi) // 2
            if _cmp(self.key(m), key) <= 0:
                lo = m + 1
            else:
                hi = m
        return lo

    def stream(self, key, direction):
        """Rows [lo, hi) that RowIter(direction).Seek(key) then Next() yields
        (segment_row_iter.go:102-207), ascending row numbering; descending
        streams are consumed from hi - 1.  Restated on block first keys:
        DescendLessOrEqual keeps walking while the block's FirstKey equals the
        key (:113-116), so a descending seek onto a block's first key starts
        in the block before it and skips that row."""
        fk = self.block_first_key
        nb = len(fk)
        if nb == 0 or self.n == 0:
            return 0, 0
        unbound_start, unbound_end = _b(key) == b"", _b(key) == b"\xff"
        if direction == DirectionAscending:
            if unbound_end:
                return self.n, self.n  # :170-171: parked past the last block
            return self._lower(key), self.n  # the Next loop stops at the first row >= key
        if unbound_start:
            return 0, 0  # :203-206: blockRowIdx -1 below the first block
        if unbound_end:
            return 0, self._upper(key)
        # stat: last block with FirstKey <= key, stepping back once more if equal
        i = -1
        for b in range(nb - 1, -1, -1):
            if _cmp(fk[b], key) <= 0:
                i = b
                if _cmp(key, fk[b]) == 0 and b > 0:
                    i = b - 1
                break
        if i < 0:
            return 0, 0  # key below every block: the Next loop runs to io.EOF
        top = int(self.block_first_row[i + 1])  # the walk starts at block i's last row
        return 0, min(top, self._upper(key))

    def get_row(self, key):  # SegmentReader.GetRow segment_reader.go:362-404
        r = self._lower(key)
        if r < self.n and self.key(r) == _b(key):
            return KVPair(self.key(r), self.value(r))
        raise SnapshotError("ErrNoRows")


# ---- windows: what a GetRange merge has to look at -------------------------------------


def window_size(limit: int) -> int:
    """Rows of each stream a merge for `limit` rows looks at: limit + 1 and a slack that
    lets a page with a few tombstones or duplicate keys still be accepted."""
    return limit + 1 + max(16, limit // 4)


def cut_windows(streams, c, direction):
    """streams [(lo, hi)] cut to at most c rows from the end the iteration starts at:
    ascending [lo, min(hi, lo + c)), descending [max(lo, hi - c), hi).
    -> (windows, frontier): frontier[i] is the row of a truncated stream i that lies
    furthest into the iteration (its last window row), None when the stream was not cut."""
    windows, frontier = [], []
    for lo, hi in streams:
        if direction == DirectionAscending:
            w = (lo, min(hi, lo + c))
            frontier.append(w[1] - 1 if w[1] < hi else None)
        else:
            w = (max(lo, hi - c), hi)
            frontier.append(w[0] if w[0] > lo else None)
        windows.append(w)
    return windows, frontier


def accept_window(frontier_keys, eof, n_rows, limit, last_key, bound, direction) -> bool:
    """Whether the GetRange loop over the windows gave what it gives over the full streams.
    frontier_keys: the keys of cut_windows' frontier rows (truncated streams only); eof: the
    merge ended in io.EOF (OKV_M_EOF); n_rows, last_key: the rows it returned and the last
    one's key; bound: `end` ascending, `start` descending.

    Let F be the frontier key the iteration reaches first.  Every event of the loop at a
    key strictly before F sees the same rows and the same successors as in the full
    streams; a truncated stream can only look run-out at F or beyond.  So the result
    stands when the loop ended before F (the limit-th row lies strictly before F), or when
    F is at or past the bound: past the bound the loop only skips L0 tombstones or breaks,
    and a spurious run-out there happens on a skip and yields io.EOF, which is rejected."""
    if not frontier_keys:
        return True
    if eof:
        return False
    asc = direction == DirectionAscending
    f = min(frontier_keys) if asc else max(frontier_keys)
    if (_cmp(f, bound) >= 0) if asc else (_cmp(f, bound) <= 0):
        return True
    if n_rows < limit:
        return False
    return (_cmp(last_key, f) < 0) if asc else (_cmp(last_key, f) > 0)


# ---- the snapshot reader --------------------------------------------------------------


def _block_range_less(a: SegmentRecord, b: SegmentRecord) -> bool:  # :29-61
    c = _cmp(a.FirstKey, b.FirstKey)
    if c != 0:
        return c < 0
    if len(_b(a.LastKey)) == 0:
        return False
    if len(_b(b.LastKey)) == 0:
        return True
    c = _cmp(a.LastKey, b.LastKey)
    if c != 0:
        return c < 0
    if a.ID == "":
        return False
    if b.ID == "":
        return True
    return a.ID < b.ID


class _Tree:
    """google/btree BTreeG: ReplaceOrInsert / Delete / DescendLessOrEqual."""

    def __init__(self, less):
        self.less, self.items = less, []

    def _key(self):
        return functools.cmp_to_key(lambda a, b: -1 if self.less(a, b) else
                                    (1 if self.less(b, a) else 0))

    def _find(self, it):
        for i, x in enumerate(self.items):
            if not self.less(x, it) and not self.less(it, x):
                return i
        return -1

    def replace_or_insert(self, it):
        i = self._find(it)
        if i >= 0:
            self.items[i] = it
        else:
            self.items.append(it)
            self.items.sort(key=self._key())

    def delete(self, it) -> bool:
        i = self._find(it)
        if i < 0:
            return False
        del self.items[i]
        return True

    def descend_le(self, pivot):
        for x in reversed(self.items):
            if not self.less(pivot, x):
                yield x


class Reader:
    """snapshot_reader.Reader.  factory(record) -> (segment bytes, file length):
    the reference's SegmentReaderFactoryFunc returns a *sst.SegmentReader; here
    the bytes are decoded once on the GPU and kept resident, by segment ID."""

    def __init__(self, factory, decoder: Decoder | None = None):
        self.segmentIDTree = _Tree(lambda a, b: a.ID < b.ID)
        self.blockRangeTree = _Tree(_block_range_less)
        self.readerFactory = factory
        self.decoder = decoder or Decoder(0)
        self._segs: dict[str, DeviceSegment] = {}
        self._raw: dict[str, tuple] = {}  # GetRows: raw bytes, block index and filter by ID
        self._bytes: dict[str, tuple] = {}  # the raw bytes on the device and the metadata by ID
        self._rows: dict = {}             # GetRanges: range.ResidentRows by ID
        self._garena = None               # GetRanges: the gather's device arenas (key, value)
        self.range_stats = dict.fromkeys(_RANGE_STATS, 0)
        self.range_profile = False        # GetRanges: also time seek / merges / gather (events)
        self._pstream = None
        self._snap = None                 # GetRows: the DeviceSnapshot of the current set

    def _seg(self, rec) -> DeviceSegment:
        s = self._segs.get(rec.ID)
        if s is None:
            data, n = self.readerFactory(rec)
            s = self._segs[rec.ID] = DeviceSegment(self.decoder, data, n)
        return s

    def UpdateSegments(self, add, drop):  # :80-96
        for d in drop or []:
            if not self.segmentIDTree.delete(d):
                continue
            self.blockRangeTree.delete(d)
            self._drop(d.ID)
        for a in add or []:
            self.segmentIDTree.replace_or_insert(a)
            self.blockRangeTree.replace_or_insert(a)
            self._drop(a.ID)
        self._snap = None

    def _drop(self, ID):
        for cache in (self._segs, self._raw, self._bytes, self._rows):
            cache.pop(ID, None)

    def _possible_for_key(self, key):  # :149-170
        out = []
        for rec in self.blockRangeTree.descend_le(SegmentRecord("", 0, key, None)):
            in_range = _cmp(key, rec.FirstKey) >= 0 and _cmp(key, rec.LastKey) <= 0
            if not in_range:
                break
            out.append(rec)
        return out

    def _possible_for_range(self, start, end):  # :172-193
        out = []
        for rec in self.blockRangeTree.descend_le(SegmentRecord("", 0, end, None)):
            in_range = not (_cmp(start, rec.LastKey) > 0 or _cmp(end, rec.FirstKey) < 0)
            if not in_range:
                break
            out.append(rec)
        return out

    def GetRow(self, key):  # :98-146
        segs = self._possible_for_key(key)
        segs.sort(key=functools.cmp_to_key(
            lambda a, b: -1 if _getrow_less(a, b) else (1 if _getrow_less(b, a) else 0)))
        for rec in segs:
            try:
                row = self._seg(rec).get_row(key)
            except SnapshotError as e:
                if e.kind == "ErrNoRows":
                    continue
                raise
            if _b(row.Value) == b"" and rec.Level == 0:
                raise SnapshotError("ErrNoRows")  # a delete
            return row.Value
        raise SnapshotError("ErrNoRows")

    def _raw_seg(self, rec):
        """The segment's raw bytes, block index and filter on the device, uploaded once
        per segment ID -> DeviceSnapshot's segment tuple."""
        s = self._raw.get(rec.ID)
        if s is None:
            from .bloom import DeviceBloom
            from .get import DeviceIndex
            t, size, md, bb = self._raw_bytes(rec)
            bloom = DeviceBloom.from_bytes(self.decoder, bb) if bb is not None else None
            s = self._raw[rec.ID] = (t, size, DeviceIndex.from_metadata(self.decoder, md),
                                     bloom, md.compression)
        return s + (rec.Level, rec.ID, rec.FirstKey, rec.LastKey)

    def _raw_bytes(self, rec):
        """The segment's bytes on the device (32 spare bytes after them: the kernels read
        aligned 16-byte lines), uploaded once per segment ID -> (device tensor, byte count,
        metadata, filter bytes or None).  No host copy of the segment is kept."""
        s = self._bytes.get(rec.ID)
        if s is None:
            import torch
            data, n = self.readerFactory(rec)
            raw = np.frombuffer(bytes(data), np.uint8)
            md = fetch_metadata(raw, n)
            t = torch.zeros(raw.size + 32, dtype=torch.uint8,
                            device=torch.device("cuda", self.decoder.device))
            if raw.size:
                t[:raw.size] = torch.from_numpy(raw.copy())
            s = self._bytes[rec.ID] = (t, raw.size, md, _bloom_bytes(raw, n))
        return s

    def _resident(self, rec):
        """The segment's rows on the device (range.ResidentRows), decoded once per segment
        ID.  A block that fails to decode and first keys that do not ascend raise what
        DeviceSegment raises."""
        r = self._rows.get(rec.ID)
        if r is None:
            from .range import ResidentRows
            t, size, md, _bb = self._raw_bytes(rec)
            r = ResidentRows(self.decoder, t, size, md)
            if r.status.size and int(np.abs(r.status).max()) != 0:
                raise OkvError(-309, f"segment blocks failed to decode: {np.unique(r.status)}")
            for a, b in zip(md.first_keys, md.first_keys[1:]):
                if _cmp(a, b) >= 0:
                    raise NotImplementedError(
                        "segment not written in key order (segment_writer.go:78)")
            self._rows[rec.ID] = r
        return r

    def _device_snapshot(self):
        """The DeviceSnapshot of blockRangeTree, rebuilt when the segment set changed; None
        when a segment carries a filter the device refuses (OKV_E_ARG)."""
        if self._snap is None:
            from .snap import DeviceSnapshot
            try:
                self._snap = DeviceSnapshot(self.decoder,
                                            [self._raw_seg(r) for r in self.blockRangeTree.items])
            except OkvError as e:
                if e.code != _lib.OKV_E_ARG:
                    raise
                self._snap = False
        return self._snap or None

    def _get_row_outcome(self, key):
        try:
            return self.GetRow(key)
        except (SnapshotError, SnapshotPanic) as e:
            return e

    def GetRows(self, keys):
        """GetRow for every key in one device call (okv_snap_get_rows): per key the value
        GetRow returns (None for nil), or the SnapshotError / SnapshotPanic Go's GetRow
        would give (returned, not raised).  zstd segments answer in the same call
        (OKV_F_GET_ZSTD: their touched blocks are inflated on the device).  Keys the device
        hands back (OKV_SNAP_FALLBACK) and snapshots with a filter the device refuses go
        through GetRow."""
        from . import snap as S
        ks = [_b(k) for k in keys]
        if not ks:
            return []
        ds = self._device_snapshot()
        if ds is None:
            return [self._get_row_outcome(k) for k in ks]
        res = S.snap_get_rows(self.decoder, ds, ks, zstd=True)
        out = []
        for i, k in enumerate(ks):
            st = int(res.state[i])
            if st == S.SNAP_FOUND:
                out.append(res.value(i))
            elif st in (S.SNAP_NO_ROWS, S.SNAP_DELETED):
                out.append(SnapshotError("ErrNoRows"))
            elif st == S.SNAP_SEG_ERROR:
                out.append(_block_error(int(res.blk_status[i]), ds.ids[int(res.seg[i])]))
            else:
                out.append(self._get_row_outcome(k))
        return out

    def GetRange(self, start, end, limit, direction):  # :214-372
        if _cmp(start, end) >= 0:
            raise SnapshotError("ErrInvalidRange", "end must be strictly greater than start")
        segs = self._possible_for_range(start, end)
        if not segs:
            return None
        segs.sort(key=functools.cmp_to_key(
            lambda a, b: -1 if _getrange_less(a, b, direction) else
            (1 if _getrange_less(b, a, direction) else 0)))
        start_range = end if direction == DirectionDescending else start
        srcs, dsegs = [], []
        for rec in segs:
            ds = self._seg(rec)
            lo, hi = ds.stream(start_range, direction)
            if hi <= lo:  # RowIter.Next after Seek returns io.EOF (:276-280)
                raise SnapshotError("EOF", f"error in sst.RowIter.Next() after start range for "
                                           f"segment {rec.ID}")
            srcs.append((ds.t, lo, hi, rec.Level))
            dsegs.append(ds)
        if limit < 0:
            raise SnapshotPanic("makeslice: len out of range")
        bound = end if direction == DirectionAscending else start
        if limit == 0:
            # rows[0] = row (:340) panics only once a row is appended; a loop
            # that breaks or errors first returns normally
            rows = self._merge(srcs, dsegs, _lib.MERGE_GETRANGE, direction, 1, _b(bound))
            if rows:
                raise SnapshotPanic("index out of range [0] with length 0")
            return rows
        return self._merge(srcs, dsegs, _lib.MERGE_GETRANGE, direction, limit, _b(bound))

    def _merge(self, srcs, dsegs, mode, direction, limit, bound):
        import torch
        dev = torch.device("cuda", self.decoder.device)
        cap = min(sum(hi - lo for _t, lo, hi, _l in srcs), limit if limit > 0 else 1 << 62)
        out = {"src": torch.empty(max(cap, 1), dtype=torch.int32, device=dev),
               "row": torch.empty(max(cap, 1), dtype=torch.int64, device=dev)}
        mo = self.decoder.merge_device(srcs, mode, direction, limit, bound, out=out,
                                       row_cap=cap)
        if mo.status == _lib.M_EOF:
            raise SnapshotError("EOF", "error in sst.RowIter.Next() rolling forward")
        n = int(mo.n_rows)
        src = out["src"][:n].cpu().numpy()
        row = out["row"][:n].cpu().numpy()
        return [KVPair(dsegs[s].key(int(r)), dsegs[s].value(int(r))) for s, r in zip(src, row)]

    # -- GetRange for a batch of queries, from the resident segments ------------------

    def GetRanges(self, queries):
        """GetRange for every (start, end, limit, direction) of queries: per query the list
        of KVPair, None (no candidate segment), or the SnapshotError / SnapshotPanic Go's
        GetRange would give (returned, not raised).  One okv_seek_rows call positions every
        (query, candidate) stream; each query's merge runs over windows of
        window_size(limit) rows -- every page of the batch in one okv_merge_pages call, a
        merge of more than PAGE_MAX_ROWS rows by okv_merge_rows -- and is run again over
        the whole streams only when accept_window refuses its result; one okv_gather_rows packs the rows of the whole
        batch on the device and they come back once per batch (the row arrays, the key arena,
        the value arena), not per row.  More than 64 candidates of one query is the merge's
        OKV_E_ARG, as in GetRange.  range_stats counts the call:
        seeks (triples), seek_calls, gather_calls, rows_merged (rows given to merges),
        windows_accepted (queries with a cut stream whose windowed result stood), reruns,
        rows_gathered, merge_calls (okv_merge_pages and okv_merge_rows calls), pages_merged
        (merges that went through okv_merge_pages).  With range_profile set it also holds seek_ms, merge_ms and gather_ms:
        device events on the decoder's stream around the three steps."""
        from . import range as RG
        st = self.range_stats = dict.fromkeys(_RANGE_STATS, 0)
        if self.range_profile:
            st.update(seek_ms=0.0, merge_ms=0.0, gather_ms=0.0)
        results = [None] * len(queries)
        plans, sources, src_at = [], [], {}
        keys, src_of, dirs = [], [], []
        for qi, (start, end, limit, direction) in enumerate(queries):
            if _cmp(start, end) >= 0:
                results[qi] = SnapshotError("ErrInvalidRange",
                                            "end must be strictly greater than start")
                continue
            segs = self._possible_for_range(start, end)
            if not segs:
                continue
            segs.sort(key=functools.cmp_to_key(
                lambda a, b: -1 if _getrange_less(a, b, direction) else
                (1 if _getrange_less(b, a, direction) else 0)))
            start_range = end if direction == DirectionDescending else start
            for rec in segs:
                if rec.ID not in src_at:
                    src_at[rec.ID] = len(sources)
                    sources.append(self._resident(rec))
                keys.append(_b(start_range))
                src_of.append(src_at[rec.ID])
                dirs.append(direction)
            plans.append((qi, segs, len(keys) - len(segs)))
        if not plans:
            return results
        t0 = self._mark()
        lo, hi = RG.seek_rows(self.decoder, sources, keys, src_of, dirs)
        self._span("seek_ms", t0)
        st["seeks"], st["seek_calls"] = len(keys), 1

        jobs = []  # per query still to merge: its streams, windows and frontier rows
        for qi, segs, at in plans:
            limit, direction = queries[qi][2], queries[qi][3]
            streams = [(int(lo[at + j]), int(hi[at + j])) for j in range(len(segs))]
            empty = [rec for rec, (a, b) in zip(segs, streams) if b <= a]
            if empty:  # RowIter.Next after Seek returns io.EOF (:276-280)
                results[qi] = SnapshotError("EOF", f"error in sst.RowIter.Next() after start "
                                                   f"range for segment {empty[0].ID}")
                continue
            if limit < 0:
                results[qi] = SnapshotPanic("makeslice: len out of range")
                continue
            lim = limit if limit > 0 else 1  # limit 0 panics only once a row is appended
            windows, frontier = cut_windows(streams, window_size(lim), direction)
            jobs.append({"qi": qi, "segs": segs, "src": src_of[at:at + len(segs)], "lim": lim,
                         "streams": streams, "windows": windows, "frontier": frontier})
        self._merge_jobs(jobs, sources, queries, results, windowed=True)
        again = [j for j in jobs if j.get("rerun")]
        st["reruns"] = len(again)
        self._merge_jobs(again, sources, queries, results, windowed=False)
        return results

    def _merge_jobs(self, jobs, sources, queries, results, windowed):
        """_merge_group over groups of jobs whose streams fit one gather's source list."""
        group, streams = [], 0
        for j in jobs:
            if group and streams + len(j["src"]) > _GATHER_SOURCES:
                self._merge_group(group, sources, queries, results, windowed)
                group, streams = [], 0
            group.append(j)
            streams += len(j["src"])
        if group:
            self._merge_group(group, sources, queries, results, windowed)

    def _merge_group(self, jobs, sources, queries, results, windowed):
        """The jobs' merges into slices of one device src / row array, then one gather and
        one copy back.  Every job that fits a page (range.pack_pages) is merged by one
        okv_merge_pages call; the others (more than PAGE_MAX_ROWS rows: usually the whole
        streams of the rerun) by one okv_merge_rows each.  The gather's sources are the
        jobs' streams one after the other: a page's src already counts in them, a single
        merge's needs the job's base added.  A job's slice is its cap slots at a fixed
        place, the slots it leaves unused are empty rows of the gather.  windowed: over
        the jobs' windows, with the frontier rows added to the gather list; a refused
        result marks the job for the rerun."""
        import torch
        from . import range as RG
        st = self.range_stats
        dev = torch.device("cuda", self.decoder.device)
        extra, gsrc = [], []  # the frontier rows, in front of the merges' rows
        for j in jobs:
            start, end, _l, j["direction"] = queries[j["qi"]]
            j["bound"] = _b(end if j["direction"] == DirectionAscending else start)
            j["ranges"] = j["windows"] if windowed else j["streams"]
            j["base"], j["fr_at"] = len(gsrc), len(extra)
            gsrc += [sources[s] for s in j["src"]]
            if windowed:
                extra += [(j["base"] + i, r) for i, r in enumerate(j["frontier"]) if r is not None]
            j["cap"] = min(sum(b - a for a, b in j["ranges"]), j["lim"])
            st["rows_merged"] += sum(b - a for a, b in j["ranges"])
        ne = len(extra)
        pages, bounds, ats, old = RG.pack_pages(jobs, ne)
        total = ne + sum(j["cap"] for j in jobs)
        d_src = torch.full((max(total, 1),), -1, dtype=torch.int32, device=dev)
        d_row = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
        if ne:  # one upload
            up = torch.tensor([e[0] for e in extra] + [e[1] for e in extra],
                              dtype=torch.int64).to(dev)
            d_src[:ne] = up[:ne].to(torch.int32)
            d_row[:ne] = up[ne:]
        # torch filled the arrays on its stream; the decoder's kernels run on another
        torch.cuda.current_stream(dev).synchronize()
        t0 = self._mark()
        for j, at in zip(jobs, ats):
            j["at"] = at
        gsrcs = RG.merge_srcs(gsrc)  # the pages' sources and the gather's
        if len(pages):
            srcs = gsrcs[0]
            for j in jobs:
                for i, (rec, (a, b)) in enumerate(zip(j["segs"], j["ranges"])):
                    m = srcs[j["base"] + i]
                    m.row_lo, m.row_hi, m.level = a, b, rec.Level
            n_rows, _nu, status = self.decoder.merge_pages_device(
                gsrcs, pages, bounds, {"src": d_src, "row": d_row})
            st["merge_calls"] += 1
            st["pages_merged"] += len(pages)
            skip = set(old)
            paged = [j for i, j in enumerate(jobs) if i not in skip]
            for j, n, s in zip(paged, n_rows.tolist(), status.tolist()):
                if s not in (0, _lib.M_EOF):  # a page fits by pack_pages, its rows by cap
                    raise OkvError(_lib.OKV_E_ARG, f"okv_merge_pages: page status {s}")
                j["eof"] = s == _lib.M_EOF
                j["n"] = 0 if j["eof"] else n
        for i in old:
            j = jobs[i]
            srcs = [(sources[s].t, a, b, rec.Level)
                    for s, rec, (a, b) in zip(j["src"], j["segs"], j["ranges"])]
            at = j["at"]
            out = {"src": d_src[at:at + j["cap"]], "row": d_row[at:at + j["cap"]]}
            mo = self.decoder.merge_device(srcs, _lib.MERGE_GETRANGE, j["direction"], j["lim"],
                                           j["bound"], out=out, row_cap=j["cap"])
            st["merge_calls"] += 1
            j["eof"] = mo.status == _lib.M_EOF
            j["n"] = 0 if j["eof"] else int(mo.n_rows)
            if j["n"] and j["base"]:  # the merge counts its inputs from 0
                d_src[at:at + j["n"]] += j["base"]
        torch.cuda.current_stream(dev).synchronize()
        t1 = self._span("merge_ms", t0)
        pos = ne + sum(j["n"] for j in jobs)  # real rows; the gather also sees the empty slots
        g = self._gather(gsrcs, d_src, d_row, total)
        self._span("gather_ms", t1)
        st["gather_calls"] += 1
        st["rows_gathered"] += pos
        for j in jobs:
            qi = j["qi"]
            direction, limit = queries[qi][3], queries[qi][2]
            bound = _b(queries[qi][1] if direction == DirectionAscending else queries[qi][0])
            if windowed:
                nf = sum(r is not None for r in j["frontier"])
                fkeys = [g.key(j["fr_at"] + i) for i in range(nf)]
                last = g.key(j["at"] + j["n"] - 1) if j["n"] else None
                if not accept_window(fkeys, j["eof"], j["n"], j["lim"], last, bound, direction):
                    j["rerun"] = True
                    continue
                st["windows_accepted"] += bool(fkeys)
            if j["eof"]:
                results[qi] = SnapshotError("EOF", "error in sst.RowIter.Next() rolling forward")
            elif limit == 0 and j["n"]:
                results[qi] = SnapshotPanic("index out of range [0] with length 0")
            else:
                results[qi] = [KVPair(k, v) for k, v in g.pairs(j["at"], j["at"] + j["n"])]

    def _mark(self):
        """range_profile: an event recorded on the decoder's stream now, else None."""
        if not self.range_profile:
            return None
        import torch
        if self._pstream is None:
            self._pstream = torch.cuda.ExternalStream(self.decoder.stream)
        e = torch.cuda.Event(enable_timing=True)
        e.record(self._pstream)
        return e

    def _span(self, name, since):
        """range_profile: add the device time since the event to range_stats[name]."""
        e = self._mark()
        if e is not None:
            e.synchronize()
            self.range_stats[name] += since.elapsed_time(e)
        return e

    def _gather(self, srcs, d_src, d_row, n):
        """okv_gather_rows (sources srcs: range.merge_srcs) of rows (d_src, d_row)[:n] into the reader's device arenas (grown
        when the call reports OKV_E_CAPACITY), copied back -> range.GatherResult on the host.
        The four per-row arrays are one device buffer: one copy brings them back."""
        import torch
        from . import range as RG
        dev = d_src.device
        m = max(n, 1)
        buf = torch.empty(24 * m, dtype=torch.uint8, device=dev)
        out = {"key_pos": buf[:8 * m].view(torch.int64), "val_pos": buf[8 * m:16 * m].view(torch.int64),
               "val_len": buf[16 * m:20 * m].view(torch.int32),
               "key_len": buf[20 * m:22 * m].view(torch.int16)}
        if self._garena is None:
            self._garena = (torch.empty(1 << 16, dtype=torch.uint8, device=dev),
                            torch.empty(1 << 20, dtype=torch.uint8, device=dev))
        for _attempt in range(2):
            out["key_arena"], out["val_arena"] = self._garena
            try:
                g = RG.gather_rows(self.decoder, srcs, d_src, d_row, n, out=out)
                break
            except OkvError as e:
                if e.code != _lib.OKV_E_CAPACITY or _attempt:
                    raise
                need = e.result
                self._garena = (
                    torch.empty(max(need.key_bytes * 3 // 2, 1 << 16), dtype=torch.uint8, device=dev),
                    torch.empty(max(need.val_bytes * 3 // 2, 1 << 20), dtype=torch.uint8, device=dev))
        h = buf.cpu().numpy()
        host = {"key_pos": h[:8 * m].view(np.uint64)[:n], "val_pos": h[8 * m:16 * m].view(np.uint64)[:n],
                "val_len": h[16 * m:20 * m].view(np.uint32)[:n],
                "key_len": h[20 * m:22 * m].view(np.uint16)[:n]}
        return RG.GatherResult(host, out["key_arena"][:g.key_bytes].cpu().numpy(),
                               out["val_arena"][:g.val_bytes].cpu().numpy(), g)

    def RowIter(self, start, direction, bufferSize=100, resident=False):  # :430-443
        """resident: the Iter pages through GetRanges (the resident segments) instead of
        GetRange."""
        return Iter(self, start, direction, bufferSize, resident)


def _bloom_bytes(raw, file_len):
    """The filter bytes of the segment's meta block (BloomFilter.WriteTo), or None."""
    import ctypes as C
    L = _lib.lib()
    h = C.c_void_p()
    if L.okv_meta_fetch(raw.ctypes.data, raw.size, file_len, C.byref(h)):
        return None
    try:
        n = C.c_uint64()
        p = L.okv_meta_bloom_bytes(h, C.byref(n))
        return C.string_at(p, n.value) if p else None
    finally:
        L.okv_meta_free(h)


def _block_error(blk_status, seg_id):
    """ReadBlockWithStat's failure (segment_reader.go:303-352) as GetRow passes it on."""
    if blk_status == _lib.BLK_PANIC:
        return SnapshotPanic(f"mustReadBytes: ErrUnexpectedBytesRead in segment {seg_id}")
    if blk_status == _lib.BLK_ZSTD_ERROR:  # zstd.NewReader / io.Copy (:321-330)
        return SnapshotError("ZstdError", f"inflating a block of segment {seg_id}")
    kind = "EOF" if blk_status == _lib.BLK_EOF else "ErrUnexpectedBytesRead"
    return SnapshotError(kind, f"reading a block of segment {seg_id}")


def _getrow_less(x, y):  # :103-110
    if x.Level != y.Level:
        return x.Level < y.Level
    return x.ID > y.ID


def _getrange_less(x, y, direction):  # :235-254
    if x.Level != y.Level:
        return x.Level < y.Level
    if x.Level == 0 and y.Level == 0:
        return x.ID > y.ID
    if direction == DirectionAscending:
        return _cmp(x.FirstKey, y.FirstKey) < 0
    return _cmp(x.LastKey, y.LastKey) > 0


class Iter:
    """snapshot_iter.go:11-116: pages through GetRange."""

    def __init__(self, reader, start, direction, bufferSize, resident=False):
        self.reader, self.lastKey, self.direction = reader, start, direction
        self.bufferSize, self.rowBuffer, self.done = bufferSize, [], False
        self.resident = resident

    def Next(self):  # :37-47
        self._check_load()
        return self.rowBuffer.pop(0)

    def Peek(self):  # :51-61
        self._check_load()
        return self.rowBuffer[0]

    def _check_load(self):  # :65-108
        if self.rowBuffer:
            return
        if self.done:
            raise SnapshotError("EOF")
        if self.direction == DirectionDescending:
            s, e = UnboundStart, self.lastKey
        else:
            s, e = self.lastKey, UnboundEnd
        if self.resident:
            rows = self.reader.GetRanges([(s, e, self.bufferSize, self.direction)])[0]
            if isinstance(rows, Exception):
                raise rows
        else:
            rows = self.reader.GetRange(s, e, self.bufferSize, self.direction)
        if not rows:
            self.done = True
            raise SnapshotError("EOF")
        self.rowBuffer = [r for i, r in enumerate(rows)
                          if not (i == 0 and _b(r.Key) == _b(self.lastKey))]
        if not self.rowBuffer:
            raise SnapshotPanic("nil pointer dereference (list.Back() of an empty list)")
        self.lastKey = self.rowBuffer[-1].Key


# ---- compaction: decode -> merge -> encode on the device ---------------------------------


def _merge_all(segments, encoder, drop_tombstones, direction):
    """compact()'s merge step: every key's owning row of the resident segments, as device
    row arrays over the inputs' arenas.  -> (rows, n_rows, key span, value span, device)."""
    import torch
    srcs = [(ds.t, 0, ds.n, lvl) for ds, lvl in segments]
    dev = torch.device("cuda", encoder.device)
    kb = min(int(ds.t["key_arena"].data_ptr()) for ds, _ in segments)
    vb = min(int(ds.t["val_arena"].data_ptr()) for ds, _ in segments)
    cap = sum(ds.n for ds, _ in segments)
    out = {"key_off": torch.empty(cap, dtype=torch.int64, device=dev),
           "key_len": torch.empty(cap, dtype=torch.int16, device=dev),
           "val_off": torch.empty(cap, dtype=torch.int64, device=dev),
           "val_len": torch.empty(cap, dtype=torch.int32, device=dev)}
    mo = encoder.merge_device(srcs, _lib.MERGE_ALL, direction, 0, None, drop_tombstones, out,
                              kb, vb, cap)
    n = int(mo.n_rows)
    kspan = max(int(ds.t["key_arena"].data_ptr()) + ds.t["key_arena"].numel()
                for ds, _ in segments) - kb
    vspan = max(int(ds.t["val_arena"].data_ptr()) + ds.t["val_arena"].numel()
                for ds, _ in segments) - vb
    rows = {"key_arena": _Addr(kb), "key_off": out["key_off"], "key_len": out["key_len"],
            "val_arena": _Addr(vb), "val_off": out["val_off"], "val_len": out["val_len"]}
    return rows, n, kspan, vspan, dev


def compact(segments, encoder: Encoder, drop_tombstones=True, threshold=3584, block_size=4096,
            direction=DirectionAscending, zstd=False, zstd_huffman=False,
            zstd_huffman_fse=False):
    """Merge resident segments (DeviceSegment, level) in priority order (newest
    first) into one new segment, on the GPU: every key's owning row (GetRange's
    rule, :294-331), L0 tombstones dropped when drop_tombstones.  zstd: write the
    output segment zstd-compressed with the device encoder (OKV_F_ZSTD_NATIVE:
    its own frames, blocks cut on raw lengths); zstd_huffman: with zstd, Huffman-coded
    literals where they are smaller (OKV_F_ZSTD_HUFFMAN); zstd_huffman_fse: with
    zstd_huffman, FSE-compressed weights (OKV_F_ZSTD_HUF_FSE).  Returns the Compacted result
    (segment bytes + block index)."""
    import torch
    rows, n, kspan, vspan, dev = _merge_all(segments, encoder, drop_tombstones, direction)
    comp = _lib.COMP_ZSTD if zstd else COMP_NONE
    try:  # size query (zero capacities; with zstd file_bytes is an upper bound)
        encoder.encode_device(rows, n, {}, threshold, block_size, comp, False,
                              key_arena_bytes=kspan, val_arena_bytes=vspan, zstd_native=zstd,
                              zstd_huffman=zstd_huffman, zstd_huffman_fse=zstd_huffman_fse)
        raise AssertionError("size query must report OKV_E_CAPACITY")
    except OkvError as e:
        if e.code != _lib.OKV_E_CAPACITY:
            raise
        need = e.out
    nb = int(need.n_blocks)
    eout = {"seg": torch.empty(int(need.file_bytes) + 64, dtype=torch.uint8, device=dev),
            "first_row": torch.empty(nb + 1, dtype=torch.int64, device=dev),
            "desc": torch.empty((nb, 4), dtype=torch.int64, device=dev),
            "hash": torch.empty(nb, dtype=torch.int64, device=dev)}
    eo = encoder.encode_device(rows, n, eout, threshold, block_size, comp, False,
                               key_arena_bytes=kspan, val_arena_bytes=vspan, zstd_native=zstd,
                               zstd_huffman=zstd_huffman, zstd_huffman_fse=zstd_huffman_fse)
    return Compacted(eout["seg"][:int(eo.file_bytes)].cpu().numpy(), int(eo.file_bytes), n,
                     int(eo.n_blocks), eout, eo)


class _Addr:
    """A raw device address where the encode wrapper expects a tensor."""

    def __init__(self, a):
        self.a = a

    def data_ptr(self):
        return self.a


class Compacted:
    """compact() result: the new segment's bytes (host), file length, rows,
    blocks, and the device outputs (seg, first_row, desc, hash)."""

    def __init__(self, seg, file_bytes, n_rows, n_blocks, dev_out, eo):
        self.seg, self.file_bytes, self.n_rows, self.n_blocks = seg, file_bytes, n_rows, n_blocks
        self.dev_out, self.eo = dev_out, eo


class CompactedSegment:
    """One output segment of compact_split(): the file's bytes (host), its rows and blocks,
    and FirstKey / LastKey for its SegmentRecord."""

    def __init__(self, seg, n_rows, n_blocks, FirstKey, LastKey):
        self.seg, self.file_bytes = seg, int(seg.size)
        self.n_rows, self.n_blocks = n_rows, n_blocks
        self.FirstKey, self.LastKey = FirstKey, LastKey

    def record(self, ID: str, Level: int = 1) -> SegmentRecord:
        return SegmentRecord(ID, Level, self.FirstKey, self.LastKey)


def compact_split(segments, encoder: Encoder, drop_tombstones=True, threshold=3584,
                  block_size=4096, split_bytes=1_000_000, split_rows=100_000, bloom=None):
    """compact()'s merge, then the range-split encode (okv_encode_split): the output is cut
    into segments by the reference's thresholds (sst/compaction_range.go: 1 000 000 bytes,
    100 000 rows), every segment with its own meta block, trailer and -- bloom=(m, k) -- its
    own filter, from one device call.  Returns the list of CompactedSegment, in key order
    (empty when no row survives the merge)."""
    rows, n, kspan, vspan, _dev = _merge_all(segments, encoder, drop_tombstones,
                                             DirectionAscending)
    if n == 0:
        return []
    res = encoder.encode_split_device(rows, n, {}, threshold, block_size,
                                      key_arena_bytes=kspan, val_arena_bytes=vspan,
                                      split_bytes=split_bytes, split_rows=split_rows,
                                      bloom=bloom)
    out = []
    for s, g in enumerate(res.segments):
        fk, lk = res.record(s)
        out.append(CompactedSegment(np.frombuffer(res.file(s), np.uint8), g.n_rows, g.n_blocks,
                                    fk, lk))
    return out
