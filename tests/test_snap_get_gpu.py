"""Snapshot GetRows on the device (okv_snap_*) against the oracle: per key
the outcome of snapshot_oracle.Reader.GetRow over pyoracle.SegmentReader -- the candidate
walk with its stop-at-first-miss quirk, the priority order, each candidate's bloom probe,
floor block and row search, tombstones and error precedence -- for the raw
okv_snap_get_rows outputs and for snapshot.Reader.GetRows."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib, snap as S
from objectkv_amd import snapshot as SN
from objectkv_amd.bloom import pack_keys
from oracle import bloom_ref as B
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO
from tests import snapshot_cases as SC

pytestmark = pytest.mark.gpu

NONE32 = 0xFFFFFFFF
FOUND, NO_ROWS, DELETED, SEG_ERROR, FALLBACK = range(5)


def _read_status(d, seg_len):
    """segment_reader.go:303-316 before any record is read: Seek, make, Read."""
    off, bs = int(d[0]), int(d[1])
    if off >= 2**63:
        return _lib.BLK_EOF
    if bs > 2**48:
        return _lib.BLK_PANIC
    if off >= seg_len:
        return _lib.BLK_EOF
    if seg_len - off < bs:
        return _lib.BLK_SHORT
    return _lib.BLK_OK


def _write(rows, bloom=None, threshold=None, block_size=None):
    kw = {}
    if threshold is not None:
        kw = dict(DataBlockThresholdBytes=threshold, DataBlockSize=block_size)
    w = P.SegmentWriter(P.SegmentWriterOptions(BloomFilter=bloom, **kw))
    for k, v in rows:
        w.WriteRow(k, v)
    n, meta = w.Close()
    return bytes(w.external), n, meta


def _seg(sid, lvl, rows, **kw):
    return (sid, lvl) + _write(rows, **kw)


def _rows_of(data, n):
    rd = P.SegmentReader(data, n)
    md = rd.FetchAndLoadMetadata()
    out = []
    for st in md.entries:
        out += [(P._b(r.Key), P._b(r.Value)) for r in rd.ReadBlockWithStat(st) or []]
    return out


def _with_filters(segs):
    """Every segment rewritten with a small filter over its own keys."""
    out = []
    for sid, lvl, data, n, _meta in segs:
        out.append(_seg(sid, lvl, _rows_of(data, n), bloom=B.BloomFilter(2048, 3)))
    return out


class Oracle:
    """One snapshot as the oracle sees it: snapshot_oracle.Reader over
    pyoracle.SegmentReaders, and the expected raw outcome of a key built from them."""

    def __init__(self, segs):
        self.segs = segs
        self.data = {sid: (d, n) for sid, _l, d, n, _m in segs}
        self.readers = {sid: P.SegmentReader(d, n) for sid, _l, d, n, _m in segs}
        self.orc = SO.Reader(lambda rec: self.readers[rec.ID])
        self.orecs = []
        for sid, lvl, _d, _n, meta in segs:
            pmd = P.bytes_to_metadata(meta)
            self.orecs.append(SO.SegmentRecord(sid, lvl, pmd.FirstKey, pmd.LastKey))
        self.orc.UpdateSegments(self.orecs, None)

    # ---- the expected raw outcome, from the oracle's parts -------------------------
    def holds(self, sid, key):
        try:
            self.readers[sid].GetRow(key)
            return True
        except (P.GoError, P.GoPanic):
            return False

    def expect(self, key, blocks=None, classes=None):
        """(state, segment ID, blk_status, value), Go's loop (:104-149) over the oracle's
        candidates and SegmentReaders; `blocks` collects the (segment, floor block)
        pairs the device stages -- of every candidate, consulted or not."""
        cands = sorted(self.orc.getPossibleSegmentsForKey(key),
                       key=functools.cmp_to_key(SO._getrow_cmp))
        answer, bloom_neg_before = None, False
        for rec in cands:
            rd = self.readers[rec.ID]
            md = rd._md()
            if md.BloomFilter is not None and not md._bloom.test(P._b(key)):
                bloom_neg_before = bloom_neg_before or answer is None
                continue
            floor = md.BlockIndex.descend_le(key)
            if not floor:
                continue
            st = floor[0]
            rs = _read_status(st.desc(), len(rd.data))
            stageable = rs == _lib.BLK_OK and md.compression != P.COMP_ZSTD and st.BlockSize <= 65536
            if stageable and blocks is not None:
                blocks.add((rec.ID, st.Offset))
            if answer is not None:
                continue
            if rs != _lib.BLK_OK:
                answer = (SEG_ERROR, rec.ID, rs, None)
            elif not stageable:
                answer = (FALLBACK, rec.ID, 0, None)
            else:
                try:
                    row = rd.GetRow(key)
                except P.GoPanic:
                    answer = (SEG_ERROR, rec.ID, _lib.BLK_PANIC, None)
                except P.GoError as e:
                    assert e.kind == P.ErrNoRows, e
                    continue
                else:
                    if not P._b(row.Value) and rec.Level == 0:
                        answer = (DELETED, rec.ID, 0, None)
                    else:
                        answer = (FOUND, rec.ID, 0, row.Value)
                    if classes is not None and bloom_neg_before and answer[0] == FOUND:
                        classes.add("bloom-negative newer, found older")
        if answer is None:
            answer = (NO_ROWS, None, 0, None)
        if classes is not None:
            holders = [r for r in cands if self.holds(r.ID, key)]
            if answer[0] == FOUND:
                classes.add("found")
            if answer[0] == DELETED:
                classes.add("tombstone")
            if len(holders) >= 2 and answer[0] in (FOUND, DELETED) and answer[1] == holders[0].ID:
                classes.add("shadowed")
            if answer[0] == NO_ROWS and any(self.holds(r.ID, key)
                                            for r in self.orc.blockRangeTree.items if r not in cands):
                classes.add("hidden")
        return answer, len(cands)


class Env(Oracle):
    """... and twice on the device: the raw objects (DeviceSnapshot) and snapshot.Reader."""

    def __init__(self, decoder, segs):
        super().__init__(segs)
        self.dec = decoder
        self.dev = SN.Reader(lambda rec: self.data[rec.ID], decoder)
        self.drecs, self.tuples = [], []
        for sid, lvl, d, n, meta in segs:
            pmd = P.bytes_to_metadata(meta)
            self.drecs.append(SN.SegmentRecord(sid, lvl, pmd.FirstKey, pmd.LastKey))
            md = okv.bytes_to_metadata(meta)
            t = torch.frombuffer(bytearray(d) + bytearray(32), dtype=torch.uint8).cuda()
            ix = okv.DeviceIndex.from_metadata(decoder, md)
            bl = okv.DeviceBloom.from_bytes(decoder, pmd.BloomFilter) \
                if pmd.BloomFilter is not None else None
            self.tuples.append((t, len(d), ix, bl, md.compression, lvl, sid, pmd.FirstKey,
                                pmd.LastKey))
        self.dev.UpdateSegments(self.drecs, None)
        self.snap = okv.DeviceSnapshot(decoder, self.tuples)

    def drop(self, i):
        self.orc.UpdateSegments(None, [self.orecs[i]])
        self.dev.UpdateSegments(None, [self.drecs[i]])
        self.snap.close()
        self.snap = okv.DeviceSnapshot(self.dec, self.tuples[:i] + self.tuples[i + 1:])

    def close(self):
        self.snap.close()
        for t in self.tuples:
            t[2].close()
            if t[3] is not None:
                t[3].close()


def _outcome(fn):
    try:
        v = fn()
    except (P.GoError, SN.SnapshotError) as e:
        return ("err", e.kind)
    except (P.GoPanic, SN.SnapshotPanic):
        return ("panic",)
    return ("value", v)


def _returned(x):
    if isinstance(x, SN.SnapshotError):
        return ("err", x.kind)
    if isinstance(x, SN.SnapshotPanic):
        return ("panic",)
    return ("value", x)


def _check(env, keys, classes=None, reader=True):
    """The raw outputs and Reader.GetRows against the oracle -> the raw result."""
    res = S.snap_get_rows(env.dec, env.snap, keys)
    assert env.dec.last_path() == _lib.PATH_SNAP_GET
    blocks, pairs, nf, nd, nfb, pos = set(), 0, 0, 0, 0, 0
    for i, k in enumerate(keys):
        (st, sid, bst, val), nc = env.expect(k, blocks, classes)
        pairs += nc
        got_id = None if int(res.seg[i]) == NONE32 else env.snap.ids[int(res.seg[i])]
        assert (int(res.state[i]), got_id, int(res.blk_status[i])) == (st, sid, bst), (k, nc)
        want = _outcome(lambda: env.orc.GetRow(k)) if st != FALLBACK else None
        if st == FOUND:
            assert want == ("value", val) and res.value(i) == val, k
            assert int(res.val_len[i]) == len(P._b(val)) and int(res.val_pos[i]) == pos
            off = int(res.val_off[i])
            assert env.data[sid][0][off:off + len(P._b(val))] == P._b(val), k
            pos += (len(P._b(val)) + 15) // 16 * 16
        else:
            assert int(res.val_len[i]) == 0 and int(res.val_off[i]) == 0
            if st in (NO_ROWS, DELETED):
                assert want == ("err", P.ErrNoRows), k
                assert (int(res.entry[i]) == NONE32) == (st == NO_ROWS)
            elif st == SEG_ERROR:
                assert want[0] in ("err", "panic") and want != ("err", P.ErrNoRows), k
                assert (want == ("panic",)) == (bst == _lib.BLK_PANIC)
        nf, nd, nfb = nf + (st == FOUND), nd + (st == DELETED), nfb + (st == FALLBACK)
    assert (res.n_found, res.n_deleted, res.n_fallback, res.val_bytes) == (nf, nd, nfb, pos)
    # read once: every stageable (segment, floor block) that passes its filter, once
    assert res.blocks_searched == len(blocks)
    assert res.pairs_probed == pairs
    if reader:
        got = env.dev.GetRows(keys)
        assert len(got) == len(keys)
        for k, g in zip(keys, got):
            assert _returned(g) == _outcome(lambda: env.orc.GetRow(k)), k
    return res


# ---- the reference's snapshot ---------------------------------------------------------


def test_reference_snapshot(decoder):
    """prepareTestReader's segments: TestGetRow's keys (:196-245), all of key000-key199,
    key0010 / key900 / key999, and again after dropping 2-0."""
    env = Env(decoder, SC.reference_segments())
    keys = [b"key000", b"key001", b"key900", b"key999", b"key800", b"key0010", b"key198"]
    keys += [b"key%03d" % i for i in range(200)]
    res = _check(env, keys)
    assert res.value(0) == b"value000" and res.value(1) == b"value001"  # TestGetRow's answers
    assert res.value(2) == b"value900" and int(res.state[3]) == NO_ROWS
    assert env.snap.ids[int(res.seg[0])] == "1-1" and env.snap.ids[int(res.seg[2])] == "2-0"
    env.drop(3)
    res = _check(env, keys)
    assert int(res.state[2]) == NO_ROWS  # key900 lived in 2-0 only
    env.close()


# ---- random snapshots and the census ----------------------------------------------------


def _snapshot_keys(keys):
    return list(keys) + [k + b"\x01" for k in keys] + [b"", b"\xff"] + list(keys[:7]) * 2


def _random_case(seed, filters):
    if seed == "quirk":
        segs = SC.quirk_segments()
        keys = sorted({k for _s, _l, d, n, _m in segs for k, _v in _rows_of(d, n)})
    else:
        segs, keys = SC.random_snapshot(seed, nseg=3 + seed % 4)
    return (_with_filters(segs) if filters else segs), _snapshot_keys(keys)


_SEEDS = list(range(6)) + ["quirk"]


@pytest.mark.parametrize("filters", [False, True])
@pytest.mark.parametrize("seed", _SEEDS)
def test_random_snapshots(decoder, seed, filters):
    """Every key of the key space, every key plus one byte, b"", b"\xff" and duplicates
    in one batch, as written and with every segment rewritten with a small filter."""
    segs, keys = _random_case(seed, filters)
    env = Env(decoder, segs)
    _check(env, keys)
    env.close()


@pytest.mark.parametrize("filters", [False, True])
def test_random_snapshots_census(filters):
    """What the batches of test_random_snapshots hold, by the oracle: over the seeds and
    the quirk set every class of outcome occurs."""
    classes, most = set(), 0
    for seed in _SEEDS:
        segs, keys = _random_case(seed, filters)
        orc = Oracle(segs)
        for k in keys:
            most = max(most, orc.expect(k, None, classes)[1])
    want = {"found", "shadowed", "tombstone", "hidden"}
    if filters:
        want.add("bloom-negative newer, found older")
    assert want <= classes and 2 <= most <= 5, (classes, most)


# ---- crafted ------------------------------------------------------------------------------


def test_tombstone_rule(decoder):
    """An empty value at level 0 over an L1 row is a delete; an empty value at level 1
    is a found row with a nil value."""
    base = [(b"a", b"1"), (b"k", b"old"), (b"z", b"9")]
    env = Env(decoder, [_seg("2", 0, [(b"a", b"x"), (b"k", b""), (b"z", b"y")]),
                        _seg("1", 1, base)])
    res = _check(env, [b"k", b"a", b"b"])
    assert [int(s) for s in res.state] == [DELETED, FOUND, NO_ROWS]
    assert env.snap.ids[int(res.seg[0])] == "2"
    env.close()
    env = Env(decoder, [_seg("2", 1, [(b"a", b"x"), (b"k", b""), (b"z", b"y")]),
                        _seg("1", 2, base)])
    res = _check(env, [b"k"])
    assert int(res.state[0]) == FOUND and res.value(0) is None and int(res.val_len[0]) == 0
    env.close()


def _corrupt_floor(seg, key):
    """seg with the key length of the first record of key's floor block set to 65535."""
    sid, lvl, data, n, meta = seg
    st = P.bytes_to_metadata(meta).BlockIndex.descend_le(key)[0]
    bad = bytearray(data)
    bad[st.Offset:st.Offset + 2] = (65535).to_bytes(2, "little")
    return (sid, lvl, bytes(bad), n, meta)


def test_error_precedence(decoder):
    """A corrupt floor block ends the key when its segment is reached, not when an older
    segment has the row; behind the answering segment, or behind its own filter's no, it
    never surfaces."""
    rows = [(b"k%03d" % i, b"v%03d" % i) for i in range(100)]
    newer = [(k, b"new-" + v) for k, v in rows]
    # the newer segment corrupt, the row also in the older one
    env = Env(decoder, [_corrupt_floor(_seg("2", 0, newer), b"k050"), _seg("1", 0, rows)])
    res = _check(env, [b"k050", b"k001"])
    assert (int(res.state[0]), int(res.blk_status[0])) == (SEG_ERROR, _lib.BLK_PANIC)
    assert env.snap.ids[int(res.seg[0])] == "2"
    env.close()
    # the older segment corrupt, the row in the newer one
    env = Env(decoder, [_seg("2", 0, newer), _corrupt_floor(_seg("1", 0, rows), b"k050")])
    res = _check(env, [b"k050"])
    assert int(res.state[0]) == FOUND and res.value(0) == b"new-v050"
    assert res.blocks_searched == 2  # ... though its block was staged and walked
    env.close()
    # the newer segment's filter says no in front of its corrupt floor block
    f = B.BloomFilter(4096, 3)
    sparse = [(k, v) for k, v in newer if k != b"k050"]
    seg2 = _corrupt_floor(_seg("2", 0, sparse, bloom=f), b"k050")
    assert not f.test(b"k050")
    env = Env(decoder, [seg2, _seg("1", 0, rows)])
    res = _check(env, [b"k050", b"k051"])
    assert int(res.state[0]) == FOUND and res.value(0) == b"v050"
    assert int(res.state[1]) == SEG_ERROR  # (a member of the filter reaches the block)
    env.close()


def test_priority_by_string_id(decoder):
    """L0 IDs "9" and "10": "9" > "10" as Go strings, so "9" is asked first; an L1
    segment with a greater ID loses to any L0."""
    mk = lambda tag: [(b"a", tag), (b"k", tag), (b"z", tag)]  # noqa: E731
    env = Env(decoder, [_seg("10", 0, mk(b"ten")), _seg("9", 0, mk(b"nine")),
                        _seg("99", 1, mk(b"l1"))])
    res = _check(env, [b"k"])
    assert res.value(0) == b"nine" and env.snap.ids[int(res.seg[0])] == "9"
    env.close()
    env = Env(decoder, [_seg("99", 1, mk(b"l1")), _seg("10", 0, mk(b"ten"))])
    res = _check(env, [b"k"])
    assert res.value(0) == b"ten"
    env.close()


def _zstd_seg(sid, lvl, rows):
    from tests import zstd_cases as ZC
    data, n, meta = ZC.Z.zstd_segment(rows, 3584, 4096, level=3)
    return (sid, lvl, data, n, meta)


def test_fallback(decoder):
    """A candidate the search does not take (BlockSize over 64 KiB, a zstd segment)
    reached before an answer hands the key back; behind a newer answer it is hidden.
    Reader.GetRows equals the oracle either way."""
    rows = [(b"k%03d" % i, b"v%03d" % i * 3) for i in range(60)]
    big = [(b"k%03d" % i, bytes([i]) * 3000) for i in range(60)]
    part = [(k, b"new-" + v) for k, v in rows if k not in (b"k030", b"k031")] + \
        [(b"k0305", b"keeps k030 inside the range")]
    part.sort()
    for older in (_seg("1", 1, big, threshold=100000, block_size=131072), _zstd_seg("1", 1, rows)):
        assert any(e.BlockSize > 65536 for e in P.bytes_to_metadata(older[4]).entries) or \
            P.bytes_to_metadata(older[4]).compression == P.COMP_ZSTD
        env = Env(decoder, [_seg("2", 0, part), older])
        res = _check(env, [b"k030", b"k010", b"k031", b"k0305", b"nope"])
        assert [int(s) for s in res.state] == [FALLBACK, FOUND, FALLBACK, FOUND, NO_ROWS]
        assert env.snap.ids[int(res.seg[0])] == "1" and res.n_fallback == 2
        assert res.value(1) == b"new-" + dict(rows)[b"k010"]
        env.close()
        # reached first: every covered key falls back
        env = Env(decoder, [older, _seg("0", 2, rows)])
        res = _check(env, [b"k030", b"k010"])
        assert [int(s) for s in res.state] == [FALLBACK, FALLBACK]
        env.close()


@pytest.mark.parametrize("nseg", [33, 65])
def test_many_candidates(decoder, nseg):
    """Every segment covers the key and only the lowest-priority one has it: there is no
    cap on the candidates of a key."""
    segs = []
    for s in range(nseg - 1):
        segs.append(_seg(f"{s:03d}", 0, [(b"a", b"%d" % s), (b"z", b"%d" % s)]))
    segs.append(_seg("zzz", 1, [(b"a", b"x"), (b"k", b"deep"), (b"z", b"x")]))
    env = Env(decoder, segs)
    res = _check(env, [b"k", b"a", b"j"], reader=nseg == 33)
    assert res.value(0) == b"deep" and env.snap.ids[int(res.seg[0])] == "zzz"
    assert res.pairs_probed == 3 * nseg and res.blocks_searched == nseg
    assert res.value(1) == b"%d" % (nseg - 2)  # the greatest L0 ID
    env.close()


# ---- modes --------------------------------------------------------------------------------


def _device_keys(keys):
    pk = pack_keys(keys)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    dk = {k: torch.from_numpy(v.copy().view(signed.get(v.dtype, v.dtype))).cuda()
          for k, v in pk.items()}
    return pk, dk


def _device_out(n, arena):
    return {"state": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
            "seg": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            "blk_status": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
            "entry": torch.zeros(n, dtype=torch.int32, device="cuda"),
            "val_off": torch.zeros(n, dtype=torch.int64, device="cuda"),
            "val_len": torch.zeros(n, dtype=torch.int32, device="cuda"),
            "val_pos": torch.zeros(n, dtype=torch.int64, device="cuda"),
            "val_arena": torch.full((arena,), 0xEE, dtype=torch.uint8, device="cuda")}


def test_modes(decoder):
    """Host mode, OKV_E_CAPACITY with the totals set and the arena untouched and success
    at the reported size, the index-only call, device pointers synchronous and with
    OKV_F_ASYNC + okv_snap_totals, n_rows == 0 and okv_last_path."""
    env = Env(decoder, SC.reference_segments())
    keys = [b"key000", b"key001", b"key900", b"key999", b"key0010", b"key198", b"key001"]
    res = _check(env, keys, reader=False)
    need = res.val_bytes
    assert need > 16 and need % 16 == 0
    with pytest.raises(okv.OkvError) as e:
        S.snap_get_rows(decoder, env.snap, keys, val_cap=need - 16)
    assert e.value.code == _lib.OKV_E_CAPACITY
    r = e.value.result
    assert (r.val_bytes, r.n_found, r.pairs_probed, r.blocks_searched) == \
        (need, res.n_found, res.pairs_probed, res.blocks_searched)
    assert not r.val_arena.any() and list(r.state) == list(res.state)
    assert list(r.val_pos) == list(res.val_pos)
    r = S.snap_get_rows(decoder, env.snap, keys, val_cap=need)  # the reported size
    assert r.val_arena[:need].tobytes() == res.val_arena[:need].tobytes()
    r = S.snap_get_rows(decoder, env.snap, keys, values=False)  # index only
    assert r.val_arena is None and r.val_bytes == need
    assert list(r.val_off) == list(res.val_off) and list(r.seg) == list(res.seg)

    pk, dk = _device_keys(keys)
    n = len(keys)
    want_tot = {k: getattr(res, k) for k in S._TOTALS}
    for sync in (True, False):
        out = _device_out(n, need + 64)
        torch.cuda.synchronize()
        r = S.snap_get_rows(decoder, env.snap, dk, out=out, sync=sync, n_rows=n,
                            key_arena_bytes=int(pk["key_arena"].size))
        if sync:
            assert {k: getattr(r, k) for k in S._TOTALS} == want_tot
        else:
            decoder.sync()
            assert S.totals(decoder) == want_tot
        assert decoder.last_path() == _lib.PATH_SNAP_GET
        for name in ("state", "blk_status", "val_off", "val_len", "val_pos"):
            assert out[name].cpu().tolist() == [int(x) for x in getattr(res, name)], name
        for name in ("seg", "entry"):
            assert (out[name].cpu().numpy().view(np.uint32) == getattr(res, name)).all(), name
        arena = out["val_arena"].cpu().numpy()
        assert arena[:need].tobytes() == res.val_arena[:need].tobytes()
        assert (arena[need:] == 0xEE).all()  # nothing past val_bytes is written
    # a device arena one line short: the totals, and nothing written
    out = _device_out(n, need - 16)
    with pytest.raises(okv.OkvError) as e:
        S.snap_get_rows(decoder, env.snap, dk, out=out, n_rows=n,
                        key_arena_bytes=int(pk["key_arena"].size))
    assert e.value.code == _lib.OKV_E_CAPACITY and e.value.result.val_bytes == need
    assert (out["val_arena"].cpu().numpy() == 0xEE).all()

    r = S.snap_get_rows(decoder, env.snap, [])  # n_rows == 0: succeeds, launches nothing
    assert (r.n_found, r.pairs_probed, r.blocks_searched) == (0, 0, 0)
    assert decoder.last_path() == 0 and S.totals(decoder)["n_found"] == 0
    assert env.dev.GetRows([]) == []
    env.close()


def test_empty_snapshot_and_arguments(decoder):
    """n_segs == 0: every key has no rows.  A foreign context's index or filter, a filter
    okv_get_rows refuses, priorities that are no permutation, NULL outputs: OKV_E_ARG."""
    empty = okv.DeviceSnapshot(decoder, [])
    res = S.snap_get_rows(decoder, empty, [b"", b"k", b"\xff"])
    assert [int(s) for s in res.state] == [NO_ROWS] * 3 and [int(s) for s in res.seg] == [NONE32] * 3
    assert (res.pairs_probed, res.blocks_searched, res.val_bytes) == (0, 0, 0)
    empty.close()
    r = SN.Reader(lambda rec: None, decoder)
    assert [_returned(x) for x in r.GetRows([b"k"])] == [("err", "ErrNoRows")]

    sid, lvl, data, n, meta = _seg("1", 0, [(b"a", b"1"), (b"k", b"2")])
    md = okv.bytes_to_metadata(meta)
    t = torch.frombuffer(bytearray(data) + bytearray(32), dtype=torch.uint8).cuda()
    other = okv.Decoder(0)
    try:
        ix, ix2 = okv.DeviceIndex.from_metadata(decoder, md), okv.DeviceIndex.from_metadata(other, md)
        bl2, big_k = okv.DeviceBloom(other, 64, 2), okv.DeviceBloom(decoder, 64, 5000)
        for index, bloom in ((ix2, None), (ix, bl2), (ix, big_k)):
            with pytest.raises(okv.OkvError) as e:
                okv.DeviceSnapshot(decoder, [(t, len(data), index, bloom, 0, 0, "1", b"a", b"k")])
            assert e.value.code == _lib.OKV_E_ARG
        L = _lib.lib()
        fk = np.frombuffer(b"ak", np.uint8)
        two = (_lib.SnapSeg * 2)(*[_lib.SnapSeg(t.data_ptr(), len(data), ix._h, None,
                                                fk.ctypes.data, fk.ctypes.data + 1, 1, 1, 0, 0, p)
                                   for p in (0, 0)])
        h = C.c_void_p()
        assert L.okv_snap_new(decoder._ctx, two, 2, C.byref(h)) == _lib.OKV_E_ARG and not h.value
        snap = okv.DeviceSnapshot(decoder, [(t, len(data), ix, None, 0, 0, "1", b"a", b"k")])
        pk = pack_keys([b"k"])
        rws = _lib.Rows(pk["key_arena"].ctypes.data, pk["key_off"].ctypes.data,
                        pk["key_len"].ctypes.data, None, None, None, 1, pk["key_arena"].size, 0)
        o = _lib.SnapOut()
        assert L.okv_snap_get_rows(decoder._ctx, snap._h, C.byref(rws), C.byref(o), 0) == _lib.OKV_E_ARG
        assert L.okv_snap_get_rows(decoder._ctx, None, C.byref(rws), C.byref(o), 0) == _lib.OKV_E_ARG
        assert L.okv_snap_get_rows(other._ctx, snap._h, C.byref(rws), C.byref(o), 0) == _lib.OKV_E_ARG
        res = S.snap_get_rows(decoder, snap, [b"k", b"b"])
        assert [int(s) for s in res.state] == [FOUND, NO_ROWS] and res.value(0) == b"2"
        for x in (snap, big_k, bl2, ix, ix2):
            x.close()
    finally:
        other.close()


def test_reader_rebuilds_and_falls_back_on_a_refused_filter(decoder):
    """UpdateSegments drops the uploaded segment and the okv_snap is rebuilt; a snapshot
    with a filter the device refuses (k > 4096) goes through GetRow key by key."""
    env = Env(decoder, SC.reference_segments())
    keys = [b"key900", b"key001", b"key000"]
    assert [_returned(g) for g in env.dev.GetRows(keys)] == \
        [_outcome(lambda: env.orc.GetRow(k)) for k in keys]
    first = env.dev._snap
    assert first is not None and set(env.dev._raw) == {"1-0", "1-1", "2-1", "2-0"}
    env.dev.GetRows(keys)
    assert env.dev._snap is first  # (one upload per segment set)
    env.orc.UpdateSegments(None, [env.orecs[3]])
    env.dev.UpdateSegments(None, [env.drecs[3]])
    assert "2-0" not in env.dev._raw
    assert [_returned(g) for g in env.dev.GetRows(keys)] == \
        [_outcome(lambda: env.orc.GetRow(k)) for k in keys]
    assert env.dev._snap is not first and len(env.dev._snap) == 3
    env.close()
    rows = [(b"k%02d" % i, b"v%02d" % i) for i in range(20)]
    seg = _seg("1", 0, rows, bloom=B.BloomFilter(64, 5000))
    data = {"1": (seg[2], seg[3])}
    rd = SN.Reader(lambda rec: data[rec.ID], decoder)
    pmd = P.bytes_to_metadata(seg[4])
    rd.UpdateSegments([SN.SegmentRecord("1", 0, pmd.FirstKey, pmd.LastKey)], None)
    got = rd.GetRows([b"k03", b"k033"])
    assert rd._snap is False and _returned(got[0]) == ("value", b"v03")
    assert _returned(got[1]) == ("err", "ErrNoRows")
