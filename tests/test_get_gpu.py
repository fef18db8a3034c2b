"""Batched GetRow on the device (okv_index_*, okv_get_rows) against the
oracle: per key the outcome of Go's GetRow (segment_reader.go:362-404) -- bloom probe,
floor block, ReadBlockWithStat in full, first equal key -- from CO.decode_soa plus the
row loop for single blocks and from pyoracle.SegmentReader.GetRow for whole segments."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib, get as G
from objectkv_amd import reader as R
from objectkv_amd.bloom import pack_keys
from oracle import bloom_ref as B
from oracle import coracle as CO
from oracle import pyoracle as P
from tests import index_cases as IC
from tests import staged_cases as SC
from tests.conftest import descs_of, unpack
from tests.test_point_gpu import _bloom_segment, _expect_get

pytestmark = pytest.mark.gpu

NONE32 = 0xFFFFFFFF
FOUND, BLOOM_NEG, NO_BLOCK, NOT_IN_BLOCK, BLOCK_ERROR, FALLBACK = range(6)


def _dev(seg: bytes):
    """The segment in device memory (kept alive by the caller) -> (tensor, length)."""
    t = torch.frombuffer(bytearray(seg) + bytearray(16), dtype=torch.uint8).cuda()
    return t, len(seg)


def _get(decoder, dseg, index, keys, bloom=None, comp=0, **kw):
    t, n = dseg
    return G.get_rows(decoder, t, n, index, list(keys), bloom=bloom, compression=comp, **kw)


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


def _check_block(decoder, dseg, seg, d, comp, keys):
    """Every key against block d behind a one-entry index whose FirstKey is empty."""
    ix = okv.DeviceIndex(decoder, np.array([d], np.uint64), [b""])
    res = _get(decoder, dseg, ix, keys, comp=comp)
    ix.close()
    ref = CO.decode_soa(seg, CO.descs_array([tuple(int(x) for x in d)]), comp, False)
    rs = _read_status(d, len(seg))
    for i, key in enumerate(keys):
        assert int(res.entry[i]) == 0
        if rs != _lib.BLK_OK:
            want = (BLOCK_ERROR, rs)
        elif int(d[1]) > 65536:
            want = (FALLBACK, 0)
        else:
            st, found, _k, v = _expect_get(ref, 0, key)
            want = (BLOCK_ERROR, st) if st else (FOUND if found else NOT_IN_BLOCK, 0)
        assert (int(res.state[i]), int(res.blk_status[i])) == want, (list(d), key[:20])
        if want[0] == FOUND:
            assert res.value(i) == (v or None), (list(d), key[:20])
            assert int(res.val_len[i]) == len(v)
            off = int(res.val_off[i])
            assert seg[off:off + len(v)] == v
        else:
            assert int(res.val_len[i]) == 0 and int(res.val_off[i]) == 0
    return res


def _block_keys(seg, d, comp):
    """Every row key, every row key plus one byte, b"" and an absent key."""
    ref = CO.decode_soa(seg, CO.descs_array([tuple(int(x) for x in d)]), comp, False)
    keys = [b"", b"no-such-key"]
    r0, r1 = int(ref["row_start"][0]), int(ref["row_start"][1])
    ka = ref["key_arena"].tobytes()
    for g in range(r0, r1):
        ko, kl = int(ref["key_off"][g]), int(ref["key_len"][g])
        k = ka[ko:ko + kl]
        keys += [k] + ([k + b"\x01"] if kl < 65535 else [])
    return keys


@pytest.mark.parametrize("comp", [_lib.COMP_NONE, _lib.COMP_LZ4])
def test_every_block_status(decoder, golden, comp):
    """Each crafted-edge block and each block of the uncompressed writer cases as the
    floor of every key: state, blk_status, value bytes and nil-ness == the oracle's
    ReadBlockWithStat + row loop; blocks over 64 KiB report FALLBACK."""
    cases = [golden["crafted_edges"]] + [c for c in golden.values()
                                         if c["kind"] == "writer" and c["compression"] != 2]
    seen = set()
    for case in cases:
        seg = unpack(case["segment_z"])
        dseg = _dev(seg)
        c = comp if case is golden["crafted_edges"] else case["compression"]
        for d in descs_of(case):
            res = _check_block(decoder, dseg, seg, d, c, _block_keys(seg, d, c))
            seen |= {(int(s), int(b)) for s, b in zip(res.state, res.blk_status)}
            assert decoder.last_path() == _lib.PATH_GET
    states = {s for s, _ in seen}
    assert {NOT_IN_BLOCK, BLOCK_ERROR, FALLBACK} <= states
    assert {(BLOCK_ERROR, _lib.BLK_EOF), (BLOCK_ERROR, _lib.BLK_SHORT),
            (BLOCK_ERROR, _lib.BLK_PANIC)} <= seen
    if comp == _lib.COMP_NONE:
        assert FOUND in states


@pytest.fixture(scope="module")
def seg40():
    """A 40-block writer segment of 4 KiB blocks (no filter) with its oracle reader."""
    w = okv.synth_segment(okv.sst.SYNTH_FIXED, 12, nblocks=39, threshold=3584, block_size=4096)
    seg = w.data().tobytes()
    md = P.bytes_to_metadata(w.meta())
    assert len(md.entries) == 40
    return seg, md, _dev(seg), w.meta()


def test_floor_search_on_the_device(decoder, seg40):
    """entry[] == the btree oracle's floor for hand-built indexes (duplicate first keys,
    9- and 16-byte shared prefixes, trees of 1, 2, 63, 64 and 65) over the key set of the
    CPU test (tests/index_cases.py)."""
    seg, md, dseg, meta40 = seg40
    descs = np.array([st.desc() for st in md.entries], np.uint64)
    trees = IC.trees()
    for name in ("n1", "n2", "n63", "n64", "n65", "n65_dup", "dups_last_wins", "empty_first_key",
                 "ab_family", "short_and_zero", "prefix_ties", "prefix_ties_dups"):
        keys = trees[name]
        d = descs[np.arange(len(keys)) % 40]
        ix = okv.DeviceIndex(decoder, d, keys)
        order, oix = IC.oracle_tree(keys)
        assert ix.info() == (len(order), len(keys))
        qs = IC.queries(keys)
        res = _get(decoder, dseg, ix, qs, values=False)
        want = [IC.oracle_floor(oix, q) for q in qs]
        got = [-1 if int(e) == NONE32 else int(e) for e in res.entry]
        assert got == want, name
        for q, e, s in zip(qs, want, res.state):
            assert (int(s) == NO_BLOCK) == (e < 0), (name, q)
        ix.close()


def _oracle_state(orr, key):
    """pyoracle GetRow -> (state, blk_status or None, value)"""
    try:
        kv = orr.GetRow(key)
        return FOUND, 0, kv.Value
    except P.GoPanic:
        return BLOCK_ERROR, _lib.BLK_PANIC, None
    except P.GoError as e:
        if e.kind != P.ErrNoRows:
            return BLOCK_ERROR, None, None
        msg = str(e)
        return (BLOOM_NEG if "bloom filter" in msg else NO_BLOCK if "potential block" in msg
                else NOT_IN_BLOCK), 0, None


def _same_as_oracle(res, keys, orr):
    for i, k in enumerate(keys):
        st, bst, v = _oracle_state(orr, k)
        assert int(res.state[i]) == st, (k, int(res.state[i]), st)
        if bst is not None:
            assert int(res.blk_status[i]) == bst, k
        if st == FOUND:
            assert res.value(i) == v, k


def test_grouping(decoder, seg40):
    """0 keys, 1 key, 300 keys on one block (more than a workgroup's threads), one key in
    every block, a shuffled list with repeated keys: every key == the oracle's GetRow,
    blocks_searched == the distinct floor blocks, results independent of key order."""
    seg, md, dseg, meta40 = seg40
    ix = okv.DeviceIndex.from_metadata(decoder, okv.bytes_to_metadata(meta40))
    orr = P.SegmentReader(seg, len(seg))
    rows = [[(P._b(r.Key), P._b(r.Value)) for r in P.read_block(seg, st.desc(), 0)[1]]
            for st in md.entries]

    res = _get(decoder, dseg, ix, [])
    assert (res.n_found, res.blocks_searched, res.val_bytes) == (0, 0, 0)
    assert decoder.last_path() == 0  # nothing launched

    res = _get(decoder, dseg, ix, [rows[7][3][0]])
    assert res.n_found == 1 and res.blocks_searched == 1 and res.value(0) == rows[7][3][1]

    blk = rows[11]
    one_block = [blk[i % len(blk)][0] if i % 3 else blk[i % len(blk)][0] + b"\x00"
                 for i in range(300)]
    res = _get(decoder, dseg, ix, one_block)
    assert res.blocks_searched == 1 and res.n_found == 200
    _same_as_oracle(res, one_block, orr)

    every = [r[len(r) // 2][0] for r in rows]
    res = _get(decoder, dseg, ix, every)
    assert res.blocks_searched == 40 and res.n_found == 40
    assert sorted(int(e) for e in res.entry) == list(range(40))
    _same_as_oracle(res, every, orr)

    rng = random.Random(4)
    mixed = [rng.choice(rng.choice(rows[:25]))[0] for _ in range(500)]
    mixed += [b"", b"\x00", rows[0][0][0][:-1], b"\xff" * 12] + [k + b"!" for k in mixed[:50]]
    mixed += mixed[:100]
    rng.shuffle(mixed)
    res = _get(decoder, dseg, ix, mixed)
    _same_as_oracle(res, mixed, orr)
    floors = {int(e) for e in res.entry if int(e) != NONE32}
    assert res.blocks_searched == len(floors)
    perm = list(range(len(mixed)))
    rng.shuffle(perm)
    res2 = _get(decoder, dseg, ix, [mixed[p] for p in perm])
    assert res2.blocks_searched == res.blocks_searched and res2.n_found == res.n_found
    for j, p in enumerate(perm):
        for f in ("state", "blk_status", "entry", "val_off", "val_len"):
            assert int(getattr(res2, f)[j]) == int(getattr(res, f)[p]), f
        assert res2.value(j) == res.value(p)
    ix.close()


def test_many_rows(decoder):
    """No cap on rows: the 1 500-record block and the 64 KiB block of 10 922 empty
    records of test_point_many_rows; in the second, b"" finds row 0."""
    rng = np.random.default_rng(3)
    body1, keys1 = bytearray(), []
    for _ in range(1500):
        kl, vl = int(rng.integers(0, 12)), int(rng.integers(0, 20))
        rec = rng.integers(0, 256, kl + vl, dtype=np.uint8).tobytes()
        body1 += kl.to_bytes(2, "little") + vl.to_bytes(4, "little") + rec
        keys1.append(rec[:kl])
    body2 = bytes(65536 // 6 * 6)
    seg = bytes(body1) + bytes(body2) + bytes(7)
    dseg = _dev(seg)
    d1 = np.array([0, len(body1), len(body1), 0], np.uint64)
    d2 = np.array([len(body1), len(body2), len(body2), 0], np.uint64)
    keys = keys1[::7] + keys1[-3:] + [k + b"\x01" for k in keys1[:20]] + [b""]
    res = _check_block(decoder, dseg, seg, d1, 0, keys)
    assert res.n_found >= len(keys1[::7])
    res = _check_block(decoder, dseg, seg, d2, 0, [b"", b"\x00", b"x"])
    assert [int(s) for s in res.state] == [FOUND, NOT_IN_BLOCK, NOT_IN_BLOCK]
    assert int(res.val_off[0]) == len(body1) + 6 and res.value(0) is None


def _one_block_reader(seg, d):
    """The oracle's reader over seg with d as its only block (FirstKey empty)."""
    st = P.BlockStat(FirstKey=b"", Offset=int(d[0]), BlockSize=int(d[1]), OriginalSize=int(d[2]))
    md = P.SegmentMetadata()
    md.entries.append(st)
    md.BlockIndex.replace_or_insert(st)
    orr = P.SegmentReader(seg, len(seg))
    orr.LoadCachedMetadata(md)
    return orr


@pytest.mark.parametrize("name", SC.WALK + SC.STAGING + SC.KEYS)
def test_staged_cases(decoder, name):
    """tests/staged_cases.py through okv_get_rows, each block as the floor of every probe
    key: == the oracle's GetRow (_oracle_state) and its ReadBlockWithStat + row loop --
    runs of 1 to 129 equal records, a bad record inside a run failing every key of its
    block, OriginalSize against the run, 1 023 to 1 025 rows, offsets & 15 of 0 / 1 / 15,
    8 192- and 8 193-byte blocks (the two kCap forms), a 64 KiB block at offset & 15 ==
    15, probe keys of 0 to 8 192 bytes, all but the last byte, prefixes, duplicates."""
    seg, d, keys = SC.cases()[name]
    dseg = _dev(seg)
    for row in d:
        res = _check_block(decoder, dseg, seg, row, 0, keys)
        _same_as_oracle(res, keys, _one_block_reader(seg, row))
        if name == "bad_in_run":
            assert all((int(s), int(b)) == (BLOCK_ERROR, _lib.BLK_PANIC)
                       for s, b in zip(res.state, res.blk_status))
    if name == "keys":
        assert res.n_found >= 8 and res.value(keys.index(b"dup")) == b"first"


def test_probe_keys_at_every_arena_alignment(decoder):
    """The probe keys packed back to back so that they start at arena offsets & 3 of 0,
    1, 2 and 3, the last one ending on the arena's last byte (no pad after it): the same
    outcomes as key by key."""
    seg, d, keys = SC.cases()["keys"]
    ks = [k for k in keys if 0 < len(k) <= 256]
    hit5 = [k for k in ks if len(k) == 5][0]
    ks.append(b"dup")
    while sum(len(k) for k in ks) & 3 != 3:
        ks.append(b"x")
    ks.append(hit5)  # starts at offset & 3 == 3, ends the arena
    pk = pack_keys(ks)
    total = int(pk["key_off"][-1]) + len(ks[-1])
    pk["key_arena"] = np.ascontiguousarray(pk["key_arena"][:total])
    assert {int(o) & 3 for o, k in zip(pk["key_off"], ks) if len(k) >= 4} == {0, 1, 2, 3}
    assert int(pk["key_off"][-1]) & 3 and len(ks[-1]) == 5
    dseg = _dev(seg)
    ix = okv.DeviceIndex(decoder, d, [b""])
    res = G.get_rows(decoder, dseg[0], dseg[1], ix, pk)
    one = _get(decoder, dseg, ix, ks)
    ix.close()
    _same_as_oracle(res, ks, _one_block_reader(seg, d[0]))
    assert int(res.state[-1]) == FOUND
    for f in ("state", "blk_status", "val_off", "val_len"):
        assert list(getattr(res, f)) == list(getattr(one, f)), f


def test_bloom_default_filter(decoder):
    """The default-options segment: members are found, rejected keys are BLOOM_NEGATIVE
    (== bloom_ref), without a filter the same absent keys are NOT_IN_BLOCK; rejected keys
    over a corrupted floor block stay BLOOM_NEGATIVE while a member of it is
    BLOCK_ERROR / OKV_BLK_PANIC."""
    rows, data, flen, meta, f = _bloom_segment()
    md = okv.bytes_to_metadata(meta)
    ix = okv.DeviceIndex.from_metadata(decoder, md)
    bl = okv.DeviceBloom.from_bytes(decoder, f.to_bytes())
    dseg = _dev(data)
    orr = P.SegmentReader(data, flen)
    absent = [b"k%06d" % i for i in range(1, 2000, 2)]
    keys = [k for k, _ in rows[::13]] + absent
    res = _get(decoder, dseg, ix, keys, bloom=bl)
    _same_as_oracle(res, keys, orr)
    rejected = [k for k in absent if not f.test(k)]
    assert len(rejected) > 900
    assert res.n_found == len(rows[::13])
    res0 = _get(decoder, dseg, ix, absent)  # no filter: every absent key reads its block
    assert all(int(s) == NOT_IN_BLOCK for s in res0.state) and res0.blocks_searched > 1

    pmd = P.bytes_to_metadata(meta)
    ent = sorted(pmd.entries, key=lambda e: e.FirstKey)
    target, nxt = ent[len(ent) // 2], ent[len(ent) // 2 + 1].FirstKey
    bad = bytearray(data)
    kl0 = int.from_bytes(bad[target.Offset:target.Offset + 2], "little")
    vl0 = int.from_bytes(bad[target.Offset + 2:target.Offset + 6], "little")
    p2 = target.Offset + 6 + kl0 + vl0
    bad[p2:p2 + 2] = (65535).to_bytes(2, "little")
    bad = bytes(bad)
    dbad = _dev(bad)
    member = target.FirstKey  # sits before the bad record: the block still fails it
    gone = [k for k in (member + b"%03d" % i for i in range(1000)) if k < nxt and not f.test(k)][:20]
    keys = [member] + gone
    res = _get(decoder, dbad, ix, keys, bloom=bl)
    assert (int(res.state[0]), int(res.blk_status[0])) == (BLOCK_ERROR, _lib.BLK_PANIC)
    assert all(int(s) == BLOOM_NEG for s in res.state[1:]) and res.blocks_searched == 1
    _same_as_oracle(res, keys, P.SegmentReader(bad, flen))
    res = _get(decoder, dbad, ix, keys)  # without the filter they all read the bad block
    assert all((int(s), int(b)) == (BLOCK_ERROR, _lib.BLK_PANIC)
               for s, b in zip(res.state, res.blk_status))
    bl.close()
    ix.close()


def test_bloom_tiny_filter_false_positives(decoder, seg40):
    """m = 64, k = 2: bloom_ref finds false positives, so "maybe, but absent"
    (NOT_IN_BLOCK) and "rejected" (BLOOM_NEGATIVE) both occur, each where bloom_ref says."""
    seg, md, dseg, meta40 = seg40
    ix = okv.DeviceIndex.from_metadata(decoder, okv.bytes_to_metadata(meta40))
    first = md.entries[0].FirstKey
    f = B.BloomFilter(64, 2)
    members = [P._b(r.Key) for r in P.read_block(seg, md.entries[3].desc(), 0)[1]][:6]
    for k in members:
        f.add(k)
    bl = okv.DeviceBloom.from_bytes(decoder, f.to_bytes())
    absent = [first + b"~%04d" % i for i in range(400)]
    keys = members + absent + [b"", b"\x00" * 17]
    res = _get(decoder, dseg, ix, keys, bloom=bl)
    seen = set()
    for k, s in zip(keys, res.state):
        if not f.test(k):
            assert int(s) == BLOOM_NEG, k
        else:
            assert int(s) == (FOUND if k in members else NO_BLOCK if k < first else NOT_IN_BLOCK), k
        seen.add(int(s))
    assert {FOUND, BLOOM_NEG, NOT_IN_BLOCK} <= seen
    bl.close()
    ix.close()


def _value_segment():
    rows = [(b"a%03d" % i, b"") for i in range(5)]
    rows += [(b"big", bytes(range(256)) * 234 + b"tail" * 24)]  # 60 000 bytes
    rows += [(b"c%03d" % i, b"v" * (i % 40)) for i in range(200)]
    assert len(rows[5][1]) == 60000
    w = okv.SegmentWriter(61000, 65536)
    for k, v in rows:
        w.WriteRow(k, v)
    flen, meta = w.Close()
    return rows, w.data().tobytes(), flen, meta


def test_values(decoder):
    """Empty values (nil), a 60 000-byte value in a 64 KiB block, val_pos 16-byte aligned
    in key order with zero pads, OKV_E_CAPACITY with the totals set and the arena
    untouched, the index-only call, and device pointers with OKV_F_ASYNC + okv_get_totals."""
    rows, data, flen, meta = _value_segment()
    ix = okv.DeviceIndex.from_metadata(decoder, okv.bytes_to_metadata(meta))
    dseg = _dev(data)
    want = dict(rows)
    keys = [b"big", b"a000", b"c007", b"nope", b"c199", b"a004", b"big", b"c001"]
    res = _get(decoder, dseg, ix, keys)
    pos = 0
    for i, k in enumerate(keys):
        if k not in want:
            assert int(res.state[i]) == NOT_IN_BLOCK
            continue
        v = want[k]
        assert int(res.state[i]) == FOUND and res.value(i) == (v or None)
        assert int(res.val_pos[i]) == pos and pos % 16 == 0
        pad = res.val_arena[pos + len(v):pos + (len(v) + 15) // 16 * 16]
        assert not pad.any()
        pos += (len(v) + 15) // 16 * 16
    assert res.val_bytes == pos and res.n_found == 7 and res.n_fallback == 0

    with pytest.raises(okv.OkvError) as e:  # one byte short
        _get(decoder, dseg, ix, keys, val_cap=pos - 16)
    assert e.value.code == _lib.OKV_E_CAPACITY
    r = e.value.result
    assert (r.val_bytes, r.n_found, r.blocks_searched) == (pos, 7, res.blocks_searched)
    assert not r.val_arena.any() and list(r.state) == list(res.state)
    assert list(r.val_pos) == list(res.val_pos)

    r = _get(decoder, dseg, ix, keys, values=False)  # index only
    assert r.val_arena is None and r.val_bytes == pos
    assert list(r.val_off) == list(res.val_off) and list(r.val_len) == list(res.val_len)
    for i, k in enumerate(keys):
        if k in want:
            off = int(r.val_off[i])
            assert data[off:off + int(r.val_len[i])] == want[k]

    # device pointers, enqueued: totals after the sync
    pk = pack_keys(keys)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    dk = {k: torch.from_numpy(v.copy().view(signed.get(v.dtype, v.dtype))).cuda()
          for k, v in pk.items()}
    n = len(keys)
    out = {"state": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
           "blk_status": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
           "entry": torch.zeros(n, dtype=torch.int32, device="cuda"),
           "val_off": torch.zeros(n, dtype=torch.int64, device="cuda"),
           "val_len": torch.zeros(n, dtype=torch.int32, device="cuda"),
           "val_pos": torch.zeros(n, dtype=torch.int64, device="cuda"),
           "val_arena": torch.full((pos + 64,), 0xEE, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    G.get_rows(decoder, dseg[0], dseg[1], ix, dk, out=out, sync=False, n_rows=n,
               key_arena_bytes=int(pk["key_arena"].size))
    decoder.sync()
    assert G.totals(decoder) == {"n_found": 7, "n_fallback": 0, "val_bytes": pos,
                                 "blocks_searched": res.blocks_searched}
    assert out["state"].cpu().tolist() == [int(s) for s in res.state]
    assert out["val_pos"].cpu().tolist() == [int(p) for p in res.val_pos]
    arena = out["val_arena"].cpu().numpy()
    assert arena[:pos].tobytes() == res.val_arena[:pos].tobytes()
    assert (arena[pos:] == 0xEE).all()  # nothing past val_bytes is written
    ix.close()


def test_block_past_4gib(decoder):
    """One block at offset 2^32 + 4096 of an uninitialised device buffer and one at 0:
    val_off and the value bytes are right (64-bit offsets throughout)."""
    far = 2**32 + 4096
    rec = lambda k, v: len(k).to_bytes(2, "little") + len(v).to_bytes(4, "little") + k + v  # noqa: E731
    b0 = rec(b"apple", b"near") + rec(b"fig", b"")
    b1 = rec(b"melon", b"far away value") + rec(b"pear", b"x" * 100)
    t = torch.empty(far + 4096, dtype=torch.uint8, device="cuda")
    t[:len(b0)] = torch.frombuffer(bytearray(b0), dtype=torch.uint8).cuda()
    t[far:far + len(b1)] = torch.frombuffer(bytearray(b1), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    descs = np.array([[0, len(b0), len(b0), 0], [far, len(b1), len(b1), 0]], np.uint64)
    ix = okv.DeviceIndex(decoder, descs, [b"", b"m"])
    keys = [b"pear", b"apple", b"melon", b"fig", b"zzz", b"lemon"]
    res = G.get_rows(decoder, t, far + 4096, ix, keys)
    assert [int(s) for s in res.state] == [FOUND, FOUND, FOUND, FOUND, NOT_IN_BLOCK, NOT_IN_BLOCK]
    assert [int(e) for e in res.entry] == [1, 0, 1, 0, 1, 0]
    assert [res.value(i) for i in range(4)] == [b"x" * 100, b"near", b"far away value", None]
    assert int(res.val_off[0]) == far + len(rec(b"melon", b"far away value")) + 6 + 4
    assert int(res.val_off[2]) == far + 6 + 5 and res.blocks_searched == 2
    ix.close()
    del t


def _both(reader, orr, keys):
    got = reader.GetRows(keys)
    assert len(got) == len(keys)
    for k, g in zip(keys, got):
        try:
            one = reader.GetRow(k)
            assert isinstance(g, R.KVPair) and (g.Key, g.Value) == (one.Key, one.Value), k
        except R.GoPanic as e:
            assert isinstance(g, R.GoPanic) and g.code == e.code, k
        except R.GoError as e:
            assert isinstance(g, R.GoError) and (g.code, g.kind) == (e.code, e.kind), k
        if orr is not None:
            st, _bst, v = _oracle_state(orr, k)
            if st == FOUND:
                assert isinstance(g, R.KVPair) and g.Value == v and g.Key == (k or None)
            elif st == BLOCK_ERROR:
                assert isinstance(g, (R.GoPanic, R.GoError)) and getattr(g, "kind", "") != "ErrNoRows"
            else:
                assert isinstance(g, R.GoError) and g.kind == "ErrNoRows", k
    return got


def test_reader_get_rows(decoder, golden):
    """SegmentReader.GetRows(keys) == [GetRow(k)], exceptions included, on the bloom
    segment, the golden rollover case, a zstd segment (every key falls back) and a
    corrupt-block segment; io_stats shows one upload and one call per batch."""
    rows, data, flen, meta, f = _bloom_segment()
    keys = [k for k, _ in rows[::41]] + [b"k%06d" % i for i in range(1, 400, 2)]
    keys += [b"", b"\xff" * 9]
    rd = R.SegmentReader(data, flen, decoder)
    rd.FetchAndLoadMetadata()
    before = rd.io_stats()
    got = rd.GetRows(keys)
    a = rd.io_stats()
    assert a["bytes_staged"] - before["bytes_staged"] == len(data)
    assert a["calls"] - before["calls"] == 1
    rd.GetRows(keys[:50])
    b = rd.io_stats()
    assert b["bytes_staged"] == a["bytes_staged"] and b["calls"] - a["calls"] == 1
    assert sum(isinstance(g, R.KVPair) for g in got) == len(rows[::41])
    # (a key longer than 65 535 bytes takes the single-key path)
    _both(rd, P.SegmentReader(data, flen), keys + [b"x" * 70000, rows[3][0] + b"y" * 66000])
    assert rd.GetRows([]) == []

    case = golden["ref_rollover_no_bloom"]
    seg = unpack(case["segment_z"])
    orr = P.SegmentReader(seg, case["file_len"])
    ks = []
    for st in P.bytes_to_metadata(bytes.fromhex(case["meta"])).entries:
        ks += [P._b(r.Key) for r in P.read_block(seg, st.desc(), 0)[1]]
    ks = ks[::3] + [k + b"\x00" for k in ks[:10]] + [b"", b"\x00"]
    _both(R.SegmentReader(seg, case["file_len"], decoder), orr, ks)

    from tests import zstd_cases as ZC
    zrows = ZC._rows(41, 300)
    zseg, zlen, _zm = ZC.Z.zstd_segment(zrows, 3584, 4096, level=3)
    zr = R.SegmentReader(zseg, zlen, decoder)
    zk = [k for k, _ in zrows[::17]] + [zrows[5][0] + b"\x01", b""]
    got = _both(zr, P.SegmentReader(zseg, zlen), zk)
    assert sum(isinstance(g, R.KVPair) for g in got) == len(zrows[::17])

    pmd = P.bytes_to_metadata(meta)
    ent = sorted(pmd.entries, key=lambda e: e.FirstKey)
    target = ent[3]
    bad = bytearray(data)
    bad[target.Offset:target.Offset + 2] = (65535).to_bytes(2, "little")
    bad = bytes(bad)
    ck = [target.FirstKey, ent[2].FirstKey, ent[4].FirstKey, target.FirstKey + b"zz", b"k000001"]
    got = _both(R.SegmentReader(bad, flen, decoder), P.SegmentReader(bad, flen), ck)
    assert isinstance(got[0], R.GoPanic) and isinstance(got[1], R.KVPair)


def test_arguments(decoder, seg40):
    """A foreign context's index or filter, NULL outputs, k > 4096: OKV_E_ARG."""
    seg, md, dseg, meta40 = seg40
    other = okv.Decoder(0)
    L = _lib.lib()
    try:
        mdp = okv.bytes_to_metadata(meta40)
        ix, ix2 = okv.DeviceIndex.from_metadata(decoder, mdp), okv.DeviceIndex.from_metadata(other, mdp)
        bl2 = okv.DeviceBloom(other, 64, 2)
        key = [md.entries[1].FirstKey]
        for kw in (dict(index=ix2), dict(index=ix, bloom=bl2)):
            with pytest.raises(okv.OkvError) as e:
                G.get_rows(decoder, dseg[0], dseg[1], kw["index"], key, bloom=kw.get("bloom"))
            assert e.value.code == _lib.OKV_E_ARG
        big_k = okv.DeviceBloom(decoder, 64, 5000)
        with pytest.raises(okv.OkvError) as e:
            _get(decoder, dseg, ix, key, bloom=big_k)
        assert e.value.code == _lib.OKV_E_ARG and "4096" in str(e.value)
        # NULL outputs
        pk = pack_keys(key)
        rws = _lib.Rows(pk["key_arena"].ctypes.data, pk["key_off"].ctypes.data,
                        pk["key_len"].ctypes.data, None, None, None, 1, pk["key_arena"].size, 0)
        o = _lib.GetOut()
        rc = L.okv_get_rows(decoder._ctx, dseg[0].data_ptr(), dseg[1], ix._h, None, C.byref(rws), 0,
                            C.byref(o), 0)
        assert rc == _lib.OKV_E_ARG
        assert L.okv_get_rows(decoder._ctx, dseg[0].data_ptr(), dseg[1], ix._h, None, C.byref(rws), 0,
                              None, 0) == _lib.OKV_E_ARG
        assert L.okv_get_rows(decoder._ctx, dseg[0].data_ptr(), dseg[1], None, None, C.byref(rws), 0,
                              C.byref(o), 0) == _lib.OKV_E_ARG
        # an index of no entries is legal: every key has no block
        empty = okv.DeviceIndex(decoder, np.zeros((0, 4), np.uint64), [])
        res = _get(decoder, dseg, empty, [b"", b"k"])
        assert [int(s) for s in res.state] == [NO_BLOCK, NO_BLOCK] and res.blocks_searched == 0
        for h in (big_k, bl2, ix, ix2, empty):
            h.close()
    finally:
        other.close()
