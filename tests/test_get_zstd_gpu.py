"""Batched GetRow on zstd segments (OKV_F_GET_ZSTD): the touched blocks are
inflated on the device inside the call and searched from the inflated bytes.  Per key the
expectation is Go's GetRow from the oracle's ReadBlockWithStat (pyoracle.read_block, which
returns 6 for a rejected frame set and 3 for a short buffer) plus the row loop; the product
reader's GetRows is compared with its own single-key GetRow."""
from __future__ import annotations

import bisect
import hashlib
import random
import struct

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib, get as G
from objectkv_amd import reader as R
from objectkv_amd.bloom import pack_keys
from oracle import bloom_ref as B
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import zstd_cases as ZC

pytestmark = pytest.mark.gpu

NONE32 = 0xFFFFFFFF
FOUND, BLOOM_NEG, NO_BLOCK, NOT_IN_BLOCK, BLOCK_ERROR, FALLBACK = range(6)
ZSTD = _lib.COMP_ZSTD
PATH_Z = _lib.PATH_GET | _lib.PATH_ZSTD
COLS = ("state", "blk_status", "entry", "val_off", "val_len", "val_pos")


def _dev(seg: bytes):
    t = torch.frombuffer(bytearray(seg) + bytearray(16), dtype=torch.uint8).cuda()
    return t, len(seg)


class Seg:
    """A zstd segment on the device with its index and the oracle's view of every block."""

    def __init__(self, decoder, seg, meta, descs=None, first_keys=None):
        self.decoder, self.seg = decoder, seg
        self.dseg = _dev(seg)
        if descs is None:
            md = P.bytes_to_metadata(meta)
            descs = [st.desc() for st in md.entries]
            first_keys = [P._b(st.FirstKey) for st in md.entries]
        self.descs, self.fks = [tuple(int(x) for x in d) for d in descs], list(first_keys)
        assert self.fks == sorted(set(self.fks))  # the floor is a bisect
        self.ix = okv.DeviceIndex(decoder, np.array(self.descs, np.uint64).reshape(-1, 4), self.fks)
        self._blk = {}

    def block(self, b):
        """-> (status, [(key, value)], inflated bytes or None)"""
        if b not in self._blk:
            d = self.descs[b]
            st, rows = P.read_block(self.seg, d, ZSTD)
            raw = None
            if d[0] < len(self.seg) and len(self.seg) - d[0] >= d[1] and d[3] <= d[1]:
                raw = Z.decompress(self.seg[d[0]:d[0] + d[3]], d[2])
            self._blk[b] = (st, [(P._b(r.Key), P._b(r.Value)) for r in rows or []], raw)
        return self._blk[b]

    def expect(self, key):
        """-> (state, blk_status, entry, value)"""
        b = bisect.bisect_right(self.fks, key) - 1
        if b < 0:
            return NO_BLOCK, 0, NONE32, None
        st, rows, raw = self.block(b)
        if st:
            return BLOCK_ERROR, st, b, None
        if raw is not None and len(raw) > _lib.GET_INFLATED_MAX:
            return FALLBACK, 0, b, None
        for k, v in rows:
            if k == key:
                return FOUND, 0, b, v
        return NOT_IN_BLOCK, 0, b, None

    def get(self, keys, **kw):
        kw.setdefault("zstd", True)
        return G.get_rows(self.decoder, self.dseg[0], self.dseg[1], self.ix, list(keys),
                          compression=ZSTD, **kw)

    def check(self, keys, res=None, **kw):
        """Every key == the oracle: state, blk_status, entry, value, nil-ness, and val_off
        inside the inflated block."""
        res = self.get(keys, **kw) if res is None else res
        for i, key in enumerate(keys):
            st, bst, ent, v = self.expect(key)
            got = (int(res.state[i]), int(res.blk_status[i]), int(res.entry[i]))
            assert got == (st, bst, ent), (key[:24], got, (st, bst, ent))
            if st == FOUND:
                assert res.value(i) == (v or None), key[:24]
                assert int(res.val_len[i]) == len(v)
                off = int(res.val_off[i])
                assert self.block(ent)[2][off:off + len(v)] == v, key[:24]
            else:
                assert int(res.val_len[i]) == 0 and int(res.val_off[i]) == 0
        want_fb = sum(self.expect(k)[0] == FALLBACK for k in keys)
        assert res.n_fallback == want_fb
        assert res.n_found == sum(self.expect(k)[0] == FOUND for k in keys)
        return res

    def floors(self, keys, bloom=None):
        return len({bisect.bisect_right(self.fks, k) for k in keys
                    if (bloom is None or bloom.test(k))} - {0})

    def close(self):
        self.ix.close()


def _all_keys(rows):
    return ([k for k, _ in rows] + [k + b"\x01" for k, _ in rows] + [b"", b"a-key-below"])


@pytest.fixture(scope="module")
def rows300():
    return ZC._rows(41, 300)


@pytest.fixture(scope="module")
def small(decoder, rows300):
    seg, _flen, meta = Z.zstd_segment(rows300, 3584, 4096)
    s = Seg(decoder, seg, meta)
    assert len(s.descs) == 14
    yield s
    s.close()


def test_opt_in(decoder, small, rows300):
    """Without the flag every key of a zstd segment that reaches a block is FALLBACK; with
    the flag on COMP_NONE and COMP_LZ4 segments every output array is byte-equal."""
    keys = [k for k, _ in rows300[::7]]
    res = small.get(keys, zstd=False)
    assert all(int(s) == FALLBACK for s in res.state) and res.n_fallback == len(keys)
    assert decoder.last_path() == _lib.PATH_GET
    w = okv.SegmentWriter(3584, 4096)
    for k, v in rows300:
        w.WriteRow(k, v)
    _flen, meta = w.Close()
    data = w.data().tobytes()
    ix = okv.DeviceIndex.from_metadata(decoder, okv.bytes_to_metadata(meta))
    dseg = _dev(data)
    keys = _all_keys(rows300)
    for comp in (_lib.COMP_NONE, _lib.COMP_LZ4):
        a = G.get_rows(decoder, dseg[0], dseg[1], ix, keys, compression=comp)
        b = G.get_rows(decoder, dseg[0], dseg[1], ix, keys, compression=comp, zstd=True)
        assert decoder.last_path() == _lib.PATH_GET
        for f in COLS:
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (comp, f)
        assert a.val_arena.tobytes() == b.val_arena.tobytes()
        assert (a.n_found, a.n_fallback, a.val_bytes, a.blocks_searched) == \
            (b.n_found, b.n_fallback, b.val_bytes, b.blocks_searched)
    ix.close()


def test_every_row_small_blocks(decoder, small, rows300):
    """14 blocks of 4 KiB: every row key, every key + one byte, b"" and a key below the
    first == the oracle; no fallback; one inflate per distinct floor block."""
    keys = _all_keys(rows300)
    res = small.check(keys)
    assert res.n_fallback == 0 and res.n_found == len(rows300)
    assert res.blocks_searched == small.floors(keys) == 14
    assert decoder.last_path() == PATH_Z


def _frame_cases():
    """block -> (frame_fn of that block, the status the oracle must report)"""
    return {
        1: (lambda raw: Z.compress(raw)[:-3], _lib.BLK_ZSTD_ERROR),
        3: (lambda raw: Z.compress(raw) + Z.compress(b"\xa5" * 700), 0),
        5: (lambda raw: Z.compress(raw[:-5]), _lib.BLK_PANIC),
        7: (lambda raw: Z.compress(raw) + Z.skippable_frame(b"skip me" * 9, 3), 0),
        9: (lambda raw: Z.compress(raw[:1500]) + Z.compress(raw[1500:]), 0),
    }


@pytest.fixture(scope="module")
def shaped(decoder, rows300):
    fc = _frame_cases()
    seg, _flen, meta = Z.zstd_segment(
        rows300, 3584, 4096, frame_fn=lambda raw, i: fc[i][0](raw) if i in fc else Z.compress(raw))
    s = Seg(decoder, seg, meta)
    yield s
    s.close()


def test_frame_shapes(decoder, shaped, rows300):
    """One block each: a cut frame (6), a junk second frame (inflates past OriginalSize:
    OK, and the regrow path), a short frame (3), a skippable frame behind the first (OK),
    two frames (OK).  A failing block fails only its own keys."""
    for b, (_fn, want) in _frame_cases().items():
        assert shaped.block(b)[0] == want, b
    assert len(shaped.block(3)[2]) == shaped.descs[3][2] + 700
    keys = _all_keys(rows300)
    res = shaped.check(keys)
    assert decoder.last_path() == PATH_Z | _lib.PATH_ZSTD_REGROW
    seen = {(int(s), int(b)) for s, b in zip(res.state, res.blk_status)}
    assert {(BLOCK_ERROR, _lib.BLK_ZSTD_ERROR), (BLOCK_ERROR, _lib.BLK_PANIC), (FOUND, 0)} <= seen
    bad = sum(len(shaped.block(b)[1]) for b in (1, 5))
    assert bad == 0 and res.n_found == len(rows300) - sum(
        1 for k, _ in rows300 if shaped.expect(k)[0] != FOUND)
    assert res.n_found > len(rows300) * 10 // 14


def _one_block(decoder, rows, T=1 << 26):
    seg, _flen, meta = Z.zstd_segment(rows, T, 4096)
    s = Seg(decoder, seg, meta)
    assert len(s.descs) == 1
    return s


def test_arm_boundary(decoder):
    """Inflated lengths 65 536 (staged) and 65 537 (global) as one-row blocks; 5 957
    records of 11 bytes (65 527: the staged arm at its most records) and 5 958 (65 538:
    the global arm)."""
    for vl in (65526, 65527):
        rows = [(b"k%03d" % (vl % 1000), bytes((i * 7) & 255 for i in range(vl)))]
        s = _one_block(decoder, rows, 65536)
        assert s.descs[0][2] == vl + 10
        s.check([rows[0][0], rows[0][0] + b"x", b"", b"zzzz"])
        s.close()
    for n in (5957, 5958):
        rows = [(b"%04d" % i, b"v") for i in range(n)]
        s = _one_block(decoder, rows)
        assert s.descs[0][2] == 11 * n
        res = s.check([b"0000", b"%04d" % (n - 1), b"%04d" % (n // 2), b"absent", b"12345"])
        assert res.n_found == 3 and res.blocks_searched == 1
        s.close()


def test_large_blocks(decoder):
    """One block of 1 037 160 inflated bytes (6 000 rows) and a block holding one 200 KiB
    value: 200 spread keys plus absent ones, through the global arm."""
    rows = ZC._rows(7, 6000)
    s = _one_block(decoder, rows, 1 << 20)
    assert s.descs[0][2] == 1037160
    keys = [k for k, _ in rows[::30]] + [k + b"\x00" for k, _ in rows[::600]] + [b"", b"zz"]
    res = s.check(keys)
    assert res.n_found == 200 and res.blocks_searched == 1
    s.close()
    big = bytes(random.Random(5).getrandbits(8) for _ in range(200 * 1024))
    rows = [(b"a", b"small"), (b"big", big), (b"c", b"")]
    s = _one_block(decoder, rows)
    res = s.check([b"big", b"c", b"a", b"b", b"big"])
    assert res.n_found == 4
    s.close()


def test_the_cap(decoder):
    """A block that inflates to exactly OKV_GET_INFLATED_MAX bytes is found; one byte more
    is FALLBACK and n_fallback counts it."""
    for extra, want in ((0, FOUND), (1, FALLBACK)):
        v = bytes((1 << 24) - 7 + extra)
        s = _one_block(decoder, [(b"a", v)])
        assert s.descs[0][2] == (1 << 24) + extra
        res = s.get([b"a", b"b"])
        assert int(res.state[0]) == want and int(res.entry[0]) == 0
        if want == FOUND:
            got = res.value(0)
            assert len(got) == len(v)
            assert hashlib.sha256(got).digest() == hashlib.sha256(v).digest()
            assert int(res.val_off[0]) == 7 and int(res.state[1]) == NOT_IN_BLOCK
            assert res.n_fallback == 0 and res.n_found == 1
        else:
            assert int(res.state[1]) == FALLBACK and res.n_fallback == 2 and res.n_found == 0
            assert int(res.val_len[0]) == 0
        s.close()


def test_grouping(decoder, small, rows300):
    """300 keys on one block, one key in every block, a shuffled list with repeats:
    results independent of key order; a smaller call after a larger one (scratch reuse)."""
    blk = small.block(6)[1]
    one_block = [blk[i % len(blk)][0] if i % 3 else blk[i % len(blk)][0] + b"\x00"
                 for i in range(300)]
    res = small.check(one_block)
    assert res.blocks_searched == 1
    each = [small.block(b)[1][-1][0] for b in range(14)]
    res = small.check(each)
    assert res.blocks_searched == 14 and res.n_found == 14
    rng = random.Random(3)
    keys = [rng.choice(rows300)[0] for _ in range(400)] + [b"nope"] * 5 + each
    res = small.check(keys)
    perm = list(range(len(keys)))
    rng.shuffle(perm)
    res2 = small.check([keys[j] for j in perm])
    for at, j in enumerate(perm):
        for f in ("state", "blk_status", "entry", "val_off", "val_len"):
            assert int(getattr(res2, f)[at]) == int(getattr(res, f)[j]), f
        assert res2.value(at) == res.value(j)
    small.check(_all_keys(rows300))  # a larger call ...
    res3 = small.check(each)         # ... then a smaller one over the same scratch
    assert res3.blocks_searched == 14


def test_filter(decoder, shaped, rows300):
    """A rejected key inflates no block, even when its floor block's frame is corrupt."""
    members = [k for k, _ in rows300[::9]]
    f = B.BloomFilter.with_estimates(len(members), 0.01)
    for k in members:
        f.add(k)
    bl = okv.DeviceBloom.from_bytes(decoder, f.to_bytes())
    lo, hi = shaped.fks[1], shaped.fks[2]  # block 1's frame is cut
    in_bad = [k for k, _ in rows300 if lo <= k < hi]
    assert in_bad and shaped.block(1)[0] == _lib.BLK_ZSTD_ERROR
    keys = members + [k + b"\x02" for k, _ in rows300[::5]] + in_bad
    res = shaped.get(keys, bloom=bl)
    for i, k in enumerate(keys):
        if not f.test(k):
            assert int(res.state[i]) == BLOOM_NEG and int(res.entry[i]) == NONE32, k
        else:
            st, bst, ent, v = shaped.expect(k)
            assert (int(res.state[i]), int(res.blk_status[i]), int(res.entry[i])) == (st, bst, ent)
            if st == FOUND:
                assert res.value(i) == (v or None)
    assert res.blocks_searched == shaped.floors(keys, f)
    only_rejected = [k for k in in_bad if not f.test(k)]
    assert only_rejected
    res = shaped.get(only_rejected, bloom=bl)
    assert res.blocks_searched == 0 and all(int(s) == BLOOM_NEG for s in res.state)
    bl.close()


def test_descriptors(decoder):
    """Behind a one-entry index: CompressedSize > BlockSize is PANIC, off >= len EOF, a
    short read SHORT, and a 131 072-byte BlockSize around a small frame is taken."""
    raw = b"".join(struct.pack("<HI", len(k), len(v)) + k + v
                   for k, v in [(b"apple", b"red"), (b"fig", b""), (b"pear", b"green" * 9)])
    frame = Z.compress(raw)
    seg = frame + bytes(131072 - len(frame)) + bytes(64)
    n, c = len(seg), len(frame)
    keys = [b"apple", b"fig", b"pear", b"plum", b""]
    for d, want in (((0, 4096, len(raw), 4097), (BLOCK_ERROR, _lib.BLK_PANIC)),
                    ((n, 4096, len(raw), c), (BLOCK_ERROR, _lib.BLK_EOF)),
                    ((n + 77, 4096, len(raw), c), (BLOCK_ERROR, _lib.BLK_EOF)),
                    ((4096, n, len(raw), c), (BLOCK_ERROR, _lib.BLK_SHORT)),
                    ((0, 131072, len(raw), c), None),
                    ((0, c, len(raw), c), None)):
        s = Seg(decoder, seg, None, [d], [b""])
        res = s.check(keys)
        if want:
            assert all((int(a), int(b)) == want for a, b in zip(res.state, res.blk_status)), d
            assert res.blocks_searched == 0
        else:
            assert [int(x) for x in res.state] == [FOUND, FOUND, FOUND, NOT_IN_BLOCK, NOT_IN_BLOCK]
            assert res.blocks_searched == 1
        s.close()


def test_modes(decoder, small, rows300):
    """Host mode == device-pointer mode byte for byte; values=False; OKV_E_CAPACITY with
    the arrays and totals set and the arena untouched; sync=False then totals()."""
    keys = [k for k, _ in rows300[::4]] + [b"nope", b""]
    res = small.check(keys)
    pos = res.val_bytes
    r = small.get(keys, values=False)
    assert r.val_arena is None and r.val_bytes == pos
    for f in COLS:
        assert getattr(r, f).tobytes() == getattr(res, f).tobytes(), f
    with pytest.raises(okv.OkvError) as e:
        small.get(keys, val_cap=pos - 16)
    assert e.value.code == _lib.OKV_E_CAPACITY
    r = e.value.result
    assert (r.val_bytes, r.n_found, r.blocks_searched) == (pos, res.n_found, res.blocks_searched)
    assert not r.val_arena.any() and list(r.state) == list(res.state)
    assert list(r.val_off) == list(res.val_off)

    pk = pack_keys(keys)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    dk = {k: torch.from_numpy(v.copy().view(signed.get(v.dtype, v.dtype))).cuda()
          for k, v in pk.items()}
    n = len(keys)
    for sync in (True, False):
        out = {"state": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
               "blk_status": torch.full((n,), -1, dtype=torch.int32, device="cuda"),
               "entry": torch.zeros(n, dtype=torch.int32, device="cuda"),
               "val_off": torch.zeros(n, dtype=torch.int64, device="cuda"),
               "val_len": torch.zeros(n, dtype=torch.int32, device="cuda"),
               "val_pos": torch.zeros(n, dtype=torch.int64, device="cuda"),
               "val_arena": torch.full((pos + 64,), 0xEE, dtype=torch.uint8, device="cuda")}
        torch.cuda.synchronize()
        G.get_rows(decoder, small.dseg[0], small.dseg[1], small.ix, dk, compression=ZSTD,
                   out=out, sync=sync, n_rows=n, key_arena_bytes=int(pk["key_arena"].size),
                   zstd=True)
        decoder.sync()
        assert G.totals(decoder) == {"n_found": res.n_found, "n_fallback": 0, "val_bytes": pos,
                                     "blocks_searched": res.blocks_searched}
        for f in COLS:
            assert out[f].cpu().numpy().tobytes() == getattr(res, f).tobytes(), f
        arena = out["val_arena"].cpu().numpy()
        assert arena[:pos].tobytes() == res.val_arena[:pos].tobytes()
        assert (arena[pos:] == 0xEE).all()


@pytest.mark.parametrize("T,D", [(3584, 4096), (61440, 65536)])
def test_own_writer(decoder, T, D):
    """Segments of the device zstd encoder (zstd_native=True) are read back: every key is
    found with its value."""
    rows = ZC._rows(23, 1500 if D == 65536 else 300)
    enc = okv.Encoder(0)
    out = enc.encode(rows, T, D, ZSTD, zstd_native=True)
    seg, meta = out.seg.tobytes(), out.meta()
    enc.close()
    s = Seg(decoder, seg, meta)
    assert len(s.descs) > 1
    keys = [k for k, _ in rows]
    res = s.check(keys)
    assert res.n_found == len(rows) and res.n_fallback == 0
    s.close()


def _both(reader, keys):
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
    return got


def test_reader(decoder, small, shaped, rows300):
    """SegmentReader.GetRows(keys) == [GetRow(k)], exceptions included, on the plain and the
    frame-shape fixtures; one upload, and at most two device calls per batch."""
    keys = _all_keys(rows300)[::3]
    for s in (small, shaped):
        rd = R.SegmentReader(s.seg, len(s.seg), decoder)
        rd.FetchAndLoadMetadata()
        before = rd.io_stats()
        got = rd.GetRows(keys)
        a = rd.io_stats()
        assert a["bytes_staged"] - before["bytes_staged"] == len(s.seg)
        assert 1 <= a["calls"] - before["calls"] <= 2
        rd.GetRows(keys[:40])
        b = rd.io_stats()
        assert b["bytes_staged"] == a["bytes_staged"] and 1 <= b["calls"] - a["calls"] <= 2
        # (a key longer than 65 535 bytes takes the single-key path)
        _both(rd, keys + [b"x" * 70000, rows300[3][0] + b"y" * 66000])
        n_found = sum(s.expect(k)[0] == FOUND for k in keys)
        assert sum(isinstance(g, R.KVPair) for g in got) == n_found
