"""Caller buffers of okv_get_rows and okv_snap_get_rows (device mode): the
segment, the key arrays and every output are tests/guarded.py frames -- no
zero bytes behind the segment or the key arena, every per-key array of exactly
n entries, the value arena of exactly val_bytes -- at base 0 and base 16 of a
128-byte line, under two poisons.

  G  guards of every frame intact after every call;
  X  states, floor entries, value offsets and lengths equal the oracle's
     GetRow; val_arena[0, val_bytes) is the found values, each zero-padded to
     16 bytes, tiling the extent;
  N  OKV_E_CAPACITY: val_arena is not written, the per-key arrays and totals
     are set; OKV_E_ARG (misaligned base): nothing is written;
  D  seg_bytes % 16 != 0: the 16-byte loads reach past the segment."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import objectkv_amd as okv
from objectkv_amd import _lib
from objectkv_amd import snap as S
from objectkv_amd.bloom import DeviceBloom, pack_keys
from oracle import bloom_ref as B
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import guarded as G
from tests.test_get_gpu import BLOOM_NEG, FOUND, NO_BLOCK, NOT_IN_BLOCK, _oracle_state
from tests.test_snap_get_gpu import Oracle as SnapOracle
from tests.test_snap_get_gpu import _seg

pytestmark = pytest.mark.gpu

POISONS = [0xA5, 0x5A]
BASES = [0, 16]
NONE32 = 0xFFFFFFFF
DEV = _lib.F_DEVICE_PTRS
GET_COLS = (("state", np.int32), ("blk_status", np.int32), ("entry", np.uint32),
            ("val_off", np.uint64), ("val_len", np.uint32), ("val_pos", np.uint64))
SNAP_COLS = (("state", np.int32), ("seg", np.uint32)) + GET_COLS[1:]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _r16(n):
    return (n + 15) & ~15


# ---- one three-block segment with a filter, and 65 keys ------------------------


def _rows():
    """Even-numbered keys; values of 0..90 bytes (one nil), few multiples of 16."""
    return [(b"k%06d" % i, b"" if i == 140 else b"v%06d" % i * (1 + i % 13)) for i in
            range(100, 420, 2)]


_CACHE = {}


def _segment(kind):
    """(file bytes, meta, compression, oracle reader, filter) -- 'plain': a writer
    segment with a small bloom filter; 'zstd': the same rows, zstd blocks."""
    if kind not in _CACHE:
        rows = _rows()
        if kind == "plain":
            f = B.BloomFilter(1024, 2)
            w = P.SegmentWriter(P.SegmentWriterOptions(BloomFilter=f))
            for k, v in rows:
                w.WriteRow(k, v)
            n, meta = w.Close()
            seg, comp = bytes(w.external), _lib.COMP_NONE
            assert n == len(seg)
        else:
            seg, n, meta = Z.zstd_segment(rows, 3584, 4096, level=3)
            seg, comp, f = bytes(seg[:n]), _lib.COMP_ZSTD, None
        md = P.bytes_to_metadata(meta)
        assert len(md.entries) == 3 and len(seg) % 16 != 0
        _CACHE[kind] = (seg, meta, comp, P.SegmentReader(seg, len(seg)), f, md)
    return _CACHE[kind]


def _keys(kind):
    """65 keys: found ones from every block (the nil value among them), absent
    keys the filter lets through and absent keys it rejects, a key below the
    first key, the empty key."""
    seg, meta, comp, orr, f, md = _segment(kind)
    rows = _rows()
    found = [rows[i][0] for i in range(0, len(rows), 5)][:33] + [b"k%06d" % 140]
    odd = [b"k%06d" % i for i in range(101, 421, 2)]
    if f is not None:
        passed = [k for k in odd if f.test(k)][:12]
        rejected = [k for k in odd if not f.test(k)][:12]
        assert len(passed) >= 6 and len(rejected) == 12
    else:
        passed, rejected = odd[:12], odd[40:52]
    below = [k for k in (b"a%04d" % i for i in range(4000)) if f is None or f.test(k)][:3]
    assert len(below) == 3  # below the first key and past the filter: no floor block
    keys = found + passed + rejected + below + [b"a-below-the-first-key", b"", b"k", b"zzzz"]
    keys = (keys + odd[60:])[:65]
    assert len(keys) == 65
    rng = np.random.default_rng(9)
    return [keys[i] for i in rng.permutation(65)]


def _expected(kind):
    """Per key (state, blk_status, value, floor entry or None)."""
    seg, meta, comp, orr, f, md = _segment(kind)
    firsts = [st.FirstKey for st in md.entries]
    out = []
    for k in _keys(kind):
        st, bst, v = _oracle_state(orr, k)
        floor = max((i for i, fk in enumerate(firsts) if fk <= k), default=None)
        out.append((st, bst, P._b(v) if st == FOUND else b"", floor))
    states = {e[0] for e in out}
    assert {FOUND, NOT_IN_BLOCK, NO_BLOCK} <= states
    if f is not None:
        assert BLOOM_NEG in states
    return out


class Keys:
    """The key arrays of okv_rows in frames of exactly their extents."""

    def __init__(self, keys, poison, base):
        k = pack_keys(keys)
        kb = int(k["key_len"].sum())
        kw = dict(base_mod=base, poison=poison, device=_dev())
        self.f = {"key_arena": G.frame_input(k["key_arena"][:kb], **kw),
                  "key_off": G.frame_input(k["key_off"], np.uint64, **kw),
                  "key_len": G.frame_input(k["key_len"], np.uint16, **kw)}
        self.c = _lib.Rows(self.f["key_arena"].ptr, self.f["key_off"].ptr, self.f["key_len"].ptr,
                           None, None, None, len(keys), kb, 0)

    def check(self):
        for name, f in self.f.items():
            f.check("keys." + name)


class Outs:
    """The per-key arrays (n entries each) and the value arena (val_cap bytes)."""

    def __init__(self, cols, n, val_cap, poison, base):
        kw = dict(base_mod=base, poison=poison, device=_dev())
        self.cols = cols
        self.f = {name: G.frame(n, dt, **kw) for name, dt in cols}
        self.f["val_arena"] = G.frame(val_cap, np.uint8, **kw)

    def ptrs(self, values=True):
        p = [self.f[name].ptr for name, _ in self.cols]
        if not values:
            p[-1] = None  # val_pos
        return p

    def check(self):
        for name, f in self.f.items():
            f.check(name)

    def untouched(self):
        for name, f in self.f.items():
            f.untouched(name)


def _assert_arena(h, val_bytes, want_vals):
    """val_arena[0, val_bytes): the found values at val_pos, each zero-padded to
    16 bytes, the padded regions tiling the extent with no gap."""
    found = [i for i, v in enumerate(want_vals) if v is not None]
    want = np.zeros(val_bytes, np.uint8)
    spans = []
    for i in found:
        v, pos = want_vals[i], int(h["val_pos"][i])
        assert pos % 16 == 0 and pos + _r16(len(v)) <= val_bytes, (i, pos)
        want[pos:pos + len(v)] = np.frombuffer(v, np.uint8)
        if v:
            spans.append((pos, _r16(len(v))))
    spans.sort()
    at = 0
    for pos, n in spans:
        assert pos == at, ("gap or overlap in val_arena at", at, pos)
        at += n
    assert at == val_bytes == sum(_r16(len(want_vals[i])) for i in found)
    bad = np.flatnonzero(h["val_arena"][:val_bytes] != want)
    assert not bad.size, ("val_arena differs, first at", int(bad[0]), "of", val_bytes)


# ---- okv_get_rows ------------------------------------------------------------------


class GetEnv:
    def __init__(self, dec, kind, poison, base):
        self.dec, self.kind = dec, kind
        seg, meta, comp, orr, f, md = _segment(kind)
        self.seg_bytes, self.comp = len(seg), comp
        self.seg = G.frame_input(seg, base_mod=base, poison=poison, device=_dev())
        self.ix = okv.DeviceIndex.from_metadata(dec, okv.bytes_to_metadata(meta))
        self.bloom = DeviceBloom.from_bytes(dec, f.to_bytes()) if f is not None else None
        self.keys = Keys(_keys(kind), poison, base)
        self.flags = DEV | (_lib.F_GET_ZSTD if kind == "zstd" else 0)

    def call(self, outs: Outs, val_cap, values=True, seg_ptr=None, arena_ptr=None):
        o = _lib.GetOut(*outs.ptrs(values),
                        (arena_ptr or outs.f["val_arena"].ptr) if values else None,
                        val_cap, 0, 0, 0, 0)
        rc = _lib.lib().okv_get_rows(
            self.dec._ctx, seg_ptr or self.seg.ptr, self.seg_bytes, self.ix._h,
            self.bloom._h if self.bloom is not None else None, C.byref(self.keys.c), self.comp,
            C.byref(o), self.flags)
        return rc, o

    def guards(self, outs):
        self.seg.check("seg")
        self.keys.check()
        outs.check()

    def close(self):
        self.ix.close()
        if self.bloom is not None:
            self.bloom.close()


def _inflated(seg, md, entry):
    """The inflated bytes of block `entry` of a zstd segment."""
    d = md.entries[entry].desc()
    return Z.decompress(seg[d[0]:d[0] + d[3]], d[2])


def _assert_get_keys(h, exp, seg, kind):
    md = _segment(kind)[5]
    for i, (st, bst, v, floor) in enumerate(exp):
        assert int(h["state"][i]) == st, (i, int(h["state"][i]), st)
        if bst is not None:
            assert int(h["blk_status"][i]) == bst, i
        if st == FOUND:
            assert int(h["val_len"][i]) == len(v), i
            off = int(h["val_off"][i])
            # (in a zstd segment val_off counts inside the inflated block entry[i])
            src = seg if kind == "plain" else _inflated(seg, md, int(h["entry"][i]))
            assert src[off:off + len(v)] == v, i
        else:
            assert int(h["val_len"][i]) == 0 and int(h["val_off"][i]) == 0, i
        if st in (FOUND, NOT_IN_BLOCK):
            assert int(h["entry"][i]) == floor, i
        if st in (NO_BLOCK, BLOOM_NEG):  # no floor block was looked up
            assert int(h["entry"][i]) == NONE32, i


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("kind", ["plain", "zstd"])
def test_get_rows(decoder, kind, poison, base):
    """Index only (no val_pos, no val_arena), then values into an arena of
    exactly val_bytes, then the arena 16 bytes short (N), on the same frames."""
    exp = _expected(kind)
    seg = _segment(kind)[0]
    n = len(exp)
    want_bytes = sum(_r16(len(v)) for st, _b, v, _f in exp if st == FOUND)
    want_vals = [v if st == FOUND else None for st, _b, v, _f in exp]
    env = GetEnv(decoder, kind, poison, base)
    try:
        # index only
        outs = Outs(GET_COLS, n, 0, poison, base)
        rc, o = env.call(outs, 0, values=False)
        env.guards(outs)
        assert rc == 0, decoder.error()
        assert decoder.last_path() == _lib.PATH_GET | (_lib.PATH_ZSTD if kind == "zstd" else 0)
        assert o.n_found == sum(1 for e in exp if e[0] == FOUND) and o.val_bytes == want_bytes
        h = {k: f.host() for k, f in outs.f.items()}
        _assert_get_keys(h, exp, seg, kind)
        outs.f["val_pos"].untouched("val_pos")
        outs.f["val_arena"].untouched("val_arena")
        # values, val_cap == val_bytes exactly
        outs = Outs(GET_COLS, n, want_bytes, poison, base)
        rc, o = env.call(outs, want_bytes)
        env.guards(outs)
        assert rc == 0, decoder.error()
        assert (o.val_bytes, o.blocks_searched) == (want_bytes, 3)
        assert decoder.last_path() == _lib.PATH_GET | (_lib.PATH_ZSTD if kind == "zstd" else 0)
        full = {k: f.host() for k, f in outs.f.items()}
        _assert_get_keys(full, exp, seg, kind)
        _assert_arena(full, want_bytes, want_vals)
        # N: 16 bytes short
        outs = Outs(GET_COLS, n, want_bytes - 16, poison, base)
        rc, o = env.call(outs, want_bytes - 16)
        env.guards(outs)
        assert rc == _lib.OKV_E_CAPACITY
        outs.f["val_arena"].untouched("val_arena")
        assert (o.val_bytes, o.n_found) == (want_bytes, sum(1 for e in exp if e[0] == FOUND))
        h = {k: f.host() for k, f in outs.f.items()}
        _assert_get_keys(h, exp, seg, kind)
        for name in ("state", "blk_status", "entry", "val_off", "val_len"):
            assert np.array_equal(h[name], full[name]), name
    finally:
        env.close()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("which", ["seg", "val_arena"])
def test_get_rows_misaligned_base_is_refused(decoder, which, poison, base):
    exp = _expected("plain")
    want_bytes = sum(_r16(len(v)) for st, _b, v, _f in exp if st == FOUND)
    env = GetEnv(decoder, "plain", poison, base)
    try:
        outs = Outs(GET_COLS, len(exp), want_bytes + 8, poison, base)
        if which == "seg":
            env.seg_bytes -= 8
            rc, _o = env.call(outs, want_bytes, seg_ptr=env.seg.ptr + 8)
        else:
            rc, _o = env.call(outs, want_bytes, arena_ptr=outs.f["val_arena"].ptr + 8)
        assert rc == _lib.OKV_E_ARG
        env.guards(outs)
        outs.untouched()
    finally:
        env.close()


# ---- okv_snap_get_rows ---------------------------------------------------------------


class ZSnapOracle(SnapOracle):
    """The expectation under OKV_F_GET_ZSTD: test_snap_get_zstd_gpu.ZEnv's, over the
    oracle's readers alone (no device objects)."""
    from tests.test_snap_get_zstd_gpu import ZEnv as _Z
    candidate, _zexpect = _Z.candidate, _Z.expect

    def expect(self, key):
        return self._zexpect(key, set())


def _snap_segments(kind="plain"):
    """Three segments: an old level-1 segment of three blocks, a newer level-0
    one with a newer version of some keys and a tombstone, and a level-0 one
    beside them.  kind 'zstd': the old one is a zstd segment."""
    if "snap" + kind not in _CACHE:
        base_rows = _rows()
        newer = [(k, b"new-" + v) for k, v in base_rows[10:60:7]] + [(base_rows[30][0], b"")]
        newer = sorted(dict(newer).items())
        beside = [(b"k%06d" % i, b"w%04d" % i * (1 + i % 5)) for i in range(461, 521, 2)]
        old = _seg(1, 1, base_rows)
        if kind == "zstd":
            data, n, meta = Z.zstd_segment(base_rows, 3584, 4096, level=3)
            old = (1, 1, bytes(data[:n]), n, meta)
            assert n % 16 != 0  # the 16-byte loads of the zstd arms reach past the segment
        segs = [old, _seg(2, 0, newer), _seg(3, 0, beside)]
        assert len(P.bytes_to_metadata(segs[0][4]).entries) == 3
        _CACHE["snap" + kind] = (segs, (ZSnapOracle if kind == "zstd" else SnapOracle)(segs))
    return _CACHE["snap" + kind]


def _snap_keys():
    rows = _rows()
    keys = [k for k, _ in rows[::4]] + [rows[30][0], rows[17][0], rows[24][0]]
    keys += [b"k%06d" % i for i in range(463, 475)] + [b"k%06d" % i for i in range(101, 121, 2)]
    keys += [b"", b"a", b"zz"]
    keys = (keys + [k for k, _ in rows[1::4]])[:65]
    assert len(keys) == 65
    rng = np.random.default_rng(10)
    return [keys[i] for i in rng.permutation(65)]


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("kind", ["plain", "zstd"])
def test_snap_get_rows(decoder, kind, poison, base):
    """Three framed segments, 65 framed keys: index only, values into exactly
    val_bytes, the arena 16 bytes short (N).  kind 'zstd': the three-block
    segment is a zstd one and the call carries OKV_F_GET_ZSTD -- the plan, pack,
    inflate and search arms read the framed segment, and the values kernel
    copies from the inflated blocks into the framed arena."""
    segs, orc = _snap_segments(kind)
    flags = DEV | (_lib.F_GET_ZSTD if kind == "zstd" else 0)
    want_path = _lib.PATH_SNAP_GET | (_lib.PATH_ZSTD if kind == "zstd" else 0)
    keys = _snap_keys()
    exp = [orc.expect(k)[0] for k in keys]  # (state, segment ID, blk_status, value)
    states = {e[0] for e in exp}
    assert {S.SNAP_FOUND, S.SNAP_NO_ROWS, S.SNAP_DELETED} <= states
    assert any(e[0] == S.SNAP_FOUND and e[1] == 2 for e in exp)  # a newer version wins
    assert any(e[0] == S.SNAP_FOUND and e[1] == 1 for e in exp)  # the (zstd) old one answers
    want_vals = [P._b(e[3]) if e[0] == S.SNAP_FOUND else None for e in exp]
    want_bytes = sum(_r16(len(v)) for v in want_vals if v is not None)
    kw = dict(base_mod=base, poison=poison, device=_dev())
    frames, ixs, tuples = [], [], []
    for sid, lvl, data, n, meta in segs:
        assert n == len(data)
        fr = G.frame_input(data, **kw)
        ix = okv.DeviceIndex.from_metadata(decoder, okv.bytes_to_metadata(meta))
        pmd = P.bytes_to_metadata(meta)
        frames.append(fr)
        ixs.append(ix)
        comp = _lib.COMP_ZSTD if pmd.compression == P.COMP_ZSTD else _lib.COMP_NONE
        assert (comp == _lib.COMP_ZSTD) == (kind == "zstd" and sid == 1)
        tuples.append((fr.ptr, n, ix, None, comp, lvl, sid, pmd.FirstKey, pmd.LastKey))
    assert any(len(d) % 16 for _s, _l, d, _n, _m in segs)
    snap = S.DeviceSnapshot(decoder, tuples)
    K = Keys(keys, poison, base)
    n = len(keys)

    def call(outs, cap, values=True):
        o = _lib.SnapOut(*outs.ptrs(values), outs.f["val_arena"].ptr if values else None, cap,
                         0, 0, 0, 0, 0, 0)
        rc = _lib.lib().okv_snap_get_rows(decoder._ctx, snap._h, C.byref(K.c), C.byref(o), flags)
        for fr in frames:
            fr.check("segment")
        K.check()
        outs.check()
        return rc, o

    def assert_keys(h):
        for i, (st, sid, bst, v) in enumerate(exp):
            assert int(h["state"][i]) == st, (i, keys[i])
            assert int(h["blk_status"][i]) == bst, i
            if sid is None:
                assert int(h["seg"][i]) == NONE32, i
            else:
                assert snap.ids[int(h["seg"][i])] == sid, i
            if st == S.SNAP_FOUND:
                v = P._b(v)
                at = [s[0] for s in segs].index(sid)
                data = segs[at][2]
                if kind == "zstd" and sid == 1:  # inside the inflated block entry[i]
                    data = _inflated(data, P.bytes_to_metadata(segs[at][4]), int(h["entry"][i]))
                off = int(h["val_off"][i])
                assert int(h["val_len"][i]) == len(v) and data[off:off + len(v)] == v, i
            else:
                assert int(h["val_len"][i]) == 0 and int(h["val_off"][i]) == 0, i

    try:
        outs = Outs(SNAP_COLS, n, 0, poison, base)
        rc, o = call(outs, 0, values=False)
        assert rc == 0, decoder.error()
        assert decoder.last_path() == want_path
        assert o.val_bytes == want_bytes
        assert_keys({k: f.host() for k, f in outs.f.items()})
        outs.f["val_pos"].untouched("val_pos")
        outs.f["val_arena"].untouched("val_arena")

        outs = Outs(SNAP_COLS, n, want_bytes, poison, base)
        rc, o = call(outs, want_bytes)
        assert rc == 0, decoder.error()
        assert decoder.last_path() == want_path
        full = {k: f.host() for k, f in outs.f.items()}
        assert_keys(full)
        assert (o.val_bytes, o.n_found, o.n_deleted) == (
            want_bytes, sum(1 for e in exp if e[0] == S.SNAP_FOUND),
            sum(1 for e in exp if e[0] == S.SNAP_DELETED))
        _assert_arena(full, want_bytes, want_vals)

        outs = Outs(SNAP_COLS, n, want_bytes - 16, poison, base)
        rc, o = call(outs, want_bytes - 16)
        assert rc == _lib.OKV_E_CAPACITY
        outs.f["val_arena"].untouched("val_arena")
        assert o.val_bytes == want_bytes
        h = {k: f.host() for k, f in outs.f.items()}
        assert_keys(h)
        for name in ("state", "seg", "blk_status", "entry", "val_off", "val_len"):
            assert np.array_equal(h[name], full[name]), name

        # misaligned bases (base + 8 inside the frames): a value arena is refused with
        # nothing written, a segment is refused by okv_snap_new
        outs = Outs(SNAP_COLS, n, want_bytes + 8, poison, base)
        o = _lib.SnapOut(*outs.ptrs(), outs.f["val_arena"].ptr + 8, want_bytes, 0, 0, 0, 0, 0, 0)
        assert _lib.lib().okv_snap_get_rows(decoder._ctx, snap._h, C.byref(K.c), C.byref(o),
                                            flags) == _lib.OKV_E_ARG
        outs.untouched()
        bad = list(tuples[0])
        bad[0], bad[1] = bad[0] + 8, bad[1] - 8
        with pytest.raises(okv.OkvError) as e:
            S.DeviceSnapshot(decoder, [tuple(bad)] + tuples[1:])
        assert e.value.code == _lib.OKV_E_ARG
    finally:
        snap.close()
        for ix in ixs:
            ix.close()
