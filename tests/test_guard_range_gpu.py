"""Caller buffers of the range, merge, bloom and hash entry points (device
mode): okv_seek_rows, okv_gather_rows, okv_merge_rows, okv_bloom_test_rows,
okv_bloom_write_to and okv_hash_blocks with every device input and output in a
tests/guarded.py frame of exactly its extent -- source arenas with no spare
bytes behind them, per-row arrays of exactly n entries -- at base 0 and base 16
of a 128-byte line, under two poisons.

  G  guards of every frame intact after every call, capacity errors included;
  X  outputs equal the references of the existing tests (pyoracle's RowIter,
     the sequential gather layout, test_merge_gpu's references, bloom_ref, the
     writer's BlockStat.Hash);
  N  okv_gather_rows on OKV_E_CAPACITY: "the arenas are not written";
     OKV_E_ARG for a misaligned arena: nothing is written."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from objectkv_amd import _lib
from objectkv_amd.bloom import DeviceBloom, pack_keys
from oracle import bloom_ref as B
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO
from tests import guarded as G
from tests import seek_cases as SK
from tests.test_merge_gpu import _small_streams, ref_all

pytestmark = pytest.mark.gpu

POISONS = [0xA5, 0x5A]
BASES = [0, 16]
DEV = _lib.F_DEVICE_PTRS
ASC, DESC = _lib.DIR_ASC, _lib.DIR_DESC
U64 = (1 << 64) - 1


def _dev():
    import torch
    return torch.device("cuda", 0)


def _r16(n):
    return (n + 15) & ~15


class Keys:
    """The key arrays of okv_rows in frames of exactly their extents."""

    def __init__(self, keys, kw):
        k = pack_keys(keys)
        kb = int(k["key_len"].sum())
        self.f = {"key_arena": G.frame_input(k["key_arena"][:kb], **kw),
                  "key_off": G.frame_input(k["key_off"], np.uint64, **kw),
                  "key_len": G.frame_input(k["key_len"], np.uint16, **kw)}
        self.c = _lib.Rows(self.f["key_arena"].ptr, self.f["key_off"].ptr, self.f["key_len"].ptr,
                           None, None, None, len(keys), kb, 0)

    def check(self):
        for name, f in self.f.items():
            f.check("keys." + name)


class Source:
    """Decoded rows as a merge / gather / seek input: the six arrays of
    okv_merge_src in frames, the arenas ending at their last byte."""

    def __init__(self, rows, kw, level=1, first=None):
        self.rows, self.level, self.lo, self.hi = rows, level, 0, len(rows)
        kl = np.array([len(k) for k, _ in rows], np.uint16)
        vl = np.array([len(v or b"") for _, v in rows], np.uint32)
        self.ko = np.concatenate([[0], np.cumsum(kl, dtype=np.uint64)[:-1]]).astype(np.uint64)
        self.vo = np.concatenate([[0], np.cumsum(vl, dtype=np.uint64)[:-1]]).astype(np.uint64)
        self.kl, self.vl = kl, vl
        self.f = {"key_arena": G.frame_input(b"".join(k for k, _ in rows), **kw),
                  "key_off": G.frame_input(self.ko, np.uint64, **kw),
                  "key_len": G.frame_input(kl, np.uint16, **kw),
                  "val_arena": G.frame_input(b"".join(v or b"" for _, v in rows), **kw),
                  "val_off": G.frame_input(self.vo, np.uint64, **kw),
                  "val_len": G.frame_input(vl, np.uint32, **kw)}
        if first is not None:
            self.f["first"] = G.frame_input(np.array(first, np.uint64), np.uint64, **kw)
        self.ka, self.va = self.f["key_arena"].ptr, self.f["val_arena"].ptr

    def merge_src(self):
        f = self.f
        return _lib.MergeSrc(f["key_arena"].ptr, f["key_off"].ptr, f["key_len"].ptr,
                             f["val_arena"].ptr, f["val_off"].ptr, f["val_len"].ptr, self.lo,
                             self.hi, self.level, 0)

    def check(self):
        for name, f in self.f.items():
            f.check("source." + name)


def _src_array(sources):
    arr = (_lib.MergeSrc * len(sources))()
    for i, s in enumerate(sources):
        arr[i] = s.merge_src()
    return arr


# ---- okv_seek_rows -------------------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_seek_rows(decoder, poison, base):
    """65 (source, key, direction) triples over the seek cases' segments: row_lo
    and row_hi of exactly 65 entries equal pyoracle's RowIter."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    sources, triples = [], []
    for s, (_name, keys, first, qs) in enumerate(SK.cases()):
        sources.append(Source([(k, b"") for k in keys], kw, first=first))
        triples += [(s, q, d, lo, hi) for q, d, lo, hi in qs]
    random.Random(5).shuffle(triples)
    batch = triples[:65]
    n = len(batch)
    assert n == 65 and len({b[0] for b in batch}) == 3 and {b[2] for b in batch} == {ASC, DESC}
    arr = (_lib.SeekSrc * len(sources))()
    for i, s in enumerate(sources):
        arr[i] = _lib.SeekSrc(s.f["key_arena"].ptr, s.f["key_off"].ptr, s.f["key_len"].ptr,
                              s.f["first"].ptr, len(s.rows), s.f["first"].n_items - 1)
    K = Keys([b[1] for b in batch], kw)
    src_of = G.frame_input(np.array([b[0] for b in batch], np.uint32), np.uint32, **kw)
    dirs = G.frame_input(np.array([b[2] for b in batch], np.uint8), np.uint8, **kw)
    lo, hi = G.frame(n, np.uint64, **kw), G.frame(n, np.uint64, **kw)
    rc = _lib.lib().okv_seek_rows(decoder._ctx, arr, len(sources), C.byref(K.c), src_of.ptr,
                                  dirs.ptr, lo.ptr, hi.ptr, DEV)
    for fr, what in ((lo, "row_lo"), (hi, "row_hi"), (src_of, "src_of"), (dirs, "direction")):
        fr.check(what)
    K.check()
    for s in sources:
        s.check()
    assert rc == 0, decoder.error()
    assert lo.host().tolist() == [b[3] for b in batch]
    assert hi.host().tolist() == [b[4] for b in batch]


# ---- okv_gather_rows ------------------------------------------------------------------


def _gather_rows(seed):
    """Ascending rows whose key and value lengths cover 0, 1, 15, 16, 17 and a
    few hundred bytes, so the offsets take every misalignment."""
    rng = random.Random(seed)
    rows = []
    for i in range(40):
        kl = rng.choice((1, 2, 15, 16, 17, 33)) + 4
        vl = rng.choice((0, 1, 15, 16, 17, 31, 300))
        rows.append(((b"%04d" % i + bytes(rng.getrandbits(8) for _ in range(kl)))[:kl],
                     bytes(rng.getrandbits(8) for _ in range(vl))))
    return rows


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_gather_rows(decoder, poison, base):
    """65 picks from two sources: the size query (both arenas NULL), the arenas
    one 16 short in turn (OKV_E_CAPACITY: the totals and the four per-row arrays
    are set, the arenas are not written), then exact capacities."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    sources = [Source(_gather_rows(s), kw) for s in (1, 2)]
    rng = random.Random(65)
    picks = [(rng.randrange(2), rng.randrange(40)) for _ in range(65)]
    n = len(picks)
    arr = _src_array(sources)
    src = G.frame_input(np.array([p[0] for p in picks], np.uint32), np.uint32, **kw)
    row = G.frame_input(np.array([p[1] for p in picks], np.uint64), np.uint64, **kw)
    want = {"key_pos": [], "key_len": [], "val_pos": [], "val_len": []}
    karena, varena = bytearray(), bytearray()
    for s, r in picks:
        k, v = sources[s].rows[r]
        want["key_pos"].append(len(karena))
        want["val_pos"].append(len(varena))
        want["key_len"].append(len(k))
        want["val_len"].append(len(v))
        karena += k + bytes(-len(k) % 16)
        varena += v + bytes(-len(v) % 16)
    kb, vb = len(karena), len(varena)
    cols = (("key_pos", np.uint64), ("key_len", np.uint16), ("val_pos", np.uint64),
            ("val_len", np.uint32))

    def call(kc, vc, arenas=True):
        f = {name: G.frame(n, dt, **kw) for name, dt in cols}
        f["key_arena"], f["val_arena"] = G.frame(kc, np.uint8, **kw), G.frame(vc, np.uint8, **kw)
        o = _lib.GatherOut(*[f[name].ptr for name, _ in cols],
                           f["key_arena"].ptr if arenas else None,
                           f["val_arena"].ptr if arenas else None, kc, vc, 0, 0)
        rc = _lib.lib().okv_gather_rows(decoder._ctx, arr, 2, src.ptr, row.ptr, n, C.byref(o), DEV)
        for name, fr in f.items():
            fr.check(name)
        src.check("src")
        row.check("row")
        for s in sources:
            s.check()
        assert (o.key_bytes, o.val_bytes) == (kb, vb)
        h = {name: fr.host() for name, fr in f.items()}
        for name, _ in cols:  # set by every call, refused ones included
            assert h[name].tolist() == want[name], name
        return rc, f, h

    rc, f, _h = call(0, 0, arenas=False)
    assert rc == 0, decoder.error()
    for kc, vc in ((kb - 16, vb), (kb, vb - 16)):
        rc, f, _h = call(kc, vc)
        assert rc == _lib.OKV_E_CAPACITY
        f["key_arena"].untouched("key_arena")
        f["val_arena"].untouched("val_arena")
    rc, f, h = call(kb, vb)
    assert rc == 0, decoder.error()
    assert h["key_arena"].tobytes() == bytes(karena)
    assert h["val_arena"].tobytes() == bytes(varena)
    # a misaligned output arena (base + 8 inside its frame): OKV_E_ARG, nothing written
    f = {name: G.frame(n, dt, **kw) for name, dt in cols}
    f["key_arena"], f["val_arena"] = G.frame(kb + 8, np.uint8, **kw), G.frame(vb, np.uint8, **kw)
    o = _lib.GatherOut(*[f[name].ptr for name, _ in cols], f["key_arena"].ptr + 8,
                       f["val_arena"].ptr, kb, vb, 0, 0)
    assert _lib.lib().okv_gather_rows(decoder._ctx, arr, 2, src.ptr, row.ptr, n, C.byref(o),
                                      DEV) == _lib.OKV_E_ARG
    for name, fr in f.items():
        fr.untouched(name)
    # a misaligned source arena likewise
    bad = _src_array(sources)
    bad[0].key_arena += 8
    o = _lib.GatherOut(*[f[name].ptr for name, _ in cols], f["key_arena"].ptr,
                       f["val_arena"].ptr, kb, vb, 0, 0)
    assert _lib.lib().okv_gather_rows(decoder._ctx, bad, 2, src.ptr, row.ptr, n, C.byref(o),
                                      DEV) == _lib.OKV_E_ARG
    for name, fr in f.items():
        fr.untouched(name)


# ---- okv_merge_rows -------------------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("direction", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("mode", [_lib.MERGE_ALL, _lib.MERGE_GETRANGE], ids=["all", "getrange"])
def test_merge_rows(decoder, mode, direction, poison, base):
    """Three sources with ties (one key in all three): every output array framed
    with row_cap entries -- one short (OKV_E_CAPACITY, n_rows set), then exact."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    shared = b"key-020-in-all"
    # (GETRANGE: all at level 1, so no tombstone rolls the loop into io.EOF)
    srcs = [Source(rs, kw, level=0 if s == 0 and mode == _lib.MERGE_ALL else 1)
            for s, rs in enumerate(_small_streams(7, 3, shared))]
    bound, limit = (b"\xff", 1 << 63) if direction == ASC else (b"", 1 << 63)
    if mode == _lib.MERGE_ALL:
        want, _n, _nu = ref_all(srcs, direction, False)
    else:
        want, _end = SO.merge_lists(
            [(s.rows, s.level, s.lo, s.hi) for s in srcs], bound, limit,
            P.DirectionDescending if direction == DESC else P.DirectionAscending)
        assert want is not None
    n_all = sum(len(s.rows) for s in srcs)
    nu = len({k for s in srcs for k, _ in s.rows})
    assert 3 <= len(want) <= nu < n_all  # ties: fewer owners than rows
    arr = _src_array(srcs)
    bnd = np.frombuffer(bound, np.uint8)
    opts = _lib.MergeOpts(mode, direction, 0, 0, limit, bnd.ctypes.data if bnd.size else None,
                          bnd.size)
    kbase, vbase = min(s.ka for s in srcs), min(s.va for s in srcs)
    cols = (("src", np.uint32), ("row", np.uint64), ("key_off", np.uint64),
            ("key_len", np.uint16), ("val_off", np.uint64), ("val_len", np.uint32))

    def call(cap):
        f = {name: G.frame(cap, dt, **kw) for name, dt in cols}
        mo = _lib.MergeOut(*[f[name].ptr for name, _ in cols], kbase, vbase, cap, 0, 0, 0, 0)
        rc = _lib.lib().okv_merge_rows(decoder._ctx, arr, 3, C.byref(opts), C.byref(mo), DEV)
        for name, fr in f.items():
            fr.check(name)
        for s in srcs:
            s.check()
        return rc, mo, f

    rc, mo, f = call(len(want) - 1)
    assert (rc, mo.n_rows, mo.n_unique) == (_lib.OKV_E_CAPACITY, len(want), nu)
    rc, mo, f = call(len(want))
    assert (rc, mo.status, mo.n_rows, mo.n_unique) == (0, 0, len(want), nu), decoder.error()
    h = {name: fr.host() for name, fr in f.items()}
    assert list(zip(h["src"].tolist(), h["row"].tolist())) == [tuple(p) for p in want]
    for i, (s, q) in enumerate(want):
        st = srcs[s]
        assert int(h["key_off"][i]) == (st.ka - kbase + int(st.ko[q])) & U64, i
        assert int(h["val_off"][i]) == (st.va - vbase + int(st.vo[q])) & U64, i
        assert (int(h["key_len"][i]), int(h["val_len"][i])) == (int(st.kl[q]), int(st.vl[q])), i


# ---- okv_bloom_test_rows, okv_bloom_write_to --------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_bloom_test_rows(decoder, n, poison, base):
    """maybe[n] is one byte per key: an odd n is where a word store overruns."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    ref = B.BloomFilter(4096, 3)
    members = [b"member-%04d" % i for i in range(300)]
    for k in members:
        ref.add(k)
    probes = [members[i * 3] if i % 2 else b"absent-%04d" % i for i in range(n)]
    want = [int(ref.test(k)) for k in probes]
    assert n < 3 or (0 in want and 1 in want)
    f = DeviceBloom.from_bytes(decoder, ref.to_bytes())
    try:
        K = Keys(probes, kw)
        maybe = G.frame(n, np.uint8, **kw)
        rc = _lib.lib().okv_bloom_test_rows(decoder._ctx, f._h, C.byref(K.c), maybe.ptr, DEV)
        maybe.check("maybe")
        K.check()
        assert rc == 0, decoder.error()
        assert maybe.host().tolist() == want
    finally:
        f.close()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("m", [64, 1000, 4099])
def test_bloom_write_to(decoder, m, poison, base):
    """WriteTo into a device buffer of exactly its size; one byte short is
    refused with nothing written."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    ref = B.BloomFilter(m, 3)
    keys = [b"k%05d" % i for i in range(50)]
    for k in keys:
        ref.add(k)
    want = ref.to_bytes()
    f = DeviceBloom(decoder, m, 3).add_rows(keys)
    try:
        assert f.write_to_bytes == len(want)
        dst = G.frame(len(want), np.uint8, **kw)
        rc = _lib.lib().okv_bloom_write_to(decoder._ctx, f._h, dst.ptr, len(want) - 1, DEV)
        assert rc == _lib.OKV_E_CAPACITY
        dst.untouched("dst")
        rc = _lib.lib().okv_bloom_write_to(decoder._ctx, f._h, dst.ptr, len(want), DEV)
        dst.check("dst")
        assert rc == 0, decoder.error()
        assert dst.host().tobytes() == want
    finally:
        f.close()


# ---- okv_hash_blocks --------------------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_hash_blocks(decoder, poison, base):
    """hashes[3] for a three-block writer segment == BlockStat.Hash.  Blocks of
    4 100 bytes: the third ends off a 16-byte boundary at the buffer's last byte,
    so the kernel's 16-byte loads reach past seg_bytes into poison."""
    kw = dict(base_mod=base, poison=poison, device=_dev())
    w = P.SegmentWriter(P.SegmentWriterOptions(3584, 4100))
    for i in range(120):
        w.WriteRow(b"key%05d" % i, b"value-%05d" % i * 6)
    n, meta = w.Close()
    ents = P.bytes_to_metadata(meta).entries
    assert len(ents) == 3
    data = bytes(w.external)[:ents[-1].Offset + ents[-1].BlockSize]
    assert len(data) % 16 != 0 and all(st.Offset % 16 for st in ents[1:])
    seg = G.frame_input(data, **kw)
    descs = G.frame_input(np.array([st.desc() for st in ents], np.uint64), np.uint64, **kw)
    hashes = G.frame(3, np.uint64, **kw)
    rc = _lib.lib().okv_hash_blocks(decoder._ctx, seg.ptr, len(data), descs.ptr, 3, hashes.ptr,
                                    DEV)
    hashes.check("hashes")
    seg.check("seg")
    descs.check("descs")
    assert rc == 0, decoder.error()
    assert hashes.host().tolist() == [st.Hash for st in ents]
