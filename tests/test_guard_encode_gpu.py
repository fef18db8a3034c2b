"""Caller buffers of the device encode (okv_encode_rows / okv_encode_close /
okv_encode_split with OKV_F_DEVICE_PTRS): the rows come from tests/guarded.py
frames of exactly their extents (no padding behind the arenas: poison), every
output is a frame of exactly the size the size query reports, at base 0 and
base 16 of a 128-byte line, under two poisons.

  G  guards of every frame intact after every call, capacity errors included;
  X  the file and the block index equal the oracle writer's, bit for bit (the
     zstd encoder's frames: the CPU model's, tests/zenc_*model.py);
  N  OKV_E_CAPACITY and the size query write nothing (okv_sst.h: "sizes in out
     set, nothing written");
  D  the bytes behind the row arenas do not matter."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import objectkv_amd as okv
from objectkv_amd import _lib
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import guarded as G
from tests.test_encode_gpu import _pack_edge_rows, oracle_segment

pytestmark = pytest.mark.gpu

POISONS = [0xA5, 0x5A]
BASES = [0, 16]
DEV = _lib.F_DEVICE_PTRS
ZSTD = _lib.COMP_ZSTD


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def enc():
    e = okv.Encoder(0)
    yield e
    e.close()


# ---- rows and their oracle files (built once) -----------------------------------


def _general_rows():
    """test_general_pack_path_vs_oracle's big rows: 150 000-byte values between
    40-byte ones (blocks over 64 KiB: the per-block pack kernel)."""
    rng = random.Random(11)
    return [(b"b%06d" % i, rng.randbytes(150_000 if i % 5 == 2 else 40)) for i in range(12)]


def _c2_rows():
    return [(i.to_bytes(16, "big"), bytes((i * 7 + j) & 255 for j in range(64)))
            for i in range(120)]


# name -> (rows, threshold, block size)
SHAPES = {
    "c2_three_blocks": lambda: (_c2_rows(), 3584, 4096),
    "fk_d48": lambda: _pack_edge_rows("fk_d48")[:3],
    "fk_d64": lambda: _pack_edge_rows("fk_d64")[:3],
    "many_blocks": lambda: _pack_edge_rows("many_blocks")[:3],
    "general": lambda: (_general_rows(), 3584, 4096),
    "general_d4100": lambda: (_general_rows(), 3584, 4100),  # block_size % 16 != 0
    "c2_d4100": lambda: (_c2_rows(), 3584, 4100),  # small records, block_size % 16 != 0
}
_CASES = {}


def _case(name):
    """(rows, T, D, oracle file, oracle meta, BlockStat entries, first rows)."""
    if name not in _CASES:
        rows, T, D = SHAPES[name]()
        rc, want, meta = oracle_segment(rows, T, D)
        assert rc == 0
        ents = P.bytes_to_metadata(meta).entries
        first, r = [], 0
        for st in ents:  # the cut, from each block's OriginalSize
            first.append(r)
            left = st.OriginalSize
            while left > 0:
                left -= 6 + len(rows[r][0]) + len(rows[r][1])
                r += 1
            assert left == 0 and rows[first[-1]][0] == st.FirstKey
        assert r == len(rows)
        _CASES[name] = (rows, T, D, want, meta, ents, first + [r])
    return _CASES[name]


class Rows:
    """okv_rows over framed device arrays of exactly their extents."""

    def __init__(self, rows, poison, base):
        r = okv.pack_rows(rows)
        kb, vb = int(r["key_len"].sum()), int(r["val_len"].sum())
        kw = dict(base_mod=base, poison=poison, device=_dev())
        self.f = {"key_arena": G.frame_input(r["key_arena"][:kb], **kw),
                  "val_arena": G.frame_input(r["val_arena"][:vb], **kw),
                  "key_off": G.frame_input(r["key_off"], np.uint64, **kw),
                  "val_off": G.frame_input(r["val_off"], np.uint64, **kw),
                  "key_len": G.frame_input(r["key_len"], np.uint16, **kw),
                  "val_len": G.frame_input(r["val_len"], np.uint32, **kw)}
        f = self.f
        self.c = _lib.Rows(f["key_arena"].ptr, f["key_off"].ptr, f["key_len"].ptr,
                           f["val_arena"].ptr, f["val_off"].ptr, f["val_len"].ptr, len(rows),
                           kb, vb)

    def check(self):
        for name, f in self.f.items():
            f.check("rows." + name)


class Out:
    """okv_encode_out over frames of exactly seg_cap / blk_cap (+ 1) entries."""

    def __init__(self, seg_cap, blk_cap, poison, base):
        kw = dict(base_mod=base, poison=poison, device=_dev())
        self.f = {"seg": G.frame(seg_cap, np.uint8, **kw),
                  "first_row": G.frame(blk_cap + 1, np.uint64, **kw),
                  "desc": G.frame(blk_cap * 4, np.uint64, **kw),
                  "hash": G.frame(blk_cap, np.uint64, **kw)}

    def c(self, seg_cap, blk_cap):
        f = self.f
        return _lib.EncodeOut(f["seg"].ptr, seg_cap, f["first_row"].ptr, f["desc"].ptr,
                              f["hash"].ptr, blk_cap)

    def check(self):
        for name, f in self.f.items():
            f.check("out." + name)

    def untouched(self):
        for name, f in self.f.items():
            f.untouched("out." + name)


def _encode(enc, R, opts, eo, flags):
    return _lib.lib().okv_encode_rows(enc._ctx, C.byref(R.c), C.byref(opts), C.byref(eo), flags)


def _size_query(enc, R, opts, flags):
    q = _lib.EncodeOut()
    assert _encode(enc, R, opts, q, flags) == _lib.OKV_E_CAPACITY, enc.error()
    return q


def _assert_index(out: Out, nb, ents, first):
    assert out.f["first_row"].host().tolist() == first
    assert out.f["desc"].host().reshape(nb, 4).tolist() == [list(st.desc()) for st in ents]
    assert out.f["hash"].host().tolist() == [st.Hash for st in ents]


# ---- uncompressed: X, G, N ---------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_encode_exact_capacities(enc, name, poison, base):
    """seg_cap == file_bytes and blk_cap == n_blocks exactly (blk_first_row of
    blk_cap + 1).  First the three refused calls -- the size query (zero
    capacities), seg_cap one short, blk_cap one short: sizes set, nothing
    written -- then the encode."""
    rows, T, D, want, meta, ents, first = _case(name)
    nb = len(ents)
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, 0, 1, None, 0)
    out = Out(len(want), nb, poison, base)
    for seg_cap, blk_cap in ((0, 0), (len(want) - 1, nb), (len(want), nb - 1)):
        eo = out.c(seg_cap, blk_cap)
        rc = _encode(enc, R, opts, eo, DEV)
        assert rc == _lib.OKV_E_CAPACITY, (seg_cap, blk_cap, rc, enc.error())
        assert (eo.n_blocks, eo.file_bytes, eo.meta_bytes) == (nb, len(want), len(meta))
        out.untouched()  # N (and the guards)
        R.check()
    eo = out.c(len(want), nb)
    rc = _encode(enc, R, opts, eo, DEV)
    out.check()
    R.check()
    assert rc == 0, enc.error()
    assert (eo.n_blocks, eo.file_bytes, eo.meta_bytes, eo.data_bytes) == \
        (nb, len(want), len(meta), len(want) - len(meta) - 25)
    got = out.f["seg"].host().tobytes()
    if got != want:
        bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))
        raise AssertionError(f"{bad.size} bytes differ, first at {int(bad[0])} of {len(want)}")
    _assert_index(out, nb, ents, first)
    assert eo.meta_hash == P.xxh64(meta)


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_no_close_then_close(enc, poison, base):
    """OKV_F_NO_CLOSE writes blocks and meta block; okv_encode_close then puts
    the 25 trailer bytes at data_bytes + meta_bytes, which end exactly at
    seg_cap."""
    rows, T, D, want, meta, ents, first = _case("c2_three_blocks")
    nb = len(ents)
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, 0, 1, None, 0)
    out = Out(len(want), nb, poison, base)
    eo = out.c(len(want), nb)
    rc = _encode(enc, R, opts, eo, DEV | _lib.F_NO_CLOSE)
    out.check()
    R.check()
    assert rc == 0, enc.error()
    body = len(want) - 25
    assert eo.data_bytes + eo.meta_bytes == body and eo.meta_hash == 0
    assert out.f["seg"].host().tobytes()[:body] == want[:body]
    _assert_index(out, nb, ents, first)
    assert _lib.lib().okv_encode_close(enc._ctx, C.byref(eo), DEV) == 0, enc.error()
    out.check()
    assert out.f["seg"].host().tobytes() == want
    assert eo.meta_hash == P.xxh64(meta) and eo.file_bytes == len(want)


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_bloom_bytes_from_a_framed_device_buffer(enc, poison, base):
    """OKV_F_BLOOM_DEVICE: opts->bloom points into a framed device buffer; the
    meta block carries the bytes as the oracle writer writes them."""
    from oracle import coracle as CO
    from oracle.bloom_ref import default_filter
    rows, T, D = _c2_rows(), 3584, 4096
    f = default_filter()
    for k, _v in rows:
        f.add(k)
    bb = f.to_bytes()
    w = CO.Writer(T, D)
    for k, v in rows:
        assert w.write_row(k, v) == 0
    w.set_bloom(bb)
    rc, want, meta = w.close()
    assert rc == 0
    bloom = G.frame_input(bb, base_mod=base, poison=poison, device=_dev())
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, 0, 1, bloom.ptr, len(bb))
    flags = DEV | _lib.F_BLOOM_DEVICE
    q = _size_query(enc, R, opts, flags)
    assert (q.file_bytes, q.n_blocks) == (len(want), 3)
    out = Out(len(want), 3, poison, base)
    eo = out.c(len(want), 3)
    rc = _encode(enc, R, opts, eo, flags)
    out.check()
    R.check()
    bloom.check("bloom")
    assert rc == 0, enc.error()
    assert out.f["seg"].host().tobytes() == want
    assert bloom.host().tobytes() == bb


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_row_arena_at_base_plus_8(enc, poison, base):
    """The row arenas carry no alignment contract (a decode's arenas are
    16-byte aligned, a caller's need not be): key_arena at base + 8 inside its
    frame encodes the same file, and the reads around it stay harmless."""
    rows, T, D, want, meta, ents, first = _case("c2_three_blocks")
    nb = len(ents)
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, 0, 1, None, 0)
    r = okv.pack_rows(rows)
    kb = int(r["key_len"].sum())
    ka = G.frame_input(bytes(8) + r["key_arena"][:kb].tobytes(), base_mod=base, poison=poison,
                       device=_dev())
    R.c.key_arena = ka.ptr + 8
    out = Out(len(want), nb, poison, base)
    eo = out.c(len(want), nb)
    rc = _encode(enc, R, opts, eo, DEV)
    out.check()
    ka.check("key_arena")
    assert rc == 0, enc.error()
    assert out.f["seg"].host().tobytes() == want


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", ["c2_three_blocks", "many_blocks", "general"])
def test_seg_at_base_plus_8(enc, name, poison, base):
    """okv_encode_rows accepts a device seg that is not 16-byte aligned (okv_sst.h:
    it takes the byte-store pack kernels): seg at base + 8 inside its frame, of
    exactly file_bytes, holds the oracle writer's file and the 8 bytes before it
    and everything behind it stay poison."""
    rows, T, D, want, meta, ents, first = _case(name)
    nb = len(ents)
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, 0, 1, None, 0)
    out = Out(len(want) + 8, nb, poison, base)
    eo = out.c(len(want), nb)
    eo.seg = out.f["seg"].ptr + 8
    rc = _encode(enc, R, opts, eo, DEV)
    out.check()
    R.check()
    assert rc == 0, enc.error()
    got = out.f["seg"].host().tobytes()
    assert got[:8] == bytes([poison]) * 8 and got[8:] == want
    _assert_index(out, nb, ents, first)


# ---- the zstd encoder ----------------------------------------------------------------

ZFLAGS = {"native": _lib.F_ZSTD_NATIVE,
          "huffman": _lib.F_ZSTD_NATIVE | _lib.F_ZSTD_HUFFMAN,
          "huf_fse": _lib.F_ZSTD_NATIVE | _lib.F_ZSTD_HUFFMAN | _lib.F_ZSTD_HUF_FSE}
_ZCASES = {}


def _zrows(name):
    from tests import zenc_cases as ZC
    from tests import zenc_fse_cases as FC
    if name == "text46":
        return ZC.text_rows(46)
    rows = dict(FC.extra())["utf8_rows"]  # byte values above 128 in every block
    assert any(b > 128 for _k, v in rows for b in v)
    return rows


def _zcase(name, mode, T, D):
    """(rows, the file around the CPU model's frames, number of blocks, whether the
    model writes a unit with Huffman literals, and one with FSE-compressed weights)."""
    key = (name, mode)
    if key not in _ZCASES:
        from tests import zenc_cases as ZC
        from tests import zenc_fse_model as F
        from tests import zenc_huf_model as H
        from tests import zenc_model as M
        from tests import split_model as SM
        rows = _zrows(name)
        _sizes, first = SM.blocks_of_rows(rows, T, D)  # the cut is on raw lengths
        raws = [ZC.raw_of(rows[first[b]:first[b + 1]]) for b in range(len(first) - 1)]
        if mode == "native":
            got = M.model_frames(raws)
        elif mode == "huffman":
            got = H.model_frames(raws, True)
        else:
            got = F.model_frames(raws)
        frames = [f for f, _u in got]
        cens = [u.census for _f, us in got for u in us] if mode != "native" else []
        huf = [c for c in cens if c.get("block") == 2 and c.get("lit") == 2]
        want_huf = bool(huf)
        want_fse = mode == "huf_fse" and any(c.get("desc") == 1 for c in huf)
        want, want_len, _meta = Z.zstd_segment(rows, T, D, frame_fn=lambda raw, i: frames[i])
        assert want_len == len(want)
        _ZCASES[key] = (rows, want, len(frames), want_huf, want_fse)
    return _ZCASES[key]


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("mode", list(ZFLAGS))
@pytest.mark.parametrize("name", ["text46", "utf8_rows"])
def test_zstd_encoder(enc, name, mode, poison, base):
    """OKV_F_ZSTD_NATIVE, | OKV_F_ZSTD_HUFFMAN, | OKV_F_ZSTD_HUF_FSE: seg_cap is
    the bound the size query reports; [0, file_bytes) equals the file around
    the CPU model's frames, and nothing is written past the bound."""
    from tests import zenc_cases as ZC
    T, D = 3584, 4096
    rows, want, nb, want_huf, want_fse = _zcase(name, mode, T, D)
    if name == "text46" and mode != "native":
        assert want_huf  # the text rows reach the Huffman writer
    if name == "utf8_rows":  # bytes above 128: Huffman literals only with FSE-compressed weights
        assert (want_huf, want_fse) == (mode == "huf_fse", mode == "huf_fse")
    strict = 0 if ZC.closes(rows, T) else 1
    flags = DEV | ZFLAGS[mode]
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(T, D, ZSTD, strict, None, 0)
    q = _size_query(enc, R, opts, flags)
    bound = int(q.file_bytes)
    assert q.n_blocks == nb and bound >= len(want)
    out = Out(bound, nb, poison, base)
    eo = out.c(bound - 1, nb)
    assert _encode(enc, R, opts, eo, flags) == _lib.OKV_E_CAPACITY
    out.untouched()
    eo = out.c(bound, nb)
    rc = _encode(enc, R, opts, eo, flags)
    out.check()
    R.check()
    assert rc == 0, enc.error()
    lp = enc.last_path()  # the route: what the frames hold, as the model says
    assert lp & _lib.PATH_ZSTD_ENC
    assert bool(lp & _lib.PATH_ZSTD_HUF) == want_huf, (lp, want_huf)
    assert bool(lp & _lib.PATH_ZSTD_HUF_FSE) == want_fse, (lp, want_fse)
    assert eo.file_bytes == len(want) and eo.n_blocks == nb
    assert out.f["seg"].host().tobytes()[:len(want)] == want
    assert out.f["first_row"].host()[-1] == len(rows)


# ---- okv_encode_split ------------------------------------------------------------------


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("poison", POISONS)
def test_split_three_segments(enc, poison, base):
    """test_split_gpu.SHAPES["short_last"] (segments of 3, 3 and 2 blocks): data,
    meta, the segment table and the block index in frames of exactly the sizes
    the size query reports.  okv_sst.h: OKV_E_CAPACITY -- "the sizes in out set,
    nothing written" -- for the size query and for each capacity one short."""
    from tests.test_split_gpu import SEG_WORDS, SHAPES as SPLIT_SHAPES, _oracle_file
    make, th, bs, sb, sr, comp, _also = SPLIT_SHAPES["short_last"]
    rows = make()
    R = Rows(rows, poison, base)
    opts = _lib.EncodeOpts(th, bs, comp, 0, None, 0)
    so = _lib.SplitOpts(sb, sr, 0, 0)
    lib = _lib.lib()
    q = _lib.SplitOut()
    assert lib.okv_encode_split(enc._ctx, C.byref(R.c), C.byref(opts), C.byref(so), C.byref(q),
                                DEV) == _lib.OKV_E_CAPACITY
    ns, nb, db, mb = int(q.n_segments), int(q.n_blocks), int(q.data_bytes), \
        int(q.meta_arena_bytes)
    assert (ns, nb) == (3, 8)
    kw = dict(base_mod=base, poison=poison, device=_dev())
    f = {"data": G.frame(db, np.uint8, **kw), "meta": G.frame(mb, np.uint8, **kw),
         "segs": G.frame(ns * SEG_WORDS, np.uint64, **kw),
         "first_row": G.frame(nb + 1, np.uint64, **kw), "desc": G.frame(nb * 4, np.uint64, **kw),
         "hash": G.frame(nb, np.uint64, **kw)}

    def call(data_cap, meta_cap, seg_cap, blk_cap):
        o = _lib.SplitOut(f["data"].ptr, data_cap, f["meta"].ptr, meta_cap, f["segs"].ptr,
                          seg_cap, f["first_row"].ptr, f["desc"].ptr, f["hash"].ptr, blk_cap)
        return lib.okv_encode_split(enc._ctx, C.byref(R.c), C.byref(opts), C.byref(so),
                                    C.byref(o), DEV), o

    for caps in ((0, 0, 0, 0), (db - 1, mb, ns, nb), (db, mb - 1, ns, nb), (db, mb, ns - 1, nb),
                 (db, mb, ns, nb - 1)):
        rc, o = call(*caps)
        assert rc == _lib.OKV_E_CAPACITY, (caps, rc, enc.error())
        assert (o.n_segments, o.n_blocks, o.data_bytes, o.meta_arena_bytes) == (ns, nb, db, mb)
        for name, fr in f.items():
            fr.untouched(name)
        R.check()
    # a device meta must be 16-byte aligned: base + 8 is OKV_E_ARG, nothing written
    o = _lib.SplitOut(f["data"].ptr, db, f["meta"].ptr + 8, mb - 8, f["segs"].ptr, ns,
                      f["first_row"].ptr, f["desc"].ptr, f["hash"].ptr, nb)
    assert lib.okv_encode_split(enc._ctx, C.byref(R.c), C.byref(opts), C.byref(so), C.byref(o),
                                DEV) == _lib.OKV_E_ARG
    for name, fr in f.items():
        fr.untouched(name)
    rc, o = call(db, mb, ns, nb)
    for name, fr in f.items():
        fr.check(name)
    R.check()
    assert rc == 0, enc.error()
    segs = f["segs"].host().reshape(ns, SEG_WORDS)
    names = [x[0] for x in _lib.SplitSeg._fields_]
    data, meta = f["data"].host(), f["meta"].host()
    row = 0
    for s in range(ns):
        g = dict(zip(names, (int(v) for v in segs[s])))
        assert g["first_row"] == row
        part = rows[row:row + g["n_rows"]]
        row += g["n_rows"]
        got = data[g["data_off"]:g["data_off"] + g["data_bytes"]].tobytes() + \
            meta[g["meta_off"]:g["meta_off"] + g["meta_bytes"] + 25].tobytes()
        assert got == _oracle_file(part, th, bs), s
        # the meta arena's padding to the next 16-byte meta_off is part of
        # meta_arena_bytes; the header does not define its bytes
    assert row == len(rows)
    assert [int(segs[s][names.index("n_blocks")]) for s in range(ns)] == [3, 3, 2]
    assert f["first_row"].host()[-1] == len(rows)
    # data at base + 8 is accepted (okv_sst.h): the same bytes, 8 further on
    d8 = G.frame(db + 8, np.uint8, **kw)
    o = _lib.SplitOut(d8.ptr + 8, db, f["meta"].ptr, mb, f["segs"].ptr, ns, f["first_row"].ptr,
                      f["desc"].ptr, f["hash"].ptr, nb)
    rc = lib.okv_encode_split(enc._ctx, C.byref(R.c), C.byref(opts), C.byref(so), C.byref(o), DEV)
    d8.check("data + 8")
    for name, fr in f.items():
        fr.check(name)
    assert rc == 0, enc.error()
    assert d8.host().tobytes() == bytes([poison]) * 8 + data.tobytes()
    assert f["meta"].host().tobytes() == meta.tobytes()
