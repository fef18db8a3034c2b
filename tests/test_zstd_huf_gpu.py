"""Huffman-coded literals in the device zstd encoder (OKV_F_ZSTD_HUFFMAN,
okv_zenc_unit_huf_kernel).

Every case runs at T=3584, D=4096 and at T=61440, D=65536, in host mode and in device-pointer
mode, and must give, byte for byte, the frames of the CPU model (tests/zenc_huf_model.py: the
parse of tests/zenc_model.py, the literals decision and the bytes by tests/zenc_huf_main.cpp
from okv_zstd_enc.hpp's statements).  libzstd on each frame, the device decoder and the C
oracle on the file inflate it; oracle/zstd_ref.zstd_segment rebuilds the file around the
frames; the row partition is the uncompressed encode's; no block is larger than without the
flag; two calls give the same bytes.  That each fixture is the shape it claims is asserted
without a GPU in tests/test_zstd_huf_host.py.

Frame census (test_census_is_complete, which runs last): Compressed_Literals_Blocks with one
stream and with four, Size_Formats 00, 10 and 11, a Compressed_Block without sequences, and
raw literals under the flag are all seen; OKV_PATH_ZSTD_HUF is set exactly when the frames of
a call hold a Huffman section."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib
from objectkv_amd import snapshot as SN
from oracle import coracle as CO
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import zenc_cases as ZC
from tests import zenc_huf_cases as HC
from tests import zenc_huf_model as H
from tests import zenc_model as M
from tests.test_get_zstd_gpu import Seg
from tests.test_snap_get_gpu import _seg
from tests.test_snap_get_zstd_gpu import ZEnv
from tests.test_snap_get_zstd_gpu import _check as snap_check

pytestmark = pytest.mark.gpu

UNIT = _lib.ZSTD_ENC_UNIT
CONFIGS = ZC.CONFIGS
ZSTD = okv.sst.COMP_ZSTD
CENSUS = set()
_raw, _closes = ZC.raw_of, ZC.closes


@pytest.fixture(scope="module")
def enc():
    e = okv.Encoder(0)
    yield e
    e.close()


def _tensors(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16,
              np.dtype(np.uint32): np.int32}
    return {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
            for k, v in r.items()}


def _encode_device(enc, rows, T, D, strict_go=True, **flags):
    """Size query, the bound, then the encode: (Encoded, bound file bytes, last_path)."""
    r = okv.pack_rows(rows)
    t = _tensors(r)
    kw = dict(key_arena_bytes=r["key_arena"].size, val_arena_bytes=r["val_arena"].size, **flags)
    with pytest.raises(okv.OkvError) as e:
        enc.encode_device(t, len(rows), {}, T, D, ZSTD, strict_go, **kw)
    assert e.value.code == _lib.OKV_E_CAPACITY
    need = e.value.out
    nb, bound = int(need.n_blocks), int(need.file_bytes)
    out = {"seg": torch.zeros(bound, dtype=torch.uint8, device="cuda"),
           "first_row": torch.zeros(nb + 1, dtype=torch.int64, device="cuda"),
           "desc": torch.zeros((nb, 4), dtype=torch.int64, device="cuda"),
           "hash": torch.zeros(nb, dtype=torch.int64, device="cuda")}
    eo = enc.encode_device(t, len(rows), out, T, D, ZSTD, strict_go, **kw)
    path = enc.last_path()
    assert eo.n_blocks == nb and eo.file_bytes <= bound
    return okv.sst.Encoded(out["seg"][:eo.file_bytes].cpu().numpy(), int(eo.file_bytes),
                           int(eo.data_bytes), int(eo.meta_bytes), int(eo.meta_hash),
                           out["first_row"].cpu().numpy().view(np.uint64),
                           out["desc"].cpu().numpy().view(np.uint64),
                           out["hash"].cpu().numpy().view(np.uint64)), bound, path


def parse_frame(frame, orig):
    """The literals sections of a frame's blocks: [(block type, literals type, streams,
    Size_Format, number of sequences is 0)], read from the bytes alone."""
    pos, out = M.frame_header_size(orig), []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        assert typ in (0, 2)
        c = frame[pos:pos + size]
        if typ == 0:
            assert 0 < size <= UNIT
            out.append((0, None, 0, 0, None))
        else:
            assert size < UNIT
            lt, sf = c[0] & 3, (c[0] >> 2) & 3
            assert lt in (0, 2)
            if lt == 0:
                hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                nlit = int.from_bytes(c[:hb], "little") >> (3 if hb == 1 else 4)
                at, streams = hb + nlit, 0
                sf = 0
            else:
                assert sf != 1, "Size_Format 01 is never written"
                hb, bits = (3, 10) if sf == 0 else (4, 14) if sf == 2 else (5, 18)
                v = int.from_bytes(c[:hb], "little")
                regen, comp = (v >> 4) & ((1 << bits) - 1), v >> (4 + bits)
                assert (regen <= 1023) == (sf == 0) and (regen <= 16383) == (sf != 3)
                assert c[hb] >= 128, "direct weights"
                assert comp < regen
                at, streams = hb + comp, 1 if sf == 0 else 4
            nseq0 = c[at] == 0
            if nseq0:
                assert at + 1 == size and lt == 2
            out.append((2, lt, streams, sf, nseq0))
        pos += size
        if last:
            break
    assert pos + 4 == len(frame)
    return out


def check(enc, decoder, rows, T, D, strict_go=True):
    """The whole contract for one row set; returns (host-mode Encoded, units of every block
    from the model, what parse_frame saw)."""
    flags = dict(zstd_native=True, zstd_huffman=True)
    got = enc.encode(rows, T, D, ZSTD, strict_go, **flags)
    path = enc.last_path()
    assert path & _lib.PATH_ZSTD_ENC
    dev, bound, dev_path = _encode_device(enc, rows, T, D, strict_go, **flags)
    again = enc.encode(rows, T, D, ZSTD, strict_go, **flags)
    seg = got.seg.tobytes()
    assert again.seg.tobytes() == seg and dev.seg.tobytes() == seg and dev_path == path
    for a in (dev, again):
        assert np.array_equal(a.first_row, got.first_row) and np.array_equal(a.descs, got.descs)
        assert np.array_equal(a.hashes, got.hashes) and a.meta_hash == got.meta_hash
    assert got.file_bytes == len(seg) <= bound
    nb = got.n_blocks
    plain = enc.encode(rows, T, D, strict_go=strict_go)
    assert np.array_equal(plain.first_row, got.first_row) and int(got.first_row[nb]) == len(rows)
    off = enc.encode(rows, T, D, ZSTD, strict_go, zstd_native=True)
    assert not enc.last_path() & _lib.PATH_ZSTD_HUF
    assert np.array_equal(off.first_row, got.first_row)
    frames, raws, seen = [], [], []
    for b in range(nb):
        o, bs, orig, cs = (int(x) for x in got.descs[b])
        raw = _raw(rows[int(got.first_row[b]):int(got.first_row[b + 1])])
        assert orig == len(raw) and bs == cs + (D - cs % D) and o % D == 0
        frame = seg[o:o + cs]
        assert Z.decompress(frame, orig) == raw, b
        assert seg[o + cs:o + bs] == bytes(bs - cs)
        assert cs <= int(off.descs[b, 3]) <= orig + 3 * -(-orig // UNIT) + 18
        seen += parse_frame(frame, orig)
        frames.append(frame)
        raws.append(raw)
    units = []
    for b, (want, us) in enumerate(H.model_frames(raws, True)):
        assert frames[b] == want, (b, len(raws[b]))
        units += us
    # the census of the bytes is the model's, and the path bit says what the bytes hold
    assert [(s[0], s[1] or 0, s[2], s[3]) for s in seen] == \
        [(u.census["block"], u.census["lit"], u.census["streams"], u.census["sf"]) for u in units]
    assert bool(path & _lib.PATH_ZSTD_HUF) == any(s[1] == 2 for s in seen)
    CENSUS.update(seen)
    want, want_len, want_meta = Z.zstd_segment(rows, T, D, frame_fn=lambda raw, i: frames[i])
    assert seg == want and got.file_bytes == want_len and got.meta() == want_meta
    dec = decoder.decode(got.seg, got.descs, ZSTD)
    assert int(dec.status.max()) == 0
    assert [kv for b in range(nb) for kv in dec.block_rows(b)] == \
        [(k, v or None) for k, v in rows]
    ref = CO.decode_soa(seg, CO.descs_array([tuple(int(x) for x in d) for d in got.descs]), 1)
    for k in ("status", "row_start", "key_off", "key_len", "val_off", "val_len"):
        assert np.array_equal(getattr(dec, k), ref[k]), k
    assert dec.key_arena.tobytes() == ref["key_arena"].tobytes()
    assert dec.val_arena.tobytes() == ref["val_arena"].tobytes()
    return got, units, seen


FIXTURES = {name: rows for name, rows, _ in HC.fixtures()}
EXTRA = dict(HC.extra())


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures(enc, decoder, T, D, name):
    rows = FIXTURES[name]
    _, units, seen = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if name == "nlit_1023":
        assert seen == [(2, 2, 1, 0, True)]
    if name == "largest_129":
        assert seen == [(0, None, 0, 0, None)]


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", [n for n in EXTRA if n != "text_46"])
def test_extra_rows(enc, decoder, T, D, name):
    rows = EXTRA[name]
    got, units, seen = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if name == "three_units_short_last":
        assert [u.n for u in units] == [UNIT, UNIT, 5]
    if name == "seven_bytes":
        assert [int(x) for x in got.descs[0]] == [0, D, 7, 6 + 3 + 7 + 4]
    if name == "random_bytes":
        assert all(s[1] != 2 for s in seen)


@pytest.mark.parametrize("T,D", CONFIGS)
def test_text_rows_are_smaller_with_the_flag(enc, decoder, T, D):
    rows = ZC.text_rows(46)
    raw = _raw(rows)
    assert len(raw) == 3542
    got, units, seen = check(enc, decoder, rows, T, D)
    want = len(H.model(raw, True)[0])
    cs = int(got.descs[0, 3])
    print(f"46 text rows: CompressedSize {cs} with the flag (model {want}), 897 without; "
          f"libzstd-1 {len(Z.compress(raw, 1))}")
    assert got.n_blocks == 1 and cs == want < 897
    assert seen[0][:2] == (2, 2)


def test_contract(enc):
    """The flag needs OKV_F_ZSTD_NATIVE; a flag-off call after flagged calls gives the bytes
    of a flag-off call made before any; the capacity contract of the encoder holds."""
    rows = ZC.text_rows(500)
    T, D = CONFIGS[0]
    fresh = okv.Encoder(0)
    try:
        before = fresh.encode(rows, T, D, ZSTD, False, zstd_native=True)
        assert not fresh.last_path() & _lib.PATH_ZSTD_HUF
        flagged = fresh.encode(rows, T, D, ZSTD, False, zstd_native=True, zstd_huffman=True)
        assert fresh.last_path() & _lib.PATH_ZSTD_HUF
        assert int(flagged.descs[:, 3].sum()) < int(before.descs[:, 3].sum())
        big = [HC.lit_row(HC.plain(UNIT))]  # (the Huffman phases write all over the scratch LDS)
        fresh.encode(big, T, D, ZSTD, False, zstd_native=True, zstd_huffman=True)
        after = fresh.encode(rows, T, D, ZSTD, False, zstd_native=True)
        assert after.seg.tobytes() == before.seg.tobytes()
        assert not fresh.last_path() & _lib.PATH_ZSTD_HUF
    finally:
        fresh.close()
    r = okv.pack_rows(rows)
    t = _tensors(r)
    for comp, native in ((ZSTD, False), (okv.sst.COMP_NONE, False), (okv.sst.COMP_LZ4, False)):
        for call in (lambda: enc.encode(rows, T, D, comp, False, zstd_native=native,
                                        zstd_huffman=True),
                     lambda: enc.encode_device(t, len(rows), {}, T, D, comp, False,
                                               zstd_native=native, zstd_huffman=True)):
            with pytest.raises(okv.OkvError) as e:
                call()
            assert e.value.code == _lib.OKV_E_ARG
    w = okv.GpuSegmentWriter(enc, zstd_level=1, zstd_huffman=True)
    w.WriteRow(b"a", b"b")
    with pytest.raises(okv.OkvError) as e:
        w.Close()
    assert e.value.code == _lib.OKV_E_ARG
    # capacity: the bound comes from the raw sizes alone, with the flag as without
    kw = dict(key_arena_bytes=r["key_arena"].size, val_arena_bytes=r["val_arena"].size,
              zstd_native=True, zstd_huffman=True)
    plain = enc.encode(rows, T, D, strict_go=False)
    with pytest.raises(okv.OkvError) as e:
        enc.encode_device(t, len(rows), {}, T, D, ZSTD, False, **kw)
    q = e.value.out
    assert e.value.code == _lib.OKV_E_CAPACITY and q.n_blocks == plain.n_blocks
    bound = 0
    for orig in (int(x) for x in plain.descs[:, 2]):
        fb = orig + 3 * -(-orig // UNIT) + 18
        bound += fb + (D - fb % D)
    assert q.data_bytes == bound and q.file_bytes == bound + q.meta_bytes + 25
    seg = torch.full((int(q.file_bytes),), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(okv.OkvError) as e:
        enc.encode_device(t, len(rows), {"seg": seg[:-1]}, T, D, ZSTD, False, **kw)
    assert e.value.code == _lib.OKV_E_CAPACITY and e.value.out.file_bytes == q.file_bytes
    assert int(seg.min()) == 0xAB
    eo = enc.encode_device(t, len(rows), {"seg": seg}, T, D, ZSTD, False, **kw)
    assert eo.file_bytes <= q.file_bytes and eo.data_bytes <= q.data_bytes
    assert seg[:eo.file_bytes].cpu().numpy().tobytes() == flagged.seg.tobytes()


def test_gpu_segment_writer(enc, decoder):
    rows = ZC.text_rows(200)
    w = okv.GpuSegmentWriter(enc, zstd_level=1, zstd_native=True, zstd_huffman=True)
    for k, v in rows:
        w.WriteRow(k, v)
    flen, _meta = w.Close()
    assert enc.last_path() & _lib.PATH_ZSTD_HUF
    md = okv.fetch_metadata(w.data(), flen)
    assert md.compression == ZSTD and flen == w.data().size
    dec = decoder.decode(w.data(), md.descs, ZSTD)
    assert [kv for b in range(md.descs.shape[0]) for kv in dec.block_rows(b)] == rows


def _meta_of(seg, flen):
    meta_off = int.from_bytes(seg[flen - 25:flen - 17], "little")
    return seg[meta_off:flen - 25]


def test_get_rows_on_a_compacted_huffman_segment(enc, decoder):
    """compact(..., zstd=True, zstd_huffman=True) writes Huffman literals; get_rows(...,
    zstd=True) and snapshot.Reader.GetRows read every key of it as the oracle does."""
    def val(s, i):
        return b'{"seg":%d,"id":%d,"name":"user%d","note":"%s"}' % (s, i, i * 7, b"lorem ipsum " *
                                                                     (1 + i % 5))
    a = [(b"key%06d" % i, val(1, i)) for i in range(0, 900, 2)]
    b = [(b"key%06d" % i, val(2, i)) for i in range(300, 1200, 3)]
    for rows in (a, b):  # (the Go writer panics in Close when the last row closed a block)
        while _closes(rows, 3584):
            rows.append((rows[-1][0] + b"+", b"tail"))
    segs = [_seg("2", 0, b), _seg("1", 1, a)]
    dsegs = [(SN.DeviceSegment(enc, d, n), lvl) for _sid, lvl, d, n, _m in segs]
    plain = SN.compact(dsegs, enc)
    got = SN.compact(dsegs, enc, zstd=True, zstd_huffman=True)
    assert enc.last_path() & _lib.PATH_ZSTD_HUF
    flat = SN.compact(dsegs, enc, zstd=True)
    assert got.n_rows == plain.n_rows and got.n_blocks == flat.n_blocks
    seg = got.seg.tobytes()[:got.file_bytes]
    meta = _meta_of(seg, got.file_bytes)
    md = P.bytes_to_metadata(meta)
    flat_md = P.bytes_to_metadata(_meta_of(flat.seg.tobytes(), flat.file_bytes))
    assert sum(st.CompressedSize for st in md.entries) < \
        sum(st.CompressedSize for st in flat_md.entries)
    kinds = [s for st in md.entries for s in
             parse_frame(seg[st.Offset:st.Offset + st.CompressedSize], st.OriginalSize)]
    assert any(s[1] == 2 for s in kinds)
    merged = dict(a)
    merged.update(dict(b))
    keys = sorted(merged) + [b"key000001", b"", b"zzz"]
    s = Seg(decoder, seg, meta)
    res = s.check(keys)
    assert res.n_found == len(merged) and res.n_fallback == 0
    assert all(res.value(i) == merged[k] for i, k in enumerate(keys[:len(merged)]))
    s.close()
    env = ZEnv(decoder, [("9", 1, seg, got.file_bytes, meta)])
    res = snap_check(env, keys)
    assert res.n_found == len(merged) and res.n_fallback == 0
    env.close()


def test_census_is_complete(enc, decoder):
    """Runs last: over the file every form was seen (the fixtures here alone show them all,
    so the test also stands when it is run alone)."""
    T, D = CONFIGS[1]
    for name in ("nlit_1023", "nlit_1024", "nlit_32768", "largest_129", "with_sequences",
                 "edge_-1", "edge_+1", "many_sequences_not_smaller"):
        rows = FIXTURES[name]
        check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    rows = EXTRA["text_1500"]
    check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    forms = {(s[1], s[2], s[3]) for s in CENSUS if s[0] == 2}
    assert {(2, 1, 0), (2, 4, 2), (2, 4, 3), (0, 0, 0)} <= forms, forms
    assert any(s[1] == 2 and s[4] for s in CENSUS), "a Compressed_Block without sequences"
    assert any(s[1] == 2 and s[4] is False for s in CENSUS), "Huffman literals and sequences"
    assert any(s[0] == 0 for s in CENSUS), "a Raw_Block"
