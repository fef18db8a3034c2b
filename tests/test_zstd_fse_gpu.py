"""FSE-compressed Huffman weights in the device zstd encoder (OKV_F_ZSTD_HUF_FSE,
okv_zenc_unit_fse_kernel).

Every case runs at T=3584, D=4096 and at T=61440, D=65536, in host mode and in device-pointer
mode, and must give, byte for byte, the frames of the CPU model (tests/zenc_fse_model.py: the
parse of tests/zenc_model.py, the literals decision, the tree description and the bytes by
tests/zenc_fse_main.cpp from okv_zstd_enc.hpp's statements).  libzstd on each frame, the device
decoder and the C oracle on the file inflate it; oracle/zstd_ref.zstd_segment rebuilds the file
around the frames; the row partition is the uncompressed encode's; no block is larger than
under OKV_F_ZSTD_HUFFMAN alone, and that none larger than flag-off; two calls give the same
bytes.  That each fixture is the shape it claims is asserted without a GPU in
tests/test_zstd_fse_host.py.

OKV_PATH_ZSTD_HUF_FSE is set exactly when a frame of the call holds a tree header byte below
128, read from the bytes.  Census (test_census_is_complete, which runs last): both
descriptions, both accuracy logs and raw literals under the flag were all seen."""
from __future__ import annotations

import functools

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
from tests import zenc_fse_cases as FC
from tests import zenc_fse_model as F
from tests import zenc_model as M
from tests.test_get_zstd_gpu import Seg
from tests.test_snap_get_gpu import _seg
from tests.test_snap_get_zstd_gpu import ZEnv
from tests.test_snap_get_zstd_gpu import _check as snap_check
from tests.test_zstd_huf_gpu import _encode_device, _meta_of, _tensors

pytestmark = pytest.mark.gpu

UNIT = _lib.ZSTD_ENC_UNIT
CONFIGS = ZC.CONFIGS
ZSTD = okv.sst.COMP_ZSTD
CENSUS = set()
_raw, _closes = ZC.raw_of, ZC.closes
FLAGS = dict(zstd_native=True, zstd_huffman=True, zstd_huffman_fse=True)


@pytest.fixture(scope="module")
def enc():
    e = okv.Encoder(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def model(raw):
    return F.model(raw, F.FSE)


def parse_frame(frame, orig):
    """Per block of a frame, from the bytes alone: (block type, literals type, tree header
    byte or None, accuracy log of an FSE description or 0)."""
    pos, out = M.frame_header_size(orig), []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        assert typ in (0, 2)
        c = frame[pos:pos + size]
        if typ == 0:
            out.append((0, None, None, 0))
        else:
            lt, sf = c[0] & 3, (c[0] >> 2) & 3
            assert lt in (0, 2)
            if lt == 0:
                out.append((2, 0, None, 0))
            else:
                assert sf != 1
                hb = 3 if sf == 0 else 4 if sf == 2 else 5
                tree = c[hb]
                out.append((2, 2, tree, 5 + (c[hb + 1] & 15) if tree < 128 else 0))
        pos += size
        if last:
            break
    assert pos + 4 == len(frame)
    return out


def check(enc, decoder, rows, T, D, strict_go=True):
    """The whole contract for one row set; returns (host-mode Encoded, units of every block
    from the model, what parse_frame saw)."""
    got = enc.encode(rows, T, D, ZSTD, strict_go, **FLAGS)
    path = enc.last_path()
    assert path & _lib.PATH_ZSTD_ENC
    dev, bound, dev_path = _encode_device(enc, rows, T, D, strict_go, **FLAGS)
    again = enc.encode(rows, T, D, ZSTD, strict_go, **FLAGS)
    seg = got.seg.tobytes()
    assert again.seg.tobytes() == seg and dev.seg.tobytes() == seg and dev_path == path
    for a in (dev, again):
        assert np.array_equal(a.first_row, got.first_row) and np.array_equal(a.descs, got.descs)
        assert np.array_equal(a.hashes, got.hashes) and a.meta_hash == got.meta_hash
    assert got.file_bytes == len(seg) <= bound
    nb = got.n_blocks
    plain = enc.encode(rows, T, D, strict_go=strict_go)
    assert np.array_equal(plain.first_row, got.first_row) and int(got.first_row[nb]) == len(rows)
    huf = enc.encode(rows, T, D, ZSTD, strict_go, zstd_native=True, zstd_huffman=True)
    assert not enc.last_path() & _lib.PATH_ZSTD_HUF_FSE
    off = enc.encode(rows, T, D, ZSTD, strict_go, zstd_native=True)
    assert not enc.last_path() & (_lib.PATH_ZSTD_HUF | _lib.PATH_ZSTD_HUF_FSE)
    assert np.array_equal(off.first_row, got.first_row)
    frames, raws, seen = [], [], []
    for b in range(nb):
        o, bs, orig, cs = (int(x) for x in got.descs[b])
        raw = _raw(rows[int(got.first_row[b]):int(got.first_row[b + 1])])
        assert orig == len(raw) and bs == cs + (D - cs % D) and o % D == 0
        frame = seg[o:o + cs]
        assert Z.decompress(frame, orig) == raw, b
        assert seg[o + cs:o + bs] == bytes(bs - cs)
        assert cs <= int(huf.descs[b, 3]) <= int(off.descs[b, 3]) <= \
            orig + 3 * -(-orig // UNIT) + 18
        seen += parse_frame(frame, orig)
        frames.append(frame)
        raws.append(raw)
    units = []
    for b, raw in enumerate(raws):
        want, us = model(raw)
        assert frames[b] == want, (b, len(raw))
        units += us
    # the census of the bytes is the model's, and the path bits say what the bytes hold
    for s, u in zip(seen, units):
        c = u.census
        assert (s[0], s[1] or 0) == (c["block"], c["lit"])
        if s[1] == 2:
            assert (s[2] < 128) == (c["desc"] == 1) and s[3] == (c["alog"] if c["desc"] else 0)
            assert s[2] == (c["dbytes"] - 1 if c["desc"] else 127 + c["last"])
    assert bool(path & _lib.PATH_ZSTD_HUF) == any(s[1] == 2 for s in seen)
    assert bool(path & _lib.PATH_ZSTD_HUF_FSE) == any(s[1] == 2 and s[2] < 128 for s in seen)
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


FIXTURES = {name: rows for name, rows, _ in FC.fixtures()}
EXTRA = dict(FC.extra())


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixtures(enc, decoder, T, D, name):
    rows = FIXTURES[name]
    _, units, seen = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if name == "largest_129":  # raw under OKV_F_ZSTD_HUFFMAN alone
        assert seen[0][:2] == (2, 2) and seen[0][2] < 128 and seen[0][3] == 6
    if name == "fse_direct_raw":
        assert [(s[0], s[1], s[2] is not None and s[2] < 128) for s in seen] == \
            [(2, 2, True), (2, 2, False), (0, None, False)]
    if name == "all_weights_equal_above_128":
        assert seen[1] == (0, None, None, 0)


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", list(EXTRA))
def test_extra_rows(enc, decoder, T, D, name):
    rows = EXTRA[name]
    got, units, seen = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if name == "seven_bytes":
        assert [int(x) for x in got.descs[0]] == [0, D, 7, 6 + 3 + 7 + 4]
    if name == "random_bytes":
        assert all(s[1] != 2 for s in seen)
    if name == "utf8_rows":  # values above 128 in every block
        assert all(s[1] == 2 and s[2] < 128 for s in seen)
    if name == "binary_rows" and T == 3584:  # few literals a block: their tree does not pay
        assert all(s[:2] == (2, 0) for s in seen)


def test_contract(enc):
    """The flag needs OKV_F_ZSTD_HUFFMAN; calls without it after flagged calls give the bytes
    of a fresh context; the capacity contract of the encoder holds."""
    rows = EXTRA["utf8_rows"]
    T, D = CONFIGS[0]
    fresh = okv.Encoder(0)
    try:
        off = fresh.encode(rows, T, D, ZSTD, False, zstd_native=True)
        huf = fresh.encode(rows, T, D, ZSTD, False, zstd_native=True, zstd_huffman=True)
    finally:
        fresh.close()
    flagged = enc.encode(rows, T, D, ZSTD, False, **FLAGS)
    assert enc.last_path() & _lib.PATH_ZSTD_HUF_FSE and enc.last_path() & _lib.PATH_ZSTD_HUF
    assert int(flagged.descs[:, 3].sum()) < int(huf.descs[:, 3].sum()) <= \
        int(off.descs[:, 3].sum())
    big = FIXTURES["all_256"]  # (the FSE phases write all over the scratch LDS)
    enc.encode(big, T, D, ZSTD, False, **FLAGS)
    after_off = enc.encode(rows, T, D, ZSTD, False, zstd_native=True)
    assert not enc.last_path() & (_lib.PATH_ZSTD_HUF | _lib.PATH_ZSTD_HUF_FSE)
    after_huf = enc.encode(rows, T, D, ZSTD, False, zstd_native=True, zstd_huffman=True)
    assert not enc.last_path() & _lib.PATH_ZSTD_HUF_FSE
    assert after_off.seg.tobytes() == off.seg.tobytes()
    assert after_huf.seg.tobytes() == huf.seg.tobytes()
    r = okv.pack_rows(rows)
    t = _tensors(r)
    for native in (True, False):  # the new flag without OKV_F_ZSTD_HUFFMAN
        for call in (lambda: enc.encode(rows, T, D, ZSTD, False, zstd_native=native,
                                        zstd_huffman_fse=True),
                     lambda: enc.encode_device(t, len(rows), {}, T, D, ZSTD, False,
                                               zstd_native=native, zstd_huffman_fse=True)):
            with pytest.raises(okv.OkvError) as e:
                call()
            assert e.value.code == _lib.OKV_E_ARG
    with pytest.raises(okv.OkvError) as e:  # all three flags, no OKV_COMP_ZSTD
        enc.encode(rows, T, D, okv.sst.COMP_NONE, False, **FLAGS)
    assert e.value.code == _lib.OKV_E_ARG
    w = okv.GpuSegmentWriter(enc, zstd_level=1, zstd_native=True, zstd_huffman_fse=True)
    w.WriteRow(b"a", b"b")
    with pytest.raises(okv.OkvError) as e:
        w.Close()
    assert e.value.code == _lib.OKV_E_ARG
    # capacity: the bound comes from the raw sizes alone, with the flag as without
    kw = dict(key_arena_bytes=r["key_arena"].size, val_arena_bytes=r["val_arena"].size, **FLAGS)
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
    rows = EXTRA["utf8_rows"][:200]
    w = okv.GpuSegmentWriter(enc, zstd_level=1, **FLAGS)
    for k, v in rows:
        w.WriteRow(k, v)
    flen, _meta = w.Close()
    assert enc.last_path() & _lib.PATH_ZSTD_HUF_FSE
    md = okv.fetch_metadata(w.data(), flen)
    assert md.compression == ZSTD and flen == w.data().size
    dec = decoder.decode(w.data(), md.descs, ZSTD)
    assert [kv for b in range(md.descs.shape[0]) for kv in dec.block_rows(b)] == rows


def test_get_rows_on_a_compacted_fse_segment(enc, decoder):
    """compact(..., zstd=True, zstd_huffman=True, zstd_huffman_fse=True) writes FSE-described
    Huffman literals; get_rows(..., zstd=True) and snapshot.Reader.GetRows read every key of it
    as the oracle does."""
    def val(s, i):
        return ('{"seg":%d,"id":%d,"name":"nutzer%d","note":"%s"}' %
                (s, i, i * 7, "größe · " * (1 + i % 5))).encode()
    a = [(b"key%06d" % i, val(1, i)) for i in range(0, 900, 2)]
    b = [(b"key%06d" % i, val(2, i)) for i in range(300, 1200, 3)]
    for rows in (a, b):  # (the Go writer panics in Close when the last row closed a block)
        while _closes(rows, 3584):
            rows.append((rows[-1][0] + b"+", b"tail"))
    segs = [_seg("2", 0, b), _seg("1", 1, a)]
    dsegs = [(SN.DeviceSegment(enc, d, n), lvl) for _sid, lvl, d, n, _m in segs]
    plain = SN.compact(dsegs, enc)
    got = SN.compact(dsegs, enc, zstd=True, zstd_huffman=True, zstd_huffman_fse=True)
    assert enc.last_path() & _lib.PATH_ZSTD_HUF_FSE
    huf = SN.compact(dsegs, enc, zstd=True, zstd_huffman=True)
    assert got.n_rows == plain.n_rows and got.n_blocks == huf.n_blocks
    seg = got.seg.tobytes()[:got.file_bytes]
    meta = _meta_of(seg, got.file_bytes)
    md = P.bytes_to_metadata(meta)
    huf_md = P.bytes_to_metadata(_meta_of(huf.seg.tobytes(), huf.file_bytes))
    assert sum(st.CompressedSize for st in md.entries) < \
        sum(st.CompressedSize for st in huf_md.entries)
    kinds = [s for st in md.entries for s in
             parse_frame(seg[st.Offset:st.Offset + st.CompressedSize], st.OriginalSize)]
    assert any(s[1] == 2 and s[2] < 128 for s in kinds)
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
    """Runs last: both descriptions, both accuracy logs, raw literals under the flag and a
    Raw_Block were seen (the fixtures here alone show them all, so the test also stands when it
    is run alone)."""
    T, D = CONFIGS[1]
    for name in ("largest_129", "listed_101", "tie_+0", "fse_direct_raw"):
        rows = FIXTURES[name]
        check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    rows = EXTRA["random_bytes"]
    check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    rows = EXTRA["text_46"]
    check(enc, decoder, rows, T, D)
    rows = EXTRA["binary_rows"][:100]
    check(enc, decoder, rows, *CONFIGS[0], strict_go=not _closes(rows, CONFIGS[0][0]))
    huf = [s for s in CENSUS if s[1] == 2]
    assert any(s[2] >= 128 for s in huf), "direct weights under the flag"
    assert {s[3] for s in huf if s[2] < 128} == {5, 6}, "both accuracy logs"
    assert any(s[:2] == (2, 0) for s in CENSUS), "raw literals in a Compressed_Block"
    assert any(s[0] == 0 for s in CENSUS), "a Raw_Block"
