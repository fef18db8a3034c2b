"""The zstd block encoder on the device (OKV_F_ZSTD_NATIVE, okv_zstd_enc.hip).

Every case runs at T=3584, D=4096 and at T=61440, D=65536, in host mode and in
device-pointer mode (the two must give the same bytes), and is checked by three
decoders -- libzstd on each frame, the device decoder and the C oracle on the file --
and by a byte-exact rebuild of the file around the device's frames
(oracle/zstd_ref.zstd_segment with frame_fn).  Every frame must also equal, byte for byte,
the frame a CPU model of the kernel's parse predicts (tests/zenc_model.py: the candidate
search, the quarter parse, the list merge and the Raw / Compressed decision restated in
numpy, the frame bytes written by tests/zenc_main.cpp without sanitizers), so a parse that
merely round-trips does not pass.

Frame census.  The encoder can emit: Raw_Blocks and Compressed_Blocks; the 1-, 2- and
3-byte Raw_Literals_Block headers; the 1- and 2-byte Number_of_Sequences forms.  All of
those are seen over this file (test_census_is_complete, which runs last).  Unreachable:
the 3-byte Number_of_Sequences form (>= 0x7F00 sequences: a unit of
OKV_ZSTD_ENC_UNIT = 32 768 bytes holds at most 8 192 matches of 4 bytes), RLE_Blocks,
RLE / Huffman literals and non-predefined table modes (not built).

The 46 text rows have 12-byte keys and 59-byte values: 46 * (6 + 12 + 59) = 3 542 raw
bytes, the figure the compression condition is stated for."""
from __future__ import annotations

import random
import struct

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import _lib
from objectkv_amd import snapshot as SN
from objectkv_amd.bloom import DeviceBloom
from oracle import coracle as CO
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import snapshot_cases as SC
from tests import zenc_cases as ZC
from tests import zenc_model as M

pytestmark = pytest.mark.gpu

UNIT = _lib.ZSTD_ENC_UNIT
CONFIGS = ZC.CONFIGS
ZSTD = okv.sst.COMP_ZSTD
CENSUS = {"block": set(), "lit": set(), "nseq": set(), "fcs": set()}


@pytest.fixture(scope="module")
def enc():
    e = okv.Encoder(0)
    yield e
    e.close()


_raw = ZC.raw_of
_text_rows, _random_rows, _closes = ZC.text_rows, ZC.random_rows, ZC.closes
_periodic, _mixed, PERIODIC, EDGES = ZC.periodic, ZC.mixed, ZC.PERIODIC, ZC.EDGES


def _tensors(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16,
              np.dtype(np.uint32): np.int32}
    return {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
            for k, v in r.items()}


def _encode_device(enc, rows, T, D, strict_go=True, bloom=None, close=True):
    """Size query, the bound, then the encode: (Encoded, bound file bytes)."""
    r = okv.pack_rows(rows)
    t = _tensors(r)
    kw = dict(key_arena_bytes=r["key_arena"].size, val_arena_bytes=r["val_arena"].size,
              zstd_native=True)
    with pytest.raises(okv.OkvError) as e:
        enc.encode_device(t, len(rows), {}, T, D, ZSTD, strict_go, bloom=bloom, **kw)
    assert e.value.code == _lib.OKV_E_CAPACITY
    need = e.value.out  # (the filter's bytes count: adding the rows twice changes no bit)
    nb, bound = int(need.n_blocks), int(need.file_bytes)
    assert need.data_bytes + need.meta_bytes + 25 == bound and need.data_bytes % D == 0
    out = {"seg": torch.zeros(bound, dtype=torch.uint8, device="cuda"),
           "first_row": torch.zeros(nb + 1, dtype=torch.int64, device="cuda"),
           "desc": torch.zeros((nb, 4), dtype=torch.int64, device="cuda"),
           "hash": torch.zeros(nb, dtype=torch.int64, device="cuda")}
    eo = enc.encode_device(t, len(rows), out, T, D, ZSTD, strict_go, close=close, bloom=bloom,
                           **kw)
    assert enc.last_path() & _lib.PATH_ZSTD_ENC
    if not close:
        assert eo.meta_hash == 0
        enc.close_device(eo)
    assert eo.n_blocks == nb and eo.file_bytes <= bound
    return okv.sst.Encoded(out["seg"][:eo.file_bytes].cpu().numpy(), int(eo.file_bytes),
                           int(eo.data_bytes), int(eo.meta_bytes), int(eo.meta_hash),
                           out["first_row"].cpu().numpy().view(np.uint64),
                           out["desc"].cpu().numpy().view(np.uint64),
                           out["hash"].cpu().numpy().view(np.uint64)), bound


def _parse_frame(frame, orig):
    """Header and block census of one frame; returns the block types."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert (fhd >> 5) & 1 == 1, "Single_Segment"
    assert (fhd >> 2) & 1 == 1, "Content_Checksum"
    assert fhd & 3 == 0 and (fhd >> 3) & 1 == 0, "no dictionary, no reserved bit"
    flag = fhd >> 6
    nb = (1, 2, 4, 8)[flag]
    fcs = int.from_bytes(frame[5:5 + nb], "little") + (256 if flag == 1 else 0)
    assert fcs == orig
    assert flag == (0 if orig < 256 else 1 if orig < 65792 else 2 if orig < 1 << 32 else 3)
    CENSUS["fcs"].add(nb)
    pos, types, total = 5 + nb, [], 0
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little")
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        pos += 3
        assert typ in (0, 2)
        content = frame[pos:pos + size]
        assert len(content) == size
        types.append(typ)
        CENSUS["block"].add(typ)
        if typ == 0:
            assert 0 < size <= UNIT
            total += size
        else:
            assert size < UNIT
            b0 = content[0]
            assert b0 & 3 == 0, "Raw_Literals_Block"
            sf = (b0 >> 2) & 3
            hb = 1 if sf in (0, 2) else 2 if sf == 1 else 3
            nlit = int.from_bytes(content[:hb], "little") >> (3 if hb == 1 else 4)
            assert hb == (1 if nlit < 32 else 2 if nlit < 4096 else 3)
            s0 = content[hb + nlit]
            form = 1 if s0 < 128 else 2 if s0 < 255 else 3
            assert s0 > 0 and content[hb + nlit + form] == 0, "Predefined_Mode x 3"
            CENSUS["lit"].add(hb)
            CENSUS["nseq"].add(form)
        pos += size
        if last:
            break
    assert pos + 4 == len(frame)
    return types


def check(enc, decoder, rows, T, D, strict_go=True, compressible=None):
    """The whole contract for one row set; returns the host-mode Encoded."""
    got = enc.encode(rows, T, D, ZSTD, strict_go, zstd_native=True)
    assert enc.last_path() & _lib.PATH_ZSTD_ENC
    dev, bound = _encode_device(enc, rows, T, D, strict_go)
    again = enc.encode(rows, T, D, ZSTD, strict_go, zstd_native=True)
    seg = got.seg.tobytes()
    # 5. determinism, and the two modes agree
    assert again.seg.tobytes() == seg and dev.seg.tobytes() == seg
    for a in (dev, again):
        assert np.array_equal(a.first_row, got.first_row) and np.array_equal(a.descs, got.descs)
        assert np.array_equal(a.hashes, got.hashes) and a.meta_hash == got.meta_hash
    assert got.file_bytes == len(seg) <= bound
    nb = got.n_blocks
    # 2. the row partition is the uncompressed encode's
    plain = enc.encode(rows, T, D, strict_go=strict_go)
    assert np.array_equal(plain.first_row, got.first_row)
    assert int(got.first_row[nb]) == len(rows)
    # 1a. libzstd on every frame; 3. census and the size bound
    frames, kinds, raws = [], [], []
    for b in range(nb):
        off, bs, orig, cs = (int(x) for x in got.descs[b])
        raw = _raw(rows[int(got.first_row[b]):int(got.first_row[b + 1])])
        assert orig == len(raw) and bs == cs + (D - cs % D) and off % D == 0
        frame = seg[off:off + cs]
        assert Z.decompress(frame, orig) == raw, b
        assert seg[off + cs:off + bs] == bytes(bs - cs)
        assert cs <= orig + 3 * -(-orig // UNIT) + 18
        kinds += _parse_frame(frame, orig)
        frames.append(frame)
        raws.append(raw)
    # 6. the frame is the one the parse means to write: the CPU model's, byte for byte
    for b, (want_frame, _units) in enumerate(M.model_frames(raws)):
        assert frames[b] == want_frame, (b, len(raws[b]))
    if compressible is True:
        assert 2 in kinds
    if compressible is False:
        assert set(kinds) == {0}
    # 2. the file around the frames, byte for byte
    want, want_len, want_meta = Z.zstd_segment(rows, T, D, frame_fn=lambda raw, i: frames[i])
    assert seg == want and got.file_bytes == want_len and got.meta() == want_meta
    rc, md = CO.fetch_meta(seg, got.file_bytes)
    assert rc == 0 and md["compression"] == 1 and len(md["entries"]) == nb
    for b, ent in enumerate(md["entries"]):
        assert [ent["offset"], ent["block_size"], ent["original_size"],
                ent["compressed_size"]] == [int(x) for x in got.descs[b]]
        assert ent["hash"] == int(got.hashes[b]) == P.xxh64(seg[ent["offset"]:ent["offset"] +
                                                               ent["block_size"]])
        assert ent["first_key"] == rows[int(got.first_row[b])][0]
    # 1b. the device decoder; 1c. the C oracle
    dec = decoder.decode(got.seg, got.descs, ZSTD)
    assert int(dec.status.max()) == 0
    assert [kv for b in range(nb) for kv in dec.block_rows(b)] == \
        [(k, v or None) for k, v in rows]
    ref = CO.decode_soa(seg, CO.descs_array([tuple(int(x) for x in d) for d in got.descs]), 1)
    for k in ("status", "row_start", "key_off", "key_len", "val_off", "val_len"):
        assert np.array_equal(getattr(dec, k), ref[k]), k
    assert dec.key_arena.tobytes() == ref["key_arena"].tobytes()
    assert dec.val_arena.tobytes() == ref["val_arena"].tobytes()
    return got


@pytest.mark.parametrize("T,D", CONFIGS)
def test_text_rows_three_decoders_and_compression(enc, decoder, T, D):
    rows = _text_rows(46)
    assert len(_raw(rows)) == 3542
    got = check(enc, decoder, rows, T, D, compressible=True)
    cs, orig = int(got.descs[:, 3].sum()), int(got.descs[:, 2].sum())
    print(f"text rows: CompressedSize {cs} of {orig}; libzstd-1 "
          f"{len(Z.compress(_raw(rows), 1))}, libzstd-3 {len(Z.compress(_raw(rows), 3))}")
    assert cs <= orig // 2
    # many rows: units with more than 127 sequences, several blocks
    rows = _text_rows(1500)
    check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T), compressible=True)


@pytest.mark.parametrize("T,D", CONFIGS)
def test_random_input_is_raw_blocks(enc, decoder, T, D):
    """Random bytes with nothing to find: one row per block (so the only structured bytes
    of a block are one 6-byte record header), every zstd block a Raw_Block, the size bound
    of the interface met (check() asserts it for every block)."""
    rows = ZC.random_raw(T)
    got = check(enc, decoder, rows, T, D, strict_go=False, compressible=False)
    assert got.n_blocks == 5
    for off, bs, orig, cs in got.descs:
        units = -(-int(orig) // UNIT)
        assert int(cs) == int(orig) + 3 * units + 4 + (9 if orig >= 65792 else 7)


@pytest.mark.parametrize("T,D", CONFIGS)
def test_random_rows_mixed(enc, decoder, T, D):
    rows = _random_rows(3, 400, 700)
    check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("N,P_", PERIODIC)
def test_periodic_value(enc, decoder, T, D, N, P_):
    rows = _periodic(P_, N)
    assert len(_raw(rows)) == N
    got = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T), compressible=True)
    cs = int(got.descs[0, 3])
    units = -(-N // UNIT)
    print(f"periodic N={N} P={P_}: CompressedSize {cs}; libzstd-1 "
          f"{len(Z.compress(_raw(rows), 1))}, libzstd-3 {len(Z.compress(_raw(rows), 3))}")
    assert got.n_blocks == 1 and cs <= units * P_ + N // 8 + 64


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edges(enc, decoder, T, D, name):
    rows = EDGES[name]()
    got = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if name == "value_200k_random":
        assert int(got.descs[-1, 1]) > 128 * 1024 and int(got.descs[-1, 3]) > 200 * 1024
    if name == "zeros_70000":
        assert int(got.descs[0, 3]) < 200
    if name == "seven_raw_bytes":
        assert [int(x) for x in got.descs[0]] == [0, D, 7, 6 + 3 + 7 + 4]


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("nblocks", [255, 256, 257])
def test_block_counts(enc, decoder, T, D, nblocks):
    """One row per block (each row alone reaches the threshold), so the last row closes
    a block: Go panics in Close (strict_go, Q1), the footer is written otherwise."""
    rows = ZC.block_pattern(T, nblocks)
    got = check(enc, decoder, rows, T, D, strict_go=False, compressible=True)
    assert got.n_blocks == nblocks
    if nblocks == 256:
        r = okv.pack_rows(rows)
        for call in (lambda: enc.encode(rows, T, D, ZSTD, True, zstd_native=True),
                     lambda: enc.encode_device(_tensors(r), nblocks, {}, T, D, ZSTD, True,
                                               zstd_native=True)):
            with pytest.raises(okv.OkvError) as e:
                call()
            assert e.value.code == _lib.W_NIL_WRITER


@pytest.mark.parametrize("T,D", CONFIGS)
def test_bloom_bytes_and_no_close(enc, decoder, T, D):
    """OKV_F_BLOOM_DEVICE together with zstd: the filter bytes sit in the meta block; and
    OKV_F_NO_CLOSE + okv_encode_close give the same file."""
    rows = _text_rows(300)
    plain = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    f = DeviceBloom(enc, 1000, 7)
    got = enc.encode(rows, T, D, ZSTD, not _closes(rows, T), bloom=f, zstd_native=True)
    bb = f.to_bytes()
    f.close()
    f = DeviceBloom(enc, 1000, 7)
    dev, _ = _encode_device(enc, rows, T, D, not _closes(rows, T), bloom=f, close=False)
    f.close()
    meta = plain.meta()
    at = 4 + len(rows[0][0]) + len(rows[-1][0])
    assert meta[at] == 0
    want_meta = meta[:at] + b"\x01" + struct.pack("<Q", len(bb)) + bb + meta[at + 1:]
    want = plain.seg.tobytes()[:plain.data_bytes] + want_meta + \
        struct.pack("<QQBQ", plain.data_bytes, P.xxh64(want_meta), 1, P.MAGIC)
    assert got.seg.tobytes() == want and dev.seg.tobytes() == want
    assert dev.meta_hash == P.xxh64(want_meta)
    rc, md = CO.fetch_meta(want, len(want))
    assert rc == 0 and md["has_bloom"] and md["compression"] == 1


def test_capacity_contract(enc):
    rows = _text_rows(500)
    T, D = CONFIGS[0]
    r = okv.pack_rows(rows)
    t = _tensors(r)
    kw = dict(key_arena_bytes=r["key_arena"].size, val_arena_bytes=r["val_arena"].size,
              zstd_native=True)
    plain = enc.encode(rows, T, D, strict_go=False)
    with pytest.raises(okv.OkvError) as e:  # the size query
        enc.encode_device(t, len(rows), {}, T, D, ZSTD, False, **kw)
    q = e.value.out
    assert e.value.code == _lib.OKV_E_CAPACITY and q.n_blocks == plain.n_blocks
    # the bound from the raw sizes alone: every block as Raw_Blocks + frame overhead, padded
    bound = 0
    for orig in (int(x) for x in plain.descs[:, 2]):
        fb = orig + 3 * -(-orig // UNIT) + 18
        bound += fb + (D - fb % D)
    assert q.data_bytes == bound and q.file_bytes == bound + q.meta_bytes + 25
    assert q.meta_bytes == plain.meta_bytes
    # one byte short of the bound: still a capacity error, nothing written
    seg = torch.full((int(q.file_bytes),), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(okv.OkvError) as e:
        enc.encode_device(t, len(rows), {"seg": seg[:-1]}, T, D, ZSTD, False, **kw)
    assert e.value.code == _lib.OKV_E_CAPACITY and e.value.out.file_bytes == q.file_bytes
    assert int(seg.min()) == 0xAB
    eo = enc.encode_device(t, len(rows), {"seg": seg}, T, D, ZSTD, False, **kw)
    assert eo.file_bytes <= q.file_bytes and eo.data_bytes <= q.data_bytes
    assert eo.file_bytes == eo.data_bytes + eo.meta_bytes + 25
    host = enc.encode(rows, T, D, ZSTD, False, zstd_native=True)
    assert seg[:eo.file_bytes].cpu().numpy().tobytes() == host.seg.tobytes()


def test_unchanged_behaviour(enc):
    """Without the flag zstd is still unsupported; the flag needs COMP_ZSTD; and the
    uncompressed encode on a context that has run the zstd encoder is the oracle writer's."""
    rows = _random_rows(11, 700, 200)

    def oracle():
        w = CO.Writer(3584, 4096, 0, False)
        for k, v in rows:
            assert w.write_row(k, v) == 0
        return w.close()
    rc, want, _ = oracle()
    strict = rc == 0
    if not strict:
        hw = okv.SegmentWriter(3584, 4096, 0, False)
        for k, v in rows:
            hw.WriteRow(k, v)
        hw.Close(strict_go=False)
        want = hw.data().tobytes()
    assert enc.encode(rows, strict_go=strict).seg.tobytes() == want
    with pytest.raises(okv.OkvError) as e:
        enc.encode(rows, compression=ZSTD)
    assert e.value.code == _lib.W_UNSUPPORTED
    w = okv.GpuSegmentWriter(enc, zstd_level=3)
    w.WriteRow(b"a", b"b")
    with pytest.raises(okv.OkvError) as e:
        w.Close()
    assert e.value.code == _lib.W_UNSUPPORTED
    for comp in (okv.sst.COMP_NONE, okv.sst.COMP_LZ4):
        with pytest.raises(okv.OkvError) as e:
            enc.encode(rows, compression=comp, zstd_native=True)
        assert e.value.code == _lib.OKV_E_ARG
    z = enc.encode(rows, compression=ZSTD, strict_go=strict, zstd_native=True)
    assert z.file_bytes > 0
    got = enc.encode(rows, strict_go=strict)
    assert got.seg.tobytes() == want and not enc.last_path() & _lib.PATH_ZSTD_ENC


def test_gpu_segment_writer_zstd_native(enc, decoder):
    rows = _text_rows(200)
    w = okv.GpuSegmentWriter(enc, zstd_level=1, zstd_native=True)
    for k, v in rows:
        w.WriteRow(k, v)
    flen, meta = w.Close()
    md = okv.fetch_metadata(w.data(), flen)
    assert md.compression == ZSTD and flen == w.data().size
    dec = decoder.decode(w.data(), md.descs, ZSTD)
    assert [kv for b in range(md.descs.shape[0]) for kv in dec.block_rows(b)] == rows


def test_compact_zstd(enc, decoder):
    """compact(..., zstd=True) over overlapping segments: the output decodes on the device
    and by libzstd to the rows of the uncompressed compaction."""
    segs, _ = SC.random_snapshot(21, nseg=2, rows_per_seg=(200, 600), keyspace=900)
    order = sorted(segs, key=lambda s: (s[1], [-ord(c) for c in s[0]]))
    dsegs = [(SN.DeviceSegment(enc, d, n), lvl) for _sid, lvl, d, n, _m in order]
    plain = SN.compact(dsegs, enc)
    got = SN.compact(dsegs, enc, zstd=True)
    assert got.n_rows == plain.n_rows and got.n_blocks == plain.n_blocks
    pmd = okv.fetch_metadata(plain.seg, plain.file_bytes)
    pdec = decoder.decode(plain.seg, pmd.descs)
    want = [kv for b in range(pmd.descs.shape[0]) for kv in pdec.block_rows(b)]
    md = okv.fetch_metadata(got.seg, got.file_bytes)
    assert md.compression == ZSTD
    dec = decoder.decode(got.seg, md.descs, ZSTD)
    assert int(dec.status.max()) == 0
    assert [kv for b in range(md.descs.shape[0]) for kv in dec.block_rows(b)] == want
    seg = got.seg.tobytes()
    raw = b"".join(Z.decompress(seg[int(o):int(o) + int(cs)], int(orig))
                   for o, _bs, orig, cs in md.descs)
    assert raw == _raw([(k, v or b"") for k, v in want])
    assert all(int(cs) <= int(orig) + 3 * -(-int(orig) // UNIT) + 18
               for _o, _bs, orig, cs in md.descs)
    assert int(md.descs[:, 3].sum()) < int(md.descs[:, 2].sum())  # (keys share prefixes)


PARSE = {name: (rows, ok) for name, rows, ok in ZC.parse_fixtures()}


@pytest.mark.parametrize("T,D", CONFIGS)
@pytest.mark.parametrize("name", list(PARSE))
def test_parse_fixtures(enc, decoder, T, D, name):
    """The smallest shapes at which a phase of the unit kernel can go wrong (tests/zenc_cases.py);
    check() holds every frame against the CPU model byte for byte.  That each fixture is the
    shape it claims to be (which quarters parse, which hash groups form, where matches end,
    the sequence counts, compressed size - n) is asserted from the model's census without a
    GPU in tests/test_zstd_enc_model.py."""
    rows, _ = PARSE[name]
    check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))


@pytest.mark.parametrize("name,T,D", [(n, T, D) for n, T, D, _ in ZC.writer_cases()])
def test_writer_options(enc, decoder, name, T, D):
    """The zstd path at block sizes that are no multiple of 16 (the place kernel's byte
    stores, the bytewise meta kernel behind an unaligned data area), at tiny thresholds, with
    multi-unit blocks at D % 16 != 0, and with long FirstKeys read through the row arrays
    (the meta kernel's byte-store arm in one group of 256 blocks and not in its neighbour)."""
    rows = {n: r for n, _T, _D, r in ZC.writer_cases()}[name]
    got = check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    if D in (1, 100):
        assert got.data_bytes % 16 != 0, "the meta block is not 16-byte aligned"
    if T == 70000:
        assert int(got.descs[:, 2].max()) > 2 * UNIT
    if name.startswith("long_first_keys"):
        assert got.n_blocks == len(rows) >= 600
        g = ZC.meta_group_bytes([rows[int(r)][0] for r in got.first_row[:-1]])
        assert g[0] > ZC.META_IMAGE and g[1] + 30 <= ZC.META_IMAGE and g[2] > ZC.META_IMAGE


def test_census_is_complete(enc, decoder):
    """Runs last: over the file, every form the encoder can emit was seen (the three
    fixtures here alone show them all, so the test also stands when it is run alone)."""
    T, D = CONFIGS[1]
    for rows in (_periodic(1, 3600),                               # < 32 literals, 1 sequence
                 _periodic(30000, 65000),                          # >= 4096 literals
                 _text_rows(1500),                                 # > 127 sequences
                 _periodic(7, 200000),                             # a 4-byte FCS
                 [(b"r", random.Random(2).randbytes(100))]):       # a Raw_Block, 1-byte FCS
        check(enc, decoder, rows, T, D, strict_go=not _closes(rows, T))
    assert CENSUS["block"] == {0, 2}
    assert CENSUS["lit"] == {1, 2, 3}
    assert CENSUS["nseq"] == {1, 2}
    assert {1, 2, 4} <= CENSUS["fcs"]
