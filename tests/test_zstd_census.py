"""What the zstd cases hold (tests/zstd_census.py), and the hand-made frames of
tests/zstd_cases.py against libzstd and both oracles.  CPU only."""
from __future__ import annotations

import struct
from collections import Counter

import pytest

from oracle import coracle as CO
from oracle import pyoracle as P
from oracle import zstd_ref as Z
from tests import zstd_cases as ZC
from tests import zstd_census as ZS

# Every part of the format that no block of the suite reached, or few did, before
# the streamed and hand-made cases: feature -> the least number of blocks (frames,
# for the frame header's fields) that the oracle decodes with status 0.
REQUIRED = {
    # never seen in what one-shot libzstd emits for <= 64 KiB
    "ll.repeat": 1, "of.repeat": 1, "ml.repeat": 1,
    "lit.treeless": 1,
    "lit.rle": 1,
    "huf.direct": 1,
    "lit.compressed.sf1": 1, "lit.compressed.sf3": 1,
    "nseq.3byte": 1,
    "nseq.0": 1,
    "fcs.1": 1, "fcs.8": 1,
    "window.mantissa.nonzero": 1,
    "dictid.1": 1, "dictid.2": 1, "dictid.4": 1,
    # seen, but thinly
    "lit.compressed.streams1": 8, "lit.compressed.streams4": 8,
    "ll.predefined": 8, "of.predefined": 8, "ml.predefined": 8,
    "cblock.later": 8, "cblock.later.uses_prev": 4,
}


def test_required_list_is_the_shared_one():
    """The GPU module asserts zstd_census.REQUIRED before its cases run; it is
    this list."""
    assert ZS.REQUIRED == REQUIRED


def test_census_reads_the_headers_it_is_given():
    """The census on frames whose content is known from how they were written."""
    by = {(g, n): fr for g, n, fr, _w, _o in ZC.handmade_frames()}
    c = ZS.frames(by["two_blocks", "repeat_after_rle"])
    assert c == Counter({
        "frame": 1, "frame.windowed": 1, "frame.no_checksum": 1, "window.log.17": 1,
        "window.mantissa.0": 1, "dictid.0": 1, "fcs.0": 1, "frame.blocks.2": 1,
        "frame.multi_block": 1, "block.compressed": 2, "cblock.first": 1, "cblock.later": 1,
        "cblock.later.uses_prev": 1, "lit.compressed": 1, "lit.compressed.sf1": 1,
        "lit.compressed.streams4": 1, "huf.direct": 1, "lit.treeless": 1, "lit.treeless.sf1": 1,
        "lit.treeless.streams4": 1, "nseq.1byte": 2, "ll.rle": 1, "of.predefined": 1, "ml.rle": 1,
        "ll.repeat": 1, "of.repeat": 1, "ml.repeat": 1})
    c = ZS.frames(by["frame_headers", "dictid_2_bytes_0"] + Z.skippable_frame(b"abc", 3) +
                  by["rle_literals", "nseq0"] + by["nseq_3byte", "nseq_0x7f00"])
    for k, n in {"frame": 3, "frame.skippable": 1, "dictid.2": 1, "fcs.4": 1, "dictid.0": 2,
                 "lit.rle.sf3": 1, "nseq.0": 1, "nseq.3byte": 1, "nseq.1byte": 1, "lit.raw.sf3": 1,
                 "lit.raw.sf0": 1, "of.rle": 1, "ml.rle": 1, "ll.predefined": 2}.items():
        assert c[k] == n, (k, c[k])
    lz = Z.compress(b"".join(struct.pack("<HI", len(k), len(v)) + k + v
                             for k, v in ZC._a16_rows(3, 10)), 3)
    c = ZS.frames(lz)
    assert c["frame.single_segment"] == c["frame.checksum"] == c["block.compressed"] == 1
    assert c["lit.compressed.sf2"] == c["huf.fse"] == c["lit.compressed.streams4"] == 1
    assert c["cblock.first"] == c["fcs.2"] == c["frame.blocks.1"] == 1
    with pytest.raises(ZS.Malformed):
        ZS.frames(lz[:len(lz) // 2])
    with pytest.raises(ZS.Malformed):
        ZS.frames(b"\x00\x01\x02\x03" + lz)


def _census_of_decoded(cases):
    tot, per = Counter(), {}
    for name, seg, descs, _note in cases:
        st = P.decode_soa(seg, descs, P.COMP_ZSTD)["status"]
        per[name] = ZS.segment(seg, descs, st)
        tot.update(per[name])
    return tot, per


def test_success_cases_meet_the_required_list():
    """The union of ZC.cases(), counting only blocks the oracle decodes: every
    required feature at its count.  A libzstd that makes other choices than
    1.4.8 fails here (or on the line for the case below), not by decoding less."""
    tot, per = _census_of_decoded(ZC.cases())
    assert not ZS.missing(tot, REQUIRED), ZS.missing(tot, REQUIRED)
    for name, holds in ZC.STREAM_HOLDS.items():
        for k in holds:
            assert per[name][k] >= 1, (name, k)
        assert per[name]["frame.multi_block"] >= 3, name
    want = {"hand_rle_literals": {"lit.rle.sf0": 2, "lit.rle.sf1": 2, "lit.rle.sf3": 2, "nseq.0": 2},
            "hand_huf_direct": {"huf.direct": 6, "lit.compressed.streams1": 2,
                                "lit.compressed.streams4": 4, "lit.compressed.sf1": 3,
                                "lit.compressed.sf3": 1},
            "hand_nseq_small": {"nseq.1byte": 1, "nseq.2byte": 5},
            "hand_nseq_3byte": {"nseq.2byte": 1, "nseq.3byte": 2, "of.rle": 3, "ml.rle": 3},
            "hand_two_blocks": {"ll.repeat": 2, "of.repeat": 2, "ml.repeat": 2, "lit.treeless": 2,
                                "cblock.later.uses_prev": 2},
            "hand_frame_headers": {"fcs.1": 1, "fcs.2": 3, "fcs.4": 1, "fcs.8": 2, "dictid.1": 1,
                                   "dictid.2": 1, "dictid.4": 1, "window.mantissa.7": 1,
                                   "frame.checksum": 2}}
    for name, feats in want.items():
        for k, n in feats.items():
            assert per[name][k] == n, (name, k, per[name][k])


def test_long_runs_case_has_no_rle_literals():
    """test_zstd_long_runs_and_rle_literals' blocks (tests/test_zstd_gpu.py): long
    matches with raw literals, no RLE literals -- hand_rle_literals has those."""
    rows = []
    for i in range(120):
        v = bytes([i % 7]) * (4500 + 37 * i) if i % 3 else (b"ab" * 2100 + bytes(range(i % 50)))
        rows.append((b"r%06d" % i, v))
    seg, _, _ = Z.zstd_segment(rows, 57344, 65536, level=3)
    c = ZS.segment(seg, [st.desc() for st in P.bytes_to_metadata(ZC._meta_of(seg)).entries])
    assert c["lit.rle"] == 0 and c["lit.raw"] == c["block.compressed"] > 0


def test_handmade_frames_model_libzstd_and_oracles_agree():
    """Per hand-made success frame: the writer's model of its sequences == what
    libzstd decompresses == the rows both oracles walk out of it, which are one
    record covering every byte (or, for the all-zero RLE-literal frames, N / 6
    empty records: any other byte or length changes the walk)."""
    frames = ZC.handmade_frames()
    assert len({(g, n) for g, n, *_ in frames}) == len(frames) >= 40
    for group, name, fr, want, one in frames:
        assert Z.decompress(fr, len(want)) == want, (group, name)
        assert ZS.frames(fr)["frame.multi_block"] == (0 if one else 1), (group, name)
        seg, descs = ZC._frames_segment([(fr, len(want))])
        py = P.decode_soa(seg, descs, P.COMP_ZSTD)
        c = CO.decode_soa(seg, CO.descs_array(descs), P.COMP_ZSTD)
        assert py["status"] == [0] and list(c["status"]) == [0], (group, name)
        assert c["key_arena"].tobytes() == py["key_arena"], (group, name)
        assert c["val_arena"].tobytes() == py["val_arena"], (group, name)
        if any(want):
            klen, vlen = struct.unpack_from("<HI", want)
            assert 6 + klen + vlen == len(want) and klen > 0, (group, name)
            pad = lambda b: b + bytes(-len(b) % 16)  # an arena region is padded to 16
            assert py["key_arena"] == pad(want[6:6 + klen]), (group, name)
            assert py["val_arena"] == pad(want[6 + klen:]), (group, name)
            assert py["key_len"] == [klen] and py["val_len"] == [vlen]
            assert int(c["row_start"][-1]) == 1
        else:
            assert len(want) % 6 == 0 and int(c["row_start"][-1]) == len(want) // 6
            assert py["key_arena"] == py["val_arena"] == b""


def test_handmade_rejects_are_rejected_by_both_oracles():
    """Every reject frame: a zstd error from the Python and the C oracle."""
    names = [n for n, _, _ in ZC.handmade_rejects()]
    assert len(set(names)) == len(names) >= 24
    cc = {n: (seg, descs) for n, seg, descs in ZC.corrupt_cases()}
    for name in names:
        seg, descs = cc[name]
        py = P.decode_soa(seg, descs, P.COMP_ZSTD)
        c = CO.decode_soa(seg, CO.descs_array(descs), P.COMP_ZSTD)
        assert py["status"] == [P.BLK_ZSTD_ERROR] == list(c["status"]), name


def test_reserved_modes_bits_are_the_oracles_own_rule():
    """libzstd 1.4.8 decodes a block whose Symbol_Compression_Modes has a reserved
    bit set; RFC 8878 3.1.1.3.2.1 says the bits must be zero, and the oracles (as
    the device) reject it: Z._modes_reserved, zstd_modes_reserved in the C one."""
    fr, n = [(f, n) for name, f, n in ZC.handmade_rejects() if name == "modes_reserved_bit"][0]
    assert Z._oneshot(Z.lib(), fr, n) is not None and Z.decompress(fr, n) is None
    for _g, _n, ok, want, _o in ZC.handmade_frames():
        for blk in _compressed_blocks(ok):
            assert not Z._modes_reserved(blk)


def _compressed_blocks(fr):
    """Contents of a hand-made frame's compressed blocks (no dictionary ID)."""
    fhd = fr[4]
    at = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3] + \
        ((fhd >> 5) & 1, 2, 4, 8)[fhd >> 6]
    while True:
        bh = int.from_bytes(fr[at:at + 3], "little")
        at += 3
        n = 1 if (bh >> 1) & 3 == 1 else bh >> 3
        if (bh >> 1) & 3 == 2:
            yield fr[at:at + n]
        at += n
        if bh & 1:
            return
