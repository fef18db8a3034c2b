"""Header-level census of zstd frames (RFC 8878 3.1): which parts of the format
a set of frames holds.  A walk of frame, block, literals and sequences headers;
nothing is entropy-decoded (the literals section's compressed size is in its
header, so the sequences header is found without decoding).  Test helper: the
suite asserts with it that the decoder's arms are reached (REQUIRED)."""
from __future__ import annotations

import struct
from collections import Counter

MAGIC = 0xFD2FB528
LIT = ("raw", "rle", "compressed", "treeless")
MODE = ("predefined", "rle", "fse", "repeat")


class Malformed(ValueError):
    pass


def _need(data, at, n):
    if at + n > len(data):
        raise Malformed(f"truncated at {at}+{n}")


def compressed_block(body: bytes, first: bool) -> Counter:
    """Features of one Compressed_Block's content (3.1.1.3)."""
    c = Counter()
    _need(body, 0, 1)
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    if lt < 2:  # Raw / RLE literals: size formats 0 and 2 are the same 1-byte header
        hb = (1, 2, 1, 3)[sf]
        _need(body, 0, hb)
        regen = int.from_bytes(body[:hb], "little") >> (3 if hb == 1 else 4)
        c[f"lit.{LIT[lt]}.sf{sf if sf & 1 else 0}"] += 1
        at = hb + (regen if lt == 0 else 1)
    else:
        hb, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        _need(body, 0, hb)
        v = int.from_bytes(body[:hb], "little") >> 4
        csize = (v >> bits) & ((1 << bits) - 1)
        streams = 1 if sf == 0 else 4
        c[f"lit.{LIT[lt]}.sf{sf}"] += 1
        c[f"lit.{LIT[lt]}.streams{streams}"] += 1
        if lt == 2:
            _need(body, hb, 1)
            c["huf.direct" if body[hb] >= 128 else "huf.fse"] += 1
        at = hb + csize
    c[f"lit.{LIT[lt]}"] += 1
    _need(body, at, 1)
    b0 = body[at]
    if b0 == 0:
        c["nseq.0"] += 1
        nseq = 0
        at += 1
    elif b0 < 128:
        c["nseq.1byte"] += 1
        nseq = b0
        at += 1
    elif b0 < 255:
        _need(body, at, 2)
        c["nseq.2byte"] += 1
        nseq = ((b0 - 128) << 8) + body[at + 1]
        at += 2
    else:
        _need(body, at, 3)
        c["nseq.3byte"] += 1
        nseq = body[at + 1] + (body[at + 2] << 8) + 0x7F00
        at += 3
    uses_prev = lt == 3
    if nseq:
        _need(body, at, 1)
        m = body[at]
        for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
            mode = (m >> sh) & 3
            c[f"{name}.{MODE[mode]}"] += 1
            uses_prev |= mode == 3
        if m & 3:
            c["modes.reserved"] += 1
    c["cblock.first" if first else "cblock.later"] += 1
    if not first and uses_prev:
        c["cblock.later.uses_prev"] += 1
    return c


def frames(data: bytes) -> Counter:
    """Features of every frame in `data` (a block's CompressedSize bytes)."""
    c = Counter()
    at = 0
    while at < len(data):
        _need(data, at, 4)
        magic, = struct.unpack_from("<I", data, at)
        at += 4
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            _need(data, at, 4)
            n, = struct.unpack_from("<I", data, at)
            _need(data, at + 4, n)
            at += 4 + n
            c["frame.skippable"] += 1
            continue
        if magic != MAGIC:
            raise Malformed(f"magic {magic:#x}")
        _need(data, at, 1)
        fhd = data[at]
        at += 1
        single = (fhd >> 5) & 1
        if fhd & 8:
            c["frame.reserved_bit"] += 1
        c["frame.single_segment" if single else "frame.windowed"] += 1
        c["frame.checksum" if fhd & 4 else "frame.no_checksum"] += 1
        if not single:
            _need(data, at, 1)
            c[f"window.log.{10 + (data[at] >> 3)}"] += 1
            c[f"window.mantissa.{data[at] & 7}"] += 1
            if data[at] & 7:
                c["window.mantissa.nonzero"] += 1
            at += 1
        did = (0, 1, 2, 4)[fhd & 3]
        c[f"dictid.{did}"] += 1
        fcs = (single, 2, 4, 8)[fhd >> 6]
        c[f"fcs.{fcs}"] += 1
        _need(data, at, did + fcs)
        at += did + fcs
        c["frame"] += 1
        nblocks = 0
        while True:
            _need(data, at, 3)
            bh = int.from_bytes(data[at:at + 3], "little")
            at += 3
            last, bt, size = bh & 1, (bh >> 1) & 3, bh >> 3
            if bt == 3:
                raise Malformed("reserved block type")
            c[("block.raw", "block.rle", "block.compressed")[bt]] += 1
            n = 1 if bt == 1 else size
            _need(data, at, n)
            if bt == 2:
                c.update(compressed_block(data[at:at + n], nblocks == 0))
            at += n
            nblocks += 1
            if last:
                break
        c[f"frame.blocks.{nblocks if nblocks < 4 else '4+'}"] += 1
        if nblocks > 1:
            c["frame.multi_block"] += 1
        if fhd & 4:
            _need(data, at, 4)
            at += 4
    return c


def segment(seg: bytes, descs, statuses=None) -> Counter:
    """Census of a segment's blocks; with `statuses`, only of the blocks whose
    status is 0."""
    c = Counter()
    for i, d in enumerate(descs):
        if statuses is not None and statuses[i] != 0:
            continue
        off, csize = int(d[0]), int(d[3])
        c.update(frames(seg[off:off + csize]))
    return c


# What the success cases of tests/zstd_cases.py must hold, counted over blocks
# the oracle decodes: feature -> minimum number of blocks (frames for the frame
# header fields).  One-shot libzstd frames of <= 64 KiB hold none of the first
# group and little of the second.
REQUIRED = {
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
    # seen before, but thinly
    "lit.compressed.streams1": 8, "lit.compressed.streams4": 8,
    "ll.predefined": 8, "of.predefined": 8, "ml.predefined": 8,
    "cblock.later": 8, "cblock.later.uses_prev": 4,
}


def missing(c: Counter, required=None) -> dict:
    """{feature: (have, want)} for what `c` lacks of `required`."""
    required = REQUIRED if required is None else required
    return {k: (c[k], n) for k, n in required.items() if c[k] < n}
