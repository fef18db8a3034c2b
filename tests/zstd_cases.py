"""zstd decode cases shared by the CPU oracle test and the GPU parity test.
The blocks are frame sets from libzstd (oracle/zstd_ref.py: one-shot and
streamed) and from the frame writer below (RFC 8878, for what libzstd never
emits); libzstd checks them all.  See DESIGN.md for why libzstd is the checker
(klauspost v1.17.9 is not available offline) and 17.6 for what the cases reach."""
from __future__ import annotations

import bisect
import functools
import random
import struct

from oracle import zstd_ref as Z


def _rows(seed, n, kmax=40, vmax=300, text=True):
    rng = random.Random(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"kv", b"segment", b"block", b"zstd"]
    out = []
    for i in range(n):
        k = b"k%07d" % i + bytes(rng.getrandbits(8) for _ in range(rng.randint(0, kmax)))
        if text:
            v = b" ".join(rng.choice(words) for _ in range(rng.randint(0, vmax // 6)))
        else:
            v = bytes(rng.getrandbits(8) for _ in range(rng.randint(0, vmax)))
        out.append((k, v))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, segment bytes, descs [(off, bsize, orig, csize)], note)]"""
    from oracle import pyoracle as P
    out = []

    def add(name, seg, note):
        md = P.bytes_to_metadata(_meta_of(seg))
        out.append((name, seg, [st.desc() for st in md.entries], note))

    for lvl in (1, 3, 9, 19):
        seg, _, _ = Z.zstd_segment(_rows(lvl, 1500), 3584, 4096, level=lvl)
        add(f"text_l{lvl}", seg, "Huffman literals, FSE sequences, repeat offsets")
    seg, _, _ = Z.zstd_segment(_rows(7, 400, vmax=4000, text=False), 57344, 65536, level=3)
    add("random_64k", seg, "incompressible: raw blocks")
    seg, _, _ = Z.zstd_segment(_rows(8, 3000, vmax=2000), 57344, 65536, level=5,
                               checksum=False, content_size=False)
    add("text_64k_nocsum_nofcs", seg, "no checksum, no frame content size")
    zeros = [(b"z%06d" % i, bytes(1000)) for i in range(300)]
    seg, _, _ = Z.zstd_segment(zeros, 57344, 65536, level=3)
    add("zeros", seg, "RLE blocks / long matches")
    seg, _, _ = Z.zstd_segment(_rows(9, 2000, vmax=600), 57344, 65536, level=19)
    add("text_64k_l19", seg, "level 19")

    def multi(raw, i):  # two frames + a skippable frame per block
        h = len(raw) // 2
        return Z.compress(raw[:h], 3) + Z.skippable_frame(b"skip%d" % i, i) + \
            Z.compress(raw[h:], 1, checksum=False)
    seg, _, _ = Z.zstd_segment(_rows(10, 600), 3584, 4096, frame_fn=multi)
    add("multi_frame_skippable", seg, "concatenated frames + skippable frame")

    # one frame per segment block, a block closed every `piece` bytes
    # (Z.compress_stream): the later blocks repeat tables and trees.  More than
    # one block per frame, so the staged path's prologue hands every one of these
    # to the general kernel (its stages take one frame of one block); both device
    # paths still decode them.
    for name, (rows, th, bs, lvl, piece) in STREAM_CASES.items():
        seg, _, _ = Z.zstd_segment(rows(), th, bs, frame_fn=lambda raw, i, lvl=lvl, piece=piece:
                                   Z.compress_stream(raw, lvl, piece))
        add(name, seg, "streamed: " + ", ".join(STREAM_HOLDS[name]))

    # hand-made frames, one per segment block, grouped
    groups = {}
    for group, name, fr, want, _one in handmade_frames():
        groups.setdefault(group, []).append((name, fr, len(want)))
    for group, frs in groups.items():
        seg, descs = _frames_segment([(fr, n) for _, fr, n in frs])
        out.append(("hand_" + group, seg, descs, "hand-made: " + ", ".join(n for n, _, _ in frs)))
    return out


def _a16_rows(seed, n):
    """Values of random letters from an alphabet of 16: four bits a byte for the
    Huffman coder, next to nothing for the match finder."""
    rng = random.Random(seed)
    return [(b"a%07d" % i, bytes(97 + rng.randrange(16) for _ in range(rng.randint(200, 1800))))
            for i in range(n)]


# name -> (rows, threshold, block size, level, bytes per flush)
STREAM_CASES = {
    "stream_a16_l1_2k": (lambda: _a16_rows(61, 180), 57344, 65536, 1, 2048),
    "stream_a16_l3_8k": (lambda: _a16_rows(62, 180), 57344, 65536, 3, 8192),
    "stream_a16_l3_20k": (lambda: _a16_rows(63, 180), 57344, 65536, 3, 20480),
    "stream_a16_l19_2k": (lambda: _a16_rows(64, 180), 57344, 65536, 19, 2048),
    "stream_a16_l1_200": (lambda: _a16_rows(66, 12), 3584, 4096, 1, 200),
    "stream_text_l19_2k": (lambda: _rows(67, 1100, vmax=600), 57344, 65536, 19, 2048),
}
# what libzstd 1.4.8 puts into each (tests/zstd_census.py's names): a CPU test
# holds it, so another libzstd's choices show there and not as lost coverage
STREAM_HOLDS = {
    "stream_a16_l1_2k": ("lit.treeless.sf1", "lit.treeless.sf2", "nseq.0"),
    "stream_a16_l3_8k": ("lit.treeless.sf0", "lit.treeless.sf1"),
    "stream_a16_l3_20k": ("lit.compressed.sf3",),
    "stream_a16_l19_2k": ("ml.repeat", "of.repeat", "lit.treeless.sf1"),
    "stream_a16_l1_200": ("lit.compressed.streams1", "lit.treeless.streams1", "nseq.0"),
    "stream_text_l19_2k": ("ll.repeat", "of.repeat", "ml.repeat"),
}


def _meta_of(seg: bytes) -> bytes:
    meta_off, = struct.unpack_from("<Q", seg, len(seg) - 25)
    return seg[meta_off:len(seg) - 25]


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """Blocks whose zstd decode fails, or whose descriptor breaks Go's slice."""
    rows = _rows(11, 300)
    seg, _, _ = Z.zstd_segment(rows, 3584, 4096, level=3)
    from oracle import pyoracle as P
    md = P.bytes_to_metadata(_meta_of(seg))
    d0 = md.entries[0]
    base = list(d0.desc())
    b = bytearray(seg)
    b[d0.Offset + d0.CompressedSize // 2] ^= 0x5A  # payload corruption
    trunc = list(base)
    trunc[3] = base[3] - 7  # truncated frame
    big = list(base)
    big[3] = base[1] + 1  # CompressedSize > BlockSize: slice bounds panic
    empty = list(base)
    empty[2], empty[3] = 0, 0  # no frames, nothing to read
    empty_rows = list(base)
    empty_rows[3] = 0  # no frames, OriginalSize > 0: mustReadBytes panic
    out = [("payload_flip", bytes(b), [tuple(base)]),
           ("truncated", seg, [tuple(trunc)]),
           ("csize_gt_bsize", seg, [tuple(big)]),
           ("empty_ok", seg, [tuple(empty)]),
           ("empty_panics", seg, [tuple(empty_rows)])]
    # hand-made frames, each one thing away from a frame that decodes
    for name, fr, orig in handmade_rejects():
        out.append((name, *_frames_segment([(fr, orig)])))
    return out


# ---- hand-made frames (RFC 8878 3.1) ----------------------------------------

def frame(blocks, fcs=None, single=False, wlog=20):
    """A zstd frame around `blocks` (already encoded block bytes): optional
    8-byte Frame_Content_Size; a Window_Descriptor of 2^wlog unless single."""
    fhd = (0x20 if single else 0) | ((3 << 6) if fcs is not None else 0)
    hdr = bytes([fhd])
    if not single:
        hdr += bytes([(wlog - 10) << 3])
    if fcs is not None:
        hdr += struct.pack("<Q", fcs)
    return struct.pack("<I", 0xFD2FB528) + hdr + b"".join(blocks)


def _bh(last, btype, size):
    return struct.pack("<I", last | (btype << 1) | (size << 3))[:3]


def rle_block(size, byte=0, last=1):
    return _bh(last, 1, size) + bytes([byte])


def raw_block(data, last=1):
    return _bh(last, 0, len(data)) + bytes(data)


def long_match_block(nseq, lits=b"\0" * 16, mlx=0xFFFF, last=1):
    """A compressed block of `nseq` sequences, each 8 literals + one match of
    ML code 52 (65 539 + mlx bytes) at offset 5, all three symbol tables in
    RLE_Mode, literals raw: the block's output is 8 + nseq * (8 + 65 539 + mlx)
    bytes from a few bytes of input."""
    body = bytes([(len(lits) << 3) | 0]) + bytes(lits)  # Raw_Literals_Block, 1-byte header
    body += bytes([nseq]) + bytes([(1 << 6) | (1 << 4) | (1 << 2)]) + bytes([8, 3, 52])
    acc, n = 0, 0
    for _ in range(nseq):  # written low to high = read last to first
        for v, nb in ((0, 0), (mlx, 16), (0, 3)):  # LL extra, ML extra, OF extra (ofv 8)
            acc |= (v & ((1 << nb) - 1)) << n
            n += nb
    acc |= 1 << n
    body += acc.to_bytes((n + 8) // 8, "little")
    return _bh(last, 2, len(body)) + body


def _frames_segment(frames_origs):
    """A zstd segment whose blocks hold the given frame bytes with the given
    OriginalSize each (padded to 4 KiB multiples as the writer pads, Q2)."""
    from oracle import pyoracle as P
    seg, index = bytearray(), []
    for i, (fr, orig) in enumerate(frames_origs):
        padded = fr + bytes(4096 - len(fr) % 4096)
        st = P.BlockStat(b"b%04d" % i, len(seg), len(padded), orig, len(fr))
        st.Hash = P.xxh64(padded)
        index.append(st)
        seg += padded
    meta = bytearray()
    fk, lk = index[0].FirstKey, index[-1].FirstKey
    meta += struct.pack("<H", len(fk)) + fk + struct.pack("<H", len(lk)) + lk
    meta += bytes([0, 1, 0]) + struct.pack("<Q", len(index))
    for st in index:
        meta += st.to_bytes()
    meta_off = len(seg)
    seg += meta
    seg += struct.pack("<QQBQ", meta_off, P.xxh64(bytes(meta)), 1, P.MAGIC)
    return bytes(seg), [st.desc() for st in index]


def past_original_cases():
    """Frames that decompress past OriginalSize (Go's io.Copy inflates the
    whole frame set, segment_reader.go:320-330, then walks records to
    OriginalSize, :338-352), OriginalSize values past Go's int() conversion
    (:340), and Block_Maximum_Size / window violations (RFC 8878 3.1.1.2.4).
    [(name, segment, descs, expected statuses or None, needs the regrow)]"""
    rows = _rows(31, 60)
    rawb = b"".join(struct.pack("<HI", len(k), len(v)) + k + v for k, v in rows)
    tail = bytes(range(256)) * 1200  # 300 KiB after the records
    big = Z.compress(rawb + tail, 3)
    half = len(rawb) // 2
    out = []
    out.append(("inflate_past_orig", *_frames_segment([(big, len(rawb))]), [0], True))
    # OriginalSize inside a record: the record is decoded from bytes past it (Q5)
    out.append(("orig_inside_record", *_frames_segment([(big, half)]), [0], True))
    out.append(("orig_zero", *_frames_segment([(big, 0)]), [0], True))
    out.append(("orig_2^63", *_frames_segment([(big, 1 << 63)]), [0], False))
    out.append(("orig_2^64-1", *_frames_segment([(Z.compress(rawb, 1), (1 << 64) - 1)]), [0], False))
    # the frame ends before OriginalSize: mustReadBytes panics
    out.append(("orig_2^40_short_frame", *_frames_segment([(Z.compress(rawb, 1), 1 << 40)]), [3],
                False))
    # 10 RLE blocks of 128 KiB (Block_Maximum_Size exactly): 1.25 MiB of zero
    # records (klen 0, vlen 0) from 44 bytes of frame
    rle10 = frame([rle_block(128 << 10, 0, last=0) for _ in range(9)] + [rle_block(128 << 10)])
    out.append(("rle_10x128k", *_frames_segment([(rle10, 600)]), [0], True))
    # two compressed blocks of exactly 128 KiB each (16 literals + one match of
    # 131 056 bytes): at the limit
    ok2 = frame([long_match_block(1, mlx=0xFFFF - 18, last=0), long_match_block(1, mlx=0xFFFF - 18)])
    out.append(("long_matches_2_blocks", *_frames_segment([(ok2, 64)]), [0], True))
    # Block_Maximum_Size violations: each is a decode error
    out.append(("rle_128k_plus_1", *_frames_segment([(frame([rle_block((128 << 10) + 1)]), 60)]),
                [6], False))
    out.append(("raw_129k", *_frames_segment([(frame([raw_block(bytes(129 << 10))]), 60)]),
                [6], False))
    out.append(("match_block_over_128k", *_frames_segment([(frame([long_match_block(2)]), 60)]),
                [6], False))
    out.append(("rle_2k_window_1k", *_frames_segment([(frame([rle_block(2048)], wlog=10), 60)]),
                [6], False))
    out.append(("window_log_41", *_frames_segment([(frame([rle_block(1024)], wlog=41), 60)]),
                [6], False))
    # several blocks in one segment: regrown, failing and plain blocks together
    mix = [(big, len(rawb)), (Z.compress(rawb, 1), len(rawb)), (rle10, 6000),
           (frame([rle_block((128 << 10) + 1)]), 60), (big, 100)]
    out.append(("mixed", *_frames_segment(mix), [0, 0, 0, 6, 0], True))
    return out


# ---- frame writer (RFC 8878), for what libzstd's compressor never emits -----
# Sequences through Predefined_Mode / RLE_Mode / Repeat_Mode tables, literals
# raw, RLE, Huffman with direct weights (1 or 4 streams) and treeless, any frame
# header; with a model that executes the sequences (3.1.1.5's repeat offsets).

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                             4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# default distributions (3.1.1.3.2.2) with their accuracy logs
LL_DEFAULT = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1,
               1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEFAULT = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEFAULT = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)


def fse_decode_table(dist, al):
    """4.1.1: [(symbol, number of bits, baseline)] per state."""
    size = 1 << al
    assert sum(abs(p) for p in dist) == size
    sym = [None] * size
    high = size - 1
    for s, p in enumerate(dist):  # "less than 1" symbols take the last states
        if p == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, p in enumerate(dist):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [abs(p) for p in dist]
    table = []
    for s in sym:
        x = nxt[s]
        nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


_PREDEF = {}


def _table(kind, mode, sym=None):
    """(decode table, accuracy log) of a symbol kind in Predefined or RLE mode."""
    if mode == "r":
        return [(sym, 0, 0)], 0
    if kind not in _PREDEF:
        dist, al = {"ll": LL_DEFAULT, "of": OF_DEFAULT, "ml": ML_DEFAULT}[kind]
        _PREDEF[kind] = (fse_decode_table(dist, al), al)
    return _PREDEF[kind]


def _code(base, v):
    return bisect.bisect_right(base, v) - 1


def _states(codes, table):
    """One state per sequence, last to first: sequence i's state holds code i
    and its [baseline, baseline + 2^nb) holds sequence i+1's state."""
    by = {}
    for st, (s, _nb, _b) in enumerate(table):
        by.setdefault(s, []).append(st)
    out = [0] * len(codes)
    out[-1] = by[codes[-1]][0]
    for i in range(len(codes) - 2, -1, -1):
        out[i] = next(st for st in by[codes[i]]
                      if table[st][2] <= out[i + 1] < table[st][2] + (1 << table[st][1]))
    return out


def _backward_bits(fields):
    """[(value, nbits)] in the order a decoder reads them -> the bytes of a
    backward bitstream (4.1 / 4.2.2: read from the end, under a final 1 bit)."""
    out, acc, n = bytearray(), 0, 0
    for v, nb in reversed(fields):
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0)
        acc |= v << n
        n += nb
        while n >= 8:
            out.append(acc & 255)
            acc >>= 8
            n -= 8
    out.append(acc | (1 << n))
    return bytes(out)


def seq_bitstream(seqs, tabs):
    """seqs [(ll, ml, offset value)], tabs {"ll"|"of"|"ml": (table, al)} ->
    the sequence section's bitstream (3.1.1.3.2.1.1's read order)."""
    codes = {"ll": [_code(LL_BASE, ll) for ll, _, _ in seqs],
             "ml": [_code(ML_BASE, ml) for _, ml, _ in seqs],
             "of": [ofv.bit_length() - 1 for _, _, ofv in seqs]}
    st = {k: _states(codes[k], tabs[k][0]) for k in codes}
    fields = [(st[k][0], tabs[k][1]) for k in ("ll", "of", "ml")]
    n = len(seqs)
    for i, (ll, ml, ofv) in enumerate(seqs):
        llc, mlc, ofc = codes["ll"][i], codes["ml"][i], codes["of"][i]
        fields.append((ofv - (1 << ofc), ofc))
        fields.append((ml - ML_BASE[mlc], ML_BITS[mlc]))
        fields.append((ll - LL_BASE[llc], LL_BITS[llc]))
        if i < n - 1:
            for k in ("ll", "ml", "of"):
                _s, nb, base = tabs[k][0][st[k][i]]
                fields.append((st[k][i + 1] - base, nb))
    return _backward_bits(fields), codes


def huf_codes(weights):
    """4.2.1: {symbol: (code, nbits)} from every symbol's weight (the last
    nonzero one is the implied one), and Max_Number_of_Bits."""
    total = sum(1 << (w - 1) for w in weights if w)
    mb = total.bit_length() - 1
    assert total == 1 << mb and weights[-1] and mb <= 11
    codes, cur = {}, 0
    for w in range(1, mb + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (cur, mb + 1 - w)
                cur += 1
        assert cur % 2 == 0 or w == mb
        cur >>= 1
    return codes, mb


def huf_tree_direct(weights):
    """Huffman tree description with direct 4-bit weights (header byte >= 128)."""
    w = list(weights[:-1])
    assert 1 <= len(w) <= 128
    w2 = w + [0]
    return bytes([127 + len(w)]) + bytes((w2[i] << 4) | w2[i + 1] for i in range(0, len(w), 2))


def _huf_stream(lits, codes):
    return _backward_bits([codes[b] for b in lits])


def lit_raw(lits, sf=None):
    n = len(lits)
    sf = sf if sf is not None else (0 if n < 32 else 1 if n < 4096 else 3)
    hb, sh = {0: (1, 3), 1: (2, 4), 3: (3, 4)}[sf]
    assert n < 1 << (8 * hb - sh)
    return ((n << sh) | (sf << 2) | 0).to_bytes(hb, "little") + bytes(lits)


def lit_rle(byte, n, sf=None):
    sf = sf if sf is not None else (0 if n < 32 else 1 if n < 4096 else 3)
    hb, sh = {0: (1, 3), 1: (2, 4), 3: (3, 4)}[sf]
    assert n < 1 << (8 * hb - sh)
    return ((n << sh) | (sf << 2) | 1).to_bytes(hb, "little") + bytes([byte])


def lit_huf(lits, weights, streams=1, sf=None, treeless=False, tree=None):
    """Compressed_Literals_Block (or Treeless, reusing `weights` as the tree the
    previous block left) with direct weights; 4 streams split as 4.2.2 says.
    `tree`: other weights to describe than the ones coded with (a reject)."""
    codes, _mb = huf_codes(weights)
    if streams == 1:
        body = _huf_stream(lits, codes)
    else:
        seg = (len(lits) + 3) // 4
        parts = [_huf_stream(lits[i * seg:(i + 1) * seg], codes) for i in range(3)]
        parts.append(_huf_stream(lits[3 * seg:], codes))
        body = struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts)
    if not treeless:
        body = huf_tree_direct(tree or weights) + body
    if sf is None:
        big = max(len(lits), len(body))
        sf = 0 if streams == 1 else (1 if big < 1024 else 2 if big < 16384 else 3)
    assert (sf == 0) == (streams == 1)
    hb, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
    assert len(lits) < 1 << bits and len(body) < 1 << bits
    v = (3 if treeless else 2) | (sf << 2) | (len(lits) << 4) | (len(body) << (4 + bits))
    return v.to_bytes(hb, "little") + body


def _nseq_bytes(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([(n >> 8) + 128, n & 255])
    return bytes([255]) + struct.pack("<H", n - 0x7F00)


def copy_match(out, off, ml, strict=True):
    assert 0 < off <= len(out) or not strict, (off, len(out))
    if off > len(out):  # a reject frame: only the length is modelled
        out += bytes(ml)
        return
    if off >= ml:
        out += out[len(out) - off:len(out) - off + ml]
    else:
        pat = bytes(out[len(out) - off:])
        out += (pat * (ml // off + 1))[:ml]


class FrameWriter:
    """Blocks of one frame, and the bytes they decode to (`out`): the model
    executes each block's sequences as it is written, with the repeat offsets
    (3.1.1.5) and the tables / Huffman tree carried from block to block."""

    def __init__(self):
        self.blocks, self.out = [], bytearray()
        self.rep = [1, 4, 8]
        self.tabs = {}

    def raw(self, data):
        self.blocks.append((0, bytes(data)))
        self.out += data
        return self

    def rle(self, byte, n):
        self.blocks.append((1, bytes([byte]), n))
        self.out += bytes([byte]) * n
        return self

    def compressed(self, lits, lit_section, seqs, modes="ppp", modes_or=0, rle_syms=None,
                   nseq=None, model=True, seq_section=None):
        """`lits`: the literal bytes `lit_section` (lit_raw / lit_rle / lit_huf)
        encodes.  modes: one letter each for LL, OF, ML: p Predefined, r RLE (every
        sequence has that one code), R Repeat_Mode (the previous block's table).
        modes_or / rle_syms / nseq overwrite header fields for the reject cases;
        model=False lets their sequences be impossible ones; seq_section is the
        whole sequences section of a block without sequences, byte by byte."""
        body = bytearray(lit_section)
        body += seq_section or _nseq_bytes(len(seqs) if nseq is None else nseq)
        assert not (seqs and seq_section)
        if seqs:
            codes = {"ll": [_code(LL_BASE, s[0]) for s in seqs],
                     "ml": [_code(ML_BASE, s[1]) for s in seqs],
                     "of": [s[2].bit_length() - 1 for s in seqs]}
            mb, syms = 0, b""
            for k, m, sh in zip(("ll", "of", "ml"), modes, (6, 4, 2)):
                if m == "R":
                    mb |= 3 << sh  # with no table to repeat (a reject): coded as Predefined
                elif m == "r":
                    assert len(set(codes[k])) == 1
                    mb |= 1 << sh
                    self.tabs[k] = _table(k, "r", codes[k][0])
                    syms += bytes([codes[k][0]])
                else:
                    self.tabs[k] = _table(k, "p")
            tabs = {k: self.tabs.get(k) or _table(k, "p") for k in ("ll", "of", "ml")}
            bits, _ = seq_bitstream(seqs, tabs)
            if rle_syms is not None:
                syms = bytes(rle_syms)
            body += bytes([mb | modes_or]) + syms + bits
        self.blocks.append((2, bytes(body)))
        lp = 0
        for ll, ml, ofv in seqs:
            assert lp + ll <= len(lits) or not model
            self.out += lits[lp:lp + ll]
            lp += ll
            r = self.rep
            if ofv > 3:
                off = ofv - 3
                self.rep = [off, r[0], r[1]]
            else:
                idx = ofv - 1 + (ll == 0)
                if idx == 0:
                    off = r[0]
                elif idx == 1:
                    off = r[1]
                    self.rep = [r[1], r[0], r[2]]
                elif idx == 2:
                    off = r[2]
                    self.rep = [r[2], r[0], r[1]]
                else:
                    off = (r[0] - 1) or 1  # libzstd: 0 is forced to 1
                    self.rep = [off, r[0], r[1]]
            copy_match(self.out, off, ml, model)
        self.out += lits[lp:]
        return self

    def block_bytes(self, bad_type_at=None):
        out = []
        for i, b in enumerate(self.blocks):
            last = int(i == len(self.blocks) - 1)
            bt = 3 if bad_type_at == i else b[0]
            out.append(_bh(last, bt, b[2] if b[0] == 1 else len(b[1])) + b[1])
        return out

    def frame(self, **kw):
        return frame2(self.block_bytes(kw.pop("bad_type_at", None)), bytes(self.out), **kw)


def frame2(blocks, content, fcs_bytes=0, fcs_delta=0, single=False, wlog=17, mant=0,
           did_bytes=0, did=0, checksum=False, checksum_xor=0, reserved=0):
    """A frame with any header (3.1.1.1): Frame_Content_Size of 0/1/2/4/8 bytes,
    Single_Segment, a Window_Descriptor of (1 + mant/8) * 2^wlog, a Dictionary_ID
    field of 0/1/2/4 bytes, Content_Checksum.  fcs_delta / checksum_xor / reserved
    make the reject frames."""
    assert fcs_bytes != 1 or single
    fl = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert not (single and fcs_bytes == 0)
    fhd = (fl << 6) | (int(single) << 5) | (reserved << 3) | (int(checksum) << 2) | \
        {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
    hdr = bytes([fhd])
    if not single:
        hdr += bytes([((wlog - 10) << 3) | mant])
    hdr += did.to_bytes(did_bytes, "little")
    if fcs_bytes:
        n = len(content) + fcs_delta - (256 if fcs_bytes == 2 else 0)
        hdr += n.to_bytes(fcs_bytes, "little")
    tail = b""
    if checksum:
        from oracle import pyoracle as P
        tail = struct.pack("<I", (P.xxh64(bytes(content)) & 0xFFFFFFFF) ^ checksum_xor)
    return struct.pack("<I", 0xFD2FB528) + hdr + b"".join(blocks) + tail


# ---- hand-made cases ---------------------------------------------------------
# Every success frame decodes to ONE record that covers its whole output: the
# first six literals are [u16 klen][u32 N - 6 - klen] and OriginalSize = N, so
# the record walk puts every decompressed byte into an arena and the parity
# check compares it.  make(hdr6, pad) builds the frame with `pad` more trailing
# literals; _record() calls it twice, first to learn N.

def _rnd(seed, n, hi=256):
    rng = random.Random(seed)
    return bytes(rng.randrange(hi) for _ in range(n))


def _record(make, klen=2, amax=255):
    """amax < 255: every byte of the record header must be <= amax (a Huffman
    alphabet of amax + 1 symbols): N is padded until vlen's bytes are.
    klen < 0: the value is -klen bytes and the key is the rest."""
    w = make(bytes(6), 0)
    if klen < 0:
        klen = len(w.out) - 6 + klen
    m = len(w.out) - 6 - klen
    v = m
    if amax < 255:
        v = m if (m & 255) <= amax else ((m >> 8) + 1) << 8
        assert (v >> 8) <= amax
    hdr = struct.pack("<HI", klen, v)
    w = make(hdr, v - m)
    assert len(w.out) == 6 + klen + v and bytes(w.out[:6]) == hdr
    return w


# 16 symbols, Max_Number_of_Bits 11: 1024 + 512 + ... + 8 + 8 * 1 = 2048
W16 = [11, 10, 9, 8, 7, 6, 5, 4, 1, 1, 1, 1, 1, 1, 1, 1]
W_0_2 = [1, 0, 1]  # symbols 0 and 2, one bit each
W_0_2_3 = [2, 0, 1, 1]  # symbols 0, 2, 3


def _simple(n, lit=lit_raw, modes="ppp", seqs=None, hi=256, **kw):
    """make() of a plain one-block frame of n bytes: 20 literals, one match."""
    def make(hdr, pad):
        lits = hdr + _rnd(n, 14 + pad, hi)
        s = seqs or [(16, n - 20, 3 + 11)]
        return FrameWriter().compressed(lits, lit(lits), s, modes, **kw)
    return make


def _mixed_seqs(seed, n):
    """n short sequences: real offsets 1..8 and repeat codes (never value 3 after
    no literals, whose rep0 - 1 may reach 0), after one that opens with 8 literals."""
    rng = random.Random(seed)
    seqs = [(8, 4, 3 + 5)]
    while len(seqs) < n:
        ll = rng.choice((0, 0, 1, 1, 2, 3, 5))
        ofv = rng.choice((1, 2, 3, 4, 5, 6, 8, 9, 10, 11))
        if ofv == 3 and ll == 0:
            ofv = 2
        seqs.append((ll, rng.randrange(3, 11), ofv))
    return seqs


def _seq_frame(seqs, seed, modes="ppp", tail=5):
    def make(hdr, pad):
        need = sum(s[0] for s in seqs) + tail + pad
        lits = hdr + _rnd(seed, need - 6)
        return FrameWriter().compressed(lits, lit_raw(lits), seqs, modes)
    return _record(make)


def _repeat_matrix_seqs():
    rng = random.Random(77)
    seqs = [(130, 5, 3 + 120), (4, 6, 3 + 90), (3, 7, 3 + 70)]
    # (offset value 1, 2, 3) x (ll > 0, ll == 0)
    seqs += [(2, 4, 1), (0, 4, 1), (2, 4, 2), (0, 4, 2), (2, 4, 3), (0, 4, 3)]
    run = lambda: [(rng.choice((0, 0, 1, 2)), rng.randrange(3, 7), rng.choice((1, 2, 3)))
                   for _ in range(75)]
    return seqs + run() + [(5, 9, 3 + 57)] + run()


def _two_block(variant):
    """Block 2 repeats all three tables and the Huffman tree of block 1, and its
    first sequence is offset value 1 after literals: block 1's last rep0."""
    def make(hdr, pad):
        w = FrameWriter()
        if variant == "predefined":
            l1 = hdr + _rnd(1, 94, 16)
            w.compressed(l1, lit_huf(l1, W16), [(40, 10, 3 + 30), (30, 8, 3 + 12), (20, 9, 3 + 25)])
            l2 = _rnd(2, 40 + pad, 16)
            s2 = [(5, 12, 1), (0, 7, 3), (10, 9, 3 + len(w.out) + 5 + 12 + 7 + 10), (6, 5, 2)]
            w.compressed(l2, lit_huf(l2, W16, treeless=True), s2, "RRR")
        else:  # LL and ML in RLE_Mode (codes 16 and 32), 4 Huffman streams
            l1 = hdr + _rnd(3, 60, 16)
            w.compressed(l1, lit_huf(l1, W16, streams=4),
                         [(16, 35, 3 + 9), (17, 36, 3 + 20), (16, 36, 2)], "rpr")
            l2 = _rnd(4, 60 + pad, 16)
            s2 = [(17, 35, 1), (16, 36, 3 + len(w.out) + 17 + 35 + 16), (16, 35, 3)]
            w.compressed(l2, lit_huf(l2, W16, streams=4, treeless=True), s2, "RRR")
        return w
    return _record(make, amax=15)


def _huf4_tiny(regen):
    """4 Huffman streams of (regen + 3) / 4 symbols each and the rest in the last:
    regen 6 leaves the last stream empty, regen 5 would need 3 * 2 > 5."""
    if regen >= 6:  # one block: the six header literals, the record's body by a match
        w = FrameWriter()
        lits = struct.pack("<HI", 2, 3) + bytes([3])[:regen - 6]
        w.compressed(lits, lit_huf(lits, W_0_2_3, streams=4, sf=1), [(regen, 11 - regen, 3 + 2)])
    else:  # a raw block ahead holds the record header
        n = 12 + regen + 4
        w = FrameWriter().raw(struct.pack("<HI", 2, n - 8) + _rnd(regen, 6))
        lits = bytes([0, 2, 3, 0, 2])[:regen]
        w.compressed(lits, lit_huf(lits, W_0_2_3, streams=4, sf=1), [(regen, 4, 3 + 9)])
    return w


def _ll35(ll):
    """ll literals (LL code 35) and a match of 3.  The literals are Huffman
    coded, about a bit each (raw they would make Block_Size itself pass 128 KiB),
    so the record header's bytes must be symbols <= 128: vlen 0x1807F, klen 0x7Fxx."""
    def make(hdr, pad):
        w5 = [0] * 129
        for s, w in zip((0, 1, hdr[0] or 2, 0x7F, 0x80), (4, 3, 2, 1, 1)):
            w5[s] = w
        rng = random.Random(ll)
        body = bytes(rng.choice((0, 0, 0, 0, 0, 0, 1, 1, 0x7F, 0x80)) for _ in range(ll - 6))
        lits = hdr + body
        return FrameWriter().compressed(lits, lit_huf(lits, w5, streams=4), [(ll, 3, 3 + 5)])
    return _record(make, klen=-0x1807F)


@functools.lru_cache(maxsize=None)
def handmade_frames():
    """[(group, name, frame bytes, the bytes it decodes to, one block?)]: the
    success frames.  A CPU test holds model == libzstd == both oracles' rows."""
    out = []

    def add(group, name, w, **hdr):
        out.append((group, name, w.frame(**hdr), bytes(w.out), len(w.blocks) == 1))

    # RLE literals.  One block: every literal is the same byte, the record header
    # too, so the byte is 0 and the output is N / 6 empty records -- any wrong byte
    # or length changes the walk.  Two blocks (a raw block holds the header): byte A7.
    z = bytes(5004)
    add("rle_literals", "seqs", FrameWriter().compressed(
        z[:300], lit_rle(0, 300), [(100, 50, 3 + 7), (200, 46, 2)]))
    add("rle_literals", "nseq0", FrameWriter().compressed(z, lit_rle(0, 5004), []))
    add("rle_literals", "tail", FrameWriter().compressed(z[:24], lit_rle(0, 24), [(6, 12, 3 + 6)]))
    for name, n, seqs in (("seqs2", 300, [(100, 50, 3 + 7), (200, 46, 2)]), ("nseq0_2", 5000, []),
                          ("tail2", 24, [(6, 12, 3 + 30)])):
        def make(hdr, pad, n=n, seqs=seqs):
            w = FrameWriter().raw(hdr + _rnd(n, 24))
            return w.compressed(b"\xA7" * (n + pad), lit_rle(0xA7, n + pad), seqs)
        add("rle_literals", name, _record(make))

    # Huffman literals with direct weights
    def two_sym(hdr, pad):
        lits = hdr + bytes(2 * (b & 1) for b in _rnd(5, 34 + pad))
        return FrameWriter().compressed(lits, lit_huf(lits, W_0_2), [(40, 480, 3 + 7)])
    add("huf_direct", "2_symbols", _record(two_sym, amax=2))

    def sixteen(hdr, pad):
        lits = hdr + bytes(range(16)) + _rnd(6, 178 + pad, 16)
        return FrameWriter().compressed(lits, lit_huf(lits, W16),
                                        [(100, 300, 3 + 50), (90, 278, 3 + 3)])
    add("huf_direct", "16_symbols_11_bits", _record(sixteen, amax=15))

    def sixteen4(hdr, pad):
        lits = hdr + _rnd(7, 1500 + pad, 16)
        return FrameWriter().compressed(lits, lit_huf(lits, W16, streams=4, sf=3),
                                        [(700, 300, 3 + 650), (701, 99, 1)])
    add("huf_direct", "4_streams_sf3", _record(sixteen4, amax=15))
    for regen in (4, 6, 7):
        add("huf_direct", f"4_streams_regen_{regen}", _huf4_tiny(regen))

    # sequence counts at the header's and the executor's edges
    for n in (127, 128, 129, 255, 256, 257):
        add("nseq_small", f"nseq_{n}", _seq_frame(_mixed_seqs(n, n), n))
    for n in (0x7EFF, 0x7F00, 0x7F00 + 100):
        rng = random.Random(n)
        seqs = [(8, 3, 4 + rng.randrange(4))] + [(1, 3, 4 + rng.randrange(4)) for _ in range(n - 1)]
        # LL Predefined (the first sequence takes the record header: 8 literals),
        # OF code 2 and ML code 0 in RLE_Mode
        add("nseq_3byte", f"nseq_{n:#x}", _seq_frame(seqs, n, "prr"))

    # repeat offsets
    add("repeat_offsets", "matrix_and_runs", _seq_frame(_repeat_matrix_seqs(), 8, tail=7))
    add("repeat_offsets", "rep0_minus_1_is_0", _seq_frame([(16, 5, 3 + 1), (0, 5, 3), (2, 4, 1)], 9))
    add("offsets", "to_frame_start", _seq_frame([(20, 10, 3 + 20), (5, 8, 3 + 35), (0, 6, 3 + 43)], 10))
    add("offsets", "overlap_1_2_3_7_8", _seq_frame(
        [(12, 40, 3 + 1), (2, 40, 3 + 2), (1, 41, 3 + 3), (3, 50, 3 + 7), (2, 50, 3 + 8)], 11, tail=3))

    # the longest codes, as far as Block_Maximum_Size lets their extra bits go:
    # 128 KiB = 131 069 literals (65 536 + FFFD) + 3, or 8 + 131 064 (65 539 + FFF5)
    add("long_codes", "ll_code_35", _ll35(131069))
    add("long_codes", "ml_code_52", _seq_frame([(8, 131064, 3 + 3)], 13, tail=0))

    # Number_of_Sequences 0 written in two bytes (80 00): libzstd still reads the
    # modes byte and the tables, runs nothing, and does not look at what follows
    for name, sec in (("predefined", b"\x80\x00\x00"), ("bytes_after", b"\x80\x00\x00\x55\x66"),
                      ("rle_tables", b"\x80\x00\x54\x23\x1f\x34")):
        def make(hdr, pad, sec=sec):
            lits = hdr + _rnd(15, 40 + pad)
            return FrameWriter().compressed(lits, lit_raw(lits), [], seq_section=sec)
        add("nseq_0_two_bytes", name, _record(make))

    add("two_blocks", "repeat_after_predefined", _two_block("predefined"))
    add("two_blocks", "repeat_after_rle", _two_block("rle"))

    # frame headers
    add("frame_headers", "fcs_1_byte", _record(_simple(100)), fcs_bytes=1, single=True)
    add("frame_headers", "fcs_2_bytes_256", _record(_simple(256)), fcs_bytes=2, checksum=True)
    add("frame_headers", "fcs_2_bytes_65791", _record(_simple(65791)), fcs_bytes=2, single=True)
    add("frame_headers", "fcs_8_bytes", _record(_simple(300)), fcs_bytes=8, checksum=True)
    add("frame_headers", "window_mantissa_7", _record(_simple(400)), mant=7, wlog=12)
    for nb in (1, 2, 4):
        add("frame_headers", f"dictid_{nb}_bytes_0", _record(_simple(277 + nb)), did_bytes=nb,
            fcs_bytes=nb * 2)
    return out


@functools.lru_cache(maxsize=None)
def flipped_handmade(per_frame=10):
    """(segment, descs): every hand-made success frame of under 4 KiB, `per_frame`
    times with one bit flipped -- half of the flips in the 12 bytes after the
    magic number (frame, block, literals and sequences headers of the small ones),
    half anywhere.  The random-flip tests over libzstd's frames reach the arms
    those frames never take only here."""
    rng = random.Random(41)
    blocks = []
    for _g, _n, fr, want, _one in handmade_frames():
        if len(fr) >= 4096:
            continue
        for v in range(per_frame):
            b = bytearray(fr)
            at = rng.randrange(4, min(16, len(b))) if v % 2 == 0 else rng.randrange(4, len(b))
            b[at] ^= 1 << rng.randrange(8)
            blocks.append((bytes(b), len(want)))
    return _frames_segment(blocks)


def handmade_rejects():
    """[(name, frame, OriginalSize)]: each one thing away from a success frame."""
    out = []
    N = 300

    def add(name, w, **hdr):
        out.append((name, w.frame(**hdr), len(w.out)))

    ok = lambda **kw: _record(_simple(N, **kw))
    add("frame_reserved_bit", ok(), reserved=1)
    add("block_type_3", ok(), bad_type_at=0)
    add("dictid_1", ok(), did_bytes=1, did=1)
    add("fcs_one_more", ok(), fcs_bytes=2, fcs_delta=1)
    add("fcs_one_less", ok(), fcs_bytes=2, fcs_delta=-1)
    add("checksum_bit", ok(), checksum=True, checksum_xor=1 << 9)
    for m in ("Rpp", "pRp", "ppR"):
        add(f"repeat_mode_first_block_{m}", ok(modes=m))
    add("treeless_first_block",
        _record(_simple(N, lit=lambda l: lit_huf(l, W16, treeless=True), hi=16), amax=15))
    add("modes_reserved_bit", ok(modes_or=1))
    add("rle_ll_symbol_36", ok(modes="rpp", rle_syms=[36]))
    add("rle_of_symbol_32", ok(modes="prp", rle_syms=[32]))
    add("rle_ml_symbol_53", ok(modes="ppr", rle_syms=[53]))
    add("offset_past_frame_start", ok(seqs=[(16, N - 20, 3 + 17)], model=False))
    add("ll_past_literals", ok(seqs=[(30, N - 20, 3 + 11)], model=False))
    bad = list(W16)
    bad[9] = 3  # 2047 - 1 + 4: what is left to the next power of two is no power of two
    add("huf_weights_no_power_of_2",
        _record(_simple(N, lit=lambda l: lit_huf(l, W16, tree=bad), hi=16), amax=15))

    # no sequences: the section is the one byte 0; in two bytes, modes and tables count
    for name, sec in (("nseq_0_then_a_byte", b"\x00\x00"), ("nseq_0_two_bytes_no_modes", b"\x80\x00"),
                      ("nseq_0_two_bytes_repeat_mode", b"\x80\x00\xfc"),
                      ("nseq_0_two_bytes_rle_symbol_64", b"\x80\x00\x54\x40\x02\x03"),
                      ("nseq_0_two_bytes_reserved_bit", b"\x80\x00\x02")):
        def make(hdr, pad, sec=sec):
            lits = hdr + _rnd(16, 40 + pad)
            return FrameWriter().compressed(lits, lit_raw(lits), [], seq_section=sec)
        add(name, _record(make))
    w = _huf4_tiny(5)  # streams 1-3 hold 2 symbols each, more than the 5 there are
    out.append(("huf_4_streams_regen_5", w.frame(), len(w.out)))
    w = _ll35(131071)  # LL code 35 with all 16 extra bits: 131 071 + 3 > 128 KiB
    out.append(("ll_code_35_all_bits_over_block_max", w.frame(), len(w.out)))
    return out
