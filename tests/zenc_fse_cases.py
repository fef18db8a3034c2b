"""Row sets for the FSE-compressed Huffman weights of the device zstd encoder
(OKV_F_ZSTD_HUF_FSE): the fixtures tests/test_zstd_fse_host.py asserts from the model's census
(tests/zenc_fse_model.py) on the CPU and tests/test_zstd_fse_gpu.py encodes on the device.  No
GPU, no device output.

A fixture is one row, so one raw block, as in tests/zenc_huf_cases.py (lit_row, plain, top).
Where a unit's literals have to be exact, record header included, they are the block's SECOND
unit: the first is 32 KiB of bytes without a match (plain), the second starts at byte 32 768
of the block and holds nothing but what the fixture says (behind, a unit sees no earlier one).
Seeds and sizes found by search are committed as they were found."""
from __future__ import annotations

import random

from tests import zenc_cases as ZC
from tests import zenc_huf_cases as HC
from tests.zenc_model import UNIT

plain, top, lit_row = HC.plain, HC.top, HC.lit_row


def row_below(body, limit):
    """lit_row with every header byte at most `limit`."""
    n = len(body)
    for klen in range(1, min(limit, n - 6) + 1):
        vlen = n - 6 - klen
        if all(b <= limit for b in vlen.to_bytes(4, "little")):
            return (bytes(body[6:6 + klen]), bytes(body[6 + klen:]))
    raise AssertionError(f"no header for {n} bytes below {limit}")


def second_unit(body):
    """One row of two units; the second unit is `body`."""
    return ZC.block(plain(UNIT) + bytes(body))


def skewed(seed, n, k, last):
    """n bytes over the k values up to `last`, the low ones much more frequent."""
    rng = random.Random(seed)
    syms = list(range(last - k + 1, last + 1))
    return bytes(syms[min(k - 1, int(rng.expovariate(0.45)))] for _ in range(n))


# FSE - direct description bytes: (seed, last, n, k) of skewed(), by search
TIE = {-1: (2, 11, 22, 4), 0: (1, 11, 22, 4), 1: (1, 11, 277, 4)}

# The binary de Bruijn sequence B(2, 4) and its first three bits again: every 4-bit window
# once, so 19 bytes of two values hold no match.
B24 = [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 0, 0]


def equal_weights():
    """272 literals: the values 0 .. 191 once each and 80 times the value 192, two small ones
    between the large: no 4-byte window repeats.  The only optimal code gives the 192 small
    values 8 bits and the large one 2 (3 * 64 / 256 + 1 / 4 = 1; moving a small value up costs
    two others a bit), so all 192 listed weights are 1."""
    out = []
    for v in range(192):
        out.append(v)
        if v % 2 == 1 and v < 160:
            out.append(192)
    assert len(out) == 272
    return bytes(out)


def _c(us, i=0):
    return us[i].census


def _fse_unit(c, nlit=None, log=None):
    assert c["block"] == 2 and c["lit"] == 2 and c["desc"] == 1, c
    assert 0 < c["dbytes"] == c["dfse"] <= 128 and 0 < c["huf"] < c["raw"], c
    assert c["ddir"] == 0 or c["dfse"] < c["ddir"], c
    assert (c["ddir"] == 0) == (c["last"] > 128), c
    assert c["alog"] == (6 if c["last"] >= 128 else 5), c
    if nlit is not None:
        assert c["nlit"] == nlit, c
    if log is not None:
        assert c["alog"] == log, c


def _direct_unit(c):
    assert c["block"] == 2 and c["lit"] == 2 and c["desc"] == 0, c
    assert 0 < c["dbytes"] == c["ddir"] and c["last"] <= 128, c
    assert c["dfse"] == 0 or c["dfse"] >= c["ddir"], c


def fixtures():
    """[(name, rows, condition over the units of the block in order)]."""
    out = []

    def largest_129(us):  # raw under OKV_F_ZSTD_HUFFMAN alone; the direct form cannot list 129
        c = _c(us)
        _fse_unit(c, 3000, 6)
        assert c["last"] == 129 and c["nseq"] == 0
    out.append(("largest_129", [lit_row(plain(3000, top(129)))], largest_129))

    def all_256(us):  # 255 listed weights
        c = _c(us)
        _fse_unit(c, None, 6)
        assert c["last"] == 255 and c["bits"] >= 9
    rng = random.Random(3)
    body = bytes(min(255, int(rng.expovariate(0.03))) for _ in range(12000)) + bytes(range(256))
    out.append(("all_256", [ZC.block(body)], all_256))

    def only_00_ff(us):  # 254 weights 0 and one weight 1: the low-probability symbol is 1 of 255
        c = _c(us, 1)
        _fse_unit(c, 19, 6)
        assert c["last"] == 255 and c["bits"] == 1 and c["nseq"] == 0 and c["n"] == 19
    out.append(("only_00_ff", [second_unit(bytes(255 * b for b in B24))], only_00_ff))

    for value in (101, 100):  # an odd and an even number of listed weights, accuracy log 5
        def listed(us, value=value):
            c = _c(us)
            _fse_unit(c, 839, 5)
            assert c["last"] == value
        out.append((f"listed_{value}", [lit_row(plain(839, top(value)))], listed))
    for value in (128, 127):  # the accuracy log changes at 128 listed weights
        def log_edge(us, value=value):
            c = _c(us)
            _fse_unit(c, 3000, 6 if value == 128 else 5)
            assert c["last"] == value and c["ddir"] == 1 + (value + 1) // 2
        out.append((f"listed_{value}", [row_below(plain(3000, top(value)), value)], log_edge))

    def all_equal(us):  # no FSE description of one value, no direct one above 128: raw
        c = _c(us, 1)
        assert c["n"] == c["nlit"] == 272 and c["nseq"] == 0, c
        assert c["last"] == 192 and c["dfse"] == c["ddir"] == c["dbytes"] == 0, c
        assert c["bits"] == 0 and c["huf"] == 0 and c["lit"] == 0 and c["block"] == 0, c
    out.append(("all_weights_equal_above_128", [second_unit(equal_weights())], all_equal))

    def direct_smaller(us):  # six listed weights: 4 bytes direct, the FSE form is larger
        c = _c(us)
        _direct_unit(c)
        assert c["dfse"] > c["ddir"] and c["last"] == 6, c
    out.append(("direct_smaller", [row_below(skewed(4, 300 - 34, 4, 6), 6)], direct_smaller))
    for d, (seed, last, n, k) in TIE.items():  # FSE only when strictly smaller
        def tie(us, d=d):
            c = _c(us)
            assert c["dfse"] and c["ddir"] and c["dfse"] - c["ddir"] == d and c["lit"] == 2, c
            (_fse_unit if d < 0 else _direct_unit)(c)
        out.append((f"tie_{d:+d}", [row_below(skewed(seed, n, k, last), last)], tie))

    for nlit in (1023, 1024):  # one stream and four, Size_Formats 00 and 10
        def streams(us, nlit=nlit):
            c = _c(us)
            _fse_unit(c, nlit)
            assert (c["streams"], c["sf"]) == ((1, 0) if nlit == 1023 else (4, 2)) and c["last"] == 200
        out.append((f"nlit_{nlit}", [lit_row(plain(nlit, top(200)))], streams))

    def with_sequences(us):
        c = _c(us)
        _fse_unit(c)
        assert c["nseq"] >= 100 and c["streams"] == 4 and c["last"] == 240, c
    body = bytearray(plain(20000, top(240)))
    for k in range(150):  # a copy of 30 earlier bytes every 100
        at = 5000 + 100 * k
        body[at:at + 30] = body[at - 4000:at - 3970]
    out.append(("with_sequences", [lit_row(bytes(body))], with_sequences))

    def three_units(us):  # FSE, direct, raw in one frame
        assert len(us) == 3
        _fse_unit(_c(us, 0))
        _direct_unit(_c(us, 1))
        c = _c(us, 2)
        assert c["block"] == 0 and c["lit"] == 0 and c["last"] == 255 and c["huf"] >= c["raw"], c
    chunk = skewed(4, 300, 4, 6)
    rng = random.Random(12)
    body = plain(UNIT, top(200)) + (chunk * (UNIT // len(chunk) + 1))[:UNIT] + rng.randbytes(9000)
    out.append(("fse_direct_raw", [ZC.block(body)], three_units))
    return out


def extra():
    """Row sets of the GPU test beyond the fixtures."""
    rng = random.Random(5)
    utf8 = [("schlüssel%05d" % i).encode() for i in range(700)]
    return [("text_46", ZC.text_rows(46)),
            ("utf8_rows", [(k, ("größe %d · straße №%d" % (i, i * 7)).encode())
                           for i, k in enumerate(utf8)]),
            ("binary_rows", [(i.to_bytes(16, "big"), bytes((i * 7 + j) & 255 for j in range(64)))
                             for i in range(600)]),
            ("two_values", [(b"t", bytes(rng.choice(b"\x00\x00\x00\xff") for _ in range(3000)))]),
            ("seven_bytes", [(b"k", b"")]),
            ("random_bytes", [(b"r", rng.randbytes(9000))])]
