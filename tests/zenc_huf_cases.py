"""Row sets for the Huffman literals of the device zstd encoder (OKV_F_ZSTD_HUFFMAN): the
fixtures tests/test_zstd_huf_host.py asserts from the model's census (tests/zenc_huf_model.py)
on the CPU and tests/test_zstd_huf_gpu.py encodes on the device.  No GPU, no device output.

A fixture is one row, so one raw block: u16 key length, u32 value length, key, value.  To
say exactly which literals a unit has, a fixture states the whole block `body`; its first six
bytes become the record header and the key is the body's own bytes behind them (lit_row), with
a key length at which every header byte is at most 128.

Bytes without a match: a prefix of the de Bruijn sequence B(16, 4) holds every 4-byte window
at most once, so the parse finds no sequence in it and the unit's literals are the unit; the
sixteen symbols are mapped to chosen byte values.  The prefix is skewed towards the low
symbols, so the code lengths differ."""
from __future__ import annotations

import random

from tests import zenc_cases as ZC
from tests.zenc_model import UNIT


def de_bruijn(k, n):
    """B(k, n) as a list of symbols 0 .. k-1 (the concatenation of Lyndon words)."""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return out


_DB = []
LOW = list(range(0x20, 0x30))  # the default sixteen byte values


def plain(n, syms=LOW):
    """n bytes in which no 4-byte window repeats, over the byte values `syms`."""
    if not _DB:
        _DB.append(de_bruijn(16, 4))
    assert n <= len(_DB[0]) and len(syms) == 16
    return bytes(syms[s] for s in _DB[0][:n])


def lit_row(body):
    """One row whose record is `body` but for its first six bytes, every header byte <= 128."""
    n = len(body)
    for klen in range(1, 129):
        vlen = n - 6 - klen
        if vlen >= 0 and all(b <= 0x80 for b in vlen.to_bytes(4, "little")):
            return (bytes(body[6:6 + klen]), bytes(body[6 + klen:]))
    raise AssertionError(f"no header for {n} bytes")


def top(value):
    """The sixteen byte values with `value` the largest."""
    return list(range(value - 15, value + 1))


# ---- fixtures: name -> rows; CONDITIONS: name -> condition over the units of the block ----
NLIT = [1023, 1024, 16383, 16384, 32768]
MOD4 = [2000, 2001, 2002, 2003]
EDGE = {-1: (1, 122), 0: (1, 120), 1: (1, 118)}  # Huffman - raw section bytes: (seed, n), by search


def edge_body(seed, n):
    """n letters and their first 40 again: one long match, so the block is Compressed with
    either kind of literals."""
    rng = random.Random(seed)
    base = bytes(rng.choice(b"  eettaoinshr") for _ in range(n))
    return base + base[:40]


def _form(nlit):
    return (1, 0) if nlit <= 1023 else (4, 2) if nlit <= 16383 else (4, 3)


def _huffman_unit(u, nlit, nseq=None):
    c = u.census
    assert c["nlit"] == nlit and c["block"] == 2 and c["lit"] == 2, c
    assert (c["streams"], c["sf"]) == _form(nlit), c
    assert 0 < c["huf"] < c["raw"] and 2 <= c["bits"] <= 11, c
    if nseq is not None:
        assert c["nseq"] == nseq, c


def _raw_literals(u):
    c = u.census
    assert c["lit"] == 0 and c["streams"] == 0, c


def fixtures():
    """[(name, rows, condition over the units of all blocks in order)]."""
    out = []
    for nlit in NLIT:  # the three header forms, one stream and four; no sequence at all
        out.append((f"nlit_{nlit}", [lit_row(plain(nlit))],
                    lambda us, nlit=nlit: _huffman_unit(us[0], nlit, 0)))
    for n in MOD4:  # the last of four streams takes n - 3 * ceil(n / 4) literals
        out.append((f"mod4_{n % 4}", [lit_row(plain(n))],
                    lambda us, n=n: _huffman_unit(us[0], n, 0)))

    def largest(us, value, huf):
        c = us[0].census
        if huf:
            _huffman_unit(us[0], 3000, 0)
            assert c["last"] == value
        else:  # a literal above 128: not eligible, the unit as without the flag
            _raw_literals(us[0])
            assert c["huf"] == 0 and c["bits"] == 0 and c["block"] == 0
    out.append(("largest_128", [lit_row(plain(3000, top(128)))], lambda us: largest(us, 128, True)))
    out.append(("largest_129", [lit_row(plain(3000, top(129)))], lambda us: largest(us, 129, False)))
    # the number of listed weights is the largest value: 128 above, 101 and 100 here
    for value in (101, 100):
        def listed(us, value=value):
            _huffman_unit(us[0], 839, 0)
            assert us[0].census["last"] == value
        out.append((f"listed_{value}", [lit_row(plain(839, top(value)))], listed))

    def one_value(us):  # the second unit is one byte value: one literal and matches
        assert len(us) == 2
        c = us[1].census
        _raw_literals(us[1])
        assert c["nlit"] == 1 and c["nseq"] >= 1 and c["huf"] == 0 and c["block"] == 2
    out.append(("one_value", [lit_row(plain(UNIT) + b"a" * 200)], one_value))

    def not_smaller(us):  # eligible, but the tree description outweighs the gain
        c = us[0].census
        _raw_literals(us[0])
        assert c["huf"] >= c["raw"] and c["bits"] > 0 and c["block"] == 0
    rng = random.Random(77)
    out.append(("not_smaller", [lit_row(bytes(rng.randrange(129) for _ in range(120)))],
                not_smaller))
    for d, (seed, n) in EDGE.items():  # Huffman only when strictly smaller
        def edge(us, d=d):
            c = us[0].census
            assert c["huf"] - c["raw"] == d and c["bits"] > 0 and c["block"] == 2, c
            assert c["lit"] == (2 if d < 0 else 0), c
        out.append((f"edge_{d:+d}", [lit_row(edge_body(seed, n))], edge))

    def with_sequences(us):  # literals gathered from between matches, four streams
        c = us[0].census
        assert c["nseq"] >= 100 and c["lit"] == 2 and c["streams"] == 4 and c["block"] == 2, c
    body = bytearray(plain(20000))
    for k in range(150):  # a copy of 30 earlier bytes every 100
        at = 5000 + 100 * k
        body[at:at + 30] = body[at - 4000:at - 3970]
    out.append(("with_sequences", [lit_row(bytes(body))], with_sequences))

    # Raw literals beside so many sequences that their bitstream (more than 3 072 bytes)
    # reaches the words of the hash-table region in which the Huffman phases keep their
    # tables: the kernel's way from those tables into phase H.  Once with eligible literals
    # that do not pay for their tree, once with a literal above 128.
    def many_sequences(us, eligible):
        c = us[0].census
        _raw_literals(us[0])
        assert c["block"] == 2 and c["nseq"] >= 800, c
        assert (c["bits"] > 0 and c["huf"] >= c["raw"]) if eligible else c["huf"] == 0, c
        assert c["csz"] - c["raw"] - 3 > 3072, c  # (2 bytes of count, 1 of modes)
    for name, high in (("many_sequences_not_smaller", False), ("many_sequences_ineligible", True)):
        rng = random.Random(91)
        body = bytearray(6) + bytearray(rng.sample(range(20, 129), 16))
        if high:
            body[10] = 200
        for _ in range(2500):  # five of those sixteen bytes again, from anywhere in them
            at = rng.randrange(6, 17)
            body += body[at:at + 5]
        out.append((name, [lit_row(bytes(body))], lambda us, e=not high: many_sequences(us, e)))
    return out


def extra():
    """Row sets of the GPU test beyond the fixtures: (name, rows, strict_go known only at T)."""
    rng = random.Random(5)
    text = ZC.raw_of(ZC.text_rows(1000))
    return [("text_46", ZC.text_rows(46)),
            ("three_units_short_last", [ZC.block(text[:2 * UNIT + 5])]),
            ("seven_bytes", [(b"k", b"")]),
            ("random_bytes", [(b"r", rng.randbytes(9000))]),
            ("text_1500", ZC.text_rows(1500))]
