"""Row sets for the device zstd encoder's tests: the fixtures of test_zstd_enc_gpu.py and
the parse fixtures whose conditions test_zstd_enc_model.py asserts from the model's census
(tests/zenc_model.py) on the CPU.  No GPU, no device output.

A raw block is its records back to back: u16 key length, u32 value length, key, value.  A
parse fixture states a whole block `body`; its first 6 + len(key) bytes are replaced by
the record header, the rest is the row's value (block())."""
from __future__ import annotations

import random
import struct

from tests.zenc_model import ML
from tests.zenc_model import QUARTER as Q
from tests.zenc_model import UNIT

CONFIGS = [(3584, 4096), (61440, 65536)]


def raw_of(rows):
    return b"".join(struct.pack("<HI", len(k), len(v)) + k + v for k, v in rows)


def blocks_of(rows, T):
    """The raw blocks of a row set: a block is cut when its raw length reaches T."""
    out, cur = [], b""
    for k, v in rows:
        cur += struct.pack("<HI", len(k), len(v)) + k + v
        if len(cur) >= T:
            out.append(cur)
            cur = b""
    return out + [cur] if cur else out


def closes(rows, T):
    """strict_go for these rows: Go panics in Close when the last row closed a block."""
    raw = 0
    for k, v in rows:
        raw = 0 if raw >= T else raw
        raw += 6 + len(k) + len(v)
    return raw >= T


def text_rows(n, vlen=59):
    rows = []
    for i in range(n):
        v = ('{"id":%d,"name":"user%d","score":%d,"active":true' %
             (100000 + 7 * i, 5000 + i, (i * 37) % 1000)).encode()
        rows.append((b"key%09d" % (i * 3), v.ljust(vlen - 1) + b"}"))
    return rows


def random_rows(seed, n, vmax):
    rng = random.Random(seed)
    return [(b"%08d" % i + rng.randbytes(rng.randint(0, 9)), rng.randbytes(rng.randint(0, vmax)))
            for i in range(n)]


def random_raw(T):
    """Random bytes with nothing to find, one row per block."""
    rng = random.Random(3)
    return [(rng.randbytes(10), rng.randbytes(T + 50 + i)) for i in range(5)]


def periodic(P_, N, seed=5):
    pat = random.Random(seed * 1000 + P_).randbytes(P_)
    return [(b"k", (pat * (N // P_ + 1))[:N - 7])]


def mixed(n, seed=9):
    rng = random.Random(seed)
    half = rng.randbytes((n - 7) // 2)
    return [(b"k", (half + half + b"x")[:n - 7])]


PERIODIC = [(N, P_) for N in (3600, 65000, 200000) for P_ in (1, 7, 64, 222, 1000)] + \
    [(65000, 30000)]

EDGES = {
    "seven_raw_bytes": lambda: [(b"k", b"")],
    "unit_minus_1": lambda: mixed(UNIT - 1),
    "unit": lambda: mixed(UNIT),
    "unit_plus_1": lambda: mixed(UNIT + 1),
    "value_200k_random": lambda: [(b"big", random.Random(1).randbytes(200 * 1024))],
    "value_200k_text": lambda: [(b"a", b"x"), (b"big", raw_of(text_rows(2700))[:200 * 1024])],
    "zeros_70000": lambda: [(b"z", bytes(70000))],
    "empty_values": lambda: [(b"k%05d" % i, b"" if i % 3 else b"v%d" % i) for i in range(900)],
    "small_then_large": lambda: [(b"a%03d" % i, b"ab" * i) for i in range(300)] +
    [(b"b", bytes(range(256)) * 300)] + [(b"c%03d" % i, b"tail") for i in range(50)],
}


def block_pattern(T, nblocks):
    pat = bytes(range(251))
    return [(b"r%05d" % i, (pat * (T // 251 + 1))[i % 7:i % 7 + T]) for i in range(nblocks)]


# ---- parse fixtures ---------------------------------------------------------------------
def block(body, key=b"k"):
    """One row whose record is `body` with its first 6 + len(key) bytes the record header."""
    return (key, bytes(body[6 + len(key):]))


def _copy(buf, dst, src, n):
    for j in range(n):  # (bytewise: an overlapping source repeats)
        buf[dst + j] = buf[src + j]


def quarter_patterns():
    """Sixteen units, one row each, unit m for mask m: quarter q is a 64-byte pattern
    repeated if bit q of m is set, random bytes otherwise."""
    rows = []
    for mask in range(16):
        body = b"".join(random.Random(100 + 4 * mask + q).randbytes(64) * (Q // 64)
                        if mask >> q & 1 else random.Random(200 + 4 * mask + q).randbytes(Q)
                        for q in range(4))
        rows.append(block(body, b"m%02d" % mask))
    return rows


def quarter_patterns_ok(units):
    assert len(units) == 16
    for mask, u in enumerate(units):
        got = sum(1 << q for q in range(4) if u.census["seq_per_quarter"][q])
        assert got == mask, (mask, u.census["seq_per_quarter"])


def hash_collision(seed):
    """Two different 4-byte windows with the same 14-bit hash, found by search."""
    rng, seen = random.Random(seed), {}
    while True:
        w = rng.randbytes(4)
        h = (int.from_bytes(w, "little") * 2654435761 & 0xFFFFFFFF) >> 18
        if h in seen and seen[h] != w:
            return seen[h], w
        seen[h] = w


def hash_groups():
    buf = bytearray(random.Random(41).randbytes(1536))
    buf[128:328] = bytes(200)            # steps 128.. and 192..: all 64 lanes one group
    for at in (400, 420):                # a group of 2 in the step 384..447
        buf[at:at + 4] = b"\xa1\xb2\xc3\xd4"
    for at in (520, 530, 540):           # a group of 3 in the step 512..575
        buf[at:at + 4] = b"\x11\x22\x33\x44"
    # one member in the step 576..639, two in 640..703, one in 704..767 (whose candidate is
    # the lane the group of two left in the table: its last)
    for at in (630, 650, 670, 720):
        buf[at:at + 4] = b"\x5a\x6b\x7c\x8d"
    w1, w2 = hash_collision(1)           # inside one step: the false candidate 790 hides 780
    buf[780:784], buf[790:794], buf[800:804] = w1, w2, w1
    w1, w2 = hash_collision(2)           # over three steps: 970 hides 900
    buf[900:904], buf[970:974], buf[1040:1044] = w1, w2, w1
    return [block(buf)]


def hash_groups_ok(units):
    (u,) = units
    g = u.census["groups"]
    assert (2, 0) in g and (3, 0) in g and (2, 1) in g and any(c == 64 for c, _ in g), g
    assert u.census["hidden"] >= 2
    assert u.cand[800] == -1 and u.cand[1040] == -1 and u.cand[790] == -1
    have = {m[0]: m for m in u.matches}
    assert have[420][2] == 400 and have[530][2] == 520 and have[540][2] == 530
    assert have[650][2] == 630 and have[670][2] == 650 and have[720][2] == 670


MATCH_ENDS_N1 = 20000


def match_ends():
    """A block of two units (UNIT and 20 000 bytes) of random bytes with planted copies,
    each 200 bytes after its source (a near source is rarely hidden by a false candidate)."""
    buf = bytearray(random.Random(43).randbytes(UNIT + MATCH_ENDS_N1))
    end = UNIT + MATCH_ENDS_N1
    for dst, n in ((Q - 20, 40),          # cut at the quarter end, resumed in the next
                   (2 * Q - 13, 12),      # ends at qe - 1
                   (3 * Q - 4, 8),        # starts at qe - 4, the last legal start
                   (UNIT - 30, 30),       # runs to the unit's last byte
                   (UNIT + Q - 3, 7),     # a candidate at qe - 3: not a start
                   (end - 50, 50)):       # runs to the block's last byte
        _copy(buf, dst, dst - 200, n)
        buf[dst - 1] = buf[dst - 201] ^ 0xFF  # the match does not start earlier
    return [block(buf)]


def match_ends_ok(units):
    u0, u1 = units
    m0, m1 = set(u0.matches), set(u1.matches)
    assert {(Q - 20, 20, Q - 220), (Q, 20, Q - 200)} <= m0
    assert (2 * Q - 13, 12, 2 * Q - 213) in m0
    assert {(3 * Q - 4, 4, 3 * Q - 204), (3 * Q, 4, 3 * Q - 200)} <= m0
    assert (UNIT - 30, 30, UNIT - 230) in m0 and u0.tail == 0
    assert u1.n == MATCH_ENDS_N1 and u1.cand[Q - 3] == Q - 203 and u1.cand[Q - 4] == -1
    assert not any(Q - 3 <= s < Q for s, _, _ in m1) and (Q, 4, Q - 200) in m1
    assert (MATCH_ENDS_N1 - 50, 50, MATCH_ENDS_N1 - 250) in m1 and u1.tail == 0


LAST_UNIT_SIZES = [UNIT + r for r in range(1, 6)] + [2 * UNIT]


def last_unit(N):
    body = raw_of(text_rows(1000))[:N - 8] + bytes(8)
    assert len(body) == N
    return [block(body)]


def last_unit_ok(units, N):
    u0, u1 = units
    assert u0.n == UNIT and u1.n == N - UNIT and len(u1.cand) == max(u1.n - 3, 0)
    assert u0.census["block"] == 2
    if u1.n == 5:  # two windows of zeros: a sequence is found, the block stays Raw
        assert u1.seqs == [(1, 4, 1)] and u1.census["block"] == 0
    elif u1.n < 5:
        assert not u1.seqs


RAW_BOUNDARY = {-1: 7, 0: 6, 1: 5}  # compressed size - n: the match length that gives it


def raw_boundary(delta):
    """7 header bytes, 8 random bytes, their first `ml` bytes again, one byte that ends the
    match: one sequence (15, ml, 8).  Compressed size = 1 (literals header) + 16 literals
    + 1 + 1 + 3 (21 bits: 3 offset bits, 18 closing bits) = 22; n = 16 + ml."""
    ml = RAW_BOUNDARY[delta]
    a = random.Random(47).randbytes(8)
    return [block(bytes(7) + a + a[:ml] + bytes([a[ml] ^ 0x55]))]


def raw_boundary_ok(units, delta):
    (u,) = units
    assert u.seqs == [(15, RAW_BOUNDARY[delta], 8)]
    assert u.census["csz_minus_n"] == delta and u.census["block"] == (2 if delta < 0 else 0)


SEQ_COUNTS = [1, 127, 128, 255, 256, 257]


def seq_count(k):
    """4 096 random bytes, then k times: 12 of those bytes again and 3 fresh ones."""
    rng = random.Random(1000 + k)
    buf = bytearray(rng.randbytes(4096))
    for j in range(k):
        at = 16 + 12 * j
        buf += buf[at:at + 12]
        lit = bytearray(rng.randbytes(3))
        if lit[0] == buf[at + 12]:
            lit[0] ^= 0xFF
        buf += lit
    return [block(buf)]


def seq_count_ok(units, k):
    (u,) = units
    assert len(u.seqs) == k and u.census["block"] == 2
    assert u.census["nseq_form"] == (1 if k < 128 else 2)


def dense():
    """One unit of a 4-gram followed by a changing separator byte."""
    rng = random.Random(53)
    return [block(b"".join(b"\xde\xad\xbe\xef" + rng.randbytes(1) for _ in range(UNIT // 5)))]


def dense_ok(units):
    (u,) = units
    assert len(u.seqs) >= 4096 and u.census["block"] == 2
    assert all(c >= 1024 for c in u.census["seq_per_quarter"])


def _emit(buf, rng, ll, ml, off):
    """Appends ll fresh bytes, a copy of ml bytes from `off` back, and one byte that ends
    the match (a literal of the next sequence)."""
    buf += rng.randbytes(ll)
    for _ in range(ml):
        buf.append(buf[-off])
    buf.append(buf[-off] ^ 0xA5)


def code_sweep():
    """Units built sequence by sequence so that, with the rest of the corpus, every
    literal-length, match-length and offset code the parse can reach is used."""
    rows = []
    # long literal runs: codes 33 and 32 in one unit, 31 .. 25 in another
    for name, runs in ((b"s0", (16384, 8192)), (b"s1", (4096, 2048, 1024, 512, 256, 128, 64))):
        rng = random.Random(60 + len(rows))
        buf = bytearray(rng.randbytes(64))
        for ll in runs:
            _emit(buf, rng, ll - 1, 8, 20)
        rows.append(block(buf + rng.randbytes(UNIT - len(buf)), name))
    # literal lengths 1 .. 63 (codes 1 .. 24), then offset codes 2 .. 14 at both ends of
    # their ranges (the largest distance here is 30 000: 32 764 would start at byte 0)
    rng = random.Random(62)
    buf = bytearray(rng.randbytes(64))
    for ll in range(1, 64):
        _emit(buf, rng, ll - 1, 5, 30)
    for c in range(2, 15):
        for off in ((1 << c) - 3, min((2 << c) - 4, 30000)):
            if len(buf) < off:
                buf += rng.randbytes(off - len(buf))
            _emit(buf, rng, 9, 6, off)
    rows.append(block(buf + rng.randbytes(UNIT - len(buf)), b"s2"))
    # match lengths: every code 1 .. 48 at its baseline, each match inside one quarter
    rng = random.Random(63)
    cur = bytearray(rng.randbytes(64))
    for ml, _ in ML[1:49]:
        s = len(cur) + 3
        if s // Q != (s + ml - 1) // Q:
            cur += rng.randbytes(Q - len(cur) % Q)
            s = len(cur) + 3
        if s + ml + 1 > UNIT:
            rows.append(block(cur + rng.randbytes(UNIT - len(cur)), b"s%d" % len(rows)))
            cur = bytearray(rng.randbytes(64))
        _emit(cur, rng, 3, ml, 40)
    rows.append(block(cur + rng.randbytes(UNIT - len(cur)), b"s%d" % len(rows)))
    return rows


REACHABLE = {"ll": set(range(0, 34)), "ml": set(range(1, 49)), "of": set(range(2, 15))}


# ---- the corpus: (name, rows) -----------------------------------------------------------
def parse_fixtures():
    """(name, rows, condition over the units of all blocks in order)."""
    out = [("quarter_patterns", quarter_patterns(), quarter_patterns_ok),
           ("hash_groups", hash_groups(), hash_groups_ok),
           ("match_ends", match_ends(), match_ends_ok),
           ("dense", dense(), dense_ok),
           ("code_sweep", code_sweep(), None)]
    out += [(f"last_unit_{N}", last_unit(N), lambda u, N=N: last_unit_ok(u, N))
            for N in LAST_UNIT_SIZES]
    out += [(f"raw_boundary_{d:+d}", raw_boundary(d), lambda u, d=d: raw_boundary_ok(u, d))
            for d in RAW_BOUNDARY]
    out += [(f"seq_count_{k}", seq_count(k), lambda u, k=k: seq_count_ok(u, k))
            for k in SEQ_COUNTS]
    return out


def corpus(T):
    """Every row set the GPU tests encode at threshold T (the writer-option cases, which
    have thresholds of their own, aside): (name, rows)."""
    out = [("text_46", text_rows(46)), ("text_1500", text_rows(1500)),
           ("text_300", text_rows(300)),
           ("random_raw", random_raw(T)),
           ("random_mixed", random_rows(3, 400, 700)),
           ("raw_100", [(b"r", random.Random(2).randbytes(100))])]
    out += [(f"periodic_{N}_{P_}", periodic(P_, N)) for N, P_ in PERIODIC]
    out += [(name, EDGES[name]()) for name in sorted(EDGES)]
    out += [("blocks_257", block_pattern(T, 257))]
    out += [(name, rows) for name, rows, _ in parse_fixtures()]
    return out


# ---- writer options the zstd path is run at: (name, T, D, rows) --------------------------
WRITER_SHAPES = {(1, 1): 20, (50, 16): 60, (3584, 100): 310, (20000, 512): 1500,
                 (70000, 100): 2700}  # (T, D): text rows
LONG_KEY_SHAPES = [(3584, 100), (3584, 4096)]
META_GROUP = 256    # blocks whose meta entries one workgroup writes
META_IMAGE = 32768  # bytes of meta entries it can stage


def long_first_keys():
    """1 112 blocks of one row each (every row alone reaches T = 3584).  Blocks 0-255: short
    keys and one key of 65 535 bytes; 256-511: short keys; 512-1111: keys of 300 to 2 000
    bytes.  The meta entries of the first and the last three groups of 256 blocks exceed
    32 KiB, those of the second group do not."""
    rng = random.Random(71)
    pat = (b'{"id":%d,"name":"user%d","active":true}' % (1234567, 89)).ljust(64, b".")
    rows = []
    for i in range(1112):
        if i == 100:
            kl = 65535
        elif i < 512:
            kl = 8 + i % 9
        else:
            kl = rng.randint(300, 2000)
        key = b"%08d" % i + rng.randbytes(kl - 8)
        rows.append((key, (pat * 57)[:max(3600 - kl, 16) + i % 5]))
    return rows


def meta_group_bytes(first_keys):
    """Bytes of meta entries (u16 length, key, five u64) per group of 256 blocks."""
    return [sum(2 + len(k) + 40 for k in first_keys[g:g + META_GROUP])
            for g in range(0, len(first_keys), META_GROUP)]


def writer_cases():
    out = [(f"text_T{T}_D{D}", T, D, text_rows(n)) for (T, D), n in WRITER_SHAPES.items()]
    return out + [(f"long_first_keys_D{D}", T, D, long_first_keys()) for T, D in LONG_KEY_SHAPES]
