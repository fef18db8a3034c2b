"""Huffman literals of the device zstd encoder (OKV_F_ZSTD_HUFFMAN), no GPU: the statements
of objectkv_amd/csrc/okv_zstd_enc.hpp run on the CPU by tests/zenc_huf_main.cpp, built with
AddressSanitizer and UBSan and run as a plain program.

* Every frame the writer gives inflates to its input by libzstd (oracle/zstd_ref.py) and by
  the C oracle's own decoder.
* huf_lengths (package-merge at 11 bits) against an independent Huffman (heapq) and an
  independent package-merge written here: the code is valid and complete, its cost equals
  the unrestricted optimum wherever that tree is at most 11 deep, and equals the
  length-limited optimum everywhere (the algorithm is package-merge, so equality, no excess).
* Each fixture of tests/zenc_huf_cases.py is the shape it claims, from the model's census.
* Without the flag the writer's frame is tests/zenc_model.py's, byte for byte; with it no
  unit is larger, and a unit whose literals stay raw is byte-identical."""
from __future__ import annotations

import heapq
import random

import numpy as np
import pytest

from oracle import zstd_ref as Z
from tests import zenc_cases as ZC
from tests import zenc_huf_cases as HC
from tests import zenc_huf_model as H
from tests import zenc_model as M

L = 11


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return H.build_huf_main(str(tmp_path_factory.mktemp("zenc_huf") / "zenc_huf_main"),
                            sanitize=True)


# ---- code lengths -----------------------------------------------------------------------
def huffman_depths(counts):
    """Unrestricted Huffman: (cost, deepest leaf) of the present symbols."""
    heap = [(c, i, 0, 0) for i, c in enumerate(counts)]  # weight, tie, cost so far, depth
    heapq.heapify(heap)
    tie = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tie, a[2] + b[2] + a[0] + b[0], max(a[3], b[3]) + 1))
        tie += 1
    return heap[0][2], heap[0][3]


def package_merge_cost(counts, limit):
    """The least sum(count * length) over prefix codes with lengths <= limit (Larmore and
    Hirschberg), with every item carrying the multiset of its leaves."""
    leaves = sorted((c, (i,)) for i, c in enumerate(counts))
    n = len(leaves)
    assert 2 <= n <= 1 << limit
    items = list(leaves)
    for _ in range(limit - 1):
        packs = [(items[k][0] + items[k + 1][0], items[k][1] + items[k + 1][1])
                 for k in range(0, len(items) - 1, 2)]
        items = sorted(leaves + packs, key=lambda it: it[0])
    length = [0] * n
    for _, members in items[:2 * n - 2]:
        for i in members:
            length[i] += 1
    assert sum(2 ** (limit - ln) for ln in length) == 2 ** limit
    return sum(c * ln for c, ln in zip(counts, length))


def fibonacci(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def histograms():
    """(name, 256 counts)."""
    rng = random.Random(9)
    out = []

    def put(name, pairs):
        h = [0] * 256
        for s, c in pairs:
            h[s] += c
        assert sum(h) <= 32768
        out.append((name, h))
    for k in range(6):
        syms = rng.sample(range(129), rng.randint(2, 129))
        put(f"random_{k}", [(s, rng.randint(1, 250)) for s in syms])
    for k in range(4):  # a few symbols carry nearly everything
        syms = rng.sample(range(129), 40)
        put(f"skewed_{k}", [(s, max(1, int(12000 * 0.6 ** i))) for i, s in enumerate(syms)])
    for name, rows in (("text_46", ZC.text_rows(46)), ("text_420", ZC.text_rows(420))):
        put(name, [(b, 1) for b in ZC.raw_of(rows)])
    put("two_symbols", [(0, 1), (128, 5000)])
    put("two_equal", [(7, 3), (9, 3)])
    put("all_129", [(s, 1 + (s * 37) % 101) for s in range(129)])
    put("all_129_equal", [(s, 200) for s in range(129)])
    put("equal_64", [(s, 17) for s in range(64)])
    put("equal_3", [(s, 5) for s in (1, 2, 3)])
    put("fibonacci_21", list(enumerate(fibonacci(21))))          # unrestricted depth 20
    put("fibonacci_14_from_60", [(60 + i, c) for i, c in enumerate(fibonacci(14))])  # depth 13
    put("fibonacci_12", list(enumerate(fibonacci(12))))          # depth 11: the limit just holds
    put("powers_of_two", [(2 * i, 1 << i) for i in range(14)])   # depth 13
    put("fibonacci_and_flat", list(enumerate(fibonacci(19))) + [(s, 3) for s in range(40, 129)])
    return out


def test_code_lengths_are_valid_and_optimal(exe):
    hists = histograms()
    got = H.code_lengths([h for _, h in hists], exe)
    bound, free = 0, 0
    for (name, h), (longest, lens) in zip(hists, got):
        present = [s for s in range(256) if h[s]]
        counts = [h[s] for s in present]
        assert all((lens[s] > 0) == (h[s] > 0) for s in range(129)), name
        assert longest == max(lens) and 1 <= longest <= L, name
        # complete: the weights 2^(longest - len) fill 2^longest exactly (Kraft with equality)
        assert sum(1 << (longest - lens[s]) for s in present) == 1 << longest, name
        cost = sum(h[s] * lens[s] for s in present)
        best, depth = huffman_depths(counts)
        limited = package_merge_cost(counts, L)
        print(f"{name}: {len(present)} symbols, unrestricted depth {depth} cost {best}, "
              f"limit-{L} optimum {limited}, huf_lengths {cost} (longest {longest})")
        assert cost == limited, name
        if depth <= L:
            assert cost == best, name
            free += 1
        else:
            assert cost > best, name
            bound += 1
    assert bound >= 4 and free >= 10
    depths = {name: huffman_depths([c for c in h if c])[1] for name, h in hists}
    assert depths["fibonacci_21"] >= 12 and depths["fibonacci_12"] == 11


def test_ineligible_histograms(exe):
    one, high, none = [0] * 256, [0] * 256, [0] * 256
    one[65] = 900
    high[3], high[129] = 5, 5
    assert [r[0] for r in H.code_lengths([one, high, none], exe)] == [0, 0, 0]


# ---- frames -----------------------------------------------------------------------------
def _frames(exe, tmp_path, rows, T=61440):
    """Per raw block of the rows: (raw, frame with the flag, units, frame without)."""
    out = []
    for raw in ZC.blocks_of(rows, T):
        on, units = H.model(raw, True, exe, str(tmp_path))
        off, units_off = H.model(raw, False, exe, str(tmp_path))
        out.append((raw, on, units, off, units_off))
    return out


def _check_block(raw, on, units, off, units_off):
    for frame in (on, off):
        got = Z.decompress(frame, len(raw))
        assert got is not None, "libzstd rejects the frame"
        assert got == raw
    assert off == M.model_frame(raw), "without the flag: the frame of tests/zenc_model.py"
    # per unit never larger; raw literals: the unit's bytes are the flag-off ones
    pos_on = pos_off = M.frame_header_size(len(raw))
    for (_t, s_on), (_t2, s_off), u in zip(M.block_headers(on, len(raw)),
                                           M.block_headers(off, len(raw)), units):
        assert s_on <= s_off
        if u.census["lit"] == 0:
            assert on[pos_on:pos_on + 3 + s_on] == off[pos_off:pos_off + 3 + s_off]
        else:
            assert s_on < s_off and u.census["block"] == 2
        pos_on += 3 + s_on
        pos_off += 3 + s_off
    assert all(u.census["lit"] == 0 for u in units_off)


FIXTURES = {name: (rows, ok) for name, rows, ok in HC.fixtures()}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_is_the_shape_it_claims(exe, tmp_path, name):
    rows, ok = FIXTURES[name]
    blocks = _frames(exe, tmp_path, rows)
    assert len(blocks) == 1
    for b in blocks:
        _check_block(*b)
    ok(blocks[0][2])
    if name == "largest_129":
        assert blocks[0][1] == blocks[0][3]


@pytest.mark.parametrize("name", [n for n, _ in HC.extra()])
def test_extra_rows_inflate(exe, tmp_path, name):
    rows = dict(HC.extra())[name]
    for T in (3584, 61440):
        for b in _frames(exe, tmp_path, rows, T):
            _check_block(*b)


def test_census_over_the_fixtures(exe, tmp_path):
    """One stream and four, Size_Formats 00 / 10 / 11, a Compressed_Block without sequences,
    Huffman literals beside sequences, raw literals under the flag, odd and even numbers of
    listed weights: all present."""
    seen = set()
    for name, (rows, _) in FIXTURES.items():
        for _raw, _on, units, _off, _uo in _frames(exe, tmp_path, rows):
            for u in units:
                c = u.census
                seen.add(("lit", c["lit"], c["streams"], c["sf"]))
                if c["lit"] == 2:
                    seen.add(("nseq0", c["nseq"] == 0))
                    seen.add(("listed_odd", c["last"] % 2))
                    seen.add(("last_stream_mod4", c["nlit"] % 4) if c["streams"] == 4 else None)
    assert {("lit", 2, 1, 0), ("lit", 2, 4, 2), ("lit", 2, 4, 3), ("lit", 0, 0, 0)} <= seen
    assert {("nseq0", True), ("nseq0", False), ("listed_odd", 0), ("listed_odd", 1)} <= seen
    assert {("last_stream_mod4", r) for r in range(4)} <= seen


def test_text_fixture_is_smaller_than_without_the_flag(exe, tmp_path):
    raw = ZC.raw_of(ZC.text_rows(46))
    assert len(raw) == 3542
    ((_, on, units, off, _uo),) = _frames(exe, tmp_path, ZC.text_rows(46))
    print(f"46 text rows: {len(off)} without the flag, {len(on)} with it; "
          f"libzstd-1 {len(Z.compress(raw, 1))}")
    assert len(off) == 897 and len(on) < 897 and units[0].census["lit"] == 2


def test_c_oracle_inflates_a_segment_of_model_frames(exe, tmp_path):
    """The file around the model's frames (zstd_segment) decodes by the C oracle to the rows."""
    from oracle import coracle as CO
    rows = ZC.text_rows(300) + [HC.lit_row(HC.plain(5000))]
    T, D = 3584, 4096
    frames = [H.model(raw, True, exe, str(tmp_path))[0] for raw in ZC.blocks_of(rows, T)]
    seg, flen, _meta = Z.zstd_segment(rows, T, D, frame_fn=lambda raw, i: frames[i])
    rc, md = CO.fetch_meta(seg, flen)
    assert rc == 0 and md["compression"] == 1
    descs = CO.descs_array([(e["offset"], e["block_size"], e["original_size"],
                             e["compressed_size"]) for e in md["entries"]])
    ref = CO.decode_soa(seg, descs, 1)
    assert int(np.max(ref["status"])) == 0
    va = ref["val_arena"].tobytes()
    got = [va[int(o):int(o) + int(n)] for o, n in zip(ref["val_off"], ref["val_len"])]
    assert got == [v for _, v in rows]
