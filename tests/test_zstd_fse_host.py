"""FSE-compressed Huffman weights of the device zstd encoder (OKV_F_ZSTD_HUF_FSE), no GPU: the
statements of objectkv_amd/csrc/okv_zstd_enc.hpp run on the CPU by tests/zenc_fse_main.cpp,
built with AddressSanitizer and UBSan and run as a plain program.

* Every frame the writer gives, in each of the three modes, inflates to its input by libzstd
  (oracle/zstd_ref.py); a segment of its frames decodes by the C oracle.
* Mode 0 frames are tests/zenc_model.py's and mode 1 frames tests/zenc_huf_model.py's.
* huf_lengths_all (package-merge at 11 bits over 256 symbols) equals huf_lengths where no
  value is above 128, and its cost equals an independent package-merge's on histograms up to
  value 255.
* Each fixture of tests/zenc_fse_cases.py is the shape it claims, from the model's census.
* Per unit: bytes with the flag <= bytes under OKV_F_ZSTD_HUFFMAN alone <= bytes flag-off."""
from __future__ import annotations

import random

import numpy as np
import pytest

from oracle import zstd_ref as Z
from tests import zenc_cases as ZC
from tests import zenc_fse_cases as FC
from tests import zenc_fse_model as F
from tests import zenc_huf_model as H
from tests import zenc_model as M
from tests.test_zstd_huf_host import L, fibonacci, histograms, package_merge_cost


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return F.build_fse_main(str(tmp_path_factory.mktemp("zenc_fse") / "zenc_fse_main"),
                            sanitize=True)


# ---- code lengths -----------------------------------------------------------------------
def test_lengths_without_a_value_above_128_are_huf_lengths(exe):
    hists = histograms()
    for (name, h), (mb, lens, mb_old, lens_old) in zip(hists, F.code_lengths(
            [h for _, h in hists], exe)):
        assert mb == mb_old > 0 and lens[:129] == lens_old and not any(lens[129:]), name
    one, none = [0] * 256, [0] * 256
    one[200] = 900
    assert [r[0] for r in F.code_lengths([one, none], exe)] == [0, 0]


def wide_histograms():
    rng = random.Random(21)
    out = []

    def put(name, pairs):
        h = [0] * 256
        for s, c in pairs:
            h[s] += c
        assert sum(h) <= 32768
        out.append((name, h))
    put("all_256", [(s, 1 + (s * 37) % 101) for s in range(256)])
    put("all_256_equal", [(s, 128) for s in range(256)])
    put("fibonacci_21_high", [(255 - i, c) for i, c in enumerate(fibonacci(21))])
    put("fibonacci_19_and_flat", [(200 + i, c) for i, c in enumerate(fibonacci(19))] +
        [(s, 3) for s in range(0, 200)])
    put("two_00_ff", [(0, 7), (255, 4000)])
    put("two_equal_00_ff", [(0, 5), (255, 5)])
    for k in range(4):
        syms = rng.sample(range(256), rng.randint(130, 256))
        put(f"random_{k}", [(s, rng.randint(1, 120)) for s in syms])
    put("skewed_wide", [(s, max(1, int(9000 * 0.7 ** i))) for i, s in
                        enumerate(rng.sample(range(256), 90))])
    return out


def test_lengths_over_256_symbols_are_valid_and_optimal(exe):
    hists = wide_histograms()
    bound = 0
    for (name, h), (mb, lens, mb_old, _) in zip(hists, F.code_lengths([h for _, h in hists], exe)):
        present = [s for s in range(256) if h[s]]
        assert max(present) > 128 and mb_old == 0, name
        assert all((lens[s] > 0) == (h[s] > 0) for s in range(256)), name
        assert mb == max(lens) and 1 <= mb <= L, name
        assert sum(1 << (mb - lens[s]) for s in present) == 1 << mb, name  # Kraft with equality
        cost = sum(h[s] * lens[s] for s in present)
        limited = package_merge_cost([h[s] for s in present], L)
        print(f"{name}: {len(present)} symbols, limit-{L} optimum {limited}, "
              f"huf_lengths_all {cost} (longest {mb})")
        assert cost == limited, name
        bound += mb == L
    assert bound >= 3  # the Fibonacci counts and all 256 values bind the limit
    two = dict(hists)["two_00_ff"]
    assert F.code_lengths([two], exe)[0][0] == 1


# ---- the description ---------------------------------------------------------------------
def test_description_cap(exe):
    """A description of exactly 127 bytes was not found: over 400 seeded lists of 255 weights,
    uniform over 6 .. 12 values (the most bytes: 12 values), the largest is 124 bytes, and
    none is refused for its size.  The header byte stays below 128 either way."""
    lists, tags = [], []
    for seed in range(400):
        rng = random.Random(seed)
        k = rng.randint(6, 12)
        lists.append([rng.randrange(k) for _ in range(255)])
        tags.append((seed, k))
    got = F.descriptions(lists, exe)
    assert all(0 < b <= 127 and a == 6 for b, a in got)
    best = max(range(400), key=lambda i: got[i][0])
    print(f"largest FSE description: {got[best][0]} bytes at (seed, values) {tags[best]}")
    assert got[best][0] == 124 and tags[best] == (95, 12)
    # no description: one weight, all weights one value; the accuracy log by the count
    got = F.descriptions([[3], [2] * 40, [1, 2], [0] * 126 + [1], [0] * 127 + [1]], exe)
    assert [b for b, _ in got[:2]] == [0, 0] and got[2][0] > 0
    assert [a for _, a in got[2:]] == [5, 5, 6]


# ---- frames -----------------------------------------------------------------------------
def _frames(exe, tmp_path, rows, T=61440):
    """Per raw block of the rows: (raw, [(frame, units) of mode 0, 1, 2])."""
    return [(raw, [F.model(raw, mode, exe, str(tmp_path)) for mode in (F.OFF, F.HUF, F.FSE)])
            for raw in ZC.blocks_of(rows, T)]


def _check_block(raw, modes):
    for frame, _ in modes:
        got = Z.decompress(frame, len(raw))
        assert got is not None, "libzstd rejects the frame"
        assert got == raw
    (off, _), (huf, units_huf), (fse, units) = modes
    assert off == M.model_frame(raw), "mode 0: the frame of tests/zenc_model.py"
    assert huf == H.model(raw, True)[0], "mode 1: the frame of tests/zenc_huf_model.py"
    sizes = [[s for _t, s in M.block_headers(f, len(raw))] for f in (fse, huf, off)]
    pos = pos_huf = M.frame_header_size(len(raw))
    for s_fse, s_huf, s_off, u, uh in zip(*sizes, units, units_huf):
        assert s_fse <= s_huf <= s_off
        c = u.census
        if c["lit"] == 0:  # raw literals under the flag: the unit's bytes of the other modes
            assert fse[pos:pos + 3 + s_fse] == huf[pos_huf:pos_huf + 3 + s_huf]
        elif c["desc"] == 0 and uh.census["lit"] == 2:  # direct weights: mode 1's unit
            assert fse[pos:pos + 3 + s_fse] == huf[pos_huf:pos_huf + 3 + s_huf]
        else:
            assert s_fse < s_huf and c["block"] == 2
            if c["desc"] == 1:
                assert fse[pos + 3 + M_huf_header(c["nlit"])] == c["dbytes"] - 1 < 128
        pos += 3 + s_fse
        pos_huf += 3 + s_huf


def M_huf_header(nlit):
    return 3 if nlit <= 1023 else 4 if nlit <= 16383 else 5


FIXTURES = {name: (rows, ok) for name, rows, ok in FC.fixtures()}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_is_the_shape_it_claims(exe, tmp_path, name):
    rows, ok = FIXTURES[name]
    blocks = _frames(exe, tmp_path, rows)
    assert len(blocks) == 1
    raw, modes = blocks[0]
    _check_block(raw, modes)
    ok(modes[2][1])
    if name == "largest_129":  # the parent's fixture: raw without the new flag
        assert modes[1][0] == modes[0][0] and len(modes[2][0]) < len(modes[1][0])
        assert modes[1][1][0].census["block"] == 0


@pytest.mark.parametrize("name", [n for n, _ in FC.extra()])
def test_extra_rows_inflate(exe, tmp_path, name):
    rows = dict(FC.extra())[name]
    for T in (3584, 61440):
        for raw, modes in _frames(exe, tmp_path, rows, T):
            _check_block(raw, modes)


def test_census_over_the_fixtures(exe, tmp_path):
    """Both descriptions, both accuracy logs, raw literals under the flag, odd and even numbers
    of listed weights, 255 listed weights, an FSE description beside sequences and without:
    all present."""
    seen = set()
    for name, (rows, _) in FIXTURES.items():
        for _raw, modes in _frames(exe, tmp_path, rows):
            for u in modes[2][1]:
                c = u.census
                seen.add(("lit", c["lit"]))
                if c["lit"] == 2:
                    seen.add(("desc", c["desc"]))
                    if c["desc"] == 1:
                        seen.add(("alog", c["alog"]))
                        seen.add(("listed_odd", c["last"] % 2))
                        seen.add(("listed", c["last"]))
                        seen.add(("nseq0", c["nseq"] == 0))
                        seen.add(("streams", c["streams"]))
    assert {("lit", 0), ("lit", 2), ("desc", 0), ("desc", 1), ("alog", 5), ("alog", 6)} <= seen
    assert {("listed_odd", 0), ("listed_odd", 1), ("listed", 255), ("nseq0", True),
            ("nseq0", False), ("streams", 1), ("streams", 4)} <= seen


def test_text_fixture_is_smaller_again(exe, tmp_path):
    raw = ZC.raw_of(ZC.text_rows(46))
    ((_, modes),) = _frames(exe, tmp_path, ZC.text_rows(46))
    sizes = [len(f) for f, _ in modes]
    print(f"46 text rows: {sizes[0]} flag-off, {sizes[1]} Huffman, {sizes[2]} with FSE weights; "
          f"libzstd-1 {len(Z.compress(raw, 1))}")
    assert sizes[0] == 897 and sizes[2] < sizes[1] < 897
    assert modes[2][1][0].census["desc"] == 1 and modes[2][1][0].census["alog"] == 5


def test_c_oracle_inflates_a_segment_of_model_frames(exe, tmp_path):
    """The file around the model's frames (zstd_segment) decodes by the C oracle to the rows."""
    from oracle import coracle as CO
    rows = dict(FC.extra())["utf8_rows"] + FIXTURES["largest_129"][0] + FIXTURES["all_256"][0]
    T, D = 3584, 4096
    frames = [F.model(raw, F.FSE, exe, str(tmp_path)) for raw in ZC.blocks_of(rows, T)]
    assert sum(u.census["desc"] == 1 and u.census["lit"] == 2 for _, us in frames for u in us) >= 3
    seg, flen, _meta = Z.zstd_segment(rows, T, D, frame_fn=lambda raw, i: frames[i][0])
    rc, md = CO.fetch_meta(seg, flen)
    assert rc == 0 and md["compression"] == 1
    descs = CO.descs_array([(e["offset"], e["block_size"], e["original_size"],
                             e["compressed_size"]) for e in md["entries"]])
    ref = CO.decode_soa(seg, descs, 1)
    assert int(np.max(ref["status"])) == 0
    va = ref["val_arena"].tobytes()
    got = [va[int(o):int(o) + int(n)] for o, n in zip(ref["val_off"], ref["val_len"])]
    assert got == [v for _, v in rows]
