"""GPU parity of the large-block pass (okv_tile_kernel: 16 KiB source tiles,
one short-lived workgroup each) at the edges of its tiling, against the C
oracle.  Every segment here averages more than 16 KiB per block, so the
decode takes the large-block path (okv_count_kernel -> okv_scan_kernel ->
okv_tile_kernel + okv_copy_kernel for big blocks).  Bit-exact."""
from __future__ import annotations

import numpy as np
import pytest

from tests import guarded as G
from tests.test_decode_gpu import _assert_same_as_oracle

pytestmark = pytest.mark.gpu

TILE = 16384


def _rec(rng, kl, vl):
    return (kl.to_bytes(2, "little") + vl.to_bytes(4, "little") +
            rng.integers(0, 256, kl + vl, dtype=np.uint8).tobytes())


def _segment(blocks, seed, pad_to=65536, gap=0):
    """blocks: list of record-shape lists [(klen, vlen), ...]; each block is
    padded to a multiple of pad_to (BlockSize) and placed `gap` bytes after
    the previous one."""
    rng = np.random.default_rng(seed)
    seg, descs = bytearray(), []
    for shape in blocks:
        body = b"".join(_rec(rng, kl, vl) for kl, vl in shape)
        bsize = max(pad_to, -(-len(body) // pad_to) * pad_to)
        off = len(seg) + gap
        seg += bytes(off - len(seg)) + body + bytes(bsize - len(body))
        descs.append((off, bsize, len(body), 0))
    return bytes(seg), np.array(descs, np.uint64).reshape(-1, 4)


def _fill_to(target, kl, rng):
    """Record shapes whose framed bytes sum exactly to target (>= 6 + kl)."""
    shape, left = [], target
    while left > 0:
        vl = int(rng.integers(500, 3000))
        if left - (6 + kl + vl) < 6 + kl + 1:
            vl = left - 6 - kl
        shape.append((kl, vl))
        left -= 6 + kl + vl
    return shape


def _boundary_segment():
    rng = np.random.default_rng(1)
    blocks = []
    for edge in (TILE, 2 * TILE, 3 * TILE):
        for delta in (-7, -6, -3, 0, 1, 3, 6, 9, 40, 200):
            # a first stretch ending `delta` bytes around the edge, then one record across it
            head = _fill_to(edge + delta - (6 + 20 + 1000), 12, rng)
            blocks.append(head + [(20, 1000)] + [(33, 777)] * 3)
    for k in (1, 2, 3, 4):  # blocks ending exactly on a tile edge
        blocks.append(_fill_to(k * TILE, 16, rng))
    return _segment(blocks, 2)


def _long_key_segment():
    rng = np.random.default_rng(3)
    blocks = [[(60000, 100), (5, 4000)],
              [(65535 - 10, 0)],
              [(int(rng.integers(0, 9)), int(rng.integers(0, 4))) for _ in range(64)],
              [(0, int(rng.integers(0, 300))) for _ in range(64)],
              [(int(rng.integers(1, 300)), 0) for _ in range(64)],
              [(7, 1)] * 64]
    blocks += [[(int(rng.integers(0, 9)), int(rng.integers(0, 4))) for _ in range(64)]
               for _ in range(40)]
    return _segment(blocks, 4)


def _odd_offset_segments():
    rng = np.random.default_rng(5)
    blocks = [_fill_to(int(rng.integers(30000, 65000)), int(rng.integers(8, 200)), rng)
              for _ in range(60)]
    for gap in (1, 3, 5, 13):
        seg, d = _segment(blocks, 6, pad_to=65536, gap=gap)
        d[-1, 1] = len(seg) - d[-1, 0]  # ends exactly at the segment end
        yield seg, d


def _line_cut_segment():
    """Blocks of 2-4 tiles whose interior 16 KiB edges meet the value-range
    cut's cases (okv_decode.hip line_cut: a cut moves up to the next 128-byte
    line of the value arena when the bytes it adds are staged by the tile
    before it).  Returns the segment, its descs and the number of such edges."""
    rng = np.random.default_rng(11)
    blocks, nedge = [], 0
    for b in range(192):
        ntile = 2 + b % 3
        shape, pos = [], 0

        def fill(target, kl):  # records up to block byte `target`
            nonlocal pos
            shape.extend(_fill_to(target - pos, kl, rng))
            pos = target

        def put(*recs):
            nonlocal pos
            shape.extend(recs)
            pos += sum(6 + kl + vl for kl, vl in recs)

        for e in range(1, ntile):
            edge, case = e * TILE, nedge % 5
            nedge += 1
            if b % 4 == 0 and e == ntile - 1:
                # the value region ends before the next line: the clamp to round16(VT)
                fill(edge - 20, 12)
                put(*[(100, 3)] * 4)
            elif case == 0:  # a value straight across the edge
                fill(edge - 1500 - (6 + 16), 16)
                put((16, 3000))
            elif case == 1:
                # a value ending d bytes after the edge, then a long key: the line
                # lies in the next value, 6 + key + up to 127 bytes further on
                d = (1, 9, 16, 40, 77, 120)[(nedge // 5) % 6]
                fill(edge + d - (6 + 16 + 600), 16)
                put((16, 600), (330 + 10 * ((nedge // 5) % 18), 300))
            elif case == 2:  # many rows inside one line: the cut stays
                fill(edge - 900, 16)
                put(*[(100, int(rng.integers(0, 13))) for _ in range(16)])
            elif case == 3:  # empty values exactly at the cut
                fill(edge - 2 * (6 + 30), 16)
                put((30, 0), (30, 0), (30, 0), (30, 0), (30, 200))
            else:  # a value ending exactly at the edge, then empty values
                fill(edge, 16)
                put((30, 0), (30, 0), (30, 64))
        if b % 4:
            fill(int(rng.integers(pos + 600, ntile * TILE - 8)), 16)
        assert (ntile - 1) * TILE < pos <= ntile * TILE and len(shape) <= 64, (b, pos, len(shape))
        blocks.append(shape)
    seg, d = _segment(blocks, 12)
    return seg, d, nedge


def test_tile_boundaries(decoder):
    """Records whose header, key or value straddles a 16 KiB tile edge, and
    values / whole blocks ending exactly on one (the last tile then owns only
    the 16-byte padding of its regions)."""
    seg, d = _boundary_segment()
    got = decoder.decode(seg, d)
    _assert_same_as_oracle(got, seg, d, 0, False)
    assert (got.status == 0).all()


def test_long_keys_and_tiny_values(decoder):
    """A 60 000-byte key spanning four tiles; 64-row blocks of 0-3 byte
    values and 0-8 byte keys (many rows per destination chunk and per 64-byte
    granule of the row lookup); empty keys; a block of empty values only."""
    seg, d = _long_key_segment()
    got = decoder.decode(seg, d)
    _assert_same_as_oracle(got, seg, d, 0, False)


def test_odd_offsets_and_segment_edges(decoder):
    """Blocks at unaligned offsets (the tile stage's lead-in line starts
    before the block; the first block's before the segment), and the last
    block ending at the segment's last byte."""
    for seg, d in _odd_offset_segments():
        got = decoder.decode(seg, d)
        _assert_same_as_oracle(got, seg, d, 0, False)


def test_value_cuts_on_arena_lines(decoder):
    """The value-range cut between two tiles of a block (okv_decode.hip
    tile_line_cut) at every kind of edge: a value straight across it (the cut
    moves to the line), a value ending 1-120 bytes after it followed by a
    330-500 byte key (the line's source on both sides of the staged
    extension), runs of 0-12 byte values (many rows in one line), empty values
    at the cut, and value regions ending before the next line; first, middle
    and last tiles, every residue of the block's arena base in its line."""
    import objectkv_amd as okv
    seg, d, nedge = _line_cut_segment()
    assert d.shape[0] <= 256 and (d[:, 1] == 65536).all() and nedge >= d.shape[0]
    got = decoder.decode(seg, d)
    assert decoder.last_path() & okv._lib.PATH_TILE, decoder.last_path()
    _assert_same_as_oracle(got, seg, d, 0, False)
    assert (got.status == 0).all()
    assert {int(v) % 128 for v in got.val_base[:d.shape[0]]} == set(range(0, 128, 16))


def test_blocks_past_the_tile_span_and_over_64_rows(decoder):
    """Big blocks mixed into a 64 KiB segment: a 128 KiB block with few rows
    (its walk ends past tiles-per-block x 16 KiB: okv_copy_kernel), blocks of
    more than kRCap (64) rows, and statuses (short, EOF, overrun) beside them."""
    rng = np.random.default_rng(7)
    blocks = []
    for i in range(48):
        if i % 7 == 3:
            blocks.append(_fill_to(100000, 40, rng))  # BlockSize 128 KiB, ~40 rows
        elif i % 7 == 5:
            blocks.append([(8, int(rng.integers(0, 200))) for _ in range(300)])
        else:
            blocks.append(_fill_to(int(rng.integers(40000, 62000)), 24, rng))
    seg, d = _segment(blocks, 8)
    d = d.copy()
    d[10, 2] += 5000  # OriginalSize past the records: the walk overruns -> panic status
    d[20, 0] = len(seg) + 10  # past the segment: EOF
    d[30, 1] = len(seg) - d[30, 0] + 1  # BlockSize past the segment end: short read
    got = decoder.decode(seg, d)
    _assert_same_as_oracle(got, seg, d, 0, False)
    assert got.status[20] == 1 and got.status[30] == 2  # EOF, short read


def test_capacity_statuses_device(decoder):
    """Device outputs sized below the totals: the blocks that do not fit
    report OKV_BLK_CAPACITY, the others are complete and equal the oracle's."""
    torch = pytest.importorskip("torch")
    import objectkv_amd as okv
    w = okv.synth_segment(okv.sst.SYNTH_ZIPF, 9, nblocks=64, threshold=57344, block_size=65536)
    seg, d = w.data(), w.descs()[:64]
    ref = decoder.decode(seg, d)
    dev = torch.device("cuda", 0)
    seg_t = torch.from_numpy(seg).to(dev)
    d_t = torch.from_numpy(d.view(np.int64)).to(dev)
    rows, kb, vb = decoder.plan_device(seg_t, seg.size, d_t, 64)
    for cut in ("val", "key", "rows"):
        frames = dict(row_start=G.frame(65, np.uint64, device=dev),
                      key_base=G.frame(64, np.uint64, device=dev),
                      val_base=G.frame(64, np.uint64, device=dev),
                      status=G.frame(64, np.int32, device=dev),
                      key_off=G.frame(rows // 2 if cut == "rows" else rows, np.uint64, device=dev),
                      key_len=G.frame(rows, np.uint16, device=dev),
                      val_off=G.frame(rows, np.uint64, device=dev),
                      val_len=G.frame(rows, np.uint32, device=dev),
                      key_arena=G.frame(kb // 2 if cut == "key" else kb, np.uint8, device=dev),
                      val_arena=G.frame(vb // 2 if cut == "val" else vb, np.uint8, device=dev))
        out = {k: f.view for k, f in frames.items()}
        with pytest.raises(Exception):
            decoder.decode_device(seg_t, seg.size, d_t, 64, out, sync=True)
        for k, f in frames.items():
            f.check(k)
        st = out["status"].cpu().numpy()
        assert (st == 5).any() and (st == 0).any(), cut
        first_bad = int(np.argmax(st != 0))
        assert (st[first_bad:] == 5).all()  # capacity failures are a suffix
        for b in range(first_bad):
            r0, r1 = int(ref.row_start[b]), int(ref.row_start[b + 1])
            assert np.array_equal(out["val_len"][r0:r1].cpu().numpy().view(np.uint32),
                                  ref.val_len[r0:r1])
            if cut != "val":
                lo, hi = int(ref.val_base[b]), int(ref.val_base[b + 1])
                assert out["val_arena"][lo:hi].cpu().numpy().tobytes() == \
                    ref.val_arena[lo:hi].tobytes()
