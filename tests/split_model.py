"""The range-split rule of okv_encode_split, restated in plain Python (no GPU): a linear walk
over the blocks, independent of the binary searches and the pointer jumping in
objectkv_amd/csrc/okv_split.hpp.

The rows are cut into blocks by the writer's greedy chain; a segment is a run of consecutive
blocks.  The segment starting at block i ends with the first block j >= i for which
sum BlockSize[i..j] >= split_bytes (split_bytes != 0) or rows(i..j) >= split_rows
(split_rows != 0); if neither holds before the last block it ends with the last block."""
from __future__ import annotations


def boundaries(block_sizes, first_rows, split_bytes, split_rows):
    """block_sizes[nb], first_rows[nb + 1] (entry nb = the row count) -> the first block of
    every segment, then nb: [0, s1, ..., nb]."""
    nb = len(block_sizes)
    assert len(first_rows) == nb + 1 and nb >= 1
    starts = [0]
    nbytes = 0
    for j in range(nb):
        nbytes += int(block_sizes[j])
        nrows = int(first_rows[j + 1]) - int(first_rows[starts[-1]])
        if j + 1 < nb and ((split_bytes and nbytes >= split_bytes) or
                           (split_rows and nrows >= split_rows)):
            starts.append(j + 1)
            nbytes = 0
    starts.append(nb)
    return starts


def blocks_of_rows(rows, threshold=3584, block_size=4096):
    """SegmentWriter's cut of [(key, value)] -> (block_sizes, first_rows): a block is flushed
    once its framed rows reach `threshold` bytes and padded to
    (len // block_size + 1) * block_size (Q2)."""
    sizes, first, cur = [], [0], 0
    for i, (k, v) in enumerate(rows):
        cur += 6 + len(k) + len(v or b"")
        if cur >= threshold:
            sizes.append((cur // block_size + 1) * block_size)
            first.append(i + 1)
            cur = 0
    if cur:
        sizes.append((cur // block_size + 1) * block_size)
        first.append(len(rows))
    return sizes, first


def edge_cases():
    """(name, block_sizes, first_rows, split_bytes, split_rows) for the edges the rule has."""
    u = [4096] * 10
    f = list(range(0, 110, 10))
    return [
        ("bytes_only", u, f, 3 * 4096, 0),
        ("rows_only", u, f, 0, 25),
        ("both_zero", u, f, 0, 0),
        ("both", u, f, 5 * 4096, 20),
        ("block_alone_over", [4096, 65536, 4096, 4096, 131072], [0, 3, 4, 9, 11, 12], 8192, 0),
        ("every_block_over", [8192] * 7, list(range(8)), 4096, 0),
        ("exact_on_last_bytes", [4096] * 6, list(range(0, 70, 10)), 3 * 4096, 0),
        ("exact_on_last_rows", [4096] * 6, list(range(0, 70, 10)), 0, 30),
        ("short_last", [4096] * 7, list(range(0, 80, 10)), 3 * 4096, 0),
        ("one_block", [4096], [0, 5], 1, 1),
        ("one_block_no_limit", [4096], [0, 5], 0, 0),
        ("rows_met_by_first_block", [4096] * 4, [0, 100, 200, 300, 400], 0, 1),
        ("huge_thresholds", u, f, 1 << 62, 1 << 62),
    ]
