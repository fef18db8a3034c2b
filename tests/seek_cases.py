"""Segments and probe keys for the seek tests (tests/test_seek_host.py on the CPU,
tests/test_range_gpu.py on the device), with the expected row ranges taken from
oracle/pyoracle.py's RowIter: Seek(key), then Next() to io.EOF.
"""
from __future__ import annotations

from oracle import pyoracle as P

ASC, DESC = P.DirectionAscending, P.DirectionDescending
PFX = b"ABCDEFGHIJKLMNOPQR"  # 18 bytes: keys that share 8, 9, 16 and 17 of them


def _write(rows, threshold, block_size):
    w = P.SegmentWriter(P.SegmentWriterOptions(threshold, block_size))
    for k, v in rows:
        w.WriteRow(k, v)
    n, _meta = w.Close()
    return bytes(w.external), n


def _two_per_block(keys):
    """Rows of 120 bytes each but the last (50), written with a 200-byte threshold: every
    second row closes a block and Close flushes the last one (a block the threshold had
    just closed would panic in Close, Q1)."""
    rows = [(k, bytes(120 - 6 - len(k))) for k in keys[:-1]]
    rows.append((keys[-1], bytes(50 - 6 - len(keys[-1]))))
    return _write(rows, 200, 256)


def segments():
    """name -> (segment bytes, file length)."""
    ties = sorted({PFX[:8], PFX[:8] + b"a", PFX[:9] + b"a", PFX[:16] + b"a", PFX[:17] + b"a",
                   PFX + b"z"})
    return {
        "one": _write([(b"m", b"v")], 3584, 4096),
        "3x2": _two_per_block([b"k%02d" % i for i in (10, 20, 30, 40, 50, 60)]),
        "ties": _two_per_block(ties),
    }


def layout(data, n):
    """-> (row keys ascending, block_first_row with the row count appended)."""
    r = P.SegmentReader(data, n)
    md = r.FetchAndLoadMetadata()
    keys, first = [], []
    for st in md.entries:
        first.append(len(keys))
        keys += [P._b(kv.Key) for kv in r.ReadBlockWithStat(st) or []]
    return keys, first + [len(keys)]


def probes(keys):
    qs = {b"", b"\xff", b"\x00", b"\xff\xff", b"\xfe", b"a", b"zzzz"}
    for k in keys:
        qs |= {k, k + b"\x00", k[:-1], k[:-1] + b"\xff", k[:-1] + bytes([max(k[-1] - 1, 0)]),
               k[:-1] + bytes([min(k[-1] + 1, 255)])}
    for n in (8, 9, 16, 17):
        qs |= {PFX[:n], PFX[:n] + b"b", PFX[:n] + b"\x00", PFX[:n - 1] + b"\xff"}
    return sorted(qs)


def expected(data, n, keys, key, direction):
    """[lo, hi) of the rows RowIter(direction).Seek(key) then Next() yields."""
    r = P.SegmentReader(data, n)
    r.FetchAndLoadMetadata()
    it = r.RowIter(direction)
    it.Seek(key)
    got = []
    while True:
        try:
            got.append(P._b(it.Next().Key))
        except P.GoError as e:
            assert e.kind == P.EOF
            break
        assert len(got) <= len(keys)
    if direction == ASC:
        assert got == keys[len(keys) - len(got):], (key, got)
        return len(keys) - len(got), len(keys)
    assert got == keys[:len(got)][::-1], (key, got)
    return 0, len(got)


def cases():
    """[(name, keys, block_first_row, [(key, direction, lo, hi)])]"""
    out = []
    for name, (data, n) in segments().items():
        keys, first = layout(data, n)
        qs = [(q, d) + expected(data, n, keys, q, d) for q in probes(keys) for d in (ASC, DESC)]
        out.append((name, keys, first, qs))
    return out
