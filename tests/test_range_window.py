"""The window rule of Reader.GetRanges (objectkv_amd/snapshot.py: cut_windows,
accept_window; no GPU): the GetRange loop run over streams cut to c rows, accepted only
when it provably gives what the loop gives over the whole streams.  The loop is
oracle/snapshot_oracle.py's merge_lists, in both directions."""
from __future__ import annotations

import random

import pytest

from objectkv_amd import snapshot as SN
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO

ASC, DESC = P.DirectionAscending, P.DirectionDescending
assert (ASC, DESC) == (SN.DirectionAscending, SN.DirectionDescending)


def windowed(streams, bound, limit, c, direction):
    """-> (truncated?, accepted?, the windowed merge's result, the full merge's result).
    streams: merge_lists' [(rows, level, lo, hi)]."""
    full = SO.merge_lists(streams, bound, limit, direction)
    windows, frontier = SN.cut_windows([(lo, hi) for _r, _l, lo, hi in streams], c, direction)
    win = [(r, lvl, a, b) for (r, lvl, _lo, _hi), (a, b) in zip(streams, windows)]
    picks, _end = got = SO.merge_lists(win, bound, limit, direction)
    fkeys = [s[0][f][0] for s, f in zip(streams, frontier) if f is not None]
    last = streams[picks[-1][0]][0][picks[-1][1]][0] if picks else None
    ok = SN.accept_window(fkeys, picks is None, len(picks or []), limit, last, bound, direction)
    return bool(fkeys), ok, got, full


def rows(spec):
    """"a b- c" -> [(b"a", b"v"), (b"b", None), (b"c", b"v")]: a trailing '-' is a tombstone."""
    return [(w.rstrip("-").encode(), None if w.endswith("-") else b"v") for w in spec.split()]


def test_window_size_and_cut():
    assert SN.window_size(1) == 18 and SN.window_size(5) == 22 and SN.window_size(100) == 126
    assert all(SN.window_size(n) >= n + 1 for n in range(1, 500))
    w, f = SN.cut_windows([(2, 30), (0, 5), (4, 9)], 5, ASC)
    assert w == [(2, 7), (0, 5), (4, 9)] and f == [6, None, None]  # exactly c rows: not cut
    w, f = SN.cut_windows([(2, 30), (0, 5), (3, 9)], 5, DESC)
    assert w == [(25, 30), (0, 5), (4, 9)] and f == [25, None, 4]  # c + 1 rows: cut
    assert SN.cut_windows([], 5, ASC) == ([], [])


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_accepted_windows_equal_the_full_merge(seed):
    """1-4 streams, 35 % tombstones, levels 0 / 1, limits 1-6, windows 1-8."""
    rng = random.Random(seed)
    accepted = rejected = truncated = 0
    ends = {}
    for _ in range(50000):
        alpha = rng.randint(3, 30)
        streams = []
        for _s in range(rng.randint(1, 4)):
            keys = sorted(rng.sample(range(1, alpha + 1), min(rng.randint(1, 14), alpha)))
            r = [(bytes([k]), None if rng.random() < 0.35 else b"v") for k in keys]
            streams.append((r, rng.choice([0, 0, 1]), rng.randint(0, len(r) - 1), len(r)))
        d = rng.choice([ASC, DESC])
        if d == DESC:
            streams = [(r, lvl, 0, rng.randint(1, len(r))) for r, lvl, _lo, _hi in streams]
        bound = bytes([rng.randint(0, alpha + 1)]) if rng.random() < 0.8 else \
            (b"\xff" if d == ASC else b"")
        limit, c = rng.randint(1, 6), rng.randint(1, 8)
        cut, ok, got, full = windowed(streams, bound, limit, c, d)
        if not cut:
            assert ok and got == full
            continue
        truncated += 1
        if ok:
            accepted += 1
            assert got[0] == full[0], (streams, d, bound, limit, c, got, full)
            ends[full[1]] = ends.get(full[1], 0) + 1
        else:
            rejected += 1
    assert truncated > 20000
    assert 3 * accepted >= truncated, (accepted, rejected)  # it does not pass by refusing
    assert {SO.END_LIMIT, SO.END_BOUND} <= set(ends)


def test_every_ending_is_accepted_somewhere():
    rng = random.Random(9)
    ends = set()
    for _ in range(30000):
        alpha = rng.randint(3, 12)
        streams = []
        for _s in range(rng.randint(1, 3)):
            keys = sorted(rng.sample(range(1, alpha + 1), rng.randint(1, alpha)))
            r = [(bytes([k]), None if rng.random() < 0.35 else b"v") for k in keys]
            streams.append((r, rng.choice([0, 0, 1]), 0, len(r)))
        d = rng.choice([ASC, DESC])
        bound = bytes([rng.randint(0, alpha + 1)])
        cut, ok, got, full = windowed(streams, bound, rng.randint(1, 6), rng.randint(1, 8), d)
        if ok:
            assert got[0] == full[0]
            ends.add((cut, full[1]))
    # with a cut stream an io.EOF is never accepted; without one it is the full merge's
    assert {e for cut, e in ends if cut} == {SO.END_LIMIT, SO.END_BOUND, SO.END_STALE}
    assert {e for _cut, e in ends} == {SO.END_LIMIT, SO.END_BOUND, SO.END_STALE, SO.END_EOF_ROLL,
                                       SO.END_EOF_STALE}


@pytest.mark.parametrize("d", [ASC, DESC])
def test_tombstone_on_the_frontier(d):
    """Stream 0 (L0) is cut on a tombstone: the windowed loop rolls it onto io.EOF where the
    full loop goes on.  Refused, whatever the limit."""
    s0 = (rows("a b c- d e"), 0, 0, 5)  # c = 3: the window ends on c- in either direction
    s1 = (rows("f g h"), 1, 0, 3) if d == ASC else (rows("0 1 2"), 1, 0, 3)
    bound = b"\xff" if d == ASC else b""
    for limit in (1, 2, 3, 6):
        cut, ok, got, full = windowed([s0, s1], bound, limit, 3, d)
        assert cut
        if limit <= 2:  # the page ends strictly before the frontier
            assert ok and got == full and full[1] == SO.END_LIMIT
        else:
            assert got[0] is None and full[0] is not None and not ok


def test_tombstone_first_past_the_bound_in_stream_zero():
    """The bound lies inside stream 0's window and the first row past it is an L0
    tombstone, the window's last row: the loop skips it before it tests the bound, rolls
    off the window and reports io.EOF; the full loop breaks on the next row.  The frontier
    is past the bound, but an io.EOF is never accepted."""
    s0 = (rows("a b c- d e"), 0, 0, 5)
    cut, ok, got, full = windowed([s0], b"bb", 6, 3, ASC)
    assert cut and got[0] is None and full == ([(0, 0), (0, 1)], SO.END_BOUND) and not ok
    # one more window row and the loop breaks at d: the frontier is past the bound
    cut, ok, got, full = windowed([s0], b"bb", 6, 4, ASC)
    assert cut and ok and got == full
    # descending: the same from the other end
    cut, ok, got, full = windowed([s0], b"cc", 6, 3, DESC)
    assert cut and got[0] is None and full == ([(0, 4), (0, 3)], SO.END_BOUND) and not ok
    cut, ok, got, full = windowed([s0], b"cc", 6, 4, DESC)
    assert cut and ok and got == full


@pytest.mark.parametrize("d", [ASC, DESC])
def test_streams_of_c_and_c_plus_one_rows(d):
    r = rows("a b c d e f")
    bound = b"\xff" if d == ASC else b""
    for n, cut_want in ((5, False), (6, True)):
        cut, ok, got, full = windowed([(r, 1, 0, n)], bound, 10, 5, d)
        assert cut == cut_want
        if not cut:
            assert ok and got == full
        else:  # five rows came back, the full stream has six: fewer than limit, refused
            assert not ok and len(got[0]) == 5 and len(full[0]) == 6


@pytest.mark.parametrize("d", [ASC, DESC])
def test_limit_one_and_unbound_bounds(d):
    s0 = (rows("a c e g i k"), 0, 0, 6)
    s1 = (rows("b d f h j l"), 1, 0, 6)
    bound = b"\xff" if d == ASC else b""  # UnboundEnd ascending, UnboundStart descending
    cut, ok, got, full = windowed([s0, s1], bound, 1, 2, d)  # c = limit + 1
    assert cut and ok and got == full and len(full[0]) == 1
    cut, ok, got, full = windowed([s0, s1], bound, 1, 1, d)  # the one row is the frontier
    assert cut and got[0] == full[0] and not ok  # right, but not provably: refused
    # an unbound bound is never reached by a frontier: only a full page is accepted
    cut, ok, got, full = windowed([s0, s1], bound, 3, 4, d)
    assert cut and ok and got == full
    cut, ok, got, full = windowed([s0, s1], bound, 12, 4, d)
    assert cut and not ok and len(got[0]) < len(full[0])


def test_an_untruncated_eof_stands():
    """No stream cut: the result is the full merge's, io.EOF included."""
    s0 = (rows("a b-"), 0, 0, 2)
    cut, ok, got, full = windowed([s0], b"\xff", 5, 8, ASC)
    assert not cut and ok and got == full and full[0] is None
