"""okv_merge_pages (objectkv_amd/csrc/okv_pages.hip): many GetRange merges in one launch,
each page against the restated Go loop (oracle.snapshot_oracle.merge_lists) and, where
named, against okv_merge_rows on the same streams.  The inputs and their preconditions are
tests/test_merge_gpu.py's, reused by import.  Every call is made through run_pages, which
lays the slices out between guard slots and checks, for every page, that the guards are
untouched, that the slots of a slice past its rows are empty markers and that src counts in
the call's sources."""
from __future__ import annotations

import ctypes as C
import random
import struct

import numpy as np
import pytest
import torch

import objectkv_amd as okv
from objectkv_amd import range as RG
from objectkv_amd import snapshot as SN
from oracle import pyoracle as P
from oracle import snapshot_oracle as SO
from tests import snapshot_cases as SC
from tests import test_merge_gpu as MG
from tests.test_range_gpu import _outcome, _pair, _returned

pytestmark = pytest.mark.gpu

L = okv._lib
ASC, DESC = L.DIR_ASC, L.DIR_DESC
MAXR = L.PAGE_MAX_ROWS
GUARD = 3
FILL = -7
EMPTY = -1  # 0xffffffff in the int32 tensor


class Spec:
    """One page: streams [src_at, src_at + nsrc) of the call's sources."""

    def __init__(self, src_at, nsrc, direction, bound, limit, cap=None):
        self.src_at, self.nsrc, self.direction = src_at, nsrc, direction
        self.bound, self.limit, self.cap = bound, limit, cap


class PageResult:
    pass


def _layout(caps, slice_order):
    """Slice starts with GUARD slots before, between and after -> (out_at per page, total)."""
    at, pos = [0] * len(caps), GUARD
    for pi in slice_order:
        at[pi] = pos
        pos += caps[pi] + GUARD
    return at, pos


def run_pages(dec, streams, specs, slice_order=None, device_mode=False, base16=False):
    """One okv_merge_pages call over `streams` (the call's sources, MG.Stream) and `specs`
    -> [PageResult] in specs order, with the raw arrays on result[0].raw.  base16: src and
    row start 16 bytes into a 128-byte line (inside a larger tensor of FILL)."""
    dev = torch.device("cuda", 0)
    caps = [sum(s.hi - s.lo for s in streams[p.src_at:p.src_at + p.nsrc]) if p.cap is None
            else p.cap for p in specs]
    at, total = _layout(caps, slice_order or range(len(specs)))
    out = {"src": torch.full((total,), FILL, dtype=torch.int32, device=dev),
           "row": torch.full((total,), FILL, dtype=torch.int64, device=dev)}
    if base16:
        whole = {"src": torch.full((total + 64,), FILL, dtype=torch.int32, device=dev),
                 "row": torch.full((total + 32,), FILL, dtype=torch.int64, device=dev)}
        for k, t in whole.items():
            skip = ((16 - t.data_ptr()) % 128) // t.element_size()
            out[k] = t[skip:skip + total]
            assert out[k].data_ptr() % 128 == 16
    bounds, pages = b"", []
    for p, a, cap in zip(specs, at, caps):
        pages.append(L.Page(p.limit, a, cap, p.src_at, p.nsrc, len(bounds), len(p.bound),
                            p.direction, 0))
        bounds += p.bound
    srcs = [s.src() for s in streams]
    torch.cuda.synchronize()  # (torch filled the arrays on its stream, the call runs on another)
    if device_mode:
        for k in ("n_rows", "n_unique", "status"):
            out[k] = torch.full((len(specs),), FILL, dtype=torch.int32, device=dev)
        dec.merge_pages_device(srcs, pages, bounds, out, sync=False)
        dec.sync()
        n_rows, n_unique, status = (out[k].cpu().numpy() for k in ("n_rows", "n_unique", "status"))
    else:
        n_rows, n_unique, status = dec.merge_pages_device(srcs, pages, bounds, out)
    src, row = out["src"].cpu().numpy(), out["row"].cpu().numpy()
    in_slice = np.zeros(total, bool)
    res = []
    for pi, (p, a, cap) in enumerate(zip(specs, at, caps)):
        r = PageResult()
        r.n_rows, r.n_unique, r.status = int(n_rows[pi]), int(n_unique[pi]), int(status[pi])
        n = r.n_rows if r.status == 0 else 0
        assert n <= cap, (pi, n, cap)
        assert not in_slice[a:a + cap].any()
        in_slice[a:a + cap] = True
        # past the rows: empty markers, row untouched
        assert (src[a + n:a + cap] == EMPTY).all(), (pi, r.status, src[a:a + cap])
        assert (row[a + n:a + cap] == FILL).all(), pi
        # src counts in the call's sources
        assert ((src[a:a + n] >= p.src_at) & (src[a:a + n] < p.src_at + p.nsrc)).all(), pi
        r.pairs = [(int(s) - p.src_at, int(q)) for s, q in zip(src[a:a + n], row[a:a + n])]
        res.append(r)
    # guard slots: everything outside the slices
    assert (src[~in_slice] == FILL).all() and (row[~in_slice] == FILL).all()
    assert int((~in_slice).sum()) == GUARD * (len(specs) + 1)
    if base16:  # nothing outside the arrays either
        for t in whole.values():
            assert int((t != FILL).sum()) == int((out["src" if t.dtype == torch.int32
                                                      else "row"] != FILL).sum())
    if res:
        res[0].raw = (src, row, np.asarray(n_rows), np.asarray(n_unique), np.asarray(status))
    return res


def check_page(r, streams, p, want=None):
    """Page result r against the Go loop over its streams -> how the loop ended."""
    mine = streams[p.src_at:p.src_at + p.nsrc]
    rows, end = want or MG.ref_getrange(mine, p.direction, p.bound, p.limit)
    assert r.n_unique == MG.n_unique_of(mine), end
    if rows is None:
        assert r.status == L.M_EOF, (end, r.status, r.n_rows)
    else:
        assert (r.status, r.n_rows) == (0, len(rows)), end
        assert r.pairs == [tuple(x) for x in rows], end
    return end


# ---- 1. the Go loop, 360 pages in one call ---------------------------------------------


def test_getrange_random_360_pages_one_call(decoder):
    cases = [MG._getrange_case(1000 + i) for i in range(360)]
    ends = MG._getrange_precondition(cases)
    assert sum(ends.values()) == 360
    streams, specs = [], []
    for i, (ss, direction, bound, limit) in enumerate(cases):
        specs.append(Spec(len(streams), len(ss), direction, bound, limit))
        streams += [MG.stream_of_rows(rows, level, lo, hi, align=(i + 7 * s) % 16)
                    for s, (rows, level, lo, hi) in enumerate(ss)]
    assert max(sum(s.hi - s.lo for s in streams[p.src_at:p.src_at + p.nsrc]) for p in specs) <= MAXR
    assert any(p.limit == 1 << 63 for p in specs)
    rng = random.Random(360)
    call_order = list(range(360))
    rng.shuffle(call_order)
    slice_order = list(range(360))
    rng.shuffle(slice_order)
    assert call_order != slice_order
    shuffled = [specs[i] for i in call_order]
    res = run_pages(decoder, streams, shuffled, slice_order)
    got = {}
    for r, p in zip(res, shuffled):
        end = check_page(r, streams, p)
        got[end] = got.get(end, 0) + 1
    assert got == ends


# ---- 2. termination ties, 7. device mode -----------------------------------------------


def _tie_pages():
    streams, specs, wants = [], [], []
    for name in sorted(MG.TERMINATION_TIES):
        ss, direction, bound, limit, want_end, want_rows = MG.TERMINATION_TIES[name]
        mine = [MG.stream_of_rows(rows, level) for rows, level in ss]
        rows, end = MG.ref_getrange(mine, direction, bound, limit)
        # precondition: the reference ends this case the way its name says
        assert end == want_end and (rows is None if want_rows is None else len(rows) == want_rows)
        specs.append(Spec(len(streams), len(mine), direction, bound, limit))
        wants.append((rows, end))
        streams += mine
    return streams, specs, wants


def test_termination_ties_one_call(decoder):
    streams, specs, wants = _tie_pages()
    res = run_pages(decoder, streams, specs)
    for r, p, want in zip(res, specs, wants):
        assert check_page(r, streams, p, want) == want[1]
    assert {r.status for r in res} == {0, L.M_EOF}


def test_termination_ties_src_and_row_at_base_16(decoder):
    """The same pages with src and row 16 bytes into a 128-byte line: the contract for
    device pointers is their natural alignment, not a line."""
    streams, specs, wants = _tie_pages()
    res = run_pages(decoder, streams, specs, base16=True)
    for r, p, want in zip(res, specs, wants):
        assert check_page(r, streams, p, want) == want[1]


def test_device_mode_equals_host_mode(decoder):
    """OKV_F_DEVICE_PTRS | OKV_F_ASYNC with device n_rows / n_unique / status, then okv_sync."""
    streams, specs, wants = _tie_pages()
    host = run_pages(decoder, streams, specs)
    dev = run_pages(decoder, streams, specs, device_mode=True)
    for a, b in zip(host[0].raw, dev[0].raw):
        assert np.array_equal(a, b)
    for r, p, want in zip(dev, specs, wants):
        check_page(r, streams, p, want)


# ---- 3. long keys ----------------------------------------------------------------------


def test_long_keys_one_call(decoder):
    rows = [[kv for kv in rs if kv[0]] for rs in MG._long_key_rows()]
    MG._long_key_precondition([[(b"", None)] + rs if s in (1, 3) else rs
                               for s, rs in enumerate(rows)])
    keys = sorted({k for rs in rows for k, _v in rs})
    assert sum(len(k) > 16 for k in keys) >= 30 and max(len(k) for k in keys) == MG.MAXKEY
    streams, specs = [], []
    for levels in ((1, 1, 1, 1), (0, 0, 1, 2)):
        at = len(streams)
        streams += [MG.stream_of_rows(rs, level=levels[s], align=(3 + 5 * s) % 16)
                    for s, rs in enumerate(rows)]
        for direction in (ASC, DESC):
            for bound in keys[::6] + [b"\xff", b""]:
                for limit in (3, 1 << 63):
                    specs.append(Spec(at, 4, direction, bound, limit))
    assert any(len(p.bound) > 16 for p in specs) and len(streams) == 8
    res = run_pages(decoder, streams, specs)
    for r, p in zip(res, specs):
        check_page(r, streams, p)
    assert max(r.n_rows for r in res if r.status == 0) >= 10  # long keys compared and emitted


# ---- 4. stream counts and empty streams ------------------------------------------------


def test_stream_counts_and_empty_streams_one_call(decoder):
    shared = b"key-020-in-all"
    streams, specs = [], []
    for nsrc in (1, 2, 63, 64):
        at = len(streams)
        streams += [MG.stream_of_rows(rs, level=0 if s < nsrc // 2 else 1, align=s % 16)
                    for s, rs in enumerate(MG._small_streams(nsrc, nsrc, shared))]
        for direction in (ASC, DESC):
            for bound, limit in ((b"\xff", 1 << 63), (b"", 1 << 63), (shared, 1000),
                                 (b"key-030", 5)):
                specs.append(Spec(at, nsrc, direction, bound, limit))
    rows = MG._small_streams(9, 5)
    all_empty = None
    for empty in ((0,), (2,), (4,), (0, 2, 4), (0, 1, 2, 3), (0, 1, 2, 3, 4)):
        at = len(streams)
        for s, rs in enumerate(rows):
            e = min(1, len(rs))  # an empty range that is not [0, 0)
            lo, hi = (e, e) if s in empty else (0, len(rs))
            streams.append(MG.stream_of_rows(rs, level=0 if s < 3 else 1, lo=lo, hi=hi))
        for direction in (ASC, DESC):
            if len(empty) == 5 and direction == ASC:
                all_empty = len(specs)
            specs.append(Spec(at, 5, direction, b"\xff" if direction == ASC else b"", 1 << 63))
            specs.append(Spec(at, 5, direction, b"key-020", 2))
    no_streams = len(specs)
    specs.append(Spec(len(streams), 0, ASC, b"\xff", 1, cap=2))  # nsrc = 0, at the array's end
    specs.append(Spec(3, 0, DESC, b"", 1, cap=0))
    res = run_pages(decoder, streams, specs)
    for r, p in zip(res, specs):
        if p.nsrc:
            check_page(r, streams, p)
    for i in (all_empty, all_empty + 1, no_streams, no_streams + 1):
        assert (res[i].n_rows, res[i].n_unique, res[i].status) == (0, 0, 0)


# ---- 5. sizes around the kernel's loops ------------------------------------------------


def _sized_streams(total, seed):
    """Three streams of `total` rows of 8-byte big-endian keys, all with the same first and
    last key (so the loop runs to the end in both directions); stream 0 on level 0 with
    every fifth row a tombstone, never its first or last row."""
    rng = random.Random(seed)
    sizes = [total - 2 * (total // 3), total // 3, total // 3]
    first, last = 0, 4 * total + 9
    out = []
    for s, n in enumerate(sizes):
        if n == 0:
            ks = []
        elif n == 1:
            ks = [last]
        else:
            ks = [first] + sorted(rng.sample(range(1, 2 * total), n - 2)) + [last]
        rows = [(struct.pack(">Q", k), None if s == 0 and q % 5 == 2 and 0 < q < n - 1 else b"v")
                for q, k in enumerate(ks)]
        out.append(MG.stream_of_rows(rows, level=0 if s == 0 else 1, align=(5 * s + total) % 16))
    assert sum(s.n for s in out) == total
    return out


def test_sizes_around_the_loops_big_and_all_equal(decoder):
    sizes = (1, 255, 256, 257, 1023, 1024, 1025, MAXR - 1, MAXR)
    streams, specs = [], []
    for total in sizes:
        at = len(streams)
        streams += _sized_streams(total, total)
        specs += [Spec(at, 3, ASC, b"\xff", 1 << 63), Spec(at, 3, DESC, b"", 1 << 63)]
    sized = len(specs)
    # a page of PAGE_MAX_ROWS + 1 rows between two small pages
    small = [[(b"a%02d" % i, b"x") for i in range(s, 30, 3)] for s in range(3)]
    at = len(streams)
    streams += [MG.stream_of_rows(rs) for rs in small]
    specs.append(Spec(at, 3, ASC, b"\xff", 1 << 63))
    big_at = len(streams)
    streams += _sized_streams(MAXR + 1, 77)
    big = len(specs)
    specs.append(Spec(big_at, 3, ASC, b"\xff", 1 << 63, cap=5))
    specs.append(Spec(at, 3, DESC, b"", 4))
    # all streams equal
    eq = [(struct.pack(">Q", 3 * i + 1), b"e") for i in range(300)]
    eq_at = len(streams)
    streams += [MG.stream_of_rows(eq, level=1, align=s) for s in range(4)]
    equal = len(specs)
    specs.append(Spec(eq_at, 4, ASC, b"\xff", 1 << 63))
    res = run_pages(decoder, streams, specs)
    for i, (r, p) in enumerate(zip(res, specs)):
        if i == big:
            assert (r.status, r.n_rows, r.n_unique) == (L.M_BIG, 0, 0)
            continue
        mine = streams[p.src_at:p.src_at + p.nsrc]
        want = MG.ref_getrange(mine, p.direction, p.bound, p.limit)
        if i < sized:  # precondition: the loop runs on, most keys are returned
            assert want[0] is not None and 2 * len(want[0]) >= MG.n_unique_of(mine), i
            m = MG.run_merge(decoder, mine, MG.GETRANGE, p.direction, p.limit, p.bound)
            assert (m.rc, m.status, m.n_rows, m.n_unique) == (0, r.status, r.n_rows, r.n_unique)
            assert [tuple(x) for x in m.pairs.tolist()] == r.pairs
        check_page(r, streams, p, want)
    assert res[equal].n_unique == 300 and res[equal].n_rows == 300
    assert all(s == 0 for s, _q in res[equal].pairs)
    # its neighbours (checked against the loop above) returned rows
    assert res[big - 1].n_rows == 28 and res[big + 1].n_rows == 4  # (stream 0 runs out on a27)


# ---- 6. capacity -----------------------------------------------------------------------


def test_capacity(decoder):
    streams = [MG.stream_of_rows(rs, level=1) for rs in MG._small_streams(3, 4)]
    want, _end = MG.ref_getrange(streams, ASC, b"\xff", 1 << 63)
    n = len(want)
    assert n >= 3
    ss, direction, bound, limit, want_end, _r = MG.TERMINATION_TIES["stale-tombstone"]
    assert want_end == SO.END_EOF_STALE
    eof_at = len(streams)
    streams += [MG.stream_of_rows(rows, level) for rows, level in ss]
    specs = [Spec(0, 4, ASC, b"\xff", 1 << 63, cap=n - 1),
             Spec(0, 4, ASC, b"\xff", 1 << 63, cap=n),
             Spec(eof_at, len(ss), direction, bound, limit, cap=0),
             Spec(0, 4, ASC, b"\xff", 1 << 63, cap=0)]
    res = run_pages(decoder, streams, specs)  # (run_pages: no row of a page with a status)
    assert (res[0].status, res[0].n_rows, res[0].n_unique) == (L.M_CAPACITY, n, MG.n_unique_of(streams[:4]))
    check_page(res[1], streams, specs[1])
    assert res[2].status == L.M_EOF
    assert (res[3].status, res[3].n_rows) == (L.M_CAPACITY, n)


# ---- 8. arguments ----------------------------------------------------------------------


def test_argument_errors_launch_nothing(decoder):
    dev = torch.device("cuda", 0)
    streams = [MG.stream_of_rows(MG._kv(b"k1", b"k2"), 1), MG.stream_of_rows(MG._kv(b"k2", b"k3"), 1)]
    assert MG.ref_getrange(streams, ASC, b"k3", 9)[0] == [(0, 0), (0, 1)]
    lib = L.lib()

    def call(nsrc=2, ranges=None, page=None, n_pages=1, bounds=b"k3", bounds_len=None,
             null=(), big_srcs=0):
        arr = (L.MergeSrc * max(nsrc, big_srcs, 1))()
        for i in range(nsrc):
            s = streams[i % 2]
            lo, hi = ranges[i] if ranges else (s.lo, s.hi)
            t = s.t
            arr[i] = L.MergeSrc(t["key_arena"].data_ptr(), t["key_off"].data_ptr(),
                                t["key_len"].data_ptr(), t["val_arena"].data_ptr(),
                                t["val_off"].data_ptr(), t["val_len"].data_ptr(), lo, hi, s.level, 0)
        kw = dict(limit=9, out_at=1, out_cap=4, src_at=0, nsrc=2, bound_at=0, bound_len=2,
                  direction=ASC, pad=0)
        kw.update(page or {})
        pages = (L.Page * 1)(L.Page(**kw))
        src = torch.full((6,), FILL, dtype=torch.int32, device=dev)
        row = torch.full((6,), FILL, dtype=torch.int64, device=dev)
        per = [np.full(1, FILL, np.int32) for _ in range(3)]
        b = np.frombuffer(bounds, np.uint8)
        po = L.PagesOut(None if "src" in null else src.data_ptr(), row.data_ptr(),
                        None if "n_rows" in null else per[0].ctypes.data, per[1].ctypes.data,
                        per[2].ctypes.data)
        rc = lib.okv_merge_pages(decoder._ctx, None if "srcs" in null else arr,
                                 big_srcs or nsrc, None if "pages" in null else pages, n_pages,
                                 None if "bounds" in null else b.ctypes.data,
                                 b.size if bounds_len is None else bounds_len,
                                 None if "out" in null else C.byref(po), 0)
        torch.cuda.synchronize()
        return rc, src.cpu().numpy(), row.cpu().numpy(), [int(a[0]) for a in per]

    def valid(**kw):
        rc, src, row, per = call(**kw)
        assert rc == 0 and per == [2, 3, 0]
        assert src.tolist() == [FILL, 0, 0, EMPTY, EMPTY, FILL]
        assert row.tolist() == [FILL, 0, 1, FILL, FILL, FILL]

    valid()
    long_bounds = b"k3" + bytes(70000)
    bad = {
        "out NULL": dict(null=("out",)),
        "srcs NULL": dict(null=("srcs",)),
        "pages NULL": dict(null=("pages",)),
        "bounds NULL": dict(null=("bounds",)),
        "n_rows NULL": dict(null=("n_rows",)),
        "src NULL": dict(null=("src",)),
        "65 streams": dict(nsrc=66, page=dict(nsrc=65)),
        "src_at + nsrc past the array": dict(page=dict(src_at=1, nsrc=2)),
        "src_at past the array": dict(page=dict(src_at=0xffffffff, nsrc=2)),
        "limit 0": dict(page=dict(limit=0)),
        "direction": dict(page=dict(direction=2)),
        "bound past bounds_len": dict(page=dict(bound_at=1, bound_len=2)),
        "bound_len > 65535": dict(bounds=long_bounds, page=dict(bound_len=65536)),
        "row_hi < row_lo": dict(ranges=[(0, 2), (2, 1)]),
        "65536 sources": dict(big_srcs=65536),
    }
    for what, kw in bad.items():
        rc, src, row, per = call(**kw)
        assert rc == L.OKV_E_ARG, what
        assert (src == FILL).all() and (row == FILL).all() and per == [FILL] * 3, what
        valid()
    valid(nsrc=64)  # 64 sources of the call, 65535 bound bytes and no pages are accepted
    valid(bounds=long_bounds)  # a larger image, then the small one again over the same scratch
    valid()
    rc, src, row, per = call(n_pages=0, null=("pages",))
    assert rc == 0 and (src == FILL).all() and per == [FILL] * 3


# ---- 9. GetRanges uses the batch -------------------------------------------------------


def test_get_ranges_uses_the_batch(decoder, monkeypatch):
    segs, keys = SC.random_snapshot(21, nseg=4, keyspace=1500, rows_per_seg=(700, 900))
    orc, dev = _pair(segs, decoder)
    packs = []
    real = RG.pack_pages

    def spy(jobs, first_slot=0):
        got = real(jobs, first_slot)
        packs.append((len(jobs), len(got[0]), len(got[3])))
        return got
    monkeypatch.setattr(RG, "pack_pages", spy)
    rng = random.Random(121)
    probes = keys + [k + b"\x00" for k in keys[::7]] + [b"", b"k", b"z", P.UnboundEnd]
    queries = []
    while len(queries) < 64:
        a, b = rng.choice(probes), rng.choice(probes)
        if SO._cmp(a, b) > 0:
            a, b = b, a
        if rng.random() < 0.1:
            a = P.UnboundStart
        queries.append((a, b, rng.choice([1, 2, 3, 7, 50]), rng.choice([ASC, DESC])))
    got = dev.GetRanges(queries)
    rows = 0
    for q, g in zip(queries, got):
        want = _outcome(lambda: orc.GetRange(*q))
        assert _returned(g) == want, (q, _returned(g), want)
        rows += want[0] == "rows" and len(want[1]) > 0
    assert rows > 20
    st = dev.range_stats
    assert set(st) == set(SN._RANGE_STATS)
    # the windowed round is one call; the reruns' pages one more, their big merges one each
    assert packs and packs[0][0] == packs[0][1] > 20 and packs[0][2] == 0
    assert SN.window_size(50) * 4 <= MAXR
    assert st["merge_calls"] == 1 + sum((p > 0) + o for _j, p, o in packs[1:])
    assert st["pages_merged"] == sum(p for _j, p, _o in packs)
    assert st["reruns"] == sum(j for j, _p, _o in packs[1:])
    assert st["merge_calls"] < len(queries)
    # one query whose page is big: the old path, the same rows
    del packs[:]
    q = (P.UnboundStart, P.UnboundEnd, 100_000, ASC)
    assert SN.window_size(q[2]) * 4 > MAXR
    got = dev.GetRanges([q])[0]
    want = _outcome(lambda: orc.GetRange(*q))
    assert _returned(got) == want
    assert packs == [(1, 0, 1)]  # its four whole streams hold more than PAGE_MAX_ROWS rows
    st = dev.range_stats
    assert (st["merge_calls"], st["pages_merged"], st["reruns"]) == (1, 0, 0)
