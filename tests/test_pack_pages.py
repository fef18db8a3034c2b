"""range.pack_pages (no GPU): the okv_merge_pages arguments of one batch of GetRange merges
-- pages, bounds, slice starts and the jobs that stay with okv_merge_rows -- from hand-made
jobs of Reader._merge_group's shape."""
from __future__ import annotations

from objectkv_amd import _lib
from objectkv_amd import range as RG

MAXR = _lib.PAGE_MAX_ROWS


def _job(ranges, lim, direction, bound, base):
    return {"ranges": ranges, "lim": lim, "direction": direction, "bound": bound, "base": base,
            "cap": min(sum(b - a for a, b in ranges), lim)}


def _jobs():
    specs = [
        ([(0, 10), (5, 9)], 100, _lib.DIR_ASC, b"end-0"),
        ([(3, 3 + MAXR)], 7, _lib.DIR_DESC, b""),                      # exactly PAGE_MAX_ROWS rows
        ([(0, MAXR), (10, 11)], 1 << 63, _lib.DIR_ASC, b"\xff"),       # PAGE_MAX_ROWS + 1: old path
        ([(i, i + 1) for i in range(64)], 3, _lib.DIR_DESC, b"k" * 40),  # 64 streams fit
        ([(i, i + 2) for i in range(65)], 1000, _lib.DIR_ASC, b"z"),   # 65 streams: old path
        ([(7, 8)], 1, _lib.DIR_ASC, b"\x00\x01"),
    ]
    jobs, base = [], 0
    for ranges, lim, direction, bound in specs:
        jobs.append(_job(ranges, lim, direction, bound, base))
        base += len(ranges)
    return jobs


def test_slices_are_disjoint_and_in_order_after_the_frontier_slots():
    jobs = _jobs()
    for first in (0, 5):
        pages, bounds, at, old = RG.pack_pages(jobs, first)
        assert len(at) == len(jobs) and at[0] == first
        for i, j in enumerate(jobs):  # every job's slice, the old path's too
            assert at[i] == first + sum(x["cap"] for x in jobs[:i])
        paged = [i for i in range(len(jobs)) if i not in old]
        assert [p.out_at for p in pages] == [at[i] for i in paged]
        assert [p.out_cap for p in pages] == [jobs[i]["cap"] for i in paged]
        ends = [at[i] + jobs[i]["cap"] for i in range(len(jobs))]
        assert all(e <= a for e, a in zip(ends, at[1:]))


def test_src_at_is_the_gather_base_and_bounds_lie_back_to_back():
    jobs = _jobs()
    pages, bounds, at, old = RG.pack_pages(jobs, 3)
    paged = [j for i, j in enumerate(jobs) if i not in old]
    assert len(pages) == len(paged) == 4
    pos = 0
    for p, j in zip(pages, paged):
        assert (p.src_at, p.nsrc) == (j["base"], len(j["ranges"]))
        assert (p.bound_at, p.bound_len) == (pos, len(j["bound"]))
        assert bounds[p.bound_at:p.bound_at + p.bound_len] == j["bound"]
        pos += len(j["bound"])
    assert pos == len(bounds) and isinstance(bounds, bytes)


def test_big_jobs_and_65_streams_stay_on_the_old_path():
    jobs = _jobs()
    _pages, _bounds, _at, old = RG.pack_pages(jobs)
    assert old == [2, 4]
    assert sum(b - a for a, b in jobs[2]["ranges"]) == MAXR + 1
    assert len(jobs[4]["ranges"]) == 65
    # PAGE_MAX_ROWS rows and 64 streams are pages
    assert sum(b - a for a, b in jobs[1]["ranges"]) == MAXR and len(jobs[3]["ranges"]) == 64


def test_limit_and_direction_are_carried_through():
    jobs = _jobs()
    pages, _bounds, _at, old = RG.pack_pages(jobs)
    paged = [j for i, j in enumerate(jobs) if i not in old]
    assert [p.limit for p in pages] == [j["lim"] for j in paged] == [100, 7, 3, 1]
    assert [p.direction for p in pages] == [j["direction"] for j in paged]
    assert all(p.pad == 0 for p in pages)


def test_no_jobs():
    pages, bounds, at, old = RG.pack_pages([], 4)
    assert (len(pages), bounds, at, old) == (0, b"", [], [])
