#!/usr/bin/env python3
"""getrange_bench.py -- one GetRange page from resident segments (Reader.GetRanges) against
the path before it (Reader.GetRange over DeviceSegment and the whole-tail merge).
DESIGN.md 23.

Needs an MI355X: it fails without one.  Everything is in one process and session; the arms
alternate round by round (--reps rounds after --warm warm-up rounds) and the median of
the host clock around a call is reported, because both paths synchronise with the host
between their device steps (each okv_merge_rows does, three times).

  snapshot: tools/snap_getrows_bench.py's -- 8 segments, 4 at level 0 and 4 at level 1, of
            --rows rows each (16-byte keys: 8 zero bytes + the big-endian index; 64-byte
            values), 4 KiB blocks; segment s holds the indices 15 000 s + 2 j + (s mod 2)
  page:     limit 100, ascending, to UnboundEnd, starting at the 1st, 50th and 99th
            percentile of the key space
  arms:     GetRanges of that one query; the parent's GetRange of it; GetRanges of 1, 64
            and 1 024 such queries (starts drawn uniformly within one percent of the key
            space after the percentile)
Also reported: the split of a GetRanges call into seek, merges and gather by device events
on the decoder's stream (Reader.range_profile), range_stats, and the bytes a segment keeps
resident on either path.

Run from the repository root:  python tools/getrange_bench.py [--log PATH]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import snapshot as SN  # noqa: E402
from tools.snap_getrows_bench import segment_rows  # noqa: E402

OUT = []
ASC = SN.DirectionAscending


def say(line):
    print(line, flush=True)
    OUT.append(line)


def key_of(i):
    return bytes(8) + int(i).to_bytes(8, "big")


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def nbytes(tensors):
    return sum(int(t.numel()) * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("getrange_bench.py needs a GPU: nothing is measured without one")
    dec = okv.Decoder(0)
    enc = okv.Encoder(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    data, recs = {}, []
    for s in range(8):
        idx = (15000 * s + 2 * np.arange(a.rows) + (s & 1)).astype(np.uint64)
        e = enc.encode(segment_rows(idx))
        md = okv.fetch_metadata(e.seg, e.file_bytes)
        sid = f"{s:02d}"
        data[sid] = (e.seg.tobytes(), e.file_bytes)
        recs.append(SN.SegmentRecord(sid, 0 if s < 4 else 1, md.first_key, md.last_key))
    span = 15000 * 7 + 2 * a.rows
    say(f"snapshot: 8 segments (4 L0, 4 L1) of {a.rows} rows, 4 KiB blocks, "
        f"{sum(len(d[0]) for d in data.values())} bytes; indices 0 .. {span}; "
        f"page: limit {a.limit} ascending to UnboundEnd, window {SN.window_size(a.limit)} rows")
    rd = SN.Reader(lambda rec: data[rec.ID], dec)
    rd.UpdateSegments(recs, None)
    rng = np.random.default_rng(23)
    batches = [int(x) for x in a.batches.split(",")]

    for pct in (1, 50, 99):
        at = span * pct // 100
        q = (key_of(at), SN.UnboundEnd, a.limit, ASC)
        qs = {n: [(key_of(at + int(x)), SN.UnboundEnd, a.limit, ASC)
                  for x in rng.integers(0, max(span // 100, 1), n)] for n in batches}
        t_new, t_old, t_b = [], [], {n: [] for n in batches}
        split = {"seek_ms": [], "merge_ms": [], "gather_ms": []}
        for r in range(a.warm + a.reps):  # the arms take turns
            rd.range_profile = False
            ms_new, got = clock(lambda: rd.GetRanges([q])[0])
            stats = dict(rd.range_stats)
            ms_old, want = clock(lambda: rd.GetRange(*q))
            assert [(x.Key, x.Value) for x in got] == [(x.Key, x.Value) for x in want]
            ms_b = {n: clock(lambda: rd.GetRanges(qs[n]))[0] for n in batches}
            rd.range_profile = True
            rd.GetRanges([q])
            if r >= a.warm:
                t_new.append(ms_new)
                t_old.append(ms_old)
                for n in batches:
                    t_b[n].append(ms_b[n])
                for k in split:
                    split[k].append(rd.range_stats[k])
        med = statistics.median
        say(f"start p{pct:02d} (index {at}): GetRanges 1 query {med(t_new):.3f} ms "
            f"(min {min(t_new):.3f}, max {max(t_new):.3f}) | parent GetRange {med(t_old):.3f} ms "
            f"(min {min(t_old):.3f}, max {max(t_old):.3f}) = x{med(t_old) / med(t_new):.1f} | "
            f"rows {len(got)} stats {stats}")
        say(f"  device split of one query (events): seek {med(split['seek_ms']) * 1e3:.1f} us, "
            f"merges {med(split['merge_ms']) * 1e3:.1f} us, gather {med(split['gather_ms']) * 1e3:.1f} us")
        for n in batches:
            say(f"  GetRanges of {n} queries: {med(t_b[n]):.3f} ms/call = "
                f"{med(t_b[n]) * 1e3 / n:.1f} us/query (min {min(t_b[n]):.3f}, max {max(t_b[n]):.3f})")

    # what a segment keeps resident on either path
    r0, s0 = rd._rows["00"], rd._segs["00"]
    raw = rd._bytes["00"][0]
    h = s0.h
    host = sum(x.nbytes for x in (h.key_arena, h.val_arena, h.key_off, h.key_len, h.val_off,
                                  h.val_len, h.row_start, h.status) if x is not None)
    say(f"resident bytes, segment 00 ({len(data['00'][0])} file bytes): raw bytes on the device "
        f"{nbytes([raw])} (shared with GetRows) + row index {r0.resident_bytes()} "
        f"({r0.resident_bytes() / max(r0.n, 1):.1f} B/row), no host copy | DeviceSegment: device "
        f"{nbytes(s0.t.values())} + host {host}")

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")
    enc.close()
    dec.close()


if __name__ == "__main__":
    main()
