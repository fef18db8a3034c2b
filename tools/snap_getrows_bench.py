#!/usr/bin/env python3
"""snap_getrows_bench.py -- the snapshot GetRows (okv_snap_get_rows) against what a caller
could do before it.

Needs an MI355X: it fails without one.  The batched call is timed by device events on the
context's stream (device pointers, OKV_F_ASYNC) after 2 warm-ups, the median of 7 calls,
as tools/getrows_bench.py does.  In the same process and session:
  (a) one okv_get_rows per segment in GetRow's priority order over the keys still
      unresolved, the state read back and the unresolved keys compacted on the host
      between the calls; the host clock around the whole loop, after one warm-up
  (b) the loop of snapshot.Reader.GetRow over --loop keys, by the host clock

  snapshot: 8 segments, 4 at level 0 and 4 at level 1, of --rows rows each in
            OKV_SYNTH_FIXED's shape (16-byte keys: 8 zero bytes + the big-endian index;
            64-byte values), 4 KiB blocks.  Segment s holds the indices
            15 000 s + 2 j + (s mod 2): the ranges overlap, and a key's candidates are
            half segments that hold it and half segments that do not
  keys:     1, 10^3, 10^5, 10^6 uniform over the union of the ranges; members, and
            non-members (a member plus one byte: the same floor blocks, absent)
  filters:  none, and the default filter (NewWithEstimates(100 000, 1e-6)) per segment
Reported per line: microseconds per call, keys/s, pairs_probed, blocks_searched, and the
two comparisons.

Run from the repository root:  python tools/snap_getrows_bench.py [--log PATH]
"""
from __future__ import annotations

import argparse
import functools
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import _lib, get as G, snap as S  # noqa: E402
from objectkv_amd import snapshot as SN  # noqa: E402
from objectkv_amd.bloom import DeviceBloom, estimate  # noqa: E402
from tools.getrows_bench import keys_of, timed, to_dev  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def segment_rows(idx):
    r = keys_of(idx)
    n = idx.size
    rng = np.random.default_rng(int(idx[0]) + 1)
    r.update(val_arena=rng.integers(0, 256, 64 * n + 16, dtype=np.uint8),
             val_off=np.arange(n, dtype=np.uint64) * np.uint64(64),
             val_len=np.full(n, 64, np.uint32))
    return r


def outputs(n, names):
    dt = {"state": torch.int32, "seg": torch.int32, "blk_status": torch.int32,
          "entry": torch.int32, "val_off": torch.int64, "val_len": torch.int32,
          "val_pos": torch.int64}
    return {k: torch.zeros(n, dtype=dt[k], device="cuda") for k in names}


def per_segment_loop(dec, segs, order, keys, filters):
    """(a): -> found keys.  segs in priority order; keys: the numpy key arrays."""
    n = keys["key_len"].size
    w = int(keys["key_len"][0])
    ka = keys["key_arena"][:n * w].reshape(n, w)
    left = np.arange(n)
    found = 0
    for s in order:
        if left.size == 0:
            break
        t, nbytes, ix, bl = segs[s][:4]
        sub = dict(key_arena=np.concatenate([ka[left].reshape(-1), np.zeros(16, np.uint8)]),
                   key_off=np.arange(left.size, dtype=np.uint64) * np.uint64(w),
                   key_len=np.full(left.size, w, np.uint16))
        dk = to_dev(sub)
        out = outputs(left.size, ("state", "blk_status", "entry", "val_off", "val_len"))
        G.get_rows(dec, t, nbytes, ix, dk, bloom=bl if filters else None, out=out,
                   n_rows=left.size, key_arena_bytes=int(dk["key_arena"].numel()))
        st = out["state"].cpu().numpy()
        found += int((st == _lib.GET_FOUND).sum())
        left = left[st != _lib.GET_FOUND]
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--loop", type=int, default=2000, help="keys of the Reader.GetRow loop")
    ap.add_argument("--sizes", default="1,1000,100000,1000000")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("snap_getrows_bench.py needs a GPU: nothing is measured without one")
    dec = okv.Decoder(0)
    enc = okv.Encoder(0)
    stream = torch.cuda.ExternalStream(dec.stream)
    say(f"device: {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(11)
    m, k = estimate(100_000, 1e-6)
    segs, data = [], {}
    for s in range(8):
        idx = (15000 * s + 2 * np.arange(a.rows) + (s & 1)).astype(np.uint64)
        e = enc.encode(segment_rows(idx))
        raw = e.seg.tobytes()
        md = okv.fetch_metadata(e.seg, e.file_bytes)
        t = torch.frombuffer(bytearray(raw) + bytearray(32), dtype=torch.uint8).cuda()
        ix = okv.DeviceIndex.from_metadata(dec, md)
        bl = DeviceBloom(dec, m, k).add_rows(keys_of(idx))
        sid = f"{s:02d}"
        segs.append((t, len(raw), ix, bl, 0, 0 if s < 4 else 1, sid, md.first_key, md.last_key))
        data[sid] = (raw, e.file_bytes)
    span = 15000 * 7 + 2 * a.rows
    say(f"snapshot: 8 segments (4 L0, 4 L1) of {a.rows} rows, 4 KiB blocks, "
        f"{sum(len(d[0]) for d in data.values())} bytes; indices 0 .. {span}; filter m={m} k={k}")
    snaps = {False: okv.DeviceSnapshot(dec, [x[:3] + (None,) + x[4:] for x in segs]),
             True: okv.DeviceSnapshot(dec, segs)}
    less = lambda x, y: x[5] < y[5] if x[5] != y[5] else x[6] > y[6]  # noqa: E731
    order = sorted(range(8), key=functools.cmp_to_key(
        lambda i, j: -1 if less(segs[i], segs[j]) else 1))

    # (b) the parent's Reader.GetRow, key by key (decoded segments, no filter probe)
    rd = SN.Reader(lambda rec: data[rec.ID], dec)
    rd.UpdateSegments([SN.SegmentRecord(x[6], x[5], x[7], x[8]) for x in segs], None)
    lk = keys_of(rng.integers(0, span, a.loop).astype(np.uint64))
    kb = [lk["key_arena"][16 * i:16 * i + 16].tobytes() for i in range(a.loop)]

    def one(key):
        try:
            return rd.GetRow(key)
        except SN.SnapshotError:
            return None
    for kk in kb[:50]:
        one(kk)
    t0 = time.perf_counter()
    hits = sum(one(kk) is not None for kk in kb)
    us_b = (time.perf_counter() - t0) * 1e6 / a.loop
    say(f"(b) Reader.GetRow loop (members): {us_b:.1f} us/key = {1e6 / us_b:.4g} keys/s over "
        f"{a.loop} keys, {hits} found")
    t0 = time.perf_counter()
    got = rd.GetRows(kb)
    us_r = (time.perf_counter() - t0) * 1e6 / a.loop
    assert sum(not isinstance(g, Exception) for g in got) == hits
    say(f"Reader.GetRows (host arrays, first call uploads the segments and filters): "
        f"{us_r:.1f} us/key over {a.loop} keys")

    for n in [int(x) for x in a.sizes.split(",")]:
        idx = rng.integers(0, span, n).astype(np.uint64)
        for member in (True, False):
            hk = keys_of(idx, extra=not member)
            dk = to_dev(hk)
            kab = int(dk["key_arena"].numel())
            out = outputs(n, ("state", "seg", "blk_status", "entry", "val_off", "val_len"))
            for filt in (False, True):
                def call():
                    S.snap_get_rows(dec, snaps[filt], dk, out=out, sync=False, n_rows=n,
                                    key_arena_bytes=kab)
                t = timed(dec, stream, call)
                dec.sync()
                tot = S.totals(dec)
                med = statistics.median(t)
                per_segment_loop(dec, segs, order, hk, filt)  # warm-up
                t0 = time.perf_counter()
                found_a = per_segment_loop(dec, segs, order, hk, filt)
                us_a = (time.perf_counter() - t0) * 1e6
                t0 = time.perf_counter()
                call()
                dec.sync()
                us_w = (time.perf_counter() - t0) * 1e6
                if member:
                    assert found_a == tot["n_found"], (found_a, tot)
                say(f"snap_get_rows n={n} {'members' if member else 'non-members'} "
                    f"filters={'default' if filt else 'none'}: {med:.1f} us/call "
                    f"(min {min(t):.1f}, max {max(t):.1f}; host clock {us_w:.1f}) "
                    f"keys/s={n / med * 1e6:.4g} found={tot['n_found']} "
                    f"pairs_probed={tot['pairs_probed']} blocks_searched={tot['blocks_searched']} "
                    f"| (a) per-segment okv_get_rows loop {us_a:.1f} us = x{us_a / med:.2f} "
                    f"| (b) Reader.GetRow loop x{us_b * n / med:.1f}")
            del dk, out

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")
    for x in segs:
        x[2].close()
        x[3].close()
    for sn in snaps.values():
        sn.close()
    enc.close()
    dec.close()


if __name__ == "__main__":
    main()
