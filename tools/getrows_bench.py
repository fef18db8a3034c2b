#!/usr/bin/env python3
"""getrows_bench.py -- the batched GetRow (okv_get_rows) against the loop of single-key
GetRow calls it replaces.

Needs an MI355X: it fails without one.  The batched call is timed by device events on
the context's stream (device pointers, OKV_F_ASYNC) after warm-up, the median of 7
calls; the single-key loop (okv_reader_get_row, the only way before this call) by the
host clock over --loop keys, in this same process.

  segment: --rows OKV_SYNTH_FIXED rows (16-byte keys: 8 zero bytes + the big-endian row
           index, so every first key shares its 8-byte prefix and each search step
           falls through to the byte compare; 64-byte values), in 4 KiB blocks and in
           64 KiB blocks, resident on the device
  keys:    1, 10, 100 (where the call overtakes the loop), 10^3, 10^5, 10^7; uniform
           and Zipf (s = 1.1) over the rows; members, and non-members (a member plus
           one byte: the same floor block, absent)
  filter:  none, and the default filter (NewWithEstimates(100 000, 1e-6)) holding
           every row key
The CPU restatement's GetRow on 1 and 16 threads is tools/getrows_cpu_bench
(tools/build_getrows_cpu_bench.sh), run beside this tool in the same session.
Reported per line: microseconds per call, keys/s, blocks_searched, and the bytes read
(blocks_searched x BlockSize) per key.

Run from the repository root:  python tools/getrows_bench.py [--log PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import _lib, get as G  # noqa: E402
from objectkv_amd import reader as R  # noqa: E402
from objectkv_amd.bloom import DeviceBloom, estimate  # noqa: E402

OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def keys_of(idx, extra=False):
    """Row indices -> the key arrays (numpy): 8 zero bytes + big-endian index (+ 0x01)."""
    n, w = idx.size, 17 if extra else 16
    ka = np.zeros((n, w), np.uint8)
    ka[:, 8:16] = idx.astype(">u8").view(np.uint8).reshape(n, 8)
    if extra:
        ka[:, 16] = 1
    return dict(key_arena=np.concatenate([ka.reshape(-1), np.zeros(16, np.uint8)]),
                key_off=np.arange(n, dtype=np.uint64) * np.uint64(w),
                key_len=np.full(n, w, np.uint16))


def to_dev(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    t = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
         for k, v in r.items()}
    torch.cuda.synchronize()
    return t


def outputs(n, arena=0):
    z = lambda dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    o = {"state": z(torch.int32), "blk_status": z(torch.int32), "entry": z(torch.int32),
         "val_off": z(torch.int64), "val_len": z(torch.int32), "val_pos": z(torch.int64)}
    if arena:
        o["val_arena"] = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    return o


def timed(dec, stream, fn, warm=2, reps=7):
    t = []
    with torch.cuda.stream(stream):
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                t.append(a.elapsed_time(b) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--loop", type=int, default=3000, help="keys of the single-key loop")
    ap.add_argument("--sizes", default="1,10,100,1000,100000,10000000")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("getrows_bench.py needs a GPU: nothing is measured without one")
    dec = okv.Decoder(0)
    stream = torch.cuda.ExternalStream(dec.stream)
    say(f"device: {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(7)
    sizes = [int(x) for x in a.sizes.split(",")]
    m, k = estimate(100_000, 1e-6)
    single = {}

    for th, bs in ((3584, 4096), (57344, 65536)):
        w = okv.synth_segment(okv.sst.SYNTH_FIXED, 1, nrows=a.rows, threshold=th, block_size=bs)
        data = w.data().tobytes()
        md = okv.bytes_to_metadata(w.meta())
        nblk = md.descs.shape[0]
        seg = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
        ix = okv.DeviceIndex.from_metadata(dec, md)
        bl = DeviceBloom(dec, m, k).add_rows(keys_of(np.arange(a.rows, dtype=np.uint64)))
        say(f"segment: {a.rows} rows, BlockSize {bs}, {nblk} blocks, {len(data)} bytes; "
            f"filter m={m} k={k}")

        # the parent's way: one okv_reader_get_row per key
        rd = R.SegmentReader(data, len(data), dec)
        rd.FetchAndLoadMetadata()
        L = _lib.lib()
        lk = keys_of(rng.integers(0, a.rows, a.loop).astype(np.uint64))
        kb = [lk["key_arena"][16 * i:16 * i + 16].tobytes() for i in range(a.loop)]
        row = _lib.Row()
        for kk in kb[:200]:
            L.okv_reader_get_row(rd._h, kk, 16, C.byref(row))
        t0 = time.perf_counter()
        for kk in kb:
            rc = L.okv_reader_get_row(rd._h, kk, 16, C.byref(row))
            assert rc == 0
        us = (time.perf_counter() - t0) * 1e6 / a.loop
        single[bs] = us
        say(f"single-key loop (okv_reader_get_row, members, no filter), BlockSize {bs}: "
            f"{us:.2f} us/key = {1e6 / us:.4g} keys/s over {a.loop} keys")
        t0 = time.perf_counter()
        got = rd.GetRows(kb)
        us_b = (time.perf_counter() - t0) * 1e6 / a.loop
        assert all(isinstance(g, R.KVPair) for g in got)
        say(f"reader GetRows (host arrays, first call uploads the storage), BlockSize {bs}: "
            f"{us_b:.2f} us/key over {a.loop} keys")

        for n in sizes:
            uni = rng.integers(0, a.rows, n).astype(np.uint64)
            zipf = np.minimum(rng.zipf(1.1, n) - 1, a.rows - 1).astype(np.uint64)
            for dist, idx in (("uniform", uni), ("zipf", zipf)):
                for member in (True, False):
                    dk = to_dev(keys_of(idx, extra=not member))
                    out = outputs(n)
                    kab = int(dk["key_arena"].numel())
                    for filt in (None, bl):
                        def call():
                            G.get_rows(dec, seg, len(data), ix, dk, bloom=filt, out=out,
                                       sync=False, n_rows=n, key_arena_bytes=kab)
                        t = timed(dec, stream, call)
                        dec.sync()
                        tot = G.totals(dec)
                        med = statistics.median(t)
                        assert tot["n_found"] == (n if member else 0), tot
                        per_key = tot["blocks_searched"] * bs / n
                        say(f"get_rows BlockSize {bs} n={n} {dist} "
                            f"{'members' if member else 'non-members'} "
                            f"filter={'default' if filt else 'none'}: {med:.1f} us/call "
                            f"(min {min(t):.1f}, max {max(t):.1f}) keys/s={n / med * 1e6:.4g} "
                            f"blocks_searched={tot['blocks_searched']} "
                            f"block bytes/key={per_key:.1f} "
                            f"vs single-key loop x{single[bs] * n / med:.1f}")
                    del dk, out
        # with the value arena, the largest uniform member batch
        n = sizes[-1]
        dk = to_dev(keys_of(rng.integers(0, a.rows, n).astype(np.uint64)))
        out = outputs(n, arena=64 * n)
        kab = int(dk["key_arena"].numel())
        t = timed(dec, stream, lambda: G.get_rows(dec, seg, len(data), ix, dk, out=out, sync=False,
                                                  n_rows=n, key_arena_bytes=kab), reps=5)
        dec.sync()
        tot = G.totals(dec)
        med = statistics.median(t)
        say(f"get_rows + values BlockSize {bs} n={n} uniform members filter=none: "
            f"{med:.1f} us/call keys/s={n / med * 1e6:.4g} val_bytes={tot['val_bytes']}")
        del dk, out
        bl.close()
        ix.close()

    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")
    dec.close()


if __name__ == "__main__":
    main()
