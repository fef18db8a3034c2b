#!/usr/bin/env python3
"""split_bench.py -- the range-split encode against the loop of single-segment encodes
(DESIGN.md 28.6).

Needs an MI355X: it fails without one.  Rows: device-resident fixed 16/64-byte records
(okv_synth_rows_fixed, CM's record shape), default thresholds (1 000 000 bytes, 100 000 rows).
Every arm is a call that synchronises with the host inside, so an arm's time is the wall
clock around it, from an idle device to its return; the arms alternate in this one process
after warm-up, and the median, the minimum and the maximum of the repeats are reported.

  (a) okv_encode_split into arenas of the size its size query reports: without filters, and
      with the default filter (bloom.EstimateParameters(100 000, 1e-6)) per segment
  (b) today's way over (a)'s boundaries: one encode_device with Close per segment, plus, in
      the filter case, a DeviceBloom per segment (okv_bloom_new, okv_bloom_add_rows,
      okv_bloom_write_to); every file is compared with (a)'s
  (c) one unsplit okv_encode_rows with OKV_F_NO_CLOSE: the floor the data stage cannot beat

Run from the repository root:  python tools/split_bench.py [--rows N] [--log PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import _lib  # noqa: E402
from objectkv_amd.bloom import DeviceBloom, estimate  # noqa: E402

OUT = []
KL, VL = 16, 64


def say(line):
    print(line, flush=True)
    OUT.append(line)


def synth(enc, n):
    t = {"key_arena": torch.empty(n * KL + 16, dtype=torch.uint8, device="cuda"),
         "key_off": torch.empty(n, dtype=torch.int64, device="cuda"),
         "key_len": torch.empty(n, dtype=torch.int16, device="cuda"),
         "val_arena": torch.empty(n * VL + 16, dtype=torch.uint8, device="cuda"),
         "val_off": torch.empty(n, dtype=torch.int64, device="cuda"),
         "val_len": torch.empty(n, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    enc.synth_fixed_device(1, 0, n, KL, VL, t)
    return t


def wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def arms(table, warm=2, reps=7):
    for _ in range(warm):
        for fn in table.values():
            fn()
    t = {k: [] for k in table}
    for _ in range(reps):
        for k, fn in table.items():
            t[k].append(wall_us(fn))
    return t


def report(tag, t, extra=""):
    med = statistics.median(t)
    say(f"{tag}: median {med / 1e3:.3f} ms (min {min(t) / 1e3:.3f}, max {max(t) / 1e3:.3f}, "
        f"n={len(t)}){extra}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    n = a.rows
    enc = okv.Encoder(0)
    t = synth(enc, n)
    kab, vab = n * KL, n * VL
    m, k = estimate(100_000, 0.000001)
    say(f"rows={n} record=6+{KL}+{VL} default filter m={m} k={k} "
        f"device={torch.cuda.get_device_name(0)}")

    def split(bloom, out):
        return enc.encode_split_device(t, n, out, key_arena_bytes=kab, val_arena_bytes=vab,
                                       bloom=bloom)

    out_plain, out_bloom = {}, {}
    res = {None: split(None, out_plain), (m, k): split((m, k), out_bloom)}
    ns = len(res[None].segments)
    say(f"segments={ns} blocks={res[None].n_blocks} data_bytes={res[None].data_bytes} "
        f"meta_arena_bytes={res[None].meta_arena_bytes} (with filters "
        f"{res[(m, k)].meta_arena_bytes})")

    # (a) the call alone, outputs preallocated (the wrapper's size query is not part of it)
    def raw_split(bloom, out):
        R = _lib.Rows(*(t[x].data_ptr() for x in ("key_arena", "key_off", "key_len",
                                                  "val_arena", "val_off", "val_len")),
                      n, kab, vab)
        o = _lib.EncodeOpts(3584, 4096, 0, 0, None, 0)
        so = _lib.SplitOpts(1_000_000, 100_000, *(bloom or (0, 0)))
        words = C.sizeof(_lib.SplitSeg) // 8
        q = _lib.SplitOut(out["data"].data_ptr(), out["data"].numel(), out["meta"].data_ptr(),
                          out["meta"].numel(), out["segs"].data_ptr(),
                          out["segs"].numel() // words, None, None, None, 0)

        def go():
            rc = _lib.lib().okv_encode_split(enc._ctx, C.byref(R), C.byref(o), C.byref(so),
                                             C.byref(q), _lib.F_DEVICE_PTRS)
            assert rc == 0, rc
        return go

    # (b) one encode_device with Close per segment, over the same boundaries
    seg_buf = torch.empty(max(g.file_bytes for g in res[(m, k)].segments) + 64,
                          dtype=torch.uint8, device="cuda")

    def slice_rows(g):
        r0, r1 = g.first_row, g.first_row + g.n_rows
        return {"key_arena": t["key_arena"], "val_arena": t["val_arena"],
                "key_off": t["key_off"][r0:r1], "key_len": t["key_len"][r0:r1],
                "val_off": t["val_off"][r0:r1], "val_len": t["val_len"][r0:r1]}

    def loop(bloom, check=False):
        def go():
            for s, g in enumerate(res[bloom].segments):
                f = DeviceBloom(enc, *bloom) if bloom else None
                eo = enc.encode_device(slice_rows(g), g.n_rows, {"seg": seg_buf},
                                       strict_go=False, key_arena_bytes=kab,
                                       val_arena_bytes=vab, bloom=f)
                if check:
                    r = res[bloom]
                    assert int(eo.file_bytes) == g.file_bytes
                    assert torch.equal(seg_buf[:g.data_bytes],
                                       r.data[g.data_off:g.data_off + g.data_bytes]), s
                    assert torch.equal(seg_buf[g.data_bytes:g.file_bytes],
                                       r.meta[g.meta_off:g.meta_off + g.meta_bytes + 25]), s
                if f is not None:
                    f.close()
        return go

    loop(None, check=True)()
    loop((m, k), check=True)()
    say(f"(b)'s {ns} files equal (a)'s, without and with filters")

    # (c) the unsplit data stage
    one = {"seg": torch.empty(res[None].data_bytes + res[None].n_blocks * 64 + 4096,
                              dtype=torch.uint8, device="cuda")}

    def unsplit():
        enc.encode_device(t, n, one, strict_go=False, close=False, key_arena_bytes=kab,
                          val_arena_bytes=vab)

    tm = arms({"a": raw_split(None, out_plain), "a_bloom": raw_split((m, k), out_bloom),
               "b": loop(None), "b_bloom": loop((m, k)), "c": unsplit})
    ma = report("(a) okv_encode_split, no filters", tm["a"])
    mab = report("(a) okv_encode_split, default filter per segment", tm["a_bloom"])
    mb = report("(b) encode_device + Close per segment", tm["b"])
    mbb = report("(b) the same + okv_bloom_* per segment", tm["b_bloom"])
    mc = report("(c) one unsplit okv_encode_rows, OKV_F_NO_CLOSE", tm["c"])
    say(f"(a) / (c) = {ma / mc:.2f}; (b) / (a) = {mb / ma:.1f}; with filters (b) / (a) = "
        f"{mbb / mab:.1f}")
    say(f"segments per second: (a) {ns / ma * 1e6:.4g}, (a) with filters {ns / mab * 1e6:.4g}, "
        f"(b) {ns / mb * 1e6:.4g}, (b) with filters {ns / mbb * 1e6:.4g}")
    say(f"data bytes per second: (a) {res[None].data_bytes / ma * 1e6 / 2**30:.1f} GiB/s, "
        f"(c) {res[None].data_bytes / mc * 1e6 / 2**30:.1f} GiB/s")
    enc.close()
    if a.log:
        os.makedirs(os.path.dirname(a.log) or ".", exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
