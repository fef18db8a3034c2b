#!/usr/bin/env python3
"""getrows_zstd_bench.py -- GetRows on zstd segments (OKV_F_GET_ZSTD).

Needs an MI355X: it fails without one.  Every figure is the median of 7 rounds after 2
warm-ups, but the single-key loop's, which is the median of 3 after 1 over at most
--loop-max keys (each key is a whole zstd block decode with its host round trips).

  arm 1  SegmentReader.GetRows(keys) (host arrays in, rows out; the host clock, as a
         caller sees it) against the loop of single-key GetRow calls over the same keys
         -- which is what GetRows was for a zstd segment before this flag; --loop-only
         prints just the loop, so the same tool run from an older tree gives its side of
         an alternating comparison.
  arm 2  okv_get_rows with the flag on the zstd segment against okv_get_rows on the same
         rows uncompressed (device pointers, values included; device events around the
         call, which synchronises inside): what the inflate costs.

  segments: --rows rows (a 16-byte key, a text value of 40 to 120 bytes), cut at 4 KiB
            and at 256 KiB of raw bytes per block
  keys:     1, 16, 1 000 and 100 000 uniform row keys

Run from the repository root:  python tools/getrows_zstd_bench.py [--log PATH]
"""
from __future__ import annotations

import argparse
import os
import random
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
from objectkv_amd.bloom import pack_keys  # noqa: E402
from oracle import zstd_ref as Z  # noqa: E402

LOG = None  # --log: every line is appended as it is measured
WORDS = [b"alpha", b"beta", b"gamma", b"delta", b"kv", b"segment", b"block", b"zstd"]


def say(line):
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as fh:
            fh.write(line + "\n")


def median_us(fn, warm=2, reps=7):
    t = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t), min(t), max(t)


def to_dev(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    t = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
         for k, v in r.items()}
    torch.cuda.synchronize()
    return t


def outputs(n, arena):
    z = lambda dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    return {"state": z(torch.int32), "blk_status": z(torch.int32), "entry": z(torch.int32),
            "val_off": z(torch.int64), "val_len": z(torch.int32), "val_pos": z(torch.int64),
            "val_arena": torch.zeros(arena, dtype=torch.uint8, device="cuda")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--sizes", default="1,16,1000,100000")
    ap.add_argument("--loop-max", type=int, default=300, help="keys the single-key loop times")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log:
        global LOG
        LOG = a.log
        os.makedirs(os.path.dirname(os.path.abspath(LOG)), exist_ok=True)
        open(LOG, "w").close()
    if not torch.cuda.is_available():
        sys.exit("getrows_zstd_bench.py needs a GPU: nothing is measured without one")
    dec = okv.Decoder(0)
    say(f"device: {torch.cuda.get_device_name(0)}")
    rng = random.Random(11)
    rows = [(b"key-%012d" % i, b" ".join(rng.choice(WORDS) for _ in range(rng.randint(8, 20))))
            for i in range(a.rows)]
    sizes = [int(x) for x in a.sizes.split(",")]
    nrng = np.random.default_rng(5)
    batches = {n: [rows[int(i)][0] for i in nrng.integers(0, a.rows, n)] for n in sizes}

    for th in (3584, 262144):
        zseg, zlen, zmeta = Z.zstd_segment(rows, th, 4096)
        # (uncompressed blocks over 64 KiB are FALLBACK: the 4 KiB cut is the comparison)
        w = okv.SegmentWriter(3584, 4096)
        for k, v in rows:
            w.WriteRow(k, v)
        _flen, pmeta = w.Close()
        pseg = w.data().tobytes()
        zmd, pmd = okv.bytes_to_metadata(zmeta), okv.bytes_to_metadata(pmeta)
        say(f"segment: {a.rows} rows cut at {th} raw bytes: {zmd.descs.shape[0]} zstd blocks, "
            f"{zlen} bytes ({len(pseg)} uncompressed)")

        # ---- arm 1: the reader ------------------------------------------------------
        rd = R.SegmentReader(zseg, zlen, dec)
        rd.FetchAndLoadMetadata()
        for n in sizes:
            ks = batches[n]
            lk = ks[:a.loop_max]
            med, lo, hi = median_us(lambda: [rd.GetRow(k) for k in lk], warm=1, reps=3)
            per = med / len(lk)
            say(f"reader single-key loop cut={th} n={n}: {per:.1f} us/key over {len(lk)} keys "
                f"(so {per * n:.0f} us for the batch; min {lo / len(lk):.1f}, max {hi / len(lk):.1f})")
            if a.loop_only:
                continue
            c0 = rd.io_stats()["calls"]
            med, lo, hi = median_us(lambda: rd.GetRows(ks))
            calls = (rd.io_stats()["calls"] - c0) / 9  # (2 warm-ups + 7 rounds)
            say(f"reader GetRows cut={th} n={n}: {med:.0f} us/batch (min {lo:.0f}, max {hi:.0f}) "
                f"= {med / n:.2f} us/key, {calls:.1f} device calls/batch, "
                f"loop/batched x{per * n / med:.2f}")
        if a.loop_only:
            continue

        # ---- arm 2: the raw call, zstd against uncompressed ---------------------------
        zt = torch.frombuffer(bytearray(zseg) + bytearray(16), dtype=torch.uint8).cuda()
        pt = torch.frombuffer(bytearray(pseg) + bytearray(16), dtype=torch.uint8).cuda()
        zix = okv.DeviceIndex.from_metadata(dec, zmd)
        pix = okv.DeviceIndex.from_metadata(dec, pmd)
        stream = torch.cuda.ExternalStream(dec.stream)
        for n in sizes:
            pk = pack_keys(batches[n])
            dk = to_dev(pk)
            kab = int(pk["key_arena"].size)
            out = outputs(n, 128 * n + 64)
            res = {}
            for name, t, nbytes, ix, comp, flag in (("zstd", zt, zlen, zix, _lib.COMP_ZSTD, True),
                                                    ("none-4KiB", pt, len(pseg), pix, 0, False)):
                ts = []
                with torch.cuda.stream(stream):
                    for i in range(9):
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        G.get_rows(dec, t, nbytes, ix, dk, compression=comp, out=out, sync=False,
                                   n_rows=n, key_arena_bytes=kab, zstd=flag)
                        e1.record()
                        e1.synchronize()
                        if i >= 2:
                            ts.append(e0.elapsed_time(e1) * 1e3)
                dec.sync()
                tot = G.totals(dec)
                assert tot["n_found"] == n and tot["n_fallback"] == 0, tot
                res[name] = statistics.median(ts)
                say(f"get_rows {name} cut={th} n={n}: {res[name]:.1f} us/call "
                    f"(min {min(ts):.1f}, max {max(ts):.1f}) keys/s={n / res[name] * 1e6:.4g} "
                    f"blocks_searched={tot['blocks_searched']} path={dec.last_path()}")
            say(f"get_rows cut={th} n={n}: zstd / uncompressed 4 KiB blocks "
                f"x{res['zstd'] / res['none-4KiB']:.2f}")
            del dk, out
        zix.close()
        pix.close()

    dec.close()


if __name__ == "__main__":
    main()
