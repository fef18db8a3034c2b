#!/usr/bin/env python3
"""bloom_bench.py -- the device bloom filter against the host Add loop.

Needs an MI355X: it fails without one.  Every device step is timed by device
events on the context's stream after warm-up; the arms of a comparison
alternate in this one process.  Reported per step: the median microseconds per
call, rows/s and the add form taken (okv_bloom_last_path).

  (a) 100 000 Zipf keys of 8-256 bytes into the default filter
      (NewWithEstimates(100 000, 1e-6)): both forced forms, plus the same at
      smaller row counts (the automatic rule's threshold)
  (b) N = 10^8 16-byte keys (okv_synth_rows_fixed) into the default filter: LDS form
  (c) the same rows into with_estimates(N, 1e-6): global form
  (d) test_rows on 10^7 keys against (a)'s filter: non-members, and members
  (e) encode_device of (b)'s rows: filter bytes from the host (today) against
      add_rows + write_to + OKV_F_BLOOM_DEVICE; outputs compared equal
  CPU: tools/bloom_cpu_bench (tools/build_bloom_bench.sh) over (a)'s and (b)'s
      keys on 1 and 16 threads

Run from the repository root:  python tools/bloom_bench.py [--rows N] [--log PATH]
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import _lib  # noqa: E402
from objectkv_amd.bloom import DeviceBloom, estimate  # noqa: E402

PATH = {0: "none", _lib.BLOOM_PATH_LDS: "lds", _lib.BLOOM_PATH_GLOBAL: "global"}
OUT = []


def say(line):
    print(line, flush=True)
    OUT.append(line)


def zipf_keys(n, seed=3, lo=8, hi=256, s=1.1):
    """Key length L in [lo, hi] with P(L) ~ (L - lo + 1)^-s; key = 8-byte
    big-endian row index + random bytes (the C3 key shape of oracle/pyoracle.py)."""
    rng = np.random.default_rng(seed)
    p = np.arange(1, hi - lo + 2, dtype=np.float64) ** (-s)
    kl = (lo + rng.choice(hi - lo + 1, n, p=p / p.sum())).astype(np.uint16)
    ko = np.zeros(n, np.uint64)
    ko[1:] = np.cumsum(kl[:-1], dtype=np.uint64)
    ka = rng.integers(0, 256, int(kl.sum()) + 16, np.uint8)
    idx = np.arange(n, dtype=">u8").view(np.uint8).reshape(n, 8)
    for b in range(8):
        ka[ko + np.uint64(b)] = idx[:, b]
    return dict(key_arena=ka, key_off=ko, key_len=kl)


def to_dev(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16}
    t = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
         for k, v in r.items()}
    torch.cuda.synchronize()
    return t


class Clock:
    """Device events on the context's stream."""

    def __init__(self, enc):
        self.enc = enc
        self.stream = torch.cuda.ExternalStream(enc.stream)

    def us(self, fn, pre=None):
        with torch.cuda.stream(self.stream):
            if pre:
                pre()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
        return a.elapsed_time(b) * 1e3

    def arms(self, arms: dict, warm=2, reps=7):
        """{name: (fn, pre)} alternated -> {name: [us, ...]}"""
        for _ in range(warm):
            for fn, pre in arms.values():
                self.us(fn, pre)
        t = {k: [] for k in arms}
        for _ in range(reps):
            for k, (fn, pre) in arms.items():
                t[k].append(self.us(fn, pre))
        return t


def report(tag, rows, t, path=""):
    med = statistics.median(t)
    say(f"{tag}: {med:.1f} us/call (min {min(t):.1f}, max {max(t):.1f}, n={len(t)}) "
        f"rows={rows} rows/s={rows / med * 1e6:.4g}" + (f" path={path}" if path else ""))
    return med


def popcount(b: bytes) -> int:
    return int(np.unpackbits(np.frombuffer(b, np.uint8)[24:]).sum())


def cpu(args):
    exe = os.path.join(ROOT, "tools", "bloom_cpu_bench")
    if not os.path.exists(exe):
        say("cpu baseline: tools/bloom_cpu_bench not built (tools/build_bloom_bench.sh): not measured")
        return None
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True)
    say(out.stdout.strip())
    return int(out.stdout.split("popcount=")[1].split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10**8, help="rows of (b), (c) and (e)")
    ap.add_argument("--probes", type=int, default=10**7)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bloom_bench.py needs a GPU: nothing is measured without one")
    enc = okv.Encoder(0)
    clk = Clock(enc)
    say(f"device: {torch.cuda.get_device_name(0)}")
    m, k = estimate(100_000, 1e-6)
    LDS, GLB = _lib.BLOOM_FORCE_LDS, _lib.BLOOM_FORCE_GLOBAL

    # ---- (a) ----
    zr = zipf_keys(100_000)
    z = to_dev(zr)
    f = DeviceBloom(enc, m, k)
    for n in (256, 1024, 4096, 16384, 32768, 65536, 100_000):
        arms = {name: ((lambda form=form: f.add_rows(z, n_rows=n, form=form, sync=False)),
                       f.clear) for name, form in (("lds", LDS), ("global", GLB))}
        t = clk.arms(arms)
        for name in arms:
            report(f"(a) add default filter m={m} k={k}, zipf keys, forced {name}", n, t[name], name)
    f.clear().add_rows(z)
    say(f"(a) automatic form at 100000 rows: {PATH[f.last_path()]}")
    fa = f.to_bytes()
    with tempfile.NamedTemporaryFile(suffix=".keys") as kf:
        kf.write(np.array([100_000, zr["key_arena"].size], np.uint64).tobytes())
        kf.write(zr["key_off"].tobytes() + zr["key_len"].tobytes() + zr["key_arena"].tobytes())
        kf.flush()
        for th in (1, 16):
            pc = cpu(["file", kf.name, m, k, th])
            if pc is not None:
                assert pc == popcount(fa), "device and CPU filters differ"

    # ---- (d) ----
    P = a.probes
    out = torch.zeros(P, dtype=torch.uint8, device="cuda")
    non = dict(key_arena=torch.zeros(16 * P, dtype=torch.uint8, device="cuda"),
               key_off=torch.zeros(P, dtype=torch.int64, device="cuda"),
               key_len=torch.zeros(P, dtype=torch.int16, device="cuda"))
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    enc.synth_fixed_device(1, 10**9, P, 16, 0, dict(non, val_arena=empty,
                                                    val_off=torch.zeros(P, dtype=torch.int64, device="cuda"),
                                                    val_len=torch.zeros(P, dtype=torch.int32, device="cuda")))
    rep = (P + 99_999) // 100_000
    mem = dict(key_arena=z["key_arena"], key_off=z["key_off"].repeat(rep)[:P].contiguous(),
               key_len=z["key_len"].repeat(rep)[:P].contiguous())
    torch.cuda.synchronize()
    t = clk.arms({"non": (lambda: f.test_rows(non, out=out, sync=False), None),
                  "mem": (lambda: f.test_rows(mem, out=out, sync=False), None)})
    report("(d) test_rows, 16-byte non-members (early exit)", P, t["non"])
    report("(d) test_rows, zipf members (all k probes)", P, t["mem"])
    assert bool(out.all()), "a member tested absent"
    del non, mem, out

    # ---- (b), (c), (e) ----
    N = a.rows
    rows = dict(key_arena=torch.zeros(16 * N, dtype=torch.uint8, device="cuda"),
                key_off=torch.zeros(N, dtype=torch.int64, device="cuda"),
                key_len=torch.zeros(N, dtype=torch.int16, device="cuda"),
                val_arena=torch.zeros(64 * N, dtype=torch.uint8, device="cuda"),
                val_off=torch.zeros(N, dtype=torch.int64, device="cuda"),
                val_len=torch.zeros(N, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    enc.synth_fixed_device(1, 0, N, 16, 64, rows)
    fb = DeviceBloom(enc, m, k)
    t = clk.arms({"lds": (lambda: fb.add_rows(rows, n_rows=N, form=LDS, sync=False), fb.clear)},
                 reps=5)
    report(f"(b) add default filter, {N} 16-byte keys, forced lds", N, t["lds"], "lds")
    # what the per-slice recompute costs: the same rows into a one-slice filter
    f1 = DeviceBloom(enc, 2**20, k)
    t = clk.arms({"lds": (lambda: f1.add_rows(rows, n_rows=N, form=LDS, sync=False), f1.clear)},
                 reps=5)
    report(f"(b) add one-slice filter m=2^20 k={k}, {N} 16-byte keys, forced lds", N, t["lds"], "lds")
    f1.close()
    fb.clear().add_rows(rows, n_rows=N)
    say(f"(b) automatic form: {PATH[fb.last_path()]}")
    bb = fb.to_bytes()
    for th in (1, 16):
        pc = cpu(["fixed", N, m, k, th])
        if pc is not None:
            assert pc == popcount(bb), "device and CPU filters differ"
    mc, kc = estimate(N, 1e-6)
    fc = DeviceBloom(enc, mc, kc)
    t = clk.arms({"global": (lambda: fc.add_rows(rows, n_rows=N, sync=False), fc.clear)},
                 warm=1, reps=3)
    report(f"(c) add with_estimates({N}, 1e-6) m={mc} k={kc} ({fc.write_to_bytes} B), automatic",
           N, t["global"], PATH[fc.last_path()])
    say(f"(c) atomic ORs per second: {N * kc / statistics.median(t['global']) * 1e6:.4g}")
    fc.close()

    try:
        enc.encode_device(rows, N, {"seg": None}, bloom=bb)
    except okv.OkvError as e:
        need = int(e.out.file_bytes)
    segs = [torch.zeros(need + 4096, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()

    def host_arm():
        enc.encode_device(rows, N, {"seg": segs[0]}, bloom=bb)

    def dev_arm():
        fb.clear()
        enc.encode_device(rows, N, {"seg": segs[1]}, bloom=fb)

    t = clk.arms({"host": (host_arm, None), "device": (dev_arm, None)}, warm=1, reps=3)
    report(f"(e) encode_device, {N} rows, filter bytes from the host", N, t["host"])
    report("(e) encode_device, add_rows + write_to + OKV_F_BLOOM_DEVICE", N, t["device"],
           PATH[fb.last_path()])
    same = bool(torch.equal(segs[0][:need], segs[1][:need]))
    say(f"(e) outputs equal: {same} ({need} bytes)")
    assert same
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")
    fb.close()
    f.close()
    enc.close()


if __name__ == "__main__":
    main()
