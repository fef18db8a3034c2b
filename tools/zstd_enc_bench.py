#!/usr/bin/env python3
"""zstd_enc_bench.py -- the device zstd encoder (OKV_F_ZSTD_NATIVE) against
libzstd level 1 on the CPU.

Needs an MI355X: it fails without one.  okv_encode_rows on device pointers is timed by
device events on the context's stream after warm-up (the call synchronises with the host
between its stages, so this is the call's whole duration); the stage split is
okv_encode_profile_read's (cut | pack into the raw image | zstd stage: unit kernel, raw
checksums, sizes, placement, block hashes | meta block).

  (a) CZ rows: --blocks (16 384) blocks of 64 KiB, text-like values (tools/zstd_gen.py's
      corpus and row shape), T = 57 344, D = 65 536
  (b) 100 000 fixed rows (16-byte keys, 64-byte generated values) at T = 3 584, D = 4 096
  CPU: the same raw blocks through oracle/zstd_ref.compress level 1 on 1 and 16 threads
      (libzstd releases the GIL inside ctypes calls), --cpu-blocks of them

Reported: GiB/s of raw bytes, output ratio (sum of CompressedSize / sum of OriginalSize),
and the uncompressed encode of the same rows beside it.

--huffman adds the encoder with Huffman-coded literals (OKV_F_ZSTD_HUFFMAN) as
a third arm beside the other two, in the same session, and a third row set:
  (c) 400 000 text rows (ASCII keys, JSON-like values: no byte above 128, which the
      Huffman arm needs; the keys of (a) and the values of (b) hold random bytes) at
      T = 57 344, D = 65 536
--huffman-fse adds the encoder with FSE-compressed Huffman weights (OKV_F_ZSTD_HUF_FSE,
DESIGN.md 27) as a further arm, and row set (c) too.
--no-cpu leaves the libzstd runs out.

Run from the repository root:  python tools/zstd_enc_bench.py [--blocks N] [--huffman]
                                      [--huffman-fse] [--no-cpu] [--log PATH]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import objectkv_amd as okv  # noqa: E402
from objectkv_amd import _lib  # noqa: E402
from oracle import zstd_ref as Z  # noqa: E402
from tools.zstd_gen import _corpus  # noqa: E402

OUT = []
GIB = float(1 << 30)


def say(line):
    print(line, flush=True)
    OUT.append(line)


def cz_rows(nblocks, seed=5, threshold=57344):
    """tools/zstd_gen.text_zstd_segment's rows as SoA arrays, and each block's raw bytes."""
    rng = np.random.default_rng(seed)
    corpus = _corpus(rng)
    keys, vals, blocks = [], [], []
    row = 0
    for _ in range(nblocks):
        recs, raw = [], 0
        while raw < threshold:
            vl = int(rng.integers(0, 4097))
            vo = int(rng.integers(0, len(corpus) - vl))
            key = row.to_bytes(8, "big") + rng.bytes(8)
            val = corpus[vo:vo + vl]
            keys.append(key)
            vals.append(val)
            recs.append(len(key).to_bytes(2, "little") + vl.to_bytes(4, "little") + key + val)
            raw += 6 + len(key) + vl
            row += 1
        blocks.append(b"".join(recs))
    kl = np.full(len(keys), 16, np.uint16)
    vl = np.array([len(v) for v in vals], np.uint32)
    ko = np.arange(len(keys), dtype=np.uint64) * 16
    vo = np.zeros(len(vals), np.uint64)
    vo[1:] = np.cumsum(vl[:-1], dtype=np.uint64)
    r = dict(key_arena=np.frombuffer(b"".join(keys) + bytes(16), np.uint8), key_off=ko, key_len=kl,
             val_arena=np.frombuffer(b"".join(vals) + bytes(16), np.uint8), val_off=vo, val_len=vl)
    return r, blocks


def text_rows(n):
    """ASCII keys and JSON-like values as SoA arrays, and the raw bytes of blocks cut at 57 344."""
    keys = [b"key%09d" % (3 * i) for i in range(n)]
    vals = [b'{"id":%d,"name":"user%d","score":%d,"active":%s,"note":"%s"}' %
            (100000 + 7 * i, 5000 + i, (i * 37) % 1000, b"true" if i % 3 else b"false",
             b"lorem ipsum dolor sit amet "[:i % 28]) for i in range(n)]
    kl = np.array([len(k) for k in keys], np.uint16)
    vl = np.array([len(v) for v in vals], np.uint32)
    ko, vo = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    ko[1:] = np.cumsum(kl[:-1], dtype=np.uint64)
    vo[1:] = np.cumsum(vl[:-1], dtype=np.uint64)
    r = dict(key_arena=np.frombuffer(b"".join(keys) + bytes(16), np.uint8), key_off=ko, key_len=kl,
             val_arena=np.frombuffer(b"".join(vals) + bytes(16), np.uint8), val_off=vo, val_len=vl)
    blocks, cur = [], []
    size = 0
    for k, v in zip(keys, vals):
        cur.append(len(k).to_bytes(2, "little") + len(v).to_bytes(4, "little") + k + v)
        size += 6 + len(k) + len(v)
        if size >= 57344:
            blocks.append(b"".join(cur))
            cur, size = [], 0
    if cur:
        blocks.append(b"".join(cur))
    return r, blocks


def to_dev(r):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint16): np.int16,
              np.dtype(np.uint32): np.int32}
    t = {k: torch.from_numpy(v.view(signed.get(v.dtype, v.dtype)).copy()).cuda()
         for k, v in r.items()}
    torch.cuda.synchronize()
    return t


def timed(enc, fn, warm=2, reps=5):
    stream = torch.cuda.ExternalStream(enc.stream)
    ms = []
    for i in range(warm + reps):
        with torch.cuda.stream(stream):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return ms


def device_case(enc, tag, t, n, T, D, kab, vab, huffman=False, huffman_fse=False):
    res = {}
    arms = [("uncompressed", okv.sst.COMP_NONE, False, False, False),
            ("zstd_native", okv.sst.COMP_ZSTD, True, False, False)]
    if huffman:
        arms.append(("zstd_native+huffman", okv.sst.COMP_ZSTD, True, True, False))
    if huffman_fse:
        arms.append(("zstd_native+huffman+fse", okv.sst.COMP_ZSTD, True, True, True))
    for name, comp, zn, zh, zf in arms:
        kw = dict(key_arena_bytes=kab, val_arena_bytes=vab)
        if zh:  # (named only here: the tool also times builds from before the flag)
            kw["zstd_huffman"] = True
        if zf:
            kw["zstd_huffman_fse"] = True
        try:
            enc.encode_device(t, n, {}, T, D, comp, False, zstd_native=zn, **kw)
        except okv.OkvError as e:
            assert e.code == _lib.OKV_E_CAPACITY
            need = e.out
        nb = int(need.n_blocks)
        out = {"seg": torch.empty(int(need.file_bytes) + 64, dtype=torch.uint8, device="cuda"),
               "desc": torch.empty((nb, 4), dtype=torch.int64, device="cuda")}
        eo = [None]

        def run():
            eo[0] = enc.encode_device(t, n, out, T, D, comp, False, zstd_native=zn, **kw)
        ms = timed(enc, run)
        enc.profile(True)
        enc.profile_reset_encode()
        for _ in range(3):
            run()
        stage, calls = enc.profile_read_encode()
        enc.profile(False)
        d = out["desc"].cpu().numpy().view(np.uint64)
        raw, cs = int(d[:, 2].sum()), int(d[:, 3].sum())
        med = statistics.median(ms)
        say(f"{tag} {name}: {med:.3f} ms/call (min {min(ms):.3f}, max {max(ms):.3f}, n={len(ms)}) "
            f"blocks={nb} raw={raw} B -> {raw / GIB / (med / 1e3):.2f} GiB/s of raw bytes; "
            f"CompressedSize/OriginalSize={cs / raw if zn else 1.0:.4f} "
            f"file={int(eo[0].file_bytes)} B")
        say(f"{tag} {name} stages (ms/call over {calls}): " +
            " ".join(f"{k}={v / max(calls, 1):.3f}" for k, v in stage.items()) +
            ("  [hash = the zstd stage]" if zn else ""))
        res[name] = med
    return res


def cpu_case(tag, blocks):
    raw = sum(len(b) for b in blocks)
    for threads in (1, 16):
        t0 = time.perf_counter()
        if threads == 1:
            sizes = [len(Z.compress(b, 1)) for b in blocks]
        else:
            with ThreadPoolExecutor(threads) as ex:
                sizes = list(ex.map(lambda b: len(Z.compress(b, 1)), blocks))
        dt = time.perf_counter() - t0
        say(f"{tag} libzstd level 1, {threads} thread(s): {len(blocks)} blocks, {raw} B in "
            f"{dt * 1e3:.1f} ms -> {raw / GIB / dt:.3f} GiB/s; ratio {sum(sizes) / raw:.4f}")
    s3 = sum(len(Z.compress(b, 3)) for b in blocks[:256])
    say(f"{tag} libzstd level 3 ratio over the first {min(256, len(blocks))} blocks: "
        f"{s3 / sum(len(b) for b in blocks[:256]):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--cpu-blocks", type=int, default=2048)
    ap.add_argument("--huffman", action="store_true")
    ap.add_argument("--huffman-fse", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zstd_enc_bench.py needs a GPU: nothing is measured without one")
    enc = okv.Encoder(0)
    say(f"device: {torch.cuda.get_device_name(0)}; unit {_lib.ZSTD_ENC_UNIT} B")
    # ---- (a) ----
    r, blocks = cz_rows(a.blocks)
    t = to_dev(r)
    device_case(enc, f"(a) CZ rows x{a.blocks}", t, int(r["key_len"].size), 57344, 65536,
                int(r["key_arena"].size), int(r["val_arena"].size), a.huffman, a.huffman_fse)
    if not a.no_cpu:
        cpu_case("(a)", blocks[:a.cpu_blocks])
    del t, r
    # ---- (b) ----
    n = 100_000
    t = dict(key_arena=torch.empty(n * 16, dtype=torch.uint8, device="cuda"),
             key_off=torch.empty(n, dtype=torch.int64, device="cuda"),
             key_len=torch.empty(n, dtype=torch.int16, device="cuda"),
             val_arena=torch.empty(n * 64, dtype=torch.uint8, device="cuda"),
             val_off=torch.empty(n, dtype=torch.int64, device="cuda"),
             val_len=torch.empty(n, dtype=torch.int32, device="cuda"))
    enc.synth_fixed_device(1, 0, n, 16, 64, t)
    device_case(enc, "(b) 100 000 fixed rows", t, n, 3584, 4096, n * 16, n * 64, a.huffman,
                a.huffman_fse)
    if not a.no_cpu:
        ka, va = t["key_arena"].cpu().numpy(), t["val_arena"].cpu().numpy()
        recs = [b"\x10\x00\x40\x00\x00\x00" + ka[16 * i:16 * i + 16].tobytes() +
                va[64 * i:64 * i + 64].tobytes() for i in range(n)]
        cpu_case("(b)", [b"".join(recs[i:i + 42]) for i in range(0, n, 42)])
    # ---- (c) ----
    if a.huffman or a.huffman_fse:
        del t
        r, blocks = text_rows(400_000)
        t = to_dev(r)
        device_case(enc, "(c) 400 000 text rows", t, int(r["key_len"].size), 57344, 65536,
                    int(r["key_arena"].size), int(r["val_arena"].size), a.huffman, a.huffman_fse)
        if not a.no_cpu:
            cpu_case("(c)", blocks[:a.cpu_blocks])
    enc.close()
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            fh.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
