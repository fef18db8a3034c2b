"""The CPU model of the device zstd encoder under OKV_F_ZSTD_HUFFMAN: the parse is
tests/zenc_model.parse_unit (phases B-E, unchanged by the flag); the literals decision, the
Huffman section and the Raw / Compressed decision are tests/zenc_huf_main.cpp's, which runs
okv_zstd_enc.hpp's statements with a sequential bit writer and reports per unit what it
chose.  Nothing of the Huffman format is restated here.

Per unit the census (Unit.census) gains: "block" (0 Raw, 2 Compressed), "lit" (0 raw, 2
Huffman), "streams" (1 / 4, 0 without Huffman), "sf" (Size_Format 0 / 2 / 3), "nlit", "nseq",
"huf" (bytes the Huffman section would take, 0 when the symbols rule it out), "raw" (bytes of
the raw section), "bits" (the longest code), "last" (the largest literal value when
eligible), "csz" (the compressed size that was compared with n)."""
from __future__ import annotations

import atexit
import os
import shutil
import struct
import subprocess
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as P
from tests import zenc_model as M

UNIT = M.UNIT
KEYS = ("block", "n", "nlit", "nseq", "lit", "streams", "sf", "huf", "raw", "bits", "last", "csz")


def build_huf_main(out, sanitize):
    """Compiles tests/zenc_huf_main.cpp to `out`; with AddressSanitizer and UBSan when
    `sanitize` (a plain program, CPU tests only), plain -O1 otherwise."""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(
        [M.clang(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", M.CSRC,
         "-I", os.path.join(M.ROOT, "include"),
         os.path.join(M.ROOT, "tests", "zenc_huf_main.cpp"), "-o", out],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return out


_PLAIN = []


def plain_exe():
    """zenc_huf_main without sanitizers, built once per process into a temporary directory."""
    if not _PLAIN:
        d = tempfile.mkdtemp(prefix="zenc_huf_model_")
        atexit.register(shutil.rmtree, d, True)
        _PLAIN.append(build_huf_main(os.path.join(d, "zenc_huf_main"), sanitize=False))
    return _PLAIN[0]


def cases(raw, units, parsed, huffman):
    body = []
    for u, pu in zip(units, parsed):
        lits = pu.literals(u)
        body.append(struct.pack("<I", len(lits)) + lits + struct.pack("<I", len(pu.seqs)) +
                    np.array(pu.seqs, "<u4").tobytes())
    return struct.pack("<QIII", len(raw), P.xxh64(raw) & 0xFFFFFFFF, len(units),
                       1 if huffman else 0) + b"".join(body)


def run_main(exe, tmp, data, args=()):
    """Runs the program over `data`; (output file bytes, stdout)."""
    stem = os.path.join(tmp, f"h{threading.get_ident()}")
    with open(stem + ".bin", "wb") as fh:
        fh.write(data)
    run = subprocess.run([exe, *args, stem + ".bin", stem + ".out"], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:] + run.stderr[-4000:])
    with open(stem + ".out", "rb") as fh:
        return fh.read(), run.stdout


def model(raw, huffman=True, exe=None, tmp=None):
    """(frame, [Unit]) the device encoder is to give for one raw block."""
    exe = exe or plain_exe()
    if tmp is None:
        with tempfile.TemporaryDirectory(prefix="zenc_huf_case_") as d:
            return model(raw, huffman, exe, d)
    raw = bytes(raw)
    units = [raw[i:i + UNIT] for i in range(0, len(raw), UNIT)] or [b""]
    parsed = [M.parse_unit(u) for u in units]
    frame, text = run_main(exe, tmp, cases(raw, units, parsed, huffman))
    lines = [ln.split() for ln in text.splitlines() if ln.startswith("block ")]
    assert len(lines) == len(parsed)
    for ln, pu in zip(lines, parsed):
        got = dict(zip(ln[0::2], (int(x) for x in ln[1::2])))
        assert set(got) == set(KEYS) and got["n"] == pu.n and got["nseq"] == len(pu.seqs)
        pu.census.update(got)
    assert [t for t, _ in M.block_headers(frame, len(raw))] == [p.census["block"] for p in parsed]
    return frame, parsed


def model_frames(raws, huffman=True, exe=None, workers=8):
    """model() of many blocks side by side: [(frame, [Unit])]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_huf_case_") as d:
        if len(raws) < 4:
            return [model(r, huffman, exe, d) for r in raws]
        with ThreadPoolExecutor(workers) as pool:
            return list(pool.map(lambda r: model(r, huffman, exe, d), raws))


def code_lengths(hists, exe=None):
    """okv_zstd_enc.hpp's huf_lengths over histograms of 256 counts: [(longest, [129 lengths])]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_huf_lens_") as d:
        data = b"".join(np.asarray(h, "<u4").tobytes() for h in hists)
        out, _ = run_main(exe, d, data, ("--lens",))
    a = np.frombuffer(out, "<u4").reshape(len(hists), 130)
    return [(int(r[0]), r[1:].tolist()) for r in a]
