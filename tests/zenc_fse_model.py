"""The CPU model of the device zstd encoder in its three modes (0: raw literals, 1:
OKV_F_ZSTD_HUFFMAN, 2: with OKV_F_ZSTD_HUF_FSE): the parse is tests/zenc_model.parse_unit
(phases B-E, the same in every mode); the literals decision, the tree description (direct or
FSE-compressed weights), the Huffman section and the Raw / Compressed decision are
tests/zenc_fse_main.cpp's, which runs okv_zstd_enc.hpp's statements with a sequential bit
writer and reports per unit what it chose.  No format is restated here.

Per unit the census (Unit.census) holds tests/zenc_huf_model.py's keys and "desc" (0 direct,
1 FSE: the description the Huffman section has, or would have had), "dbytes" (that
description's bytes with its header byte, 0: none), "dfse" / "ddir" (the FSE and the direct
description's bytes, 0 where there is none) and "alog" (the FSE description's accuracy
log)."""
from __future__ import annotations

import atexit
import os
import shutil
import struct
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import zenc_huf_model as H
from tests import zenc_model as M

UNIT = M.UNIT
KEYS = H.KEYS + ("desc", "dbytes", "dfse", "ddir", "alog")
OFF, HUF, FSE = 0, 1, 2


def build_fse_main(out, sanitize):
    """Compiles tests/zenc_fse_main.cpp to `out`; with AddressSanitizer and UBSan when
    `sanitize` (a plain program, CPU tests only), plain -O1 otherwise."""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(
        [M.clang(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", M.CSRC,
         "-I", os.path.join(M.ROOT, "include"),
         os.path.join(M.ROOT, "tests", "zenc_fse_main.cpp"), "-o", out],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return out


_PLAIN = []


def plain_exe():
    """zenc_fse_main without sanitizers, built once per process into a temporary directory."""
    if not _PLAIN:
        d = tempfile.mkdtemp(prefix="zenc_fse_model_")
        atexit.register(shutil.rmtree, d, True)
        _PLAIN.append(build_fse_main(os.path.join(d, "zenc_fse_main"), sanitize=False))
    return _PLAIN[0]


def model(raw, mode=FSE, exe=None, tmp=None):
    """(frame, [Unit]) the device encoder is to give for one raw block in `mode`."""
    exe = exe or plain_exe()
    if tmp is None:
        with tempfile.TemporaryDirectory(prefix="zenc_fse_case_") as d:
            return model(raw, mode, exe, d)
    raw = bytes(raw)
    units = [raw[i:i + UNIT] for i in range(0, len(raw), UNIT)] or [b""]
    parsed = [M.parse_unit(u) for u in units]
    data = bytearray(H.cases(raw, units, parsed, False))
    struct.pack_into("<I", data, 16, mode)
    frame, text = H.run_main(exe, tmp, bytes(data))
    lines = [ln.split() for ln in text.splitlines() if ln.startswith("block ")]
    assert len(lines) == len(parsed)
    for ln, pu in zip(lines, parsed):
        got = dict(zip(ln[0::2], (int(x) for x in ln[1::2])))
        assert set(got) == set(KEYS) and got["n"] == pu.n and got["nseq"] == len(pu.seqs)
        pu.census.update(got)
    assert [t for t, _ in M.block_headers(frame, len(raw))] == [p.census["block"] for p in parsed]
    return frame, parsed


def model_frames(raws, mode=FSE, exe=None, workers=8):
    """model() of many blocks side by side: [(frame, [Unit])]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_fse_case_") as d:
        if len(raws) < 4:
            return [model(r, mode, exe, d) for r in raws]
        with ThreadPoolExecutor(workers) as pool:
            return list(pool.map(lambda r: model(r, mode, exe, d), raws))


def code_lengths(hists, exe=None):
    """Over histograms of 256 counts: [(longest, [256 lengths] of huf_lengths_all, longest,
    [129 lengths] of huf_lengths)]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_fse_lens_") as d:
        data = b"".join(np.asarray(h, "<u4").tobytes() for h in hists)
        out, _ = H.run_main(exe, d, data, ("--lens",))
    a = np.frombuffer(out, "<u4").reshape(len(hists), 257 + 130)
    return [(int(r[0]), r[1:257].tolist(), int(r[257]), r[258:].tolist()) for r in a]


def descriptions(weight_lists, exe=None):
    """The FSE description of each list of weights: [(bytes without the header byte, 0 when
    there is none or it is above 127; accuracy log)]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_fse_desc_") as d:
        data = b"".join(struct.pack("<I", len(w)) + bytes(w) for w in weight_lists)
        out, _ = H.run_main(exe, d, data, ("--desc",))
    a = np.frombuffer(out, "<u4").reshape(len(weight_lists), 2)
    return [(int(r[0]), int(r[1])) for r in a]
