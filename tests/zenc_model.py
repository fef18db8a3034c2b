"""A CPU model of the device zstd encoder's parse (okv_zstd_enc.hip, phases B-E and the
Raw / Compressed decision of G), so that a frame can be predicted byte for byte.

Per unit of OKV_ZSTD_ENC_UNIT source bytes (n of them in the last unit of a block):

* Windows.  npos = n - 3 if n >= 4 else 0.  Position i < npos has the little-endian u32
  w[i] of bytes i .. i+3; its hash is (w[i] * 2654435761 mod 2^32) >> 18 (14 bits).
* Candidate.  cand[i] is the nearest earlier position with the same hash, dropped when
  w[cand[i]] != w[i].
* Greedy parse, quarter by quarter.  Quarters are [q0, qe), UNIT / 4 bytes each, clipped
  to n.  A match may start at s only if q0 <= s, s + 4 <= qe and s < npos.  The parse takes
  the first position at or after the cursor that has a candidate; the length starts at 4
  and grows while s + len < qe and byte[s + len] == byte[cand + len] (the source may
  overlap the match).  The sequence is (s - lit0, len, s - cand); cursor and lit0 move to
  s + len.  Literals left at a quarter's end join the next sequence's literal length;
  literals after the last sequence are the block's tail.
* Block form.  No sequence: a Raw_Block.  Otherwise Compressed only if the compressed
  size is smaller than n, else Raw.

The frame bytes come from tests/zenc_main.cpp (okv_zstd_enc.hpp's statements on the CPU):
FSE, the codes and the headers are not restated here.  zenc_main runs once with every
parsed unit as a sequence block; the block headers of that frame give each unit's
compressed size; units whose size is >= n become literals-only blocks in a second run.

The census of a unit (Unit.census) comes from this model alone, never from device output.
"""
from __future__ import annotations

import atexit
import os
import shutil
import struct
import subprocess
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np

from objectkv_amd import _lib
from oracle import pyoracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")
UNIT = _lib.ZSTD_ENC_UNIT
QUARTER = UNIT // 4
HASH_LOG = 14
STEP = 64  # positions one step of the candidate walk takes

# RFC 8878 3.1.1.3.2.1.1: (baseline, extra bits) per code
LL = [(i, 0) for i in range(16)] + [(16, 1), (18, 1), (20, 1), (22, 1), (24, 2), (28, 2), (32, 3),
                                    (40, 3), (48, 4), (64, 6), (128, 7), (256, 8), (512, 9),
                                    (1024, 10), (2048, 11), (4096, 12), (8192, 13), (16384, 14),
                                    (32768, 15), (65536, 16)]
ML = [(i + 3, 0) for i in range(32)] + [(35, 1), (37, 1), (39, 1), (41, 1), (43, 2), (47, 2),
                                        (51, 3), (59, 3), (67, 4), (83, 4), (99, 5), (131, 7),
                                        (259, 8), (515, 9), (1027, 10), (2051, 11), (4099, 12),
                                        (8195, 13), (16387, 14), (32771, 15), (65539, 16)]


def code(table, v):
    return max(c for c, (base, _) in enumerate(table) if base <= v)


def _codes(table, values):
    bases = np.array([b for b, _ in table], np.int64)
    return set((np.searchsorted(bases, np.asarray(values, np.int64), side="right") - 1).tolist())


# ---- tests/zenc_main.cpp as a program ---------------------------------------------------
def clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def build_zenc_main(out, sanitize):
    """Compiles tests/zenc_main.cpp to `out`; with AddressSanitizer and UBSan when
    `sanitize` (a plain program, CPU tests only), plain -O1 otherwise."""
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    build = subprocess.run(
        [clang(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", CSRC,
         "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "zenc_main.cpp"),
         "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return out


_PLAIN = []


def plain_exe():
    """zenc_main without sanitizers, built once per process into a temporary directory."""
    if not _PLAIN:
        d = tempfile.mkdtemp(prefix="zenc_model_")
        atexit.register(shutil.rmtree, d, True)
        _PLAIN.append(build_zenc_main(os.path.join(d, "zenc_main"), sanitize=False))
    return _PLAIN[0]


# ---- the parse --------------------------------------------------------------------------
@dataclass
class Unit:
    n: int
    seqs: list            # (literal length, match length, distance)
    matches: list         # (start, length, source) as positions in the unit
    cand: np.ndarray      # per window position: the candidate that passed the 4-byte check, -1
    tail: int             # literals after the last sequence
    census: dict = field(default_factory=dict)

    def literals(self, u):
        out, p = bytearray(), 0
        for ll, ml, _ in self.seqs:
            out += u[p:p + ll]
            p += ll + ml
        return bytes(out + u[p:])


def quarters(n):
    return [(min(q * QUARTER, n), min(min(q * QUARTER, n) + QUARTER, n)) for q in range(4)]


def parse_unit(u) -> Unit:
    n = len(u)
    assert n <= UNIT
    a = np.frombuffer(u, np.uint8)
    npos = n - 3 if n >= 4 else 0
    census = {"n": n, "seq_per_quarter": [0, 0, 0, 0], "groups": set(), "hidden": 0,
              "ll": set(), "ml": set(), "of": set(), "lit_form": None, "nseq_form": None,
              "block": 0, "csz_minus_n": None}
    if npos == 0:
        return Unit(n, [], [], np.zeros(0, np.int64), n, census)
    b = a.astype(np.uint32)
    w = b[:npos] | (b[1:npos + 1] << 8) | (b[2:npos + 2] << 16) | (b[3:npos + 3] << 24)
    h = ((w.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> (32 - HASH_LOG)
    # nearest earlier position with the same hash: the predecessor in a stable sort by hash
    order = np.argsort(h, kind="stable")
    same = h[order][1:] == h[order][:-1]
    cand = np.full(npos, -1, np.int64)
    cand[order[1:][same]] = order[:-1][same]
    had = cand >= 0
    ok = had.copy()
    ok[had] = w[cand[had]] == w[had]
    cand[~ok] = -1
    # census: a dropped candidate that hid an older position with the same four bytes
    _, first, inv = np.unique(w, return_index=True, return_inverse=True)
    census["hidden"] = int(np.count_nonzero(had & ~ok & (first[inv] < np.arange(npos))))
    # census: hash groups inside one step of 64 positions, and how many of the group's
    # hash the step before held: (members in this step, members in the previous step)
    key = (np.arange(npos, dtype=np.int64) // STEP << HASH_LOG) | h.astype(np.int64)
    keys, counts = np.unique(key, return_counts=True)
    prev = keys - (1 << HASH_LOG)
    at = np.searchsorted(keys, prev)
    at_c = np.minimum(at, len(keys) - 1)
    pc = np.where(keys[at_c] == prev, counts[at_c], 0)
    multi = counts >= 2
    census["groups"] = set(zip(counts[multi].tolist(), pc[multi].tolist()))
    # the greedy parse
    has = np.nonzero(cand >= 0)[0]
    seqs, matches, lit0 = [], [], 0
    for q, (q0, qe) in enumerate(quarters(n)):
        pe = min(npos, max(qe - 3, 0))  # match starts: s + 4 <= qe and s < npos
        p = q0
        while p < pe:
            j = int(np.searchsorted(has, p))
            if j >= len(has) or has[j] >= pe:
                break
            s = int(has[j])
            cs = int(cand[s])
            ln = 4
            while s + ln < qe:
                m = min(qe - s - ln, 256)
                d = np.nonzero(a[s + ln:s + ln + m] != a[cs + ln:cs + ln + m])[0]
                if len(d):
                    ln += int(d[0])
                    break
                ln += m
            seqs.append((s - lit0, ln, s - cs))
            matches.append((s, ln, cs))
            census["seq_per_quarter"][q] += 1
            p = lit0 = s + ln
    if seqs:
        arr = np.array(seqs, np.int64)
        census["ll"] = _codes(LL, arr[:, 0])
        census["ml"] = _codes(ML, arr[:, 1])
        census["of"] = {int(v).bit_length() - 1 for v in np.unique(arr[:, 2] + 3)}
    return Unit(n, seqs, matches, cand, n - lit0, census)


# ---- frames -----------------------------------------------------------------------------
def frame_header_size(orig):
    return 5 + (1 if orig < 256 else 2 if orig < 65792 else 4 if orig < 1 << 32 else 8)


def _cases(raw, units, parsed, as_raw):
    body = []
    for u, pu, r in zip(units, parsed, as_raw):
        if r:
            body.append(struct.pack("<I", len(u)) + u + struct.pack("<I", 0))
        else:
            lits = pu.literals(u)
            body.append(struct.pack("<I", len(lits)) + lits + struct.pack("<I", len(pu.seqs)) +
                        np.array(pu.seqs, "<u4").tobytes())
    return struct.pack("<QII", len(raw), P.xxh64(raw) & 0xFFFFFFFF, len(units)) + b"".join(body)


def _zenc_main(exe, tmp, cases):
    stem = os.path.join(tmp, f"t{threading.get_ident()}")
    with open(stem + ".bin", "wb") as fh:
        fh.write(cases)
    run = subprocess.run([exe, stem + ".bin", stem + ".zst"], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    with open(stem + ".zst", "rb") as fh:
        return fh.read()


def block_headers(frame, orig):
    """[(type, size)] of a frame's blocks."""
    pos, out = frame_header_size(orig), []
    while True:
        hd = int.from_bytes(frame[pos:pos + 3], "little")
        out.append(((hd >> 1) & 3, hd >> 3))
        pos += 3 + (hd >> 3)
        if hd & 1:
            break
    assert pos + 4 == len(frame)
    return out


def model(raw, exe=None, tmp=None):
    """(frame, [Unit]) the device encoder is to give for one raw block."""
    exe = exe or plain_exe()
    if tmp is None:
        with tempfile.TemporaryDirectory(prefix="zenc_case_") as d:
            return model(raw, exe, d)
    raw = bytes(raw)
    units = [raw[i:i + UNIT] for i in range(0, len(raw), UNIT)] or [b""]
    parsed = [parse_unit(u) for u in units]
    as_raw = [not pu.seqs for pu in parsed]
    frame = _zenc_main(exe, tmp, _cases(raw, units, parsed, as_raw))
    flipped = False
    for i, ((typ, size), pu) in enumerate(zip(block_headers(frame, len(raw)), parsed)):
        if typ == 2:
            pu.census["csz_minus_n"] = size - pu.n
            if size >= pu.n:  # Compressed only when smaller than the source
                as_raw[i] = flipped = True
    if flipped:
        frame = _zenc_main(exe, tmp, _cases(raw, units, parsed, as_raw))
    for pu, r in zip(parsed, as_raw):
        if not r:
            nlit, ns = pu.n - sum(m[1] for m in pu.matches), len(pu.seqs)
            pu.census.update(block=2, lit_form=1 if nlit < 32 else 2 if nlit < 4096 else 3,
                             nseq_form=1 if ns < 128 else 2 if ns < 0x7F00 else 3)
    assert [t for t, _ in block_headers(frame, len(raw))] == [p.census["block"] for p in parsed]
    return frame, parsed


def model_frame(raw, exe=None):
    return model(raw, exe)[0]


def model_frames(raws, exe=None, workers=8):
    """model() of many blocks, the zenc_main runs side by side: [(frame, [Unit])]."""
    exe = exe or plain_exe()
    with tempfile.TemporaryDirectory(prefix="zenc_case_") as d:
        if len(raws) < 4:
            return [model(r, exe, d) for r in raws]
        with ThreadPoolExecutor(workers) as pool:
            return list(pool.map(lambda r: model(r, exe, d), raws))
