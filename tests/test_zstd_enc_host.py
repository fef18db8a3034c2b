"""The zstd encoder's format statements (objectkv_amd/csrc/okv_zstd_enc.hpp, no GPU):
tests/zenc_main.cpp writes frames from literals and sequence lists with that header's
functions alone -- the statements the device encoder runs -- on the CPU under
AddressSanitizer and UBSan, as a plain program.  libzstd (oracle/zstd_ref.decompress)
inflates each frame and the result must be the bytes the sequences describe.

Values no zstd block can hold: a block's content is at most 128 KiB (RFC 8878
3.1.1.2.4), so literal-length code 35 and match-length code 52 cannot take their
largest extra bits (131 071 literals, a match of 131 074); those two cases use the
largest value that fits the block.  A block must also be no larger than its frame's
Block_Maximum_Size = min(Window_Size, 128 KiB), and a Single_Segment frame's window is
its content size: every case is therefore one whose compressed form is smaller than
its content (what the device encoder guarantees by falling back to Raw_Blocks)."""
from __future__ import annotations

import os
import random
import struct
import subprocess

import pytest

from oracle import pyoracle as P
from oracle import zstd_ref as Z

from tests.zenc_model import CSRC, LL, ML, build_zenc_main
from tests.zenc_model import code as _code

BLOCK_MAX = 128 * 1024


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_zenc_main(str(tmp_path_factory.mktemp("zenc") / "zenc_main"), sanitize=True)


WARM = (8, 24, 8)  # gives every frame eight bytes to point back into


def _blocks(seqs, tail=0):
    """Sequences packed into blocks of at most 128 KiB of content; `tail` literals after
    the last sequence of the last block."""
    blocks, cur, size = [], [], 0
    for s in seqs:
        if size + s[0] + s[1] > BLOCK_MAX:
            blocks.append((cur, 0))
            cur, size = [], 0
        cur.append(s)
        size += s[0] + s[1]
    if size + tail > BLOCK_MAX:
        return blocks + [(cur, 0), ([], tail)]
    return blocks + [(cur, tail)]


def _run(exe, tmp_path, blocks, seed=1):
    """blocks: [(sequences, trailing literals)].  Returns (frame, expected content)."""
    rng = random.Random(seed)
    content = bytearray()
    body = []
    for seqs, tail in blocks:
        lits = bytearray()
        for ll, ml, off in seqs:
            new = rng.randbytes(ll)
            lits += new
            content += new
            assert 1 <= off <= len(content) and ml >= 3
            if off >= ml:
                content += content[len(content) - off:len(content) - off + ml]
            else:
                pat = bytes(content[-off:])
                content += (pat * (ml // off + 1))[:ml]
        new = rng.randbytes(tail)
        lits += new
        content += new
        body.append(struct.pack("<I", len(lits)) + bytes(lits) + struct.pack("<I", len(seqs)) +
                    b"".join(struct.pack("<III", *s) for s in seqs))
    content = bytes(content)
    head = struct.pack("<QII", len(content), P.xxh64(content) & 0xFFFFFFFF, len(blocks))
    cases, frame = str(tmp_path / "cases.bin"), str(tmp_path / "frame.zst")
    with open(cases, "wb") as fh:
        fh.write(head + b"".join(body))
    run = subprocess.run([exe, cases, frame], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    with open(frame, "rb") as fh:
        return fh.read(), content


def _check(exe, tmp_path, blocks, seed=1):
    frame, content = _run(exe, tmp_path, blocks, seed)
    got = Z.decompress(frame, len(content))
    assert got is not None, "libzstd rejects the frame"
    assert got == content
    return frame


def test_every_literal_length_code(exe, tmp_path):
    seqs, seen = [WARM], set()
    for c, (base, bits) in enumerate(LL):
        for ll in (base, min(base + (1 << bits) - 1, BLOCK_MAX - 16)):
            assert _code(LL, ll) == c
            seqs.append((ll, 16, 1))
            seen.add(c)
    assert seen == set(range(36))
    _check(exe, tmp_path, _blocks(seqs))


def test_every_match_length_code(exe, tmp_path):
    seqs, seen = [WARM], set()
    for c, (base, bits) in enumerate(ML):
        for ml in (base, min(base + (1 << bits) - 1, BLOCK_MAX - 1)):
            assert _code(ML, ml) == c
            seqs.append((1, ml, 1 + c % 5))
            seen.add(c)
    assert seen == set(range(53))
    _check(exe, tmp_path, _blocks(seqs, tail=9))


def test_offset_codes_2_to_17(exe, tmp_path):
    """Offset_Value = offset + 3 in [2^c, 2^(c+1)): code c at its baseline and with all
    extra bits set.  Three Raw_Blocks of literals first, so that 262 140 bytes exist."""
    seqs = []
    for c in range(2, 18):
        seqs += [(2, 5, (1 << c) - 3), (2, 5, (2 << c) - 4)]
    assert max(s[2] for s in seqs) == 262140 and min(s[2] for s in seqs) == 1
    raw = [([], BLOCK_MAX)] * 3
    _check(exe, tmp_path, raw + [(seqs, 3)])


@pytest.mark.parametrize("nseq", [1, 127, 128, 0x7F00])
def test_sequence_count_forms(exe, tmp_path, nseq):
    lit = 3 if nseq < 1000 else 1  # (0x7F00 sequences must stay inside one 128 KiB block)
    seqs = [WARM] + [(k % lit, 3 + k % 2, 1 + k % 7) for k in range(nseq - 1)]
    frame = _check(exe, tmp_path, [(seqs, 5)], seed=nseq)
    assert frame[:4] == b"\x28\xb5\x2f\xfd"


def test_last_sequence_ends_the_block(exe, tmp_path):
    _check(exe, tmp_path, [([WARM, (4, 20, 3)], 0)])
    _check(exe, tmp_path, [([WARM, (4, 20, 3)], 0), ([(0, 7, 30)], 0)])


def test_overlapping_match(exe, tmp_path):
    frame = _check(exe, tmp_path, [([(1, 65000, 1)], 0)])
    assert len(frame) < 40
    _check(exe, tmp_path, [([(3, 65000, 2), (0, 1000, 3)], 1)])


@pytest.mark.parametrize("nlit", [31, 32, 4095, 4096])
def test_literal_header_forms(exe, tmp_path, nlit):
    frame = _check(exe, tmp_path, [([(nlit, 40, 1)], 0)], seed=nlit)
    hs = 6 if nlit + 40 < 256 else 7
    lit0 = frame[hs + 3]
    assert lit0 & 3 == 0  # Raw_Literals_Block
    fmt = (lit0 >> 2) & 3  # (the 1-byte format has one format bit: 0 or 2 here)
    assert (fmt & 1 == 0) if nlit < 32 else fmt == (1 if nlit < 4096 else 3)


def test_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_zstd_enc.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
