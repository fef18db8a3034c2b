"""RowIter.Seek + Next stated once (objectkv_amd/csrc/okv_seek.hpp, no GPU): the search the
seek kernel runs, run in tests/seek_main.cpp on the CPU under AddressSanitizer and UBSan,
against the row ranges oracle/pyoracle.py's RowIter yields (tests/seek_cases.py)."""
from __future__ import annotations

import os
import struct
import subprocess

from tests import seek_cases as SK
from tests.test_snap_route_host import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")


def _key(k):
    return struct.pack("<I", len(k)) + k


def _case_file(path):
    cases = SK.cases()
    out = [struct.pack("<I", len(cases))]
    nq = 0
    for _name, keys, first, qs in cases:
        out.append(struct.pack("<I", len(keys)) + b"".join(_key(k) for k in keys))
        out.append(struct.pack("<I", len(first) - 1) + struct.pack(f"<{len(first)}I", *first))
        out.append(struct.pack("<I", len(qs)))
        for k, d, lo, hi in qs:
            out.append(_key(k) + struct.pack("<III", d, lo, hi))
        nq += len(qs)
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return len(cases), nq


def test_cases_cover_what_the_issue_names():
    cases = {name: (keys, first, qs) for name, keys, first, qs in SK.cases()}
    assert cases["one"][1] == [0, 1] and cases["3x2"][1] == [0, 2, 4, 6]
    assert cases["ties"][1] == [0, 2, 4, 6]
    keys, _first, qs = cases["3x2"]
    want = {(q, d): (lo, hi) for q, d, lo, hi in qs}
    assert want[(b"a", SK.ASC)] == (0, 6) and want[(b"a", SK.DESC)] == (0, 0)  # below all
    assert want[(b"zzzz", SK.ASC)] == (6, 6) and want[(b"zzzz", SK.DESC)] == (0, 6)  # above all
    assert want[(b"k10", SK.ASC)] == (0, 6) and want[(b"k10", SK.DESC)] == (0, 1)  # block 0
    # the first key of a block b > 0, descending: the walk starts in the block before and
    # the row equal to the key is skipped
    assert want[(b"k30", SK.DESC)] == (0, 2) and want[(b"k50", SK.DESC)] == (0, 4)
    assert want[(b"k30", SK.ASC)] == (2, 6)
    assert want[(b"k40", SK.DESC)] == (0, 4)  # not a first key: the row itself is yielded
    assert want[(b"k60", SK.ASC)] == (5, 6) and want[(b"k60", SK.DESC)] == (0, 6)  # last key
    assert want[(b"", SK.ASC)] == (0, 6) and want[(b"", SK.DESC)] == (0, 0)  # UnboundStart
    assert want[(b"\xff", SK.ASC)] == (6, 6) and want[(b"\xff", SK.DESC)] == (0, 6)  # UnboundEnd
    keys, _first, qs = cases["ties"]
    for shared in (8, 9, 16, 17):  # probes that tie with a row on exactly that many bytes
        assert any(q[:shared] == k[:shared] and q[:shared + 1] != k[:shared + 1] and
                   len(q) > shared and len(k) > shared for q, _d, _l, _h in qs for k in keys)
    assert any(k.startswith(q) and q != k and q for q, _d, _l, _h in qs for k in keys)  # prefixes
    assert len({(lo, hi) for _q, _d, lo, hi in qs}) >= 10


def test_seek_header_against_row_iter_under_sanitizers(tmp_path):
    exe = str(tmp_path / "seek_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "seek_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = str(tmp_path / "cases.bin")
    nseg, nq = _case_file(cases)
    assert nseg == 3 and nq > 200
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_seek_header_includes_no_hip_header_and_shares_the_compare():
    src = open(os.path.join(CSRC, "okv_seek.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    assert "index::lower" in src and "index::upper" in src and "index::compare" in src
    assert "memcmp" not in src and "for (" not in src and "while (" not in src  # no second compare
