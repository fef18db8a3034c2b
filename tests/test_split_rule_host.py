"""The range-split rule stated once (objectkv_amd/csrc/okv_split.hpp, no GPU): the binary
searches and the pointer-jumping rounds the grouping kernels run, run in tests/split_main.cpp
on the CPU under AddressSanitizer and UBSan, against the linear walk of tests/split_model.py."""
from __future__ import annotations

import os
import random
import struct
import subprocess

from tests import split_model as SM
from tests.test_snap_route_host import _clang

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")


def _random_cases(seed, count):
    rng = random.Random(seed)
    out = []
    for c in range(count):
        nb = rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 31, 64, 65, 200, 1025])
        unit = rng.choice([100, 4096, 65536])
        sizes = [unit * rng.choice([1, 1, 1, 2, 5, 40]) for _ in range(nb)]
        first = [0]
        for _ in range(nb):
            first.append(first[-1] + rng.choice([1, 1, 3, 50, 512, 5000]))
        total = sum(sizes)
        sb = rng.choice([0, 1, unit, unit + 1, 3 * unit, total // 3 + 1, total, total + 1])
        sr = rng.choice([0, 1, 2, 64, first[-1] // 4 + 1, first[-1], first[-1] + 1])
        out.append((f"random{c}", sizes, first, sb, sr))
    return out


def _case_file(path, cases):
    words = [len(cases)]
    for _name, sizes, first, sb, sr in cases:
        want = SM.boundaries(sizes, first, sb, sr)
        words += [len(sizes), sb, sr, *sizes, *first, len(want), *want]
    with open(path, "wb") as fh:
        fh.write(struct.pack(f"<{len(words)}Q", *words))


def test_model_on_the_edges_the_issue_names():
    got = {name: SM.boundaries(s, f, sb, sr) for name, s, f, sb, sr in SM.edge_cases()}
    assert got["bytes_only"] == [0, 3, 6, 9, 10]
    assert got["rows_only"] == [0, 3, 6, 9, 10]  # 30 rows >= 25
    assert got["both_zero"] == [0, 10] and got["huge_thresholds"] == [0, 10]
    assert got["both"] == [0, 2, 4, 6, 8, 10]  # the row threshold is met first
    assert got["block_alone_over"] == [0, 2, 4, 5]  # 4096 + 65536, 4096 + 4096, 131072
    assert got["every_block_over"] == list(range(8))
    assert got["exact_on_last_bytes"] == [0, 3, 6] and got["exact_on_last_rows"] == [0, 3, 6]
    assert got["short_last"] == [0, 3, 6, 7]
    assert got["one_block"] == [0, 1] and got["one_block_no_limit"] == [0, 1]
    assert got["rows_met_by_first_block"] == [0, 1, 2, 3, 4]


def test_model_cut_matches_the_oracle_writer():
    from oracle import pyoracle as P
    rng = random.Random(5)
    rows = [(b"k%06d" % i, bytes(rng.randrange(256) for _ in range(rng.choice([0, 7, 300, 5000]))))
            for i in range(400)]
    for th, bs in ((3584, 4096), (64, 100), (1, 16)):
        w = P.SegmentWriter(P.SegmentWriterOptions(th, bs))
        for k, v in rows:
            w.WriteRow(k, v)
        if w.block_open:
            w._flush()
        sizes, first = SM.blocks_of_rows(rows, th, bs)
        assert sizes == [st.BlockSize for st in w.index]
        assert [rows[r][0] for r in first[:-1]] == [st.FirstKey for st in w.index]


def test_split_header_against_the_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "split_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(ROOT, "tests", "split_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = SM.edge_cases() + _random_cases(1, 300)
    path = str(tmp_path / "cases.bin")
    _case_file(path, cases)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{len(cases)} cases: all checks passed" in run.stdout


def test_split_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_split.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    inc = open(os.path.join(CSRC, "okv_split.inc")).read()
    assert "split::next(" in inc and "split::jump(" in inc and "split::rounds(" in inc
