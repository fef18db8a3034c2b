"""The block index stated once (objectkv_amd/csrc/okv_index.hpp, no GPU): the
ReplaceOrInsert order, the lower / upper searches the reader uses and the floor search
the device runs over the flat image run in tests/index_main.cpp on the CPU under
AddressSanitizer and UBSan, against cases written from oracle/pyoracle.py's BlockIndex
(tests/index_cases.py)."""
from __future__ import annotations

import os
import struct
import subprocess

from tests import index_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def _case_file(path):
    trees = IC.trees()
    out = [struct.pack("<I", len(trees))]
    n_queries = 0
    for name, keys in trees.items():
        out.append(struct.pack("<I", len(keys)))
        out += [struct.pack("<I", len(k)) + k for k in keys]
        order, ix = IC.oracle_tree(keys)
        assert len(order) == len(set(keys)), name
        out.append(struct.pack(f"<I{len(order)}I", len(order), *order))
        qs = IC.queries(keys)
        out.append(struct.pack("<I", len(qs)))
        for q in qs:
            out.append(struct.pack("<I", len(q)) + q + struct.pack("<q", IC.oracle_floor(ix, q)))
        n_queries += len(qs)
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return len(trees), n_queries


def test_cases_cover_what_the_issue_names():
    t = IC.trees()
    assert {len(set(t[f"n{n}"])) for n in (1, 2, 3, 63, 64, 65)} == {1, 2, 3, 63, 64, 65}
    order, _ = IC.oracle_tree(t["dups_last_wins"])
    assert order == [7, 5, 3, 6]  # the last of each equal first key stays
    assert b"" in t["empty_first_key"]
    _, ix = IC.oracle_tree(t["ab_family"])
    assert [IC.oracle_floor(ix, q) for q in (b"ab", b"ab\x00", b"abc", b"aa", b"")] == [1, 2, 0, 3, -1]
    keys = t["prefix_ties"]
    for shared in (8, 9, 16):
        assert sum(1 for a in keys for b in keys if a < b and a[:shared] == b[:shared]
                   and len(a) >= shared) >= 3
    qs = IC.queries(keys)
    _, ix = IC.oracle_tree(keys)
    floors = [IC.oracle_floor(ix, q) for q in qs]
    assert -1 in floors and len(set(floors)) == len(set(keys)) + 1  # below, and every entry


def test_index_header_against_btree_oracle_under_sanitizers(tmp_path):
    exe = str(tmp_path / "index_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "index_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = str(tmp_path / "cases.bin")
    ntrees, nq = _case_file(cases)
    assert ntrees >= 20 and nq > 2000
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_index_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_index.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src


def test_reader_uses_the_shared_index():
    """The reader's btree helpers are the header's: no second binary search or
    ReplaceOrInsert loop in okv_reader.cpp."""
    src = open(os.path.join(CSRC, "okv_reader.cpp")).read()
    assert '#include "okv_index.hpp"' in src
    assert "okv::index::tree_order" in src and "okv::index::upper" in src
    assert "(lo + hi) / 2" not in src
