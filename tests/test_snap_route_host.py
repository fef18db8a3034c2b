"""The snapshot routing stated once (objectkv_amd/csrc/okv_snap_route.hpp, no GPU): the
flat image of blockRangeTree and the walk of getPossibleSegmentsForKey that the device
route kernel runs, run in tests/snap_route_main.cpp on the CPU under AddressSanitizer and
UBSan, against cases written from oracle/snapshot_oracle.py's Reader."""
from __future__ import annotations

import os
import struct
import subprocess

from oracle import snapshot_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def _ladder(n):  # n overlapping segments: each range reaches into the next two
    return [(f"{i:03d}", i % 3, b"k%04d" % (10 * i), b"k%04d" % (10 * i + 25)) for i in range(n)]


P8, P9, P16 = b"ABCDEFGH", b"ABCDEFGHI", b"ABCDEFGHIJKLMNOP"


def snapshots():
    """name -> [(ID, Level, FirstKey, LastKey)] in no particular order."""
    s = {f"n{n}": _ladder(n) for n in (0, 1, 2, 63, 64, 65)}
    s["equal_first"] = [("a", 0, b"k10", b"k20"), ("b", 0, b"k10", b"k30"), ("c", 1, b"k10", b"k15"),
                        ("d", 1, b"k05", b"k40")]
    s["identical_ranges"] = [(i, l, b"k10", b"k20") for i, l in (("9", 0), ("10", 0), ("2", 1),
                                                                ("1", 0))]
    s["empty_first"] = [("a", 0, b"", b"k50"), ("b", 1, b"", b"k20"), ("c", 0, b"k10", b"k60")]
    # an empty LastKey sorts last of its FirstKey and covers only the empty key: it hides
    # every record below it from keys >= k10
    s["empty_last"] = [("a", 1, b"k00", b"k99"), ("b", 0, b"k10", b""), ("c", 0, b"k10", b"k50"),
                       ("d", 0, b"", b"")]
    s["quirk"] = [("a", 1, b"k00", b"k99"), ("b", 0, b"k40", b"k45"), ("c", 0, b"k60", b"k70")]
    s["prefix_ties"] = [
        ("a", 0, P8, P8 + b"zz"), ("b", 0, P8 + b"\x00", P9), ("c", 1, P9, P9 + b"\xff"),
        ("d", 0, P9 + b"A", P16), ("e", 1, P16, P16 + b"\x00"), ("f", 0, P16[:15], P16 + b"Q"),
        ("g", 2, P16 + b"Q", P16 + b"R"), ("h", 0, P8[:7], P8), ("i", 1, P16 + b"A", P16 + b"B")]
    return s


def queries(segs):
    qs = {b"", b"\x00", b"\xff", b"\xff\xff\xff", b"a", b"k", b"k0", b"zzzz", P8, P9, P16}
    for _i, _l, first, last in segs:
        for k in (first, last):
            qs |= {k, k + b"\x00", k + b"\x01", k[:-1], k[:-1] + b"\xff"}
            if k:
                qs |= {k[:-1] + bytes([max(k[-1] - 1, 0)]), k[:-1] + bytes([min(k[-1] + 1, 255)])}
    return sorted(qs)


def oracle_reader(segs):
    r = SO.Reader(None)
    r.UpdateSegments([SO.SegmentRecord(*s) for s in segs], None)
    return r


def priorities(tree):
    """record -> rank in GetRow's order (Level ascending, then ID descending)."""
    import functools
    order = sorted(tree, key=functools.cmp_to_key(SO._getrow_cmp))
    return {id(rec): p for p, rec in enumerate(order)}


def oracle_run(r, key):
    """[lo, hi) of tree positions getPossibleSegmentsForKey collects, hi - 1 first."""
    tree = r.blockRangeTree.items
    pos = {id(rec): t for t, rec in enumerate(tree)}
    hi = sum(1 for rec in tree if SO._cmp(rec.FirstKey, key) <= 0)
    assert all(SO._cmp(rec.FirstKey, key) <= 0 for rec in tree[:hi])  # a prefix of the order
    got = [pos[id(rec)] for rec in r.getPossibleSegmentsForKey(key)]
    assert got == list(range(hi - 1, hi - 1 - len(got), -1)), (key, got, hi)
    return hi - len(got), hi


def _case_file(path):
    snaps = snapshots()
    out = [struct.pack("<I", len(snaps))]
    nq = 0
    for _name, segs in snaps.items():
        r = oracle_reader(segs)
        tree = r.blockRangeTree.items
        prio = priorities(tree)
        out.append(struct.pack("<I", len(tree)))
        for rec in tree:
            f, l_ = SO._b(rec.FirstKey), SO._b(rec.LastKey)
            out.append(struct.pack("<I", len(f)) + f + struct.pack("<I", len(l_)) + l_ +
                       struct.pack("<II", rec.Level, prio[id(rec)]))
        qs = queries(segs)
        out.append(struct.pack("<I", len(qs)))
        for q in qs:
            out.append(struct.pack("<I", len(q)) + q + struct.pack("<II", *oracle_run(r, q)))
        nq += len(qs)
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return len(snaps), nq


def test_cases_cover_what_the_issue_names():
    s = snapshots()
    assert [len(oracle_reader(s[f"n{n}"]).blockRangeTree.items) for n in (0, 1, 2, 63, 64, 65)] == \
        [0, 1, 2, 63, 64, 65]
    r = oracle_reader(s["equal_first"])
    assert [x.ID for x in r.blockRangeTree.items] == ["d", "c", "a", "b"]
    assert oracle_run(r, b"k18") == (2, 4) and oracle_run(r, b"k25") == (3, 4)
    r = oracle_reader(s["identical_ranges"])
    assert [x.ID for x in r.blockRangeTree.items] == ["1", "10", "2", "9"]  # Go string order
    assert oracle_run(r, b"k15") == (0, 4)
    r = oracle_reader(s["empty_first"])
    assert oracle_run(r, b"") == (0, 2) and oracle_run(r, b"k15") == (0, 3)
    r = oracle_reader(s["empty_last"])
    assert [x.ID for x in r.blockRangeTree.items] == ["d", "a", "c", "b"]
    assert oracle_run(r, b"k20") == (4, 4)  # "b" stops the walk: "c" and "a" hold k20
    assert oracle_run(r, b"k05") == (1, 2) and oracle_run(r, b"") == (0, 1)
    r = oracle_reader(s["quirk"])
    assert oracle_run(r, b"k42") == (0, 2)
    assert oracle_run(r, b"k50") == (2, 2)  # stop at the first miss: "a" is never asked
    assert oracle_run(r, b"k65") == (2, 3)  # ... and not behind "b" either
    r = oracle_reader(s["n65"])
    assert oracle_run(r, b"a") == (0, 0) and oracle_run(r, b"zzzz") == (65, 65)  # below, above
    assert oracle_run(r, b"k0100") == (8, 11) and oracle_run(r, b"k0025") == (0, 3)  # first, last
    keys = [k for seg in s["prefix_ties"] for k in seg[2:]]
    for shared in (8, 9, 16):
        assert sum(1 for a in keys for b in keys if a < b and a[:shared] == b[:shared]
                   and len(a) >= shared) >= 3
    r = oracle_reader(s["prefix_ties"])
    runs = {oracle_run(r, q) for q in queries(s["prefix_ties"])}
    assert len(runs) >= 8 and any(hi - lo >= 3 for lo, hi in runs)


def test_route_header_against_snapshot_oracle_under_sanitizers(tmp_path):
    exe = str(tmp_path / "snap_route_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "snap_route_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = str(tmp_path / "cases.bin")
    nsnap, nq = _case_file(cases)
    assert nsnap >= 12 and nq > 2000
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_route_header_includes_no_hip_header_and_shares_the_compare():
    src = open(os.path.join(CSRC, "okv_snap_route.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    assert "index::floor_upper" in src and "index::tie_le" in src
    assert "memcmp" not in src and "for (" not in src  # no second byte compare
