"""Host-mode staging stated once (objectkv_amd/csrc/okv_stage.hpp, no GPU): Layout, place
and check_keys run in tests/stage_main.cpp on the CPU under AddressSanitizer and UBSan.
What they must give is stated here: the offset chains the entry points wrote out by hand
before the header existed, and the key check's edges."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")

NS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)  # 8-, 4-, 2-, 1-byte columns
KABS = (0, 1, 255, 256, 257)                                        # cross a 256-byte line here
NSRC = 3
SEEK_SRC = 48  # sizeof(okv_seek_src): four pointers and two counts


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def al(x):
    return (x + 255) & ~255


def old_chain(sizes):
    """off[0] = 0, off[i + 1] = off[i] + al(size[i]): the chains as they were written."""
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += al(s)
    return offs, at


def old_layout(name, n, kab):
    """-> (sizes, offsets, end) of the hand-written chain of each call."""
    keys = [kab, n * 8, n * 2]
    if name == "seek":  # osr, oko, okl, oso, odi, olo; ohi = olo + n * 8, end = ohi + n * 8
        sizes = [kab, SEEK_SRC * NSRC, n * 8, n * 2, n * 4, n, n * 16]
        offs, _ = old_chain(sizes)
        return sizes, offs, offs[-1] + n * 16
    sizes = {"bloom_add": keys,
             "bloom_test": keys + [n],
             "get": keys + [n * 4, n * 4, n * 4, n * 8, n * 4, n * 8],
             "snap": keys + [n * 4, n * 4, n * 4, n * 4, n * 8, n * 4, n * 8],
             "gather": [n * 8, n * 2, n * 8, n * 4]}[name]
    offs, end = old_chain(sizes)
    return sizes, offs, end


SETS = ("bloom_add", "bloom_test", "get", "snap", "seek", "gather")
BIG = 1 << 64


def key_cases():
    """(line of the case file, expected answer, what it is)"""
    def case(bounds, kab, rows, nulls=(0, 0, 0)):
        flat = " ".join(f"{o} {ln}" for o, ln in rows)
        return f"keys {bounds} {nulls[0]} {nulls[1]} {nulls[2]} {kab} {len(rows)} {flat}".rstrip()

    out = []
    for kab in KABS:
        out += [(case(1, kab, [(kab, 0)]), "ok", "key_off == key_arena_bytes, empty key"),
                (case(1, kab, [(0, min(kab, 65535))]), "ok", "one key, the whole arena"),
                (case(1, kab, [(0, 0), (kab + 1, 0)]), "outside", "key_off one past"),
                (case(0, kab, [(0, 0), (kab + 1, 0)]), "ok", "device mode: no bounds check"),
                (case(1, kab, [(kab // 2, kab - kab // 2 + 1)]), "outside", "key_len one past"),
                (case(1, kab, [(kab // 2, kab - kab // 2)]), "ok", "key_len to the end"),
                (case(1, kab, [(BIG - 1, 1)]), "outside", "off + len wraps to 0"),
                (case(1, kab, [(BIG - 2, 3)]), "outside", "off + len wraps to 1")]
    for bounds in (0, 1):
        out += [(case(bounds, 8, [(0, 1)], (1, 0, 0)), "null_array", "NULL arena with bytes"),
                (case(bounds, 0, [(0, 0)], (1, 0, 0)), "ok", "NULL arena without bytes"),
                (case(bounds, 8, [(0, 1)], (0, 1, 0)), "null_array", "NULL key_off"),
                (case(bounds, 8, [(0, 1)], (0, 0, 1)), "null_array", "NULL key_len"),
                # the entry points accept n == 0 before they look at the arrays
                (case(bounds, 8, [], (1, 1, 1)), "ok", "n == 0, every array NULL"),
                (case(bounds, 0, [], (0, 1, 0)), "ok", "n == 0, NULL key_off")]
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stage")
    exe = str(tmp / "stage_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "stage_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    layouts = [(s, n, kab) for s in SETS for n in NS for kab in KABS]
    lines = [f"layout {s} {n} {kab} {NSRC}" for s, n, kab in layouts]
    keys = key_cases()
    lines += [k[0] for k in keys]
    path = str(tmp / "cases.txt")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    got = run.stdout.split("\n")
    assert got[len(lines)] == "done" and len(got) == len(lines) + 2
    return dict(layouts=list(zip(layouts, got[:len(layouts)])),
                keys=list(zip(keys, got[len(layouts):len(lines)])))


def test_layouts_are_the_old_chains(answers):
    assert len(answers["layouts"]) == len(SETS) * len(NS) * len(KABS)
    for (name, n, kab), line in answers["layouts"]:
        words = line.split()
        assert words[0] == "layout"
        regions = [tuple(int(x) for x in w.split(":")) for w in words[1:-1]]
        end = int(words[-1])
        sizes, offs, old_end = old_layout(name, n, kab)
        what = (name, n, kab)
        assert [b for _, b in regions] == sizes, what
        at = 0
        for off, nbytes in regions:  # 256-byte lines, declaration order, no overlap
            assert off % 256 == 0 and off >= at, what
            at = off + nbytes
        assert [o for o, _ in regions] == offs, what
        assert end % 256 == 0 and end >= at, what
        if name == "seek":
            # the old chain left its last region, the (row_lo, row_hi) pairs, unrounded;
            # what is copied (the inputs: offs[-1] bytes; the pairs: n * 16) is the same
            assert old_end == offs[-1] + n * 16 and end == al(old_end), what
        else:
            assert end == old_end, what


def test_check_keys_edges(answers):
    assert len(answers["keys"]) >= 50
    for (line, want, what), got in answers["keys"]:
        assert got == "keys " + want, (what, line)


def test_plain_part_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_stage.hpp")).read()
    plain = src[:src.index("#ifdef OKV_BUF_HIP")]
    assert "#include <hip" not in src and '#include "hip' not in src
    for name in ("class Layout", "check_keys(", "struct Col", "void place("):
        assert name in plain, name
    for word in ("hipMemcpy", "hipStream", "okv_ctx*", "DevBuf"):
        assert word not in plain, word
