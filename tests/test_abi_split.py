"""CPU-side checks of the range-split encode's C-ABI (no GPU calls): okv_encode_split is
exported, the three structs of include/okv_sst.h have the layout of their ctypes mirrors
(a small C program prints sizeof / offsetof), the ABI version is unchanged, and the library
carries the new kernels."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

from objectkv_amd import _lib
from tests.conftest import ROOT
from tests.test_snap_route_host import _clang

MIRRORS = {"okv_split_opts": _lib.SplitOpts, "okv_split_seg": _lib.SplitSeg,
           "okv_split_out": _lib.SplitOut}

KERNELS = ["okv_split_next_kernel", "okv_split_jump_kernel", "okv_split_number_kernel",
           "okv_split_start_kernel", "okv_split_layout_kernel", "okv_split_meta_kernel",
           "okv_split_bloom_add_kernel", "okv_split_bloom_write_kernel",
           "okv_split_trailer_kernel"]


def test_symbol_and_abi_version():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert any(ln.split()[-1] == "okv_encode_split" and " T " in ln for ln in out.splitlines())
    assert "okv_encode_split" in _lib.SYMBOLS
    L = _lib.lib()
    assert L.okv_abi_version() == 6
    assert L.okv_encode_split.argtypes[3]._type_ is _lib.SplitOpts
    assert L.okv_encode_split.argtypes[4]._type_ is _lib.SplitOut
    hdr = open(os.path.join(ROOT, "include", "okv_sst.h")).read()
    assert "#define OKV_ABI_VERSION 6 " in hdr


def test_struct_layouts_match_the_header(tmp_path):
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "okv_sst.h"',
             "int main(void) {"]
    for cname, mirror in MIRRORS.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _t in mirror._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "layout")
    cc = _clang().replace("clang++", "clang")
    build = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I",
                            os.path.join(ROOT, "include"), str(src), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    got = dict(ln.split() for ln in subprocess.run([exe], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    n = 0
    for cname, mirror in MIRRORS.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for fname, _t in mirror._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(mirror, fname).offset, (cname, fname)
            n += 1
    assert n == 4 + 10 + 15
    assert C.sizeof(_lib.SplitSeg) == 80 and C.sizeof(_lib.SplitOpts) == 32


def test_library_has_the_split_kernels():
    data = open(_lib.LIB_PATH, "rb").read()
    for k in KERNELS:
        assert k.encode() in data, k
