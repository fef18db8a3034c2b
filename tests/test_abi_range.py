"""The range path's C-ABI (no GPU): include/okv_sst.h declares okv_seek_rows and
okv_gather_rows, the library exports them, and the ctypes mirror in objectkv_amd/_lib.py
takes as many arguments as each prototype and lays okv_seek_src and okv_gather_out out as
the header does."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

from objectkv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"okv_seek_rows": 9, "okv_gather_rows": 8}


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _prototypes():
    out = {}
    for m in re.finditer(r"\b(okv_\w+)\s*\(([^;{]*?)\)\s*;", _header("okv_sst.h"), re.S):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def _struct_fields(name):
    """[(field, is a pointer, C type)] of a typedef struct in okv_sst.h."""
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;",
                  _header("okv_sst.h"), re.S)
    assert m, name
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        for part in decl.split(","):
            fields.append((re.search(r"(\w+)\s*$", part.strip()).group(1), "*" in decl, ctype))
    return fields


def test_header_declares_the_new_symbols():
    protos = _prototypes()
    for name, arity in NEW.items():
        assert protos.get(name) == arity, (name, protos.get(name))
    assert re.search(r"#define\s+OKV_ABI_VERSION\s+6\b", _header("okv_sst.h"))
    # okv_gather_rows takes the merge's sources and outputs as they are
    assert re.search(r"okv_gather_rows\s*\(\s*okv_ctx\s*\*\s*ctx\s*,\s*const\s+okv_merge_src\s*\*",
                     _header("okv_sst.h"))


def test_library_exports_them_and_ctypes_matches():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = _lib.lib()
    for name, arity in NEW.items():
        assert name in exported and name in _lib.SYMBOLS, name
        assert len(getattr(L, name).argtypes) == arity, name
        assert getattr(L, name).restype is C.c_int
    assert L.okv_abi_version() == 6


def test_struct_layouts_match_the_header():
    for name, mirror in (("okv_seek_src", _lib.SeekSrc), ("okv_gather_out", _lib.GatherOut)):
        fields = _struct_fields(name)
        assert [f for f, _p, _t in fields] == [f for f, _ in mirror._fields_], name
        for (field, pointer, ctype), (_, mtype) in zip(fields, mirror._fields_):
            assert pointer or ctype == "uint64_t", (name, field)
            assert mtype is (C.c_void_p if pointer else C.c_uint64), (name, field)
        assert C.sizeof(mirror) == 8 * len(fields)
    # the gather reads the first six pointers of okv_merge_src: the mirror's too
    assert [f for f, _p, _t in _struct_fields("okv_merge_src")][:6] == \
        [f for f, _ in _lib.MergeSrc._fields_][:6] == \
        ["key_arena", "key_off", "key_len", "val_arena", "val_off", "val_len"]


def test_library_carries_the_kernels_and_reads_no_environment():
    data = open(_lib.LIB_PATH, "rb").read()
    for name in (b"okv_seek_kernel", b"okv_gather_index_kernel", b"okv_gather_copy_kernel"):
        assert name in data, name
    for f in ("okv_seek.hip", "okv_seek.hpp"):
        src = open(os.path.join(ROOT, "objectkv_amd", "csrc", f)).read()
        assert "getenv" not in src and "knob(" not in src and "OKV_ABLATE" not in src
