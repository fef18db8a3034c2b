"""The batched GetRow's C-ABI (no GPU): include/okv_sst.h and okv_host.h declare the new
symbols, the library exports them, and the ctypes mirror in objectkv_amd/_lib.py takes
as many arguments as each prototype and lays okv_get_out out as the header does."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

from objectkv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"okv_index_new": 7, "okv_index_free": 1, "okv_index_info": 3, "okv_get_rows": 9,
       "okv_get_totals": 2, "okv_reader_get_rows": 6, "okv_meta_bloom_bytes": 2}


def _header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _prototypes():
    out = {}
    for h in ("okv_sst.h", "okv_host.h"):
        for m in re.finditer(r"\b(okv_\w+)\s*\(([^;{]*?)\)\s*;", _header(h), re.S):
            params = m.group(2).strip()
            out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_header_declares_the_new_symbols():
    protos = _prototypes()
    for name, arity in NEW.items():
        assert protos.get(name) == arity, (name, protos.get(name))
    src = _header("okv_sst.h")
    want = {"OKV_GET_FOUND": 0, "OKV_GET_BLOOM_NEGATIVE": 1, "OKV_GET_NO_BLOCK": 2,
            "OKV_GET_NOT_IN_BLOCK": 3, "OKV_GET_BLOCK_ERROR": 4, "OKV_GET_FALLBACK": 5}
    for name, value in want.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    m = re.search(r"#define\s+OKV_PATH_GET\s+(\d+)u", src)
    assert m and int(m.group(1)) == _lib.PATH_GET
    paths = [int(x) for x in re.findall(r"#define\s+OKV_PATH_\w+\s+(\d+)u", src)]
    assert len(paths) == len(set(paths)) and all(p & (p - 1) == 0 for p in paths)
    assert re.search(r"#define\s+OKV_ABI_VERSION\s+6\b", src)
    assert (_lib.GET_FOUND, _lib.GET_BLOOM_NEGATIVE, _lib.GET_NO_BLOCK, _lib.GET_NOT_IN_BLOCK,
            _lib.GET_BLOCK_ERROR, _lib.GET_FALLBACK) == (0, 1, 2, 3, 4, 5)


def test_library_exports_them_and_ctypes_matches():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = _lib.lib()
    for name, arity in NEW.items():
        assert name in exported and name in _lib.SYMBOLS, name
        assert len(getattr(L, name).argtypes) == arity, name
    assert L.okv_get_rows.restype is C.c_int and L.okv_index_free.restype is None
    assert L.okv_meta_bloom_bytes.restype is C.c_void_p


def test_get_out_layout_matches_the_header():
    m = re.search(r"typedef\s+struct\s+okv_get_out\s*\{(.*?)\}\s*okv_get_out\s*;",
                  _header("okv_sst.h"), re.S)
    assert m
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        pointer = "*" in decl
        for part in decl.split(","):
            fields.append((re.search(r"(\w+)\s*$", part.strip()).group(1), pointer))
    assert [f for f, _ in fields] == [f for f, _ in _lib.GetOut._fields_]
    for (name, pointer), (_, ctype) in zip(fields, _lib.GetOut._fields_):
        assert ctype is (C.c_void_p if pointer else C.c_uint64), name
    assert C.sizeof(_lib.GetOut) == 8 * len(fields)


def test_library_carries_the_get_kernels_and_reads_no_environment():
    data = open(_lib.LIB_PATH, "rb").read()
    for name in (b"okv_get_locate_kernel", b"okv_get_scatter_kernel", b"okv_get_search_kernel",
                 b"okv_get_values_kernel"):
        assert name in data, name
    src = open(os.path.join(ROOT, "objectkv_amd", "csrc", "okv_get.hip")).read()
    assert "getenv" not in src and "knob(" not in src and "OKV_ABLATE" not in src
