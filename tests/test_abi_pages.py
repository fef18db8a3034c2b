"""The batched GetRange merge's C-ABI (no GPU): include/okv_sst.h declares okv_merge_pages,
the library exports it, the ctypes mirror in objectkv_amd/_lib.py takes as many arguments as
the prototype and lays okv_page and okv_pages_out out as the header does, the constants
agree, and the merge's compare is stated once (okv_merge_kernels.hpp)."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

from objectkv_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")
CTYPES = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32}


def _header():
    src = open(os.path.join(ROOT, "include", "okv_sst.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _define(name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", _header())
    assert m, name
    return int(m.group(1))


def _struct_fields(name):
    """[(field, is a pointer, C type)] of a typedef struct in okv_sst.h."""
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;",
                  _header(), re.S)
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


def test_header_declares_okv_merge_pages():
    m = re.search(r"\bokv_merge_pages\s*\(([^;{]*?)\)\s*;", _header(), re.S)
    assert m and m.group(1).count(",") + 1 == 9
    assert re.search(r"#define\s+OKV_ABI_VERSION\s+6\b", _header())
    # it takes the merge's sources as they are
    assert re.search(r"okv_merge_pages\s*\(\s*okv_ctx\s*\*\s*ctx\s*,\s*const\s+okv_merge_src\s*\*",
                     _header())


def test_library_exports_it_and_ctypes_matches():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = _lib.lib()
    assert "okv_merge_pages" in exported and "okv_merge_pages" in _lib.SYMBOLS
    assert len(L.okv_merge_pages.argtypes) == 9
    assert L.okv_merge_pages.restype is C.c_int
    assert L.okv_abi_version() == 6


def test_struct_layouts_match_the_header():
    for name, mirror in (("okv_page", _lib.Page), ("okv_pages_out", _lib.PagesOut)):
        fields = _struct_fields(name)
        assert [f for f, _p, _t in fields] == [f for f, _ in mirror._fields_], name
        for (field, pointer, ctype), (_, mtype) in zip(fields, mirror._fields_):
            assert mtype is (C.c_void_p if pointer else CTYPES[ctype]), (name, field)
    assert C.sizeof(_lib.Page) == 48
    assert [f for f, _ in _lib.Page._fields_] == [
        "limit", "out_at", "out_cap", "src_at", "nsrc", "bound_at", "bound_len", "direction",
        "pad"]
    assert C.sizeof(_lib.PagesOut) == 8 * 5


def test_constants_equal_the_headers_defines():
    assert _lib.PAGE_MAX_ROWS == _define("OKV_PAGE_MAX_ROWS")
    assert 1024 <= _lib.PAGE_MAX_ROWS
    assert _lib.M_BIG == _define("OKV_M_BIG")
    assert _lib.M_CAPACITY == _define("OKV_M_CAPACITY")
    assert _lib.M_EOF == _define("OKV_M_EOF")
    assert len({0, _lib.M_EOF, _lib.M_BIG, _lib.M_CAPACITY}) == 4


def test_library_carries_the_kernel_and_the_new_files_read_no_environment():
    assert b"okv_merge_page_kernel" in open(_lib.LIB_PATH, "rb").read()
    for f in ("okv_pages.hip", "okv_merge_kernels.hpp"):
        src = open(os.path.join(CSRC, f)).read()
        assert "getenv" not in src and "knob(" not in src and "OKV_ABLATE" not in src, f


def test_one_compare_and_one_statement_of_the_go_loop():
    hdr = open(os.path.join(CSRC, "okv_merge_kernels.hpp")).read()
    shared = ("key_cmp", "be_prefix", "be_word", "find_src", "go_outcome", "term_key")
    for name in shared:
        assert len(re.findall(r"\b" + name + r"\s*\([^;{]*\)\s*\{", hdr)) == 1, name
    assert "struct Key16" in hdr and "kEmitErr" in hdr
    for f in ("okv_merge.hip", "okv_pages.hip"):
        src = open(os.path.join(CSRC, f)).read()
        assert '#include "okv_merge_kernels.hpp"' in src, f
        for name in shared:  # used, never defined again
            assert not re.search(r"__device__[^;{()]*\b" + name + r"\s*\(", src), (f, name)
        assert "struct Key16" not in src and "kEmitErr" not in src.replace("mrg::kEmitErr", "")
        assert "go_outcome(" in src and "term_key(" in src and "key_cmp(" in src, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HIP_SRCS\s*:=.*\bokv_pages\b", mk, re.M)
    assert re.search(r"^HDRS\s*:=.*\bokv_merge_kernels\.hpp\b", mk, re.M)
