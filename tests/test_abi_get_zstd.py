"""GetRows on zstd segments, the C-ABI (no GPU): include/okv_sst.h defines OKV_F_GET_ZSTD
and OKV_GET_INFLATED_MAX as objectkv_amd/_lib.py has them, the flag shares its bit with
no other OKV_F_*, the Python entry points take zstd=, the library carries the inflate
arms' kernels, and OKV_ABI_VERSION is still 6."""
from __future__ import annotations

import inspect
import os
import re

from objectkv_amd import _lib
from objectkv_amd import get as G
from objectkv_amd import snap as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "okv_sst.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_flag_and_cap():
    src = _header()
    flags = {m.group(1): int(m.group(2))
             for m in re.finditer(r"#define\s+(OKV_F_\w+)\s+(\d+)u", src)}
    assert flags["OKV_F_GET_ZSTD"] == 128 == _lib.F_GET_ZSTD
    assert all(v & (v - 1) == 0 for v in flags.values())
    assert len(set(flags.values())) == len(flags)  # no two flags share a bit
    m = re.search(r"#define\s+OKV_GET_INFLATED_MAX\s+\(1u\s*<<\s*(\d+)\)", src)
    assert m and 1 << int(m.group(1)) == 1 << 24 == _lib.GET_INFLATED_MAX
    assert re.search(r"#define\s+OKV_ABI_VERSION\s+6\b", src)
    m = re.search(r"#define\s+OKV_BLK_ZSTD_ERROR\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.BLK_ZSTD_ERROR


def test_python_entry_points_take_zstd():
    for fn in (G.get_rows, S.snap_get_rows):
        p = inspect.signature(fn).parameters.get("zstd")
        assert p is not None and p.default is False, fn.__name__


def test_library_carries_the_inflate_arms():
    data = open(_lib.LIB_PATH, "rb").read()
    for stem in (b"zplan", b"zpack", b"zsearch", b"zglobal", b"zfix"):
        for file in (b"get", b"snap"):
            assert b"okv_" + file + b"_" + stem + b"_kernel" in data, (file, stem)
    for name in ("okv_get.hip", "okv_snap.hip", "okv_get_kernels.hpp"):
        src = open(os.path.join(ROOT, "objectkv_amd", "csrc", name)).read()
        assert "getenv" not in src and "knob(" not in src and "OKV_ABLATE" not in src
