"""FSE-compressed Huffman weights in the device zstd encoder, the C-ABI (no GPU):
include/okv_sst.h defines OKV_F_ZSTD_HUF_FSE and OKV_PATH_ZSTD_HUF_FSE as objectkv_amd/_lib.py
has them, neither shares its bit with another, the Python entry points take zstd_huffman_fse=,
the library carries okv_zenc_unit_fse_kernel beside the two earlier unit kernels, and
OKV_ABI_VERSION is still 6."""
from __future__ import annotations

import inspect
import os
import re

import objectkv_amd as okv
from objectkv_amd import _lib
from objectkv_amd import snapshot as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "okv_sst.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_flag_and_path_bit():
    src = _header()
    for prefix in ("OKV_F_", "OKV_PATH_"):
        vals = {m.group(1): int(m.group(2))
                for m in re.finditer(r"#define\s+(%s\w+)\s+(\d+)u" % prefix, src)}
        assert all(v & (v - 1) == 0 for v in vals.values()), prefix
        assert len(set(vals.values())) == len(vals), prefix  # no two share a bit
        if prefix == "OKV_F_":
            assert vals["OKV_F_ZSTD_HUF_FSE"] == 512 == _lib.F_ZSTD_HUF_FSE
            assert vals["OKV_F_ZSTD_HUFFMAN"] == 256 == _lib.F_ZSTD_HUFFMAN
        else:
            assert vals["OKV_PATH_ZSTD_HUF_FSE"] == 131072 == _lib.PATH_ZSTD_HUF_FSE
            assert vals["OKV_PATH_ZSTD_HUF"] == 65536 == _lib.PATH_ZSTD_HUF
    assert re.search(r"#define\s+OKV_ABI_VERSION\s+6\b", src)


def test_python_entry_points_take_the_keyword():
    for fn in (okv.Encoder.encode, okv.Encoder.encode_device, okv.GpuSegmentWriter.__init__,
               SN.compact):
        p = inspect.signature(fn).parameters.get("zstd_huffman_fse")
        assert p is not None and p.default is False, fn.__qualname__


def test_library_carries_the_three_unit_kernels():
    data = open(_lib.LIB_PATH, "rb").read()
    for name in (b"okv_zenc_unit_kernel", b"okv_zenc_unit_huf_kernel",
                 b"okv_zenc_unit_fse_kernel"):
        assert name in data, name
