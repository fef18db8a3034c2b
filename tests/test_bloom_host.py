"""The device bloom filter's host-checkable parts (no GPU): the shared arithmetic
header okv_bloom_hash.hpp -- the form the kernels of okv_bloom.hip use -- runs
in tests/bloom_hash_main.cpp on the CPU under AddressSanitizer and UBSan
against values from oracle/bloom_ref.py; okv_bloom_estimate against
BloomFilter.with_estimates; and what the built library carries."""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from objectkv_amd import _lib
from oracle import bloom_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")
PRODUCT = os.path.join(ROOT, "objectkv_amd", "libokv_sst.so")

KEY_LENGTHS = list(range(81)) + [255, 256, 4095, 65535]
MS = [1, 2, 63, 64, 65, 1000, 2875518, 2**32 - 5, 2**32, 2**32 + 11, 2**63 + 9, 2**64 - 1]
KS = [1, 2, 3, 4, 5, 20, 33]
KERNELS = (b"okv_bloom_add_lds_kernel", b"okv_bloom_add_global_kernel", b"okv_bloom_test_kernel",
           b"okv_bloom_write_kernel")


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def _case_file(path):
    """Keys, their four base hashes, and for every (m, k) the k locations, all
    from bloom_ref (layout: tests/bloom_hash_main.cpp)."""
    rng = np.random.default_rng(20)
    keys = [rng.integers(0, 256, n, np.uint8).tobytes() for n in KEY_LENGTHS]
    out = [struct.pack("<I", len(keys))]
    for key in keys:
        h = B.BloomFilter._base(key)
        out.append(struct.pack("<I", len(key)) + key + struct.pack("<4Q", *h))
    out.append(struct.pack(f"<I{len(MS)}Q", len(MS), *MS))
    out.append(struct.pack(f"<I{len(KS)}Q", len(KS), *KS))
    f = B.BloomFilter.__new__(B.BloomFilter)
    n = 0
    for key in keys:
        for m in MS:
            for k in KS:
                f.m, f.k = m, k
                locs = list(f._locations(key))
                assert len(locs) == k and all(0 <= x < m for x in locs)
                out.append(struct.pack(f"<{k}Q", *locs))
                n += k
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    return n


def test_hash_header_against_bloom_ref_under_sanitizers(tmp_path):
    """murmur3_x64_128, base_hashes (the shared block loop; n % 16 == 15 adds a
    body block) and location (the reciprocal reduction, m up to 2^64 - 1) equal
    bloom_ref; every key is hashed at offsets 0..7 of a buffer whose words
    without a key byte are poisoned, so a load outside the 'aligned words that
    contain a key byte' aborts."""
    exe = str(tmp_path / "bloom_hash_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(ROOT, "tests", "bloom_hash_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = str(tmp_path / "cases.bin")
    n = _case_file(cases)
    assert n == len(KEY_LENGTHS) * len(MS) * sum(KS)
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_hash_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_bloom_hash.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src


@pytest.mark.parametrize("n,p,want", [
    (100_000, 1e-6, (2875518, 20)), (1, 0.5, None), (1000, 0.01, None), (10**6, 1e-3, None),
    (10**8, 1e-6, None)])
def test_estimate_matches_with_estimates(n, p, want):
    m, k = C.c_uint64(), C.c_uint64()
    _lib.lib().okv_bloom_estimate(n, p, C.byref(m), C.byref(k))
    ref = B.BloomFilter.with_estimates(n, p)
    assert (m.value, k.value) == (ref.m, ref.k)
    if want:
        assert (m.value, k.value) == want


def test_library_carries_the_bloom_kernels_and_reads_no_environment():
    data = open(PRODUCT, "rb").read()
    for name in KERNELS:
        assert name in data, name
    dyn = subprocess.run(["nm", "-D", "--undefined-only", PRODUCT], capture_output=True,
                         text=True, check=True).stdout
    assert not re.search(r"\bgetenv\b", dyn), "the product library imports getenv"
    src = open(os.path.join(CSRC, "okv_bloom.hip")).read()
    assert "getenv" not in src and "knob(" not in src and "OKV_ABLATE" not in src
