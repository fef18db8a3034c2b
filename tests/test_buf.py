"""okv::Buf, the owning type of every scratch allocation (okv_buf.hpp): its
failure paths run on the CPU, in tests/buf_main.cpp, over a malloc-backed
memory source that can fail the k-th allocation.  Built with the ROCm clang
under AddressSanitizer and UBSan; host only, links no HIP, no GPU needed."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "objectkv_amd", "csrc")


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for sub in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
        path = os.path.join(rocm, sub)
        if os.path.exists(path):
            return path
    raise AssertionError(f"no clang++ under {rocm}")


def test_buf_failure_paths_under_sanitizers(tmp_path):
    exe = str(tmp_path / "buf_main")
    build = subprocess.run(
        [_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
         os.path.join(ROOT, "tests", "buf_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_buf_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, "okv_buf.hpp")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
