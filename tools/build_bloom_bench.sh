#!/bin/bash
# Builds tools/bloom_cpu_bench, the CPU baseline of tools/bloom_bench.py (run from the repo root).
set -e
CXX=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin/clang++
[ -x "$CXX" ] || CXX=${ROCM_PATH:-/opt/rocm}/llvm/bin/clang++
"$CXX" -O2 -std=c++17 -pthread -Iobjectkv_amd/csrc tools/bloom_cpu_bench.cpp -o tools/bloom_cpu_bench
