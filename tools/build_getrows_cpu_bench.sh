#!/bin/bash
# Builds tools/getrows_cpu_bench (host C++ only) against the in-tree product library.
# Runs from any directory; the compiler is ROCm's clang++ (ROCM_PATH, default /opt/rocm).
set -e
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
ROCM="${ROCM_PATH:-/opt/rocm}"
CXX=""
for c in "$ROCM/llvm/bin/clang++" "$ROCM/lib/llvm/bin/clang++"; do
  if [ -x "$c" ]; then CXX="$c"; break; fi
done
[ -n "$CXX" ] || { echo "no clang++ under $ROCM" >&2; exit 1; }
"$CXX" -O2 -std=c++17 -I"$ROOT/include" "$ROOT/tools/getrows_cpu_bench.cpp" \
  -o "$ROOT/tools/getrows_cpu_bench" \
  -L"$ROOT/objectkv_amd" -lokv_sst -Wl,-rpath,'$ORIGIN/../objectkv_amd' -ldl -lpthread
