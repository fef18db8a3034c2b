#!/bin/bash
# CM with and without the merge staging (OKV_MERGE_STAGE), each under a kernel
# trace.  Logs go to $OKV_OUT_DIR (default build/cm_ab, which git ignores).
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
O=${OKV_OUT_DIR:-build/cm_ab}
mkdir -p "$O"
timeout -k 10 300 python3 -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_snapshot_gpu.py > $O/t_snap.log 2>&1 || exit 1
for st in 1 0; do
  OKV_MERGE_STAGE=$st timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/cm_tr$st -o run --output-format csv -- python3 bench.py --full --config cm --no-cpu --no-verify --steps 5 --warmup 2 > $O/cm_tr$st.log 2>&1 || exit 1
done
