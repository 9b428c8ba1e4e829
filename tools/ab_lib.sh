#!/bin/bash
# A/B of two builds of the library on the full bench inside one gpurun call: bash tools/ab_lib.sh <other.so>
# (other.so: e.g. make -C vq_seg_amd/csrc ab ABSRC=conv_igemm ABFLAGS=-DSTEM_ABL=1 -> vq_seg_amd/libvqseg_hip_ab.so)
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
LOG=$(mktemp)
for rep in 1 2 3; do
  for lib in "" "$1"; do
    VQSEG_LIB="$lib" timeout -k 10 300 python $ROOT/bench.py --full --no-cpu-baseline > "$LOG" 2>&1
    python3 - "${lib:-in-tree}" "$LOG" <<'PY'
import json, sys
l = json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
print(f"[{sys.argv[1][-40:]:40s}] {l['value']:8.2f} img/s  {l['ms_per_step']:7.2f} ms  roofline {l['roofline']['frac']:.4f}", flush=True)
PY
  done
done
rm -f "$LOG"
