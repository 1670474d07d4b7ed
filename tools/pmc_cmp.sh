#!/bin/bash
# SQ counters of the default build and an experimental build (GFPL_LIB_DIR=$1)
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
B=${B:-4096}
CTRS="SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY"
OUT=${OUT:-bench_out}   # output directory
mkdir -p $OUT/cmp && rm -rf $OUT/cmp/*
for v in base exp; do
  if [ $v = exp ]; then export GFPL_LIB_DIR=$1; fi
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc $CTRS -d $OUT/cmp/$v -o $v -f csv -- \
      python3 bench.py --full --batch $B --steps 2 --warmup 1 --no-cpu > $OUT/cmp/$v.log 2>&1 || exit 1
  python3 tools/pmc_summary.py $OUT/cmp/$v $B $OUT/cmp/$v.json | grep -E "^k_" | cut -c1-220 | sed "s/^/$v /"
done
