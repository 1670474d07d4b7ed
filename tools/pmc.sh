#!/bin/bash
# PMC passes over a short bench run (one counter group per pass, --kernel-trace only,
# as MI355X_MICROARCH.md §rocprofv3 prescribes), then the per-kernel summary.
set -o pipefail
B=${1:-4096}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}   # output directory
mkdir -p $OUT/pmc
run() {  # name counters...
  local name=$1; shift
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc "$@" -d $OUT/pmc/$name -o $name -f csv -- \
      python3 bench.py --full --batch $B --steps 2 --warmup 1 --no-cpu > $OUT/pmc/$name.log 2>&1
}
run fetch FETCH_SIZE && \
run write WRITE_SIZE && \
run sq1 SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY && \
run sq2 SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT GRBM_GUI_ACTIVE GRBM_COUNT && \
python3 tools/pmc_summary.py $OUT/pmc $B $OUT/pmc/pmc_latest.json > $OUT/pmc/summary.txt
rc=$?
cat $OUT/pmc/summary.txt
exit $rc
