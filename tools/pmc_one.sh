#!/bin/bash
# One PMC pass (counters given as args) over a short bench run; summary to stdout.
set -o pipefail
B=${B:-4096}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}   # output directory
mkdir -p $OUT/pmc1
rm -rf $OUT/pmc1/*
timeout -k 10 400 rocprofv3 --kernel-trace --pmc "$@" -d $OUT/pmc1/run -o run -f csv -- \
    python3 bench.py --full --batch $B --steps 2 --warmup 1 --no-cpu > $OUT/pmc1/run.log 2>&1 && \
python3 tools/pmc_summary.py $OUT/pmc1 $B $OUT/pmc1/pmc.json
