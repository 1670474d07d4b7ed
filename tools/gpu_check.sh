#!/bin/bash
# One GPU-box session: parity tests, then the default bench (each step time-limited).
set -o pipefail
OUT=${OUT:-bench_out}   # output directory
mkdir -p $OUT
timeout -k 10 900 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1
rc=$?
tail -5 $OUT/pytest_gpu.log
if [ $rc -ne 0 ]; then echo "pytest rc=$rc"; grep -E "Error|assert|mismatch|differ" $OUT/pytest_gpu.log | head -30; exit $rc; fi
timeout -k 10 600 python bench.py --full "$@" > $OUT/bench.log 2>&1
rc=$?
tail -1 $OUT/bench.log
exit $rc
