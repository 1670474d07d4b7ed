export GFPL_LIB_DIR=${LIBV:-build/cutprof}
OUT=${OUT:-bench_out}   # output directory
mkdir -p $OUT
timeout -k 10 300 python bench.py --full --batch 16384 --steps 1 --warmup 0 --no-cpu > $OUT/cutprof.log 2>&1; rc=$?
grep -E "cutprof|cutstats|spprof" $OUT/cutprof.log | tail -24; exit $rc
