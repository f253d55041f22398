#!/bin/bash
# rocprofv3 passes for the bench workload: kernel trace, then PMC passes (each its own run, kernel-trace
# only).  Summaries (text) land in $OUT/prof/*.txt; copy the ones to keep into profiles/.
OUT=${OUT:-logs}   # log directory
mkdir -p $OUT/prof
export TMPDIR=/tmp
R=$(pwd)
ARGS="--steps 5 --warmup 1 --no-cpu-baseline --no-f32-engine $BENCH_ARGS"
echo "== bench --full"; timeout 900 python bench.py --full > $OUT/bench_default.log 2>&1; tail -1 $OUT/bench_default.log
echo "== kernel trace"
rm -rf $OUT/prof/trace
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $R/$OUT/prof/trace -o trace -- python $R/bench.py $ARGS > $R/$OUT/prof/trace.log 2>&1); tail -1 $OUT/prof/trace.log | cut -c1-300
python scripts/rocpd_summary.py $OUT/prof/trace > $OUT/prof/trace_summary.txt 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  echo "== pmc $c"
  rm -rf $OUT/prof/pmc_$c
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --pmc $c -d $R/$OUT/prof/pmc_$c -o pmc -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-f32-engine $BENCH_ARGS > $R/$OUT/prof/pmc_$c.log 2>&1)
  python scripts/rocpd_summary.py $OUT/prof/pmc_$c > $OUT/prof/pmc_${c}_summary.txt 2>&1
done
echo "== pmc SQ"
rm -rf $OUT/prof/pmc_sq
(cd /tmp && timeout 600 rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_IDX_ACTIVE -d $R/$OUT/prof/pmc_sq -o pmc -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-f32-engine $BENCH_ARGS > $R/$OUT/prof/pmc_sq.log 2>&1)
python scripts/rocpd_summary.py $OUT/prof/pmc_sq > $OUT/prof/pmc_sq_summary.txt 2>&1
head -30 $OUT/prof/trace_summary.txt | cut -c1-170
grep -h "flat_scan" $OUT/prof/pmc_*_summary.txt | cut -c1-170
find $OUT/prof -name "*.db" -size +20M -delete; du -sh $OUT/prof
