#!/bin/bash
# rocprofv3 kernel trace of a short bench run → per-kernel summary.  tools/prof_step.sh TAG [bench args...]
export TMPDIR=/tmp RESULTS=${RESULTS:-results}; mkdir -p $RESULTS
TAG=$1; shift
rm -rf $RESULTS/${TAG}_prof
# The table describes the step as a plain bench run executes it (no --full): rocprofv3 times every kernel itself, so
# the bench's own HIP-event bracketing, traced warm-up step and MFMA peak probe would only add launches and stream
# bubbles to the trace.  Pass --full among the bench args to trace that variant instead; the probe stays off then
# (its 4 launches of ~30 ms would dominate the per-kernel table).
export CMHAR_BENCH_PEAK_PROBE=0
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $RESULTS/${TAG}_prof -o run -- \
  python bench.py --steps 4 --warmup 2 --no-cpu-baseline "$@" > $RESULTS/${TAG}_prof.log 2>&1 || exit $?
CMHAR_KSTATS_CONTEXT=${CMHAR_KSTATS_CONTEXT:-FillFunctor,copyBuffer,colsum_rows2} python tools/kstats.py $RESULTS/${TAG}_prof > $RESULTS/${TAG}_kernels.txt
find $RESULTS/${TAG}_prof -name "*kernel_trace.csv" -delete
tail -3 $RESULTS/${TAG}_kernels.txt
