#!/bin/bash
# The non-headline BASELINE configs through bench.py --workload (same JSON schema), plus the R3D-18 step trace and
# PMC traffic.  usage: tools/gpu_r03_workloads.sh TAG
TAG=${1:-r03w}
export RESULTS=${RESULTS:-results}; mkdir -p $RESULTS
export TMPDIR=/tmp
set -o pipefail
for W in r3d fusion ood_fp16; do
  echo "== $W"
  timeout -k 10 400 python bench.py --workload $W --steps 20 --warmup 5 > $RESULTS/${TAG}_${W}.log 2>&1 || exit $?
  tail -1 $RESULTS/${TAG}_${W}.log | cut -c1-200
done
echo "== r3d trace"
tools/prof_step.sh ${TAG}_r3d --workload r3d || exit $?
echo "== r3d pmc"
CMD="python bench.py --workload r3d --steps 2 --warmup 1 --no-trace"
timeout -s KILL 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $RESULTS/${TAG}_r3d_fetch -o run -- \
  python bench.py --workload r3d --steps 2 --warmup 1 --no-trace > $RESULTS/${TAG}_r3d_fetch.log 2>&1 || exit $?
timeout -s KILL 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $RESULTS/${TAG}_r3d_write -o run -- \
  python bench.py --workload r3d --steps 2 --warmup 1 --no-trace > $RESULTS/${TAG}_r3d_write.log 2>&1 || exit $?
python tools/pmc_traffic.py $RESULTS/${TAG}_r3d_fetch $RESULTS/${TAG}_r3d_write $RESULTS/${TAG}_r3d_pmc_traffic.json \
  "$(cat .commit 2>/dev/null)" "$CMD" > $RESULTS/${TAG}_r3d_pmc_traffic.txt 2>&1 || exit $?
find $RESULTS/${TAG}_r3d_fetch $RESULTS/${TAG}_r3d_write -name "*.csv" -size +20M -delete
head -12 $RESULTS/${TAG}_r3d_pmc_traffic.txt
exit 0
