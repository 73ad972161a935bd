#!/bin/bash
# The bench step with alternative library builds (CMHAR_LIB), alternated twice.  usage: lib_step_ab.sh TAG lib...
TAG=$1; shift
set -o pipefail
export TMPDIR=/tmp
export RESULTS=${RESULTS:-results}; mkdir -p $RESULTS
for rep in 1 2; do
  for lib in "$@"; do
    n=$(basename $lib .so)
    CMHAR_LIB=$PWD/$lib timeout -k 10 300 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline \
      > $RESULTS/${TAG}_${n}_${rep}.log 2>&1 || exit $?
    echo "$n rep=$rep $(tail -1 $RESULTS/${TAG}_${n}_${rep}.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); k=d["kernels"]; print(d["value"], d["ms_per_step"], {a: b["ms_per_step"] for a, b in k.items()})')"
  done
done
exit 0
