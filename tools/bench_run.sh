#!/bin/bash
# bench.py --full runs, each under its own time limit: CONFIGS="sac_hopper vanilla_sac_hcheetah" EXTRA="--no-pmc"
# OUT=dir for the logs (default bench_out/ in the repository).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
cd $R
mkdir -p $OUT
for c in ${CONFIGS:-sac_hopper}; do
  timeout -k 10 ${TMO:-600} python -u bench.py --full --trace-dir $OUT --config $c ${EXTRA} > $OUT/bench_$c.log 2>&1 || { tail -30 $OUT/bench_$c.log; exit 1; }
  tail -1 $OUT/bench_$c.log
done
