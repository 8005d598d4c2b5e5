#!/bin/bash
# the full record (bench.py --full) of every config (1 GPU); stops at the first failure.
# CONFIGS="sac_hopper sac_ant_bf16" to pick, OUT=dir for the logs (default bench_out/ in the repository).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$R/bench_out}
cd $R; mkdir -p $OUT
for C in ${CONFIGS:-sac_hopper ddpg_hcheetah sac_ant sac_ant_bf16 ppo_hcheetah vanilla_sac_hcheetah}; do
  X="--cpu-seconds 5"; [ $C = sac_hopper ] && X=""
  timeout -k 10 400 python -u bench.py --full --trace-dir $OUT --config $C $X ${ARGS} > $OUT/bench_$C.log 2>&1
  tail -1 $OUT/bench_$C.log
done
