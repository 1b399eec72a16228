#!/bin/bash
# Round-end evidence on the GPU box: the full bench (--full), a rocprofv3 kernel-trace/stats run
# of the same command, and the two PMC traffic passes.  Outputs under $OUT (default: profile_out/).
# usage: tools/profile_round.sh <tag>
TAG=${1:-rXX}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-$R/profile_out}
mkdir -p $OUT
cd $R && timeout -k 10 300 python3 bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit 1
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof_bench
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_bench -- python3 $R/bench.py --full --no-cpu-baseline --no-alt-mode > $OUT/prof_bench.log 2>&1 || exit 1
cp $(find $OUT/prof_bench -name "*kernel_stats.csv" | head -1) $OUT/kernel_stats_$TAG.csv
cd $R && timeout -k 10 500 bash tools/traffic_run.sh || exit 1
cp gpurun_out/traffic.json gpurun_out/traffic_$TAG.json
tail -c 600 $OUT/bench_$TAG.json
