#!/bin/bash
# first measured bench line + rocprofv3 kernel stats of the same command
set -e
cd "$GRAFT_REPO_ROOT"
mkdir -p scratch/tmp
python bench.py --full --steps 3 --warmup 1 > scratch/tmp/bench_r01.json 2> scratch/tmp/bench_r01.err || { tail -20 scratch/tmp/bench_r01.err; exit 1; }
cat scratch/tmp/bench_r01.json
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d scratch/tmp/prof_r01 -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > scratch/tmp/prof_bench.json 2> scratch/tmp/prof_bench.err || { tail -20 scratch/tmp/prof_bench.err; exit 1; }
find scratch/tmp/prof_r01 -name "*kernel_stats*" | head
