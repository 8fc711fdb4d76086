#!/bin/bash
# bench line + rocprofv3 kernel stats + PMC passes (FETCH_SIZE / WRITE_SIZE in separate runs) of the same workload
cd "$GRAFT_REPO_ROOT"
mkdir -p scratch/tmp
TAG=${1:-r01_v3}
python bench.py --full --steps 3 --warmup 1 > scratch/tmp/bench_$TAG.json 2> scratch/tmp/bench_$TAG.err || { tail -20 scratch/tmp/bench_$TAG.err; exit 1; }
cat scratch/tmp/bench_$TAG.json
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d scratch/tmp/prof_$TAG -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras > scratch/tmp/prof_$TAG.json 2> scratch/tmp/prof_$TAG.err || { tail -20 scratch/tmp/prof_$TAG.err; exit 1; }
echo "stats done"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d scratch/tmp/pmc_fetch_$TAG -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras --decode-tokens 16 > scratch/tmp/pmc_fetch_$TAG.json 2> scratch/tmp/pmc_fetch_$TAG.err || { tail -20 scratch/tmp/pmc_fetch_$TAG.err; exit 1; }
echo "pmc fetch done"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d scratch/tmp/pmc_write_$TAG -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras --decode-tokens 16 > scratch/tmp/pmc_write_$TAG.json 2> scratch/tmp/pmc_write_$TAG.err || { tail -20 scratch/tmp/pmc_write_$TAG.err; exit 1; }
echo "pmc write done"
find scratch/tmp/pmc_fetch_$TAG scratch/tmp/pmc_write_$TAG -name "*.csv" | head
