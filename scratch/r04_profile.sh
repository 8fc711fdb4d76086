#!/bin/bash
# Round-4 profile of the bench workload on the GPU box: per-kernel time (rocprofv3 --kernel-trace --stats) and HBM traffic (two separate
# --pmc passes: FETCH_SIZE, WRITE_SIZE), summarised into profiles/<tag>_*.  usage: bash scratch/r03_profile.sh <tag>
cd "$GRAFT_REPO_ROOT"
mkdir -p scratch/tmp
export TMPDIR=/tmp
TAG=${1:-r04_v1}
rm -rf scratch/tmp/prof_$TAG scratch/tmp/pmcf_$TAG scratch/tmp/pmcw_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d scratch/tmp/prof_$TAG -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-extras > scratch/tmp/prof_$TAG.json 2> scratch/tmp/prof_$TAG.err || tail -5 scratch/tmp/prof_$TAG.err
cp $(ls -t $(find scratch/tmp/prof_$TAG -name '*kernel_stats.csv') | head -1) scratch/tmp/${TAG}_bench_kernel_stats.csv
rocprofv3 --pmc FETCH_SIZE --output-format csv -d scratch/tmp/pmcf_$TAG -- python3 bench.py --full --steps 1 --warmup 0 --decode-tokens 16 --no-cpu-baseline --no-extras > scratch/tmp/pmcf_$TAG.log 2>&1 || tail -5 scratch/tmp/pmcf_$TAG.log
rocprofv3 --pmc WRITE_SIZE --output-format csv -d scratch/tmp/pmcw_$TAG -- python3 bench.py --full --steps 1 --warmup 0 --decode-tokens 16 --no-cpu-baseline --no-extras > scratch/tmp/pmcw_$TAG.log 2>&1 || tail -5 scratch/tmp/pmcw_$TAG.log
python3 scratch/pmc_summarize.py scratch/tmp/pmcf_$TAG scratch/tmp/pmcw_$TAG $TAG
cp profiles/${TAG}_pmc_per_kernel.csv profiles/${TAG}_pmc_traffic.json scratch/tmp/
find scratch/tmp/prof_$TAG scratch/tmp/pmcf_$TAG scratch/tmp/pmcw_$TAG -name '*.csv' -size +2M -delete
head -12 scratch/tmp/${TAG}_bench_kernel_stats.csv
