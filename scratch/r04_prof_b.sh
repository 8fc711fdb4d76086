#!/bin/bash
# per-kernel time of the bench workload at another batch size: bash scratch/r04_prof_b.sh <batch>
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp
mkdir -p scratch/tmp
B=${1:-1}
rm -rf scratch/tmp/prof_b$B
rocprofv3 --kernel-trace --stats --output-format csv -d scratch/tmp/prof_b$B -- python3 bench.py --full --batch $B --steps 5 --warmup 2 --no-cpu-baseline --no-extras > scratch/tmp/prof_b$B.json 2> scratch/tmp/prof_b$B.err || tail -5 scratch/tmp/prof_b$B.err
cp $(ls -t $(find scratch/tmp/prof_b$B -name '*kernel_stats.csv') | head -1) scratch/tmp/r04_b${B}_kernel_stats.csv
find scratch/tmp/prof_b$B -name '*.csv' -size +2M -delete
head -12 scratch/tmp/r04_b${B}_kernel_stats.csv | cut -c1-220
