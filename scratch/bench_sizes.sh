#!/bin/bash
cd "$GRAFT_REPO_ROOT"
mkdir -p scratch/tmp
for b in 1 8; do
  python bench.py --full --steps 3 --warmup 1 --batch $b --no-cpu-baseline > scratch/tmp/bench_b$b.json 2> scratch/tmp/bench_b$b.err || tail -5 scratch/tmp/bench_b$b.err
  python -c "import json; d=json.load(open('scratch/tmp/bench_b$b.json')); print('B=$b', d['value'], d['ms_per_step'], d['stage_ms'])"
done
