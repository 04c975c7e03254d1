#!/bin/bash
# Bench lines for the reference's runtime toggles (useBVH=0, MT, Fresnel) on config 3.
# Results go to $OUT (default bench_out/).
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
TAG=${1:-r02}
for t in brute mt fresnel; do
  timeout -k 10 240 python bench.py --full --no-cpu --$t --steps ${STEPS:-30} --warmup 3 > $OUT/bench_${TAG}_$t.json 2> $OUT/bench_${TAG}_$t.err || { echo "bench --$t failed"; tail -5 $OUT/bench_${TAG}_$t.err; exit 1; }
  python -c "import json,sys; d=json.load(open('$OUT/bench_${TAG}_$t.json')); print('$t', round(d['ms_per_step'],4), 'serial', round(d['serial_ms_per_step'],4), d['roofline']['kernel'])"
done
