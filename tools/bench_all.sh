#!/bin/bash
# Dev aid (GPU box): the --full bench line of every BASELINE config -> <out>/r3_bench_config<N>.json
# Usage: tools/bench_all.sh [out dir, default $TMPDIR/bench_all]
cd "$(dirname "$0")/.."
OUT=${1:-${TMPDIR:-/tmp}/bench_all}
mkdir -p "$OUT"
for c in 3 2 5 4 1; do
    timeout -k 10 500 python3 bench.py --full --config $c > "$OUT/r3_bench_config$c.json" 2> "$OUT/r3_bench_config$c.err" || echo "config $c failed"
    cut -c1-400 "$OUT/r3_bench_config$c.json"
done
