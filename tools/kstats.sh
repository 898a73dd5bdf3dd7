#!/bin/bash
# Dev aid (on the MI355X): rocprofv3 kernel stats of a short bench run; prints the top kernels and the bench line's ms_per_step.
# Usage: tools/kstats.sh [bench args]   (after the defaults --steps 20 --warmup 2 --no-cpu, so they override them)
#   e.g. tools/kstats.sh --config 4 --steps 45 --warmup 1 --batch 512
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=$(mktemp -d "$TMPDIR/kstats.XXXXXX")
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --steps 20 --warmup 2 --no-cpu "$@" > $OUT/bench.log 2>&1 || { echo "bench under rocprofv3 failed (see $OUT/bench.log)"; tail -3 $OUT/bench.log; exit 1; }
python3 - "$OUT" <<'PY'
import csv, glob, json, sys
out = sys.argv[1]
rows = list(csv.DictReader(open(glob.glob(out + "/prof/*/*kernel_stats.csv")[0])))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:14]:
    print("%-62s calls %6s  avg %9.1f us  total %8.1f ms  %5.1f%%" % (r["Name"].replace("(anonymous namespace)::", "")[:62], r["Calls"],
          float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6, 100 * float(r["TotalDurationNs"]) / tot))
lines = [l for l in open(out + "/bench.log") if l.startswith("{")]
if lines:
    print("ms_per_step", json.loads(lines[-1])["ms_per_step"])
PY
rm -rf $OUT
