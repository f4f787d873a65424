#!/bin/bash
# One GPU call: selected GPU tests, then the full bench (and optionally a kernel-trace profile of it).
#   tools/gpu_quick.sh tag "pytest selection" [prof]    (logs go to $APNEAUQ_OUT, default bench_out/)
set -o pipefail
tag=$1; sel=$2; prof=$3
out=${APNEAUQ_OUT:-bench_out}
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest $sel -m gpu -x -v --timeout 240 --timeout-method thread > "$out/${tag}_tests.log" 2>&1
rc=$?; tail -4 "$out/${tag}_tests.log"
[ $rc -eq 0 ] || { echo "TESTS FAILED rc=$rc"; grep -E "Error|error|assert|FAILED" "$out/${tag}_tests.log" | head -30; exit $rc; }
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err" || { echo BENCH FAILED; tail -20 "$out/${tag}_bench.err"; exit 1; }
python tools/bench_brief.py "$out/${tag}_bench.json"
if [ -n "$prof" ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_prof" -o p -- python3 bench.py --full --steps 3 --warmup 1 --no-deviation > "$out/${tag}_prof.log" 2>&1 || { echo PROF FAILED; tail "$out/${tag}_prof.log"; exit 1; }
  f=$(find "$out/${tag}_prof" -name "*kernel_stats.csv" | head -1); python tools/prof_summary.py $f 14
fi
