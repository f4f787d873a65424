#!/bin/bash
# One GPU call: the WHOLE GPU test tier, then bench.py --full and a kernel-trace profile of it.
#   tools/gpu_full.sh tag                               (logs go to $APNEAUQ_OUT, default bench_out/)
set -o pipefail
tag=$1
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root"
out=${APNEAUQ_OUT:-$root/bench_out}
mkdir -p "$out"
export TMPDIR=/tmp
timeout -k 10 1000 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread -p no:cacheprovider \
  > "$out/${tag}_suite.log" 2>&1
rc=$?
grep -E "FAILED|ERROR" "$out/${tag}_suite.log" | head -30
tail -2 "$out/${tag}_suite.log"
case $rc in 0|1) ;; *) echo "pytest rc=$rc: stopping"; exit $rc;; esac
timeout -k 10 500 python bench.py --full --steps 20 --warmup 5 > "$out/${tag}_bench.json" 2> "$out/${tag}_bench.err" \
  || { echo BENCH FAILED; tail -20 "$out/${tag}_bench.err"; exit 1; }
python tools/bench_brief.py "$out/${tag}_bench.json"
cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/${tag}_prof" -o p -- \
  python3 "$root/bench.py" --full --steps 3 --warmup 1 --no-deviation > "$out/${tag}_prof.log" 2>&1 \
  || { echo PROF FAILED; tail "$out/${tag}_prof.log"; exit 1; }
cd "$root"
f=$(find "$out/${tag}_prof" -name "*kernel_stats.csv" | head -1); python tools/prof_summary.py $f 30
exit $rc
