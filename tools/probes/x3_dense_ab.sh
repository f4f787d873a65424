#!/bin/bash
# A/B of the dense-row mapping of the x3 layer kernels against whole-window slots with the run-time
# switch (APNEAUQ_X3_DENSE, ops/x3.py), alternating in one session on one box:
#   tools/probes/x3_dense_ab.sh [rounds] [dense layer list]
# Every run is a kernel trace of bench/x3_micro.py --only mcd,de --passes 20 in a process of its own; the
# DENSE template parameter keeps the kernel names apart.  Prints, per layer kernel, the mean and the
# spread (min .. max over the rounds) of its total time in both mappings.  Output: $OUT (bench_out/x3_dense_ab).
set -o pipefail
rounds=${1:-3}; layers=${2:-1,2,3,4}
R=$PWD; export PYTHONPATH=$R
OUT=${OUT:-$R/bench_out/x3_dense_ab}; TRACE=$(mktemp -d); mkdir -p $OUT
for r in $(seq 1 $rounds); do
  for v in slot dense; do
    [ $v = slot ] && sel="" || sel=$layers
    APNEAUQ_X3_DENSE="$sel" timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $TRACE/$v$r -o run -- \
      python3 bench/x3_micro.py --only mcd,de --passes 20 > $OUT/$v$r.log 2>&1 || { echo "$v round $r failed"; tail -20 $OUT/$v$r.log; exit 1; }
    cp $(find $TRACE/$v$r -name "*kernel_stats.csv") $OUT/$v$r.kernel_stats.csv
    grep mcd_batch_ms $OUT/$v$r.log | sed "s/^/$v $r: /"
  done
done
python3 - "$OUT" <<'PY'
import collections, csv, glob, os, re, sys
tot = collections.defaultdict(lambda: collections.defaultdict(list))  # layer shape -> variant -> [ms]
for f in sorted(glob.glob(os.path.join(sys.argv[1], "*.kernel_stats.csv"))):
    v = "dense" if os.path.basename(f).startswith("dense") else "slot"
    for r in csv.DictReader(open(f)):
        m = re.search(r"layer_kernel<([^>]*)>", r["Name"])
        if m:
            a = [t.strip() for t in m.group(1).split(",")]
            tot[", ".join(a[:3])][(v, a[-1] == "true")].append(float(r["TotalDurationNs"]) / 1e6)
print("| kernel <Cin, Cout, k> | slot ms (min .. max) | dense ms (min .. max) | gain | slot spread | dense spread |")
print("|---|---:|---:|---:|---:|---:|")
for k, d in sorted(tot.items()):
    s = d.get(("slot", False), [])
    e = d.get(("dense", True), []) or d.get(("dense", False), [])
    if not s or not e:
        continue
    ms, me = sum(s) / len(s), sum(e) / len(e)
    print(f"| {k} | {ms:.2f} ({min(s):.2f} .. {max(s):.2f}) | {me:.2f} ({min(e):.2f} .. {max(e):.2f}) | "
          f"{100 * (ms - me) / ms:+.2f} % | {100 * (max(s) - min(s)) / ms:.2f} % | {100 * (max(e) - min(e)) / me:.2f} % |")
PY
rm -rf $TRACE
