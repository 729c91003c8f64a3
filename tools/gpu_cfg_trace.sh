#!/bin/bash
# kernel trace of the other configurations (bench.py --full's other_configs leg) + the full default bench line
#   OUT=<directory for the log and the trace> tools/gpu_cfg_trace.sh
cd "$GRAFT_REPO_ROOT" || exit 1
export OUT=${OUT:-build/cfg}
mkdir -p "$OUT/prof"
export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof/cfg" -o trace -- python bench.py --full --steps 8 --warmup 2 --batches 4 --no-cpu > "$OUT/cfg_trace.log" 2>&1; echo "trace rc=$?"
tail -1 "$OUT/cfg_trace.log" | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(json.dumps(j.get('other_configs'), indent=1))"
python - <<'PY'
import csv
import os
rows = list(csv.DictReader(open(os.path.join(os.environ["OUT"], "prof", "cfg", "trace_kernel_stats.csv"))))
for r in rows:
    n = r["Name"]
    if n.startswith(("fq_", "void fq", "__amd")):
        print(f"{n[:70]:70s} calls {r['Calls']:>5s} avg {float(r['AverageNs'])/1e6:8.3f} ms total {float(r['TotalDurationNs'])/1e6:9.2f} ms")
PY
