#!/bin/bash
# the other configurations (bench.py --full's other_configs leg) + overrep parity tests
#   OUT=<directory for the logs> tools/gpu_cfg_quick.sh
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-build/cfg}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -x -q -k "overrep or config4 or config1" > "$OUT/pytest_cfg.log" 2>&1; echo "pytest rc=$?"; tail -2 "$OUT/pytest_cfg.log"
timeout 600 python bench.py --full --steps 8 --warmup 2 --batches 4 --no-cpu > "$OUT/cfg.log" 2>&1; echo "bench rc=$?"
tail -1 "$OUT/cfg.log" | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(json.dumps(j.get('other_configs'), indent=1))"
