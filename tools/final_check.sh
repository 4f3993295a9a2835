#!/bin/bash
# Round-end verification on the GPU box: GPU tests, smoke, two default bench runs.
set -o pipefail
O=${OUT_DIR:-out}; mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > $O/final_tests.log 2>&1 || { tail -30 $O/final_tests.log; exit 1; }
tail -3 $O/final_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/final_smoke.log 2>&1 || { tail -20 $O/final_smoke.log; exit 1; }
tail -1 $O/final_smoke.log
timeout -k 10 400 python bench.py --full > $O/final_bench1.json 2> $O/final_bench1.err || { tail -20 $O/final_bench1.err; exit 1; }
timeout -k 10 400 python bench.py --full --cpu-crop 0 > $O/final_bench2.json 2> $O/final_bench2.err || exit 1
python - <<PY
import json
for f in ("$O/final_bench1.json", "$O/final_bench2.json"):
    d = json.load(open(f))
    print(f, d["ms_per_step"], d["value"], d["roofline"]["frac"], d["roofline"]["avg_launch_ms"], d.get("cpu_baseline"))
PY
