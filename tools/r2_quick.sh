#!/bin/bash
# quick GPU check after a tail-kernel change: its parity tests, then the default bench line
set -o pipefail
O=${OUT_DIR:-out}; mkdir -p "$O"
timeout -k 10 600 python -m pytest tests/test_gpu_ops.py tests/test_gpu_model.py -m gpu -x -q -k "ffn2 or hab_tail or headline or tiny or cfg or ocab or plan or linear or conv" > $O/quick_tests.log 2>&1 || { tail -30 $O/quick_tests.log; exit 1; }
tail -2 $O/quick_tests.log
timeout -k 10 400 python bench.py --full --no-f32-path > $O/quick_bench.json 2> $O/quick_bench.err || { tail -20 $O/quick_bench.err; exit 1; }
python - <<PY
import json
d = json.loads([l for l in open("$O/quick_bench.json") if l.startswith("{")][-1])
print(d["ms_per_step"], d["value"], d["roofline"]["kernel"], d["roofline"]["frac"], d["roofline"].get("avg_ms"))
PY
