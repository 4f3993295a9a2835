#!/bin/bash
# A/B on ONE box: default bench with and without an environment switch, twice each, interleaved.  usage: tools/ab_env.sh VAR=VALUE
set -o pipefail
O=${OUT_DIR:-out}; mkdir -p "$O"
for i in 1 2; do
  for arm in base "$1"; do
    if [ "$arm" = base ]; then
      timeout -k 10 300 python bench.py --full --no-f32-path --cpu-crop 0 > $O/ab.json 2> $O/ab.err || { tail -20 $O/ab.err; exit 1; }
    else
      env "$arm" timeout -k 10 300 python bench.py --full --no-f32-path --cpu-crop 0 > $O/ab.json 2> $O/ab.err || { tail -20 $O/ab.err; exit 1; }
    fi
    python - "$arm" <<PY
import json, sys
d = json.loads([l for l in open("$O/ab.json") if l.startswith("{")][-1])
print(sys.argv[1], d["ms_per_step"], d["roofline"]["kernel"], d["roofline"]["frac"], flush=True)
PY
  done
done
