#!/bin/bash
# usage: tools/bench_stages.sh <tag>  — sweep + build benches (bench.py --full), stage table; the lines in $OUT
tag=$1
out=${OUT:-.}
timeout 600 python bench.py --full --steps 5 --warmup 1 2>&1 | tail -1 > "$out/${tag}_sweep.json"
timeout 600 python bench.py --full --workload cfg3 --steps 5 --warmup 1 2>&1 | tail -1 > "$out/${tag}_build.json"
python - "$out" <<PY
import json, os, sys
for f in ("${tag}_sweep","${tag}_build"):
    d=json.load(open(os.path.join(sys.argv[1], "%s.json"%f))); print(f, round(d["ms_per_step"],3), d["stages_ms_per_step"])
PY
