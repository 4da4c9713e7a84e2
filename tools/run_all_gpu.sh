#!/bin/bash
# full GPU suite + the default bench line with --full      bash tools/run_all_gpu.sh OUT   (OUT: output directory)
O=${1:?usage: bash tools/run_all_gpu.sh OUT}
mkdir -p $O
timeout 1500 python -m pytest tests -x -q -m gpu > $O/pytest_gpu.log 2>&1; echo pytest rc=$?
tail -5 $O/pytest_gpu.log
timeout 900 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; echo bench rc=$?
python - "$O" <<'PY'
import json, sys
r = json.load(open(sys.argv[1] + "/bench_default.json"))
print(r["metric"], r["value"], r["ms_per_step"], r["roofline"]["frac"], r["setup_seconds"], r["setup_breakdown"], r.get("cpu_baseline", {}).get("value"))
s = r.get("secondary", {}).get("c3")
if s:
    print("c3:", s["value"], s["ms_per_step"], s["roofline"]["frac"], s["setup_seconds"], s["setup_breakdown"], s["device_memory"])
PY
tail -3 $O/bench_default.err
