#!/bin/bash
# bench.py with its default steps and every side measurement (--full), timed from the outside.  Usage: scripts/run_default_bench.sh <outdir>
out=${1:?usage: scripts/run_default_bench.sh <outdir>}
mkdir -p "$out"
s=$(date +%s)
python bench.py --full > "$out/bench_default_stdout.txt" 2> "$out/bench_default_stderr.txt"
echo rc=$? seconds=$(( $(date +%s) - s ))
wc -c "$out/bench_default_stdout.txt"
OUT="$out" python - <<'P'
import json, os
d=json.loads(open(os.path.join(os.environ["OUT"], "bench_default_stdout.txt")).read().strip().splitlines()[-1])
print(d["value"], d["steps"], d["warmup"], d["ms_per_step"], d["roofline"]["kernel_ms"], d["roofline"]["frac"], d["reorder"])
print(json.load(open("bench_full.json"))["phase_seconds"])
P
