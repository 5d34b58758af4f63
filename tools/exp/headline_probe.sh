#!/bin/bash
# Where the headline step's time goes: host profile, kernel trace, and three bench runs.  Writes under $OUT (default: bench_out/).
cd "$(dirname "$0")/../.." || exit 1; export TMPDIR=/tmp
ROOT="$(pwd)"; OUT="${OUT:-$ROOT/bench_out}"; mkdir -p "$OUT"
timeout 300 python tools/headline_host_profile.py > "$OUT/headline_host.txt" 2>&1
rm -rf "$OUT/prof_hl"
(cd /tmp && timeout 300 rocprofv3 --kernel-trace -f csv -d "$OUT/prof_hl" -o hl -- python "$ROOT/tools/headline_host_profile.py" --trace) > "$OUT/headline_trace.log" 2>&1
python tools/headline_host_profile.py --analyse "$(find "$OUT/prof_hl" -name '*kernel_trace.csv' | head -1)" >> "$OUT/headline_host.txt" 2>&1
for i in 1 2 3; do python bench.py --full --steps 20 --warmup 5 --no-cpu --no-gat --no-trainer --no-shard-base --no-papers --no-pmc --no-sage 2>/dev/null | python -c "import json,sys; r=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('bench --steps 20 --warmup 5: value', r['value'], 'ms_per_step', r['ms_per_step'], 'kernel_ms_in_step', r['roofline']['kernel_ms_in_step'])" >> "$OUT/headline_host.txt" 2>&1; done
head -60 "$OUT/headline_host.txt" | cut -c1-180
tail -25 "$OUT/headline_host.txt" | cut -c1-180
