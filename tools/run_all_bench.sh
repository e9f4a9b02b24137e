#!/bin/bash
# run every bench workload with --full and print the one-line summaries (+ wall seconds)
# usage: tools/run_all_bench.sh <output dir>      (bench_<workload>.json / .err land there)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${1:?usage: run_all_bench.sh <output dir>}; mkdir -p "$OUT"
for w in chain sos fir fftconv; do
  s=$SECONDS
  python $R/bench.py --workload $w --full > "$OUT/bench_$w.json" 2> "$OUT/bench_$w.err"
  echo "$w wall $((SECONDS-s)) s"
done
python - "$OUT" <<'PY'
import json, sys
out = sys.argv[1]
for w in ("chain", "sos", "fir", "fftconv"):
    try:
        d = json.loads(open(f"{out}/bench_{w}.json").read().strip().splitlines()[-1])
        print(w, d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"].get("step_frac"), json.dumps(d["cpu_baseline"])[:420])
    except Exception as e:
        print(w, "FAILED", e)
PY
