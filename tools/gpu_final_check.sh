#!/bin/bash
# the end-of-work check, timed: the -m gpu suite, smoke(), a plain bench run (the headline alone) and a --full one (every leg)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out/final}
mkdir -p $OUT
( time python -m pytest tests -x -q -m gpu ) > $OUT/gpu_tests.txt 2>&1
( time python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" ) > $OUT/smoke.txt 2>&1
( time python bench.py --steps 20 --warmup 5 ) > $OUT/bench20.json 2> $OUT/bench20.err
( time python bench.py --full ) > $OUT/bench_full.json 2> $OUT/bench_full.err
tail -4 $OUT/gpu_tests.txt; tail -4 $OUT/smoke.txt; tail -4 $OUT/bench20.err; tail -4 $OUT/bench_full.err
python - "$OUT" <<'PY'
import json, sys
d = json.loads(open("%s/bench20.json" % sys.argv[1]).read().strip().splitlines()[-1])
print("bench20", d["value"], d["ms_per_step"], d["steps"])
d = json.loads(open("%s/bench_full.json" % sys.argv[1]).read().strip().splitlines()[-1])
print("bench_full", d["value"], d["ms_per_step"], d["steps"], d["al_round"].get("ms"), d["roofline"]["kernel"], d["roofline"]["frac"], d["cpu_baseline"]["value"])
PY
