#!/bin/bash
# one visit: the whole GPU suite, smoke and the bench line (the short form of tools/gpu_round.sh)
# usage (from the repo root): bash tools/gpu_call.sh <output dir>
OUT=${1:?usage: bash tools/gpu_call.sh <output dir>}
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -4
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
CREAM_BENCH_EXTRA=$OUT/call_bench_extra.json timeout 600 python bench.py --full > $OUT/call_bench.json 2> $OUT/call_bench.err; cut -c1-400 $OUT/call_bench.json
