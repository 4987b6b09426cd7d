#!/bin/bash
# GPU box: full GPU test suite, then short benches (env variants in $VARIANTS, e.g.
# "SCCG_WALK_CHUNK=8192"; "-" = defaults) and an optional SCCG_DEBUG trace.
# Logs and bench lines go to $OUT/check (default prof_out/check).
set -eo pipefail
OUT=${OUT:-prof_out}/check
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/pytest.log" 2>&1
i=0
for v in ${VARIANTS:--}; do
  if [ "$v" = "-" ]; then v=""; fi
  env $v timeout -k 10 150 python -u bench.py --full --no-cpu-baseline --steps 10 --warmup 2 > "$OUT/bench_$i.json" 2> "$OUT/bench_$i.err"
  echo "$v" > "$OUT/bench_$i.env"
  i=$((i+1))
done
if [ -n "$WALKDBG" ]; then
  SCCG_DEBUG=1 timeout -k 10 200 python -u sccg-genome-compression_amd/tools/dbg_walk.py hg 247249719 249250621 1 > "$OUT/dbg_walk.log" 2>&1
fi
