set -eo pipefail
OUT=${OUT:-prof_out}/sq
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -s KILL 120 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d "$OUT/a" -o run -- python3 bench.py --full --no-cpu-baseline --no-check --steps 2 --warmup 1 > /dev/null 2> "$OUT/a.err"
F=$(find "$OUT/a" -name '*counter_collection.csv' | head -n 1)
python3 sccg-genome-compression_amd/tools/sq_summary.py "$F" > "$OUT/summary.txt"
rm -rf "$OUT/a"
