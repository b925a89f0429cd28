# Round-end record, from the repository root on a GPU host: the GPU tests, smoke() and the full
# benchmark line, kept under $OUT/<name> (default build/<name>).  usage: bash tools/gpu_round_end.sh [name]
set -o pipefail
R=${1:-round_end}
OUT=${OUT:-build}/$R
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q > "$OUT/gpu_tests.log" 2>&1 && \
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.txt" 2>&1 && \
timeout -k 10 400 python -u bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
