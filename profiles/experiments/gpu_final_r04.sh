cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash gpu_final_r04.sh <output directory>}
mkdir -p "$OUT/r04"
timeout -k 10 900 python -m pytest tests -x -q -m gpu --durations=25 > "$OUT/r04/full_final.log" 2>&1
echo "tests rc $?"; tail -4 "$OUT/r04/full_final.log"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout -k 10 400 python bench.py --full > "$OUT/bench_r04_final.json" 2> "$OUT/bench_r04_final.err"
echo "bench rc $?"; cut -c1-200 "$OUT/bench_r04_final.json"
