cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash collect_r04_final.sh <output directory>}
mkdir -p "$OUT"
bash profiles/collect.sh r04_final > "$OUT/collect_r04_final.log" 2>&1
echo "collect rc $?"
timeout -k 10 500 python bench.py --full > "$OUT/bench_r04_final.json" 2> "$OUT/bench_r04_final.err"
echo "bench rc $?"; cut -c1-300 "$OUT/bench_r04_final.json"
