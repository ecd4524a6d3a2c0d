cd $GRAFT_REPO_ROOT
OUT=${1:?usage: bash bench_r04_mid.sh <output directory>}
mkdir -p "$OUT/r04"
timeout -k 10 500 python bench.py --full > "$OUT/r04/bench_n1.json" 2> "$OUT/r04/bench_n1.err"
echo "n1 rc $?"; cut -c1-700 "$OUT/r04/bench_n1.json"
MGGCN_BENCH_REHEARSAL=1 timeout -k 10 600 python bench.py --gpus 4 --steps 3 --warmup 1 --full > "$OUT/r04/bench_rehearsal4.json" 2> "$OUT/r04/bench_rehearsal4.err"
echo "rehearsal4 rc $?"; python3 -c "
import json, sys; j=json.load(open(sys.argv[1])); print({k:v for k,v in j.items() if k.startswith('cli') or k in ('value','n_gpus','loss_first_last')}); print(j['comm'])" "$OUT/r04/bench_rehearsal4.json"
