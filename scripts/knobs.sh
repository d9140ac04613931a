# (per-stage kernel times: a --full run; its output under $BENCH_OUT, default bench_out/)
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
for cfg in "1 2" "2 2" "4 2" "1 4" "1 8" "2 4"; do set -- $cfg; MOSS_PREPROCESS_ITEMS=$1 MOSS_SCATTER_ITEMS=$2 python bench.py --full --no-cpu-baseline --no-callers --steps 100 > "$OUT/tmp_b.json" 2>> "$OUT/tmp_b.err"; python -c "
import json; r=json.load(open('$OUT/tmp_b.json')); print('prep_items $1 scatter_items $2', r['value'], {k: round(v*1000,1) for k,v in r['stages_ms'].items() if k in ('preprocess_fwd','scan','scatter','tile_sort')})"; done
