# (per-stage kernel times: a --full run; its output under $BENCH_OUT, default bench_out/)
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
for cfg in "1 0 3" "2 0 2" "2 256 2" "1 256 3"; do set -- $cfg; MOSS_BLEND_WGS_PER_CU=$1 MOSS_FWD_DEBUG=$2 MOSS_BWD_WGS_PER_CU=$3 python bench.py --full --no-cpu-baseline --no-callers --steps 100 > "$OUT/tmp_b.json" 2>> "$OUT/tmp_b.err"; python -c "
import json; r=json.load(open('$OUT/tmp_b.json')); print('fwd_wgs $1 prio $2 bwd_wgs $3', r['value'], {k: round(v*1000,1) for k,v in r['stages_ms'].items() if k.startswith('blend')})"; done
