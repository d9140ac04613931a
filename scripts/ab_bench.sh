# A/B of kernel variants through the DIAGNOSTIC build: bash scripts/ab_bench.sh "<label> ENV=.. ENV=.." ...   (one bench run per argument)
# prints value, ms/step and the per-stage kernel times of each (a --full run: they come from its per-kernel replay); results under
# $BENCH_OUT/ab_<label>.json (default bench_out/)
OUT=${BENCH_OUT:-bench_out}; mkdir -p "$OUT"
for spec in "$@"; do
  set -- $spec; label=$1; shift
  env MOSS_AMD_LIB_DIR=lib_diag "$@" python bench.py --full --no-callers --no-cpu-baseline --steps 200 > "$OUT/ab_$label.json" 2> "$OUT/ab_$label.err"
  python - "$label" "$OUT" <<'PY'
import json, sys
lab, out = sys.argv[1], sys.argv[2]
try:
    d = json.load(open(f"{out}/ab_{lab}.json"))
    st = d["stages_ms"]
    print(f"{lab:14s} {d['value']:8.1f} it/s {d['ms_per_step']*1000:7.1f} us | " + " ".join(f"{k}={v*1000:.1f}" for k, v in st.items()) + f" | sum={sum(st.values())*1000:.1f}")
except Exception as e:
    print(lab, "FAILED", e, open(f"{out}/ab_{lab}.err").read()[-800:])
PY
done
