# tests of one keyword + the default bench + rocprofv3 kernel statistics of a 100-step bench: bash scripts/quick_stats.sh <tag> [pytest -k expression]
# (outputs under $BENCH_OUT, default bench_out/; the bench line is a --full one, so that a short timed region carries its long_run)
TAG=${1:-q}; KEXPR=${2:-}
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUT=$(mkdir -p "${BENCH_OUT:-bench_out}" && cd "${BENCH_OUT:-bench_out}" && pwd)
cd "$ROOT"
if [ -n "$KEXPR" ]; then timeout -k 10 600 python -m pytest tests -x -q -m gpu -k "$KEXPR" > $OUT/t_$TAG.log 2>&1; tail -4 $OUT/t_$TAG.log; fi
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-callers > $OUT/b_$TAG.json 2> $OUT/b_$TAG.err; tail -c 300 $OUT/b_$TAG.err
python -c "
import json; d=json.load(open('$OUT/b_$TAG.json')); print('VALUE', d['value'], d['ms_per_step'], d.get('long_run'))"
cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -o ks -- python3 $ROOT/bench.py --steps 100 > $OUT/prof_$TAG.log 2>&1
python3 -c "
import csv,glob
f=glob.glob('$OUT/prof_$TAG/**/*kernel_stats.csv', recursive=True)[0]
tot=0
for r in list(csv.DictReader(open(f)))[:11]:
    print(r['Name'].replace('moss::(anonymous namespace)::','')[:44].ljust(46), r['Calls'].rjust(5), round(float(r['AverageNs'])/1000,1)); 
"
