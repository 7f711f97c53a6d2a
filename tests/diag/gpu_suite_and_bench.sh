set -e
# the GPU suite, then two short --full bench runs (value, ms per step, phase times); logs under $1 (default diag_out/)
OUT=${1:-diag_out}
mkdir -p $OUT
python -m pytest tests -m gpu -q > $OUT/gputest_last.log 2>&1 || { tail -80 $OUT/gputest_last.log | cut -c1-300; exit 1; }
tail -3 $OUT/gputest_last.log
for i in 1 2; do
python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline > $OUT/bench_last_$i.json 2> $OUT/bench_last_$i.err || { tail -30 $OUT/bench_last_$i.err; exit 1; }
python -c "
import json; d=json.loads(open('$OUT/bench_last_$i.json').read().strip().splitlines()[-1]); print('bf16', d['value'], d['ms_per_step'], {k:v.get('ms') for k,v in d['roofline']['phases'].items() if isinstance(v,dict) and 'ms' in v})"
done
