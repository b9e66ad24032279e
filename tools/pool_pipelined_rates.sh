# developer: pool and pipelined rates with the throughput form of the factorisation, one box
#   bash tools/pool_pipelined_rates.sh <output directory>
out=${1:?usage: bash tools/pool_pipelined_rates.sh <output directory>}
mkdir -p $out
python bench.py --full --steps 24 --warmup 3 --no-clocks --no-cpu-baseline --no-secondary --nightly-pools 1,3,4,8,12,16 --nightly-jobs 32 > $out/b.json 2> $out/b.err || { tail -5 $out/b.err; exit 1; }
python - <<P
import json
d=json.loads(open('$out/b.json').read().strip().splitlines()[-1])
print('step', round(d['ms_per_step'],3), 'hp_solve', round(d['kernels']['hp_solve']['ms_per_step'],3), 'sub', round(d['legs']['subtract_ms'],3))
print('  nightly', {k: (round(v['ms_per_subtraction'],3), v['failed']) for k,v in d['nightly']['pools'].items()})
print('  pipelined', {k: d['pipelined'][k] for k in ('ms_per_step','mpix_s','status_ok','subtractions_in_flight')})
P
