# developer: the fused kernel's item headers early on the second stream (ZM_FF_FORK=1) or not, on one box
#   bash tools/ff_fork_ab.sh <output directory>
out=${1:?usage: bash tools/ff_fork_ab.sh <output directory>}
mkdir -p $out
python -m pytest tests -x -q -m gpu -k "fused or coadd or config1 or device_chain" > $out/tests.log 2>&1 || { tail -20 $out/tests.log; exit 1; }
tail -2 $out/tests.log
for f in 0 1 0 1; do
ZM_FF_FORK=$f python bench.py --full --steps 20 --warmup 3 --no-clocks --no-cpu-baseline --no-secondary --no-nightly --no-pipelined > $out/f$f.json 2> $out/f$f.err || exit 1
python - <<P
import json
d=json.loads(open('$out/f$f.json').read().strip().splitlines()[-1])
print('fork $f', 'step', round(d['ms_per_step'],3), 'coadd', round(d['legs']['coadd_ms'],3), 'sub', round(d['legs']['subtract_ms'],3))
P
done
