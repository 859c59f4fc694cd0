#!/bin/bash
# repeated full default bench runs: every run is gated on parity (verdicts, dealer digests, CPU sample); prints value / fallbacks
#   tools/soak.sh OUTDIR   (the lines and stderr of the runs go to OUTDIR/runN.json, OUTDIR/runN.err)
OUT=${1:?usage: tools/soak.sh OUTDIR}
mkdir -p "$OUT"
for i in 1 2 3 4 5 6; do
  python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/run$i.json" 2> "$OUT/run$i.err" || { echo "run $i FAILED"; tail -5 "$OUT/run$i.err"; }
  python - <<PY
import json
d=json.loads(open('$OUT/run$i.json').read().strip().splitlines()[-1])
print($i, round(d['value']), round(d['compute']['frac'],3), 'fd_fallbacks', d['compute']['fd_fallbacks'], 'dealer', round(d['distribute']['value']), 'W_B', round(d['verify_share']['value']), 'ec', [round(e['value']) for e in d['ec'].values()], 'keys', round(d['registered_keys']['value']))
PY
done
