#!/bin/bash
# A/B of environment-selected variants on one box: scripts/ab.sh "VAR=a" "VAR=b" ...   (each runs bench.py --full briefly: its roofline leg prints the per-shape lines)
# prints the JSON value of every variant; its JSON line and per-shape lines stay in $AB_OUT/ab_<i>.json / ab_<i>.log (default: a fresh temporary directory)
OUT=${AB_OUT:-$(mktemp -d)}
mkdir -p "$OUT"
echo "logs in $OUT"
i=0
for v in "$@"; do
  env $v python bench.py --full --steps 1 --warmup 1 --ddim-steps ${AB_DDIM:-20} --no-cpu-baseline ${AB_EXTRAS:---no-extras} > "$OUT/ab_$i.json" 2> "$OUT/ab_$i.log"
  echo "== $v: $(python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(d['value'], d['unit'], d['roofline']['achieved'])" "$OUT/ab_$i.json")"
  i=$((i+1))
done
