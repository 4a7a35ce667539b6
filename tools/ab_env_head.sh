#!/bin/bash
# A/B of one environment switch (0 / 1) on the headline line (128^3), interleaved inside one box:  bash tools/ab_env_head.sh MGCR_SB_REAL
# (results under $AB_OUT, default ab_out/)
VAR=$1; shift
for kv in "$@"; do export "$kv"; done
out=${AB_OUT:-ab_out}
mkdir -p $out
for rep in 1 2 3; do for v in 0 1; do
env $VAR=$v python bench.py --steps 20 --warmup 5 --full --no-extras --no-cpu-baseline > $out/abh_$v.json || exit 1
python - $VAR $v $out <<'P'
import json,sys
var,v,out=sys.argv[1:4]
a=json.loads(open("%s/abh_%s.json"%(out,v)).read().strip().splitlines()[-1])
print(var,v,"headline", round(a["value"]), "max", round(a["timing_repeated"]["it_per_s_max"]), "roofline", a["roofline"]["frac"], flush=True)
P
done; done
