#!/bin/bash
# A/B of library variants on the headline line (one-launch and three-kernel path) and the 256^3 workload:
#   bash tools/ab_bench.sh head pin2     (tools/build/ab/lib_<name>.so; results under $AB_OUT, default ab_out/)
L=mgpreconditionedgcr_amd/libmgcr_hip.so
out=${AB_OUT:-ab_out}
mkdir -p $out
cp $L $out/lib_keep.so
for rep in 1 2; do
for v in "$@"; do
  cp tools/build/ab/lib_$v.so $L || exit 1
  python bench.py --steps 20 --warmup 5 --full --no-extras --no-cpu-baseline > $out/ab_$v.json || exit 1
  MGCR_STEPBUILD=0 python bench.py --steps 20 --warmup 5 --full --no-extras --no-cpu-baseline > $out/ab3_$v.json || exit 1
  python bench.py --workload poisson256_gcr > $out/ab256_$v.json || exit 1
  python - "$v" "$out" <<'P'
import json,sys
v,out=sys.argv[1:3]
a=json.loads(open("%s/ab_%s.json"%(out,v)).read().strip().splitlines()[-1])
b=json.loads(open("%s/ab3_%s.json"%(out,v)).read().strip().splitlines()[-1])
c=json.loads(open("%s/ab256_%s.json"%(out,v)).read().strip().splitlines()[-1])
print(v, "one-launch", round(a["value"]), "min", round(a["timing_repeated"]["it_per_s_max"]), "| three-kernel", round(b["value"]), "max", round(b["timing_repeated"]["it_per_s_max"]), [round(b["phases"][k]["us_per_iteration"],1) for k in ("xr","apply_dots","build")], "| 256^3", round(c["it_per_s"],1), [round(c["phases"][k]["us_per_iteration"],1) for k in ("xr","apply_dots","build")], flush=True)
P
done
done
cp $out/lib_keep.so $L
