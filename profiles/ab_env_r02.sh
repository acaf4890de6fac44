#!/bin/bash
# Development aid: the hg38-scale workload under different environment knobs within ONE box lease (the index is built once).
#   bash profiles/ab_env_r02.sh <tag> NAME:VAR=value[,VAR=value...] ...    -> gpurun_out/ab_<tag>/*.json + summary.txt
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-env}; shift
OUT=$R/gpurun_out/ab_$TAG
mkdir -p $OUT
cd $R
ARGS="--full --cpu-sample 0 --no-gather-probe --no-ingest --steps 20 --warmup 5"
run() {   # name, env assignments...
	local name=$1; shift
	env "$@" VARGENO_VERBOSE=1 python3 bench.py $ARGS > $OUT/$name.json 2> $OUT/$name.err
	python3 - $OUT/$name.json $name <<'PY' | tee -a $OUT/summary.txt
import json, sys
try:
    j = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
    d = j["device_ms_per_step"]
    print("%-12s reads/s %.4g  ms/step %.3f  wave %.3f  pack %.3f  tiers %.3f (deep %.3f)  frac %.3f  spilled %s" % (sys.argv[2], j["value"], j["ms_per_step"], d["wave"], d["pack"], d["spill_tiers_overlapped"], d["of_which_deep_list_wave_tier"], j["roofline"]["frac"], j["reads_per_step_spilled_to_lane_tier"]))
except Exception as e:
    print(sys.argv[2], "FAILED", e)
PY
}
run base
grep -E "vargeno index:|resident|parity" $OUT/base.err | tee -a $OUT/summary.txt
for spec in "$@"; do
	name=${spec%%:*}
	run $name $(echo ${spec#*:} | tr ',' ' ')
	grep -E "parity" $OUT/$name.err | tee -a $OUT/summary.txt
done
run base2
