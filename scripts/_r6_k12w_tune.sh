#!/bin/bash
# K12W (pinned schedule): GPU tests of the GEMM/conv paths, re-time the Linear / 1x1 weight-gradient choices, bench with them
#   bash scripts/_r6_k12w_tune.sh <out dir>
set -e
O=${1:?usage: $0 <out dir>}
mkdir -p $O; rm -rf $O/tuning
timeout -k 10 600 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gemm_gpu.py tests/test_gemmp_gpu.py tests/test_models_gpu.py > $O/tests.log 2>&1
tail -n1 $O/tests.log
timeout -k 10 900 python -u scripts/record_tuning.py --out $O/tuning --keep-table --retime dgrad:* > $O/tuning.log 2>&1
tail -n1 $O/tuning.log
cp $O/tuning/choices_gfx950.json madnn/tuning/choices_gfx950.json
timeout -k 10 600 python -u bench.py --full > $O/bench_default.json 2> $O/bench_default.log
python - $O/bench_default.json <<'PY'
import json, sys
r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("resnet", r["value"], r["config"]["std_batch"]["value"], "gpt2", r["gpt2_pp"]["tokens_per_s"], "tuning", r["config"].get("tuning_timings"))
PY
