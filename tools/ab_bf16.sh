#!/bin/bash
# A/B of the bf16 bench (C3) between the in-tree library and exp/$VARIANT.so (tools/build_exp.sh), alternating three
# times on one box.  Usage: VARIANT=name tools/ab_bf16.sh
# Logs go to $OUT (default bench_out/abb).
set -o pipefail
cd "$(dirname "$0")/.."
O=${OUT:-bench_out/abb}
mkdir -p $O && export TMPDIR=/tmp
for rep in 1 2 3; do
  for v in base ${VARIANT:?name of an exp/NAME.so build}; do
    if [ $v = base ]; then L=""; else L="NERF_AMD_LIB=$PWD/exp/$v.so"; fi
    env $L timeout -k 10 200 python bench.py --full --precision bf16 --no-cpu-baseline --no-psnr > $O/b_$v.log 2>&1 || { tail -20 $O/b_$v.log; exit 1; }
    echo "$rep $v $(tail -1 $O/b_$v.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); r=d["roofline"]["classes"]; print(d["value"], d["ms_per_step"], {k: v["mean_launch_ms"] for k, v in r.items()})')"
  done
done
