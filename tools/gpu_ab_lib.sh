#!/bin/bash
# A/B of two BUILDS of libmisonet_hip.so ON ONE BOX (boxes differ by ~8 % in sustained clocks): alternate the arms.
# usage: gpu_ab_lib.sh libA.so libB.so [rounds] [extra bench args]
R=${GRAFT_REPO_ROOT:-/root/repo}
A="$1"; B="$2"; N=${3:-3}; shift 3
for i in $(seq $N); do
  for ARM in "$A" "$B"; do
    V=$(MISONET_LIB_PATH=$R/$ARM timeout 300 python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-alt "$@" 2>/dev/null | python -c "
import sys,json
d=json.loads(sys.stdin.read()); r=d.get('roofline') or {}
print(d['value'], 'utt/s  conv', r.get('achieved'), 'TF/s', (r.get('time_share') or {}))")
    echo "round $i  [$ARM]  $V"
  done
done
