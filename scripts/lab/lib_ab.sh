#!/bin/bash
# A/B of compile-time variants of libpmc.so: parelagmc_amd/lib/libpmc_<v>.so are swapped in on the GPU box's scratch copy
set -e
cd $GRAFT_REPO_ROOT
cp parelagmc_amd/lib/libpmc.so parelagmc_amd/lib/libpmc_base.so
J=$(mktemp)   # the bench line of the current variant
for rep in 1 2; do
for v in base "$@"; do
  cp parelagmc_amd/lib/libpmc_$v.so parelagmc_amd/lib/libpmc.so
  for s in 1 4; do
  python bench.py --full --streams $s --steps 60 --warmup 5 --no-cpu-baseline --no-mlmc --no-r6 > $J 2> $J.err
  python - <<PY
import json
d=json.loads(open("$J").read().strip().splitlines()[-1])
print("$v streams=$s", round(d["value"],1), "K5 us", round(d["roofline"]["avg_kernel_ms"]*1e3,1), round(d["roofline"]["frac"],3), "iso", round(d["roofline"]["isolated"]["frac"],3), "solver", round(d["roofline"]["solver"]["frac"],3))
PY
  done
  if [ $rep = 1 ] && [ -z "$NO_R6" ]; then
  python bench.py --full --refine 6 --streams 1 --steps 6 --warmup 2 --no-cpu-baseline --no-mlmc --no-r6 > $J 2> $J.err
  python - <<PY
import json
d=json.loads(open("$J").read().strip().splitlines()[-1])
print("$v r6", round(d["value"],1), "K5 us", round(d["roofline"]["avg_kernel_ms"]*1e3,1), round(d["roofline"]["frac"],3), "iso", round(d["roofline"]["isolated"]["frac"],3), "solver", round(d["roofline"]["solver"]["frac"],3))
PY
  fi
done
done
