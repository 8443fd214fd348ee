#!/bin/bash
# usage: [REPS=5] scripts/ab_build.sh [bench args] -- same-box A/B of two library builds, reporting the list-build time too.
# Every run has its own time limit and the first failure ends the series.
cd "$(dirname "$0")/.."
mkdir -p bench_out
D=moleculardynamics/jl_amd/csrc
for rep in $(seq 1 ${REPS:-3}); do
  for v in ${VARIANTS:-A B}; do
    cp $D/libmdhip_$v.so $D/libmdhip.so || exit 1
    timeout -k 10 ${RUN_TIMEOUT:-240} python bench.py --full --no-cpu-baseline "$@" > bench_out/ab_$v.json 2>bench_out/ab_$v.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v rep $rep: bench.py ended with $rc"; tail -5 bench_out/ab_$v.err; exit $rc; fi
    python -c "
import json
d=json.loads([l for l in open('bench_out/ab_$v.json') if l.startswith('{')][-1])
b=d['step_breakdown_ms']
print('$v rep $rep: value %.5g ms/step %.4f  ord %.4f prune %.4f build %.4f'%(d['value'],d['ms_per_step'],b['ordinary_kernel'],b['prune_kernel'] or 0,b['list_build'] or 0))" || exit 1
  done
done
