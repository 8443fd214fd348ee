#!/bin/bash
# usage: [REPS=5] [FULL=] scripts/ab.sh [bench args]  -- same-box A/B of two library builds (csrc/libmdhip_A.so,
# libmdhip_B.so), alternating.  FULL= (empty) times the plain command, i.e. the headline value without the per-kernel
# events of --full.  Every run has its own time limit and the first failure ends the series.
cd "$(dirname "$0")/.."
mkdir -p bench_out
D=moleculardynamics/jl_amd/csrc
FULL=${FULL---full}
for rep in $(seq 1 ${REPS:-3}); do
  for v in ${VARIANTS:-A B}; do
    cp $D/libmdhip_$v.so $D/libmdhip.so || exit 1
    timeout -k 10 ${RUN_TIMEOUT:-240} python bench.py $FULL --no-cpu-baseline "$@" > bench_out/ab_$v.json 2>bench_out/ab_$v.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v rep $rep: bench.py ended with $rc"; tail -5 bench_out/ab_$v.err; exit $rc; fi
    python -c "
import json
d=json.loads([l for l in open('bench_out/ab_$v.json') if l.startswith('{')][-1])
k=(d.get('roofline') or {}).get('kernel_ms')
print('$v rep $rep: value %.5g ms/step %.4f kern_ms %s'%(d['value'],d['ms_per_step'],'%.4f'%k if k else 'n/a'))" || exit 1
  done
done
