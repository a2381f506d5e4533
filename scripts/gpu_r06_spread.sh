#!/bin/bash
# r06 spread: XT128 with the next step's A split spread over all 8 column blocks (TIK_XSPLIT_SPREAD build) vs default, same box
cd $GRAFT_REPO_ROOT
O=gpurun_out
TIK_LIB=$GRAFT_REPO_ROOT/build/ab/libtik_spread.so timeout -k 10 200 python -u -m pytest -x -q --timeout 120 --timeout-method thread tests/test_gpu_ik.py -k "golden or batch_invariant or xtws" > $O/pytest_r06sp.log 2>&1 || { tail -20 $O/pytest_r06sp.log; exit 1; }
tail -1 $O/pytest_r06sp.log
for i in 1 2 3; do
  for v in base spread0 spread; do
    TIK_LIB=$PWD/build/ab/libtik_$v.so timeout -k 10 120 python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --no-compare --no-extras > $O/bench_r06sp.json 2> $O/bench_r06sp.err || exit 1
    python -c "
import json;d=json.load(open('$O/bench_r06sp.json'));L=d['forward']['launches']
print('%-6s' % '$v', d['ms_per_step'], ' '.join('%s %.4f' % (k, v['avg_ms']) for k, v in L.items() if k.startswith(('XT128','XH128'))))"
  done
done | tee $O/ab_r06spread.txt
