#!/bin/bash
# same-box A/B of two builds, KNN families shown: tools/gpu_ab_knn.sh abtmp/lib_a.so abtmp/lib_b.so
cd $GRAFT_REPO_ROOT
for r in 1 2 3; do for lib in "$@"; do
  echo -n "bench $lib: "
  SSDR_AL_LIBRARY=$PWD/$lib timeout 120 python3 bench.py --full --no-cpu-baseline --steps 100 2>/dev/null | grep '^{"metric"' | python3 -c "import sys,json; d=json.loads(sys.stdin.read()); o=d['roofline']['others']; print(d['value'], d['ms_per_step'], d['stage_ms']['knn_pyramid'], {k: o[k]['ms_per_step'] for k in o if k.startswith('knn')})"
done; done
