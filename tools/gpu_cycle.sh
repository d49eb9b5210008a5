#!/bin/bash
# usage: tools/gpu_cycle.sh TAG OUTDIR   -> runs gpu tests, then the full bench under rocprofv3 kernel-trace; outputs under OUTDIR/
TAG=$1
OUT=${2:?usage: tools/gpu_cycle.sh TAG OUTDIR}
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -m gpu -x -q > "$OUT/test_$TAG.log" 2>&1
rc=$?; tail -3 "$OUT/test_$TAG.log"
if [ $rc -ne 0 ]; then echo "TESTS FAILED rc=$rc"; exit $rc; fi
root=$(pwd); cd /tmp && export TMPDIR=/tmp && cd "$root"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -- python3 bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > "$OUT/bench_$TAG.log" 2>&1
grep metric "$OUT/bench_$TAG.log" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms/step',d['ms_per_step'],'value',d['value']); print(d.get('roofline'))"
