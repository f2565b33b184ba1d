#!/bin/bash
# last call of the round: what the driver runs at round end, on the committed tree -- the GPU suite, smoke(), its bench command
# (with --full: the reader below wants the roofline, the CPU baseline and the full schedule).  Usage: tools/r4_last.sh OUTDIR
OUT=${1:?usage: tools/r4_last.sh OUTDIR}
mkdir -p $OUT
timeout -k 10 700 python -m pytest tests -x -q -m gpu > $OUT/tests.log 2>&1; rc=$?; echo "pytest exit $rc" >> $OUT/tests.log
tail -3 $OUT/tests.log
[ $rc = 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?"; tail -n 2 $OUT/smoke.log
timeout -k 10 600 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_driver_form.json 2> $OUT/bench.err; echo "bench exit $?"
python - "$OUT/bench_driver_form.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['steps'], d['roofline'], d['cpu_baseline']['value'], d['full_schedule']['bf16']['psnr_db'], d['full_schedule']['fp32']['psnr_db'])
PY
