#!/bin/bash
# sanity run of a restored tree: the GPU suite, then the default bench line (with --full: the reader wants the roofline and the
# sub-records).  Usage: tools/r4_check.sh OUTDIR
OUT=${1:?usage: tools/r4_check.sh OUTDIR}
mkdir -p $OUT
timeout -k 10 700 python -m pytest tests -x -q -m gpu > $OUT/tests.log 2>&1; rc=$?; echo "pytest exit $rc" >> $OUT/tests.log
tail -3 $OUT/tests.log
[ $rc = 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err; echo "bench exit $?"
python - "$OUT/bench_default.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d.get('kernels_ms_per_step'), d['roofline']['frac'])
print({k: v.get('value') for k, v in d.get('sub_records', {}).items()} if isinstance(d.get('sub_records'), dict) else d.get('sub_records'))
PY
