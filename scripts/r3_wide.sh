#!/bin/bash
# BASELINE configs[4] geometry on one GPU: per-kernel breakdown of the fp8 and bf16 steps
OUT=${OUT:-out}; export OUT; mkdir -p "$OUT"      # results go under $OUT (default: out/ in the repository root)
mkdir -p $OUT/r3w
for dt in ${DTYPES:-fp8 bf16}; do
  python bench.py --full --hidden 4096 --batch 8192 --dtype $dt --steps 20 --warmup 5 --no-cpu-baseline ${BENCH_ARGS} > $OUT/r3w/$dt.json 2> $OUT/r3w/$dt.err || exit 1
  python - $dt <<'PY'
import json, os, sys
d=json.loads(open(os.environ['OUT'] + '/r3w/%s.json'%sys.argv[1]).read().strip().splitlines()[-1])
r=d['roofline']; st=r['step']
print(sys.argv[1], 'ms/step %.4f  frac %.4f  allk %.4f'%(d['ms_per_step'], r['frac'], st['all_kernels_ms']))
for k,v in list(st['kernel_ms'].items())[:18]: print('   %-66s %.4f  x%.0f'%(k[:66],v,st['kernel_launches'][k]))
PY
done
