#!/bin/bash
# Timing of diagnostic library builds (build_diag/VARIANT from tools/diag/variant.py, or lib/libnof_VARIANT.so;
# "" = product) for one precision.
# usage: PREC=f32 tools/diag_lib.sh VARIANT...   (results of diagnostic builds are garbage)
OUT=${OUT:-bench_out}
mkdir -p $OUT
for v in "" "$@"; do
  lib=nerf-or-nothing_amd/lib/libnof${v:+_$v}.so
  [ -n "$v" ] && [ -f build_diag/$v/nerf-or-nothing_amd/lib/libnof.so ] && lib=build_diag/$v/nerf-or-nothing_amd/lib/libnof.so
  NOF_LIB=$PWD/$lib timeout -k 10 120 python bench.py --full --no-cpu-baseline --no-integrator --no-alt --steps 20 --warmup 3 --precision ${PREC:-f32} > $OUT/dl_$v.json 2>/dev/null || exit 1
  python -c "import json; d=json.load(open('$OUT/dl_$v.json')); k=d['kernels']; print('${v:-full}', {n:round(x['avg_launch_ms'],4) for n,x in k.items() if n.startswith(('mlp','wgrad'))})"
done
