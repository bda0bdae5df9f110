#!/bin/bash
# same-box A/B of sweep builds: ab.sh libA libB ... ; prints value + sweep kernel ms for each, twice
OUT=${OUT:-$PWD/profiles/out}
mkdir -p $OUT
mkdir -p gpurun_out
for rep in 1 2; do
for lib in "$@"; do
  VBNMF_LIB=$PWD/profiles/ubench/libs/$lib python bench.py --full --steps 200 --warmup 10 --no-cpu 2>/dev/null > $OUT/ab_$lib.$rep.log || exit 1
  echo "$lib rep$rep $(grep -o '"value": [0-9.]*\|kernel_ms": [0-9.]*' $OUT/ab_$lib.$rep.log | tr '\n' ' ')"
done
done
