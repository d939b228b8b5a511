#!/bin/bash
# The other BASELINE configs' bench lines: configs[3] large batch (512 images / GPU) and configs[4]
# (celeba128, builder-defined).  TAG=<name>: outputs $OUT/TAG_bench_b512_config3.json and
# $OUT/TAG_bench_celeba128_config4.json (extra env passes through, e.g. ENCDIFF_ATTN_FP8=1).
set -o pipefail
OUT=${OUT:-bench_out}  # where the logs and results go (relative to the repository root)
cd "$(dirname "$0")/.." && mkdir -p $OUT
T=${TAG:-cfg}
timeout -k 10 500 python bench.py --full --batch 512 --skip-cpu --skip-ref-api --skip-ddim --steps 10 --warmup 3 > $OUT/${T}_b512.log 2>&1 || { tail -5 $OUT/${T}_b512.log; exit 1; }
tail -1 $OUT/${T}_b512.log > $OUT/${T}_bench_b512_config3.json
cut -c1-200 $OUT/${T}_bench_b512_config3.json
timeout -k 10 600 python bench.py --full --config celeba128 --skip-cpu --skip-ref-api --steps 10 --warmup 3 > $OUT/${T}_c4.log 2>&1 || { tail -5 $OUT/${T}_c4.log; exit 1; }
tail -1 $OUT/${T}_c4.log > $OUT/${T}_bench_celeba128_config4.json
cut -c1-200 $OUT/${T}_bench_celeba128_config4.json
