#!/bin/bash
# On the GPU box: the long form of tools/ab_run.sh for figures that go into DESIGN -- every variant in build_ab/*
# (tools/ab_build.sh) benched in interleaved rounds, bench.py --steps STEPS --warmup WARMUP (default 50 / 5), one line
# per variant and round (blind-rotate kernel ms).  A variant that crashes stops the run.
#   ROUNDS="1 2 3" bash tools/ab_rounds.sh            (results under $AB_OUT, default ab_out/)
cd "$(dirname "$0")/.."
OUT=${AB_OUT:-ab_out}
mkdir -p "$OUT"
for round in ${ROUNDS:-1 2 3}; do
  for d in build_ab/${ONLY:-*}/; do
    n=$(basename $d)
    j=$OUT/ab_$n.json
    rm -f $j
    TFHE_HIP_LIB=$PWD/$d/libtfhe_hip.so timeout -k 10 300 python bench.py ${BENCH_ARGS:-} --steps ${STEPS:-50} --warmup ${WARMUP:-5} --no-cpu > $j 2>/dev/null
    rc=$?
    if [ ! -s $j ]; then echo "$n CRASHED rc=$rc"; exit 1; fi
    python -c "import json;d=json.load(open('$j'));print('$n', 'round $round', 'PBS/s', d['value'], 'br_ms', d['roofline']['kernel_ms'], 'ks_ms', d['keyswitch_ms'], 'ok', d['decrypt_ok'])"
  done
done
