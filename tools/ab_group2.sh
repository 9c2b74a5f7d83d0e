#!/bin/bash
# FIXING_FLOAT grouping knobs on C5, alternated.   tools/ab_group2.sh [output directory]
O=${1:-build/ab_group2}; mkdir -p $O
for r in 1 2; do
  for v in "0 1024" "160 256" "160 512" "160 128"; do
    set -- $v
    PSF_FF_GROUP_MB=$1 PSF_FF_GROUP_MMWG=$2 timeout -k 10 200 python bench.py --config c5 --full --no-cpu-baseline > $O/b.json 2>$O/b.err || exit 1
    python -c "import json; d=json.load(open('$O/b.json')); k=d['roofline']['kernels']; print('$v', d['value'], {a: (v['launches'], v['avg_us']) for a, v in k.items()})"
  done
done
