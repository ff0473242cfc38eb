#!/bin/bash
# tools/gpu_session.sh step: the other BASELINE configs through bench.py's own flags (one GPU); records under $SDN_OUT_DIR (default out/)
# (config 4 without --steps: the whole 256-pose orbit, as the config defines it)
label=$1
out=${SDN_OUT_DIR:-$(cd "$(dirname "$0")/.." && pwd)/out}; mkdir -p $out
for c in 3 4 5; do steps=$([ $c = 4 ] || echo "--steps 5"); SDN_BENCH_DETAIL=$out/${label}_bench_config${c}_1gpu_detail.json timeout 400 python bench.py --config $c $steps --warmup 2 --full --no-cpu-baseline --no-dropin --no-other-configs > $out/${label}_bench_config${c}_1gpu.json 2> $out/${label}_c$c.err; echo "config $c rc=$?"; done
python - <<PY
import json
for c in (3,4,5):
    try:
        d=json.loads(open('$out/${label}_bench_config%d_1gpu.json' % c).read().strip().splitlines()[-1])
        print(c, round(d['value'],3), 'fps', round(d['ms_per_step'],2), 'ms', d['steps'], 'steps', d.get('band_ms'))
    except Exception as e: print(c, 'ERR', e)
PY
