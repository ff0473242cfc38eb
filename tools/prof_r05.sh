#!/bin/bash
# Round-5 evidence, all on one box:  tools/gpu_session.sh <label> prof_r05
#   PMC passes first (so that the bench line of the same session finds a profile of THIS build for `roofline.traffic`), kernel
#   trace + timeline of the driver's bench command, stall passes, the bench with --full, then the whole GPU suite.  Records
#   under $SDN_OUT_DIR (default out/).
T=$1
R=$(cd "$(dirname "$0")/.." && pwd); O=${SDN_OUT_DIR:-$R/out}; cd $R; mkdir -p $O
C="$(cat tools/.commit 2>/dev/null)"
cd /tmp && export TMPDIR=/tmp
P=/tmp/prof_$T
timeout 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $P/f -o f -- python $R/tools/frame_once.py fused 3 > $O/prof.log 2>&1
python $R/tools/rocpd_stats.py $P/f/f_results.db 8 _kernel > $O/${T}_pmc_fetch.md
timeout 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $P/w -o w -- python $R/tools/frame_once.py fused 3 >> $O/prof.log 2>&1
python $R/tools/rocpd_stats.py $P/w/w_results.db 8 _kernel > $O/${T}_pmc_write.md
timeout 200 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_WAIT_ANY GRBM_GUI_ACTIVE -d $P/m -o m -- python $R/tools/frame_once.py fused 3 >> $O/prof.log 2>&1
python $R/tools/rocpd_stats.py $P/m/m_results.db 8 _kernel > $O/${T}_pmc_mfma.md
SDN_FIELD_SINGLE_KERNEL=0 timeout 200 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $P/f2 -o f2 -- python $R/tools/frame_once.py fused 3 >> $O/prof.log 2>&1
SDN_FIELD_SINGLE_KERNEL=0 timeout 200 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $P/w2 -o w2 -- python $R/tools/frame_once.py fused 3 >> $O/prof.log 2>&1
python $R/tools/pmc_traffic.py $P/f/f_results.db $P/w/w_results.db $P/m/m_results.db "$C" $P/f2/f2_results.db $P/w2/w2_results.db > $O/${T}_pmc_traffic.json
cp $O/${T}_pmc_traffic.json $R/profiles/r05_pmc_traffic.json
echo "pmc done ($(date +%T))"
MIOPEN_FIND_MODE=FAST timeout 300 rocprofv3 --kernel-trace --stats -d $P/k -o k -- python $R/bench.py --steps 20 --warmup 5 --profile > $O/${T}_bench_under_rocprof.json 2>> $O/prof.log
python $R/tools/rocpd_stats.py $P/k/k_results.db 16 > $O/${T}_kernel_stats.md
python $R/tools/rocpd_timeline.py $P/k/k_results.db 12 2 > $O/${T}_timeline.md
cd $R && bash tools/prof_stall.sh $T > /dev/null 2>&1
echo "traces done ($(date +%T))"
timeout 600 python bench.py --full > $O/${T}_bench_final.json 2> $O/${T}_bench_final.err; echo "bench (defaults, --full) rc=$?"
timeout 400 python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-dropin --no-other-configs > $O/${T}_bench_20steps.json 2>/dev/null; echo "bench 20 steps rc=$?"
python - <<PY
import json
for f in ('${T}_bench_final.json', '${T}_bench_20steps.json'):
    d=json.loads(open('$O/' + f).read().strip().splitlines()[-1])
    r=d['roofline']
    print(f, {k:d[k] for k in ('value','ms_per_step','frame_ms_p10_p50_p90')}, 'field', r['avg_launch_ms'], r['frac'], r.get('achieved_counting_skipped_colour_branch'), 'traffic', r['traffic'], 'cnn', d['roofline_cnn']['avg_ms_in_timed_region'], d['roofline_cnn']['alone_ms'])
    print('   grid dram', d['roofline_grid_sampler'].get('dram_GBps_from_profile'), 'sky', (d.get('roofline_sky') or {}).get('frac'), 'precision', d.get('precision',{}).get('max_abs_err'), (d.get('precision',{}).get('vs_gpu_placement_fp32_path') or {}).get('max_abs_diff'), 'fallback fps', d.get('fallback_fp32_path_frames_per_s'), 'cpu', (d.get('cpu_baseline') or {}).get('value'), 'dropin', [(x.get('frames_per_s')) for x in (d.get('dropin') or {}).get('runs', [])], (d.get('dropin') or {}).get('max_abs_diff_vs_renderer'))
PY
tail -3 $O/${T}_timeline.md
timeout 1500 python -m pytest tests -m gpu -q -s --durations=15 > $O/${T}_pytest_gpu_final.log 2>&1; echo "pytest rc=$?"; tail -2 $O/${T}_pytest_gpu_final.log
timeout 300 python __graft_entry__.py smoke > $O/${T}_smoke.log 2>&1; echo "smoke rc=$?"; grep "\[smoke\]" $O/${T}_smoke.log
