#!/bin/bash
# Round-3 evidence batch (GPU box): the three rocprofv3 passes + bench line (tools/profile.sh), every 1/8 shard and
# the 1/4, 1/2 splits timed alone, the balanced shards of a band-head line list, the --config lines, and the
# kernel trace of the configs[2] / [3] kernels.
set -u
tag=${1:-r03_v1}
out=gpurun_out/$tag
mkdir -p $out
bash tools/profile.sh $tag > $out/profile.log 2>&1; tail -3 $out/profile.log
{
for s in 0/8 1/8 2/8 3/8 4/8 5/8 6/8 7/8 0/4 1/4 2/4 3/4 0/2 1/2; do timeout -k 10 120 python bench.py --full --shard $s --cpu-seconds 0 --steps 100 --warmup 10 2>/dev/null | python -c "
import json,sys; d=json.loads(sys.stdin.read()); r=d['roofline']; print('shard %s: %.3f ms/step  op %.3f  serial: prep %.3f ff %.3f wings %.3f zones %.3f' % (d['config']['sharding'][11:14], d['ms_per_step'], r['coefficient_op_ms_in_timed_steps'], r['sr_prep_kernel_ms'], *[v['ms'] for v in r['kernels'].values()]))"; done
timeout -k 10 200 python tools/balanced_shards.py
} > $out/shards.txt 2>&1; cat $out/shards.txt
for c in 2 3 4; do timeout -k 10 400 python bench.py --config $c --cpu-seconds 8 > $out/config$c.json 2> $out/config$c.err; echo "config $c rc=$?"; done
timeout -k 10 400 python bench.py --config 3 --3d --steps 10 > $out/config3_3d.json 2> $out/config3_3d.err; echo "config 3 3d rc=$?"
timeout -k 10 200 python bench.py --full --rays 64 --cpu-seconds 0 > $out/rays64.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/kt_c2 -o kt -- python3 bench.py --config 2 --steps 3 --warmup 1 --cpu-seconds 0 > /dev/null 2>&1
python3 tools/rocprof_summary.py /tmp/kt_c2/kt_results.db > $out/config2_kernel_trace_stats.txt
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/kt_c3 -o kt -- python3 bench.py --config 3 --steps 4 --warmup 1 --cpu-seconds 0 > /dev/null 2>&1
python3 tools/rocprof_summary.py /tmp/kt_c3/kt_results.db > $out/config3_kernel_trace_stats.txt
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE WRITE_SIZE SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVES -d /tmp/pmc_c3 -o pmc -- python3 bench.py --config 3 --steps 4 --warmup 1 --cpu-seconds 0 > /dev/null 2>&1
python3 tools/rocprof_summary.py /tmp/pmc_c3/pmc_results.db | grep -i "adjoint\|limb\|los_col\|kernel " > $out/config3_pmc_limb_kernels.txt
head -12 $out/config3_kernel_trace_stats.txt
