#!/bin/bash
# Runs on the GPU box (via gpurun): the round's judged artifacts in one call.
#   tools/round_artifacts.sh <tag>
# -> gpurun_out/<tag>/bench_final.json, workload_*.json, pytest_gpu.txt and gpurun_out/prof_<tag>/ (rocprofv3)
set -u
TAG=${1:-r2}
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/$TAG
mkdir -p $O
cd $R
# both libraries from THIS tree first: a stale development library once overwrote three evidence files with tracebacks
# 
python -m gglasso_amd.build --dev || { echo "build failed"; exit 1; }
# keep <file> <command...>: run the command, keep its output only if it exited 0 and holds no traceback
FAILED=""
keep() {
  local out=$1; shift
  if "$@" > $out.tmp 2>&1 && ! grep -q "Traceback" $out.tmp; then mv $out.tmp $out
  else echo "FAILED: $* (output left in $out.failed)"; mv $out.tmp $out.failed; FAILED="$FAILED $(basename $out)"; fi
}
( time python -m pytest tests -m gpu -x -q --durations=10 ) > $O/pytest_gpu.txt 2>&1
tail -4 $O/pytest_gpu.txt
bash tools/profile_round.sh $TAG > $O/profile.log 2>&1
cd $R
python bench.py --full > $O/bench_final.log 2>&1
grep "^{" $O/bench_final.log > $O/bench_final.json
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>&1 | grep "^{" > $O/bench_driver_args.json
for w in ggl_K20_p200 ggl_K4_p500 ggl_K8_p500 ggl_K16_p500 ggl_K32_p1000 fgl_K50_p500_latent ggl_K256_p1000 ggl_K64_p100 ggl_K256_p64 ggl_K32_p128; do
  python bench.py --full --workload $w --steps 30 --warmup 8 --regions 5 --no-cpu-baseline 2>&1 | grep "^{" > $O/workload_$w.json
done
python bench.py --full --opt ns_tol=0 --no-cpu-baseline 2>&1 | grep "^{" > $O/workload_ggl_K32_p500_exact_omega_step.json
python bench.py --full --opt ns_mode=2 --steps 40 --warmup 10 --no-cpu-baseline 2>&1 | grep "^{" > $O/workload_ggl_K32_p500_stable.json
python bench.py --full --eig 2 --steps 10 --warmup 3 --regions 3 --no-cpu-baseline 2>&1 | grep "^{" > $O/workload_ggl_K32_p500_rocsolver.json
for w in ggl_K4_p500 ggl_K8_p500; do
  GGL_BENCH_FORCE_DIST=1 python bench.py --full --workload $w --steps 30 --warmup 8 --regions 5 --no-cpu-baseline --comm capi 2>&1 | grep "^{" > $O/workload_${w}_sharded_1rank_rccl_capi.json
done
GGL_BENCH_FORCE_DIST=1 python bench.py --full --workload ggl_K4_p500 --steps 30 --warmup 8 --regions 5 --no-cpu-baseline --comm torch 2>&1 | grep "^{" > $O/workload_ggl_K4_p500_sharded_1rank_torch.json
T=$(find $R/gpurun_out/prof_$TAG/stats -name "*kernel_trace.csv" | head -1)
python tools/gap_analysis.py $T 8 > $O/timeline.txt 2>&1
python tools/bench_grid.py 2>&1 | grep "^{" > $O/workload_sgl_grid_p1000_L20.json
python tools/bench_mgl_grid.py 2>&1 | grep "^{" > $O/workload_mgl_grid_8x1_K4_p500.json
python tools/bench_mgl_grid.py --reg FGL --K 6 --p 300 --l1 4 --l2 3 2>&1 | grep "^{" > $O/workload_mgl_grid_4x3_fgl_K6_p300.json
K=32 TOL=1e-10 python tools/parity_headline.py ns_tol=2e-12,0 > $O/parity_headline.txt 2>&1
keep $O/tile_variants.txt python tools/bench_tile_variants.py
keep $O/small_batches_product_kernel.txt python tools/bench_small_batches.py
# (round 4: everything a doc cites comes out of this script -- VERDICT r3 weak #10)
keep $O/jacobi_kernel_measured.txt python tools/bench_jacobi.py
bash tools/small_p_artifacts.sh $TAG > $O/small_p_artifacts.log 2>&1
keep $O/i8_product_kernel.txt python tools/bench_i8.py 500 4 16 32
keep $O/i8_omega_step_chain.txt python tools/bench_omega_i8.py 500 4 16 32
keep $O/stress_solve.txt python tools/stress_solve.py
REG=FGL LATENT=1 K=50 SEED=1237 TOL=1e-9 python tools/parity_headline.py >> $O/parity_headline.txt 2>&1
P=$(dirname $O)/prof_$TAG
( cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $P/c4 -o bench -- python3 $R/bench.py --full --workload fgl_K50_p500_latent --steps 20 --warmup 5 --regions 2 --no-cpu-baseline > $O/c4_prof.log 2>&1 )
python - <<PY > $O/c4_kernel_stats.txt 2>&1
import csv, glob
f = glob.glob("$R/gpurun_out/prof_$TAG/c4/**/*kernel_stats.csv", recursive=True)
for r in list(csv.DictReader(open(f[0])))[:14]:
    print(f'{r["Name"][:90]:90s} calls {r["Calls"]:>6s} avg {float(r["AverageNs"]) / 1e3:9.1f} us  {r["Percentage"]:>6s} %')
PY
head -c 700 $O/bench_final.json
rm -rf $R/gpurun_out/prof_$TAG/*/*.db 2>/dev/null
find $R/gpurun_out/prof_$TAG -name "*kernel_trace.csv" -size +20M -delete
# (round 5) the batch drivers' loop in C, the K-sharded slabs incl. K = 16, the fused-W A/B, timelines by kernel
{
  for a in "--p 50 --points 20" "--p 64 --points 100"; do python tools/bench_grid.py $a --no-sequential 2>&1 | grep "^{"; done
  python tools/time_batch.py --p 1000 --points 20 2>&1 | grep -v amdgpu.ids
  python tools/time_batch.py --p 64 --points 100 2>&1 | grep -v amdgpu.ids
  python tools/time_batch.py --p 50 --points 20 2>&1 | grep -v amdgpu.ids
} > $O/grids.txt 2>&1
GGL_BENCH_FORCE_DIST=1 python bench.py --full --workload ggl_K16_p500 --steps 30 --warmup 8 --regions 5 --no-cpu-baseline --comm capi 2>&1 | grep "^{" > $O/workload_ggl_K16_p500_sharded_1rank_rccl_capi.json
{
  echo "bench.py --full [--workload w] --opt fused_w=1|0 (GGL_OPT_FUSED_W), interleaved in one box: it/s"
  for rep in 1 2; do for w in ggl_K32_p500 ggl_K8_p500 ggl_K4_p500 ggl_K20_p200; do for fw in 1 0; do
    python bench.py --full --workload $w --steps 30 --warmup 8 --regions 5 --no-cpu-baseline --no-exact-region --opt fused_w=$fw 2>/dev/null | grep "^{" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$w fused_w=$fw', round(d['value'],1), 'it/s', round(d['ms_per_step'],4), 'ms', (d.get('newton_schulz') or {}).get('pipeline_totals'))"
  done; done; done
} > $O/fused_w_ab.txt 2>&1
keep $O/fuzz_sgl_batch.txt python tools/fuzz_sgl_batch.py 60 1
bash tools/r5_s.sh > $O/lds_pinned_ab.txt 2>&1
bash tools/trace_iteration.sh ggl_K4_p500 > $O/timeline_K4.txt 2>&1
bash tools/trace_iteration.sh ggl_K32_p500 > $O/timeline_headline_by_kernel.txt 2>&1
rm -rf $R/gpurun_out/trace_*/*.db $R/gpurun_out/trace_*/*/*.db 2>/dev/null
[ -z "$FAILED" ] || { echo "round_artifacts: sub-tools failed:$FAILED"; exit 1; }
