#!/bin/bash
# usage: FNN_OUT=<folder> bash tools/final_capture.sh   - what a round's final capture runs on ONE machine with an MI355X (about 30 GPU-minutes):
# the GPU suite, tools/capture_all.sh for every workload (bench line, kernel trace, per-layer table, clocks, MFMA and traffic counters), the five-fold,
# sharded-on-one-rank and driver-shaped bench lines (with --full), and the kernel coverage of the suite under rocprofv3.  Output: $FNN_OUT/final/ and
# $FNN_OUT/cap_*/ (FNN_OUT relative to the repository root; tools/install_capture.sh copies them into profiles/).
cd $GRAFT_REPO_ROOT
export FNN_KNOBS=1
R=${FNN_ROUND:-r06}
out=$(mkdir -p "${FNN_OUT:?FNN_OUT: the folder that receives the captures}" && cd "$FNN_OUT" && pwd); export FNN_OUT=$out
mkdir -p $out/final; rm -f $out/final/*; rm -rf $out/cap_*
timeout 2400 python -m pytest tests -m gpu -q -rP > $out/final/pytest_gpu.log 2>&1; grep -E "passed|failed" $out/final/pytest_gpu.log | tail -2
FNN_ROUND=$R bash tools/capture_all.sh > $out/final/capture_all_$R.log 2>&1
for t in bone iso128_r2 iso128_teacher resenc160_r2 resenc160_r2_f8 bone_autocast bone_mirror; do cp $out/cap_$t/traffic.txt $out/final/${R}_${t}_traffic_by_kernel.txt 2>/dev/null; done
timeout 600 python bench.py --full --workload iso128_teacher --folds 5 --steps 3 --warmup 1 2> /dev/null | grep "^{" > $out/final/${R}_iso128_teacher_folds5_bench.json
timeout 600 python bench.py --full --gpus 1 --force-sharded --steps 5 --warmup 2 --no-cpu-baseline 2> /dev/null | grep "^{" > $out/final/${R}_bone_sharded1_bench.json
timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 5 2> /dev/null | grep "^{" > $out/final/${R}_bone_driver_shaped_bench.json
timeout 1500 python tools/plan_sweep.py --out $out/final/${R}_plan_sweep > $out/final/${R}_plan_sweep.log 2>&1
root=$GRAFT_REPO_ROOT
(cd /tmp && export TMPDIR=/tmp && rm -rf $out/suite_trace && timeout 1800 rocprofv3 --kernel-trace --stats --output-format csv -d $out/suite_trace -- python3 -m pytest $root/tests -q -m gpu > $out/final/suite_trace.log 2>&1)
python tools/kernel_coverage.py $out/suite_trace > $out/final/${R}_kernel_coverage.txt 2>&1
rm -rf $out/suite_trace
tail -3 $out/final/capture_all_$R.log; tail -3 $out/final/${R}_kernel_coverage.txt
cut -c1-400 $out/final/${R}_bone_driver_shaped_bench.json
