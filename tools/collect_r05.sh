#!/bin/bash
# Run ON the GPU box (through gpurun): the measurements profiles/r05_* are made from.  Outputs go to gpurun_out/;
# python tools/make_profiles_r05.py turns them into the committed summaries.  bench.py's default GEMM arithmetic
# is bf16x6 (fp32 class) since round 5; every exact-fp32 run says --gemm fp32.
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out/r05
rm -rf $O; mkdir -p $O
cd $R
python tools/hbm_kernel_bench.py $O/hbm_class_isolated.json > $O/hbm_kernels.txt 2>/dev/null
cp $O/hbm_class_isolated.json profiles/hbm_class_isolated.json      # (so that the default line below carries it)
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
F2G_GEMM_REPORT=90 python bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-fast-mode 2> $O/shapes_x6.txt > /dev/null
F2G_GEMM_REPORT=90 python bench.py --full --gemm fp32 --steps 3 --warmup 2 --no-cpu-baseline --no-fast-mode 2> $O/shapes_fp32.txt > /dev/null
for w in stage1 infer4; do
  python bench.py --full --workload $w --steps 10 --warmup 3 --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_$w.json
done
python bench.py --full --model mel_44k_128band_512x_base --steps 6 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_44k.json
python bench.py --full --n-timesteps 4 --steps 4 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_n4.json
python bench.py --optimizer --steps 8 --warmup 3 --no-cpu-baseline --no-roofline --no-fast-mode 2>/dev/null | tail -1 > $O/bench_opt.json
python bench.py --full --workload infer4 --steps 10 --warmup 3 --no-cpu-baseline --no-fast-mode --gemm bf16 2>/dev/null | tail -1 > $O/bench_infer4_bf16.json
( for m in bf16x6 fp32; do for k in "" mrd mpd mel "mpd,mrd" "mpd,mrd,mel"; do MODE=$m KO=$k python tools/knockout.py 2>&1 | tail -1; done; done ) > $O/knockout.txt
( for m in fp32 bf16x6; do echo "## MODE=$m"; MODE=$m python tools/conv32_probe.py 2>&1 | grep -v amdgpu.ids; done ) > $O/conv32_probe.txt
cd /tmp && export TMPDIR=/tmp
B="python3 $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --no-fast-mode"
F2G_STREAMS=0 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_serial -o p -- $B > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_lanes -o p -- $B > /dev/null 2>&1
F2G_STREAMS=0 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_fp32 -o p -- $B --gemm fp32 > /dev/null 2>&1
for d in prof_serial prof_lanes prof_fp32; do find $O/$d -type f ! -name "p_kernel_stats.csv" -delete; done
B1="python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-roofline --no-fast-mode"
for set in FETCH_SIZE WRITE_SIZE; do
  F2G_STREAMS=0 timeout 400 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/pmcb_x6_$set -o p -- $B1 > /dev/null 2>&1
  F2G_STREAMS=0 timeout 400 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/pmcb_$set -o p -- $B1 --gemm fp32 > /dev/null 2>&1
done
for d in pmcb_FETCH_SIZE pmcb_WRITE_SIZE pmcb_x6_FETCH_SIZE pmcb_x6_WRITE_SIZE; do find $O/$d -type f ! -name "p_counter_collection.csv" -delete; done
cd $R
G=gpurun_out/r05 MODE=bf16x6 python3 tools/pmc_traffic_json.py $O/pmc_x6_traffic.json
G=gpurun_out/r05 MODE=fp32 python3 tools/pmc_traffic_json.py $O/pmc_gemm_traffic.json
bash tools/pmc_busy.sh r05_x6 > /dev/null 2>&1; cp gpurun_out/pmc_busy_r05_x6.txt $O/pmc_busy_x6.txt
bash tools/pmc_busy.sh r05_fp32 --gemm fp32 > /dev/null 2>&1; cp gpurun_out/pmc_busy_r05_fp32.txt $O/pmc_busy_fp32.txt
tail -1 $O/bench_default.json | cut -c1-200
