#!/bin/bash
# Run ON the GPU box AFTER the last change to the library: the whole GPU suite (three GEMM modes), the PMC
# traffic of the dominant kernel (carries f2g_version()), the full bench line.  -> OUTDIR (first argument)
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$(realpath -m "${1:?usage: bash tools/final_round.sh OUTDIR}")
cd $R
mkdir -p $O
( time python -m pytest tests -x -q -m gpu --durations=15 ) > $O/gputest_final.txt 2>&1
tail -4 $O/gputest_final.txt
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
bash tools/pmc_traffic.sh > $O/pmc_traffic.log 2>&1
cp gpurun_out/r04_pmc_gemm_traffic.json gpurun_out/r04_pmc_x6_traffic.json profiles/   # (bench.py reads profiles/)
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err
python bench.py --full --gemm bf16x6 --no-fast-mode > $O/bench_x6_candidate.json 2>/dev/null
tail -c 400 $O/bench_default.json
