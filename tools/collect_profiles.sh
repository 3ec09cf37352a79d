#!/bin/bash
# usage (on the GPU box, from the repo root): tools/collect_profiles.sh <tag> [extra bench.py args]
# -> tools_out/profiles_<tag>/ (TOOLS_OUT overrides the folder): <tag>_bench_kernel_stats.csv, <tag>_bench_by_level.md,
#    <tag>_pmc_traffic.{md,json}; copy them into profiles/ afterwards.
# PMC passes are separate runs with --kernel-trace only (gpurun refuses --pmc with the
# sys/hip/hsa trace domains).  Every GPU step runs under a time limit of its own (STEP_LIMIT seconds).
set -o pipefail
tag=$1; shift
root=${GRAFT_REPO_ROOT:-$(pwd)}
res=$(realpath -m "${TOOLS_OUT:-$root/tools_out}"); mkdir -p $res
out=$res/profiles_$tag
mkdir -p $out
cd /tmp && export TMPDIR=/tmp
lim="timeout -k 10 ${STEP_LIMIT:-600}"
$lim rocprofv3 --kernel-trace --stats --output-format csv -d $res/prof_$tag -o d -- python3 $root/bench.py --steps 20 --warmup 3 --full --no-cpu --no-csr-ref "$@" > $out/${tag}_bench_line.json 2> $out/${tag}_kernel_trace.log || exit 1
$lim rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $res/pmc_f_$tag -o d -- python3 $root/bench.py --steps 4 --warmup 1 --full --no-cpu --no-csr-ref "$@" > $out/pmc_f.log 2>&1 || exit 1
$lim rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $res/pmc_w_$tag -o d -- python3 $root/bench.py --steps 4 --warmup 1 --full --no-cpu --no-csr-ref "$@" > $out/pmc_w.log 2>&1 || exit 1
cd $root
cp $res/prof_$tag/d_kernel_stats.csv $out/${tag}_bench_kernel_stats.csv
python3 tools/rocprof_summary.py $res/prof_$tag/d_kernel_trace.csv > $out/${tag}_bench_by_level.md
note="default layout (dictionary-coded rows, K-Patch on levels 0-3)"
case " $* " in *" --layout sell "*) note="--layout sell (CSR sliced into 64-row panels, 16-bit relative columns)";; esac
PMC_OUT_DIR=$out python3 tools/pmc_traffic.py $res/pmc_f_$tag/d_counter_collection.csv $res/pmc_w_$tag/d_counter_collection.csv $tag "$note" > /dev/null
grep -v "^$" $out/${tag}_pmc_traffic.md | head -30
