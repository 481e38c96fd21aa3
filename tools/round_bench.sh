#!/bin/bash
# Round-closing numbers (run on a machine with the GPU): full GPU suite, smoke, the official bench line (config 2
# with --full: CPU baseline, kernel table, layer rooflines), config 4, graph-mode step, configs 3/5/f1, rocprofv3
# kernel summary of the default (single-stream) step.  Output in $OUT (default bench_out/); copy what is judged into
# profiles/.   bash tools/round_bench.sh r03
export TMPDIR=/tmp
TAG=${1:-r04}
OUT=${OUT:-bench_out}
mkdir -p $OUT
STGCN_TEST_REPORT=1 timeout -k 10 900 python -u -m pytest tests -m gpu -x -v -s --timeout 300 --timeout-method thread -p no:cacheprovider > $OUT/gpu_tests_$TAG.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/gpu_tests_$TAG.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1 || exit $?
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || exit $?
echo "bench: $(cut -c1-200 $OUT/bench_$TAG.json)"
timeout -k 10 300 python bench.py --full --config 4 --steps 120 --no-cpu-baseline > $OUT/bench_c4_$TAG.json 2> $OUT/bench_c4_$TAG.err || exit $?
timeout -k 10 300 python bench.py --full --graph --steps 120 --no-cpu-baseline --no-layer-roofline > $OUT/bench_graph_$TAG.json 2> $OUT/bench_graph_$TAG.err || exit $?
timeout -k 10 600 python tools/bench_configs.py > $OUT/configs_$TAG.json 2> $OUT/configs_$TAG.err || exit $?
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o bench --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-layer-roofline --kernel-steps 0 > $OUT/prof_$TAG.log 2>&1
echo "prof rc=$?"
