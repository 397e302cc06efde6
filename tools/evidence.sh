#!/bin/bash
# End-of-round evidence on one box (TAG names the round, e.g. r05).  PART=a: the GPU suite, smoke, the
# default bench line and a rocprofv3 --kernel-trace --stats of that same bench command (+ the fused lookup's
# in-forward vs back-to-back means, tools/roofline_rocprof.py) and a config-2 forward trace.  PART=b: the
# in-forward PMC passes (tools/pmc_forward.sh -> $OUT_DIR/<TAG>_*_pmc.json) and the configs 3-5 lines.
# Each GPU step time-limited; the chain stops at the first failure.
set -o pipefail
cd "$(dirname "$0")/.."
export OUT_DIR=${OUT_DIR:-bench_out}
mkdir -p $OUT_DIR
export TMPDIR=/tmp
TAG=${1:-r05}
if [ "${PART:-a}" = a ]; then
  timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT_DIR/t_${TAG}_ev.log 2>&1
  rc=$?; tail -3 $OUT_DIR/t_${TAG}_ev.log; [ $rc -eq 0 ] || exit $rc
  timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" || exit 1
  timeout -k 10 300 python bench.py --full > $OUT_DIR/bench_${TAG}.json 2> $OUT_DIR/bench_${TAG}.err || { tail -20 $OUT_DIR/bench_${TAG}.err; exit 1; }
  cat $OUT_DIR/bench_${TAG}.json
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT_DIR/prof_${TAG} -o run --output-format csv -- python bench.py --full --no-cpu-baseline > $OUT_DIR/bench_${TAG}_rocprof.json 2> $OUT_DIR/bench_${TAG}_rocprof.err || { tail -20 $OUT_DIR/bench_${TAG}_rocprof.err; exit 1; }
  python tools/roofline_rocprof.py $OUT_DIR/prof_${TAG}/run_kernel_trace.csv $OUT_DIR/bench_${TAG}_rocprof.json > $OUT_DIR/${TAG}_roofline_rocprof.json
  cat $OUT_DIR/${TAG}_roofline_rocprof.json
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT_DIR/fwd_${TAG} -o run --output-format csv -- python tools/fwd_profile.py 1 440 1024 f16x3 > $OUT_DIR/fwd_${TAG}.log 2>&1 || { tail -20 $OUT_DIR/fwd_${TAG}.log; exit 1; }
  python tools/phase_summary.py $OUT_DIR/fwd_${TAG}/run_kernel_trace.csv > $OUT_DIR/${TAG}_forward_phases_config2.txt 2>&1
  grep -E "forward span|encoder phase span|loop span" $OUT_DIR/${TAG}_forward_phases_config2.txt
else
  # the lookup-only forward (RAFT_FUSE_CONVF1=0, pmc_forward.py's default): <TAG>_lookup_pmc.json
  PMC_OUT=$OUT_DIR PMC_ROUND=$TAG timeout -k 10 600 bash tools/pmc_forward.sh 1 > $OUT_DIR/pmc_${TAG}.log 2>&1 || { tail -20 $OUT_DIR/pmc_${TAG}.log; exit 1; }
  mkdir -p $OUT_DIR/pmc_unfused && cp $OUT_DIR/${TAG}_halo_pmc.json $OUT_DIR/pmc_unfused/
  # the bench's forward (the fused lookup launch): <TAG>_lookup_conv_pmc.json and its conv counters
  RAFT_FUSE_CONVF1=1 PMC_OUT=$OUT_DIR PMC_ROUND=$TAG timeout -k 10 600 bash tools/pmc_forward.sh 1 > $OUT_DIR/pmc2_${TAG}.log 2>&1 || { tail -20 $OUT_DIR/pmc2_${TAG}.log; exit 1; }
  tail -5 $OUT_DIR/pmc2_${TAG}.log
  [ -n "$PMC_ONLY" ] && exit 0
  timeout -k 10 900 bash tools/config_sweep.sh $TAG || exit 1
fi
