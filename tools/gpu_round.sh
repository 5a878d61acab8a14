# Round-end measurement on the GPU box (run from the repo root via gpurun):
#   GPU tests, the bench line (with CPU baseline), the rocprofv3 kernel-trace
#   summary of the same bench command, per-kernel micro-benchmarks and the PMC
#   passes for HBM traffic.  SKIP_TESTS=1 skips the pytest step.
# Every GPU step has its own time limit; the script stops at the first failure.
set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p gpurun_out
if [ -z "${SKIP_TESTS:-}" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 300 --timeout-method thread > gpurun_out/pytest_gpu.log 2>&1
  tail -2 gpurun_out/pytest_gpu.log
fi
# the bench line with every side measurement (bench.py --full), into $BENCH_OUT
BENCH_OUT=${BENCH_OUT:-bench_out}
mkdir -p $BENCH_OUT
timeout -k 10 600 python bench.py --full > $BENCH_OUT/bench.json 2> $BENCH_OUT/bench.err
tail -c 300 $BENCH_OUT/bench.json
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $BENCH_OUT/prof -o bench -- python3 bench.py --full > $BENCH_OUT/bench_prof.json 2> $BENCH_OUT/bench_prof.err
timeout -k 10 300 python tools/bench_kernels.py > gpurun_out/bench_kernels.json 2> gpurun_out/bench_kernels.err
ONLY=${ONLY:-} bash tools/pmc_pass.sh
python tools/pmc_summary.py gpurun_out gpurun_out/pmc_traffic.json > /dev/null
echo round-ok
