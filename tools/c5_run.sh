# BASELINE config 5 on one GPU on the current tree: the c5 bench line, with every side
# measurement (bench.py --full), into $BENCH_OUT.
BENCH_OUT=${BENCH_OUT:-bench_out}
cd "$(dirname "$0")/.." && mkdir -p $BENCH_OUT
timeout -k 10 600 python bench.py --full --config c5 --steps 10 --warmup 2 > $BENCH_OUT/c5_bench.json 2> $BENCH_OUT/c5_bench.err; rc=$?; tail -c 600 $BENCH_OUT/c5_bench.json; exit $rc
