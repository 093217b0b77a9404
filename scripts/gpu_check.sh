# parity suite + smoke + default bench line (one box call); stops at the first failure
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
BENCH_OUT=${BENCH_OUT:-bench_out}  # where the bench lines go
mkdir -p "$BENCH_OUT"
mkdir -p gpurun_out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > gpurun_out/gpu_tests.log 2>&1 && \
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/smoke.log 2>&1 && \
timeout -k 10 600 python -u bench.py --full ${BENCH_ARGS:-} > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err"
echo "exit $?"
