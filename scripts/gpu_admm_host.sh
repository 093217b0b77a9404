# ADMM host-side bookkeeping change: ADMM GPU parity, coordinated legs, full default bench line
set -o pipefail
mkdir -p gpurun_out
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
BENCH_OUT=${BENCH_OUT:-bench_out}  # where the bench lines go
mkdir -p "$BENCH_OUT"
timeout -k 10 400 python -u -m pytest tests/test_gpu_admm.py -m gpu -x -q --timeout 200 --timeout-method thread > gpurun_out/gpu_admm.log 2>&1 && \
timeout -k 10 300 python -u bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-e2e --admm-agents 0 --nn-zones 0 --mhe-agents 0 > "$BENCH_OUT/legs.json" 2> "$BENCH_OUT/legs.err" && \
timeout -k 10 500 python -u bench.py --full > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err"
echo "admm_host exit $?"
