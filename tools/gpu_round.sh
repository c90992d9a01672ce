# Full GPU check used between milestones: parity tests, bench, rocprof stats.
# Writes under $OUT_DIR/round (default bench_out/round).
set -e
out=${OUT_DIR:-bench_out}/round
mkdir -p $out
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $out/gpu_tests.log 2>&1
timeout -k 10 300 python bench.py --full > $out/bench.log 2>&1
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o run -- python3 bench.py --full --steps 5 --no-cpu > $out/prof.log 2>&1
timeout -k 10 300 python tools/opbench.py > $out/opbench.json 2> $out/opbench.err
