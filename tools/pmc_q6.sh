set -e
# Writes under $OUT_DIR/pmcq6 (default bench_out/pmcq6).
out=${OUT_DIR:-bench_out}/pmcq6
mkdir -p $out
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $out/f -o run -- python3 bench.py --full --no-q1 --no-dist-legs --no-cpu --steps 3 --warmup 1 > $out/f.log 2>&1
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $out/w -o run -- python3 bench.py --full --no-q1 --no-dist-legs --no-cpu --steps 3 --warmup 1 > $out/w.log 2>&1
