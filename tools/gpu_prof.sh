# rocprofv3 kernel trace + stats of one bench run (no counters).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
R="$GRAFT_REPO_ROOT"
O="${MCS_PROF_DIR:-$R/bench_out}"
mkdir -p "$O"
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o run -- python3 "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline "$@" > "$O/prof.log" 2>&1
