# bench lines (paste-only and multi-band; $RIG chain|cylinder, $BLENDS) for the main library and
# variants/<name>.so given as arguments, alternating twice (timing only); logs under $MCS_OUT_DIR
# (default bench_out/)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
R="$GRAFT_REPO_ROOT"
O="${MCS_OUT_DIR:-$R/bench_out}"
mkdir -p "$O"
for i in 1 2; do
  for v in "$@"; do
    if [ "$v" = main ]; then unset MCS_LIBRARY; else export MCS_LIBRARY="$R/variants/$v.so"; fi
    for b in ${BLENDS:-none multiband}; do
      timeout -k 10 200 python bench.py --full --rig ${RIG:-chain} --blend $b --no-cpu-baseline --no-paste-ref --no-also > "$O/var_$v.log" 2>&1 || { tail -20 "$O/var_$v.log"; exit 1; }
      tail -1 "$O/var_$v.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$v $b', d['value'], 'launch', d['kernels']['launch_ms'], 'diff', d['max_abs_diff'])"
    done
  done
done
