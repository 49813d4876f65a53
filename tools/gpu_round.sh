# round refresh on one MI355X: every GPU test, the full bench line, then tools/profile_round.sh's passes
# usage: bash tools/gpu_round.sh [output directory, default round_out]
export TMPDIR=/tmp
O=${1:-round_out}
mkdir -p "$O"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread > "$O/gpu_tests.log" 2>&1
rc=$?; tail -2 "$O/gpu_tests.log"; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$O/bench.json" 2> "$O/bench.err" || exit 1
tail -c 600 "$O/bench.json"
bash tools/profile_round.sh "$O/prof" || exit 1
cat "$O/prof/pmc_traffic.txt" "$O/prof/clock.txt"
# the reverse sweep (Q(x) at B=128, 100 steps) under rocprofv3: the team kernel's share of a sweep
timeout -s KILL 240 rocprofv3 --kernel-trace --stats -d "$O/prof/sweep" -o run --output-format csv -- \
  python3 tools/sweep_profile.py 128 > "$O/prof/sweep_profile.log" 2>&1 || exit 1
tail -4 "$O/prof/sweep_profile.log"
