cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
O=${1:?usage: bash tools/r4_gaps.sh OUTDIR}
mkdir -p "$O"
rm -rf "$O"/trace
rocprofv3 --kernel-trace -d "$O"/trace -o t --output-format csv -- python3 bench.py --steps 3 --warmup 2 --full --profile-steps 1 --no-cpu-baseline --no-extra > "$O"/trace_bench.json 2> "$O"/trace_bench.err || exit 2
f=$(find "$O"/trace -name 't_kernel_trace.csv' | head -1)
# steps in the trace: 2 warm-up + 3 timed + 1 + 1 profiled = 7; step index 3 = a timed (overlapped) step, 6 = the one-stream profiled step
python3 tools/gap_analysis.py "$f" 7 3 > "$O"/gaps_overlapped.txt 2>&1
python3 tools/gap_analysis.py "$f" 7 6 > "$O"/gaps_onestream.txt 2>&1
rm -rf "$O"/trace
cat "$O"/gaps_overlapped.txt; echo; cat "$O"/gaps_onestream.txt
