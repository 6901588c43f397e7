# Round-4 closing run on an MI355X: the whole -m gpu suite, smoke(), the default bench line with everything --full adds.
O=${1:?usage: bash tools/r4_final.sh OUTDIR}
mkdir -p "$O" && export PYTHONUNBUFFERED=1
timeout -k 10 1100 python -m pytest tests -q -m gpu --durations=8 > "$O"/gpu_tests_final.log 2>&1; tail -14 "$O"/gpu_tests_final.log | cut -c1-220
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O"/smoke_final.log 2>&1; tail -2 "$O"/smoke_final.log
timeout -k 10 900 python bench.py --full > "$O"/bench_final.json 2> "$O"/bench_final.err; python tools/show_bench.py "$O"/bench_final.json | head -4
