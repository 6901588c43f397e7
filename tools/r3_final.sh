set -x
O=${1:?usage: bash tools/r3_final.sh OUTDIR}
mkdir -p "$O"
export PYTHONUNBUFFERED=1
timeout -k 10 1100 python -m pytest tests -q -m gpu -x > "$O"/gpu_tests_final.log 2>&1 ; tail -3 "$O"/gpu_tests_final.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O"/smoke_final.log 2>&1 ; tail -2 "$O"/smoke_final.log
timeout -k 10 600 python bench.py --full > "$O"/bench_default_final.json 2> "$O"/bench_default_final.err
python3 - "$O" <<'PY'
import json, sys
l=json.loads(open(sys.argv[1] + '/bench_default_final.json').read().strip().splitlines()[-1])
print(l['ms_per_step'], l['value'], l['roofline']['frac'], l['roofline'].get('traffic'))
print({k:(v['ms_per_step']) for k,v in l['extra'].items()}, l['extra']['configs3_highres'].get('bf16_thin_channel',{}).get('ms_per_step'), l['cpu_baseline']['value'])
PY
