# full GPU suite + smoke + the bench line with every leg (--full) (the driver's round-end sequence): bash tools/gpu_verify_round.sh [tag, default r06]
T=${1:-r06}
OUT=${OUT:-out}   # where the logs and the bench line go
mkdir -p $OUT
timeout 1800 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/${T}_pytest_gpu_full.log 2>&1; echo "pytest exit $?" | tee -a $OUT/${T}_pytest_gpu_full.log
grep -a "passed\|failed" $OUT/${T}_pytest_gpu_full.log | tail -3
timeout 300 python __graft_entry__.py smoke 2>&1 | tail -1
timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${T}_bench_driver_style.json 2> $OUT/${T}_bench_driver_style.err; echo "bench exit $?"
python - <<PY
import json
d = json.loads(open('$OUT/${T}_bench_driver_style.json').read().strip().splitlines()[-1])
print({k: d.get(k) for k in ('value', 'ms_per_step', 'sustained_images_per_sec', 'legs_ms', 'synthetic_nms_tensor')}); print('roofline frac', d['roofline']['frac'], d['roofline'].get('mfma_busy_frac_pmc'), d['roofline']['traffic_source'])
print('train', {k: d['train'].get(k) for k in ('value', 'ms_per_step')}, d['train'].get('roofline', {}).get('kernel_groups'))
PY
