set -o pipefail
export PYTHONUNBUFFERED=1
export O=${O:-evidence}  # output folder of this script
mkdir -p "$O"
timeout -k 10 600 python tools/r06_persist_check.py > $O/r06_persist_check.log 2>&1
rc=$?
grep -v amdgpu.ids $O/r06_persist_check.log | tail -8
[ $rc -eq 0 ] || exit $rc
for m in fc1qkv on fc1qkv on; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras --persistent-fc1 $m > $O/r06_pf_$m.json 2> $O/r06_pf_$m.err || exit 1
  python - $m <<'PY'
import json, os, sys
m=sys.argv[1]
d=json.loads(open(f"{os.environ['O']}/r06_pf_{m}.json").read().strip().splitlines()[-1]); k=d["kernels"]
print(m, d["value"], d["ms_per_step"], {n: k[n]["ms_per_step"] for n in ("qkv_gemm","proj_gemm","fc1_gemm","fc2_gemm","dec_conv3x3") if n in k}, flush=True)
PY
done
