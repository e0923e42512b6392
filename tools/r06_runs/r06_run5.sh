set -o pipefail
export PYTHONUNBUFFERED=1
export O=${O:-evidence}  # output folder of this script
mkdir -p "$O"
cp burn_depth_amd/libmi_depth.so /tmp/good.so
for v in good nostats nocopy good nostats nocopy; do
  if [ $v = good ]; then cp /tmp/good.so burn_depth_amd/libmi_depth.so; else cp burn_depth_amd/libmi_$v.so burn_depth_amd/libmi_depth.so; fi
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > $O/r06_v_$v.json 2> $O/r06_v_$v.err || exit 1
  python - $v <<'PY'
import json, os, sys
m=sys.argv[1]
d=json.loads(open(f"{os.environ['O']}/r06_v_{m}.json").read().strip().splitlines()[-1]); k=d["kernels"]
print(m, d["value"], d["ms_per_step"], {n: k[n]["ms_per_step"] for n in ("qkv_gemm","proj_gemm","fc1_gemm","fc2_gemm") if n in k}, flush=True)
PY
done
cp /tmp/good.so burn_depth_amd/libmi_depth.so
