"""Normals of the point path, measurement: prints one JSON line and writes it to
profiles/points_normals_bench.json.

md_op_unproject / md_op_unproject_normals alone on device tensors, on the seeded noise scene of tools/points_bench.py (depth =
exp(N(0.5, 0.6)) in [0.5, 6], conf = 1 + 2 U(0,1) >= 1.8: about 0.58 of the pixels are kept), at 8x1536x1536 and 1x518x518: the
dense map and the list, each without normals, with normals, and with normals and the grazing-angle test (min_cos = 0.05).
Microseconds per call (the operator allocates and frees its scratch: the kernels' own times are in a kernel trace of this tool),
the extra time of the normals, and the fraction of the achievable HBM rate against the algorithmic bytes.

  python tools/points_normals_bench.py [--steps 20] [--warmup 3] [--shape 8x1536] [--out profiles/points_normals_bench.json]

The kernel table of DESIGN 12.2 is the raw statistics of one trace-only run per shape, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/points_normals_bench.py --shape 8x1536 --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/points_normals_kernel_stats_8x1536.csv (and --shape 1x518 likewise)"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes / s
MIN_COS = 0.05


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps  # ms


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=["8x1536", "1x518"], default="", help="measure this shape only (a kernel trace per shape)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_normals_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {}
    kw = dict(depth_min=0.5, depth_max=6.0, conf_min=1.8)
    for B, S in ((8, 1536), (1, 518)):
        if a.shape and a.shape != f"{B}x{S}":
            continue
        rng = np.random.default_rng(7)
        d = torch.from_numpy(np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)).cuda()
        c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
        f = torch.full((B,), 0.9 * S, device="cuda")
        npx = B * S * S
        row = {}
        for name, nk in (("plain", {}), ("normals", dict(normals=True)), ("normals_min_cos", dict(normals=True, normal_min_cos=MIN_COS))):
            dense = ops.unproject(dev, d, focal_px=f, conf=c, compact=False, **kw, **nk)
            lst = ops.unproject(dev, d, focal_px=f, conf=c, dense=False, **kw, **nk)
            share = float(lst.count[-1].item()) / npx
            ms_dense = _time(lambda: ops.unproject(dev, d, focal_px=f, conf=c, compact=False, out=dense, **kw, **nk), a.steps, a.warmup)
            ms_list = _time(lambda: ops.unproject(dev, d, focal_px=f, conf=c, dense=False, out=lst, **kw, **nk), a.steps, a.warmup)
            extra = 12 if nk else 0  # the normal beside the point
            bytes_dense = npx * (4 + 4 + 12 + 1 + extra)
            bytes_list = npx * (2 * (4 + 4) + 1 / 8 + (12 + extra) * share)
            row[name] = {"kept_share": round(share, 4), "dense_us": round(ms_dense * 1e3, 1),
                         "dense_hbm_fraction": round(bytes_dense / (ms_dense * 1e-3) / HBM_ACHIEVABLE, 3),
                         "list_us": round(ms_list * 1e3, 1), "list_hbm_fraction": round(bytes_list / (ms_list * 1e-3) / HBM_ACHIEVABLE, 3)}
            del dense, lst
        for name in ("normals", "normals_min_cos"):
            row[name]["dense_extra_us"] = round(row[name]["dense_us"] - row["plain"]["dense_us"], 1)
            row[name]["list_extra_us"] = round(row[name]["list_us"] - row["plain"]["list_us"], 1)
        res[f"{B}x{S}x{S}"] = row
        del d, c
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
