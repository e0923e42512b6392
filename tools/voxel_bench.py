"""Voxel thinning measurement: prints one JSON line and writes it to profiles/voxel_bench.json.

md_op_voxel_thin alone on device lists: the kept list (xyz, conf) of tools/points_bench.py's seeded noise scene at
8x1536x1536 (world = 1 with eight cameras on a circle, so the views overlap), and the cloud of DA3 `small` (seeded
weights) at 3x518x518 through `infer_points`. Per list two voxel sizes, found by bisection on the device, that leave about
1/2 and about 1/8 of the points. Microseconds per call (the operator allocates and frees its table: the kernels' own times
are in a kernel trace of this tool), the algorithmic bytes (rows read twice, the slot word written and read, 20 B per table
slot reset and 20 B per row touched, surviving rows written) against the achievable HBM rate, and the host route the call
replaces: device -> host copy of the list plus pipeline.voxel_thin.

  python tools/voxel_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--out profiles/voxel_bench.json]

The kernel table of DESIGN 12.3 is the raw statistics of one trace-only run, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/voxel_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/voxel_kernel_stats_8x1536.csv"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes / s


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


def _noise_scene(dev, B=8, S=1536):
    """the kept list of points_bench's scene, unprojected into one world frame"""
    from burn_depth_amd import ops
    rng = np.random.default_rng(7)
    d = torch.from_numpy(np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)).cuda()
    c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
    f = torch.full((B,), 0.9 * S, device="cuda")
    E = np.zeros((B, 3, 4), np.float32)
    for b in range(B):  # cameras turned by 5 degrees each about Y, half a unit apart
        a = np.radians(5.0 * b)
        E[b, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[b, :, 3] = [0.5 * b, 0, 0]
    pc = ops.unproject(dev, d, focal_px=f, extrinsics=torch.from_numpy(E).cuda(), conf=c, dense=False, world=True, depth_min=0.5, depth_max=6.0,
                       conf_min=1.8)
    xyz, _, conf = pc.points()
    return xyz.clone(), conf.clone()


def _da3_scene(dev, V=3, S=518):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, V
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(V, 3, S, S, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        pc = m.infer_points(x, dense=False, world=True)
        xyz, _, conf = pc.points()
        return xyz.clone(), conf.clone()
    finally:
        m.destroy()


def _voxel_for(dev, xyz, conf, share):
    """bisection on the device: the voxel size that leaves about `share` of the rows"""
    from burn_depth_amd import ops
    fin = xyz[torch.isfinite(xyz).all(1)]
    span = float((fin.max(0).values - fin.min(0).values).max())
    lo, hi = span * 2.0 ** -19, span
    out = ops.voxel_thin(dev, xyz, hi, conf=conf)
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        ops.voxel_thin(dev, xyz, mid, conf=conf, out=out)
        if out.count[-1].item() > share * xyz.shape[0]:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only (a kernel trace per list)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {}
    for name, make in (("8x1536", _noise_scene), ("da3_3x518", _da3_scene)):
        if a.case and a.case != name:
            continue
        xyz, conf = make(dev)
        n = int(xyz.shape[0])
        slots = 1024
        while slots < 2 * n:
            slots *= 2
        row = {"rows": n, "table_slots": slots}
        for label, share in (("half", 0.5), ("eighth", 0.125)):
            voxel = _voxel_for(dev, xyz, conf, share)
            out = ops.voxel_thin(dev, xyz, voxel, conf=conf)
            m = int(out.count[-1].item())
            ms = _time(lambda: ops.voxel_thin(dev, xyz, voxel, conf=conf, out=out), a.steps, a.warmup)
            # insert reads xyz + conf and writes the slot; select reads the slot and the rank word; scatter reads the kept rows, their
            # slot and count word and writes xyz, conf, index, weight; the table is reset (20 B per slot) and touched (20 B per row)
            nbytes = n * (16 + 4) + n * (4 + 8) + m * (16 + 4 + 4 + 16 + 8) + 20 * slots + 20 * n
            r = {"voxel": voxel, "survivors": m, "share": round(m / n, 4), "dropped": int(out.dropped.item()), "call_us": round(ms * 1e3, 1),
                 "algorithmic_bytes": int(nbytes), "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3)}
            if not a.no_host:
                t0 = time.perf_counter()
                hx, hc = xyz.cpu().numpy(), conf.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.voxel_thin(hx, voxel, hc)
                t2 = time.perf_counter()
                assert int(ref.count[-1]) == m and np.array_equal(ref.index, out.index[:m].cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[label] = r
            del out
        res[name] = row
        del xyz, conf
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
