"""Depth-grid mesh measurement: prints one JSON line and writes it to profiles/mesh_bench.json.

tools/points_bench.py's seeded noise scene at 8x1536x1536 and 1x518x518, max_rtol 0 and 0.05:
  operator   md_op_unproject_mesh (list + pixel_index + faces) against md_op_unproject_normals with a NULL mesh (the list
             alone) on the same arguments, measured A, B, B, A: microseconds per call and their difference, the mesh stage;
             md_op_mesh_grid alone on the finished map (both operators allocate and free their scratch inside the call: the
             kernels' own times are in a kernel trace of this tool).
  bytes      the algorithmic bytes per kernel (index: 4 B per pixel written plus the ballot bits; classify: 4 + 4 B per lattice
             node read; scatter: the same plus 12 B per face) and the time they take at the achievable HBM rate.
  host       the route the call replaces: device -> host copy of the depth and the mask, pipeline.pixel_index and
             pipeline.mesh_grid (their result is compared with the device's).
`--model`: md_infer_points_mesh against md_infer_points_render without a mesh at DA3 `small` 3x518x518, eager and graph, A, B, B, A.

  python tools/mesh_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--no-host] [--model] [--out FILE]

The kernel table of DESIGN 12.5 is the raw statistics of one trace-only run, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mesh_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/mesh_kernel_stats_8x1536.csv"""
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
RTOLS = (0.0, 0.05)


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


def _abba(fa, fb, steps, warmup):
    """A, B, B, A -> (ms of A, ms of B), each the mean of its two runs"""
    a1, b1, b2, a2 = _time(fa, steps, warmup), _time(fb, steps, warmup), _time(fb, steps, warmup), _time(fa, steps, warmup)
    return (a1 + a2) / 2, (b1 + b2) / 2


def _scene(B, S):
    rng = np.random.default_rng(7)
    d = torch.from_numpy(np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)).cuda()
    c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
    return d, c, torch.full((B,), 0.9 * S, device="cuda")


def _model_rows(dev, steps, warmup):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, 3
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(3, 3, 518, 518, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        row = {}
        for mode in ("eager", "graph"):
            m.enable_graph(mode == "graph")
            for rtol in RTOLS:
                mesh = dict(max_rtol=rtol)
                plain = m.infer_points(x, dense=False, world=True)
                meshed = m.infer_points(x, dense=False, world=True, mesh=mesh)
                ms_p, ms_m = _abba(lambda: m.infer_points(x, dense=False, world=True, out=plain),
                                   lambda: m.infer_points(x, dense=False, world=True, out=meshed, mesh=mesh), steps, warmup)
                row[f"{mode}_rtol{rtol}"] = {"render_entry_ms": round(ms_p, 3), "mesh_entry_ms": round(ms_m, 3), "delta_us": round((ms_m - ms_p) * 1e3, 1),
                                             "points": int(meshed.count[-1].item()), "faces": int(meshed.face_count[-1].item())}
        return row
    finally:
        m.enable_graph(False)
        m.destroy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "1x518", "none"], default="", help="measure this scene only (a kernel trace per scene; none: --model alone)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--model", action="store_true", help="also md_infer_points_mesh against md_infer_points_render (DA3 small, 3x518x518)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {}
    for name, B, S in (("8x1536", 8, 1536), ("1x518", 1, 518)):
        if a.case and a.case != name:
            continue
        d, c, f = _scene(B, S)
        kw = dict(focal_px=f, conf=c, dense=False, depth_min=0.5, depth_max=6.0, conf_min=1.8)
        plain = ops.unproject(dev, d, **kw)
        row = {"pixels": B * S * S, "points": int(plain.count[-1].item())}
        for rtol in RTOLS:
            mesh = dict(max_rtol=rtol)
            out = ops.unproject(dev, d, mesh=mesh, **kw)
            ms_p, ms_m = _abba(lambda: ops.unproject(dev, d, out=plain, **kw), lambda: ops.unproject(dev, d, out=out, mesh=mesh, **kw), a.steps, a.warmup)
            ms_g = _time(lambda: ops.mesh_grid(dev, d, out.pixel_index, max_rtol=rtol, vertex_limit=int(out.xyz.shape[0]), faces=out.faces,
                                               face_count=out.face_count), a.steps, a.warmup)
            faces = int(out.face_count[-1].item())
            px = B * S * S
            nbytes = {"index": 4 * px + px // 8, "classify": 8 * px, "scatter": 8 * px + 12 * faces}
            r = {"list_call_us": round(ms_p * 1e3, 1), "list_and_mesh_call_us": round(ms_m * 1e3, 1), "mesh_stage_us": round((ms_m - ms_p) * 1e3, 1),
                 "mesh_grid_call_us": round(ms_g * 1e3, 1), "faces": faces, "algorithmic_bytes": nbytes,
                 "us_at_hbm_rate": {k: round(v / HBM_ACHIEVABLE * 1e6, 1) for k, v in nbytes.items()}}
            if not a.no_host:
                mask = ops.unproject(dev, d, **dict(kw, dense=True, compact=False)).mask
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hd, hm = d.cpu().numpy(), mask.cpu().numpy()
                t1 = time.perf_counter()
                pi = P.pixel_index(hm)
                hf, hc = P.mesh_grid(hd, pi, max_rtol=rtol)
                t2 = time.perf_counter()
                assert np.array_equal(hc, out.face_count.cpu().numpy()) and np.array_equal(hf, out.faces[:faces].cpu().numpy())
                assert np.array_equal(pi, out.pixel_index.cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
                del mask
            row[f"rtol{rtol}"] = r
            del out
        res[name] = row
        del d, c, plain
    if a.model:
        res["da3_small_3x518"] = _model_rows(dev, a.steps, a.warmup)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
