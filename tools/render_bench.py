"""Point rendering measurement: prints one JSON line and writes it to profiles/render_bench.json.

md_op_render_points alone on device lists: the kept list of tools/points_bench.py's seeded noise scene at 8x1536x1536
(world = 1, eight cameras on a circle) rendered into T = 1 and 4 of its own cameras at 1536x1536 with radius 0 and 1, and the
1x518x518 list into one 518x518 target. Microseconds per call (the operator allocates and frees its key buffer: the kernels'
own times are in a kernel trace of this tool), the candidates (visible point-target pairs times the footprint), the
algorithmic bytes per kernel (clear 8 B per pixel; splat 12 B per row read and 8 B per candidate; resolve 8 B read and
4 + 4 + 3 B written per pixel) and the time those bytes take at the achievable HBM rate, and the host route the call
replaces: device -> host copy of the list plus pipeline.render_points (T = 1, radius 0 only: numpy's minimum.at is slow).
`--model`: md_infer_points_render against md_infer_points_voxel at DA3 `small` 3x518x518, eager and graph.

  python tools/render_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--no-host] [--model] [--lib PATH] [--out FILE]

`--lib`: measure another build of the library (the splat without the load in front of the atomic is
`make EXTRA=-DMD_RENDER_PEEK=0 BUILD=build_nopeek OUT=../libmi_depth_nopeek.so`); the two forms are run A, B, B, A.
The kernel table of DESIGN 12.4 is the raw statistics of one trace-only run, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/render_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/render_kernel_stats_8x1536.csv"""
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


def _scene(dev, B, S):
    """the kept list of points_bench's scene in one world frame, with colours, and its cameras"""
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
    E = torch.from_numpy(E).cuda()
    pc = ops.unproject(dev, d, focal_px=f, extrinsics=E, conf=c, dense=False, world=True, depth_min=0.5, depth_max=6.0, conf_min=1.8)
    n = int(pc.count[-1].item())
    xyz = pc.xyz[:n].clone()
    rgb = torch.randint(0, 256, (n, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    return xyz, rgb, f, E


def _visible_pairs(xyz, f, E, S):
    """point-target pairs inside the image (torch arithmetic: a count for the byte model, not the contract)"""
    total = 0
    for j in range(E.shape[0]):
        p = xyz @ E[j, :, :3].T + E[j, :, 3]
        u, v = torch.floor(f[j] * p[:, 0] / p[:, 2] + S / 2 + 0.5), torch.floor(f[j] * p[:, 1] / p[:, 2] + S / 2 + 0.5)
        total += int(((p[:, 2] > 0) & (u >= 0) & (u < S) & (v >= 0) & (v < S)).sum())
    return total


def _model_rows(dev, steps, warmup):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, 3
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(3, 3, 518, 518, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        xyz, _, _ = m.infer_points(x, dense=False, world=True).points()
        c = xyz.mean(0)  # seeded weights put the cloud anywhere: one target that looks at it along +z from twice its extent
        d = 2 * float((xyz - c).norm(dim=1).max())
        K = torch.tensor([[[0.9 * 518, 0, 259], [0, 0.9 * 518, 259], [0, 0, 1]]], device="cuda")
        E = torch.tensor([[[1.0, 0, 0, -float(c[0])], [0, 1, 0, -float(c[1])], [0, 0, 1, d - float(c[2])]]], device="cuda")
        render = dict(H=518, W=518, intrinsics=K, extrinsics=E)
        row = {}
        for mode in ("eager", "graph"):
            m.enable_graph(mode == "graph")
            plain = m.infer_points(x, dense=False, world=True)
            rend = m.infer_points(x, dense=False, world=True, render=render)
            ms_p = _time(lambda: m.infer_points(x, dense=False, world=True, out=plain), steps, warmup)
            ms_r = _time(lambda: m.infer_points(x, dense=False, world=True, out=rend, render=render), steps, warmup)
            row[mode] = {"voxel_entry_ms": round(ms_p, 3), "render_entry_ms": round(ms_r, 3), "delta_us": round((ms_r - ms_p) * 1e3, 1),
                         "filled": int(rend.render.filled[-1].item())}
        return row
    finally:
        m.enable_graph(False)
        m.destroy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "1x518", "none"], default="", help="measure this list only (a kernel trace per list; none: --model alone)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--model", action="store_true", help="also md_infer_points_render against md_infer_points_voxel (DA3 small, 3x518x518)")
    ap.add_argument("--lib", default="", help="another build of libmi_depth.so to measure")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {"lib": os.path.basename(_lib.LIB_PATH)}
    for name, B, S, forms in (("8x1536", 8, 1536, ((1, 0), (1, 1), (4, 0), (4, 1))), ("1x518", 1, 518, ((1, 0),))):
        if a.case and a.case != name:
            continue
        xyz, rgb, f, E = _scene(dev, B, S)
        n = int(xyz.shape[0])
        row = {"rows": n}
        for T, radius in forms:
            kw = dict(focal_px=f[:T].contiguous(), extrinsics=E[:T].contiguous(), rgb=rgb, radius=radius)
            out = ops.render_points(dev, xyz, S, S, **kw)
            ms = _time(lambda: ops.render_points(dev, xyz, S, S, out=out, **kw), a.steps, a.warmup)
            px = T * S * S
            cand = _visible_pairs(xyz, f[:T], E[:T], S) * (2 * radius + 1) ** 2
            nbytes = {"clear": 8 * px, "splat": 12 * n + 8 * cand, "resolve": (8 + 4 + 4 + 3) * px}
            r = {"call_us": round(ms * 1e3, 1), "filled": int(out.filled[-1].item()), "pixels": px, "candidates": cand, "algorithmic_bytes": nbytes,
                 "us_at_hbm_rate": {k: round(v / HBM_ACHIEVABLE * 1e6, 1) for k, v in nbytes.items()}}
            if not a.no_host and (T, radius) == (1, 0):
                t0 = time.perf_counter()
                hx, hc = xyz.cpu().numpy(), rgb.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.render_points(hx, S, S, focal_px=f[:1].cpu().numpy(), extrinsics=E[:1].cpu().numpy(), rgb=hc)
                t2 = time.perf_counter()
                assert np.array_equal(ref.index, out.index.cpu().numpy()) and np.array_equal(ref.filled, out.filled.cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[f"T{T}_r{radius}"] = r
            del out
        res[name] = row
        del xyz, rgb
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
