"""Mesh rasterisation measurement: prints one JSON line and writes it to profiles/raster_bench.json.

Two scenes at 8x1536x1536 and 1x518x518, unprojected into one world frame (render_bench's eight cameras) with the mesh of the
list at max_rtol 0.05:
  noise    section 12's seeded noise scene (points_bench / mesh_bench / render_bench: log-normal depth, 42 % of the pixels kept
           by conf_min). Neighbouring depths differ by far more than 5 %, so max_rtol 0.05 leaves almost no face: the row shows
           what the call costs when the mesh is nearly empty.
  smooth   a wavy surface with a depth step (tools/mesh_bench.py has no smooth scene; this one is this tool's own): every quad
           away from the step gives two faces.
Each mesh is rendered into its own first camera (triangles of about one pixel) and into a camera at half the distance
(triangles of 2x2 to 4x4 pixels: the `large` path is live). Per form: microseconds per md_op_render_mesh call, filled pixels,
skipped faces; beside it md_op_render_points at radius 0 and 1 on the same list; and the host route (list and faces copied to
the host, pipeline.render_mesh; 1x518 only unless --host-all). The operators allocate and free their scratch inside the call:
the kernels' own times are in a kernel trace of this tool.

  python tools/raster_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--no-host] [--lib PATH] [--only-mesh] [--out FILE]

`--lib PATH` loads another build of the library (kernels/raster.hip built with -DMD_RASTER_INLINE_PIXELS=N) for the A, B, B, A
comparison of DESIGN 12.6; `--only-mesh` then skips the point renders and the host route.
The kernel table of DESIGN 12.6 is the raw statistics of one trace-only run, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/raster_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/raster_kernel_stats_8x1536.csv"""
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


def _scene(dev, kind, B, S):
    """depth, confidence and cameras of a scene -> the world-space list with its mesh, colours, focal lengths and extrinsics"""
    from burn_depth_amd import ops
    rng = np.random.default_rng(7)
    if kind == "noise":
        d = np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)
        kw = dict(depth_min=0.5, depth_max=6.0, conf_min=1.8)
    else:
        v, u = np.mgrid[0:S, 0:S] / S
        d = np.stack([2.0 + 0.3 * np.sin(9 * u + b) + 0.2 * np.cos(7 * v) + 1.5 * (u > 0.6) for b in range(B)]).astype(np.float32)
        kw = dict()
    c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
    f = torch.full((B,), 0.9 * S, device="cuda")
    E = np.zeros((B, 3, 4), np.float32)
    for b in range(B):  # cameras turned by 5 degrees each about Y, half a unit apart
        a = np.radians(5.0 * b)
        E[b, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[b, :, 3] = [0.5 * b, 0, 0]
    near = E[:1].copy()
    near[0, 2, 3] -= 0.5 * float(np.median(d[0]))  # the first camera moved half the median depth towards the scene
    E = torch.from_numpy(E).cuda()
    pc = ops.unproject(dev, torch.from_numpy(d).cuda(), focal_px=f, extrinsics=E, conf=c, dense=False, world=True,
                       mesh=dict(max_rtol=0.05, pixel_index=False), **kw)
    n = int(pc.count[-1].item())
    rgb = torch.randint(0, 256, (int(pc.xyz.shape[0]), 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    return pc, n, rgb, f, {"own": E[:1].contiguous(), "half": torch.from_numpy(near).cuda()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "1x518"], default="", help="measure this size only (a kernel trace per size)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-all", action="store_true", help="the host route at 8x1536 too (minutes)")
    ap.add_argument("--only-mesh", action="store_true", help="md_op_render_mesh alone: no point renders, no host route")
    ap.add_argument("--lib", default="", help="another build of libmi_depth.so (the kInlinePixels comparison)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {"inline_pixels": ops.raster_inline_pixels()}
    for name, B, S in (("8x1536", 8, 1536), ("1x518", 1, 518)):
        if a.case and a.case != name:
            continue
        for kind in ("noise", "smooth"):
            pc, n, rgb, f, cams = _scene(dev, kind, B, S)
            faces = int(pc.face_count[-1].item())
            row = {"points": n, "faces": faces}
            for cam, E in cams.items():
                kw = dict(focal_px=f[:1].contiguous(), extrinsics=E)
                mesh = lambda out=None: ops.render_mesh(dev, pc.xyz, pc.faces, S, S, rgb=rgb, face_count=pc.face_count[-1:], out=out, **kw)  # noqa: E731
                out = mesh()
                ms = _time(lambda: mesh(out), a.steps, a.warmup)
                px = S * S
                # what the call must move: the faces and their vertices once, 8 B per pixel of keys cleared and read, the images written
                nbytes = 12 * faces + 36 * faces + 8 * px * 2 + px * (4 + 4 + 3) + 9 * 3 * int(out.filled[-1].item())
                r = {"mesh_call_us": round(ms * 1e3, 1), "filled": int(out.filled[-1].item()), "skipped": int(out.skipped[-1].item()),
                     "algorithmic_bytes": nbytes, "us_at_hbm_rate": round(nbytes / HBM_ACHIEVABLE * 1e6, 1)}
                if not a.only_mesh:
                    for radius in (0, 1):
                        pts = lambda o=None: ops.render_points(dev, pc.xyz, S, S, rgb=rgb, count=pc.count[-1:], radius=radius, out=o, **kw)  # noqa: E731
                        o = pts()
                        r[f"points_r{radius}_call_us"] = round(_time(lambda: pts(o), a.steps, a.warmup) * 1e3, 1)
                        r[f"points_r{radius}_filled"] = int(o.filled[-1].item())
                    if not a.no_host and (name == "1x518" or a.host_all):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        hx, hf, hc = pc.xyz[:n].cpu().numpy(), pc.faces[:faces].cpu().numpy(), rgb[:n].cpu().numpy()
                        t1 = time.perf_counter()
                        ref = P.render_mesh(hx, hf, S, S, focal_px=f[:1].cpu().numpy(), extrinsics=E.cpu().numpy(), rgb=hc)
                        t2 = time.perf_counter()
                        same = all(np.array_equal(getattr(ref, k).view(np.uint8), getattr(out, k).cpu().numpy().view(np.uint8))
                                   for k in ("depth", "face", "rgb", "filled", "skipped"))
                        r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1), "same_bits": bool(same)}
                row[cam] = r
                del out
            res[f"{name}_{kind}"] = row
            del pc, rgb
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
