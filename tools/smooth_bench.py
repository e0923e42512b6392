"""Mesh-smoothing measurement: prints one JSON line and writes it to profiles/smooth_bench.json.

md_op_smooth_mesh alone on the two meshes of tools/components_bench.py at max_rtol 0.05: the kept list of the seeded noise scene
at 8x1536x1536 with its faces, and the cloud of DA3 `small` (seeded weights) at 3x518x518 with its faces; Taubin (lambda 0.5,
mu -0.53) with the boundary pinned and normals, at iterations 1 and 10, the lattice side the list's largest |coordinate| / 2^21.
Per mesh and iteration count: microseconds per call (the operator allocates and frees its scratch: the kernels' own times are in a
kernel trace of this tool), the counters, and the host route the call replaces (device -> host copy of the rows and faces plus
pipeline.smooth_mesh) on the small mesh, where both routes are asserted to give equal bits (--host-large adds the large one). A
fan of 10^5 faces around one row is timed too: the contended accumulator.

  python tools/smooth_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--iterations 10] [--model] [--out profiles/smooth_bench.json]

--model adds the model call: md_infer_points_smooth against the same call without `smooth`, DA3 `small` at 3x518x518, in A, B, B, A
order, eagerly and under graph replay.

The kernel split of DESIGN 12.10 is the raw statistics of one trace-only run per mesh, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/smooth_bench.py --case 8x1536 --iterations 10 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/smooth_kernel_stats_8x1536.csv"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from components_bench import _da3, _da3_mesh, _noise_mesh  # noqa: E402
from voxel_bench import _time  # noqa: E402

RTOL, LAM, MU = 0.05, 0.5, -0.53


def _step(xyz) -> float:
    import torch
    v = xyz.abs()
    return float(np.float32(float(v[torch.isfinite(v)].max().item()) / 2097152.0))


def _fan_row(dev, ops, steps, warmup, F=100000):
    import torch
    a = torch.arange(F + 1, dtype=torch.float32) * (2 * np.pi / (F + 1))
    xyz = torch.cat([torch.tensor([[0.01, -0.02, 0.4]]), torch.stack([a.cos(), a.sin(), 0.05 * (7 * a).sin()], 1)]).cuda()
    f = torch.arange(F, dtype=torch.int32)
    faces = torch.stack([torch.zeros_like(f), f + 1, f + 2], 1).cuda()
    out = ops.smooth_mesh(dev, xyz, faces, 1.0 / 1048576.0, 10, LAM, mu=MU, pin_boundary=False, normals=True)
    ms = _time(lambda: ops.smooth_mesh(dev, xyz, faces, 1.0 / 1048576.0, 10, LAM, mu=MU, pin_boundary=False, normals=True, out=out), steps, warmup)
    return {"faces": F, "iterations": 10, "call_us": round(ms * 1e3, 1), "stats": out.stats.tolist()}


def _model_rows(dev, steps, warmup, iterations):
    """md_infer_points_smooth against the same call without `smooth`: DA3 `small` at 3x518x518, max_rtol 0.05; A, B, B, A,
    eagerly and under graph replay"""
    from mesh_bench import _abba
    m, x = _da3(dev)
    try:
        kw = dict(dense=False, world=True, mesh=dict(max_rtol=RTOL))
        plain = m.infer_points(x, **kw)
        n = int(plain.count[-1].item())
        rows = {"step": _step(plain.xyz[:n])}
        for it in iterations:
            sm = dict(step=rows["step"], iterations=it, lam=LAM, mu=MU, pin_boundary=True, normals=True)
            row = {}
            for mode in ("eager", "graph"):
                m.enable_graph(mode == "graph")
                plain = m.infer_points(x, **kw)
                done = m.infer_points(x, smooth=sm, **kw)
                ms_p, ms_s = _abba(lambda: m.infer_points(x, out=plain, **kw), lambda: m.infer_points(x, out=done, smooth=sm, **kw), steps, warmup)
                row[mode] = {"mesh_entry_ms": round(ms_p, 3), "smooth_entry_ms": round(ms_s, 3), "delta_us": round((ms_s - ms_p) * 1e3, 1),
                             "vertices": n, "faces": int(plain.face_count[-1].item()), "stats": done.smooth.stats.tolist()}
            rows["iterations_%d" % it] = row
        return rows
    finally:
        m.enable_graph(False)
        m.destroy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518", "fan", "none"], default="", help="measure this mesh only (a kernel trace per mesh; none: --model alone)")
    ap.add_argument("--iterations", type=int, default=None, help="measure this iteration count only (default: 1 and 10)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-large", action="store_true", help="the host route of the 8x1536 mesh too")
    ap.add_argument("--model", action="store_true", help="also md_infer_points_smooth against the call without it (DA3 small, 3x518x518)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    iterations = (1, 10) if a.iterations is None else (a.iterations,)
    res = {}
    for name, make in (("8x1536", _noise_mesh), ("da3_3x518", _da3_mesh)):
        if a.case and a.case != name:
            continue
        xyz, _, faces = make(dev, RTOL)
        n, nf, step = int(xyz.shape[0]), int(faces.shape[0]), _step(xyz)
        res[name] = {"vertices": n, "faces": nf, "step": step}
        for it in iterations:
            kw = dict(mu=MU, pin_boundary=True, normals=True)
            out = ops.smooth_mesh(dev, xyz, faces, step, it, LAM, **kw)
            ms = _time(lambda: ops.smooth_mesh(dev, xyz, faces, step, it, LAM, out=out, **kw), a.steps, a.warmup)
            r = {"iterations": it, "call_us": round(ms * 1e3, 1), "stats": out.stats.tolist()}
            if not a.no_host and (name != "8x1536" or a.host_large):
                t0 = time.perf_counter()
                hx, hf = xyz.cpu().numpy(), faces.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.smooth_mesh(hx, hf, step, it, LAM, **kw)
                t2 = time.perf_counter()
                assert ref.stats.tolist() == r["stats"]
                assert np.array_equal(ref.xyz.view(np.uint32), out.xyz.cpu().numpy().view(np.uint32))
                assert np.array_equal(ref.normals.view(np.uint32), out.normals.cpu().numpy().view(np.uint32))
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            res[name]["iterations_%d" % it] = r
            print(json.dumps({name: r}), flush=True)
            del out
        del xyz, faces
    if a.case in ("", "fan"):
        res["fan"] = _fan_row(dev, ops, a.steps, a.warmup)
        print(json.dumps({"fan": res["fan"]}), flush=True)
    if a.model:
        res["model_call_da3_small_3x518"] = _model_rows(dev, a.steps, a.warmup, iterations)
        print(json.dumps({"model_call_da3_small_3x518": res["model_call_da3_small_3x518"]}), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
