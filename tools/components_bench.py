"""Connected-components measurement: prints one JSON line and writes it to profiles/components_bench.json.

md_op_mesh_components alone on the two meshes of tools/mesh_bench.py, each at max_rtol 0 and 0.05: the kept list of
the seeded noise scene at 8x1536x1536 with its faces, and the cloud of DA3 `small` (seeded weights) at 3x518x518 with its faces, at
min_faces 64. Per mesh: microseconds per call without and with `compact` (the operator allocates and frees its scratch: the
kernels' own times are in a kernel trace of this tool), the components and what the largest of them holds, and two yardsticks:
the host route the call replaces (device -> host copy of the faces plus pipeline.mesh_components, on the small mesh, where both
routes are asserted to agree; --host-large adds the large one), and ops.decimate_mesh on the same mesh at the voxel side that
leaves about a quarter of the vertices.

  python tools/components_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--rtol 0.05] [--model] [--out profiles/components_bench.json]

--model adds the model call: md_infer_points_components against the same call without `comp`, DA3 `small` at 3x518x518, in A, B, B, A
order, eagerly and under graph replay, at max_rtol 0.05 (nothing reaches min_faces: the stage's fixed cost) and at 0 (all faces kept).

The kernel split of DESIGN 12.9 is the raw statistics of one trace-only run per mesh, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/components_bench.py --case 8x1536 --rtol 0 --no-host --no-yardstick --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/components_kernel_stats_rtol0_8x1536.csv (likewise --rtol 0.05)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from voxel_bench import _time  # noqa: E402

MIN_FACES = 64


def _noise_mesh(dev, rtol):
    from burn_depth_amd import ops
    from mesh_bench import _scene
    d, c, f = _scene(8, 1536)
    pc = ops.unproject(dev, d, focal_px=f, conf=c, dense=False, depth_min=0.5, depth_max=6.0, conf_min=1.8, mesh=dict(max_rtol=rtol))
    n, nf = int(pc.count[-1].item()), int(pc.face_count[-1].item())
    return pc.xyz[:n].clone(), pc.conf[:n].clone(), pc.faces[:nf].clone()


def _da3(dev):
    import torch
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, 3
    x = ((torch.rand(3, 3, 518, 518, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
    return DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY), x


def _da3_mesh(dev, rtol):
    m, x = _da3(dev)
    try:
        pc = m.infer_points(x, dense=False, world=True, mesh=dict(max_rtol=rtol))
        n, nf = int(pc.count[-1].item()), int(pc.face_count[-1].item())
        return pc.xyz[:n].clone(), pc.conf[:n].clone(), pc.faces[:nf].clone()
    finally:
        m.destroy()


def _model_rows(dev, steps, warmup):
    """md_infer_points_components against the same call without `comp` (md_infer_points_mesh's launches): DA3 `small` at
    3x518x518, min_faces 64; A, B, B, A, eagerly and under graph replay. Two cuts: max_rtol 0.05, where no component reaches
    min_faces and the stage keeps nothing (its fixed cost over the rows), and max_rtol 0, where it keeps the whole mesh (the
    hook over three components of one view each, and the scatter of every face)"""
    from mesh_bench import _abba
    m, x = _da3(dev)
    try:
        comp = dict(min_faces=MIN_FACES)
        rows = {"min_faces": MIN_FACES}
        for rtol in (0.05, 0.0):
            kw = dict(dense=False, world=True, mesh=dict(max_rtol=rtol))
            row = {}
            for mode in ("eager", "graph"):
                m.enable_graph(mode == "graph")
                plain = m.infer_points(x, **kw)
                done = m.infer_points(x, components=comp, **kw)
                ms_p, ms_c = _abba(lambda: m.infer_points(x, out=plain, **kw), lambda: m.infer_points(x, out=done, components=comp, **kw), steps, warmup)
                row[mode] = {"mesh_entry_ms": round(ms_p, 3), "components_entry_ms": round(ms_c, 3), "delta_us": round((ms_c - ms_p) * 1e3, 1),
                             "vertices": int(plain.count[-1].item()), "faces": int(plain.face_count[-1].item()),
                             "faces_kept": int(done.face_count[-1].item()), "stats": done.component_stats.tolist()}
            rows["max_rtol_%g" % rtol] = row
        return rows
    finally:
        m.enable_graph(False)
        m.destroy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518", "none"], default="", help="measure this mesh only (a kernel trace per mesh; none: --model alone)")
    ap.add_argument("--rtol", type=float, default=None, help="measure this max_rtol only (default: 0 and 0.05)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-large", action="store_true", help="the host route of the 8x1536 mesh too")
    ap.add_argument("--no-yardstick", action="store_true", help="skip ops.decimate_mesh on the same mesh")
    ap.add_argument("--model", action="store_true", help="also md_infer_points_components against the call without it (DA3 small, 3x518x518)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    from voxel_bench import _voxel_for
    dev = Device(0)
    res = {}
    for name, make in (("8x1536", _noise_mesh), ("da3_3x518", _da3_mesh)):
        if a.case and a.case != name:
            continue
        res[name] = {}
        for rtol in ((0.0, 0.05) if a.rtol is None else (a.rtol,)):
            xyz, conf, faces = make(dev, rtol)
            n, nf = int(xyz.shape[0]), int(faces.shape[0])
            out = ops.mesh_components(dev, faces, n, MIN_FACES)
            full = ops.mesh_components(dev, faces, n, MIN_FACES, xyz=xyz, conf=conf, compact=True)
            stats, k = out.component_stats.tolist(), int(out.face_count[-1].item())
            ms = _time(lambda: ops.mesh_components(dev, faces, n, MIN_FACES, out=out), a.steps, a.warmup)
            ms_c = _time(lambda: ops.mesh_components(dev, faces, n, MIN_FACES, xyz=xyz, conf=conf, compact=True, out=full), a.steps, a.warmup)
            r = {"vertices": n, "faces": nf, "min_faces": MIN_FACES, "faces_invalid": stats[0], "faces_dropped": stats[1], "faces_kept": k,
                 "components": stats[3], "components_kept": stats[4], "largest_component_faces": int(out.component_faces.max().item()) if n else 0,
                 "vertices_out": int(full.count[-1].item()), "call_us": round(ms * 1e3, 1), "compact_call_us": round(ms_c * 1e3, 1)}
            r["largest_component_share"] = round(r["largest_component_faces"] / max(nf - stats[0], 1), 4)
            if not a.no_yardstick:
                voxel = _voxel_for(dev, xyz, conf, 0.25)
                dec = ops.decimate_mesh(dev, xyz, faces, voxel, conf=conf)
                r["decimate_mesh_call_us"] = round(_time(lambda: ops.decimate_mesh(dev, xyz, faces, voxel, conf=conf, out=dec), a.steps, a.warmup) * 1e3, 1)
                del dec
            if not a.no_host and (name != "8x1536" or a.host_large):
                t0 = time.perf_counter()
                hf = faces.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.mesh_components(hf, n, MIN_FACES)
                t2 = time.perf_counter()
                assert ref.stats.tolist() == stats and ref.face_count.tolist() == out.face_count.tolist()
                assert np.array_equal(ref.label, out.label.cpu().numpy()) and np.array_equal(ref.component_faces, out.component_faces.cpu().numpy())
                assert np.array_equal(ref.faces, out.faces[:k].cpu().numpy()) and np.array_equal(ref.face_index, out.face_index[:k].cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            res[name]["max_rtol_%g" % rtol] = r
            print(json.dumps({name: {"max_rtol_%g" % rtol: r}}), flush=True)
            del xyz, conf, faces, out, full
    if a.model:
        res["model_call_da3_small_3x518"] = _model_rows(dev, a.steps, a.warmup)
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
