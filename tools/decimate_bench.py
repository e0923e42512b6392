"""Mesh decimation measurement: prints one JSON line and writes it to profiles/decimate_bench.json.

md_op_decimate_mesh alone on the two meshes of tools/mesh_bench.py, each at max_rtol 0: the kept list of the seeded
noise scene at 8x1536x1536 with its faces, and the cloud of DA3 `small` (seeded weights) at 3x518x518 with its faces. Per mesh two
voxel sides, found by bisection on the device, that leave about 0.25 and about 0.05 of the vertices. Microseconds per call (the
operator allocates and frees its scratch: the kernels' own times are in a kernel trace of this tool), the faces of every class,
the algorithmic bytes (voxel thinning's, remap written and read once per row, per face the triple read, three remap words gathered,
the mapped triple written and read by insert, select and scatter, one probed triple, the slot word written and read, 4 B per
table slot reset and one slot read twice, the kept rows written) against the achievable HBM rate, and the host route the call
replaces: device -> host copy of the vertices and faces plus pipeline.decimate_mesh, on the small mesh (the large one's host
route is left out by default: --host-large adds it).

  python tools/decimate_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--model] [--out profiles/decimate_bench.json]

--model adds the model call: md_infer_points_decimate against the same call without `dec`, DA3 `small` at 3x518x518, in A, B, B, A
order, eagerly and under graph replay.

The kernel table of DESIGN 12.8 is the raw statistics of one trace-only run per mesh, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/decimate_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/decimate_kernel_stats_8x1536.csv"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from voxel_bench import HBM_ACHIEVABLE, _time  # noqa: E402


def _noise_mesh(dev):
    from burn_depth_amd import ops
    from mesh_bench import _scene
    d, c, f = _scene(8, 1536)
    pc = ops.unproject(dev, d, focal_px=f, conf=c, dense=False, depth_min=0.5, depth_max=6.0, conf_min=1.8, mesh=dict(max_rtol=0.0))
    n, nf = int(pc.count[-1].item()), int(pc.face_count[-1].item())
    return pc.xyz[:n].clone(), pc.conf[:n].clone(), pc.faces[:nf].clone()


def _da3_mesh(dev):
    import torch
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, 3
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(3, 3, 518, 518, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        pc = m.infer_points(x, dense=False, world=True, mesh=dict(max_rtol=0.0))
        n, nf = int(pc.count[-1].item()), int(pc.face_count[-1].item())
        return pc.xyz[:n].clone(), pc.conf[:n].clone(), pc.faces[:nf].clone()
    finally:
        m.destroy()


def _model_rows(dev, steps, warmup):
    """md_infer_points_decimate against the same call without `dec` (md_infer_points_mesh's launches): DA3 `small` at 3x518x518,
    max_rtol 0, the voxel side that leaves about a quarter of the vertices; A, B, B, A, eagerly and under graph replay"""
    import torch
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from mesh_bench import _abba
    from voxel_bench import _voxel_for
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, 3
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(3, 3, 518, 518, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        kw = dict(dense=False, world=True, mesh=dict(max_rtol=0.0))
        plain = m.infer_points(x, **kw)
        n = int(plain.count[-1].item())
        voxel = _voxel_for(dev, plain.xyz[:n].clone(), plain.conf[:n].clone(), 0.25)
        dec = dict(voxel=voxel)
        row = {"voxel": voxel}
        for mode in ("eager", "graph"):
            m.enable_graph(mode == "graph")
            plain = m.infer_points(x, **kw)
            done = m.infer_points(x, decimate=dec, **kw)
            ms_p, ms_d = _abba(lambda: m.infer_points(x, out=plain, **kw), lambda: m.infer_points(x, out=done, decimate=dec, **kw), steps, warmup)
            row[mode] = {"mesh_entry_ms": round(ms_p, 3), "decimate_entry_ms": round(ms_d, 3), "delta_us": round((ms_d - ms_p) * 1e3, 1),
                         "vertices": int(plain.count[-1].item()), "faces": int(plain.face_count[-1].item()),
                         "vertices_out": int(done.count[-1].item()), "faces_kept": int(done.face_count[-1].item()),
                         "faces_dropped": done.faces_dropped.tolist()}
        return row
    finally:
        m.enable_graph(False)
        m.destroy()


def _slots(n):
    s = 1024
    while s < 2 * n:
        s *= 2
    return s


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518", "none"], default="", help="measure this mesh only (a kernel trace per mesh; none: --model alone)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--host-large", action="store_true", help="the host route of the 8x1536 mesh too")
    ap.add_argument("--model", action="store_true", help="also md_infer_points_decimate against the call without it (DA3 small, 3x518x518)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decimate_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    from voxel_bench import _voxel_for
    dev = Device(0)
    res = {}
    for name, make in (("8x1536", _noise_mesh), ("da3_3x518", _da3_mesh)):
        if a.case and a.case != name:
            continue
        xyz, conf, faces = make(dev)
        n, nf = int(xyz.shape[0]), int(faces.shape[0])
        row = {"vertices": n, "faces": nf, "vertex_table_slots": _slots(n), "face_table_slots": _slots(nf)}
        out = ops.decimate_mesh(dev, xyz, faces, 1.0, conf=conf)
        for label, share in (("quarter", 0.25), ("twentieth", 0.05)):
            voxel = _voxel_for(dev, xyz, conf, share)
            ops.decimate_mesh(dev, xyz, faces, voxel, conf=conf, out=out)
            m, k = int(out.count[-1].item()), int(out.face_count[-1].item())
            classes = out.faces_dropped.tolist()
            ms = _time(lambda: ops.decimate_mesh(dev, xyz, faces, voxel, conf=conf, out=out), a.steps, a.warmup)
            ms_thin = _time(lambda: ops.voxel_thin(dev, xyz, voxel, conf=conf, out=out), a.steps, a.warmup)
            live = nf - classes[0] - classes[1]
            nbytes = (n * (12 + 4 + 4) + n * (4 + 8) + 20 * _slots(n) + m * (12 + 12 + 4 + 4 + 4)  # voxel thinning: insert, select, table, scatter
                      + n * (4 + 8 + 4 + 4)                                                        # remap: slot, rank word, survivor's row, the row
                      + nf * (12 + 12 + 12) + live * (12 + 12 + 4 + 4)                             # map; insert: own and one probed triple, slot
                      + nf * (4 + 4 + 4) + 4 * _slots(nf) + k * (12 + 12 + 4))                     # select; table reset; scatter
            r = {"voxel": voxel, "vertices_out": m, "share": round(m / n, 4), "faces_invalid": classes[0], "faces_degenerate": classes[1],
                 "faces_duplicate": classes[2], "faces_kept": k, "call_us": round(ms * 1e3, 1), "voxel_thin_call_us": round(ms_thin * 1e3, 1),
                 "algorithmic_bytes": int(nbytes), "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3)}
            if not a.no_host and (name != "8x1536" or a.host_large):
                t0 = time.perf_counter()
                hx, hc, hf = xyz.cpu().numpy(), conf.cpu().numpy(), faces.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.decimate_mesh(hx, hf, voxel, hc)
                t2 = time.perf_counter()
                assert int(ref.vertices.count[-1]) == m and ref.faces_dropped.tolist() == classes and len(ref.faces) == k
                assert np.array_equal(ref.remap, out.remap.cpu().numpy()) and np.array_equal(ref.faces, out.faces[:k].cpu().numpy())
                assert np.array_equal(ref.face_index, out.face_index[:k].cpu().numpy())
                assert np.array_equal(ref.vertices.index, out.index[:m].cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[label] = r
            print(json.dumps({name: {label: r}}), flush=True)
        res[name] = row
        del xyz, conf, faces, out
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
