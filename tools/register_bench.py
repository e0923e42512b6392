"""Rigid registration measurement: prints one JSON line and writes it to profiles/register_bench.json.

md_op_register_points alone on the two device lists of tools/match_bench.py with its perturbed target and its two radii per list,
K = 10 iterations. Milliseconds per call (the operator allocates and frees its scratch), the yardstick md_op_match_points at the
same lists and radius measured in the same run, and the ratio call / ((K + 1) match calls): an iteration is about one `nearest`
launch plus sixteen f64 accumulators and a one-workgroup reduce, and the call builds the grid once. At the small list and the
first radius also the host route the call replaces: device -> host copy of both lists plus pipeline.register_points, asserted
bit-equal.

  python tools/register_bench.py [--steps 10] [--warmup 2] [--case da3_3x518] [--no-host] [--out profiles/register_bench.json]

--metric plane (written to profiles/register_plane_bench.json): the point-to-plane form on the same lists,
radii and K against the perturbed target with that target's own normals (the list's normals under the target's rotation), and the
point-to-point call measured in the same run as the yardstick: milliseconds per call of both, their ratio, and the pairs and the RMS
distance of the first and the evaluation pass of both metrics.

A kernel trace of one list wraps a --trace-config run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/register_bench.py --case da3_3x518 --trace-config R --out \"\""""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from match_bench import ANGLE, SHARES, SHIFT, _moved, _radius_for_share  # noqa: E402
from voxel_bench import _da3_scene, _noise_scene, _time  # noqa: E402

K = 10


def _da3_scene_normals(dev, V=3, S=518):
    """voxel_bench's DA3 list with its normals"""
    import torch
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.small()
    cfg.precision, cfg.max_batch = Precision.BF16, V
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        x = ((torch.rand(V, 3, S, S, generator=torch.Generator().manual_seed(0)) - 0.45) / 0.225).cuda()
        pc = m.infer_points(x, dense=False, world=True, normals=True)
        n = int(pc.count[-1])
        return pc.xyz[:n].clone(), pc.normals[:n].clone()
    finally:
        m.destroy()


def _noise_scene_normals(dev, B=8, S=1536):
    """voxel_bench's noise list with its normals"""
    import torch
    from burn_depth_amd import ops
    rng = np.random.default_rng(7)
    d = torch.from_numpy(np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)).cuda()
    c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
    f = torch.full((B,), 0.9 * S, device="cuda")
    E = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        a = np.radians(5.0 * b)
        E[b, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[b, :, 3] = [0.5 * b, 0, 0]
    pc = ops.unproject(dev, d, focal_px=f, extrinsics=torch.from_numpy(E).cuda(), conf=c, dense=False, world=True, depth_min=0.5, depth_max=6.0,
                       conf_min=1.8, normals=True)
    n = int(pc.count[-1])
    return pc.xyz[:n].clone(), pc.normals[:n].clone()


def _plane_rows(a, torch, ops, dev, res):
    """--metric plane: both metrics on every list and radius, in one run"""
    for name, make in (("da3_3x518", _da3_scene_normals), ("8x1536", _noise_scene_normals)):
        if a.case and a.case != name:
            continue
        xyz, nrm = make(dev)
        fin = xyz[torch.isfinite(xyz).all(1)]
        extent = float((fin.max(0).values - fin.min(0).values).max())
        target = _moved(torch, xyz, extent)
        c, s = float(np.cos(ANGLE)), float(np.sin(ANGLE))
        rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=xyz.device)
        tn = (nrm @ rot.T).contiguous()
        row = {"rows": int(xyz.shape[0]), "target_rows": int(target.shape[0]), "target_rows_with_a_normal": int((tn != 0).any(1).sum())}
        for share in SHARES:
            radius = _radius_for_share(ops, dev, xyz, target, share, extent)
            r = {"radius": radius}
            for metric, kw in (("point", {}), ("plane", {"target_normals": tn})):
                out = ops.register_points(dev, xyz, target, radius, iterations=K, min_pairs=6, **kw)
                ms = _time(lambda: ops.register_points(dev, xyz, target, radius, iterations=K, min_pairs=6, **kw), a.steps, a.warmup)
                pairs = out.pairs.cpu().numpy()
                rms = lambda t: [float(np.sqrt(t[k].item() / max(int(pairs[k]), 1))) for k in (0, K)]  # noqa: E731
                r[metric] = {"call_ms": round(ms, 3), "stats": out.stats.cpu().tolist(), "pairs": pairs.tolist(), "rms_first_last": rms(out.sum_d2)}
                if metric == "plane":
                    r[metric]["rms_residual_first_last"] = rms(out.sum_r2)
                del out
            r["ratio_plane_to_point"] = round(r["plane"]["call_ms"] / r["point"]["call_ms"], 3)
            row[f"share{share}"] = r
            print(json.dumps({name: {f"share{share}": r}}), flush=True)
        res[name] = row
        del xyz, nrm, fin, target, tn


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only")
    ap.add_argument("--trace-config", type=float, default=0.0, metavar="R", help="only radius R, no yardstick and no host route: the run a kernel trace wraps")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--metric", choices=["point", "plane"], default="point", help="plane: the point-to-plane form beside the point-to-point call")
    ap.add_argument("--out", default=None, help="default: profiles/register_bench.json, or profiles/register_plane_bench.json with --metric plane")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "register_plane_bench.json" if a.metric == "plane" else "register_bench.json")
    import torch
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {"steps": a.steps, "warmup": a.warmup, "angle": ANGLE, "shift": SHIFT, "iterations": K}
    if a.metric == "plane":
        res["metric"] = "plane"
        _plane_rows(a, torch, ops, dev, res)
    for name, make in (("da3_3x518", _da3_scene), ("8x1536", _noise_scene)):
        if a.metric == "plane" or (a.case and a.case != name):
            continue
        xyz, _ = make(dev)
        n = int(xyz.shape[0])
        fin = xyz[torch.isfinite(xyz).all(1)]
        extent = float((fin.max(0).values - fin.min(0).values).max())
        target = _moved(torch, xyz, extent)
        row = {"rows": n, "target_rows": int(target.shape[0])}
        if a.trace_config:
            _time(lambda: ops.register_points(dev, xyz, target, a.trace_config, iterations=K), a.steps, a.warmup)
            continue
        for share in SHARES:
            radius = _radius_for_share(ops, dev, xyz, target, share, extent)
            yard = ops.match_points(dev, xyz, target, radius)
            yard_ms = _time(lambda: ops.match_points(dev, xyz, target, radius, out=yard), a.steps, a.warmup)
            out = ops.register_points(dev, xyz, target, radius, iterations=K)
            ms = _time(lambda: ops.register_points(dev, xyz, target, radius, iterations=K), a.steps, a.warmup)
            pairs = out.pairs.cpu().numpy()
            r = {"radius": radius, "call_ms": round(ms, 3), "match_call_ms": round(yard_ms, 3), "ratio_to_K_plus_1_match_calls": round(ms / ((K + 1) * yard_ms), 3),
                 "stats": out.stats.cpu().tolist(), "pairs": pairs.tolist(), "rms_first_last": [float(np.sqrt(s / max(int(c), 1))) for s, c in
                                                                                                  ((out.sum_d2[0].item(), pairs[0]), (out.sum_d2[K].item(), pairs[K]))]}
            if name == "da3_3x518" and share == SHARES[0] and not a.no_host:
                t0 = time.perf_counter()
                hx, ht = xyz.cpu().numpy(), target.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.register_points(hx, ht, radius, iterations=K)
                t2 = time.perf_counter()
                assert np.array_equal(ref.transform.view(np.uint64), out.transform.cpu().numpy().view(np.uint64))
                assert np.array_equal(ref.pairs, pairs) and np.array_equal(ref.stats, out.stats.cpu().numpy())
                assert np.array_equal(ref.sum_d2.view(np.uint64), out.sum_d2.cpu().numpy().view(np.uint64))
                assert np.array_equal(ref.nearest, out.nearest.cpu().numpy()) and ref.dropped == int(out.dropped.item())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[f"share{share}"] = r
            print(json.dumps({name: {f"share{share}": r}}), flush=True)
            del out, yard
        res[name] = row
        del xyz, fin, target
    line = json.dumps(res)
    print(line)
    if a.out and not a.trace_config:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
