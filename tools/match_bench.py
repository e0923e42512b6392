"""Cloud-to-cloud matching measurement: prints one JSON line and writes it to profiles/match_bench.json.

md_op_match_points alone on the two device lists of tools/voxel_bench.py: the kept list of the seeded noise scene at 8x1536x1536
and the cloud of DA3 `small` (seeded weights) at 3x518x518. The target is the same list under a small rigid motion (a rotation
about z and a shift, both a fraction of the extent). Per list two radii, found on the device by bisection so that roughly 0.9
and 0.5 of the rows have a counterpart. Milliseconds per call (the operator allocates and frees its scratch), the yardstick
md_op_radius_outliers on the target list at the same radius with k = 2^20, which walks all 27 buckets to their ends, the ratio of
the two, and at the small list the host route the call replaces: device -> host copy of both lists plus pipeline.match_points,
asserted bit-equal.

  python tools/match_bench.py [--steps 20] [--warmup 3] [--case da3_3x518] [--no-host] [--stats da3_3x518=DIR ...] [--out profiles/match_bench.json]

The kernels' shares are the raw statistics of one trace-only run per list at the first radius, read back through --stats:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/match_bench.py --case da3_3x518 --trace-config R --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/match_kernel_stats_da3_3x518.csv"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from voxel_bench import _da3_scene, _noise_scene, _time  # noqa: E402

SHARES = (0.9, 0.5)
ANGLE, SHIFT = 2e-3, 1e-3  # the rigid motion of the target: radians about z, and the shift as a fraction of the extent


def _kernel_shares(folder):
    """the kernels of a rocprofv3 --kernel-trace --stats run of --trace-config: name -> microseconds per launch, and the share of
    the nearest kernel in their sum"""
    files = glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {folder}")
    rows = {}
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            kernel = re.search(r"\b(match_\w+|voxel_scan_kernel|voxel_scatter_kernel)\b", r["Name"])
            if kernel:
                short = kernel.group(1)
                calls, ns = rows.get(short, (0, 0))
                rows[short] = (calls + int(r["Calls"]), ns + int(r["TotalDurationNs"]))
    total = sum(ns for _, ns in rows.values())
    return {"kernels_us_per_launch": {k: round(ns / c / 1e3, 2) for k, (c, ns) in sorted(rows.items())},
            "kernel_shares": {k: round(ns / total, 4) for k, (_, ns) in sorted(rows.items())} if total else None,
            "stats_file": os.path.basename(files[0])}, files[0]


def _moved(torch, xyz, extent):
    """the list under the rigid motion; rows that are not finite stay as they are"""
    c, s = float(np.cos(ANGLE)), float(np.sin(ANGLE))
    rot = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32, device=xyz.device)
    return (xyz @ rot.T + torch.tensor([SHIFT * extent, -SHIFT * extent, SHIFT * extent], dtype=torch.float32, device=xyz.device)).contiguous()


def _radius_for_share(ops, dev, xyz, target, share, extent):
    """the radius at which about `share` of the rows have a counterpart: bisection on the device, 12 steps"""
    n = int(xyz.shape[0])
    lo, hi = 0.0, 0.05 * extent
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        hit = int(ops.match_points(dev, xyz, target, mid).match.stats[1].item())
        lo, hi = (lo, mid) if hit >= share * n else (mid, hi)
    return float(np.float32(hi))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only (a kernel trace per list)")
    ap.add_argument("--trace-config", type=float, default=0.0, metavar="R", help="only radius R, no yardstick and no host route: the run a kernel trace wraps")
    ap.add_argument("--stats", action="append", default=[], metavar="CASE=DIR", help="the rocprofv3 output folder of a --trace-config run of that list")
    ap.add_argument("--results", default="", metavar="JSON", help="with --stats: add the trace rows to the result line of an earlier run instead of measuring again")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    a = ap.parse_args(argv)
    stats_dirs = dict(s.split("=", 1) for s in a.stats)

    def trace_rows(name, row):
        row["trace_share0.9"], src = _kernel_shares(stats_dirs[name])
        if a.out:
            dst = os.path.join(os.path.dirname(os.path.abspath(a.out)), f"match_kernel_stats_{name}.csv")
            with open(src) as fi, open(dst, "w") as fo:
                fo.write(fi.read())

    def finish(res):
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return 0

    if a.results:  # the radii of the traces come from that run
        with open(a.results) as fh:
            res = json.loads(fh.read())
        for name in stats_dirs:
            trace_rows(name, res[name])
        return finish(res)
    import torch
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {"steps": a.steps, "warmup": a.warmup, "angle": ANGLE, "shift": SHIFT}
    for name, make in (("da3_3x518", _da3_scene), ("8x1536", _noise_scene)):
        if a.case and a.case != name:
            continue
        xyz, _ = make(dev)
        n = int(xyz.shape[0])
        fin = xyz[torch.isfinite(xyz).all(1)]
        extent = float((fin.max(0).values - fin.min(0).values).max())
        target = _moved(torch, xyz, extent)
        row = {"rows": n, "target_rows": int(target.shape[0])}
        if a.trace_config:
            out = ops.match_points(dev, xyz, target, a.trace_config)
            _time(lambda: ops.match_points(dev, xyz, target, a.trace_config, out=out), a.steps, a.warmup)
            continue
        for share in SHARES:
            radius = _radius_for_share(ops, dev, xyz, target, share, extent)
            yard = ops.radius_outliers(dev, target, radius, 1 << 20)
            yard_ms = _time(lambda: ops.radius_outliers(dev, target, radius, 1 << 20, out=yard), a.steps, a.warmup)
            tol = (radius / 2, radius)
            out = ops.match_points(dev, xyz, target, radius, tol=tol)
            ms = _time(lambda: ops.match_points(dev, xyz, target, radius, tol=tol, out=out), a.steps, a.warmup)
            stats = out.match.stats.cpu().numpy()
            r = {"radius": radius, "call_ms": round(ms, 3), "outliers_k2p20_ms": round(yard_ms, 3), "ratio": round(ms / yard_ms, 3),
                 "stats": stats.tolist(), "share_matched": round(float(stats[1]) / n, 4)}
            if name == "da3_3x518" and not a.no_host:
                t0 = time.perf_counter()
                hx, ht = xyz.cpu().numpy(), target.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.match_points(hx, ht, radius, tol=tol)
                t2 = time.perf_counter()
                assert np.array_equal(ref.nearest, out.match.nearest.cpu().numpy()) and np.array_equal(ref.stats, stats)
                assert np.array_equal(ref.dist2.view(np.uint32), out.match.dist2.cpu().numpy().view(np.uint32))
                assert ref.dropped == int(out.match.dropped.item())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[f"share{share}"] = r
            print(json.dumps({name: {f"share{share}": r}}), flush=True)
            del out, yard
        if name in stats_dirs:
            trace_rows(name, row)
        res[name] = row
        del xyz, fin, target
    return finish(res)


if __name__ == "__main__":
    sys.exit(main())
