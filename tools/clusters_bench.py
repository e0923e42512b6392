"""DBSCAN / Euclidean clustering measurement: prints one JSON line and writes it to profiles/clusters_bench.json.

md_op_cluster_points alone on the two device lists of tools/voxel_bench.py: the kept list of the seeded noise scene at 8x1536x1536
and the cloud of DA3 `small` (seeded weights) at 3x518x518. Per list two radii, found on the device by bisection so that roughly
0.9 and 0.5 of the rows fall into kept clusters (k = 0, min_points = 10), each at k = 0 and k = 8. Milliseconds per call (the
operator allocates and frees its scratch), the yardstick md_op_radius_outliers at the same radius with k = 2^20, which also walks
all 27 buckets to their ends, the ratio of the two, and at the small list the host route the call replaces: device -> host copy of
the list plus pipeline.cluster_points, asserted bit-equal.

  python tools/clusters_bench.py [--steps 20] [--warmup 3] [--case da3_3x518] [--no-host] [--stats da3_3x518=DIR ...] [--out profiles/clusters_bench.json]

The union kernel's share is the raw statistics of one trace-only run per list at the first radius and k = 8, read back through --stats:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/clusters_bench.py --case da3_3x518 --trace-config R --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/clusters_kernel_stats_da3_3x518.csv"""
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

MIN_POINTS = 10
SHARES = (0.9, 0.5)


def _kernel_shares(folder):
    """the kernels of a rocprofv3 --kernel-trace --stats run of --trace-config: name -> microseconds per launch, and the shares of the
    union, count and border kernels in their sum"""
    files = glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {folder}")
    rows = {}
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            kernel = re.search(r"\b(clusters_\w+|voxel_scan_kernel|voxel_scatter_kernel|decimate_rank_kernel)\b", r["Name"])
            if kernel:
                short = kernel.group(1)
                calls, ns = rows.get(short, (0, 0))
                rows[short] = (calls + int(r["Calls"]), ns + int(r["TotalDurationNs"]))
    total = sum(ns for _, ns in rows.values())
    share = lambda k: round(rows.get(f"clusters_{k}_kernel", (0, 0))[1] / total, 4) if total else None  # noqa: E731
    return {"kernels_us_per_launch": {k: round(ns / c / 1e3, 2) for k, (c, ns) in sorted(rows.items())}, "union_kernel_share": share("union"),
            "count_kernel_share": share("count"), "border_kernel_share": share("border"), "stats_file": os.path.basename(files[0])}, files[0]


def _radius_for_share(ops, dev, xyz, share, extent):
    """the radius at which about `share` of the rows lie in kept clusters at k = 0: bisection on the device, 12 steps"""
    n = int(xyz.shape[0])
    lo, hi = 0.0, 0.05 * extent
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        kept = int(ops.cluster_points(dev, xyz, radius=mid, min_points=MIN_POINTS, table=0).clusters.stats[3].item())
        lo, hi = (lo, mid) if kept >= share * n else (mid, hi)
    return float(np.float32(hi))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only (a kernel trace per list)")
    ap.add_argument("--trace-config", type=float, default=0.0, metavar="R", help="only radius R at k = 8, no yardstick and no host route: the run a kernel trace wraps")
    ap.add_argument("--stats", action="append", default=[], metavar="CASE=DIR", help="the rocprofv3 output folder of a --trace-config run of that list")
    ap.add_argument("--results", default="", metavar="JSON", help="with --stats: add the trace rows to the result line of an earlier run instead of measuring again")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters_bench.json"))
    a = ap.parse_args(argv)
    stats_dirs = dict(s.split("=", 1) for s in a.stats)

    def trace_rows(name, row):
        row["trace_share0.9_k8"], src = _kernel_shares(stats_dirs[name])
        if a.out:
            dst = os.path.join(os.path.dirname(os.path.abspath(a.out)), f"clusters_kernel_stats_{name}.csv")
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
    res = {"steps": a.steps, "warmup": a.warmup, "min_points": MIN_POINTS}
    for name, make in (("da3_3x518", _da3_scene), ("8x1536", _noise_scene)):
        if a.case and a.case != name:
            continue
        xyz, _ = make(dev)
        n = int(xyz.shape[0])
        fin = xyz[torch.isfinite(xyz).all(1)]
        extent = float((fin.max(0).values - fin.min(0).values).max())
        row = {"rows": n}
        if a.trace_config:
            kw = dict(radius=a.trace_config, min_neighbours=8, min_points=MIN_POINTS, table=256)
            out = ops.cluster_points(dev, xyz, **kw)
            _time(lambda: ops.cluster_points(dev, xyz, out=out, **kw), a.steps, a.warmup)
            continue
        for share in SHARES:
            radius = _radius_for_share(ops, dev, xyz, share, extent)
            yard = ops.radius_outliers(dev, xyz, radius, 1 << 20)
            yard_ms = _time(lambda: ops.radius_outliers(dev, xyz, radius, 1 << 20, out=yard), a.steps, a.warmup)
            for k in (0, 8):
                kw = dict(radius=radius, min_neighbours=k, min_points=MIN_POINTS, table=256)
                out = ops.cluster_points(dev, xyz, **kw)
                ms = _time(lambda: ops.cluster_points(dev, xyz, out=out, **kw), a.steps, a.warmup)
                stats = out.clusters.stats.cpu().numpy()
                r = {"radius": radius, "call_ms": round(ms, 3), "outliers_k2p20_ms": round(yard_ms, 3), "ratio": round(ms / yard_ms, 3),
                     "stats": stats.tolist(), "share_kept": round(float(stats[3]) / n, 4)}
                if name == "da3_3x518" and not a.no_host:
                    t0 = time.perf_counter()
                    hx = xyz.cpu().numpy()
                    t1 = time.perf_counter()
                    ref = P.cluster_points(hx, **kw)
                    t2 = time.perf_counter()
                    c = out.clusters
                    assert np.array_equal(ref.label, c.label.cpu().numpy()) and np.array_equal(ref.cluster, c.cluster.cpu().numpy())
                    assert np.array_equal(ref.cluster_size, c.cluster_size.cpu().numpy()) and np.array_equal(ref.stats, stats)
                    t = len(ref.table_label)
                    assert np.array_equal(ref.table_label, c.table_label.cpu().numpy()[:t])
                    assert np.array_equal(ref.box.view(np.uint32), c.box.cpu().numpy()[:t].view(np.uint32))
                    r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
                row[f"share{share}_k{k}"] = r
                print(json.dumps({name: {f"share{share}_k{k}": r}}), flush=True)
                del out
            del yard
        if name in stats_dirs:
            trace_rows(name, row)
        res[name] = row
        del xyz, fin
    return finish(res)


if __name__ == "__main__":
    sys.exit(main())
