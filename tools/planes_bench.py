"""RANSAC plane extraction measurement: prints one JSON line and writes it to profiles/planes_bench.json.

md_op_fit_planes alone on the two device lists of tools/voxel_bench.py: the kept list of the seeded noise scene at 8x1536x1536 and
the cloud of DA3 `small` (seeded weights) at 3x518x518. Per list P = 1 and 3 planes of Hh = 256 and 1024 hypotheses each, tol = 1 %
of the list's extent, min_inliers = 3 so that every round succeeds and runs its full work. Milliseconds per call (the operator
allocates and frees its scratch: the kernels' own times are in a kernel trace of this tool), the point-plane tests per second that
this is, and the host route the call replaces at the small list: device -> host copy of the list plus pipeline.fit_planes.

  python tools/planes_bench.py [--steps 20] [--warmup 3] [--case da3_3x518] [--stats da3_3x518=DIR ...] [--out profiles/planes_bench.json]

The count kernel's share is the raw statistics of one trace-only run per list at P = 3, Hh = 1024, read back through --stats:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/planes_bench.py --case da3_3x518 --trace-config --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/planes_kernel_stats_da3_3x518.csv"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from voxel_bench import _da3_scene, _noise_scene, _time  # noqa: E402

CONFIGS = ((1, 256), (1, 1024), (3, 256), (3, 1024))
MIN_INLIERS = 3
SEED = 1


def _kernel_shares(folder):
    """the plane kernels of a rocprofv3 --kernel-trace --stats run: name -> (calls, total ns), and the count kernel's share of them"""
    files = glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {folder}")
    rows = {}
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Name"]
            if "planes_" in name or "voxel_scan" in name or "voxel_scatter" in name:
                short = name.split("(anonymous namespace)::")[-1].split("(")[0]
                calls, ns = rows.get(short, (0, 0))
                rows[short] = (calls + int(r["Calls"]), ns + int(r["TotalDurationNs"]))
    total = sum(ns for _, ns in rows.values())
    count = sum(ns for k, (_, ns) in rows.items() if k.startswith("planes_count_kernel"))
    return {"kernels_us_per_launch": {k: round(ns / c / 1e3, 2) for k, (c, ns) in sorted(rows.items())},
            "count_kernel_share": round(count / total, 4) if total else None, "stats_file": os.path.basename(files[0])}, files[0]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only (a kernel trace per list)")
    ap.add_argument("--trace-config", action="store_true", help="only P = 3, Hh = 1024 and no host route: the run a kernel trace wraps")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--stats", action="append", default=[], metavar="CASE=DIR", help="the rocprofv3 output folder of a --trace-config run of that list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planes_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    stats = dict(s.split("=", 1) for s in a.stats)
    res = {"steps": a.steps, "warmup": a.warmup, "min_inliers": MIN_INLIERS, "seed": SEED}
    for name, make in (("da3_3x518", _da3_scene), ("8x1536", _noise_scene)):
        if a.case and a.case != name:
            continue
        xyz, _ = make(dev)
        n = int(xyz.shape[0])
        fin = xyz[torch.isfinite(xyz).all(1)]
        tol = float(np.float32(0.01 * float((fin.max(0).values - fin.min(0).values).max())))
        row = {"rows": n, "tol": tol}
        for planes, hyp in (((3, 1024),) if a.trace_config else CONFIGS):
            kw = dict(planes=planes, hypotheses=hyp, tol=tol, min_inliers=MIN_INLIERS, seed=SEED)
            out = ops.fit_planes(dev, xyz, **kw)
            ms = _time(lambda: ops.fit_planes(dev, xyz, out=out, **kw), a.steps, a.warmup)
            counts = out.planes.plane_count.cpu().numpy()
            live = n - int(out.planes.dropped.item()) - np.concatenate([[0], np.cumsum(counts[:planes])[:-1]])  # live rows of every round
            tests = int(sum(int(m) * hyp for m in live[:int(counts[planes])]))
            r = {"call_ms": round(ms, 3), "planes_found": int(counts[planes]), "inliers": counts[:planes].tolist(), "tests": tests,
                 "tests_per_s": round(tests / (ms * 1e-3), 0)}
            if name == "da3_3x518" and not a.no_host and not a.trace_config:
                t0 = time.perf_counter()
                hx = xyz.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.fit_planes(hx, **kw)
                t2 = time.perf_counter()
                assert np.array_equal(ref.plane_count, counts) and np.array_equal(ref.label, out.planes.label.cpu().numpy())
                assert np.array_equal(ref.plane.view(np.uint32), out.planes.plane.cpu().numpy().view(np.uint32))
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[f"P{planes}_H{hyp}"] = r
            print(json.dumps({name: {f"P{planes}_H{hyp}": r}}), flush=True)
            del out
        if name in stats:
            row["trace_P3_H1024"], src = _kernel_shares(stats[name])
            if a.out:
                dst = os.path.join(os.path.dirname(os.path.abspath(a.out)), f"planes_kernel_stats_{name}.csv")
                with open(src) as fi, open(dst, "w") as fo:
                    fo.write(fi.read())
        res[name] = row
        del xyz, fin
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
