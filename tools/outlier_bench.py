"""Radius outlier removal measurement: prints one JSON line and writes it to profiles/outlier_bench.json.

md_op_radius_outliers alone on the two device lists of tools/voxel_bench.py: the kept list of the seeded noise scene at
8x1536x1536 and the cloud of DA3 `small` (seeded weights) at 3x518x518. Per list two radii, found by bisection on the device,
that leave about 0.9 and about 0.5 of the rows at min_neighbours = 8. Microseconds per call (the operator allocates and frees its
scratch: the kernels' own times are in a kernel trace of this tool), the algorithmic bytes (rows read by insert, fill and search,
the slot and position words written and read, 20 B per table slot reset and read, the buckets written once and read about
min_neighbours rows per search, the surviving rows written) against the achievable HBM rate, and the host route the call replaces:
device -> host copy of the list plus pipeline.radius_outliers.

  python tools/outlier_bench.py [--steps 20] [--warmup 3] [--case 8x1536] [--out profiles/outlier_bench.json]

The kernel table of DESIGN 12.7 is the raw statistics of one trace-only run per list, copied to profiles/:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/outlier_bench.py --case 8x1536 --no-host --out ""
  -> DIR/**/*_kernel_stats.csv = profiles/outlier_kernel_stats_8x1536.csv"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from voxel_bench import HBM_ACHIEVABLE, _da3_scene, _noise_scene, _time  # noqa: E402

K = 8


def _radius_for(dev, xyz, share, out):
    """bisection on the device: the radius that leaves about `share` of the rows at K neighbours"""
    import torch
    from burn_depth_amd import ops
    fin = xyz[torch.isfinite(xyz).all(1)]
    span = float((fin.max(0).values - fin.min(0).values).max())
    lo, hi = span * 2.0 ** -16, span * 2.0 ** -3  # a coarser grid than that puts every row into a few cells (cost bounds)
    for _ in range(20):
        mid = (lo * hi) ** 0.5
        ops.radius_outliers(dev, xyz, mid, K, out=out)
        if out.count[-1].item() < share * xyz.shape[0]:
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", choices=["8x1536", "da3_3x518"], default="", help="measure this list only (a kernel trace per list)")
    ap.add_argument("--no-host", action="store_true", help="skip the host route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outlier_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {}
    for name, make in (("8x1536", _noise_scene), ("da3_3x518", _da3_scene)):
        if a.case and a.case != name:
            continue
        xyz, _ = make(dev)
        n = int(xyz.shape[0])
        slots = 1024
        while slots < 2 * n:
            slots *= 2
        row = {"rows": n, "table_slots": slots, "min_neighbours": K}
        out = ops.radius_outliers(dev, xyz, 1.0, K)
        for label, share in (("most", 0.9), ("half", 0.5)):
            radius = _radius_for(dev, xyz, share, out)
            ops.radius_outliers(dev, xyz, radius, K, out=out)
            m = int(out.count[-1].item())
            ms = _time(lambda: ops.radius_outliers(dev, xyz, radius, K, out=out), a.steps, a.warmup)
            # insert reads xyz and writes the slot; alloc reads and writes 8 B per slot; fill reads xyz, slot and start, writes the
            # bucket row and the position; search reads xyz, slot, position, 27 keys and at least K bucket rows, writes neighbours;
            # scatter reads the kept rows and writes xyz and index; the table is reset (20 B per slot)
            nbytes = n * (12 + 4) + 8 * slots + n * (12 + 4 + 4 + 12 + 4) + n * (12 + 4 + 4 + 27 * 8 + K * 12 + 4) + m * (12 + 12 + 4) + 20 * slots
            r = {"radius": radius, "survivors": m, "share": round(m / n, 4), "dropped": int(out.dropped.item()), "call_us": round(ms * 1e3, 1),
                 "algorithmic_bytes": int(nbytes), "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3)}
            if not a.no_host:
                t0 = time.perf_counter()
                hx = xyz.cpu().numpy()
                t1 = time.perf_counter()
                ref = P.radius_outliers(hx, radius, K)
                t2 = time.perf_counter()
                assert int(ref.count[-1]) == m and np.array_equal(ref.neighbours, out.neighbours.cpu().numpy())
                r["host_route_ms"] = {"copy": round((t1 - t0) * 1e3, 1), "numpy": round((t2 - t1) * 1e3, 1)}
            row[label] = r
            print(json.dumps({name: {label: r}}), flush=True)
        res[name] = row
        del xyz, out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
