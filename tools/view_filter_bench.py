"""View filter measurement: prints one JSON line and writes it to profiles/view_filter_bench.json.

  operator      md_op_filter_views alone on device tensors, on synthetic views of the plane n . X = 4 with 30 % wrong depths
                (the scene of tests/test_view_filter.py) at 8x1536x1536 and 3x518x518: the percentile alone (q = 40), the
                cross-view test alone (view_rtol 0.02, min_views 1) and both; microseconds per call (the operator allocates and
                frees its scratch and waits for the stream: the kernels' own times are in the kernel trace) and the fraction of
                the achievable HBM rate against the algorithmic bytes (select: conf four times + depth once; support: depth +
                conf in, depth + support out);
  model         md_infer_points_filtered against md_infer_points on the same shape (device in / out, graph off and on): DA3
                `small` bf16 at 3x518x518; milliseconds per call and the ratio unfiltered / filtered.

  python tools/view_filter_bench.py [--steps 20] [--warmup 3] [--skip-models] [--out profiles/view_filter_bench.json]"""
import argparse
import json
import os
import sys

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


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) if axis == "x" else np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def scene(B, S, outliers=0.3, seed=11):
    """B cameras on an arc look at the plane (0.1, -0.05, 1) . X = 4 -> depth, conf, K, E as f32."""
    n = np.array([0.1, -0.05, 1.0])
    K, E = np.zeros((B, 3, 3)), np.zeros((B, 3, 4))
    depth = np.zeros((B, S, S), np.float32)
    v, u = np.mgrid[0:S, 0:S].astype(np.float64)
    for b in range(B):
        K[b] = [[0.9 * S + b, 0, S / 2 + 0.3], [0, 0.8 * S + 2 * b, S / 2 - 0.7], [0, 0, 1]]
        R = _rot("y", 0.06 * (b - (B - 1) / 2)) @ _rot("x", 0.03 * b)
        t = np.array([0.25 * (b - (B - 1) / 2), 0.05 * b, 0.1 * b])
        E[b, :, :3], E[b, :, 3] = R, t
        rn = R @ n
        depth[b] = (4.0 + rn @ t) / (rn[0] * (u - K[b, 0, 2]) / K[b, 0, 0] + rn[1] * (v - K[b, 1, 2]) / K[b, 1, 1] + rn[2])
    rng = np.random.default_rng(seed)
    bad = rng.random((B, S, S)) < outliers
    depth = np.where(bad, depth * np.where(rng.random((B, S, S)) < 0.5, 0.7, 1.35), depth).astype(np.float32)
    conf = (1 + 2 * rng.random((B, S, S))).astype(np.float32)
    return depth, conf, K.astype(np.float32), E.astype(np.float32)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_filter_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.depth_pro import Device
    dev = Device(0)
    res = {"operator": {}, "model": {}}
    for B, S in ((8, 1536), (3, 518)):
        d, c, K, E = (torch.from_numpy(t).cuda() for t in scene(B, S))
        npx = B * S * S
        bytes_select, bytes_support = npx * (4 * 4 + 4), npx * (4 + 4 + 4 + 1)
        row = {}
        for name, kw, nbytes, launches in (("percentile", dict(conf_percentile=40), bytes_select + bytes_support, 10),
                                           ("views", dict(view_rtol=0.02, min_views=1), bytes_support, 2),
                                           ("both", dict(conf_percentile=40, view_rtol=0.02, min_views=1), bytes_select + bytes_support, 10)):
            out = dict(zip(("depth", "support", "tau", "kept"), ops.filter_views(dev, d, c, intrinsics=K, extrinsics=E, **kw)))
            ms = _time(lambda: ops.filter_views(dev, d, c, intrinsics=K, extrinsics=E, out=out, **kw), a.steps, a.warmup)
            row[name] = {"us": round(ms * 1e3, 1), "launches": launches, "kept_share": round(float(out["kept"][-1].item()) / npx, 4),
                         "algorithmic_mb": round(nbytes / 1e6, 1), "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_ACHIEVABLE, 3)}
        res["operator"][f"{B}x{S}x{S}"] = row
        del d, c
    if not a.skip_models:
        cfg = DepthAnything3Config.small()
        cfg.precision, cfg.max_batch = Precision.BF16, 3
        m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
        x = ((torch.rand(3, 3, 518, 518) - 0.45) / 0.225).cuda()
        fkw = dict(conf_percentile=40, view_rtol=0.02, min_views=1)
        out = {}
        for graph in (False, True):
            m.enable_graph(graph)
            plain = m.infer_points(x, dense=False, world=True)
            filt = m.infer_points(x, dense=False, world=True, **fkw)
            ms_p = _time(lambda: m.infer_points(x, dense=False, world=True, out=plain), a.steps, a.warmup)
            ms_f = _time(lambda: m.infer_points(x, dense=False, world=True, out=filt, **fkw), a.steps, a.warmup)
            out["graph" if graph else "eager"] = {"points_ms": round(ms_p, 3), "filtered_ms": round(ms_f, 3), "ratio": round(ms_p / ms_f, 3),
                                                  "extra_us": round((ms_f - ms_p) * 1e3, 1)}
        m.enable_graph(False)
        m.destroy()
        res["model"]["da3_small_bf16_3x518"] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
