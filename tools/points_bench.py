"""Point path measurement: prints one JSON line.

  operator      md_op_unproject alone on device tensors: the dense map, and the list at the ~0.58 kept share of the seeded noise
                scene (depth = exp(N(0.5, 0.6)) in [0.5, 6], conf = 1 + 2 U(0,1) >= 1.8), at 8x1536x1536 and 1x518x518: microseconds
                per call (the operator allocates and frees its scratch: the kernels' own times are in the kernel trace) and the
                fraction of the achievable HBM rate against the algorithmic bytes;
  model         md_infer_points (device in / out, graph off and on) against the bare model call: DA3 `small` bf16 at 518, Depth Pro
                bf16 at 1x1536; milliseconds per call and the ratio bare / points;
  host_route    what the call replaces: device -> host copy of depth (and confidence) + pipeline.unproject_depth.

  python tools/points_bench.py [--steps 20] [--warmup 3] [--skip-models]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-models", action="store_true")
    a = ap.parse_args(argv)
    from burn_depth_amd import ops, pipeline as P, weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, DepthProConfig, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.depth_pro import DepthPro, Device
    dev = Device(0)
    res = {"operator": {}, "model": {}, "host_route": {}}
    kw = dict(depth_min=0.5, depth_max=6.0, conf_min=1.8)
    for B, S in ((8, 1536), (1, 518)):
        rng = np.random.default_rng(7)
        d = torch.from_numpy(np.exp(rng.normal(0.5, 0.6, (B, S, S))).astype(np.float32)).cuda()
        c = torch.from_numpy((1 + 2 * rng.random((B, S, S))).astype(np.float32)).cuda()
        f = torch.full((B,), 0.9 * S, device="cuda")
        npx = B * S * S
        dense = ops.unproject(dev, d, focal_px=f, conf=c, compact=False, **kw)
        lst = ops.unproject(dev, d, focal_px=f, conf=c, dense=False, **kw)
        share = float(lst.count[-1].item()) / npx
        ms_dense = _time(lambda: ops.unproject(dev, d, focal_px=f, conf=c, compact=False, out=dense, **kw), a.steps, a.warmup)
        ms_list = _time(lambda: ops.unproject(dev, d, focal_px=f, conf=c, dense=False, out=lst, **kw), a.steps, a.warmup)
        bytes_dense = npx * (4 + 4 + 12 + 1)
        bytes_list = npx * (2 * (4 + 4) + 1 / 8 + 12 * share)
        t0 = time.perf_counter()
        P.unproject_depth(d.cpu().numpy(), focal_px=f.cpu().numpy(), conf=c.cpu().numpy(), **kw)
        host_ms = (time.perf_counter() - t0) * 1e3
        res["operator"][f"{B}x{S}x{S}"] = {
            "kept_share": round(share, 4), "dense_us": round(ms_dense * 1e3, 1), "dense_launches": 1,
            "dense_hbm_fraction": round(bytes_dense / (ms_dense * 1e-3) / HBM_ACHIEVABLE, 3),
            "list_us": round(ms_list * 1e3, 1), "list_launches": 3,
            "list_hbm_fraction": round(bytes_list / (ms_list * 1e-3) / HBM_ACHIEVABLE, 3)}
        res["host_route"][f"{B}x{S}x{S}"] = {"copy_and_numpy_ms": round(host_ms, 1)}
        del dense, lst, d, c
    if not a.skip_models:
        def model_case(name, m, S, bare):
            x = ((torch.rand(1, 3, S, S) - 0.45) / 0.225).cuda()
            out = {}
            for graph in (False, True):
                m.enable_graph(graph)
                pc = m.infer_points(x, dense=False, stride=2)
                ms_p = _time(lambda: m.infer_points(x, dense=False, stride=2, out=pc), a.steps, a.warmup)
                ms_b = _time(lambda: bare(m, x), a.steps, a.warmup)
                out["graph" if graph else "eager"] = {"points_ms": round(ms_p, 3), "bare_ms": round(ms_b, 3), "ratio": round(ms_b / ms_p, 3)}
            m.enable_graph(False)
            res["model"][name] = out

        cfg = DepthAnything3Config.small()
        cfg.precision = Precision.BF16
        m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
        depth = torch.empty((1, 518, 518), device="cuda")
        model_case("da3_small_bf16_518", m, 518, lambda mm, x: mm.infer_into(x, depth))
        m.destroy()
        cfg = DepthProConfig()
        cfg.precision = Precision.BF16
        m = DepthPro.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
        S = m.img_size()
        bufs = [torch.empty((1, S, S), device="cuda")] + [torch.empty((1,), device="cuda") for _ in range(3)]
        model_case(f"depth_pro_bf16_1x{S}", m, S, lambda mm, x: mm.infer_into(x, *bufs))
        m.destroy()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
