"""Multi-view Depth-Anything-v3 `small` measurement: writes profiles/da3_views_bench.json and prints it.

For bf16 and f16x2 at 518 x 518 and V = 2, 4, 8 views of one scene, device in / out, graph off and on:

  views_ms      md_da3_infer_views on 1 x V views (cross-view attention in the global blocks);
  batch_ms      md_da3_infer_ex on the same V images as a batch: the same work minus the cross-view keys;
  ratio         views_ms / batch_ms;
  attention     from the per-launch timing of an eager call: the milliseconds of the cross-view attention launches
                (`attention_views`), of the per-view attention launches, and their share of all kernel time.

  python tools/da3_views_bench.py [--steps 20] [--warmup 5] [--out profiles/da3_views_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "da3_views_bench.json"))
    a = ap.parse_args(argv)
    from burn_depth_amd import _lib, weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.depth_pro import Device
    dev, lib = Device(0), _lib.load()
    S = 518
    res = {"size": S, "steps": a.steps, "warmup": a.warmup, "runs": []}
    for pname, prec in (("bf16", Precision.BF16), ("f16x2", Precision.F16X2)):
        for V in a.views:
            cfg = DepthAnything3Config.small()
            cfg.precision, cfg.max_batch = prec, V
            model = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
            if prec == Precision.F16X2:
                model.round_weights_to_f16()
            torch.manual_seed(1)
            x = torch.randn(V, 3, S, S, device="cuda")
            ah = 8 * (S // cfg.patch_size)
            f = lambda *s: torch.empty(s, device="cuda")  # noqa: E731
            bufs = [f(V, S, S), f(V, S, S), f(V, cfg.aux_output_dim - 1, ah, ah), f(V, ah, ah), f(V, 1, 9), f(V, 1, 3, 4), f(V, 1, 3, 3)]
            o = _lib.MdDa3Outputs(*(t.data_ptr() for t in bufs))
            views = lambda: _lib.check(lib.md_da3_infer_views(model._h, C.c_void_p(x.data_ptr()), 1, V, S, S, _lib.MD_MEM_DEVICE, C.byref(o), _lib.MD_MEM_DEVICE, None))  # noqa: E731
            batch = lambda: _lib.check(lib.md_da3_infer_ex(model._h, C.c_void_p(x.data_ptr()), V, S, S, _lib.MD_MEM_DEVICE, C.byref(o), _lib.MD_MEM_DEVICE, None))  # noqa: E731
            run = {"precision": pname, "views": V}
            for gname, graph in (("eager", False), ("graph", True)):
                model.enable_graph(graph)
                tv, tb = _time(views, a.steps, a.warmup), _time(batch, a.steps, a.warmup)
                run[gname] = {"views_ms": round(tv, 4), "batch_ms": round(tb, 4), "ratio": round(tv / tb, 4)}
            model.enable_graph(False)
            model.enable_timing(True)
            views()
            tm = model.read_timing()
            model.enable_timing(False)
            tot = sum(v[0] for v in tm.values())
            av, ap_ = tm.get("attention_views", (0.0, 0)), tm.get("attention", (0.0, 0))
            run["attention"] = {"views_launches": int(av[1]), "views_ms": round(av[0], 4), "per_view_launches": int(ap_[1]), "per_view_ms": round(ap_[0], 4),
                                "kernel_ms": round(tot, 4), "views_share": round(av[0] / tot, 4), "all_attention_share": round((av[0] + ap_[0]) / tot, 4)}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            model.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
