"""Frames per second of the frame path on DA3 `small` at 518 (the viewer's default model): a seeded 1920x1080 uint8 frame through

  host      the host numpy pipeline (pipeline.prepare_depth_anything3_image -> rgb_to_input_tensor -> infer -> depth_to_u8 with
            the restore to 1920x1080), today's CLI path;
  frame_host       md_process_frame from a host frame (pinned staging, u8 display restored to the frame's size);
  frame_dev        md_process_frame from a device frame, eager;
  frame_dev_graph  the same with graph replay;

beside the bare model step md_da3_infer on a device input of 518x518 (eager and graph). Prints one JSON line (and writes it to
--out when given).

  python tools/frame_bench.py [--iters 200] [--warmup 20] [--precision bf16] [--out profiles/frame_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--precision", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--only-device", action="store_true", help="run the device-frame path alone (for a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch
    from burn_depth_amd import pipeline as P, weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.depth_pro import Device
    from burn_depth_amd.inference import rgb_to_input_tensor

    dev = Device(0)
    cfg = DepthAnything3Config.small()
    cfg.precision = Precision.BF16 if a.precision == "bf16" else Precision.F32
    m = DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    rgb = np.random.default_rng(0).integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    t = m.img_size()

    def fps(step, iters, warmup):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return iters / (time.perf_counter() - t0)

    res = {"metric": "frame_path_fps", "model": "da3-small", "precision": a.precision, "frame": [1920, 1080], "target": t}
    dframe = torch.from_numpy(rgb).cuda()
    kw = dict(target=0, restore=True, normalize=True, fmt="u8", prepared=False)
    if a.only_device:
        out = m.process_frame(dframe, **kw)
        res["frame_dev"] = fps(lambda: m.process_frame(dframe, out=out, **kw), a.iters, a.warmup)
    else:
        def host_step():
            prep = P.prepare_depth_anything3_image(rgb, t)
            d = m.infer(rgb_to_input_tensor(prep.rgb.tobytes(), t, t, dev)).depth
            P.depth_to_u8(d.cpu().numpy(), prep.crop, (1920, 1080))
        res["host"] = fps(host_step, a.host_iters, 1)
        out = m.process_frame(rgb, **kw)
        res["frame_host"] = fps(lambda: m.process_frame(rgb, out=out, **kw), a.iters, a.warmup)
        out = m.process_frame(dframe, **kw)
        res["frame_dev"] = fps(lambda: m.process_frame(dframe, out=out, **kw), a.iters, a.warmup)
        x = torch.randn(1, 3, t, t, device="cuda")
        depth = torch.empty(1, t, t, device="cuda")
        res["bare_da3_infer"] = fps(lambda: m.infer_into(x, depth), a.iters, a.warmup)
        m.enable_graph(True)
        res["frame_dev_graph"] = fps(lambda: m.process_frame(dframe, out=out, **kw), a.iters, a.warmup)
        res["bare_da3_infer_graph"] = fps(lambda: m.infer_into(x, depth), a.iters, a.warmup)
        m.enable_graph(False)
        res["frame_dev_graph_vs_bare_graph"] = res["frame_dev_graph"] / res["bare_da3_infer_graph"]
        res["frame_dev_vs_bare"] = res["frame_dev"] / res["bare_da3_infer"]
    res["gpu"] = torch.cuda.get_device_name(0)
    m.destroy()
    line = json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
