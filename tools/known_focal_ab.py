"""A/B of DepthPro::infer with the FOV network (plain) against the call with a known focal length (no FOV encoder / head), on the
default configuration in bf16 with device memory, at [8,3,1536,1536] and at B = 1. One process, one model; blocks of timed steps
alternate between the two forms (the order flips every block), each block behind its own warm-up, HIP events around
device-synchronised steps. Prints one JSON line.

  python tools/known_focal_ab.py [--blocks 6] [--steps 10] [--warmup 3] [--out profiles/known_focal_ab.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_block(step, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        step()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / steps


def ab(model, B: int, blocks: int, steps: int, warmup: int) -> dict:
    S = model.img_size()
    torch.manual_seed(0)
    x = torch.randn(B, 3, S, S, device="cuda")
    depth = torch.empty(B, S, S, device="cuda")
    focal, fovx, fovy = (torch.empty(B, device="cuda") for _ in range(3))
    model.infer_into(x, depth, focal, fovx, fovy)
    torch.cuda.synchronize()
    f_px = focal.clone()  # the predicted focal lengths: both forms compute the same depth
    forms = {"plain": lambda: model.infer_into(x, depth, focal, fovx, fovy),
             "known_focal": lambda: model.infer_into(x, depth, focal, fovx, fovy, f_px=f_px)}
    ms = {k: [] for k in forms}
    for i in range(blocks):
        order = ("plain", "known_focal") if i % 2 == 0 else ("known_focal", "plain")
        for k in order:
            ms[k].append(time_block(forms[k], steps, warmup))
    out = {"B": B, "image": S, "blocks": blocks, "steps_per_block": steps}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"ms_per_step": round(med, 4), "frames_per_s": round(B * 1000.0 / med, 3),
                  "block_ms": [round(t, 4) for t in v], "spread": round((max(v) - min(v)) / med, 5)}
    out["known_over_plain_frames_per_s"] = round(out["known_focal"]["frames_per_s"] / out["plain"]["frames_per_s"], 5)
    out["ms_saved_per_step"] = round(out["plain"]["ms_per_step"] - out["known_focal"]["ms_per_step"], 4)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthProConfig, Precision
    from burn_depth_amd.depth_pro import DepthPro, Device
    cfg = DepthProConfig()
    cfg.precision = Precision.BF16
    cfg.max_batch = 8
    model = DepthPro.new(Device(0), cfg, seed=0, init_scheme=Wt.INIT_PARITY)
    res = {"metric": "known_focal_ab", "precision": "bf16", "memory": "device",
           "device": torch.cuda.get_device_name(0),
           "runs": [ab(model, B, a.blocks, a.steps, a.warmup) for B in (8, 1)]}
    model.destroy()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
