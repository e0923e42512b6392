"""What the point-path test files share (test_points, test_view_filter, test_points_normals, test_voxel_thin, test_points_voxel):
the library / device fixtures, bit-pattern and tensor helpers, seeded cameras, the reduced models and the cloud comparisons.
A plain module, imported like close_check.py; scene builders stay in the file that owns them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402

f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _t(a):
    """numpy -> a device tensor; always a contiguous copy (the shared scenes are read-only)"""
    return torch.from_numpy(np.array(a, order="C")).cuda() if a is not None else None


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _cameras(rng, B, H, W):
    K = np.zeros((B, 3, 3), f32)
    E = np.zeros((B, 3, 4), f32)
    for b in range(B):
        K[b] = [[0.9 * W + b, 0, W / 2 + 0.3], [0, 0.8 * W + 2 * b, H / 2 - 0.7], [0, 0, 1]]
        E[b, :, :3] = _rotation(rng)
        E[b, :, 3] = rng.uniform(-2, 2, 3)
    return K, E


def _da3(dev, variant="tiny_dual", precision="BF16", max_batch=2):
    """Depth-Anything-v3 at a reduced preset (70 x 70): "tiny" (mono) or "tiny_dual" (confidence and a camera decoder)"""
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = {"tiny": DepthAnything3Config.tiny_test, "tiny_dual": DepthAnything3Config.tiny_dual_test}[variant]()
    cfg.max_batch, cfg.precision = max_batch, getattr(Precision, precision)
    return DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _pro(dev, preset="tiny", precision="BF16", max_batch=2):
    """Depth Pro at the "tiny" or the "small" preset (128-pixel windows); both take a 512 x 512 input"""
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthProConfig, Precision
    from burn_depth_amd.depth_pro import DepthPro
    cfg = {"tiny": DepthProConfig.tiny_test, "small": DepthProConfig.small_test}[preset]()
    cfg.max_batch, cfg.precision = max_batch, getattr(Precision, precision)
    return DepthPro.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _image(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, S, S, generator=g) - 0.45) / 0.225


def _cloud_np(pc):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(pc).items()}


def _same_cloud(a, b, what="", normals=False):
    """b holds what a holds, bit for bit: the dense maps (and the depth where both carry one), then the list rows that are
    points. normals=True: the normal outputs too, and the dense maps must then be present on both sides."""
    for k in ("count", "mask", "point_map", "depth") + (("normal_map",) if normals else ()):
        if normals and k != "depth":
            assert a[k] is not None and b[k] is not None, (what, k)
        if a[k] is not None and b.get(k) is not None:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)
    n = min(int(a["count"][-1]), a["xyz"].shape[0])
    for k in ("xyz", "rgb", "conf") + (("normals",) if normals else ()):
        if a[k] is not None:
            assert b[k] is not None and np.array_equal(a[k][:n].view(np.uint8), b[k][:n].view(np.uint8)), (what, k)


def _da3_subset(m, x):
    """md_da3_infer_ex with the outputs the md_infer_points* entries ask the model for: depth, confidence, extrinsics, intrinsics."""
    B, _, H, W = x.shape
    f = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")  # noqa: E731
    depth, conf, extr, intr = f(B, H, W), f(B, H, W), f(B, 1, 3, 4), f(B, 1, 3, 3)
    o = _lib.MdDa3Outputs(depth.data_ptr(), conf.data_ptr(), None, None, None, extr.data_ptr(), intr.data_ptr())
    _lib.check(_lib.load().md_da3_infer_ex(m._h, C.c_void_p(x.data_ptr()), B, H, W, _lib.MD_MEM_DEVICE, C.byref(o), _lib.MD_MEM_DEVICE,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return depth, conf, extr, intr
