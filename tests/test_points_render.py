"""Model -> cloud -> rendered images in one call: `infer_points(render=...)` (md_infer_points_render) against
`ops.render_points` (md_op_render_points) applied to the list of the same call without rendering (md_infer_points_voxel).
include/mi_depth.h states the contract, DESIGN 12.4 the kernels. Every comparison is bit for bit. Runs with `-m gpu` on an MI355X."""
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
from points_util import _da3, _image, _pro, _t, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
FIELDS = ("depth", "index", "rgb", "filled")


def _rgb(B, S):
    return torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()


def _list(pc):
    """the rows of a PointCloud that hold points, on the host"""
    torch.cuda.synchronize()
    n = min(int(pc.count[-1]), int(pc.xyz.shape[0]))
    return pc.xyz[:n].cpu().numpy(), n


def _targets_at(xyz, T, H, W, seed=0):
    """T seeded cameras that look at the centroid of `xyz` from twice its extent away, each with its own yaw and pitch"""
    rng = np.random.default_rng(seed)
    c = xyz.mean(0).astype(np.float64)
    d = 2.0 * float(np.linalg.norm(xyz - c, axis=1).max()) + 1e-3
    K, E = np.zeros((T, 3, 3), f32), np.zeros((T, 3, 4), f32)
    for j in range(T):
        a, b = rng.uniform(-0.4, 0.4, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Ry @ Rx
        K[j] = [[0.9 * W + j, 0, W / 2 + 0.3], [0, 0.8 * W + 2 * j, H / 2 - 0.7], [0, 0, 1]]
        E[j, :, :3], E[j, :, 3] = R, np.array([0, 0, d]) - R @ c
    return _t(K), _t(E)


def _np(r):
    torch.cuda.synchronize()
    return {k: (getattr(r, k).cpu().numpy() if getattr(r, k) is not None else None) for k in FIELDS}


def _same(got, want, what=""):
    for k in FIELDS:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k)


def _expect(dev, full, render):
    """ops.render_points on the list of the call without rendering, with its device count word"""
    from burn_depth_amd import ops
    return _np(ops.render_points(dev, full.xyz, rgb=full.rgb, count=full.count[-1:], **render))


def test_da3_two_views_rendered_equals_rendering_the_list(dev):
    m = _da3(dev)
    try:
        x, rgb = _image(2, 70).cuda(), _rgb(2, 70)
        forms = (dict(world=True, rgb=rgb, **OPTS), dict(world=True, rgb=rgb, conf_percentile=30, voxel=None, **OPTS), dict(world=True, **OPTS))
        for i, kw in enumerate(forms):
            full = m.infer_points(x, **dict(kw, voxel=0.0))
            xyz, n = _list(full)
            assert n > 300
            if "voxel" in kw:  # a voxel that leaves about a third of the filtered list
                kw["voxel"] = float(np.ptp(xyz, axis=0).max()) / 12
                full = m.infer_points(x, **kw)
                xyz, thinned = _list(full)
                assert 0 < thinned < n and full.index is not None
            for (H, W), radius in (((70, 70), 0), ((48, 64), 1)):
                K, E = _targets_at(xyz, 2, H, W)
                render = dict(H=H, W=W, intrinsics=K, extrinsics=E, pixel_offset=0.5, radius=radius)
                want = _expect(dev, full, render)
                assert (want["filled"][:2] > 20).all() and (want["rgb"] is None) == ("rgb" not in kw)
                got = m.infer_points(x, render=render, **kw)
                _same(_np(got.render), want, (i, H, W))
                rows = len(xyz)  # the cloud is the one of the call without rendering
                assert torch.equal(got.count, full.count) and torch.equal(got.xyz[:rows], full.xyz[:rows]) and torch.equal(got.depth, full.depth)
    finally:
        m.destroy()


def test_depth_pro_camera_frame(dev):
    m = _pro(dev, "tiny")
    try:
        x = _image(2, 512).cuda()
        kw = dict(dense=False, **OPTS)
        full = m.infer_points(x, **kw)
        xyz, n = _list(full)
        assert n > 1000
        H, W = 48, 64
        with np.errstate(all="ignore"):
            reach = np.percentile(np.abs(xyz[:, :2] / xyz[:, 2:]), 90)
        render = dict(H=H, W=W, focal_px=torch.tensor([0.4 * H / reach], device="cuda"), radius=1)  # extrinsics None: p = X
        want = _expect(dev, full, render)
        assert want["filled"][0] > 100 and want["rgb"] is None
        _same(_np(m.infer_points(x, render=render, **kw).render), want, "depth pro")
    finally:
        m.destroy()


FILL = dict(point_map=123456.0, mask=77, xyz=123456.0, rgb=77, conf=123456.0, count=-7, depth=123456.0, r_depth=123456.0, r_index=-7, r_rgb=77,
            r_filled=-7)
CANARY = 64  # elements behind the end of every rendered output


def _buffers(B, S, cap, T, H, W, host):
    """Poisoned outputs of one call (the rendered ones with a canary tail), numpy (host) or device tensors"""
    f, u8, i32 = np.float32, np.uint8, np.int32
    shapes = dict(point_map=((B, S, S, 3), f), mask=((B, S, S), u8), xyz=((cap, 3), f), rgb=((cap, 3), u8), conf=((cap,), f),
                  count=((B + 1,), i32), depth=((B, S, S), f), r_depth=((T * H * W + CANARY,), f), r_index=((T * H * W + CANARY,), i32),
                  r_rgb=((T * H * W * 3 + CANARY,), u8), r_filled=((T + 1 + CANARY,), i32))
    t = {k: np.full(shape, FILL[k], dt) for k, (shape, dt) in shapes.items()}
    if not host:
        t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
    outs = _lib.MdPointsOutputs(ptr("point_map"), ptr("mask"), ptr("xyz"), ptr("rgb"), ptr("conf"), ptr("count"), cap, ptr("depth"))
    routs = _lib.MdRenderOutputs(ptr("r_depth"), ptr("r_index"), ptr("r_rgb"), ptr("r_filled"))
    return t, outs, routs


def _read(t):
    torch.cuda.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}


def _same_bytes(a, b, what, keys=None):
    n = min(int(a["count"][-1]), a["xyz"].shape[0])
    assert n > 0, what
    for k in keys or a:
        rows = n if k in ("xyz", "rgb", "conf") else None
        assert np.array_equal(a[k][:rows].view(np.uint8), b[k][:rows].view(np.uint8)), (what, k)
    return n


def _call(m, entry, x, rgb, host, T, H, W, cams, render=True):
    """md_infer_points_voxel or md_infer_points_render through ctypes, everything in host or in device memory -> outputs"""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    B, S = x.shape[0], x.shape[2]
    t, outs, routs = _buffers(B, S, B * 35 * 35, T, H, W, host)
    o = _points_opts(world=True, **OPTS)
    kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
    p = lambda a: C.c_void_p(a.ctypes.data if host else a.data_ptr())  # noqa: E731
    xin, cin = (x.cpu().numpy(), rgb.cpu().numpy()) if host else (x, rgb)
    K, E = (c.cpu().numpy() if host else c for c in cams)
    rnd = _lib.MdPointsRender(T, H, W, _lib.MdPointsCameras(p(K).value, p(E).value, None), _lib.MdRenderOpts(0.5, 0.0, 0.0, 1), routs)
    st = None if host else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (m._h, p(xin), B, S, S, kind, p(cin), None, None, C.byref(o), C.byref(outs), None, None)
    if entry == "voxel":
        _lib.check(lib.md_infer_points_voxel(*head, kind, st))
    else:
        _lib.check(lib.md_infer_points_render(*head, C.byref(rnd) if render else None, kind, st))
    return _read(t)


def test_null_render_is_the_voxel_entry(dev):
    m = _da3(dev)
    try:
        x, rgb = _image(2, 70).cuda(), _rgb(2, 70)
        cams = _targets_at(np.zeros((2, 3), f32), 1, 8, 8)
        m.enable_timing(True)
        names = {}
        outs = {}
        for entry in ("voxel", "render"):
            m.read_timing()
            outs[entry] = _call(m, entry, x, rgb, False, 1, 8, 8, cams, render=False)
            names[entry] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["voxel"] == names["render"] and "points_unproject" in names["voxel"] and "points_render" not in names["render"]
        _same_bytes(outs["voxel"], outs["render"], "rnd NULL")
        for k in ("r_depth", "r_index", "r_rgb", "r_filled"):
            assert (outs["render"][k] == np.asarray(FILL[k], outs["render"][k].dtype)).all(), k
    finally:
        m.destroy()


def test_host_in_host_out_equals_device(dev):
    m = _da3(dev)
    try:
        x, rgb = _image(2, 70).cuda(), _rgb(2, 70)
        xyz, _ = _list(m.infer_points(x, world=True, **OPTS))
        T, H, W = 2, 48, 64
        cams = _targets_at(xyz, T, H, W)
        on_device = _call(m, "render", x, rgb, False, T, H, W, cams)
        on_host = _call(m, "render", x, rgb, True, T, H, W, cams)
        n = _same_bytes(on_device, on_host, "host against device")
        assert (on_host["r_filled"][:T] > 20).all() and on_host["r_filled"][T] == on_host["r_filled"][:T].sum()
        assert (on_host["xyz"][n:] == f32(FILL["xyz"])).all()
        for k, used in (("r_depth", T * H * W), ("r_index", T * H * W), ("r_rgb", T * H * W * 3), ("r_filled", T + 1)):
            for side in (on_host, on_device):  # nothing behind the images is written
                assert (side[k][used:] == np.asarray(FILL[k], side[k].dtype)).all(), k
        assert (on_host["r_index"][:T * H * W] >= -1).all() and on_host["r_index"][:T * H * W].max() < n
    finally:
        m.destroy()


def test_graph_replay_and_allocations(dev):
    m = _da3(dev)
    try:
        x, rgb = _image(2, 70).cuda(), _rgb(2, 70)
        kw = dict(world=True, rgb=rgb, conf_min=1.0, **OPTS)
        full = m.infer_points(x, **kw)
        xyz, n = _list(full)
        K, E = _targets_at(xyz, 2, 48, 64)
        render = dict(H=48, W=64, intrinsics=K, extrinsics=E, pixel_offset=0.5, radius=1)
        want = _expect(dev, full, render)
        assert (want["filled"][:2] > 20).all()
        _same(_np(m.infer_points(x, render=render, **kw).render), want, "eager")
        m.enable_graph(True)
        out = m.infer_points(x, render=render, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (1, 2, 3, 4):  # capture, then replays: the keys are cleared inside the graph
            out.render.depth.fill_(123456.0)
            out.render.index.fill_(-7)
            out.render.filled.fill_(-7)
            out = m.infer_points(x, out=out, render=render, **kw)
            _same(_np(out.render), want, f"graph call {call}")
        # another radius on the same pointers: its own graph and its own result
        render2 = dict(render, radius=0)
        want2 = _expect(dev, full, render2)
        assert want2["filled"][-1] < want["filled"][-1]
        for _ in range(3):
            out = m.infer_points(x, out=out, render=render2, **kw)
        _same(_np(out.render), want2, "radius 0")
        for _ in range(2):
            m.infer_points(x, out=out, render=render, **kw)
            m.infer_points(x, out=out, render=render2, **kw)
        _same(_np(out.render), want2, "after the loop")
        assert m.query("allocs") == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


def test_rendering_needs_the_list(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        K, E = _targets_at(np.zeros((2, 3), f32), 1, 8, 8)
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, compact=False, world=True, render=dict(H=8, W=8, intrinsics=K, extrinsics=E))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG and "`xyz` and `count`" in e.value.message
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, world=True, render=dict(H=8, W=8, intrinsics=K, extrinsics=E, radius=17))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG and "radius" in e.value.message
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, world=True, render=dict(H=0, W=8, intrinsics=K, extrinsics=E))
        assert e.value.code == _lib.MD_ERR_SHAPE
    finally:
        m.destroy()
