"""The mesh rasterised inside the model call: `infer_points(mesh=, raster=)` (md_infer_points_raster) against `ops.render_mesh` on the
list and the faces of the call without `raster`. include/mi_depth.h states the contract, DESIGN 12.6 the kernels. Selection on
integer coverage: every comparison is bit for bit. Runs with `-m gpu` on an MI355X."""
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
from points_util import _bits, _da3, _image, _pro, _t, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
FIELDS = ("depth", "face", "rgb", "filled", "skipped")
TH, TW = 48, 64


def _cams(pc, T):
    """T seeded cameras that look at the centroid of the cloud from twice the distance four fifths of its points lie within, each
    with its own yaw and pitch -> K, E. (The reduced models' clouds have far outliers: what a test needs is some filled pixels.)"""
    rng = np.random.default_rng(0)
    xyz = pc.xyz[:int(pc.count[-1])].cpu().numpy()
    c = xyz.mean(0).astype(np.float64)
    d = 2.0 * float(np.percentile(np.linalg.norm(xyz - c, axis=1), 80)) + 1e-3
    K, E = np.zeros((T, 3, 3), f32), np.zeros((T, 3, 4), f32)
    for j in range(T):
        a, b = rng.uniform(-0.4, 0.4, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Ry @ Rx
        K[j] = [[0.9 * TW + j, 0, TW / 2 + 0.3], [0, 0.8 * TW + 2 * j, TH / 2 - 0.7], [0, 0, 1]]
        E[j, :, :3], E[j, :, 3] = R, np.array([0, 0, d]) - R @ c
    return K, E


def _target(pc, T=1):
    K, E = _cams(pc, T)
    return dict(H=TH, W=TW, intrinsics=_t(K), extrinsics=_t(E))


def _same_raster(got, want, what=""):
    torch.cuda.synchronize()
    for k in FIELDS:
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            assert torch.equal(g, w), (what, k)


def _op(dev, plain, target, **kw):
    """ops.render_mesh on the list and the faces of a call without `raster`, with the call's own device count word"""
    from burn_depth_amd import ops
    return ops.render_mesh(dev, plain.xyz, plain.faces, target["H"], target["W"], target["intrinsics"], target["extrinsics"], rgb=plain.rgb,
                           face_count=plain.face_count[-1:], **kw)


def test_da3_raster_equals_the_operator_on_the_calls_mesh(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        rgb = torch.randint(0, 256, (2, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, mesh=dict(max_rtol=0.2), **OPTS)
        plain = m.infer_points(x, **kw)
        for T, opts in ((1, dict()), (3, dict(cull=1, max_extent=20, pixel_offset=0.5))):
            target = _target(plain, T)
            want = _op(dev, plain, target, **opts)
            got = m.infer_points(x, raster=dict(target, **opts), **kw)
            _same_raster(got.raster, want, (T, opts))
            filled = want.filled.tolist()
            print(f"da3 raster T={T} {opts}: filled {filled}, skipped {want.skipped.tolist()}, {int(plain.face_count[-1])} faces")
            assert filled[-1] > 0 and got.raster.rgb is not None
            rows = min(int(plain.count[-1]), len(plain.xyz))  # the cloud and the mesh are those of the call without raster
            assert torch.equal(got.count, plain.count) and torch.equal(got.xyz[:rows], plain.xyz[:rows])
            assert torch.equal(got.face_count, plain.face_count) and torch.equal(got.faces[:int(plain.face_count[-1])], plain.faces[:int(plain.face_count[-1])])
    finally:
        m.destroy()


def test_depth_pro_raster_beside_rendering(dev):
    m = _pro(dev, "tiny")
    try:
        x = _image(2, 512).cuda()
        kw = dict(dense=False, mesh=dict(max_rtol=0.05), **OPTS)
        plain = m.infer_points(x, **kw)
        target = _target(plain)
        want = _op(dev, plain, target)
        got = m.infer_points(x, raster=target, **kw)
        _same_raster(got.raster, want, "depth pro")
        assert int(want.filled[-1]) > 0 and got.raster.rgb is None
        # beside render=: the point images are those of the call without raster, the raster that of the call without render
        render = dict(target, radius=1)
        only = m.infer_points(x, render=render, **kw)
        both = m.infer_points(x, render=render, raster=target, **kw)
        _same_raster(both.raster, want, "with render")
        for k in ("depth", "index", "filled"):
            assert torch.equal(getattr(both.render, k), getattr(only.render, k)), k
        print(f"depth pro: mesh fills {int(want.filled[-1])} pixels, points at radius 1 {int(only.render.filled[-1])}")
    finally:
        m.destroy()


FILL = dict(xyz=123456.0, count=-7, faces=-7, face_count=-7, depth=123456.0, face=-7, filled=-7, skipped=-7)
CANARY = 64


def _call(m, entry, x, host, cams, rst=True, thin=0.0, faces=True, xyz=True, cull=0, max_extent=0, z_near=0.0, T=2):
    """md_infer_points_mesh or md_infer_points_raster through ctypes, everything in host or in device memory -> (rc, outputs);
    cams: K [T,3,3], E [T,3,4] of the targets; the raster outputs lie between canaries"""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    B, S = x.shape[0], x.shape[2]
    cap, fcap, px = B * 35 * 35, 2 * B * 34 * 34, T * TH * TW
    shapes = dict(xyz=((cap, 3), f32), count=((B + 1,), np.int32), faces=((fcap, 3), np.int32), face_count=((B + 1,), np.int32),
                  depth=((px + 2 * CANARY,), f32), face=((px + 2 * CANARY,), np.int32), filled=((T + 1 + 2 * CANARY,), np.int32),
                  skipped=((T + 1 + 2 * CANARY,), np.int32))
    t = {k: np.full(shape, FILL[k], dt) for k, (shape, dt) in shapes.items()}
    K, E = (np.ascontiguousarray(a) for a in cams)
    if not host:
        t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
        K, E = torch.from_numpy(K).cuda(), torch.from_numpy(E).cuda()
    ptr = lambda v, skip=0: (v.ctypes.data if host else v.data_ptr()) + 4 * skip  # noqa: E731
    outs = _lib.MdPointsOutputs(None, None, ptr(t["xyz"]) if xyz else None, None, None, ptr(t["count"]), cap, None)
    g = _lib.MdPointsMesh(0.2, ptr(t["faces"]) if faces else None, ptr(t["face_count"]), fcap, None)
    r = _lib.MdPointsRaster(T, TH, TW, _lib.MdPointsCameras(ptr(K), ptr(E), None), _lib.MdRasterOpts(0.5, z_near, 0.0, cull, max_extent),
                            _lib.MdRasterOutputs(ptr(t["depth"], CANARY), ptr(t["face"], CANARY), None, ptr(t["filled"], CANARY),
                                                 ptr(t["skipped"], CANARY)))
    vox = _lib.MdPointsVoxel(thin, None, None, None)
    o = _points_opts(world=True, **OPTS)
    kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
    xin = x.cpu().numpy() if host else x
    st = None if host else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (m._h, C.c_void_p(xin.ctypes.data if host else xin.data_ptr()), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None,
            C.byref(vox) if thin else None, None, C.byref(g))
    if entry == "mesh":
        rc = lib.md_infer_points_mesh(*head, kind, st)
    else:
        rc = lib.md_infer_points_raster(*head, C.byref(r) if rst else None, kind, st)
    torch.cuda.synchronize()
    return rc, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}


RASTER = ("depth", "face", "filled", "skipped")


def test_null_raster_is_the_mesh_entry(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        cams = _cams(m.infer_points(x, world=True, **OPTS), 2)
        m.enable_timing(True)
        names, outs = {}, {}
        for entry in ("mesh", "raster", "with"):
            m.read_timing()
            rc, outs[entry] = _call(m, "mesh" if entry == "mesh" else "raster", x, False, cams, rst=entry == "with")
            assert rc == _lib.MD_OK
            names[entry] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["mesh"] == names["raster"] and "points_mesh" in names["raster"] and "points_raster" not in names["raster"]
        assert names["with"][-1] == "points_raster" and names["with"][:-1] == names["mesh"]
        for k in outs["mesh"]:
            assert np.array_equal(outs["mesh"][k].view(np.uint8), outs["raster"][k].view(np.uint8)), k
        for k in RASTER:
            assert (outs["raster"][k] == np.asarray(FILL[k], outs["raster"][k].dtype)).all(), k
        for k in ("xyz", "count", "faces", "face_count"):
            assert np.array_equal(outs["mesh"][k].view(np.uint8), outs["with"][k].view(np.uint8)), k
        assert outs["with"]["filled"][CANARY + 2] > 0
    finally:
        m.destroy()


def test_host_in_host_out_equals_device_between_canaries(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        cams = _cams(m.infer_points(x, world=True, **OPTS), 2)
        rc, on_device = _call(m, "raster", x, False, cams, max_extent=30)
        assert rc == _lib.MD_OK
        rc, on_host = _call(m, "raster", x, True, cams, max_extent=30)
        assert rc == _lib.MD_OK
        px = 2 * TH * TW
        for t in (on_device, on_host):
            for k, used in (("depth", px), ("face", px), ("filled", 3), ("skipped", 3)):
                fill = np.asarray(FILL[k], t[k].dtype)
                assert (t[k][:CANARY] == fill).all() and (t[k][CANARY + used:] == fill).all(), k
        for k in RASTER + ("count", "face_count"):
            assert np.array_equal(on_host[k].view(np.uint8), on_device[k].view(np.uint8)), k
        filled = on_device["filled"][CANARY:CANARY + 3]
        assert filled[2] == filled[:2].sum() > 0 and (on_device["face"][CANARY:CANARY + px] >= 0).sum() == filled[2]
    finally:
        m.destroy()


def test_graph_replay_and_allocations(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, conf_min=1.0, mesh=dict(max_rtol=0.2), **OPTS)
        plain = m.infer_points(x, **kw)
        target = _target(plain, 2)
        want = {c: _op(dev, plain, target, cull=c) for c in (0, 1)}
        torch.cuda.synchronize()
        assert 0 < int(want[1].filled[-1]) <= int(want[0].filled[-1])
        m.enable_graph(True)
        out = m.infer_points(x, raster=dict(target, cull=0), **kw)  # call 1 of this key (fresh output pointers): eager
        _same_raster(out.raster, want[0], "eager")
        allocs = m.query("allocs")
        for call in (1, 2, 3, 4):  # capture, then replays
            for k in ("depth", "face", "filled", "skipped"):
                getattr(out.raster, k).fill_(-7)
            out = m.infer_points(x, out=out, raster=dict(target, cull=0), **kw)
            _same_raster(out.raster, want[0], f"graph call {call}")
        for _ in range(3):  # another option on the same pointers: its own graph and its own result
            out = m.infer_points(x, out=out, raster=dict(target, cull=1), **kw)
        _same_raster(out.raster, want[1], "cull 1")
        for _ in range(2):
            m.infer_points(x, out=out, raster=dict(target, cull=0), **kw)
            m.infer_points(x, out=out, raster=dict(target, cull=1), **kw)
        _same_raster(out.raster, want[1], "after the loop")
        assert m.query("allocs") == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


def test_refusals_leave_the_outputs_untouched(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        E, S = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
        bad = [(dict(cull=2), E, "cull"), (dict(max_extent=1025), E, "max_extent"), (dict(max_extent=-1), E, "max_extent"),
               (dict(z_near=float("nan")), E, "z_near"), (dict(faces=False), E, "`faces`"), (dict(xyz=False), E, "`xyz`"),
               (dict(thin=0.05), E, "voxel thinning"), (dict(T=0), S, "shape")]
        cams = _cams(m.infer_points(x, world=True, **OPTS), 2)
        for host in (False, True):
            for kw, code, word in bad:
                rc, t = _call(m, "raster", x, host, cams, **kw)
                assert rc == code and word in _lib.load().md_last_error().decode(), (kw, host, _lib.load().md_last_error().decode())
                for k, v in t.items():
                    assert (v == np.asarray(FILL[k], v.dtype)).all(), (kw, host, k)
        with pytest.raises(_lib.MdError) as e:  # raster without a mesh
            m.infer_points(x, world=True, raster=dict(H=8, W=8, focal_px=torch.tensor([5.0], device="cuda")))
        assert e.value.code == E and "`faces`" in e.value.message
        with pytest.raises(_lib.MdError) as e:  # an rgb image without the list's rgb
            out = m.infer_points(x, world=True, mesh=True, raster=dict(H=8, W=8, focal_px=torch.tensor([5.0], device="cuda")))
            out.raster.rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
            m.infer_points(x, world=True, mesh=True, out=out, raster=dict(H=8, W=8, focal_px=torch.tensor([5.0], device="cuda")))
        assert e.value.code == E and "rgb" in e.value.message
    finally:
        m.destroy()
