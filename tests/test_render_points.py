"""Rendering a point list into target cameras: md_op_render_points and its host reference pipeline.render_points.
include/mi_depth.h states the contract, DESIGN 12.4 the kernels. A z-buffer on 64-bit keys is selection, not blending: every
comparison is bit for bit.

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402
from burn_depth_amd import pipeline as P  # noqa: E402
from points_util import _bits, _cameras, _t, dev, lib  # noqa: E402,F401

f32 = np.float32
NEW_ENTRIES = ("md_render_opts_default", "md_op_render_points", "md_infer_points_render")
TINY, HUGE = f32(np.finfo(f32).tiny), f32(np.finfo(f32).max)


def _targets(rng, T, H, W):
    """T cameras near the origin that look down +z with a small yaw and offset each: all of them see most of `_cloud`"""
    K = np.zeros((T, 3, 3), f32)
    E = np.zeros((T, 3, 4), f32)
    for j in range(T):
        K[j] = [[0.9 * W + j, 0, W / 2 + 0.3], [0, 0.8 * W + 2 * j, H / 2 - 0.7], [0, 0, 1]]
        a = rng.uniform(-0.15, 0.15)
        E[j, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[j, :, 3] = rng.uniform(-0.3, 0.3, 3)
    return K, E


def _cloud(rng, n):
    """n world points in a box in front of `_targets`, wider than their view, with colours"""
    xyz = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n), rng.uniform(2.0, 6.0, n)], 1).astype(f32)
    return xyz, rng.integers(0, 256, (n, 3), dtype=np.uint8)


def _dict_render(xyz, H, W, K, E, off, radius, n=None, z_near=0.0, z_far=0.0):
    """The contract once more, point by point and pixel by pixel with a dictionary of scalars -> {(j, v, u): (bits(p.z), i)}"""
    zn, zf = (f32(z_near) if z_near > 0 else TINY), (f32(z_far) if z_far > 0 else HUGE)
    off, half = f32(off), f32(0.5)
    best = {}
    xyz = np.asarray(xyz, f32)
    with np.errstate(all="ignore"):
        for i in range(len(xyz) if n is None else n):
            x, y, z = xyz[i]
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            for j in range(len(K)):
                if E is None:
                    p = (x, y, z)
                else:
                    p = [((E[j, a, 0] * x + E[j, a, 1] * y) + E[j, a, 2] * z) + E[j, a, 3] for a in range(3)]
                if not (np.isfinite(p[2]) and zn <= p[2] <= zf):
                    continue
                uf = ((K[j, 0, 0] * (p[0] / p[2])) + K[j, 0, 2]) - off
                vf = ((K[j, 1, 1] * (p[1] / p[2])) + K[j, 1, 2]) - off
                uu, vv = np.floor(uf + half), np.floor(vf + half)
                if not (0 <= uu < W and 0 <= vv < H):
                    continue
                key = (int(f32(p[2]).view(np.uint32)), i)
                for v in range(max(int(vv) - radius, 0), min(int(vv) + radius, H - 1) + 1):
                    for u in range(max(int(uu) - radius, 0), min(int(uu) + radius, W - 1) + 1):
                        if (j, v, u) not in best or key < best[(j, v, u)]:
                            best[(j, v, u)] = key
    return best


def _same_as_dict(r, best, T, H, W):
    depth, index = np.zeros((T, H, W), np.uint32), np.full((T, H, W), -1, np.int32)
    for (j, v, u), (zb, i) in best.items():
        depth[j, v, u], index[j, v, u] = zb, i
    assert np.array_equal(_bits(r.depth), depth) and np.array_equal(r.index, index)
    per = [(index[j] >= 0).sum() for j in range(T)]
    assert r.filled.tolist() == per + [sum(per)]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_render_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    for struct in ("md_render_opts", "md_render_outputs", "md_points_render"):
        assert "} %s;" % struct in header
    assert [n for n, _ in _lib.MdRenderOpts._fields_] == ["pixel_offset", "z_near", "z_far", "radius"]
    assert [n for n, _ in _lib.MdRenderOutputs._fields_] == ["depth", "index", "rgb", "filled"]
    assert [n for n, _ in _lib.MdPointsRender._fields_] == ["T", "H", "W", "cam", "opts", "out"]
    o = _lib.MdRenderOpts(1.0, 2.0, 3.0, 4)
    lib.md_render_opts_default(C.byref(o))
    assert (o.pixel_offset, o.z_near, o.z_far, o.radius) == (0.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("N", [0, 1, 300, 5000])
def test_reference_against_the_dictionary_restatement(N):
    rng = np.random.default_rng(N)
    xyz, rgb = _cloud(rng, N)
    for T in (1, 3):
        for H, W in ((4, 4), (37, 53)):
            K, E = _targets(rng, T, H, W)
            for radius in (0, 1, 2):
                r = P.render_points(xyz, H, W, K, E, rgb=rgb, pixel_offset=0.5, radius=radius)
                _same_as_dict(r, _dict_render(xyz, H, W, K, E, 0.5, radius), T, H, W)
                hit = r.index >= 0
                assert N < 300 or hit.any()
                assert np.array_equal(r.rgb[hit], rgb[r.index[hit]]) and not r.rgb[~hit].any()
    # the count word, the bounds and the camera frame
    if N >= 300:
        K, E = _targets(rng, 2, 9, 11)
        for count in (-3, 0, 100, N + 7):
            r = P.render_points(xyz, 9, 11, K, E, count=count, radius=1)
            _same_as_dict(r, _dict_render(xyz, 9, 11, K, E, 0.0, 1, n=min(max(count, 0), N)), 2, 9, 11)
        r = P.render_points(xyz, 9, 11, K, E, z_near=3.0, z_far=4.5)
        _same_as_dict(r, _dict_render(xyz, 9, 11, K, E, 0.0, 0, z_near=3.0, z_far=4.5), 2, 9, 11)
        assert r.depth[r.index >= 0].min() >= 3.0 and r.depth.max() <= 4.5
        _same_as_dict(P.render_points(xyz, 9, 11, K), _dict_render(xyz, 9, 11, K, None, 0.0, 0), 2, 9, 11)
        f = np.array([7.0, 9.5], f32)
        Kf = np.array([[[v, 0, 11 / 2], [0, v, 9 / 2], [0, 0, 1]] for v in f], f32)
        _same_as_dict(P.render_points(xyz, 9, 11, focal_px=f, extrinsics=E), _dict_render(xyz, 9, 11, Kf, E, 0.0, 0), 2, 9, 11)


def _round_trip_scene():
    H, W = 37, 53
    rng = np.random.default_rng(11)
    K, _ = _cameras(rng, 1, H, W)
    depth = rng.uniform(0.5, 20.0, (1, H, W)).astype(f32)
    depth[0, 3, 5:9] = 0.0  # invalid pixels: holes of the round trip
    depth[0, 30, 50] = np.nan
    return H, W, K, depth, P.unproject_depth(depth, K, pixel_offset=0.5, world=False, stride=1)


def _check_round_trip(r, depth, hp):
    valid = hp.mask[0].astype(bool)
    rank = np.full(valid.shape, -1, np.int32)
    rank[valid] = np.arange(valid.sum())
    assert np.array_equal(r.index[0], rank)
    assert np.array_equal(_bits(r.depth[0]), _bits(np.where(valid, depth[0], f32(0))))
    assert r.filled.tolist() == [int(valid.sum())] * 2


def test_round_trip_on_the_host():
    H, W, K, depth, hp = _round_trip_scene()
    # every point lands on its own pixel: rendered alone (no z-buffer), point i fills pixel i of the valid ones
    vs, us = np.nonzero(hp.mask[0])
    for i in range(0, len(hp.xyz), 97):
        one = P.render_points(hp.xyz[i:i + 1], H, W, K, pixel_offset=0.5)
        assert np.argwhere(one.index[0] == 0).tolist() == [[vs[i], us[i]]], i
    best = _dict_render(hp.xyz, H, W, K, None, 0.5, 0)
    assert sorted(best) == [(0, v, u) for v, u in zip(vs, us)]
    _check_round_trip(P.render_points(hp.xyz, H, W, K, pixel_offset=0.5), depth, hp)


def test_reference_refuses_bad_arguments():
    xyz = np.zeros((3, 3), f32)
    for kw in (dict(radius=-1), dict(radius=17), dict(z_near=-1.0), dict(z_far=float("nan")), dict(z_near=2.0, z_far=1.0),
               dict(pixel_offset=float("inf"))):
        with pytest.raises(ValueError):
            P.render_points(xyz, 4, 4, focal_px=[3.0], **kw)
    with pytest.raises(ValueError):
        P.render_points(xyz, 4, 4)
    with pytest.raises(ValueError):
        P.render_points(xyz, 0, 4, focal_px=[3.0])


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev_render(dev, xyz, H, W, K=None, E=None, focal=None, rgb=None, count=None, **kw):
    from burn_depth_amd import ops
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    r = ops.render_points(dev, _t(np.asarray(xyz, f32).reshape(-1, 3)), H, W, _t(K), _t(E), _t(focal), rgb=_t(rgb), count=cnt, **kw)
    torch.cuda.synchronize()
    return r


def _same(got, want, what=""):
    for k in ("depth", "index", "rgb", "filled"):
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            g = g.cpu().numpy()
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, int((g != w).sum()))


def _both(dev, xyz, H, W, K=None, E=None, focal=None, rgb=None, count=None, what="", **kw):
    want = P.render_points(xyz, H, W, K, E, focal, rgb=rgb, count=count, **kw)
    _same(_dev_render(dev, xyz, H, W, K, E, focal, rgb, count, **kw), want, what)
    return want


@gpu
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 50001])
def test_tails(dev, N):
    rng = np.random.default_rng(100 + N)
    xyz, rgb = _cloud(rng, N)
    for H, W in ((37, 53), (96, 96)):
        for T in (1, 3):
            K, E = _targets(rng, T, H, W)
            want = _both(dev, xyz, H, W, K, E, rgb=rgb, pixel_offset=0.5, what=(N, H, W, T))
            assert (want.filled[:-1] > 0).all() or N < 63


@gpu
def test_count_word(dev):
    rng = np.random.default_rng(1)
    xyz, rgb = _cloud(rng, 3000)  # every row lies in front of the cameras: rows past n must not appear
    K, E = _targets(rng, 2, 37, 53)
    full = P.render_points(xyz, 37, 53, K, E, rgb=rgb)
    assert full.index.max() > 2900
    for count in (1000, 3000 + 17, 0, -5, 1):
        want = _both(dev, xyz, 37, 53, K, E, rgb=rgb, count=count, what=count)
        assert want.index.max() < max(min(count, 3000), 0) or count > 3000
    assert P.render_points(xyz, 37, 53, K, E, count=0).filled.tolist() == [0, 0, 0]


@gpu
def test_contention_ties_and_descending_order(dev):
    n = 20000
    rng = np.random.default_rng(2)
    K = np.array([[[1, 0, 2], [0, 1, 2], [0, 0, 1]]], f32)  # 4 x 4: pixel = floor(x / z + 2.5)
    z = np.full(n, 2.0, f32)
    far = np.arange(n) >= n // 2
    z[far] = (1.0 + (n - np.arange(n)[far]) * 1e-4).astype(f32)  # distinct, the nearest has the largest row
    assert len(np.unique(z[far])) == far.sum()
    col = np.where(far, rng.uniform(-0.4, 1.4, n), rng.uniform(-2.4, -0.6, n))  # ties on columns 0..1, the rest on 2..3
    xyz = np.stack([col * z, rng.uniform(-1.9, 1.4, n) * z, z], 1).astype(f32)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    want = _both(dev, xyz, 4, 4, K, rgb=rgb, what="contention")
    assert want.filled.tolist() == [16, 16]
    tie = want.index[0][:, :2]
    assert (tie < 200).all() and (want.depth[0][:, :2] == 2.0).all()  # among some 1250 equal keys per pixel the smallest row
    assert (want.index[0][:, 2:] > n - 200).all()
    _both(dev, xyz, 4, 4, K, rgb=rgb, radius=2, what="contention, radius 2")


@gpu
def test_rejection(dev):
    K = np.array([[[8, 0, 2], [0, 8, 2], [0, 0, 1]]], f32)  # 8 x 8, z = 1: uf + 0.5 = 8 x + 2.5, exact in f32
    lo, hi = f32(-2.5 / 8), f32(5.5 / 8)                    # uf + 0.5 = 0 and = W
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))    # noqa: E731
    mid = f32(0.125)
    probes = [((lo, mid, 1), True), ((below(lo), mid, 1), False), ((hi, mid, 1), False), ((below(hi), mid, 1), True),
              ((mid, lo, 1), True), ((mid, below(lo), 1), False), ((mid, hi, 1), False), ((mid, below(hi), 1), True),
              ((np.nan, 0, 1), False), ((0, np.inf, 1), False), ((0, 0, -np.inf), False), ((0, 0, np.nan), False),
              ((0, 0, 0), False), ((0, 0, -1), False), ((3e38, 0, 1e-30), False), ((-3e38, 0, 1e-30), False), ((0, 3e38, 1e-30), False),
              ((1e29, 0, 1), False), ((0, -1e29, 1), False), ((0.25, 0.25, 1), True)]
    xyz = np.array([p for p, _ in probes], f32)
    with np.errstate(all="ignore"):
        seen = [bool(P.render_points(xyz[i:i + 1], 8, 8, K).filled[-1]) for i in range(len(xyz))]
    assert seen == [s for _, s in probes]
    want = _both(dev, xyz, 8, 8, K, what="probes")
    assert want.index[0, 3, 0] == 0 and want.index[0, 3, 7] == 3 and want.index[0, 0, 3] == 4 and want.index[0, 7, 3] == 7
    # the bounds on p.z
    zs = np.array([[0.125 * k * z, 0, z] for k, z in enumerate((0.5, 1.0, 1.5, 2.0, 2.5))], f32)  # pixel (2, 2 + k) each
    want = _both(dev, zs, 8, 8, K, z_near=1.0, z_far=2.0, what="bounds")
    assert sorted(want.index[want.index >= 0].tolist()) == [1, 2, 3]
    # a camera with NaN in t sees nothing; its neighbour is not disturbed
    rng = np.random.default_rng(3)
    cloud, _ = _cloud(rng, 500)
    for slot in (0, 2):
        K3, E3 = _targets(rng, 3, 37, 53)
        E3[1, slot, 3] = np.nan
        want = _both(dev, cloud, 37, 53, K3, E3, what=("nan t", slot))
        assert want.filled[1] == 0 and want.filled[0] > 0 and want.filled[2] > 0


@gpu
def test_footprint_clipping_and_occlusion(dev):
    H, W = 9, 12
    K = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], f32)  # z = 1: pixel (v, u) = (y, x)
    hits = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 5), (H - 1, 6), (4, 0), (5, W - 1)]
    xyz = np.array([[u, v, 1.0] for v, u in hits], f32)
    for radius in (1, 2):
        want = _both(dev, xyz, H, W, K, radius=radius, what=("corners", radius))
        assert want.filled[-1] > len(hits)
    # a far splat partly hidden by a nearer one
    two = np.array([[5 * 3.0, 4 * 3.0, 3.0], [6, 5, 1.0]], f32)
    want = _both(dev, two, H, W, K, radius=2, what="occlusion")
    assert (want.index[0] == 0).sum() == 25 - 16 and (want.index[0] == 1).sum() == 25


@gpu
def test_camera_forms_and_single_outputs(dev):
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import RenderedPoints
    rng = np.random.default_rng(4)
    xyz, rgb = _cloud(rng, 4000)
    K, E = _targets(rng, 2, 37, 53)
    f = np.array([40.0, 55.5], f32)
    _both(dev, xyz, 37, 53, focal=f, E=E, rgb=rgb, radius=1, what="focal")
    _both(dev, xyz, 37, 53, K, rgb=rgb, what="camera frame")
    want = _both(dev, xyz, 37, 53, K, E, what="no rgb")
    assert want.rgb is None
    want = P.render_points(xyz, 37, 53, K, E, rgb=rgb, radius=1)
    shapes = dict(depth=((2, 37, 53), torch.float32), index=((2, 37, 53), torch.int32), rgb=((2, 37, 53, 3), torch.uint8),
                  filled=((3,), torch.int32))
    for k, (shape, dt) in shapes.items():
        out = RenderedPoints(**{k: torch.full(shape, 77, dtype=dt, device="cuda")})
        got = ops.render_points(dev, _t(xyz), 37, 53, _t(K), _t(E), rgb=_t(rgb), radius=1, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(getattr(got, k).cpu().numpy().view(np.uint8), getattr(want, k).view(np.uint8)), k


@gpu
def test_round_trip_on_the_device(dev):
    from burn_depth_amd import ops
    H, W, K, depth, hp = _round_trip_scene()
    pc = ops.unproject(dev, _t(depth), _t(K), dense=False, pixel_offset=0.5)
    r = ops.render_points(dev, pc.xyz, H, W, _t(K), count=pc.count[-1:], pixel_offset=0.5)  # the list's own count word
    torch.cuda.synchronize()
    want = P.render_points(hp.xyz, H, W, K, pixel_offset=0.5)
    _same(r, want, "round trip")
    _check_round_trip(want, depth, hp)


@gpu
def test_world_round_trip(dev):
    H, W = 37, 53
    rng = np.random.default_rng(12)
    K, E = _cameras(rng, 2, H, W)
    depth = rng.uniform(0.5, 20.0, (2, H, W)).astype(f32)
    hp = P.unproject_depth(depth, K, E, pixel_offset=0.5, world=True)
    want = _both(dev, hp.xyz, H, W, K[:1], E[:1], pixel_offset=0.5, what="world")
    own = P.render_points(hp.xyz[:hp.count[0]], H, W, K[:1], E[:1], pixel_offset=0.5)  # view 0's own points alone
    seen = own.index[0] >= 0
    assert seen.sum() > 0.9 * H * W
    assert (want.index[0][seen] >= 0).all() and (want.depth[0][seen] <= own.depth[0][seen]).all()  # more points only come nearer


@gpu
def test_refusals_leave_the_outputs_untouched(dev, lib):
    xyz = torch.tensor([[0.0, 0.0, 1.0]] * 8, device="cuda")  # eight points on pixel (0, 0)
    rgb = torch.zeros(8, 3, dtype=torch.uint8, device="cuda")
    cams = torch.eye(3, device="cuda").reshape(1, 3, 3).contiguous()
    outs = dict(depth=torch.full((2, 2), 77.0, device="cuda"), index=torch.full((2, 2), 77, dtype=torch.int32, device="cuda"),
                rgb=torch.full((2, 2, 3), 77, dtype=torch.uint8, device="cuda"), filled=torch.full((2,), 77, dtype=torch.int32, device="cuda"))
    INV, SHP = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
    all_out = _lib.MdRenderOutputs(*(outs[k].data_ptr() for k in ("depth", "index", "rgb", "filled")))
    cam = _lib.MdPointsCameras(cams.data_ptr(), None, None)
    ok = _lib.MdRenderOpts(0.0, 0.0, 0.0, 0)

    def call(code, N=8, T=1, H=2, W=2, cam=cam, o=ok, out=all_out, rgb_in=rgb, dev_h=dev.handle):
        rc = lib.md_op_render_points(dev_h, xyz.data_ptr(), rgb_in.data_ptr() if rgb_in is not None else None, N, None, T, H, W,
                                     C.byref(cam) if cam else None, C.byref(o) if o else None, C.byref(out) if out else None, None)
        assert rc == code, (rc, lib.md_last_error().decode())

    call(INV, o=None)
    call(INV, out=None)
    call(INV, cam=None)
    call(INV, out=_lib.MdRenderOutputs(None, None, None, None))
    call(INV, rgb_in=None)
    call(INV, cam=_lib.MdPointsCameras(None, None, None))
    call(INV, o=_lib.MdRenderOpts(0.0, 0.0, 0.0, -1))
    call(INV, o=_lib.MdRenderOpts(0.0, 0.0, 0.0, 17))
    for bad in (float("nan"), float("inf")):
        call(INV, o=_lib.MdRenderOpts(bad, 0.0, 0.0, 0))
        call(INV, o=_lib.MdRenderOpts(0.0, bad, 0.0, 0))
        call(INV, o=_lib.MdRenderOpts(0.0, 0.0, bad, 0))
    call(INV, o=_lib.MdRenderOpts(0.0, -1.0, 0.0, 0))
    call(INV, o=_lib.MdRenderOpts(0.0, 0.0, -1.0, 0))
    call(INV, o=_lib.MdRenderOpts(0.0, 2.0, 1.0, 0))
    call(INV, dev_h=None)
    call(SHP, N=-1)
    call(SHP, N=1 << 31)
    for shape in (dict(T=0), dict(H=0), dict(W=-1), dict(T=1, H=1 << 16, W=1 << 15), dict(H=1 << 24, W=1), dict(H=1, W=1 << 24)):
        call(SHP, **shape)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert (t == 77).all(), k
    call(_lib.MD_OK)  # the same arguments without a fault are accepted
    torch.cuda.synchronize()
    assert outs["filled"].tolist() == [1, 1] and outs["index"].reshape(-1).tolist() == [0, -1, -1, -1]
