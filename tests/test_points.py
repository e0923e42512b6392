"""The point path: md_op_unproject (depth + pinhole cameras -> point map, mask and the ordered compacted cloud on the device),
md_infer_points (the model, then the same kernels, in one call) and their host reference pipeline.unproject_depth.

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import importlib.util
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
from points_util import _bits, _cameras, _cloud_np, _da3, _da3_subset, _image, _pro, _rotation, _same_cloud, _t, dev, lib  # noqa: E402,F401

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of f32
NEW_ENTRIES = ("md_points_opts_default", "md_op_unproject", "md_infer_points")


def _noise_scene(B, H, W, seed=7):
    """depth = exp(N(0.5, 0.6)), conf = 1 + 2 U(0,1): with depth in [0.5, 6] and conf_min 1.8 the reference keeps 0.57-0.58."""
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.5, 0.6, (B, H, W))).astype(f32), (1 + 2 * rng.random((B, H, W))).astype(f32)


def _step_scene(H, W):
    """Two planes (2 left of W/2, 5 right of it) plus a ramp of 0.002 per row, and a block of depth 1 inside the left plane."""
    v, u = np.mgrid[0:H, 0:W]
    d = np.where(u < W / 2, 2.0, 5.0) + 0.002 * v
    y0, x0, n = H // 7, W // 10 + 1, min(20, H // 3, W // 4)
    d[y0:y0 + n, x0:x0 + n] = 1.0
    return d.astype(f32), (y0, x0, n)


def _assert_covered(ref, lo=0.25, hi=0.75):
    """The coverage condition of every randomised comparison: the host reference keeps between a quarter and three quarters
    of each view, so a comparison cannot pass because almost nothing (or everything) was kept."""
    share = ref.mask.reshape(ref.mask.shape[0], -1).mean(1)
    assert ((share >= lo) & (share <= hi)).all(), share


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_point_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    for s in ("md_points_opts", "md_points_cameras", "md_points_outputs"):
        assert f"}} {s};" in header
    o = _lib.MdPointsOpts(9, 9, 9, 9, 9, 9, 9)
    lib.md_points_opts_default(C.byref(o))
    assert (o.pixel_offset, o.depth_min, o.depth_max, o.conf_min, o.edge_rtol, o.stride, o.world) == (0, 0, 0, 0, 0, 1, 0)


def test_reference_closed_forms_exact_in_f32():
    H, W = 16, 24
    # a fronto-parallel plane: d = 2, fx = fy = 128, integer principal point -> X = (u - cx) / 64 exactly
    K = np.array([[[128, 0, 12], [0, 128, 8], [0, 0, 1]]], f32)
    r = P.unproject_depth(np.full((1, H, W), 2, f32), intrinsics=K)
    v, u = np.mgrid[0:H, 0:W]
    assert np.array_equal(r.point_map[0, ..., 0], ((u - 12) / 64).astype(f32))
    assert np.array_equal(r.point_map[0, ..., 1], ((v - 8) / 64).astype(f32))
    assert (r.point_map[0, ..., 2] == 2).all() and r.mask.all() and r.count.tolist() == [H * W, H * W]
    assert np.array_equal(r.xyz, r.point_map.reshape(-1, 3))
    # focal form: K = (f, f, W/2, H/2); pixel centres shift the grid by half a pixel
    rf = P.unproject_depth(np.full((1, H, W), 2, f32), focal_px=[128.0], pixel_offset=0.5)
    assert np.array_equal(rf.point_map[0, ..., 0], ((u + 0.5 - 12) / 64).astype(f32))
    # a camera rotated 90 degrees about Y with an integer translation. World-to-camera p_c = R p_w + t with
    # R = [[0,0,-1],[0,1,0],[1,0,0]], t = (1,2,3): p_w = R^T (p_c - t) = (zc - 3, yc - 2, -(xc - 1))
    E = np.array([[[0, 0, -1, 1], [0, 1, 0, 2], [1, 0, 0, 3]]], f32)
    rw = P.unproject_depth(np.full((1, H, W), 2, f32), intrinsics=K, extrinsics=E, world=True)
    xc, yc = (u - 12) / 64, (v - 8) / 64
    want = np.stack([np.full_like(xc, 2.0 - 3), yc - 2, -(xc - 1)], -1).astype(f32)
    assert np.array_equal(rw.point_map[0], want)


def test_reference_world_to_camera_convention():
    """camera.rs:248-254: c2w_R = R^T, c2w_t = -R^T t. The camera centre is -R^T t, and a pixel on the optical axis at depth d
    lands at centre + d R^T e_z."""
    rng = np.random.default_rng(3)
    R, t = _rotation(rng), rng.uniform(-3, 3, 3)
    E = np.concatenate([R, t[:, None]], 1)[None]
    K = np.array([[[100, 0, 5], [0, 90, 4], [0, 0, 1]]], np.float64)
    centre = -R.T @ t
    for d in (0.5, 2.0, 7.25):
        depth = np.zeros((1, 9, 11))
        depth[0, 4, 5] = d  # the principal point
        r = P.unproject_depth(depth, intrinsics=K, extrinsics=E, world=True, dtype=np.float64)
        assert r.count.tolist() == [1, 1]
        np.testing.assert_allclose(r.xyz[0], centre + d * R.T[:, 2], rtol=0, atol=1e-13)
    # and a general pixel maps back through p_c = R p_w + t to (rx d, ry d, d)
    depth = rng.uniform(1, 4, (1, 9, 11))
    r = P.unproject_depth(depth, intrinsics=K, extrinsics=E, world=True, dtype=np.float64)
    pc = r.point_map[0] @ R.T + t
    v, u = np.mgrid[0:9, 0:11]
    np.testing.assert_allclose(pc, np.stack([(u - 5) / 100 * depth[0], (v - 4) / 90 * depth[0], depth[0]], -1), atol=1e-12)


def test_reference_f32_against_f64_with_a_derived_bound():
    """Each rounded f32 operation contributes at most 2^-24 of the magnitude it produces (first order; the bound carries a
    factor 1.01 for the second-order terms). A camera-space coordinate is 3 operations deep -- (u + off) - c, / f, * d; the
    offsets here (0, 0.5) make the first addition exact --, so |err| <= 3 u |X|. A world coordinate adds the subtraction of t
    (one operation on each q) and 3 multiplies + 2 adds: every term R_ij q_i carries the 3 u of q's camera part, 1 of the
    subtraction and 1 of the multiply, and the two additions 1 each of the partial sums, so
    |err| <= u (3 |R_.j|.|p_c| + 2 |R_.j|.|q| + 2 sum |R_ij q_i|) <= 7 u M with M = sum_i |R_ij| (|p_c,i| + |t_i|)."""
    B, H, W = 3, 70, 98
    rng = np.random.default_rng(5)
    d, _ = _noise_scene(B, H, W)
    K, E = _cameras(rng, B, H, W)
    for off in (0.0, 0.5):
        a = P.unproject_depth(d, intrinsics=K, pixel_offset=off)
        b = P.unproject_depth(d, intrinsics=K, pixel_offset=off, dtype=np.float64)
        assert a.point_map.dtype == np.float32 and np.array_equal(a.mask, b.mask)
        assert (np.abs(a.point_map - b.point_map) <= 1.01 * 3 * U * np.abs(b.point_map)).all()
        aw = P.unproject_depth(d, intrinsics=K, extrinsics=E, pixel_offset=off, world=True)
        bw = P.unproject_depth(d, intrinsics=K, extrinsics=E, pixel_offset=off, world=True, dtype=np.float64)
        Rabs, tabs = np.abs(E[:, :, :3].astype(np.float64)), np.abs(E[:, :, 3].astype(np.float64))
        M = np.einsum("bij,bhwi->bhwj", Rabs, np.abs(b.point_map) + tabs[:, None, None, :])
        assert (np.abs(aw.point_map - bw.point_map) <= 1.01 * 7 * U * M).all()


def test_reference_validity_on_planted_pixels():
    d = np.full((1, 6, 8), 2, f32)
    c = np.full((1, 6, 8), 3, f32)
    planted = {(0, 0): np.nan, (0, 1): np.inf, (0, 2): -np.inf, (0, 3): 0.0, (0, 4): -1.0, (1, 0): 0.25, (1, 1): 9.0}
    for (v, u), val in planted.items():
        d[0, v, u] = val
    c[0, 2, 0], c[0, 2, 1], c[0, 2, 2] = 1.5, np.nextafter(f32(1.5), f32(0)), np.nan  # exactly at conf_min: kept
    r = P.unproject_depth(d, focal_px=[10.0], conf=c, depth_min=0.5, depth_max=6, conf_min=1.5)
    want = np.ones((6, 8), np.uint8)
    for vu in planted:
        want[vu] = 0
    want[2, 1] = want[2, 2] = 0
    assert np.array_equal(r.mask[0], want)
    assert (r.point_map[0][want == 0] == 0).all() and r.count.tolist() == [int(want.sum())] * 2
    assert np.array_equal(r.conf, c[0][want == 1])
    # the default range: every positive normal f32 is kept, zero and negatives are not
    tiny = np.finfo(f32).tiny
    r = P.unproject_depth(np.array([[[tiny, np.finfo(f32).max, 0.0, -tiny]]], f32), focal_px=[10.0])
    assert r.mask.ravel().tolist() == [1, 1, 0, 0]
    # stride thins the list, not the dense map; the order is (b, v, u)
    dd = np.arange(1, 2 * 5 * 7 + 1, dtype=f32).reshape(2, 5, 7)
    r = P.unproject_depth(dd, focal_px=[10.0, 10.0], stride=3)
    assert r.mask.all() and r.count.tolist() == [6, 6, 12]
    assert np.array_equal(r.xyz[:, 2], dd[:, ::3, ::3].ravel())


def test_reference_edge_filter_on_the_step_scene():
    """edge_rtol = 0.05 drops the pixels either side of every depth step and nothing else (the ramp's 0.002 per row is far
    below 5 %). The count follows from the edge lengths: the plane boundary runs over H rows, two pixels wide; the block's
    outline loses its own rim (4 n - 4) and the n pixels outside each of its four sides."""
    H, W = 70, 98
    d, (y0, x0, n) = _step_scene(H, W)
    assert n == 20
    r = P.unproject_depth(d[None], focal_px=[100.0], edge_rtol=0.05)
    dropped = 2 * H + (4 * n - 4) + 4 * n
    assert dropped == 296 and int(r.count[1]) == H * W - dropped
    assert abs(r.mask.mean() - 0.957) < 5e-4
    m = r.mask[0]
    assert not m[:, W // 2 - 1].any() and not m[:, W // 2].any() and m[:, W // 2 - 2].sum() == H and m[:, W // 2 + 1].all()
    assert not m[y0, x0:x0 + n].any() and not m[y0 - 1, x0:x0 + n].any() and m[y0 - 1, x0 - 1] and m[y0 + 1, x0 + 1:x0 + n - 1].all()
    # a neighbour that is not finite or <= 0 is ignored: a hole does not eat its surroundings
    d2 = d.copy()
    d2[50, 70], d2[51, 70] = np.nan, 0.0
    r2 = P.unproject_depth(d2[None], focal_px=[100.0], edge_rtol=0.05)
    assert int(r2.count[1]) == H * W - dropped - 2


def test_coverage_of_the_noise_scene():
    d, c = _noise_scene(3, 70, 98)
    r = P.unproject_depth(d, focal_px=[100.0] * 3, conf=c, depth_min=0.5, depth_max=6, conf_min=1.8)
    share = r.mask.reshape(3, -1).mean(1)
    assert share.min() >= 0.574 and share.max() <= 0.582, share
    _assert_covered(r)
    _assert_covered(P.unproject_depth(d, focal_px=[100.0] * 3, depth_min=1.2, depth_max=3.0))  # the range used without confidence


def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(257, 3)).astype(f32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    for col in (None, rgb):
        path = str(tmp_path / "sub" / "cloud.ply")
        P.write_ply(path, xyz, col)
        head = open(path, "rb").read(64)
        assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 257\n")
        x2, c2 = P.read_ply(path)
        assert np.array_equal(_bits(x2), _bits(xyz))
        assert (c2 is None) if col is None else np.array_equal(c2, col)
    P.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), f32))
    assert P.read_ply(str(tmp_path / "empty.ply"))[0].shape == (0, 3)
    with pytest.raises(ValueError):
        P.write_ply(str(tmp_path / "bad.ply"), xyz, rgb[:5])


def test_point_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched: with a null device the valid call is refused last."""
    buf = (C.c_float * 64)()
    px = C.cast(buf, C.c_void_p)
    cam = _lib.MdPointsCameras(px.value, px.value, None)

    def call(o=None, out=None, cam_=cam, B=1, H=2, W=2, conf=None, rgb=None, no_o=False, no_out=False, no_cam=False):
        o = o or _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
        out = out or _lib.MdPointsOutputs(px.value, None, None, None, None, None, 0, None)
        return lib.md_op_unproject(None, px, conf, rgb, B, H, W, None if no_cam else C.byref(cam_), None if no_o else C.byref(o),
                                   None if no_out else C.byref(out), None)

    E = _lib.MD_ERR_INVALID_ARG
    assert call(no_o=True) == E and call(no_out=True) == E and call(no_cam=True) == E
    assert call(o=_lib.MdPointsOpts(0, 0, 0, 0, 0, 0, 0)) == E  # stride < 1
    assert call(out=_lib.MdPointsOutputs(None, None, px.value, None, None, px.value, -1, None)) == E  # capacity < 0
    assert call(out=_lib.MdPointsOutputs(None, None, px.value, None, None, None, 4, None)) == E  # xyz without count
    assert call(out=_lib.MdPointsOutputs(None, None, px.value, px.value, None, px.value, 4, None)) == E  # rgb out, no rgb in
    assert call(out=_lib.MdPointsOutputs(None, None, px.value, None, px.value, px.value, 4, None)) == E  # conf out, no conf
    for bad in (float("nan"), float("inf"), -1.0):
        for field in ("edge_rtol", "conf_min", "depth_min", "depth_max"):
            o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
            setattr(o, field, bad)
            assert call(o=o) == E, (field, bad)
    assert call(o=_lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 1), cam_=_lib.MdPointsCameras(px.value, None, None)) == E  # world, no E
    assert call(cam_=_lib.MdPointsCameras(None, px.value, None)) == E  # neither intrinsics nor focal
    for shape in ((0, 2, 2), (1, 0, 2), (1, 2, -1), (1, 65536, 65536)):
        assert call(B=shape[0], H=shape[1], W=shape[2]) == _lib.MD_ERR_SHAPE, shape
    assert call() == E  # the null device, after everything else passed
    out = _lib.MdPointsOutputs()
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    assert lib.md_infer_points(None, px, 1, 2, 2, 1, None, None, C.byref(o), C.byref(out), 1, None) == E
    assert (np.frombuffer(buf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0


def _run_op(dev, d, K=None, E=None, focal=None, conf=None, rgb=None, capacity=None, **opts):
    """ops.unproject on poisoned outputs -> numpy dict."""
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import PointCloud
    B, H, W = d.shape
    cap = B * H * W if capacity is None else capacity
    out = PointCloud(point_map=torch.full((B, H, W, 3), POISON, device="cuda"), mask=torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda"),
                     xyz=torch.full((cap, 3), POISON, device="cuda"), count=torch.full((B + 1,), -5, dtype=torch.int32, device="cuda"),
                     rgb=torch.full((cap, 3), 77, dtype=torch.uint8, device="cuda") if rgb is not None else None,
                     conf=torch.full((cap,), POISON, device="cuda") if conf is not None else None)
    ops.unproject(dev, _t(d), intrinsics=_t(K), extrinsics=_t(E), focal_px=_t(focal), conf=_t(conf), rgb=_t(rgb), out=out, **opts)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(out).items()}


def _assert_same(got, ref, capacity=None, what=""):
    assert np.array_equal(got["count"], ref.count), (what, got["count"], ref.count)
    assert np.array_equal(got["mask"], ref.mask), what
    assert np.array_equal(_bits(got["point_map"]), _bits(ref.point_map)), what
    n = int(ref.count[-1]) if capacity is None else min(int(ref.count[-1]), capacity)
    assert np.array_equal(_bits(got["xyz"][:n]), _bits(ref.xyz[:n])), what
    assert (got["xyz"][n:] == f32(POISON)).all(), what
    if got["rgb"] is not None:
        assert np.array_equal(got["rgb"][:n], ref.rgb[:n]) and (got["rgb"][n:] == 77).all(), what
    if got["conf"] is not None:
        assert np.array_equal(_bits(got["conf"][:n]), _bits(ref.conf[:n])) and (got["conf"][n:] == f32(POISON)).all(), what


# (world, offset, conf, edge, stride, focal form, gathers): every option both ways, every stride, over the list
COMBOS = [(0, 0.0, 1, 0, 1, 0, 1), (1, 0.5, 0, 0, 2, 0, 0), (1, 0.0, 1, 0, 3, 1, 1), (0, 0.5, 0, 1, 1, 1, 0), (1, 0.5, 1, 1, 2, 0, 1),
          (0, 0.0, 0, 0, 3, 1, 0), (1, 0.0, 0, 1, 1, 0, 1), (0, 0.5, 1, 0, 2, 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(3, 70, 98), (2, 518, 518), (1, 1536, 1536), (2, 37, 53)])
def test_unproject_is_bit_identical_to_the_host_reference(dev, B, H, W):
    rng = np.random.default_rng(100 + H)
    K, E = _cameras(rng, B, H, W)
    focal = np.array([0.85 * W + 3 * b for b in range(B)], f32)
    rgb = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    noise_d, noise_c = _noise_scene(B, H, W)
    step = np.stack([_step_scene(H, W)[0] * f32(1 + 0.25 * b) for b in range(B)])
    step[:, H // 2, W // 3], step[:, H // 2 + 1, W // 3] = np.nan, 0.0
    combos = COMBOS if H < 1000 else COMBOS[:3] + COMBOS[4:5]
    for world, off, use_conf, edge, stride, focal_form, gather in combos:
        d = step if edge else noise_d
        conf = noise_c if use_conf else None
        kw = dict(pixel_offset=off, stride=stride, world=bool(world), edge_rtol=0.05 if edge else 0.0)
        if not edge:  # the randomised inputs: ranges that keep about half (see test_coverage_of_the_noise_scene)
            kw.update(depth_min=0.5, depth_max=6.0, conf_min=1.8) if use_conf else kw.update(depth_min=1.2, depth_max=3.0)
        elif use_conf:
            kw.update(conf_min=1.8)
        cams = dict(focal=focal) if focal_form else dict(K=K)
        ref = P.unproject_depth(d, intrinsics=cams.get("K"), focal_px=cams.get("focal"), extrinsics=E if world else None, conf=conf,
                                rgb=rgb if gather else None, **kw)
        if not edge:
            _assert_covered(ref)
        got = _run_op(dev, d, E=E if world else None, conf=conf, rgb=rgb if gather else None, **cams, **kw)
        if not (gather and use_conf):
            got["conf"] = None if not use_conf else got["conf"]
        _assert_same(got, ref, what=(world, off, use_conf, edge, stride, focal_form, gather))


@pytest.mark.gpu
def test_unproject_one_pixel(dev):
    for val, n in ((2.0, 1), (0.0, 0)):
        d = np.array([[[val]]], f32)
        for world in (False, True):
            E = np.array([[[0, 0, -1, 1], [0, 1, 0, 2], [1, 0, 0, 3]]], f32)
            ref = P.unproject_depth(d, focal_px=[3.0], extrinsics=E, world=world, pixel_offset=0.5)
            assert ref.count.tolist() == [n, n]
            _assert_same(_run_op(dev, d, focal=np.array([3.0], f32), E=E, world=world, pixel_offset=0.5), ref)


@pytest.mark.gpu
def test_compaction_edges(dev):
    B, H, W = 3, 70, 98
    K, E = _cameras(np.random.default_rng(1), B, H, W)
    d, c = _noise_scene(B, H, W)
    # all invalid: every count 0, xyz untouched
    got = _run_op(dev, np.zeros((B, H, W), f32), K=K)
    assert got["count"].tolist() == [0] * (B + 1) and (got["xyz"] == f32(POISON)).all() and not got["mask"].any()
    # all valid
    ones = np.full((B, H, W), 1.5, f32)
    got = _run_op(dev, ones, K=K, E=E, world=True)
    _assert_same(got, P.unproject_depth(ones, intrinsics=K, extrinsics=E, world=True))
    assert got["count"].tolist() == [H * W] * B + [B * H * W]
    # capacity = half the total: the first `capacity` entries, poison beyond them, the true totals in count
    kw = dict(depth_min=0.5, depth_max=6.0, conf_min=1.8)
    ref = P.unproject_depth(d, intrinsics=K, conf=c, **kw)
    _assert_covered(ref)
    cap = int(ref.count[-1]) // 2
    got = _run_op(dev, d, K=K, conf=c, capacity=cap, **kw)
    _assert_same(got, ref, capacity=cap)
    assert got["xyz"].shape[0] == cap and int(got["count"][-1]) > cap
    got = _run_op(dev, d, K=K, conf=c, capacity=0, **kw)
    assert np.array_equal(got["count"], ref.count)
    # one valid pixel, the last of the last view
    last = np.zeros((B, H, W), f32)
    last[-1, -1, -1] = 2.0
    got = _run_op(dev, last, K=K)
    ref = P.unproject_depth(last, intrinsics=K)
    assert ref.count.tolist() == [0, 0, 1, 1]
    _assert_same(got, ref)


@pytest.mark.gpu
def test_four_views_of_a_plane_fuse_onto_it(dev):
    """Independent of the numpy twin: a plane n.p = c seen by four cameras; the depth of a pixel is the ray-plane intersection
    in f64 (cameras taken at their f32 values, camera-to-world = R^T (p_c - t) as camera.rs:248-254 defines it); the device
    unprojects the f32-rounded depths. Error budget of n.p_w, first order in u = 2^-24: the depth's rounding (1), the
    back-projection (3), the subtraction of t (1), the rotation (3 multiplies + 2 adds over three terms: at most 3 per
    coordinate) -- 8 u on intermediates each bounded by M = |p_c|_1 + |t|_1, summed over the plane normal: |n|_1 8 u M; the
    test allows 1.01 of it for the second-order terms."""
    from burn_depth_amd import ops
    B, H, W = 4, 120, 160
    rng = np.random.default_rng(21)
    n, c = np.array([0.2, -0.3, 1.0]), 6.0
    K = np.zeros((B, 3, 3), f32)
    E = np.zeros((B, 3, 4), f32)
    angles = [(0.0, 0.0), (0.5, 0.1), (-0.4, 0.3), (1.3, -0.2)]  # the last one looks along the plane: part of its rays miss
    for b, (ay, ax) in enumerate(angles):
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        E[b, :, :3] = Ry @ Rx
        E[b, :, 3] = rng.uniform(-1, 1, 3)
        K[b] = [[110 + 5 * b, 0, W / 2], [0, 105 + 5 * b, H / 2], [0, 0, 1]]
    K64, E64 = K.astype(np.float64), E.astype(np.float64)
    v, u = np.mgrid[0:H, 0:W]
    depth = np.zeros((B, H, W))
    for b in range(B):
        R, t = E64[b, :, :3], E64[b, :, 3]
        ray = np.stack([(u - K64[b, 0, 2]) / K64[b, 0, 0], (v - K64[b, 1, 2]) / K64[b, 1, 1], np.ones((H, W))], -1)
        origin, direction = -R.T @ t, ray @ R  # rows of (ray @ R) = R^T ray
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (c - n @ origin) / (direction @ n)
        depth[b] = np.where(np.isfinite(s) & (s > 0) & (s < 60), s, 0.0)
    d32 = depth.astype(f32)
    hits = (d32 > 0).reshape(B, -1).sum(1)
    assert (hits[:3] > 0.9 * H * W).all() and 0 < hits[3] < 0.9 * H * W, hits  # the scene: three views see the plane, one grazes it
    pc = ops.unproject(dev, _t(d32), intrinsics=_t(K), extrinsics=_t(E), world=True, dense=False)
    torch.cuda.synchronize()
    assert pc.count.cpu().tolist() == hits.tolist() + [int(hits.sum())]
    xyz = pc.points()[0].cpu().numpy().astype(np.float64)
    assert xyz.shape[0] == hits.sum()
    view = np.repeat(np.arange(B), hits)
    dd = np.concatenate([depth[b][d32[b] > 0] for b in range(B)])
    rays = np.concatenate([np.stack([np.abs(u - K64[b, 0, 2]) / K64[b, 0, 0], np.abs(v - K64[b, 1, 2]) / K64[b, 1, 1], np.ones((H, W))], -1)[d32[b] > 0]
                           for b in range(B)])
    M = (rays * dd[:, None]).sum(1) + np.abs(E64[view, :, 3]).sum(1)
    err = np.abs(xyz @ n - c)
    assert (err <= 1.01 * np.abs(n).sum() * 8 * U * M).all(), float((err / M).max() / U)


# ---- the model call ----


def _rgb(B, S):
    return np.random.default_rng(4).integers(0, 256, (B, S, S, 3), dtype=np.uint8)


OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["F32", "BF16"])
def test_infer_points_da3_equals_infer_then_unproject(dev, precision):
    from burn_depth_amd import ops
    m = _da3(dev, "tiny_dual", precision)
    try:
        x = _image(2, 70).cuda()
        rgb = _rgb(2, 70)
        depth, conf, extr, intr = _da3_subset(m, x)
        cmin = float(conf.median())
        # the model's own cameras
        want = _cloud_np(ops.unproject(dev, depth, intrinsics=intr, extrinsics=extr, conf=conf, rgb=_t(rgb), world=True, conf_min=cmin, **OPTS))
        got = _cloud_np(m.infer_points(x, rgb=_t(rgb), world=True, conf_min=cmin, **OPTS))
        assert 0 < want["count"][-1] < 2 * 35 * 35
        assert np.array_equal(_bits(got["depth"]), _bits(depth.cpu().numpy()))
        _same_cloud(want, got, "own cameras")
        # (md_model_fork refuses Depth-Anything-v3 models: the fork is exercised on Depth Pro below)
        # the caller's cameras replace the model's; camera space needs no extrinsics
        K, E = _cameras(np.random.default_rng(2), 2, 70, 70)
        want = _cloud_np(ops.unproject(dev, depth, intrinsics=_t(K), extrinsics=_t(E), conf=conf, world=True, conf_min=cmin, **OPTS))
        _same_cloud(want, _cloud_np(m.infer_points(x, intrinsics=K, extrinsics=E, world=True, conf_min=cmin, **OPTS)), "caller cameras")
        want = _cloud_np(ops.unproject(dev, depth, focal_px=_t(np.array([80, 90], f32)), conf=conf, conf_min=cmin, **OPTS))
        _same_cloud(want, _cloud_np(m.infer_points(x, focal_px=[80.0, 90.0], conf_min=cmin, **OPTS)), "caller focal")
        # host in, host out
        hw = _cloud_np(ops.unproject(dev, depth, intrinsics=intr, extrinsics=extr, conf=conf, rgb=_t(rgb), world=True, conf_min=cmin, **OPTS))
        _same_cloud(hw, _host_call(m, x.cpu().numpy(), rgb, None, dict(world=True, conf_min=cmin, **OPTS), want_conf=True), "host")
    finally:
        m.destroy()


def _host_call(m, x, rgb, cams, opts, want_conf):
    """md_infer_points with every input and output in host memory -> numpy dict (poisoned beyond the points)."""
    from burn_depth_amd.points import _points_opts
    B, _, H, W = x.shape
    cap = B * H * W
    x = np.ascontiguousarray(x, f32)
    out = dict(point_map=np.full((B, H, W, 3), POISON, f32), mask=np.full((B, H, W), 77, np.uint8), xyz=np.full((cap, 3), POISON, f32),
               rgb=np.full((cap, 3), 77, np.uint8) if rgb is not None else None, conf=np.full(cap, POISON, f32) if want_conf else None,
               count=np.full(B + 1, -5, np.int32), depth=np.zeros((B, H, W), f32))
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = _points_opts(**opts)
    outs = _lib.MdPointsOutputs(ptr(out["point_map"]), ptr(out["mask"]), ptr(out["xyz"]), ptr(out["rgb"]), ptr(out["conf"]), ptr(out["count"]),
                                cap, ptr(out["depth"]))
    keep = [np.ascontiguousarray(a, f32) if a is not None else None for a in (cams or (None, None, None))]
    cam = _lib.MdPointsCameras(*(ptr(a) for a in keep))
    _lib.check(_lib.load().md_infer_points(m._h, C.c_void_p(x.ctypes.data), B, H, W, _lib.MD_MEM_HOST, C.c_void_p(ptr(rgb)),
                                           C.byref(cam) if cams else None, C.byref(o), C.byref(outs), _lib.MD_MEM_HOST, None))
    n = int(out["count"][-1])
    assert (out["xyz"][n:] == f32(POISON)).all()
    return out


@pytest.mark.gpu
def test_infer_points_da3_mono_needs_the_callers_cameras(dev):
    from burn_depth_amd import ops
    m = _da3(dev, "tiny", "BF16")
    try:
        x = _image(2, 70).cuda()
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x)
        assert e.value.code == _lib.MD_ERR_UNSUPPORTED
        with pytest.raises(_lib.MdError) as e:  # world space without extrinsics: nothing predicts them here
            m.infer_points(x, focal_px=80.0, world=True)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        K, _ = _cameras(np.random.default_rng(2), 2, 70, 70)
        depth = m.infer(x).depth
        want = _cloud_np(ops.unproject(dev, depth, intrinsics=_t(K), conf_min=5.0, **OPTS))  # conf_min is ignored: no confidence
        got = _cloud_np(m.infer_points(x, intrinsics=K, conf_min=5.0, **OPTS))
        assert want["count"][-1] > 0 and got["conf"] is None
        _same_cloud(want, got)
    finally:
        m.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["F32", "BF16"])
def test_infer_points_depth_pro_equals_infer_then_unproject(dev, precision):
    from burn_depth_amd import ops
    m = _pro(dev, "tiny", precision)
    fork = None
    try:
        x = _image(2, 512).cuda()
        rgb = _rgb(2, 512)
        ref = m.infer(x)
        want = _cloud_np(ops.unproject(dev, ref.depth, focal_px=ref.focallength_px, rgb=_t(rgb), **OPTS))
        got = _cloud_np(m.infer_points(x, rgb=_t(rgb), **OPTS))
        assert want["count"][-1] > 0 and np.array_equal(_bits(got["depth"]), _bits(ref.depth.cpu().numpy()))
        _same_cloud(want, got, "predicted focal")
        fork = m.fork()
        _same_cloud(want, _cloud_np(fork.infer_points(x, rgb=_t(rgb), **OPTS)), "fork")
        _same_cloud(want, _host_call(m, x.cpu().numpy(), rgb, None, OPTS, want_conf=False), "host")
        # a known focal length: infer(x, f_px) + the operator, and the FOV network does not run
        f = torch.tensor([400.0, 650.0], device="cuda")
        E = _cameras(np.random.default_rng(2), 2, 512, 512)[1]
        known = m.infer(x, f_px=f)
        want = _cloud_np(ops.unproject(dev, known.depth, focal_px=f, extrinsics=_t(E), world=True, **OPTS))
        _same_cloud(want, _cloud_np(m.infer_points(x, f_px=f, extrinsics=E, world=True, **OPTS)), "known focal")
        _same_cloud(want, _host_call(m, x.cpu().numpy(), None, (None, E, f.cpu().numpy()), dict(world=True, **OPTS), want_conf=False), "known focal, host")
        with pytest.raises(_lib.MdError) as e:  # Depth Pro predicts no extrinsics
            m.infer_points(x, world=True)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        m.enable_timing(True)
        m.read_timing()
        m.infer_points(x, f_px=f, **OPTS)
        torch.cuda.synchronize()
        known_names = m.read_launch_order()
        m.read_timing()
        m.infer_points(x, **OPTS)
        torch.cuda.synchronize()
        plain_names = m.read_launch_order()
        m.read_timing()
        m.enable_timing(False)
        assert any(n.startswith("fov_") for n in plain_names) and not [n for n in known_names if n.startswith("fov")], known_names
        assert known_names.count("points_unproject") == 1 and plain_names.count("points_unproject") == 1
    finally:
        if fork is not None:
            fork.destroy()
        m.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["da3", "pro"])
def test_infer_points_graph_replay_and_allocations(dev, model):
    m = _da3(dev, "tiny_dual", "BF16") if model == "da3" else _pro(dev, "tiny", "BF16")
    S = 70 if model == "da3" else 512
    try:
        x = _image(2, S).cuda()
        rgb = _t(_rgb(2, S))
        kw = dict(rgb=rgb, conf_min=1.0, world=model == "da3", **OPTS)
        eager = _cloud_np(m.infer_points(x, **kw))
        assert eager["count"][-1] > 0
        again = _cloud_np(m.infer_points(x, **kw))
        _same_cloud(eager, again, "two eager runs")  # the list order is deterministic
        m.enable_graph(True)
        out = m.infer_points(x, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (1, 2, 3, 4):  # 2: capture, 3 and 4: replay
            for t in (out.xyz, out.point_map, out.depth):
                t.fill_(POISON)
            out = m.infer_points(x, out=out, **kw)
            torch.cuda.synchronize()
            got = _cloud_np(out)
            _same_cloud(eager, got, f"graph call {call}")
            assert np.array_equal(_bits(got["depth"]), _bits(eager["depth"]))
        # a replay reads the inputs at run time
        x2 = _image(2, S, seed=1).cuda()
        want2 = _cloud_np(m.infer_points(x2, **kw))
        x.copy_(x2)
        _same_cloud(want2, _cloud_np(m.infer_points(x, out=out, **kw)), "replay on new pixels")
        # another option or pointer takes another graph (and still computes its own result)
        kw3 = dict(kw, stride=3)
        out3 = m.infer_points(x, **kw3)
        for _ in range(2):
            out3 = m.infer_points(x, out=out3, **kw3)
        torch.cuda.synchronize()
        got3 = _cloud_np(out3)
        assert got3["count"][-1] < want2["count"][-1]
        m.enable_graph(False)
        _same_cloud(_cloud_np(m.infer_points(x, **kw3)), got3, "stride 3")
        m.enable_graph(True)
        before = m.query("allocs")
        for _ in range(3):
            m.infer_points(x, out=out, **kw)
            m.infer_points(x, out=out3, **kw3)
        torch.cuda.synchronize()
        assert m.query("allocs") == before == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


@pytest.mark.gpu
def test_point_refusals_leave_the_outputs_untouched(dev):
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import PointCloud
    B, H, W = 2, 37, 53
    d, c = _noise_scene(B, H, W)
    K, E = _cameras(np.random.default_rng(1), B, H, W)
    rgb = _rgb(B, 53)[:, :H]

    def fresh():
        return PointCloud(point_map=torch.full((B, H, W, 3), POISON, device="cuda"), mask=torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda"),
                          xyz=torch.full((B * H * W, 3), POISON, device="cuda"), count=torch.full((B + 1,), -5, dtype=torch.int32, device="cuda"))

    cases = [dict(stride=0), dict(edge_rtol=float("nan")), dict(edge_rtol=-0.1), dict(conf_min=float("inf")), dict(depth_min=-1.0),
             dict(depth_max=float("nan")), dict(depth_min=3.0, depth_max=2.0), dict(pixel_offset=float("inf")), dict(world=True)]
    for kw in cases:
        out = fresh()
        with pytest.raises(_lib.MdError) as e:
            ops.unproject(dev, _t(d), intrinsics=_t(K), conf=_t(c), out=out, **kw)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, kw
        torch.cuda.synchronize()
        assert (out.point_map == POISON).all() and (out.xyz == POISON).all() and (out.count == -5).all() and (out.mask == 77).all(), kw
    for bad in (dict(xyz=None, count=None, rgb=torch.zeros(4, 3, dtype=torch.uint8, device="cuda")),  # compacted output without count
                dict(rgb=torch.zeros(4, 3, dtype=torch.uint8, device="cuda")),                       # rgb output without rgb input
                dict(conf=torch.zeros(4, device="cuda"))):                                          # conf output without a confidence map
        out = fresh()
        for k, v in bad.items():
            setattr(out, k, v)
        with pytest.raises(_lib.MdError) as e:
            ops.unproject(dev, _t(d), intrinsics=_t(K), out=out)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
        assert (out.point_map == POISON).all()
    out = fresh()
    with pytest.raises(_lib.MdError) as e:  # neither intrinsics nor a focal length
        ops.unproject(dev, _t(d), extrinsics=_t(E), out=out)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG and (out.point_map == POISON).all()
    # the model call: batch beyond max_batch, and the same option checks
    m = _da3(dev, "tiny_dual", "BF16", max_batch=1)
    try:
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(_image(2, 70).cuda())
        assert e.value.code == _lib.MD_ERR_SHAPE
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(_image(1, 70).cuda(), stride=0)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        with pytest.raises(_lib.MdError) as e:  # an rgb output without an rgb input
            m.infer_points(_image(1, 70).cuda(), out=PointCloud(xyz=torch.zeros(9, 3, device="cuda"), count=torch.zeros(2, dtype=torch.int32, device="cuda"),
                                                                  rgb=torch.zeros(9, 3, dtype=torch.uint8, device="cuda")))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
    finally:
        m.destroy()
    assert rgb.shape == (B, H, W, 3)


@pytest.mark.gpu
def test_infer_cli_writes_the_device_cloud_as_ply(dev, tmp_path):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.inference import rgb_to_input_tensor
    spec = importlib.util.spec_from_file_location("infer_cli", os.path.join(ROOT, "tools", "infer.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = DepthAnything3Config.small()
    ck = str(tmp_path / "da3_small.safetensors")
    Wt.save_container(ck, Wt.generate_da3_weights(cfg, 0, Wt.INIT_PARITY), dtype="F16")
    rgb = np.load(os.path.join(ROOT, "tests", "golden", "test_jpg_rgb.npy"))
    img = str(tmp_path / "img.npy")
    np.save(img, rgb)
    ply = str(tmp_path / "cloud.ply")
    assert cli.main(["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "2", "--edge-rtol", "0.5"]) == 0
    xyz, col = P.read_ply(ply)
    m = DepthAnything3.load_file(dev, cfg, ck)
    try:
        prep = P.prepare_depth_anything3_image(rgb, 518).rgb
        x = rgb_to_input_tensor(prep.tobytes(), 518, 518, dev)
        pc = m.infer_points(x, rgb=_t(prep[None]), dense=False, stride=2, edge_rtol=0.5, world=True)
        want_xyz, want_col, _ = pc.points()
    finally:
        m.destroy()
    assert cfg.precision == Precision.BF16 and xyz.shape[0] > 0
    assert np.array_equal(_bits(xyz), _bits(want_xyz.cpu().numpy())) and np.array_equal(col, want_col.cpu().numpy())
