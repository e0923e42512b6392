"""Surface normals and the grazing-angle filter of the point path: md_op_unproject_normals / md_infer_points_normals and their
host reference pipeline.unproject_depth(normals=True, normal_min_cos=...). include/mi_depth.h states the contract, DESIGN 12.2
the kernels.

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import functools
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
import points_util  # noqa: E402
from points_util import _bits, _cameras, _cloud_np, _da3, _da3_subset, _image, _pro, _t, dev, lib  # noqa: E402,F401

_same_cloud = functools.partial(points_util._same_cloud, normals=True)

f32 = np.float32
U = 2.0 ** -24  # unit roundoff of f32
NEW_ENTRIES = ("md_op_unproject_normals", "md_infer_points_normals")
MIN_COS = 0.5


def _scene(B, H, W, seed=11):
    """A wavy surface around depth 2.5 whose slope and noise are a few pixel footprints per pixel (they scale with 1 / size, as
    the footprint d / f does with f ~ 0.85 W), so the normals spread over every angle; 15 % of the pixels are 0, 15 % NaN and
    3 % lie at 9, beyond depth_max = 6. conf = 1 + 2 U(0,1)."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    base = 2.5 + 0.3 * np.sin(u * (3 * np.pi / W)) + 0.3 * np.cos(v * (3 * np.pi / H))
    d = np.stack([base * (1 + 0.1 * b) for b in range(B)]) * (1 + rng.normal(size=(B, H, W)) / max(H, W))
    r = rng.random((B, H, W))
    d = np.where(r < 0.15, 0.0, d)
    d = np.where((r >= 0.15) & (r < 0.30), np.nan, d)
    d = np.where((r >= 0.30) & (r < 0.33), 9.0, d)
    return d.astype(f32), (1 + 2 * rng.random((B, H, W))).astype(f32)


def _scene_opts(use_conf, edge):
    kw = dict(depth_min=0.5, depth_max=6.0, edge_rtol=0.05 if edge else 0.0)
    if use_conf:
        kw.update(conf_min=1.4)
    return kw


def _defined(normal_map):
    return (np.asarray(normal_map) != 0).any(-1)  # a defined normal has unit length


def _angle(a, b):
    """angle between the directions of a and b [..., 3], in f64, stable for small angles"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    b = b / np.linalg.norm(b, axis=-1, keepdims=True)
    return 2 * np.arcsin(np.clip(np.linalg.norm(a - b, axis=-1) / 2, 0, 1))


def _step_scene(H, W):
    """The step scene of tests/test_points.py: two planes (2 left of W/2, 5 right of it) plus a ramp of 0.002 per row, and a block
    of depth 1 inside the left plane."""
    v, u = np.mgrid[0:H, 0:W]
    d = np.where(u < W / 2, 2.0, 5.0) + 0.002 * v
    y0, x0, n = H // 7, W // 10 + 1, min(20, H // 3, W // 4)
    d[y0:y0 + n, x0:x0 + n] = 1.0
    return d.astype(f32), (y0, x0, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_normal_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "} md_points_normals;" in header
    assert [n for n, _ in _lib.MdPointsNormals._fields_] == ["normal_map", "normals", "min_cos"]


def test_reference_closed_forms_exact_in_f32():
    H, W = 16, 24
    K = np.array([[[128, 0, 12], [0, 128, 8], [0, 0, 1]]], f32)
    d = np.full((1, H, W), 2, f32)
    r = P.unproject_depth(d, intrinsics=K, normals=True)
    assert r.normal_map.dtype == f32 and r.normal_map.shape == (1, H, W, 3)
    # a fronto-parallel plane: (0, 0, -1) everywhere, the border pixels (two pairs) and the corners (one) included
    assert (r.normal_map[..., :2] == 0).all() and (r.normal_map[..., 2] == -1).all()
    assert np.array_equal(r.normals, r.normal_map.reshape(-1, 3)) and r.mask.all()
    # the corners use exactly one pair: taking its second neighbour away leaves no pair, taking any other pixel away changes nothing
    for (cv, cu), ring in (((0, 0), [(0, 1), (1, 0)]), ((0, W - 1), [(0, W - 2), (1, W - 1)]), ((H - 1, 0), [(H - 2, 0), (H - 1, 1)]),
                           ((H - 1, W - 1), [(H - 1, W - 2), (H - 2, W - 1)])):
        for nb in ring:
            d2 = d.copy()
            d2[0][nb] = 0
            assert not _defined(P.unproject_depth(d2, intrinsics=K, normals=True).normal_map)[0, cv, cu]
        d2 = np.zeros_like(d)
        d2[0, cv, cu] = 2
        for nb in ring:
            d2[0][nb] = 2
        assert P.unproject_depth(d2, intrinsics=K, normals=True).normal_map[0, cv, cu].tolist() == [0, 0, -1]
    # the defaults are the call without normals
    r0 = P.unproject_depth(d, intrinsics=K)
    assert r0.normal_map is None and r0.normals is None
    # world: R = a quarter turn about Y; n_w = R^T (0, 0, -1) = -(row 2 of R)
    E = np.array([[[0, 0, -1, 1], [0, 1, 0, 2], [1, 0, 0, 3]]], f32)
    rw = P.unproject_depth(d, intrinsics=K, extrinsics=E, world=True, normals=True)
    assert (rw.normal_map == np.array([-1, 0, 0], f32)).all()
    # no pair: one pixel, one row, one column
    for shape in ((1, 1, 1), (1, 1, 9), (1, 9, 1)):
        one = np.full(shape, 2, f32)
        r = P.unproject_depth(one, focal_px=[8.0], normals=True)
        assert r.mask.all() and not r.normal_map.any() and not r.normals.any() and r.normals.shape == (one.size, 3)
        r = P.unproject_depth(one, focal_px=[8.0], normals=True, normal_min_cos=1e-3)
        assert not r.mask.any() and r.count.tolist() == [0, 0] and r.xyz.shape == (0, 3) and r.normals.shape == (0, 3)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            P.unproject_depth(d, intrinsics=K, normals=True, normal_min_cos=bad)


def test_every_defined_normal_faces_the_camera():
    """For positive depths the sign of P_c . (e_a x e_b) is the sign of det(r_c, r_a, r_b) of the pixel rays: it does not depend on
    the depths, so cosv > 0 for every defined normal, however rough the surface. Evaluated in f64 on pure noise."""
    B, H, W = 2, 37, 53
    rng = np.random.default_rng(7)
    d = np.exp(rng.normal(0.5, 0.6, (B, H, W)))
    d[rng.random((B, H, W)) < 0.2] = 0
    K, _ = _cameras(rng, B, H, W)
    for off in (0.0, 0.5):
        r = P.unproject_depth(d, intrinsics=K, pixel_offset=off, normals=True, dtype=np.float64)
        de = _defined(r.normal_map)
        assert de.sum() > 0.5 * B * H * W
        cosv = -(r.normal_map * r.point_map).sum(-1)[de] / np.linalg.norm(r.point_map[de], axis=-1)
        assert (cosv > 0).all() and cosv.min() < 0.05 and cosv.max() > 0.9, (cosv.min(), cosv.max())
        assert np.abs(np.linalg.norm(r.normal_map[de], axis=-1) - 1).max() < 1e-14


def _plane_depth(K, E, n, c, H, W):
    """f64 depth of the world plane n.p = c along the pixel rays of the cameras (K, E at their f32 values)"""
    B = K.shape[0]
    K64, E64 = K.astype(np.float64), E.astype(np.float64)
    v, u = np.mgrid[0:H, 0:W]
    depth = np.zeros((B, H, W))
    for b in range(B):
        R, t = E64[b, :, :3], E64[b, :, 3]
        ray = np.stack([(u - K64[b, 0, 2]) / K64[b, 0, 0], (v - K64[b, 1, 2]) / K64[b, 1, 1], np.ones((H, W))], -1)
        depth[b] = (c - n @ (-R.T @ t)) / ((ray @ R) @ n)
    return depth


def _angle_bounds(pm):
    """Per interior pixel of a camera-space f64 point map [B,H,W,3] of a plane: (arithmetic, input) bounds on the angle error
    of the normal, first order in u = 2^-24.

    A camera-space coordinate carries 3 u of its magnitude (tests/test_points.py), so |dP| <= 3 u |P|, and the edge
    e = P_n - P_c, one more rounded subtraction, |de| <= 3 u (|P_n| + |P_c|) + u |e|: the cancellation term 3 u (|P_n| + |P_c|) / |e|
    dominates. A cross a x b of edges with errors da, db is off by at most |da||b| + |a||db|, plus its own roundings: a
    component (ay bz) - (az by) carries 2 u (|ay bz| + |az by|) <= 2 u |a||b|, the vector 2 sqrt(3) u |a||b|. Relative to
    |a x b| = |a||b| sin(phi): (|da|/|a| + |db|/|b| + 2 sqrt(3) u) / sin(phi). On a plane every cross is parallel to the
    normal, so the sum's relative error is at most the largest of its terms' plus sqrt(3) u for each of the 3 additions; the
    normalisation scales the vector (no angle) up to the final division's u per component, sqrt(3) u; so the angle is at most
    max over the pairs + 4 sqrt(3) u. The input bound is the same propagation for the rounding of the depth to f32, which moves a
    point by u |P| along its ray: |de| <= u (|P_n| + |P_c|)."""
    c = pm[:, 1:-1, 1:-1]
    ring = {"E": pm[:, 1:-1, 2:], "S": pm[:, 2:, 1:-1], "W": pm[:, 1:-1, :-2], "N": pm[:, :-2, 1:-1]}
    nc = np.linalg.norm(c, axis=-1)
    e = {k: q - c for k, q in ring.items()}
    ne = {k: np.linalg.norm(e[k], axis=-1) for k in e}
    arith = {k: (3 * U * (np.linalg.norm(ring[k], axis=-1) + nc) + U * ne[k]) / ne[k] for k in e}
    inp = {k: U * (np.linalg.norm(ring[k], axis=-1) + nc) / ne[k] for k in e}
    ba, bi = 0, 0
    for a, b in (("S", "E"), ("E", "N"), ("N", "W"), ("W", "S")):
        sin = np.linalg.norm(np.cross(e[a], e[b]), axis=-1) / (ne[a] * ne[b])
        ba = np.maximum(ba, (arith[a] + arith[b] + 2 * np.sqrt(3) * U) / sin)
        bi = np.maximum(bi, (inp[a] + inp[b]) / sin)
    return 1.01 * (ba + 4 * np.sqrt(3) * U), 1.01 * bi


def _tilted_plane_scene(B=2, H=48, W=64):
    """One world plane seen by B cameras at 30-60 degrees to their view axes, focal length 1.2 W: a pixel's footprint is
    d / f ~ 1/77 of its depth, so the edge vectors are not tiny against the points."""
    n = np.array([0.0, 0.0, 1.0])
    K = np.zeros((B, 3, 3), f32)
    E = np.zeros((B, 3, 4), f32)
    for b, (ay, ax) in enumerate([(np.radians(40), np.radians(10)), (np.radians(-50), np.radians(-15))][:B]):
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        E[b, :, :3] = Ry @ Rx
        E[b, :, 3] = [0.3 * b, -0.2, 0.1 + 0.2 * b]
        K[b] = [[1.2 * W + 2 * b, 0, W / 2], [0, 1.2 * W + b, H / 2], [0, 0, 1]]
    depth = _plane_depth(K, E, n, 4.0, H, W)
    assert (depth > 1).all() and (depth < 40).all()
    tilt = np.degrees(np.arccos(np.abs(E[:, :, :3].astype(np.float64) @ n)[:, 2]))
    assert ((tilt > 30) & (tilt < 60)).all(), tilt
    return n, K, E, depth


def test_reference_f32_against_f64_with_a_derived_bound():
    """The angle between the f32 and the f64 normals, and between both and the analytic plane normal, against the bounds
    _angle_bounds derives from the cancellation in the edge vectors. world = 1 adds R^T: 3 multiplies and 2 additions per
    coordinate of a unit vector, at most 5 u each, 5 sqrt(3) u on the angle (allowed: 10 u)."""
    n, K, E, depth = _tilted_plane_scene()
    d32 = depth.astype(f32)
    inner = (slice(None), slice(1, -1), slice(1, -1))
    for world in (False, True):
        kw = dict(intrinsics=K, extrinsics=E, world=world, normals=True)
        a = P.unproject_depth(d32, **kw)
        b = P.unproject_depth(d32, dtype=np.float64, **kw)
        assert a.normal_map.dtype == f32 and _defined(a.normal_map).all() and _defined(b.normal_map).all()
        arith, inp = _angle_bounds(P.unproject_depth(d32, intrinsics=K, dtype=np.float64).point_map)
        rot = 10 * U if world else 0.0
        R = E[:, :, :3].astype(np.float64)
        want = np.stack([-(n if world else R[i] @ n) * np.sign((R[i] @ n)[2]) for i in range(K.shape[0])])[:, None, None, :]
        ab = _angle(a.normal_map, b.normal_map)[inner]
        assert (ab <= arith + rot).all(), float((ab / (arith + rot)).max())
        assert ab.max() > 2 * U  # the scene does exercise the cancellation
        b_true = _angle(b.normal_map, want)[inner]
        assert (b_true <= inp + 1e-12).all(), float((b_true / inp).max())
        a_true = _angle(a.normal_map, want)[inner]
        assert (a_true <= arith + inp + rot).all(), float((a_true / (arith + inp + rot)).max())


def test_planted_unusable_neighbours_remove_exactly_their_two_pairs():
    """A 3 x 3 patch of a slanted surface; the centre's normal with neighbour X made unusable equals the sum of the two pairs
    that do not contain X, recomputed here from the point map of the intact patch."""
    rng = np.random.default_rng(2)
    d = (2 + 0.05 * rng.random((1, 3, 3))).astype(f32)
    c = np.full((1, 3, 3), 3, f32)
    kw = dict(focal_px=[6.0], conf=c, depth_min=0.5, depth_max=6.0, conf_min=1.5)
    pm = P.unproject_depth(d, **kw).point_map[0]
    pos = {"E": (1, 2), "S": (2, 1), "W": (1, 0), "N": (0, 1)}
    e = {k: pm[vu] - pm[1, 1] for k, vu in pos.items()}

    def expect(dead):
        m = None
        for a, b in (("S", "E"), ("E", "N"), ("N", "W"), ("W", "S")):
            if a in dead or b in dead:
                continue
            x = np.array([(e[a][1] * e[b][2]) - (e[a][2] * e[b][1]), (e[a][2] * e[b][0]) - (e[a][0] * e[b][2]),
                          (e[a][0] * e[b][1]) - (e[a][1] * e[b][0])], f32)
            m = x if m is None else m + x
        return m / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])

    full = P.unproject_depth(d, normals=True, **kw)
    assert np.array_equal(_bits(full.normal_map[0, 1, 1]), _bits(expect(())))
    causes = {"below depth_min": ("d", 0.25), "above depth_max": ("d", 9.0), "nan": ("d", np.nan), "inf": ("d", np.inf), "zero": ("d", 0.0),
              "low confidence": ("c", 1.25)}
    for name, (what, val) in causes.items():
        for k, vu in pos.items():
            d2, c2 = d.copy(), c.copy()
            (d2 if what == "d" else c2)[0][vu] = val
            r = P.unproject_depth(d2, normals=True, **dict(kw, conf=c2))
            assert r.mask[0, 1, 1] == 1 and np.array_equal(_bits(r.normal_map[0, 1, 1]), _bits(expect((k,)))), (name, k)
            assert not np.array_equal(_bits(r.normal_map[0, 1, 1]), _bits(full.normal_map[0, 1, 1])), (name, k)
    # the edge test: a neighbour 10 % nearer. Without edge_rtol it is used. With edge_rtol = 0.05 the point path's own edge test
    # (symmetric in the two depths) already drops the centre, so its normal is 0 in every output; that the neighbour test then
    # removes exactly the two pairs shows on the reference's per-pixel function, which does not look at the centre's validity.
    tiny = f32(np.finfo(f32).tiny)
    for k, vu in pos.items():
        d2 = d.copy()
        d2[0][vu] = d[0][vu] * f32(0.9)
        r = P.unproject_depth(d2, normals=True, **kw)
        assert _defined(r.normal_map)[0, 1, 1] and not np.array_equal(_bits(r.normal_map[0, 1, 1]), _bits(expect((k,))))
        pts = tuple(r.point_map[..., i] for i in range(3))
        with np.errstate(all="ignore"):
            n, defined, _ = P._pixel_normals(d2, c, pts, f32(0.5), f32(6.0), f32(1.5), f32(0.05), tiny)
        assert defined[0, 1, 1] and np.array_equal(_bits(np.array([x[0, 1, 1] for x in n])), _bits(expect((k,)))), k
        r = P.unproject_depth(d2, normals=True, edge_rtol=0.05, **kw)
        assert r.mask[0, 1, 1] == 0 and not r.normal_map[0, 1, 1].any()


def test_edge_test_keeps_each_side_of_the_step_on_its_own_plane():
    """The step scene of tests/test_points.py, planes d = d0 + 0.002 v with d0 = 2 left of column W/2 and 5 right of it. With
    edge_rtol = 0.05 the two rim columns W/2 - 1 and W/2 are dropped (normal 0) and the columns beside them, W/2 - 2 and W/2 + 1,
    carry their own side's plane normal. Without edge_rtol the rim pixels are valid and their normals lean across the step."""
    H, W = 70, 98
    d, _ = _step_scene(H, W)
    with_edge = P.unproject_depth(d[None], focal_px=[100.0], edge_rtol=0.05, normals=True)
    without = P.unproject_depth(d[None], focal_px=[100.0], normals=True)
    rows = slice(40, 60)  # clear of the block

    def plane_normal(v, u, d0):  # P(v, u) = ((u - W/2) / f, (v - H/2) / f, 1) (d0 + 0.002 v): the cross of its two tangents
        f, dd = 100.0, d0 + 0.002 * v
        tu = np.array([dd / f, 0, 0])
        tv = np.array([(u - W / 2) / f * 0.002, dd / f + (v - H / 2) / f * 0.002, 0.002])
        return np.cross(tv, tu)

    for v in (40, 50, 59):
        for u, d0 in ((W // 2 - 2, 2.0), (W // 2 + 1, 5.0)):
            assert with_edge.mask[0, v, u] == 1 and _angle(with_edge.normal_map[0, v, u], plane_normal(v, u, d0)) < 1e-3
        for u, d0 in ((W // 2 - 1, 2.0), (W // 2, 5.0)):
            assert without.mask[0, v, u] == 1 and _angle(without.normal_map[0, v, u], plane_normal(v, u, d0)) > 0.5
    assert not with_edge.mask[0, rows, W // 2 - 1:W // 2 + 1].any() and not with_edge.normal_map[0, rows, W // 2 - 1:W // 2 + 1].any()


# (world, offset, conf, edge, stride, focal form, min_cos): every option both ways
COMBOS = [(0, 0.0, 1, 0, 1, 0, 0), (1, 0.5, 0, 0, 3, 0, 1), (1, 0.0, 1, 1, 3, 1, 1), (0, 0.5, 0, 1, 1, 1, 0), (1, 0.5, 1, 0, 1, 0, 1),
          (0, 0.0, 0, 1, 3, 1, 1)]
SHAPES = [(2, 37, 53), (3, 70, 98), (1, 64, 64)]
DEGENERATE = [(1, 1, 1), (1, 1, 130), (1, 130, 1)]


def _reference(d, c, K, E, focal, combo, **extra):
    world, off, use_conf, edge, stride, focal_form, mc = combo
    kw = dict(pixel_offset=off, stride=stride, world=bool(world), normals=True, normal_min_cos=MIN_COS if mc else 0.0, **_scene_opts(use_conf, edge))
    kw.update(extra)
    cams = dict(focal_px=focal) if focal_form else dict(intrinsics=K)
    return kw, cams, P.unproject_depth(d, extrinsics=E if world else None, conf=c if use_conf else None, **cams, **kw)


def test_coverage_of_the_scene_used_on_the_gpu():
    """Every share lies in [0.1, 0.9]: pixels with a defined normal among the candidates (the valid pixels of the point path),
    pixels min_cos keeps among those with a defined normal, pixels kept overall."""
    for B, H, W in SHAPES:
        d, c = _scene(B, H, W)
        K, E = _cameras(np.random.default_rng(100 + H), B, H, W)
        focal = np.array([0.85 * W + 3 * b for b in range(B)], f32)
        for combo in COMBOS:
            kw, cams, off = _reference(d, c, K, E, focal, combo, normal_min_cos=0.0)
            _, _, on = _reference(d, c, K, E, focal, combo, normal_min_cos=MIN_COS)
            cand, de = off.mask.astype(bool), _defined(off.normal_map)
            assert not (de & ~cand).any() and not (on.mask.astype(bool) & ~de).any()
            shares = (de.sum() / cand.sum(), on.mask.sum() / de.sum(), on.mask.mean())
            assert all(0.1 <= s <= 0.9 for s in shares), (B, H, W, combo, shares)


def test_ply_round_trip_with_normals(tmp_path):
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(257, 3)).astype(f32)
    nrm = rng.normal(size=(257, 3)).astype(f32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    path = str(tmp_path / "cloud.ply")
    for col in (None, rgb):
        P.write_ply(path, xyz, col, normals=nrm)
        head = open(path, "rb").read(200).decode("ascii", "replace")
        assert "property float nx\nproperty float ny\nproperty float nz\n" in head
        x2, c2, n2 = P.read_ply_normals(path)
        assert np.array_equal(_bits(x2), _bits(xyz)) and np.array_equal(_bits(n2), _bits(nrm))
        assert (c2 is None) if col is None else np.array_equal(c2, col)
        x3, c3 = P.read_ply(path)  # the two-value reader skips the normals
        assert np.array_equal(_bits(x3), _bits(xyz)) and ((c3 is None) if col is None else np.array_equal(c3, col))
    P.write_ply(path, xyz, rgb)  # a file without normals reads as before
    x2, c2, n2 = P.read_ply_normals(path)
    assert n2 is None and np.array_equal(_bits(x2), _bits(xyz)) and np.array_equal(c2, rgb)
    assert b"nx" not in open(path, "rb").read(200)
    with pytest.raises(ValueError):
        P.write_ply(path, xyz, normals=nrm[:5])


def test_normal_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched. With a null device each call ends in MD_ERR_INVALID_ARG whatever it
    is refused for, so the reason is read from md_last_error: a bad argument is refused for itself, the valid call last, for
    the null device."""
    buf = (C.c_float * 64)()
    px = C.cast(buf, C.c_void_p)
    cam = _lib.MdPointsCameras(px.value, px.value, None)
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    E = _lib.MD_ERR_INVALID_ARG
    dense = _lib.MdPointsOutputs(px.value, None, None, None, None, None, 0, None)
    listed = _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, 4, None)

    def why(nrm, out=dense, opts=o):
        rc = lib.md_op_unproject_normals(None, px, None, None, 1, 2, 2, C.byref(cam), C.byref(opts), C.byref(out), C.byref(nrm) if nrm else None, None)
        assert rc == E
        return lib.md_last_error().decode()

    for bad in (float("nan"), float("inf"), -0.25, 1.5):
        assert "min_cos" in why(_lib.MdPointsNormals(px.value, None, bad)), bad
        assert "min_cos" in why(_lib.MdPointsNormals(None, None, bad), listed), bad
    assert "normals need `count`" in why(_lib.MdPointsNormals(None, px.value, 0.0))  # normals without count
    for ok in (_lib.MdPointsNormals(px.value, None, 1.0), _lib.MdPointsNormals(px.value, None, 0.0), None):
        assert "device is null" in why(ok)  # valid: the null device, after everything else
    assert "device is null" in why(_lib.MdPointsNormals(None, px.value, 0.5), listed)
    assert "stride" in why(None, listed, _lib.MdPointsOpts(0, 0, 0, 0, 0, 0, 0))  # the point path's own refusals still apply
    nrm = _lib.MdPointsNormals(px.value, None, 2.0)
    assert lib.md_infer_points_normals(None, px, 1, 2, 2, 1, None, None, None, C.byref(o), C.byref(listed), C.byref(nrm), 1, None) == E
    assert "model is null" in lib.md_last_error().decode()
    assert (np.frombuffer(buf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0
CANARY = 16  # elements behind the end of every output buffer


def _guarded(shape, fill, dtype=torch.float32):
    """(a tensor of `shape` filled with `fill`, its backing store with CANARY more elements behind it)"""
    n = int(np.prod(shape))
    store = torch.full((n + CANARY,), fill, dtype=dtype, device="cuda")
    return store[:n].view(shape), store


def _fresh(B, H, W, cap, rgb, conf, normals=True):
    from burn_depth_amd.depth_pro import PointCloud
    out, stores = PointCloud(), {}

    def put(name, shape, fill, dtype=torch.float32):
        t, stores[name] = _guarded(shape, fill, dtype)
        setattr(out, name, t)

    put("point_map", (B, H, W, 3), POISON)
    put("mask", (B, H, W), 77, torch.uint8)
    put("xyz", (cap, 3), POISON)
    put("count", (B + 1,), -5, torch.int32)
    if rgb:
        put("rgb", (cap, 3), 77, torch.uint8)
    if conf:
        put("conf", (cap,), POISON)
    if normals:
        put("normal_map", (B, H, W, 3), POISON)
        put("normals", (cap, 3), POISON)
    return out, stores


def _canaries_intact(out, stores):
    fills = dict(point_map=POISON, mask=77, xyz=POISON, count=-5, rgb=77, conf=POISON, normal_map=POISON, normals=POISON)
    for name, store in stores.items():
        assert (store[-CANARY:] == fills[name]).all(), name


def _run_op(dev, d, K=None, E=None, focal=None, conf=None, rgb=None, capacity=None, normals=True, **opts):
    """ops.unproject on poisoned, guarded outputs -> numpy dict."""
    from burn_depth_amd import ops
    B, H, W = d.shape
    cap = B * H * W if capacity is None else capacity
    out, stores = _fresh(B, H, W, cap, rgb is not None, conf is not None, normals)
    ops.unproject(dev, _t(d), intrinsics=_t(K), extrinsics=_t(E), focal_px=_t(focal), conf=_t(conf), rgb=_t(rgb), out=out, **opts)
    torch.cuda.synchronize()
    _canaries_intact(out, stores)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(out).items()}


def _assert_same(got, ref, capacity=None, what=""):
    assert np.array_equal(got["count"], ref.count), (what, got["count"], ref.count)
    assert np.array_equal(got["mask"], ref.mask), what
    assert np.array_equal(_bits(got["point_map"]), _bits(ref.point_map)), what
    assert np.array_equal(_bits(got["normal_map"]), _bits(ref.normal_map)), what
    n = int(ref.count[-1]) if capacity is None else min(int(ref.count[-1]), capacity)
    for k in ("xyz", "normals"):
        assert np.array_equal(_bits(got[k][:n]), _bits(getattr(ref, k)[:n])), (what, k)
        assert (got[k][n:] == f32(POISON)).all(), (what, k)
    if got["rgb"] is not None:
        assert np.array_equal(got["rgb"][:n], ref.rgb[:n]) and (got["rgb"][n:] == 77).all(), what
    if got["conf"] is not None:
        assert np.array_equal(_bits(got["conf"][:n]), _bits(ref.conf[:n])) and (got["conf"][n:] == f32(POISON)).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", SHAPES + DEGENERATE)
def test_normals_are_bit_identical_to_the_host_reference(dev, B, H, W):
    rng = np.random.default_rng(100 + H)
    K, E = _cameras(rng, B, H, W)
    focal = np.array([0.85 * W + 3 * b for b in range(B)], f32)
    rgb = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    d, c = _scene(B, H, W)
    for combo in COMBOS:
        kw, cams, ref = _reference(d, c, K, E, focal, combo, rgb=rgb)
        world, _, use_conf = combo[:3]
        if (B, H, W) in SHAPES:
            assert 0 < ref.count[-1] and _defined(ref.normal_map).any()
        kw.pop("rgb")
        got = _run_op(dev, d, K=cams.get("intrinsics"), focal=cams.get("focal_px"), E=E if world else None, conf=c if use_conf else None, rgb=rgb, **kw)
        _assert_same(got, ref, what=combo)


@pytest.mark.gpu
def test_null_and_all_zero_normals_are_the_call_without_them(dev, lib):
    B, H, W = 2, 37, 53
    d, c = _scene(B, H, W)
    K, E = _cameras(np.random.default_rng(1), B, H, W)
    rgb = np.random.default_rng(4).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    kw = dict(pixel_offset=0.5, stride=2, world=True, **_scene_opts(True, True))
    want = _run_op(dev, d, K=K, E=E, conf=c, rgb=rgb, normals=False, **kw)
    assert want["count"][-1] > 0
    from burn_depth_amd.depth_pro import _stream_ptr
    from burn_depth_amd.points import _points_cameras, _points_opts, _points_outputs
    td, tc, trgb = _t(d), _t(c), _t(rgb)
    for nrm in (None, _lib.MdPointsNormals(None, None, 0.0)):
        out, stores = _fresh(B, H, W, B * H * W, True, True, normals=False)
        _, outs = _points_outputs(td.device, B, H, W, True, True, None, 2, True, True, False, out)
        cam, keep = _points_cameras(td.device, B, K, E, None)
        o = _points_opts(**kw)
        _lib.check(lib.md_op_unproject_normals(dev.handle, td.data_ptr(), tc.data_ptr(), trgb.data_ptr(), B, H, W, C.byref(cam), C.byref(o),
                                               C.byref(outs), C.byref(nrm) if nrm is not None else None, _stream_ptr(dev.ordinal)))
        torch.cuda.synchronize()
        _canaries_intact(out, stores)
        for k in ("point_map", "mask", "xyz", "rgb", "conf", "count"):
            assert np.array_equal(getattr(out, k).cpu().numpy().view(np.uint8), want[k].view(np.uint8)), (k, nrm is None)


@pytest.mark.gpu
def test_list_rows_equal_the_dense_map_and_capacity_cuts_the_list(dev):
    B, H, W = 3, 70, 98
    d, c = _scene(B, H, W)
    K, E = _cameras(np.random.default_rng(1), B, H, W)
    kw = dict(pixel_offset=0.5, stride=3, world=True, normal_min_cos=MIN_COS, **_scene_opts(True, False))
    full = _run_op(dev, d, K=K, E=E, conf=c, **kw)
    total = int(full["count"][-1])
    assert total > 100
    # the pixel of a row, from the mask and the stride alone
    sel = full["mask"].astype(bool)
    keep = np.zeros((H, W), bool)
    keep[::3, ::3] = True
    sel &= keep[None]
    assert sel.sum() == total
    assert np.array_equal(_bits(full["xyz"][:total]), _bits(full["point_map"][sel]))
    assert np.array_equal(_bits(full["normals"][:total]), _bits(full["normal_map"][sel]))
    assert _defined(full["normals"][:total]).all()  # min_cos > 0: every listed pixel has a normal
    cap = total // 2
    cut = _run_op(dev, d, K=K, E=E, conf=c, capacity=cap, **kw)
    assert np.array_equal(cut["count"], full["count"]) and cut["normals"].shape[0] == cap
    assert np.array_equal(_bits(cut["normals"]), _bits(full["normals"][:cap])) and np.array_equal(_bits(cut["xyz"]), _bits(full["xyz"][:cap]))
    # the list alone (no dense outputs): the scatter form recomputes what classify would have written
    from burn_depth_amd import ops
    pc = ops.unproject(dev, _t(d), intrinsics=_t(K), extrinsics=_t(E), conf=_t(c), dense=False, normals=True, **kw)
    torch.cuda.synchronize()
    assert pc.normal_map is None and np.array_equal(_bits(pc.normals[:total].cpu().numpy()), _bits(full["normals"][:total]))
    # the dense map alone
    pc = ops.unproject(dev, _t(d), intrinsics=_t(K), extrinsics=_t(E), conf=_t(c), compact=False, normals=True, **kw)
    torch.cuda.synchronize()
    assert pc.normals is None and np.array_equal(_bits(pc.normal_map.cpu().numpy()), _bits(full["normal_map"]))


@pytest.mark.gpu
def test_two_views_of_a_tilted_plane_agree_on_its_world_normal(dev):
    """Independent of the numpy twin: the depths are ray-plane intersections in f64, the expected normal is the plane's, turned
    towards each camera. Fails when R^T, the pair order or the orientation is wrong. Bounds: test 4's (_angle_bounds)."""
    from burn_depth_amd import ops
    n, K, E, depth = _tilted_plane_scene()
    d32 = depth.astype(f32)
    pc = ops.unproject(dev, _t(d32), intrinsics=_t(K), extrinsics=_t(E), world=True, normals=True, compact=False)
    torch.cuda.synchronize()
    got = pc.normal_map.cpu().numpy()
    assert pc.mask.cpu().numpy().all() and _defined(got).all()
    arith, inp = _angle_bounds(P.unproject_depth(d32, intrinsics=K, dtype=np.float64).point_map)
    R = E[:, :, :3].astype(np.float64)
    for b in range(2):
        want = -n * np.sign((R[b] @ n)[2])  # the side of the plane that faces camera b
        err = _angle(got[b], want)[1:-1, 1:-1]
        lim = (arith + inp)[b] + 10 * U
        assert (err <= lim).all(), float((err / lim).max())
    assert _angle(got[0, 5, 5], got[1, 20, 30]) < 1e-4  # both cameras stand on the same side here: one normal


# ---- the model call ----


OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
NRM = dict(normals=True, normal_min_cos=0.05)


def _host_call(m, x, opts, min_cos, want_conf):
    """md_infer_points_normals with every input and output in host memory -> numpy dict (poisoned beyond the points)."""
    from burn_depth_amd.points import _points_opts
    B, _, H, W = x.shape
    cap = B * H * W
    x = np.ascontiguousarray(x, f32)
    out = dict(point_map=np.full((B, H, W, 3), POISON, f32), mask=np.full((B, H, W), 77, np.uint8), xyz=np.full((cap, 3), POISON, f32), rgb=None,
               conf=np.full(cap, POISON, f32) if want_conf else None, count=np.full(B + 1, -5, np.int32), depth=np.zeros((B, H, W), f32),
               normal_map=np.full((B, H, W, 3), POISON, f32), normals=np.full((cap, 3), POISON, f32))
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = _points_opts(**opts)
    outs = _lib.MdPointsOutputs(ptr(out["point_map"]), ptr(out["mask"]), ptr(out["xyz"]), None, ptr(out["conf"]), ptr(out["count"]), cap,
                                ptr(out["depth"]))
    nrm = _lib.MdPointsNormals(ptr(out["normal_map"]), ptr(out["normals"]), min_cos)
    _lib.check(_lib.load().md_infer_points_normals(m._h, C.c_void_p(x.ctypes.data), B, H, W, _lib.MD_MEM_HOST, None, None, None, C.byref(o),
                                                   C.byref(outs), C.byref(nrm), _lib.MD_MEM_HOST, None))
    n = int(out["count"][-1])
    assert (out["xyz"][n:] == f32(POISON)).all() and (out["normals"][n:] == f32(POISON)).all()  # only the rows that exist travel
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["F32", "BF16"])
def test_infer_points_normals_da3_equals_infer_filter_unproject(dev, precision):
    from burn_depth_amd import ops
    m = _da3(dev, precision=precision)
    try:
        x = _image(2, 70).cuda()
        depth, conf, extr, intr = _da3_subset(m, x)
        cmin = float(conf.median())
        kw = dict(world=True, conf_min=cmin, **OPTS, **NRM)
        want = _cloud_np(ops.unproject(dev, depth, intrinsics=intr, extrinsics=extr, conf=conf, **kw))
        got = _cloud_np(m.infer_points(x, **kw))
        assert 0 < want["count"][-1] < 2 * 35 * 35 and _defined(want["normals"][:int(want["count"][-1])]).all()
        _same_cloud(want, got, "no filter")
        _same_cloud(want, _host_call(m, x.cpu().numpy(), dict(world=True, conf_min=cmin, **OPTS), NRM["normal_min_cos"], True), "host")
        # with the view filter in front
        fkw = dict(conf_percentile=30, view_rtol=0.5, min_views=1)
        fdepth, _, _, _ = ops.filter_views(dev, depth, conf, intrinsics=intr, extrinsics=extr, pixel_offset=0.5, **fkw)
        kw = dict(world=True, **OPTS, **NRM)
        want = _cloud_np(ops.unproject(dev, fdepth, intrinsics=intr, extrinsics=extr, conf=conf, **kw))
        got = _cloud_np(m.infer_points(x, **fkw, **kw))
        assert np.array_equal(_bits(got["depth"]), _bits(fdepth.cpu().numpy()))
        _same_cloud(want, got, "view filter")
    finally:
        m.destroy()


@pytest.mark.gpu
def test_infer_points_normals_depth_pro_equals_infer_then_unproject(dev):
    from burn_depth_amd import ops
    m = _pro(dev, "small", "BF16")
    fork = None
    try:
        x = _image(2, 512).cuda()
        ref = m.infer(x)
        kw = dict(**OPTS, **NRM)
        want = _cloud_np(ops.unproject(dev, ref.depth, focal_px=ref.focallength_px, **kw))
        got = _cloud_np(m.infer_points(x, **kw))
        assert want["count"][-1] > 0 and _defined(want["normal_map"]).any()
        _same_cloud(want, got, "predicted focal")
        fork = m.fork()
        _same_cloud(want, _cloud_np(fork.infer_points(x, **kw)), "fork")
        f = torch.tensor([400.0, 650.0], device="cuda")
        E = _cameras(np.random.default_rng(2), 2, 512, 512)[1]
        known = m.infer(x, f_px=f)
        want = _cloud_np(ops.unproject(dev, known.depth, focal_px=f, extrinsics=_t(E), world=True, **kw))
        _same_cloud(want, _cloud_np(m.infer_points(x, f_px=f, extrinsics=E, world=True, **kw)), "known focal")
    finally:
        if fork is not None:
            fork.destroy()
        m.destroy()


@pytest.mark.gpu
def test_infer_points_normals_graph_replay_and_allocations(dev):
    m = _da3(dev, precision="BF16")
    try:
        x = _image(2, 70).cuda()
        kw = dict(conf_min=1.0, world=True, **OPTS, **NRM)
        eager = _cloud_np(m.infer_points(x, **kw))
        assert eager["count"][-1] > 0
        m.enable_graph(True)
        out = m.infer_points(x, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            for t in (out.xyz, out.point_map, out.normal_map, out.normals):
                t.fill_(POISON)
            out = m.infer_points(x, out=out, **kw)
            torch.cuda.synchronize()
            _same_cloud(eager, _cloud_np(out), f"graph call {call}")
        # min_cos changed, same pointers: its own graph and its own result
        kw2 = dict(kw, normal_min_cos=0.3)
        m.enable_graph(False)
        want2 = _cloud_np(m.infer_points(x, **kw2))
        m.enable_graph(True)
        assert want2["count"][-1] < eager["count"][-1]
        for _ in range(3):
            out = m.infer_points(x, out=out, **kw2)
        torch.cuda.synchronize()
        _same_cloud(want2, _cloud_np(out), "min_cos 0.3")
        out = m.infer_points(x, out=out, **kw)
        torch.cuda.synchronize()
        _same_cloud(eager, _cloud_np(out), "back to the first key")
        before = m.query("allocs")
        for _ in range(3):
            m.infer_points(x, out=out, **kw)
            m.infer_points(x, out=out, **kw2)
        torch.cuda.synchronize()
        assert m.query("allocs") == before == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


@pytest.mark.gpu
def test_normal_refusals_leave_the_outputs_untouched(dev):
    from burn_depth_amd import ops
    B, H, W = 2, 37, 53
    d, c = _scene(B, H, W)
    K, _ = _cameras(np.random.default_rng(1), B, H, W)

    def untouched(out, stores):
        torch.cuda.synchronize()
        fills = dict(point_map=POISON, mask=77, xyz=POISON, count=-5, normal_map=POISON, normals=POISON)
        for k, store in stores.items():
            assert (store == fills[k]).all(), k

    for bad in (float("nan"), float("inf"), -0.1, 1.01):
        out, stores = _fresh(B, H, W, B * H * W, False, False)
        with pytest.raises(_lib.MdError) as e:
            ops.unproject(dev, _t(d), intrinsics=_t(K), conf=_t(c), out=out, normal_min_cos=bad)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
        untouched(out, stores)
    out, stores = _fresh(B, H, W, B * H * W, False, False)
    out.xyz = out.count = None  # normals without count
    with pytest.raises(_lib.MdError) as e:
        ops.unproject(dev, _t(d), intrinsics=_t(K), out=out)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    untouched(out, stores)
    out, stores = _fresh(B, H, W, B * H * W, False, False, normals=False)
    with pytest.raises(_lib.MdError) as e:  # normals asked for, into an `out` that has no tensor for them
        ops.unproject(dev, _t(d), intrinsics=_t(K), out=out, normals=True)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    untouched(out, stores)
    out, stores = _fresh(B, H, W, B * H * W, False, False)
    with pytest.raises(_lib.MdError) as e:  # the point path's own refusals, through the new entry
        ops.unproject(dev, _t(d), intrinsics=_t(K), out=out, stride=0)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    untouched(out, stores)
    m = _da3(dev, precision="BF16", max_batch=1)
    try:
        for kw in (dict(normal_min_cos=2.0), dict(normal_min_cos=float("nan"))):
            out, stores = _fresh(1, 70, 70, 70 * 70, False, True)
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(_image(1, 70).cuda(), out=out, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG
            untouched(out, {k: v for k, v in stores.items() if k != "conf"})
    finally:
        m.destroy()


@pytest.mark.gpu
def test_infer_cli_writes_the_normals_into_the_ply(dev, tmp_path):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
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
    assert cli.main(["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "2", "--edge-rtol", "0.5",
                     "--normals", "--normal-min-cos", "0.05"]) == 0
    xyz, col, nrm = P.read_ply_normals(ply)
    m = DepthAnything3.load_file(dev, cfg, ck)
    try:
        prep = P.prepare_depth_anything3_image(rgb, 518).rgb
        x = rgb_to_input_tensor(prep.tobytes(), 518, 518, dev)
        pc = m.infer_points(x, rgb=_t(prep[None]), dense=False, stride=2, edge_rtol=0.5, world=True, normals=True, normal_min_cos=0.05)
        want_xyz, want_col, _ = pc.points()
        want_nrm = pc.normals[:want_xyz.shape[0]]
    finally:
        m.destroy()
    assert xyz.shape[0] > 0 and nrm is not None and _defined(nrm).all()
    assert np.array_equal(_bits(xyz), _bits(want_xyz.cpu().numpy())) and np.array_equal(col, want_col.cpu().numpy())
    assert np.array_equal(_bits(nrm), _bits(want_nrm.cpu().numpy()))
