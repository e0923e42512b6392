"""Rasterising the mesh into target cameras: md_op_render_mesh and its host reference pipeline.render_mesh.
include/mi_depth.h states the contract, DESIGN 12.6 the kernels. Coverage is integer arithmetic at 1/256 pixel and a pixel keeps
the minimum of a 64-bit key: selection, not blending, so every comparison is bit for bit.

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
NEW_ENTRIES = ("md_raster_opts_default", "md_op_render_mesh", "md_infer_points_raster", "md_raster_inline_pixels", "md_debug_raster_queue")
TINY, HUGE = f32(np.finfo(f32).tiny), f32(np.finfo(f32).max)
EYE = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]], f32)  # with z = 1: uf = x, vf = y
FIELDS = ("depth", "face", "rgb", "filled", "skipped")


def _targets(rng, T, H, W):
    """T cameras near the origin that look down +z with a small yaw and offset each: all of them see most of `_surface`"""
    K = np.zeros((T, 3, 3), f32)
    E = np.zeros((T, 3, 4), f32)
    for j in range(T):
        K[j] = [[0.9 * W + j, 0, W / 2 + 0.3], [0, 0.8 * W + 2 * j, H / 2 - 0.7], [0, 0, 1]]
        a = rng.uniform(-0.15, 0.15)
        E[j, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[j, :, 3] = rng.uniform(-0.3, 0.3, 3)
    return K, E


def _surface(rng, side, F=None):
    """A wavy sheet of side x side jittered vertices in front of `_targets`, wider than their view, with colours; its quads as
    2 (side - 1)^2 faces in a shuffled order with random windings, a few of them far in front of the rest -> (xyz, rgb, faces)"""
    g = np.linspace(-3.5, 3.5, side)
    x, y = np.meshgrid(g, g)
    step = 7.0 / max(side - 1, 1)
    x = x + rng.uniform(-0.3, 0.3, x.shape) * step
    y = y + rng.uniform(-0.3, 0.3, y.shape) * step
    z = 4.0 + 0.8 * np.sin(1.3 * x) * np.cos(0.9 * y) + rng.uniform(-0.05, 0.05, x.shape)
    z[rng.random(z.shape) < 0.02] = 2.5  # spikes towards the cameras: occlusion and stretched faces
    xyz = np.stack([x, y, z], -1).reshape(-1, 3).astype(f32)
    i = np.arange(side * side).reshape(side, side)
    a, b, c, d = i[:-1, :-1], i[:-1, 1:], i[1:, :-1], i[1:, 1:]
    faces = np.concatenate([np.stack([a, c, d], -1).reshape(-1, 3), np.stack([a, d, b], -1).reshape(-1, 3)])
    faces = faces[rng.permutation(len(faces))]
    flip = rng.random(len(faces)) < 0.3
    faces[flip] = faces[flip][:, ::-1]
    faces = faces[:F] if F is not None else faces
    return xyz, rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8), np.ascontiguousarray(faces, np.int32)


def _loop_raster(xyz, faces, H, W, K, E=None, off=0.0, n=None, z_near=0.0, z_far=0.0, cull=0, max_extent=0):
    """The contract once more, face by face and pixel by pixel: Python ints for the coverage, numpy scalars for the float steps
    -> ({(j, v, u): (bits(z), f)}, skipped [T+1])"""
    zn, zf = (f32(z_near) if z_near > 0 else TINY), (f32(z_far) if z_far > 0 else HUGE)
    off, half, one = f32(off), f32(0.5), f32(1)
    ext = max_extent or 64
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    N, F = len(xyz), len(faces)
    n = F if n is None else min(max(n, 0), F)
    best, skipped = {}, [0] * (len(K) + 1)
    edge = lambda a, b, p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])  # noqa: E731
    with np.errstate(all="ignore"):
        for f in range(n):
            idx = [int(i) for i in faces[f]]
            if any(i < 0 or i >= N for i in idx) or not np.isfinite(xyz[idx]).all():
                continue
            for j in range(len(K)):
                V, iz = [], []
                for i in idx:
                    x, y, z = xyz[i]
                    p = (x, y, z) if E is None else [((E[j, a, 0] * x + E[j, a, 1] * y) + E[j, a, 2] * z) + E[j, a, 3] for a in range(3)]
                    if not (np.isfinite(p[2]) and zn <= p[2] <= zf):
                        break
                    uf = ((K[j, 0, 0] * (p[0] / p[2])) + K[j, 0, 2]) - off
                    vf = ((K[j, 1, 1] * (p[1] / p[2])) + K[j, 1, 2]) - off
                    sx, sy = np.floor(uf * f32(256) + half), np.floor(vf * f32(256) + half)
                    if not (np.abs(sx) < f32(16777216) and np.abs(sy) < f32(16777216)):
                        break
                    V.append((int(sx), int(sy)))
                    iz.append(one / f32(p[2]))
                if len(V) < 3:
                    continue
                A = edge(V[0], V[1], V[2])
                if A == 0 or (cull and A > 0):
                    continue
                sign = -1 if A < 0 else 1
                A *= sign
                xs, ys = [v[0] for v in V], [v[1] for v in V]
                u0, u1 = max(0, (min(xs) + 255) >> 8), min(W - 1, max(xs) >> 8)
                v0, v1 = max(0, (min(ys) + 255) >> 8), min(H - 1, max(ys) >> 8)
                if u0 > u1 or v0 > v1:
                    continue
                if u1 - u0 + 1 > ext or v1 - v0 + 1 > ext:
                    skipped[j] += 1
                    skipped[-1] += 1
                    continue
                for v in range(v0, v1 + 1):
                    for u in range(u0, u1 + 1):
                        pt = (256 * u, 256 * v)
                        w = [sign * edge(V[1], V[2], pt), sign * edge(V[2], V[0], pt), sign * edge(V[0], V[1], pt)]
                        if min(w) < 0:
                            continue
                        b = [f32(np.float64(k) / np.float64(A)) for k in w]
                        z = one / ((b[0] * iz[0] + b[1] * iz[1]) + b[2] * iz[2])
                        if not (np.isfinite(z) and zn <= z <= zf):
                            continue
                        key = (int(f32(z).view(np.uint32)), f)
                        if (j, v, u) not in best or key < best[(j, v, u)]:
                            best[(j, v, u)] = key
    return best, skipped


def _same_as_loop(r, loop, T, H, W, what=""):
    best, skipped = loop
    depth, face = np.zeros((T, H, W), np.uint32), np.full((T, H, W), -1, np.int32)
    for (j, v, u), (zb, f) in best.items():
        depth[j, v, u], face[j, v, u] = zb, f
    assert np.array_equal(r.face, face), what
    assert np.array_equal(_bits(r.depth), depth), what
    per = [(face[j] >= 0).sum() for j in range(T)]
    assert r.filled.tolist() == per + [sum(per)] and r.skipped.tolist() == skipped, what


def _loop_colour(xyz, faces, rgb, r, K, off=0.0):
    """The colour of every filled pixel from the winner `r.face` names, camera-space vertices (E = None), scalar by scalar"""
    out = np.zeros(r.face.shape + (3,), np.uint8)
    edge = lambda a, b, p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])  # noqa: E731
    for j, v, u in np.argwhere(r.face >= 0):
        idx = faces[r.face[j, v, u]]
        V = []
        for i in idx:
            x, y, z = xyz[i]
            uf, vf = ((K[j, 0, 0] * (x / z)) + K[j, 0, 2]) - f32(off), ((K[j, 1, 1] * (y / z)) + K[j, 1, 2]) - f32(off)
            V.append((int(np.floor(uf * f32(256) + f32(0.5))), int(np.floor(vf * f32(256) + f32(0.5)))))
        A = edge(V[0], V[1], V[2])
        pt = (256 * int(u), 256 * int(v))
        w = [edge(V[1], V[2], pt), edge(V[2], V[0], pt), edge(V[0], V[1], pt)]
        sign = -1 if A < 0 else 1
        b = [f32(np.float64(sign * k) / np.float64(sign * A)) for k in w]
        c = rgb[idx].astype(f32)
        out[j, v, u] = np.minimum(np.floor(((b[0] * c[0] + b[1] * c[1]) + b[2] * c[2]) + f32(0.5)), f32(255)).astype(np.uint8)
    return out


below = lambda v: np.nextafter(f32(v), f32(-np.inf))  # noqa: E731
# The largest sx below the guard band is 2^24 - 2: uf * 256 = 2^24 - 1 plus 0.5 rounds to 2^24 in f32 and fails, 2^24 - 2 plus 0.5
# rounds back to 2^24 - 2. On the negative side -(2^24 - 1) + 0.5 rounds to -(2^24 - 2) and passes as well.
INSIDE = f32(65536 - 2 / 256)

# Small scenes on an 8 x 8 target with K = EYE, one per clause of the contract: (name, xyz, faces, keywords, what must hold)
QUAD = np.array([[1, 1, 1], [6, 1, 1], [1, 6, 1], [6, 6, 1]], f32)  # a, b, c, d of a quad on pixel centres
SCENES = [
    ("one triangle on pixel centres", QUAD, [[0, 2, 1]], {}, lambda r: r.filled[0] == 21 and (r.face[0, [1, 1, 6, 3], [1, 6, 1, 4]] == 0).all()),
    ("two faces share an edge", QUAD, [[0, 2, 3], [0, 3, 1]], {}, lambda r: r.filled[0] == 36 and (r.face[0, 1:7, 1:7] >= 0).all()),
    ("a duplicated face", QUAD, [[0, 2, 1], [0, 2, 1]], {}, lambda r: r.filled[0] == 21 and r.face.max() == 0),
    ("both windings, both sides drawn", QUAD, [[0, 2, 1], [3, 2, 1]], dict(cull=0), lambda r: set(np.unique(r.face)) == {-1, 0, 1}),
    ("both windings, culled", QUAD, [[0, 2, 1], [3, 2, 1]], dict(cull=1), lambda r: set(np.unique(r.face)) == {-1, 0}),
    ("the other winding, culled", QUAD, [[0, 1, 2]], dict(cull=1), lambda r: r.filled[0] == 0),
    ("no area", np.array([[1, 1, 1], [3, 3, 1], [5, 5, 1], [1, 1, 1]], f32), [[0, 1, 2], [0, 3, 1]], {}, lambda r: r.filled[0] == 0),
    ("an index outside the list", QUAD, [[0, 2, 4], [0, -1, 1], [0, 2, 1]], {}, lambda r: r.filled[0] == 21 and r.face.max() == 2),
    ("a vertex that is not finite", np.array([[1, 1, 1], [6, 1, np.nan], [1, 6, 1], [np.inf, 6, 1]], f32), [[0, 2, 1], [0, 2, 3]], {},
     lambda r: r.filled[0] == 0),
    ("a vertex at z_near", QUAD * f32(2), [[0, 2, 1]], dict(z_near=2.0), lambda r: r.filled[0] == 21),
    ("a vertex one ulp below z_near", np.concatenate([QUAD[:2] * f32(2), QUAD[2:3] * below(2)]), [[0, 2, 1]], dict(z_near=2.0),
     lambda r: r.filled[0] == 0),
    ("sx at the guard band", np.array([[1, 1, 1], [65536, 3, 1], [1, 6, 1], [-65536, 3, 1]], f32), [[0, 2, 1], [0, 2, 3]], {},
     lambda r: r.filled[0] == 0),
    ("sx one step inside the guard band", np.array([[1, 1, 1], [INSIDE, 3, 1], [1, 6, 1], [-INSIDE, 3, 1]], f32), [[0, 2, 1], [0, 2, 3]], {},
     lambda r: (r.face[0, 3, 1:] == 0).all() and (r.face[0, 3, :2] == [1, 0]).all()),
    ("max_extent at the box size", QUAD, [[0, 2, 1]], dict(max_extent=6), lambda r: r.filled[0] == 21 and r.skipped.tolist() == [0, 0]),
    ("max_extent one below the box size", QUAD, [[0, 2, 1], [0, 2, 3]], dict(max_extent=5), lambda r: r.filled[0] == 0 and r.skipped.tolist() == [2, 2]),
    ("a far face behind a near one", np.concatenate([QUAD, f32([[1, 1, 0.5], [2, 1, 0.5], [1, 2, 0.5]])]), [[0, 2, 3], [0, 3, 1], [4, 6, 5]], {},
     lambda r: (r.face == 2).sum() == 6 and (r.depth[r.face == 2] == 0.5).all() and r.filled[0] == 36),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_raster_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    for struct in ("md_raster_opts", "md_raster_outputs", "md_points_raster"):
        assert "} %s;" % struct in header
    assert [n for n, _ in _lib.MdRasterOpts._fields_] == ["pixel_offset", "z_near", "z_far", "cull", "max_extent"]
    assert [n for n, _ in _lib.MdRasterOutputs._fields_] == ["depth", "face", "rgb", "filled", "skipped"]
    assert [n for n, _ in _lib.MdPointsRaster._fields_] == ["T", "H", "W", "cam", "opts", "out"]
    o = _lib.MdRasterOpts(1.0, 2.0, 3.0, 1, 7)
    lib.md_raster_opts_default(C.byref(o))
    assert (o.pixel_offset, o.z_near, o.z_far, o.cull, o.max_extent) == (0.0, 0.0, 0.0, 0, 0)
    assert 1 <= lib.md_raster_inline_pixels() <= 1024 * 1024
    assert lib.md_debug_raster_queue(-1) < 0
    prev = lib.md_debug_raster_queue(7)
    assert lib.md_debug_raster_queue(prev) == 7 and lib.md_debug_raster_queue(prev) == prev


@pytest.mark.parametrize("scene", SCENES, ids=[s[0] for s in SCENES])
def test_reference_on_the_clauses_of_the_contract(scene):
    _, xyz, faces, kw, holds = scene
    with np.errstate(all="ignore"):
        r = P.render_mesh(xyz, faces, 8, 8, EYE, **kw)
    _same_as_loop(r, _loop_raster(xyz, faces, 8, 8, EYE, **kw), 1, 8, 8)
    assert holds(r), (r.face[0], r.filled, r.skipped)


def test_reference_against_the_loop_restatement():
    rng = np.random.default_rng(5)
    xyz, rgb, faces = _surface(rng, 12)
    F = len(faces)
    for T in (1, 3):
        for H, W in ((8, 8), (37, 53)):
            K, E = _targets(rng, T, H, W)
            for kw in (dict(off=0.5), dict(cull=1), dict(max_extent=9 if W > 8 else 3), dict(z_near=3.6, z_far=4.4)):
                ref_kw = {("pixel_offset" if k == "off" else k): v for k, v in kw.items()}
                r = P.render_mesh(xyz, faces, H, W, K, E, rgb=rgb, **ref_kw)
                _same_as_loop(r, _loop_raster(xyz, faces, H, W, K, E, **kw), T, H, W, (T, H, W, kw))
                assert r.filled[-1] > 0 and not r.rgb[r.face < 0].any()
    # the count word, and both camera forms
    K, E = _targets(rng, 2, 9, 11)
    for count in (-3, 0, F // 2, F + 7):
        r = P.render_mesh(xyz, faces, 9, 11, K, E, face_count=count)
        _same_as_loop(r, _loop_raster(xyz, faces, 9, 11, K, E, n=count), 2, 9, 11, count)
        assert r.face.max() < max(min(count, F), 0) or count <= 0
    cam = ((E[0, :, :3].astype(np.float64) @ xyz.T.astype(np.float64)).T + E[0, :, 3]).astype(f32)  # the sheet in camera 0's frame
    r = P.render_mesh(cam, faces, 9, 11, K[:1], rgb=rgb)
    _same_as_loop(r, _loop_raster(cam, faces, 9, 11, K[:1]), 1, 9, 11, "camera frame")
    assert np.array_equal(r.rgb, _loop_colour(cam, faces, rgb, r, K[:1]))
    fo = np.array([7.0, 9.5], f32)
    Kf = np.array([[[v, 0, 11 / 2], [0, v, 9 / 2], [0, 0, 1]] for v in fo], f32)
    _same_as_loop(P.render_mesh(xyz, faces, 9, 11, focal_px=fo, extrinsics=E), _loop_raster(xyz, faces, 9, 11, Kf, E), 2, 9, 11, "focal")


def _plane_scene():
    """A tilted plane seen by a 37 x 53 source camera, as the full-grid mesh of its list, and a target camera rotated in the
    image plane and shifted -> (H, W, xyz, faces, K, E of the target)"""
    H, W = 37, 53
    K = np.array([[[48.0, 0, 26.2], [0, 44.0, 18.1], [0, 0, 1]]], f32)
    v, u = np.mgrid[0:H, 0:W]
    nrm, c = np.array([0.25, -0.15, 1.0]), 3.0  # the plane nrm . X = c; on the ray of pixel (u, v): d = c / (nrm . ray)
    ray = np.stack([(u + 0.5 - 26.2) / 48.0, (v + 0.5 - 18.1) / 44.0, np.ones_like(u, float)], -1)
    depth = (c / (ray @ nrm)).astype(f32)[None]
    hp = P.unproject_depth(depth, K, pixel_offset=0.5, world=False)
    faces, count = P.mesh_grid(depth, P.pixel_index(hp), max_rtol=0.0)
    assert count[-1] == 2 * (H - 1) * (W - 1) == len(faces)
    a = 0.3
    E = np.array([[[np.cos(a), -np.sin(a), 0, 0.2], [np.sin(a), np.cos(a), 0, -0.1], [0, 0, 1, 0.4]]], f32)
    return H, W, hp.xyz, faces, K, E


def _check_no_cracks(r, H, W, xyz, K, E):
    """The filled set is the set of pixel centres inside the outline of the four projected corners, computed in ints from their
    snapped positions. Every boundary vertex and every corner is snapped to 1/256 pixel on its own (an error of at most 0.71
    of that step each), so the mesh leaves the straight outline by less than 1.5 steps; the scene is one in which no pixel centre
    lies within 2 steps of an outline edge (asserted here, from the corners alone), so the equality is exact."""
    corners = [0, W - 1, H * W - 1, (H - 1) * W]  # around the grid
    S = []
    for i in corners:
        p = [((E[0, a, 0] * xyz[i, 0] + E[0, a, 1] * xyz[i, 1]) + E[0, a, 2] * xyz[i, 2]) + E[0, a, 3] for a in range(3)]
        uf, vf = ((K[0, 0, 0] * (p[0] / p[2])) + K[0, 0, 2]) - f32(0.5), ((K[0, 1, 1] * (p[1] / p[2])) + K[0, 1, 2]) - f32(0.5)
        S.append((int(np.floor(uf * f32(256) + f32(0.5))), int(np.floor(vf * f32(256) + f32(0.5)))))
    turn = 1 if sum(S[k][0] * S[(k + 1) % 4][1] - S[(k + 1) % 4][0] * S[k][1] for k in range(4)) > 0 else -1
    inside = np.zeros((H, W), bool)
    margin = np.inf
    for v in range(H):
        for u in range(W):
            e = []  # the distance of the centre from the line of every outline edge, in 1/256 pixel, positive on the inner side
            for k in range(4):
                (ax, ay), (bx, by) = S[k], S[(k + 1) % 4]
                e.append(turn * ((bx - ax) * (256 * v - ay) - (by - ay) * (256 * u - ax)) / np.hypot(bx - ax, by - ay))
            inside[v, u] = min(e) >= 0
            margin = min(margin, abs(min(e)))
    assert margin > 2.0, f"a pixel centre lies {margin / 256} pixels from the outline: choose another target camera"
    assert 400 < inside.sum() < H * W
    assert np.array_equal(r.face[0] >= 0, inside), np.argwhere((r.face[0] >= 0) != inside)
    assert r.filled.tolist() == [inside.sum()] * 2 and r.skipped.tolist() == [0, 0]


def test_no_cracks_on_the_host():
    H, W, xyz, faces, K, E = _plane_scene()
    _check_no_cracks(P.render_mesh(xyz, faces, H, W, K, E, pixel_offset=0.5), H, W, xyz, K, E)


def _round_trip_scene():
    H, W = 37, 53
    rng = np.random.default_rng(11)
    K, _ = _cameras(rng, 1, H, W)
    v, u = np.mgrid[0:H, 0:W]
    depth = (2.0 + 0.3 * np.sin(0.2 * u) + 0.2 * np.cos(0.15 * v) + 1.5 * (u > 30)).astype(f32)[None]  # a 1.5 depth step
    hp = P.unproject_depth(depth, K, pixel_offset=0.5, world=False)
    faces, _ = P.mesh_grid(depth, P.pixel_index(hp), max_rtol=0.05)
    return H, W, K, depth, hp, faces


def _check_round_trip(r, depth, hp, faces):
    """Rendered into its own camera every listed pixel is a vertex on its own pixel centre: b = (1, 0, 0) there, z = 1 / (1 / d),
    which is within one ulp of d"""
    listed = hp.mask[0].astype(bool)
    assert len(faces) > 3000 and r.filled.tolist() == [len(hp.xyz)] * 2 == [listed.sum()] * 2
    assert np.array_equal(r.face[0] >= 0, listed)
    got, want = _bits(r.depth[0][listed]).astype(np.int64), _bits(depth[0][listed]).astype(np.int64)
    assert np.abs(got - want).max() <= 1
    print(f"round trip: {listed.sum()} of {len(hp.xyz)} filled, {100 * (got == want).mean():.0f} % exact")


def test_round_trip_on_the_host():
    H, W, K, depth, hp, faces = _round_trip_scene()
    _check_round_trip(P.render_mesh(hp.xyz, faces, H, W, K, pixel_offset=0.5), depth, hp, faces)


def test_reference_refuses_bad_arguments():
    xyz, faces = np.zeros((3, 3), f32), [[0, 1, 2]]
    for kw in (dict(cull=2), dict(cull=-1), dict(max_extent=-1), dict(max_extent=1025), dict(z_near=-1.0), dict(z_far=float("nan")),
               dict(z_near=2.0, z_far=1.0), dict(pixel_offset=float("inf"))):
        with pytest.raises(ValueError):
            P.render_mesh(xyz, faces, 4, 4, focal_px=[3.0], **kw)
    with pytest.raises(ValueError):
        P.render_mesh(xyz, faces, 4, 4)
    with pytest.raises(ValueError):
        P.render_mesh(xyz, faces, 0, 4, focal_px=[3.0])
    assert P.render_mesh(xyz, faces, 4, 4, focal_px=[3.0], max_extent=1024).filled.tolist() == [0, 0]


INV, SHP = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
NAN, INF = float("nan"), float("inf")
# (keywords of `call` in the refusal tests, the code); o = (pixel_offset, z_near, z_far, cull, max_extent)
REFUSALS = [(dict(o=None), INV), (dict(out=None), INV), (dict(cam=None), INV), (dict(out=()), INV), (dict(rgb_in=False), INV),
            (dict(cam=()), INV), (dict(o=(0, 0, 0, 2, 0)), INV), (dict(o=(0, 0, 0, -1, 0)), INV), (dict(o=(0, 0, 0, 0, -1)), INV),
            (dict(o=(0, 0, 0, 0, 1025)), INV), (dict(o=(NAN, 0, 0, 0, 0)), INV), (dict(o=(0, INF, 0, 0, 0)), INV), (dict(o=(0, 0, NAN, 0, 0)), INV),
            (dict(o=(0, -1.0, 0, 0, 0)), INV), (dict(o=(0, 0, -1.0, 0, 0)), INV), (dict(o=(0, 2.0, 1.0, 0, 0)), INV), (dict(faces_in=False), INV),
            (dict(xyz_in=False), INV), (dict(N=-1), SHP), (dict(N=1 << 31), SHP), (dict(F=-1), SHP), (dict(F=1 << 31), SHP), (dict(T=0), SHP),
            (dict(H=0), SHP), (dict(W=-1), SHP), (dict(T=1, H=1 << 16, W=1 << 15), SHP), (dict(H=1 << 24, W=1), SHP), (dict(H=1, W=1 << 24), SHP)]


def _refusal_call(lib, dev_h, ptr, code, N=3, F=1, T=1, H=2, W=2, cam=True, o=(0, 0, 0, 0, 0), out=True, rgb_in=True, faces_in=True, xyz_in=True):
    """md_op_render_mesh with one argument at fault; ptr: name -> address (the outputs by their field names)"""
    cams = _lib.MdPointsCameras(ptr["K"], None, None) if cam is True else (_lib.MdPointsCameras(None, None, None) if cam == () else None)
    opts = _lib.MdRasterOpts(*o) if o is not None else None
    outs = (_lib.MdRasterOutputs(*(ptr[k] for k in FIELDS)) if out is True else (_lib.MdRasterOutputs(None, None, None, None, None) if out == () else None))
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    rc = lib.md_op_render_mesh(dev_h, ptr["xyz"] if xyz_in else None, ptr["rgb_row"] if rgb_in else None, N, ptr["faces"] if faces_in else None,
                               F, None, T, H, W, ref(cams), ref(opts), ref(outs), None)
    assert rc == code, (rc, lib.md_last_error().decode())


def test_c_entries_refuse_before_they_look_at_the_device(lib):
    """With a null device every refusal above still comes first and names its own code; the pointers are never read"""
    buf = (C.c_char * 64)()
    ptr = {k: C.addressof(buf) for k in FIELDS + ("K", "xyz", "rgb_row", "faces")}
    for kw, code in REFUSALS:
        _refusal_call(lib, None, ptr, code, **kw)
    _refusal_call(lib, None, ptr, INV)
    assert "device is null" in lib.md_last_error().decode()
    assert lib.md_infer_points_raster(None, C.addressof(buf), 1, 2, 2, 1, None, None, None, None, None, None, None, None, None, None, 1, None) == INV


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _dev_raster(dev, xyz, faces, H, W, K=None, E=None, focal=None, rgb=None, face_count=None, **kw):
    from burn_depth_amd import ops
    cnt = None if face_count is None else torch.tensor([face_count], dtype=torch.int32, device="cuda")
    fc = torch.from_numpy(np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))).cuda()
    r = ops.render_mesh(dev, _t(np.asarray(xyz, f32).reshape(-1, 3)), fc, H, W, _t(K), _t(E), _t(focal), rgb=_t(rgb), face_count=cnt, **kw)
    torch.cuda.synchronize()
    return r


def _same(got, want, what=""):
    for k in FIELDS:
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            g = g.cpu().numpy()
            assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, int((g != w).sum()))


def _both(dev, xyz, faces, H, W, K=None, E=None, focal=None, rgb=None, face_count=None, what="", **kw):
    with np.errstate(all="ignore"):
        want = P.render_mesh(xyz, faces, H, W, K, E, focal, rgb=rgb, face_count=face_count, **kw)
    _same(_dev_raster(dev, xyz, faces, H, W, K, E, focal, rgb, face_count, **kw), want, what)
    return want


@gpu
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 257, 5001])
def test_tails(dev, F):
    rng = np.random.default_rng(100 + F)
    xyz, rgb, faces = _surface(rng, 52, F)
    assert len(faces) == F
    for H, W in ((37, 53), (96, 96)):
        for T in (1, 3):
            K, E = _targets(rng, T, H, W)
            want = _both(dev, xyz, faces, H, W, K, E, rgb=rgb, pixel_offset=0.5, what=(F, H, W, T))
            assert (want.filled[:-1] > 0).all() or F < 257


@gpu
def test_a_second_group_of_cameras(dev):
    rng = np.random.default_rng(65)
    xyz, rgb, faces = _surface(rng, 12)
    K, E = _targets(rng, 65, 8, 8)
    want = _both(dev, xyz, faces, 8, 8, K, E, rgb=rgb, what="T = 65")
    assert want.filled[64] > 0 and want.filled[-1] == want.filled[:-1].sum()
    want = _both(dev, xyz, faces, 8, 8, K, E, rgb=rgb, max_extent=7, what="T = 65, max_extent 7")  # the last cameras are the closest
    assert want.skipped[64] > 0 and want.skipped[-1] == want.skipped[:-1].sum()


@gpu
def test_count_word(dev):
    rng = np.random.default_rng(1)
    xyz, rgb, faces = _surface(rng, 40)
    F = len(faces)
    K, E = _targets(rng, 2, 37, 53)
    assert P.render_mesh(xyz, faces, 37, 53, K, E).face.max() > F - 200
    for count in (F // 3, F + 17, 0, -5, 1):
        want = _both(dev, xyz, faces, 37, 53, K, E, rgb=rgb, face_count=count, what=count)
        assert want.face.max() < max(min(count, F), 0) or count <= 0


@gpu
def test_the_clauses_of_the_contract_on_the_device(dev):
    for name, xyz, faces, kw, holds in SCENES:
        assert holds(_both(dev, xyz, faces, 8, 8, EYE, what=name, **kw)), name
    # a camera with NaN in t sees nothing; its neighbours are not disturbed
    rng = np.random.default_rng(3)
    xyz, rgb, faces = _surface(rng, 20)
    for slot in (0, 2):
        K3, E3 = _targets(rng, 3, 37, 53)
        E3[1, slot, 3] = np.nan
        want = _both(dev, xyz, faces, 37, 53, K3, E3, rgb=rgb, what=("nan t", slot))
        assert want.filled[1] == 0 and want.filled[0] > 0 and want.filled[2] > 0


def _right_triangles(boxes, W):
    """One right triangle per (bw, bh), legs on pixel centres, so that its box holds bw x bh pixels; side by side on rows of a
    W-wide image at z = 1 + a little per face -> (xyz, faces)"""
    xyz, faces, u, v, row = [], [], 0, 0, 0
    for k, (bw, bh) in enumerate(boxes):
        if u + bw > W:
            u, v, row = 0, v + row, 0
        z = 1 + k / 64
        xyz += [[u * z, v * z, z], [(u + bw - 1) * z, v * z, z], [u * z, (v + bh - 1) * z, z]]
        faces.append([3 * k, 3 * k + 2, 3 * k + 1])
        u, row = u + bw, max(row, bh)
    return np.array(xyz, f32), np.array(faces, np.int32)


@gpu
def test_boxes_around_the_inline_threshold(dev, lib):
    """Faces whose boxes hold at most md_raster_inline_pixels() pixels are drawn by their setup thread, larger ones go through the
    queue: boxes just under, at and just over the shipped value run both paths"""
    k = int(lib.md_raster_inline_pixels())
    bw = max(int(np.sqrt(k)), 1)
    bh = k // bw
    boxes = [(bw, bh), (bw, bh + 1), (bw + 1, bh), (max(bw - 1, 1), bh), (bw + 1, bh + 1), (2 * bw, 2 * bh)] * 6
    assert bw * bh <= k < bw * (bh + 1) and k < (bw + 1) * bh + (bh == 0)
    xyz, faces = _right_triangles(boxes, 96)
    want = _both(dev, xyz, faces, 96, 96, EYE, rgb=np.random.default_rng(0).integers(0, 256, (len(xyz), 3), dtype=np.uint8), what=k)
    assert set(np.unique(want.face)) == set(range(-1, len(faces)))


@gpu
def test_a_full_queue_draws_in_place(dev, lib):
    rng = np.random.default_rng(9)
    k = int(lib.md_raster_inline_pixels())
    side = int(np.sqrt(k)) + 3
    step = (96 - side) // 9
    assert side * side > k and step >= 1  # 100 faces beyond the inline threshold on a 10 x 10 grid of corners, overlapping
    xyz, faces = [], []
    for i in range(100):
        u, v, z = (i % 10) * step, (i // 10) * step, 1 + i / 64
        xyz += [[u * z, v * z, z], [(u + side - 1) * z, v * z, z], [u * z, (v + side - 1) * z, z]]
        faces.append([3 * i, 3 * i + 2, 3 * i + 1])
    xyz, faces = np.array(xyz, f32), np.array(faces, np.int32)
    rgb = rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    K = np.repeat(EYE, 2, 0)
    prev = lib.md_debug_raster_queue(4)
    try:
        want = _both(dev, xyz, faces, 96, 96, K, rgb=rgb, what="queue of 4")
    finally:
        lib.md_debug_raster_queue(prev)
    assert want.filled[0] > 50 * side and len(np.unique(want.face)) > 50 and lib.md_debug_raster_queue(prev) == prev
    _both(dev, xyz, faces, 96, 96, K, rgb=rgb, what="default queue")


@gpu
def test_each_output_alone_between_canaries(dev):
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import RasterisedMesh
    rng = np.random.default_rng(4)
    xyz, rgb, faces = _surface(rng, 30)
    K, E = _targets(rng, 2, 37, 53)
    want = P.render_mesh(xyz, faces, 37, 53, K, E, rgb=rgb, max_extent=4)
    assert want.skipped[-1] > 0 and want.filled[-1] > 0
    shapes = dict(depth=((2, 37, 53), torch.float32), face=((2, 37, 53), torch.int32), rgb=((2, 37, 53, 3), torch.uint8),
                  filled=((3,), torch.int32), skipped=((3,), torch.int32))
    pad = 64
    for names in [(k,) for k in FIELDS] + [FIELDS]:
        store = {k: torch.full((int(np.prod(shapes[k][0])) + 2 * pad,), 77, dtype=shapes[k][1], device="cuda") for k in names}
        out = RasterisedMesh(**{k: store[k][pad:-pad].view(shapes[k][0]) for k in names})
        ops.render_mesh(dev, _t(xyz), _t(faces), 37, 53, _t(K), _t(E), rgb=_t(rgb), max_extent=4, out=out)
        torch.cuda.synchronize()
        for k in names:
            assert np.array_equal(getattr(out, k).cpu().numpy().view(np.uint8), getattr(want, k).view(np.uint8)), (names, k)
            assert (store[k][:pad] == 77).all() and (store[k][-pad:] == 77).all(), (names, k)


@gpu
def test_round_trips_on_the_device(dev):
    from burn_depth_amd import ops
    H, W, K, depth, hp, faces = _round_trip_scene()
    pc = ops.unproject(dev, _t(depth), _t(K), dense=False, pixel_offset=0.5, mesh=dict(max_rtol=0.05))
    r = ops.render_mesh(dev, pc.xyz, pc.faces, H, W, _t(K), face_count=pc.face_count[-1:], pixel_offset=0.5)  # the mesh's own count word
    torch.cuda.synchronize()
    want = P.render_mesh(hp.xyz, faces, H, W, K, pixel_offset=0.5)
    _same(r, want, "round trip")
    _check_round_trip(want, depth, hp, faces)
    H, W, xyz, faces, K, E = _plane_scene()
    _check_no_cracks(_both(dev, xyz, faces, H, W, K, E, pixel_offset=0.5, what="plane"), H, W, xyz, K, E)


@gpu
def test_refusals_leave_the_outputs_untouched(dev, lib):
    xyz = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], device="cuda")  # one triangle over three pixels of 2 x 2
    row = torch.zeros(3, 3, dtype=torch.uint8, device="cuda")
    faces = torch.tensor([[0, 2, 1]], dtype=torch.int32, device="cuda")
    cams = torch.eye(3, device="cuda").reshape(1, 3, 3).contiguous()
    outs = dict(depth=torch.full((2, 2), 77.0, device="cuda"), face=torch.full((2, 2), 77, dtype=torch.int32, device="cuda"),
                rgb=torch.full((2, 2, 3), 77, dtype=torch.uint8, device="cuda"), filled=torch.full((2,), 77, dtype=torch.int32, device="cuda"),
                skipped=torch.full((2,), 77, dtype=torch.int32, device="cuda"))
    ptr = dict({k: v.data_ptr() for k, v in outs.items()}, xyz=xyz.data_ptr(), faces=faces.data_ptr(), K=cams.data_ptr(), rgb_row=row.data_ptr())
    for kw, code in REFUSALS:
        _refusal_call(lib, dev.handle, ptr, code, **kw)
    _refusal_call(lib, None, ptr, INV)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == 77).all(), k
    _refusal_call(lib, dev.handle, ptr, _lib.MD_OK)  # the same arguments without a fault are accepted
    torch.cuda.synchronize()
    assert outs["filled"].tolist() == [3, 3] and outs["face"].reshape(-1).tolist() == [0, 0, 0, -1] and outs["skipped"].tolist() == [0, 0]
