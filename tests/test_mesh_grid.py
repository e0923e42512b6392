"""Triangle mesh of the depth grid: md_op_mesh_grid (the face kernels on planted index maps) and its host reference
pipeline.pixel_index / pipeline.mesh_grid. include/mi_depth.h states the contract, DESIGN 12.5 the kernels. The outputs are
integers: every comparison is np.array_equal. The CPU tests check the vectorised reference against a per-quad loop written from
the contract text; the GPU tests (`-m gpu`, MI355X) check the kernels against the reference."""
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
from points_util import _bits, _t, dev, lib  # noqa: E402,F401

f32 = np.float32
NEW_ENTRIES = ("md_op_mesh_grid", "md_op_unproject_mesh", "md_infer_points_mesh")


def _loop_mesh(depth, index, stride=1, max_rtol=0.0, vertex_limit=0):
    """The contract once more, quad by quad with f32 scalars -> (faces, face_count)."""
    d, pi = np.asarray(depth, f32), np.asarray(index)
    B, H, W = d.shape
    hs, ws = -(-H // stride), -(-W // stride)
    rt = f32(max_rtol)

    def usable(i):
        return i >= 0 and (vertex_limit == 0 or i < vertex_limit)

    def edge(dx, dy):
        if max_rtol == 0:
            return True
        with np.errstate(all="ignore"):
            return bool(np.abs(f32(dx - dy)) <= f32(rt * np.fmin(dx, dy)))

    faces, count = [], []
    for b in range(B):
        n = 0
        for i in range(hs - 1):
            for j in range(ws - 1):
                at = {"a": (i, j), "b": (i, j + 1), "c": (i + 1, j), "d": (i + 1, j + 1)}
                row = {k: int(pi[b, v * stride, u * stride]) for k, (v, u) in at.items()}
                dep = {k: d[b, v * stride, u * stride] for k, (v, u) in at.items()}
                use = {k: usable(row[k]) for k in at}
                if all(use.values()):
                    with np.errstate(all="ignore"):
                        ad = bool(np.abs(f32(dep["a"] - dep["d"])) <= np.abs(f32(dep["b"] - dep["c"])))
                elif not use["a"] or not use["d"]:
                    ad = False
                else:
                    ad = True
                for tri in (("acd", "adb") if ad else ("acb", "bcd")):
                    if all(use[k] for k in tri) and all(edge(dep[x], dep[y]) for x, y in (tri[:2], tri[1:], tri[2] + tri[0])):
                        faces.append([row[k] for k in tri])
                        n += 1
        count.append(n)
    return np.asarray(faces, np.int32).reshape(-1, 3), np.asarray(count + [sum(count)], np.int32)


def _scene(B, H, W, seed, keep=0.85):
    """A smooth depth with planted steps (a raised rectangle and a far half plane) and a random mask -> (depth, mask)"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    d = np.stack([2.0 + 0.3 * np.sin(0.11 * u + b) + 0.2 * np.cos(0.07 * v) for b in range(B)]).astype(f32)
    d *= (1 + 0.004 * rng.standard_normal(d.shape)).astype(f32)
    d[:, H // 4:H // 2, W // 3:2 * W // 3] *= f32(0.8)
    d[:, :, 3 * W // 4:] *= f32(1.5)
    return d, rng.random((B, H, W)) < keep


def _same_as_loop(d, pi, **kw):
    faces, count = P.mesh_grid(d, pi, **kw)
    lf, lc = _loop_mesh(d, pi, **kw)
    assert faces.dtype == np.int32 and count.dtype == np.int32 and faces.shape[1:] == (3,)
    assert np.array_equal(count, lc), (kw, count, lc)
    assert np.array_equal(faces, lf), kw
    return faces, count


def _patterns_2x2():
    """The 16 usable-corner patterns of a 2 x 2 image as one batch: (depth [16,2,2], index [16,2,2]); rows count per view"""
    d = np.tile(np.array([[1.0, 1.2], [1.3, 1.05]], f32), (16, 1, 1))
    pi = np.full((16, 2, 2), -1, np.int32)
    n = 0
    for m in range(16):
        for k in range(4):
            if (m >> k) & 1:
                pi[m, k // 2, k % 2] = n
                n += 1
    return d, pi


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_mesh_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "} md_points_mesh;" in header
    assert [n for n, _ in _lib.MdPointsMesh._fields_] == ["max_rtol", "faces", "face_count", "face_capacity", "pixel_index"]


def test_the_sixteen_corner_patterns():
    d, pi = _patterns_2x2()
    faces, count = _same_as_loop(d, pi)
    # four usable corners: two faces; three: one; fewer: none
    want = [2 if m == 15 else int(bin(m).count("1") == 3) for m in range(16)]
    assert count[:16].tolist() == want and count[16] == sum(want)
    # |da - dd| = 0.05 < |db - dc|: the full quad splits along a-d; the rows of view 15 are the last four
    n = int(pi.max()) + 1
    a, b, c, dd = n - 4, n - 3, n - 2, n - 1
    assert faces[-2:].tolist() == [[a, c, dd], [a, dd, b]]
    # corner a missing (pattern 14) leaves (b, c, d), corner d missing (7) leaves (a, c, b), b missing (13) (a, c, d), c missing (11) (a, d, b)
    one = {m: faces[sum(want[:m])].tolist() for m in (14, 7, 13, 11)}
    r = lambda m: [int(v) for v in pi[m].reshape(-1)]  # noqa: E731  rows of a, b, c, d
    assert one[14] == [r(14)[1], r(14)[2], r(14)[3]] and one[7] == [r(7)[0], r(7)[2], r(7)[1]]
    assert one[13] == [r(13)[0], r(13)[2], r(13)[3]] and one[11] == [r(11)[0], r(11)[3], r(11)[1]]


def test_a_depth_step_cuts_exactly_one_edge_and_ties_take_a_d():
    pi = np.arange(4, dtype=np.int32).reshape(1, 2, 2)
    # only a-b is too long (0.06 > 0.05 * 1.0; d-b: 0.04 <= 0.05 * 1.02); diagonal a-d (0.02 <= 0.06): (a, c, d) stays, (a, d, b) goes
    d = np.array([[[1.0, 1.06], [1.0, 1.02]]], f32)
    faces, count = _same_as_loop(d, pi, max_rtol=0.05)
    assert faces.tolist() == [[0, 2, 3]] and count.tolist() == [1, 1]
    assert P.mesh_grid(d, pi)[1].tolist() == [2, 2]  # no cut without max_rtol
    # 3 x 3 with a far top right corner (row 2): quad (0, 1) keeps (a, c, d) = (1, 4, 5), the triangle that does not touch it,
    # and the quads (0, 0), (1, 0), (1, 1) stay whole
    d = np.ones((1, 3, 3), f32)
    d[0, 0, 2] = 2.0
    faces, count = _same_as_loop(d, np.arange(9, dtype=np.int32).reshape(1, 3, 3), max_rtol=0.05)
    assert count.tolist() == [7, 7] and faces[2:3].tolist() == [[1, 4, 5]] and not (faces == 2).any()
    # ties |da - dd| == |db - dc|: a-d
    for d in (np.ones((1, 2, 2), f32), np.array([[[1.0, 3.0], [2.0, 2.0]]], f32), np.array([[[1.0, 2.0], [3.0, 2.0]]], f32)):
        assert abs(d[0, 0, 0] - d[0, 1, 1]) == abs(d[0, 0, 1] - d[0, 1, 0])
        assert _same_as_loop(d, pi)[0].tolist() == [[0, 2, 3], [0, 3, 1]]
    # and the other diagonal when it is strictly shorter
    d = np.array([[[1.0, 2.0], [2.0, 3.0]]], f32)
    assert _same_as_loop(d, pi)[0].tolist() == [[0, 2, 1], [1, 2, 3]]
    # a not-a-number depth fails every edge it touches once max_rtol is on, and loses the diagonal comparison
    d = np.array([[[np.nan, 1.0], [1.0, 1.0]]], f32)
    assert _same_as_loop(d, pi, max_rtol=0.05)[0].tolist() == [[1, 2, 3]] and _same_as_loop(d, pi)[1].tolist() == [2, 2]


def test_max_rtol_exactly_at_and_one_ulp_below_the_threshold():
    pi = np.arange(4, dtype=np.int32).reshape(1, 2, 2)
    near, far = f32(1.0), f32(1.0) + f32(2.0 ** -4)
    d = np.array([[[near, near], [near, far]]], f32)  # the edges c-d and d-b carry the step 2^-4 = rtol * min exactly; diagonal b-c
    at = f32(2.0 ** -4)
    below = np.nextafter(at, f32(0))
    assert f32(at * near) == f32(far - near) and f32(below * near) < f32(far - near)
    assert _same_as_loop(d, pi, max_rtol=float(at))[1].tolist() == [2, 2]
    # one ulp below: d hangs on no edge, (b, c, d) goes and (a, c, b) stays
    faces, count = _same_as_loop(d, pi, max_rtol=float(below))
    assert faces.tolist() == [[0, 2, 1]] and count.tolist() == [1, 1]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_random_masks_against_the_loop(B, stride):
    H, W = 37, 53  # no multiple of 2 or 3 less one: the last lattice row and column are partial strides from the border
    d, mask = _scene(B, H, W, 5 + B)
    pi = P.pixel_index(mask, stride)
    rows = int(pi.max()) + 1
    on = np.zeros((B, H, W), bool)
    on[:, ::stride, ::stride] = mask[:, ::stride, ::stride]
    assert rows == on.sum() and np.array_equal(pi[on], np.arange(rows)) and (pi[~on] == -1).all()
    for rtol in (0.0, 0.05):
        faces, count = _same_as_loop(d, pi, stride=stride, max_rtol=rtol)
        assert count[-1] > 50 and (count[:B] > 0).all()
    assert P.mesh_grid(d, pi, stride=stride, max_rtol=0.05)[1][-1] < P.mesh_grid(d, pi, stride=stride)[1][-1]
    # a vertex limit that cuts the list in the middle of a lattice row of the last view
    ws = -(-W // stride)
    limit = rows - 3 * ws - ws // 2
    faces, count = _same_as_loop(d, pi, stride=stride, max_rtol=0.05, vertex_limit=limit)
    assert 0 < count[-1] and faces.max() < limit and faces.min() >= 0
    # a quad that loses a or d to the limit turns its diagonal: the faces are no subset of the unlimited ones
    assert count[-1] >= ((P.mesh_grid(d, pi, stride=stride, max_rtol=0.05)[0] < limit).all(1)).sum()


def test_pixel_index_of_the_host_points_and_vertex_bound():
    B, H, W = 2, 37, 53
    d, mask = _scene(B, H, W, 3)
    dm = np.where(mask, d, f32(0))  # depth 0 is never valid
    K = np.tile(np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]], f32), (B, 1, 1))
    for stride in (1, 2):
        hp = P.unproject_depth(dm, intrinsics=K, stride=stride, pixel_offset=0.5)
        pi = P.pixel_index(hp, stride)
        assert np.array_equal(pi, P.pixel_index(hp.mask, stride))
        sel = pi >= 0
        assert sel.sum() == hp.count[-1] and np.array_equal(_bits(hp.xyz[pi[sel]]), _bits(hp.point_map[sel]))
        for limit in (0, int(hp.count[-1]) // 2):
            faces, count = P.mesh_grid(dm, pi, stride=stride, max_rtol=0.05, vertex_limit=limit)
            assert len(faces) == count[-1] > 0 and faces.min() >= 0
            assert faces.max() < min(int(hp.count[-1]), limit or 2 ** 31)


def test_every_face_turns_its_front_to_the_camera():
    """In camera space, x right, y down, z forward, the contract's windings give ((p1 - p0) x (p2 - p0)).z < 0, evaluated in f64.
    The z component is the signed area of the triangle's x, y coordinates, x = rx d. Along an edge x1 - x0 = d1 / f + rx0 (d1 - d0),
    so the sign of the image-plane winding is kept as long as |rx0 (d1 - d0)| < d1 / f, i.e. |d1 - d0| / d < 1 / |u - cx|:
    at 37 x 53 with the principal point in the centre that is 1 / 27 = 3.7 %, and max_rtol = 0.01 keeps every emitted edge
    below it with room for both terms of the cross product."""
    B, H, W = 2, 37, 53
    d, mask = _scene(B, H, W, 8)
    rng = np.random.default_rng(1)
    d = (d * (1 + 0.005 * rng.standard_normal(d.shape))).astype(f32)  # rough enough that max_rtol cuts inside the smooth parts too
    dm = np.where(mask, d, f32(0))
    K = np.tile(np.array([[55.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], f32), (B, 1, 1))
    hp = P.unproject_depth(dm, intrinsics=K, pixel_offset=0.5, dtype=np.float64)
    faces, count = P.mesh_grid(dm, P.pixel_index(hp), max_rtol=0.01)
    assert count[-1] > 200 and count[-1] < P.mesh_grid(dm, P.pixel_index(hp))[1][-1]
    p0, p1, p2 = (hp.xyz[faces[:, k]].astype(np.float64) for k in range(3))
    z = np.cross(p1 - p0, p2 - p0)[:, 2]
    assert (z < 0).all(), float(z.max())


def _expected_ply(xyz, rgb=None, normals=None):
    """The bytes of a face-less file, put together from the format alone"""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}", "property float x", "property float y", "property float z"]
    cols = [np.asarray(xyz, "<f4").view(np.uint8).reshape(len(xyz), 12)]
    if normals is not None:
        head += ["property float nx", "property float ny", "property float nz"]
        cols.append(np.asarray(normals, "<f4").view(np.uint8).reshape(len(xyz), 12))
    if rgb is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
        cols.append(np.asarray(rgb, np.uint8))
    return ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + np.concatenate(cols, 1).tobytes()


def test_ply_without_faces_is_unchanged_and_faces_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    xyz = rng.normal(size=(257, 3)).astype(f32)
    nrm = rng.normal(size=(257, 3)).astype(f32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    faces = rng.integers(0, 257, (400, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    for col, n in ((None, None), (rgb, None), (rgb, nrm), (None, nrm)):
        P.write_ply(path, xyz, col, n)
        plain = open(path, "rb").read()
        assert plain == _expected_ply(xyz, col, n)
        P.write_ply(path, xyz, col, n, faces=None)
        assert open(path, "rb").read() == plain
        assert P.read_ply_faces(path)[3] is None
        P.write_ply(path, xyz, col, n, faces=faces)
        got = open(path, "rb").read()
        assert got[:got.index(b"element face")] == plain[:plain.index(b"end_header")]
        assert b"element face 400\nproperty list uchar int vertex_indices\nend_header\n" in got and len(got) == len(plain) + len("element face 400\nproperty list uchar int vertex_indices\n") + 400 * 13
        x2, c2, n2, f2 = P.read_ply_faces(path)
        assert np.array_equal(_bits(x2), _bits(xyz)) and f2.dtype == np.int32 and np.array_equal(f2, faces)
        assert ((c2 is None) if col is None else np.array_equal(c2, col)) and ((n2 is None) if n is None else np.array_equal(_bits(n2), _bits(n)))
        x3, c3, n3 = P.read_ply_normals(path)  # the older readers skip the faces
        assert np.array_equal(_bits(x3), _bits(xyz)) and ((c3 is None) if col is None else np.array_equal(c3, col))
    P.write_ply(path, xyz, faces=np.zeros((0, 3), np.int32))
    assert P.read_ply_faces(path)[3].shape == (0, 3)
    for bad in ([[0, 1, 257]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            P.write_ply(path, xyz, faces=np.asarray(bad))


def test_refusals_of_the_reference():
    d, pi = np.ones((1, 3, 3), f32), np.zeros((1, 3, 3), np.int32)
    for kw in (dict(stride=0), dict(max_rtol=-0.1), dict(max_rtol=float("nan")), dict(max_rtol=float("inf")), dict(vertex_limit=-1)):
        with pytest.raises(ValueError):
            P.mesh_grid(d, pi, **kw)
    with pytest.raises(ValueError):
        P.mesh_grid(d, pi[:, :2])
    with pytest.raises(ValueError):
        P.mesh_grid(d[0], pi[0])
    with pytest.raises(ValueError):
        P.mesh_grid(d, pi.astype(f32))
    with pytest.raises(ValueError):
        P.pixel_index(np.ones((3, 3), bool))
    with pytest.raises(ValueError):
        P.pixel_index(np.ones((1, 3, 3), bool), 0)
    for shape in ((1, 1, 1), (1, 1, 7), (1, 7, 1), (2, 2, 5)):  # no quads (at stride 3 for the last)
        faces, count = P.mesh_grid(np.ones(shape, f32), np.zeros(shape, np.int32), stride=3)
        assert faces.shape == (0, 3) and count.tolist() == [0] * (shape[0] + 1)


def test_mesh_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched. With a null device each call ends in an error whatever it is refused
    for, so the reason is read from md_last_error: a bad argument is refused for itself, the valid call last, for the null device."""
    buf = (C.c_int32 * 64)()
    px = C.cast(buf, C.c_void_p)
    E, S = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
    ok = dict(max_rtol=0.05, faces=px.value, face_count=px.value, face_capacity=4, pixel_index=None)

    def grid(B=1, H=2, W=2, stride=1, limit=0, depth=px, index=px, null=False, **kw):
        g = _lib.MdPointsMesh(**dict(ok, **kw))
        return lib.md_op_mesh_grid(None, depth, index, B, H, W, stride, limit, None if null else C.byref(g), None), lib.md_last_error().decode()

    for bad in (float("nan"), float("inf"), -0.25):
        rc, why = grid(max_rtol=bad)
        assert rc == E and "max_rtol" in why, bad
    for kw, word in ((dict(face_capacity=-1), "face_capacity"), (dict(face_count=None), "face_count"), (dict(stride=0), "stride"),
                     (dict(stride=-2), "stride"), (dict(limit=-1), "vertex_limit"), (dict(depth=None), "null"), (dict(index=None), "null"),
                     (dict(null=True), "mesh is null")):
        rc, why = grid(**kw)
        assert rc == E and word in why, (kw, why)
    for shape in ((1 << 10, 1 << 10, 1 << 10), (0, 2, 2), (1, 2, -1)):
        rc, why = grid(*shape)
        assert rc == S, (shape, why)
    assert "device is null" in grid()[1] and "device is null" in grid((1 << 10) - 1, 1 << 10, 1 << 10)[1]  # valid: the null device, last
    assert "device is null" in grid(max_rtol=0.0, faces=None)[1]

    # the combined operator: the mesh part is refused like the stand-alone one, and needs the list's count
    fbuf = (C.c_float * 64)()
    fx = C.cast(fbuf, C.c_void_p)
    cam = _lib.MdPointsCameras(fx.value, None, None)
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    dense = _lib.MdPointsOutputs(fx.value, None, None, None, None, None, 0, None)
    listed = _lib.MdPointsOutputs(None, None, fx.value, None, None, px.value, 4, None)

    def unproject(out, B=1, H=2, W=2, **kw):
        g = _lib.MdPointsMesh(**dict(ok, **kw))
        rc = lib.md_op_unproject_mesh(None, fx, None, None, B, H, W, C.byref(cam), C.byref(o), C.byref(out), None, C.byref(g), None)
        return rc, lib.md_last_error().decode()

    rc, why = unproject(listed)
    assert rc == E and "device is null" in why
    rc, why = unproject(dense)
    assert rc == E and "`count`" in why
    rc, why = unproject(dense, faces=None, face_count=None, pixel_index=px.value)
    assert rc == E and "`count`" in why
    assert "device is null" in unproject(dense, faces=None, face_count=None)[1]  # no mesh output: the call without a mesh
    assert "max_rtol" in unproject(listed, max_rtol=-1.0)[1] and "face_count" in unproject(listed, face_count=None)[1]
    rc, why = unproject(listed, 1 << 10, 1 << 10, 1 << 10)
    assert rc == S and "2^30" in why
    assert lib.md_op_unproject_mesh(None, fx, None, None, 1, 2, 2, C.byref(cam), C.byref(o), C.byref(listed), None, None, None) == E
    assert "device is null" in lib.md_last_error().decode()  # mesh NULL: md_op_unproject_normals

    # the model call: a null model is refused first; the mesh refusals run on a model in test_points_mesh.py
    g = _lib.MdPointsMesh(**ok)
    assert lib.md_infer_points_mesh(None, fx, 1, 2, 2, 1, None, None, None, C.byref(o), C.byref(listed), None, None, None, C.byref(g), 1, None) == E
    assert "model is null" in lib.md_last_error().decode()
    assert (np.frombuffer(buf, np.int32) == 0).all() and (np.frombuffer(fbuf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: md_op_mesh_grid on planted index maps
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = -7
CANARY = 48  # int32 words behind the end of the face buffer


def _run(dev, d, pi, stride=1, max_rtol=0.0, vertex_limit=0, face_capacity=None):
    """ops.mesh_grid on poisoned outputs with a canary tail -> (faces [cap,3] as written, face_count, the words behind the capacity)"""
    from burn_depth_amd import ops
    B, H, W = d.shape
    full = 2 * B * (-(-H // stride) - 1) * (-(-W // stride) - 1)
    cap = full if face_capacity is None else face_capacity
    store = torch.full((max(cap, 1) * 3 + CANARY,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((B + 1 + CANARY,), POISON, dtype=torch.int32, device="cuda")
    faces = store[:max(cap, 1) * 3].view(-1, 3)
    ops.mesh_grid(dev, _t(d), _t(pi), stride=stride, max_rtol=max_rtol, vertex_limit=vertex_limit, face_capacity=cap, faces=faces, face_count=count)
    torch.cuda.synchronize()
    assert (count[B + 1:] == POISON).all()
    return store.cpu().numpy()[:cap * 3].reshape(-1, 3), count[:B + 1].cpu().numpy(), store.cpu().numpy()[cap * 3:]


def _check(dev, d, pi, what, **kw):
    """ample capacity, capacity 0 and a capacity in the middle of the list, each against the reference"""
    want, wc = P.mesh_grid(d, pi, **kw)
    n = len(want)
    for cap in dict.fromkeys((None, 0, n // 2)):
        got, gc, tail = _run(dev, d, pi, face_capacity=cap, **kw)
        assert np.array_equal(gc, wc), (what, cap, gc, wc)  # the true totals, whatever the capacity
        m = min(n, len(got))
        assert np.array_equal(got[:m], want[:m]), (what, cap)
        assert (got[m:] == POISON).all() and (tail == POISON).all(), (what, cap)
    return wc


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1)])
def test_images_without_quads(dev, H, W):
    for B in (1, 3):
        d, mask = _scene(B, H, W, 2)
        got, gc, tail = _run(dev, d, P.pixel_index(mask), face_capacity=5)
        assert gc.tolist() == [0] * (B + 1) and (got == POISON).all() and (tail == POISON).all()
    d, mask = _scene(1, 2, 70, 2)
    _, gc, _ = _run(dev, d, P.pixel_index(mask, 2), stride=2, face_capacity=5)  # one lattice row at stride 2
    assert gc.tolist() == [0, 0]


@pytest.mark.gpu
def test_the_sixteen_corner_patterns_on_the_device(dev):
    d, pi = _patterns_2x2()
    wc = _check(dev, d, pi, "2 x 2")
    assert wc[-1] == 6
    _check(dev, d, pi, "2 x 2, limit", vertex_limit=int(pi.max()) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(65, 64), (37, 53), (96, 96)])
def test_faces_are_identical_to_the_host_reference(dev, B, H, W):
    """65 x 64: the quad lattice is 64 x 63, so the ballot words straddle lattice rows. 96 x 96: 9025 quads, three workgroups
    with a tail. Stride 2 and 3 leave partial strides at the border of every shape."""
    d, mask = _scene(B, H, W, 20 + H)
    for stride in (1, 2, 3):
        pi = P.pixel_index(mask, stride)
        rows = int(pi.max()) + 1
        for rtol in (0.0, 0.05):
            for limit in (0, rows // 2 + 3):
                wc = _check(dev, d, pi, (stride, rtol, limit), stride=stride, max_rtol=rtol, vertex_limit=limit)
                assert wc[-1] > 0
        cut, whole = P.mesh_grid(d, pi, stride=stride, max_rtol=0.05)[1][-1], P.mesh_grid(d, pi, stride=stride)[1][-1]
        assert cut < whole  # the planted steps are cut


@pytest.mark.gpu
def test_all_kept_and_none_kept_maps(dev):
    B, H, W = 2, 96, 96
    d, _ = _scene(B, H, W, 4)
    wc = _check(dev, d, P.pixel_index(np.ones((B, H, W), bool)), "all kept")
    assert wc.tolist() == [2 * 95 * 95, 2 * 95 * 95, 4 * 95 * 95]
    wc = _check(dev, d, np.full((B, H, W), -1, np.int32), "none kept", max_rtol=0.05)
    assert wc.tolist() == [0, 0, 0]
    # an arbitrary planted map (rows in no order, repeated, beyond any list) is taken as it is
    rng = np.random.default_rng(0)
    pi = rng.integers(-3, 1 << 30, (B, H, W)).astype(np.int32)
    _check(dev, d, pi, "planted", max_rtol=0.05, vertex_limit=1 << 29)
