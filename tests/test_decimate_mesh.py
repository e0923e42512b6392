"""Vertex-clustering decimation of a mesh: md_op_decimate_mesh and its host reference pipeline.decimate_mesh. include/mi_depth.h
states the contract, DESIGN 12.8 the kernels. Selection only: a vertex is an input row and a face an input face with new
indices, so every comparison is bit for bit.

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
from points_util import _bits, _t, dev, lib  # noqa: E402,F401

f32 = np.float32
HALF = 1 << 20


def _loop_decimate(xyz, faces, voxel, conf=None, capacity=None, face_counts=None):
    """The contract once more, row by row and face by face with dictionaries -> (index, remap, faces, face_index, face_count,
    faces_dropped)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    N, vs = len(xyz), f32(voxel)
    cell_of, best = {}, {}
    for i, p in enumerate(xyz):
        with np.errstate(all="ignore"):
            c = [np.floor(f32(a) / vs) for a in p]
        if not all(np.isfinite(a) for a in p) or not all(-HALF <= a < HALF for a in c):
            continue
        key = tuple(int(a) for a in c)
        cell_of[i] = key
        w = f32(0)
        if conf is not None and np.isfinite(conf[i]) and conf[i] >= 0:
            w = f32(conf[i]) + f32(0)
        if key not in best or w > best[key][0]:
            best[key] = (w, i)
    index = sorted(i for _, i in best.values())
    row_of = {i: r for r, i in enumerate(index)}
    remap = [row_of[best[cell_of[i]][1]] if i in cell_of else -1 for i in range(N)]
    cap = N if capacity is None else capacity
    seen, kept, kept_index, dropped = {}, [], [], [0, 0, 0]
    for f, tri in enumerate(np.asarray(faces, np.int64).reshape(-1, 3).tolist()):
        if any(c < 0 or c >= N for c in tri):
            dropped[0] += 1
            continue
        m = [remap[c] for c in tri]
        if any(c < 0 or c >= cap for c in m):
            dropped[0] += 1
            continue
        if m[0] == m[1] or m[1] == m[2] or m[0] == m[2]:
            dropped[1] += 1
            continue
        k = m.index(min(m))
        rot = (m[k], m[(k + 1) % 3], m[(k + 2) % 3])
        if rot in seen:
            dropped[2] += 1
            continue
        seen[rot] = f
        kept.append(m)
        kept_index.append(f)
    F = len(np.asarray(faces).reshape(-1, 3))
    b = np.minimum(np.concatenate([[0], np.cumsum([F] if face_counts is None else face_counts)]), F)
    ki = np.array(kept_index, np.int64)
    per_view = [int(((ki >= b[i]) & (ki < b[i + 1])).sum()) for i in range(len(b) - 1)]
    return (np.array(index, np.int32), np.array(remap, np.int32), np.array(kept, np.int32).reshape(-1, 3), ki.astype(np.int32),
            np.array(per_view + [len(ki)], np.int32), np.array(dropped, np.int32))


def _check_against_loop(xyz, faces, voxel, conf=None, capacity=None, face_counts=None):
    r = P.decimate_mesh(xyz, faces, voxel, conf, capacity=capacity, face_counts=face_counts)
    index, remap, kept, kept_index, face_count, dropped = _loop_decimate(xyz, faces, voxel, conf, capacity, face_counts)
    assert np.array_equal(r.vertices.index, index)
    assert np.array_equal(r.remap, remap)
    assert np.array_equal(r.faces, kept) and np.array_equal(r.face_index, kept_index)
    assert np.array_equal(r.face_count, face_count) and np.array_equal(r.faces_dropped, dropped)
    assert r.faces_dropped.sum() + len(r.faces) == len(np.asarray(faces).reshape(-1, 3))
    assert r.remap.dtype == np.int32 and r.faces.dtype == np.int32 and r.face_index.dtype == np.int32
    return r


def _cloud(n, side, seed):
    """n points uniform in a cube of `side`^3 voxels of size 0.25 around the origin, distinct confidences in (0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-side / 2, side / 2, (n, 3)) * 0.25).astype(f32)
    conf = (0.5 + rng.permutation(n) / n).astype(f32)
    return xyz, conf


def _random_faces(nf, n, seed, bad=0):
    """nf random triples over n rows; `bad` of them get a corner of -1 or n"""
    rng = np.random.default_rng(seed)
    faces = rng.integers(0, n, (nf, 3)).astype(np.int32)
    if bad:
        rows = rng.permutation(nf)[:bad]
        faces[rows, rng.integers(0, 3, bad)] = np.array([-1, n, -(1 << 31), (1 << 31) - 1], np.int64)[rng.integers(0, 4, bad)].astype(np.int32)
    return faces


_PLANE = {}


def _plane_scene():
    """Two noisy views of one tilted plane at 2 x 37 x 53, identity cameras: 3922 vertices, 7488 faces, the sheets overlap."""
    if not _PLANE:
        u = np.arange(53, dtype=f32)[None, None, :]
        v = np.arange(37, dtype=f32)[None, :, None]
        noise = np.random.default_rng(0).standard_normal((2, 37, 53))
        depth = (2 + 0.01 * u + 0.02 * v + 0.002 * noise).astype(f32)
        hp = P.unproject_depth(depth, focal_px=np.full(2, 60, f32))
        faces, face_count = P.mesh_grid(depth, P.pixel_index(hp.mask))
        rng = np.random.default_rng(1)
        _PLANE.update(xyz=hp.xyz, faces=faces, face_count=face_count, count=hp.count, conf=rng.random(len(hp.xyz)).astype(f32),
                      rgb=rng.integers(0, 256, (len(hp.xyz), 3), dtype=np.uint8), normals=rng.normal(size=(len(hp.xyz), 3)).astype(f32))
        for a in _PLANE.values():
            a.setflags(write=False)
    return _PLANE


def _reversed_pairs(faces):
    """kept faces whose reversed triple is kept too"""
    def rot(t):
        k = t.index(min(t))
        return (t[k], t[(k + 1) % 3], t[(k + 2) % 3])
    have = {rot(t) for t in faces.tolist()}
    return sum(rot(t[::-1]) in have for t in faces.tolist()) // 2


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_decimate_entry(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    assert "md_op_decimate_mesh" in declared, "include/mi_depth.h does not declare md_op_decimate_mesh"
    assert hasattr(raw, "md_op_decimate_mesh"), "libmi_depth.so does not export md_op_decimate_mesh"
    assert "md_op_decimate_mesh" in _lib.SYMBOLS
    assert "} md_points_decimate;" in header
    assert [n for n, _ in _lib.MdPointsDecimate._fields_] == ["voxel", "index", "weight", "dropped", "remap", "faces", "face_index", "face_count",
                                                              "face_capacity", "faces_dropped"]
    assert C.sizeof(_lib.MdPointsDecimate) == 80  # a float padded to 8, eight pointers, one int64
    assert "reversed triple is a DIFFERENT face" in header  # the orientation decision is part of the contract


def test_reference_against_the_per_face_loop():
    for n, nf, side, seed in ((1, 5, 4, 0), (300, 900, 4, 1), (2000, 5000, 6, 2), (500, 700, 64, 3)):
        xyz, conf = _cloud(n, side, seed)
        faces = _random_faces(nf, n, seed + 10, bad=nf // 20)
        r = _check_against_loop(xyz, faces, 0.25, conf)
        _check_against_loop(xyz, faces, 0.25)
        assert (np.diff(r.face_index) > 0).all()
    assert len(P.decimate_mesh(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), 1.0).faces) == 0
    r = P.decimate_mesh(np.zeros((0, 3), f32), np.array([[0, 1, 2]], np.int32), 1.0)  # no vertices: every face is invalid
    assert r.faces_dropped.tolist() == [1, 0, 0] and r.face_count.tolist() == [0, 0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.decimate_mesh(xyz, faces, bad)
    with pytest.raises(ValueError):
        P.decimate_mesh(xyz, faces, 0.25, capacity=-1)


def test_reference_clause_by_clause():
    # five vertices in their own voxels of side 1, vertex 5 shares voxel 0 with vertex 0, vertex 6 is NaN, vertex 7 out of range
    xyz = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [4.5, 0.5, 0.5], [0.6, 0.6, 0.6], [np.nan, 0, 0],
                    [3e7, 0, 0]], f32)
    N = len(xyz)
    dec = lambda faces, **kw: _check_against_loop(xyz, np.array(faces, np.int32), 1.0, **kw)  # noqa: E731
    assert dec([[0, 1, 2]]).remap.tolist() == [0, 1, 2, 3, 4, 0, -1, -1]
    # the three rotations of a triple are duplicates of the first; it keeps the rotation it came in
    r = dec([[1, 2, 0], [0, 1, 2], [2, 0, 1], [1, 2, 0]])
    assert r.faces.tolist() == [[1, 2, 0]] and r.face_index.tolist() == [0] and r.faces_dropped.tolist() == [0, 0, 3]
    # the reversal is the other side of a fold and is kept
    r = dec([[0, 1, 2], [2, 1, 0], [0, 2, 1]])
    assert r.faces.tolist() == [[0, 1, 2], [2, 1, 0]] and r.faces_dropped.tolist() == [0, 0, 1]
    # two corners in one voxel: degenerate (5 maps to row 0); through remap a duplicate can come from other input corners
    r = dec([[0, 5, 1], [5, 1, 2], [0, 1, 2], [3, 3, 4]])
    assert r.faces.tolist() == [[0, 1, 2]] and r.face_index.tolist() == [1] and r.faces_dropped.tolist() == [0, 2, 1]
    # the class order: an invalid face is not counted as degenerate ...
    r = dec([[6, 6, 1], [-1, -1, 0], [N, N, N], [7, 7, 7]])
    assert r.faces_dropped.tolist() == [4, 0, 0] and len(r.faces) == 0
    # ... and neither an invalid nor a degenerate face shadows a later valid copy: they never enter the set
    r = dec([[0, 1, 6], [0, 0, 1], [0, 1, 2], [0, 5, 1], [1, 2, 0]])
    assert r.face_index.tolist() == [2] and r.faces_dropped.tolist() == [1, 2, 1]
    # corner indices -1 and N, a NaN vertex and a vertex out of range
    r = dec([[-1, 1, 2], [0, N, 2], [0, 1, 6], [7, 1, 2], [2, 3, 4]])
    assert r.face_index.tolist() == [4] and r.faces_dropped.tolist() == [4, 0, 0]
    # remap >= capacity: rows 3 and 4 are not written with capacity 3, so no kept face may name them; remap stays the true rank
    r = dec([[0, 1, 2], [1, 2, 3], [2, 3, 4], [2, 1, 0]], capacity=3)
    assert r.remap.tolist() == [0, 1, 2, 3, 4, 0, -1, -1]
    assert r.face_index.tolist() == [0, 3] and r.faces_dropped.tolist() == [2, 0, 0]
    assert int(r.vertices.count[-1]) == 5  # the true count, beyond the capacity
    assert dec([[0, 1, 2]], capacity=0).faces_dropped.tolist() == [1, 0, 0]


def test_reference_vertices_are_voxel_thinning():
    xyz, conf = _cloud(3000, 8, 4)
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (3000, 3), dtype=np.uint8)
    nrm = rng.normal(size=(3000, 3)).astype(f32)
    xyz[rng.permutation(3000)[:50], 0] = np.nan
    faces = _random_faces(4000, 3000, 6)
    r = P.decimate_mesh(xyz, faces, 0.25, conf, rgb, nrm, counts=[1000, 0, 2000])
    t = P.voxel_thin(xyz, 0.25, conf, rgb, nrm, counts=[1000, 0, 2000])
    for k in ("xyz", "conf", "normals"):
        assert np.array_equal(_bits(getattr(r.vertices, k)), _bits(getattr(t, k))), k
    for k in ("rgb", "index", "weight", "count"):
        assert np.array_equal(getattr(r.vertices, k), getattr(t, k)), k
    assert r.vertices.dropped == t.dropped == 50
    # remap names the survivor of the row's voxel: the same cell, and the survivors map to themselves
    ok = r.remap >= 0
    assert (~ok).sum() == 50
    assert np.array_equal(np.floor(t.xyz[r.remap[ok]] / f32(0.25)), np.floor(xyz[ok] / f32(0.25)))
    assert np.array_equal(r.remap[t.index], np.arange(len(t.index)))
    # unreferenced vertices stay in the list
    few = P.decimate_mesh(xyz, faces[:3], 0.25, conf)
    assert np.array_equal(few.vertices.index, t.index)


def test_reference_shuffle_and_per_view_counts():
    xyz, conf = _cloud(1500, 3, 7)  # 64 voxels: collapsed faces and copies by the hundred
    faces = _random_faces(6000, 1500, 8, bad=100)
    a = P.decimate_mesh(xyz, faces, 0.25, conf)
    assert a.faces_dropped.min() > 50 and len(a.faces) > 500

    def smallest(r, order):  # oriented triangle -> its smallest source face in the unshuffled numbering
        out = {}
        for t, f in zip(r.faces.tolist(), order[r.face_index].tolist()):
            k = t.index(min(t))
            out[(t[k], t[(k + 1) % 3], t[(k + 2) % 3])] = f
        return out

    perm = np.random.default_rng(9).permutation(6000)
    b = P.decimate_mesh(xyz, faces[perm], 0.25, conf)
    assert np.array_equal(a.faces_dropped, b.faces_dropped)
    sa, sb = smallest(a, np.arange(6000)), smallest(b, perm)
    assert sa.keys() == sb.keys()  # the same set of triangles survives
    copies = {}  # oriented triangle -> the source faces that map to it, from remap alone
    for f, t in enumerate(faces.tolist()):
        if all(0 <= c < 1500 for c in t):
            m = [int(a.remap[c]) for c in t]
            if min(m) >= 0 and len(set(m)) == 3:
                k = m.index(min(m))
                copies.setdefault((m[k], m[(k + 1) % 3], m[(k + 2) % 3]), []).append(f)
    assert copies.keys() == sa.keys()
    inv = np.argsort(perm)  # the position of source face f in the shuffled order
    for tri, fs in copies.items():  # each call kept, of every triangle, the copy with the smallest index in ITS order
        assert sa[tri] == min(fs) and sb[tri] == min(fs, key=lambda f: inv[f])
    _check_against_loop(xyz, faces[perm], 0.25, conf)
    # per-view face counts follow the views of the source faces
    r = _check_against_loop(xyz, faces, 0.25, conf, face_counts=[1000, 0, 3000, 2000])
    edges = np.array([0, 1000, 1000, 4000, 6000])
    assert r.face_count.tolist() == [int(((r.face_index >= edges[i]) & (r.face_index < edges[i + 1])).sum()) for i in range(4)] + [len(r.faces)]
    assert r.face_count[1] == 0


def test_reference_on_the_plane_scene_where_every_class_occurs():
    s = _plane_scene()
    assert len(s["xyz"]) == 3922 and len(s["faces"]) == 7488
    for voxel, verts, dropped, kept in ((0.05, 1766, [0, 1352, 2082], 4054), (0.1, 565, None, 1214)):
        r = P.decimate_mesh(s["xyz"], s["faces"], voxel, face_counts=s["face_count"][:-1], counts=s["count"][:-1])
        assert int(r.vertices.count[-1]) == verts and len(r.faces) == kept
        if dropped:
            assert r.faces_dropped.tolist() == dropped
        assert r.faces_dropped[1] > 0 and r.faces_dropped[2] > 0 and r.faces_dropped.sum() + kept == 7488
        assert r.face_count[0] + r.face_count[1] == kept and r.face_count[0] > r.face_count[1] > 0  # the second sheet is mostly copies
        assert _reversed_pairs(r.faces) >= 1
        assert r.faces.min() >= 0 and r.faces.max() < verts
    s = _plane_scene()
    bad = np.array(s["faces"][:200])
    bad[::2, 1] = -1
    faces = np.concatenate([bad, s["faces"]])
    r = _check_against_loop(s["xyz"], faces, 0.05, s["conf"])
    assert (r.faces_dropped > 0).all()


def test_decimate_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched: with a null device the valid call is refused last, for the device."""
    buf = (C.c_float * 64)()
    px = C.cast(buf, C.c_void_p)
    listed = _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, 4, None)
    no_count = _lib.MdPointsOutputs(None, None, None, None, None, None, 4, None)

    def D(voxel=0.5, index=None, weight=None, dropped=None, remap=None, faces=None, face_index=None, face_count=None, face_capacity=4,
          faces_dropped=None):
        return _lib.MdPointsDecimate(voxel, index, weight, dropped, remap, faces, face_index, face_count, face_capacity, faces_dropped)

    def why(dec, out=listed, N=4, F=4, code=_lib.MD_ERR_INVALID_ARG, conf=None, normals_out=None, faces=px, xyz=px):
        rc = lib.md_op_decimate_mesh(None, xyz, conf, None, None, N, faces, F, C.byref(dec) if dec else None, C.byref(out), normals_out, None)
        assert rc == code, rc
        return lib.md_last_error().decode()

    for bad in (float("nan"), float("inf"), -0.5, 0.0):
        assert "voxel" in why(D(bad)), bad
    assert "face_capacity" in why(D(face_capacity=-1))
    assert "capacity" in why(D(), _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, -1, None))
    assert "need `face_count`" in why(D(faces=px.value))
    assert "need `face_count`" in why(D(face_index=px.value))
    assert "need `count`" in why(D(index=px.value), no_count)
    assert "need `count`" in why(D(weight=px.value), no_count)
    assert "need `count`" in why(D(), _lib.MdPointsOutputs(None, None, px.value, None, None, None, 4, None))
    assert "negative" in why(D(), N=-1)
    assert "negative" in why(D(), F=-1)
    assert "2^30" in why(D(), N=1 << 30, code=_lib.MD_ERR_SHAPE)
    assert "2^30" in why(D(), F=1 << 30, code=_lib.MD_ERR_SHAPE)
    assert "confidence row" in why(D(), _lib.MdPointsOutputs(None, None, px.value, None, px.value, px.value, 4, None))
    assert "normals row" in why(D(), normals_out=px)
    assert "dense" in why(D(), _lib.MdPointsOutputs(px.value, None, px.value, None, None, px.value, 4, None))
    assert "faces pointer" in why(D(), faces=None)
    assert "xyz pointer" in why(D(), xyz=None)
    assert "options are null" in why(None)
    assert "device is null" in why(D(0.5, px.value, px.value, px.value, px.value, px.value, px.value, px.value, 4, px.value))
    assert (np.frombuffer(buf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0
CANARY = 16  # elements behind the end of every output buffer
FILLS = dict(xyz=POISON, conf=POISON, rgb=77, normals=POISON, index=-7, weight=-7, count=-5, dropped=-5, remap=-9, faces=-11, face_index=-11,
             face_count=-5, faces_dropped=-5)


def _fresh(n, cap, fcap, conf, rgb, normals):
    from burn_depth_amd.depth_pro import PointCloud
    out, stores = PointCloud(), {}

    def put(name, shape, dtype=torch.float32):
        size = int(np.prod(shape))
        stores[name] = torch.full((size + CANARY,), FILLS[name], dtype=dtype, device="cuda")
        setattr(out, name, stores[name][:size].view(shape))

    put("xyz", (cap, 3))
    for name, shape in (("index", (cap,)), ("weight", (cap,)), ("count", (2,)), ("dropped", (1,)), ("remap", (n,)), ("faces", (fcap, 3)),
                        ("face_index", (fcap,)), ("face_count", (2,)), ("faces_dropped", (3,))):
        put(name, shape, torch.int32)
    if conf:
        put("conf", (cap,))
    if rgb:
        put("rgb", (cap, 3), torch.uint8)
    if normals:
        put("normals", (cap, 3))
    return out, stores


def _run(dev, xyz, faces, voxel, conf=None, rgb=None, normals=None, capacity=None, face_capacity=None):
    """ops.decimate_mesh on poisoned, guarded outputs -> numpy dict"""
    from burn_depth_amd import ops
    cap = len(xyz) if capacity is None else capacity
    fcap = len(faces) if face_capacity is None else face_capacity
    out, stores = _fresh(len(xyz), cap, fcap, conf is not None, rgb is not None, normals is not None)
    ops.decimate_mesh(dev, _t(xyz), _t(faces), voxel, conf=_t(conf), rgb=_t(rgb), normals=_t(normals), out=out)
    torch.cuda.synchronize()
    for name, store in stores.items():
        assert (store[-CANARY:] == FILLS[name]).all(), name
    return {k: v.cpu().numpy() for k, v in vars(out).items() if v is not None}


def _assert_same(got, ref, what=""):
    """every output of the operator against the reference (computed with the same capacity), and the rows behind them untouched"""
    v = ref.vertices
    assert got["count"].tolist() == [int(v.count[-1])] * 2, (what, got["count"], v.count)
    assert int(got["dropped"][0]) == v.dropped, what
    n = min(int(v.count[-1]), got["xyz"].shape[0])
    for k in ("xyz", "conf", "normals"):
        if k in got:
            assert np.array_equal(_bits(got[k][:n]), _bits(getattr(v, k)[:n])), (what, k)
            assert (got[k][n:] == f32(POISON)).all(), (what, k)
    if "rgb" in got:
        assert np.array_equal(got["rgb"][:n], v.rgb[:n]) and (got["rgb"][n:] == 77).all(), what
    for k in ("index", "weight"):
        assert np.array_equal(got[k][:n], getattr(v, k)[:n]) and (got[k][n:] == -7).all(), (what, k)
    assert np.array_equal(got["remap"], ref.remap), what
    assert got["face_count"].tolist() == ref.face_count.tolist(), (what, got["face_count"], ref.face_count)
    assert got["faces_dropped"].tolist() == ref.faces_dropped.tolist(), (what, got["faces_dropped"], ref.faces_dropped)
    nf = min(len(ref.faces), got["faces"].shape[0])
    assert np.array_equal(got["faces"][:nf], ref.faces[:nf]) and (got["faces"][nf:] == -11).all(), what
    assert np.array_equal(got["face_index"][:nf], ref.face_index[:nf]) and (got["face_index"][nf:] == -11).all(), what


_FIXED = {}


def _fixed_vertices():
    """700 vertices in 64 voxels with distinct confidences, and 4097 random faces over them, a twentieth with a bad corner"""
    if not _FIXED:
        xyz, conf = _cloud(700, 3, 30)
        _FIXED.update(xyz=xyz, conf=conf, faces=_random_faces(4097, 700, 31, bad=200))
        for a in _FIXED.values():
            a.setflags(write=False)
    return _FIXED


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [1, 63, 64, 65, 4095, 4096, 4097])
def test_wave_and_workgroup_edges_are_bit_identical_to_the_host_reference(dev, nf):
    s = _fixed_vertices()
    faces = s["faces"][:nf]
    ref = P.decimate_mesh(s["xyz"], faces, 0.25, s["conf"])
    if nf >= 4095:
        assert (ref.faces_dropped > 0).all() and len(ref.faces) > 1000
    _assert_same(_run(dev, s["xyz"], faces, 0.25, s["conf"]), ref, nf)


@pytest.mark.gpu
def test_ten_thousand_copies_of_one_triangle_leave_face_zero(dev):
    xyz = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5]], f32)
    rot = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]], np.int32)
    faces = rot[np.random.default_rng(1).integers(0, 3, 10000)]
    faces[0] = [1, 2, 0]
    got = _run(dev, xyz, faces, 1.0)
    _assert_same(got, P.decimate_mesh(xyz, faces, 1.0))
    assert got["face_count"].tolist() == [1, 1] and got["faces_dropped"].tolist() == [0, 0, 9999]
    assert got["face_index"][0] == 0 and got["faces"][0].tolist() == [1, 2, 0]


@pytest.mark.gpu
def test_ten_thousand_distinct_faces_are_all_kept(dev):
    n = 150  # every vertex in its own voxel; the first 10 000 of the 150 * 149 * 148 / 3 oriented triangles with a < b, a < c
    xyz = (np.stack([np.arange(n) % 8, np.arange(n) // 8 % 8, np.arange(n) // 64], 1) + 0.5).astype(f32)
    tri = [(a, b, c) for a in range(3) for b in range(a + 1, n) for c in range(a + 1, n) if b != c][:10000]
    rng = np.random.default_rng(2)
    faces = np.array(tri, np.int32)[rng.permutation(10000)]
    faces = np.stack([np.roll(f, k) for f, k in zip(faces, rng.integers(0, 3, 10000))])  # mixed rotations, both windings of many pairs
    got = _run(dev, xyz, faces, 1.0)
    _assert_same(got, P.decimate_mesh(xyz, faces, 1.0))
    assert got["face_count"].tolist() == [10000, 10000] and got["faces_dropped"].tolist() == [0, 0, 0]
    assert np.array_equal(got["faces"], faces) and np.array_equal(got["face_index"], np.arange(10000))


@pytest.mark.gpu
@pytest.mark.parametrize("voxel", [0.05, 0.1])
@pytest.mark.parametrize("carried", [False, True])
def test_plane_scene_with_and_without_the_carried_rows(dev, voxel, carried):
    s = _plane_scene()
    rows = dict(conf=s["conf"], rgb=s["rgb"], normals=s["normals"]) if carried else {}
    ref = P.decimate_mesh(s["xyz"], s["faces"], voxel, **rows)
    assert (ref.faces_dropped[1:] > 0).all() and _reversed_pairs(ref.faces) >= 1
    got = _run(dev, s["xyz"], s["faces"], voxel, **rows)
    _assert_same(got, ref, (voxel, carried))
    assert ("conf" in got) == carried


@pytest.mark.gpu
def test_vertex_outputs_are_voxel_thinnings(dev):
    from burn_depth_amd import ops
    s = _plane_scene()
    got = _run(dev, s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], s["normals"])
    thin = ops.voxel_thin(dev, _t(s["xyz"]), 0.05, conf=_t(s["conf"]), rgb=_t(s["rgb"]), normals=_t(s["normals"]))
    torch.cuda.synchronize()
    n = int(thin.count[-1].item())
    assert got["count"].tolist() == thin.count.tolist() and got["dropped"].tolist() == thin.dropped.tolist()
    for k in ("xyz", "conf", "rgb", "normals", "index", "weight"):
        assert np.array_equal(got[k][:n].view(np.uint8), getattr(thin, k)[:n].cpu().numpy().view(np.uint8)), k


@pytest.mark.gpu
def test_capacities_below_the_outputs_keep_the_true_counts(dev):
    s = _plane_scene()
    full = P.decimate_mesh(s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"])
    M, K = int(full.vertices.count[-1]), len(full.faces)
    for fcap in (K // 2, 1, 0, K - 1):  # face_capacity < kept: the true total, the rows behind it untouched (_run's sentinels)
        got = _run(dev, s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], face_capacity=fcap)
        assert got["faces"].shape[0] == fcap
        _assert_same(got, full, ("fcap", fcap))
    for cap in (M // 2, 1, 0, M - 1):  # capacity < M: faces that name an unwritten row are invalid; remap stays the true rank
        ref = P.decimate_mesh(s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], capacity=cap)
        assert ref.faces_dropped[0] > 0 and np.array_equal(ref.remap, full.remap)
        got = _run(dev, s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], capacity=cap)
        _assert_same(got, ref, ("cap", cap))
        n = min(int(got["face_count"][-1]), got["faces"].shape[0])
        assert n == 0 or got["faces"][:n].max() < cap


@pytest.mark.gpu
def test_invalid_indices_and_non_finite_vertices(dev):
    s = _plane_scene()
    xyz = np.array(s["xyz"])
    rng = np.random.default_rng(3)
    bad = rng.permutation(len(xyz))[:300]
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:200], rng.integers(0, 3, 100)] = np.inf
    xyz[bad[200:], 0] = f32(HALF) * f32(0.05) * f32(1.5)  # beyond the grid
    faces = np.array(s["faces"])
    rows = rng.permutation(len(faces))[:400]
    faces[rows, rng.integers(0, 3, 400)] = np.array([-1, len(xyz), -(1 << 31), (1 << 31) - 1], np.int64)[rng.integers(0, 4, 400)].astype(np.int32)
    ref = P.decimate_mesh(xyz, faces, 0.05, s["conf"])
    assert ref.vertices.dropped == 300 and ref.faces_dropped[0] > 400 and (ref.remap == -1).sum() == 300
    _assert_same(_run(dev, xyz, faces, 0.05, s["conf"]), ref)
    nothing = _run(dev, np.full((70, 3), np.nan, f32), faces[:100] % 70, 1.0)
    assert nothing["count"].tolist() == [0, 0] and nothing["face_count"].tolist() == [0, 0] and nothing["faces_dropped"].tolist() == [100, 0, 0]
    assert (nothing["remap"] == -1).all()


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_empty_lists_are_no_error(dev):
    from burn_depth_amd import ops
    s = _plane_scene()
    a = _run(dev, s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], s["normals"])
    b = _run(dev, s["xyz"], s["faces"], 0.05, s["conf"], s["rgb"], s["normals"])
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    got = ops.decimate_mesh(dev, torch.empty((0, 3), device="cuda"), torch.empty((0, 3), dtype=torch.int32, device="cuda"), 0.25)
    torch.cuda.synchronize()
    assert got.count.tolist() == [0, 0] and got.face_count.tolist() == [0, 0] and got.faces_dropped.tolist() == [0, 0, 0]
    got = ops.decimate_mesh(dev, _t(s["xyz"]), torch.empty((0, 3), dtype=torch.int32, device="cuda"), 0.05)  # vertices without faces
    torch.cuda.synchronize()
    assert got.count.tolist() == [1766, 1766] and got.face_count.tolist() == [0, 0]


@pytest.mark.gpu
def test_decimate_refusals_leave_the_outputs_untouched(dev):
    from burn_depth_amd import ops
    s = _plane_scene()

    def refused(code, voxel=0.05, strip=()):
        out, stores = _fresh(len(s["xyz"]), 500, 500, True, False, False)
        for name in strip:
            setattr(out, name, None)
        with pytest.raises(_lib.MdError) as e:
            ops.decimate_mesh(dev, _t(s["xyz"]), _t(s["faces"]), voxel, conf=_t(s["conf"]), out=out)
        assert e.value.code == code
        torch.cuda.synchronize()
        for name, store in stores.items():
            assert (store == FILLS[name]).all(), name

    for bad in (float("nan"), float("inf"), -0.25, 0.0):
        refused(_lib.MD_ERR_INVALID_ARG, voxel=bad)
    refused(_lib.MD_ERR_INVALID_ARG, strip=("count",))
    refused(_lib.MD_ERR_INVALID_ARG, strip=("face_count",))
