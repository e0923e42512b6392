"""Connected components of a mesh and island removal: md_op_mesh_components and its host reference pipeline.mesh_components.
include/mi_depth.h states the contract, DESIGN 12.9 the kernels. Integers only: the label of a row is the smallest row of its
component and the size of a component a face count, so every comparison is bit for bit.

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402
from burn_depth_amd import pipeline as P  # noqa: E402
from points_util import _t, dev, lib  # noqa: E402,F401

f32 = np.float32
SENTINEL = 0x5A


def _loop_components(faces, N, min_faces=1, face_counts=None, compact=False, capacity=None, face_capacity=None):
    """The contract once more, face by face: a dictionary union-find whose root is always the smaller row -> (label,
    component_faces, faces, face_index, face_count, stats, index, remap)."""
    parent = list(range(N))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v

    tris = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    ok = [all(0 <= c < N for c in t) for t in tris]
    for t, good in zip(tris, ok):
        if good:
            for u, v in ((t[0], t[1]), (t[1], t[2])):
                u, v = find(u), find(v)
                if u != v:
                    parent[max(u, v)] = min(u, v)
    label = [find(i) for i in range(N)]
    size = {}
    for t, good in zip(tris, ok):
        if good:
            size[label[t[0]]] = size.get(label[t[0]], 0) + 1
    cf = [size.get(label[i], 0) for i in range(N)]
    cap = N if capacity is None else capacity
    survive = [i for i in range(N) if cf[i] >= min_faces]
    remap = [-1] * N
    for r, i in enumerate(survive):
        remap[i] = r
    kept, kept_index, stats = [], [], [0, 0, 0, len(size), sum(1 for s in size.values() if s >= min_faces)]
    for f, (t, good) in enumerate(zip(tris, ok)):
        if not good:
            stats[0] += 1
        elif size[label[t[0]]] < min_faces:
            stats[1] += 1
        elif compact and any(remap[c] >= cap for c in t):
            stats[2] += 1
        else:
            kept.append([remap[c] for c in t] if compact else t)
            kept_index.append(f)
    F = len(tris)
    b = np.minimum(np.concatenate([[0], np.cumsum([F] if face_counts is None else face_counts)]), F)
    ki = np.array(kept_index, np.int64)
    per_view = [int(((ki >= b[i]) & (ki < b[i + 1])).sum()) for i in range(len(b) - 1)]
    if face_capacity is not None:  # the counts stay the true ones; only the rows that fit are written
        kept, total, ki = kept[:face_capacity], len(ki), ki[:face_capacity]
        return (np.array(label, np.int32), np.array(cf, np.int32), np.array(kept, np.int32).reshape(-1, 3), ki.astype(np.int32),
                np.array(per_view + [total], np.int32), np.array(stats, np.int32), np.array(survive, np.int32), np.array(remap, np.int32))
    return (np.array(label, np.int32), np.array(cf, np.int32), np.array(kept, np.int32).reshape(-1, 3), ki.astype(np.int32),
            np.array(per_view + [len(ki)], np.int32), np.array(stats, np.int32), np.array(survive, np.int32), np.array(remap, np.int32))


def _check_against_loop(faces, N, min_faces=1, **kw):
    r = P.mesh_components(faces, N, min_faces, **kw)
    label, cf, kept, kept_index, face_count, stats, index, remap = _loop_components(faces, N, min_faces, **kw)
    assert np.array_equal(r.label, label) and np.array_equal(r.component_faces, cf)
    assert np.array_equal(r.faces, kept) and np.array_equal(r.face_index, kept_index)
    assert np.array_equal(r.face_count, face_count) and np.array_equal(r.stats, stats), (r.stats, stats)
    assert stats[:3].sum() + face_count[-1] == len(np.asarray(faces).reshape(-1, 3))
    assert all(a.dtype == np.int32 for a in (r.label, r.component_faces, r.faces, r.face_index, r.face_count, r.stats))
    if kw.get("compact"):
        assert np.array_equal(r.index, index) and np.array_equal(r.remap, remap)
    else:
        assert r.index is None and r.remap is None
    return r


def _islands(count=2000, seed=3, shuffle=True):
    """`count` disjoint strips of 1..8 faces with a row between them that no face names -> (faces, N)"""
    faces, n = [], 0
    for i in range(count):
        k = 1 + i % 8
        faces += [[n + f, n + f + 1, n + f + 2] for f in range(k)]
        n += k + 3
    faces = np.array(faces, np.int32)
    if shuffle:
        faces = faces[np.random.default_rng(seed).permutation(len(faces))]
    return faces, n


def _strip(F):
    a = np.arange(F, dtype=np.int32)
    return np.stack([a, a + 1, a + 2], 1), F + 2


def _random_faces(F, seed=5):
    """sparse enough to leave many components of several sizes"""
    rng = np.random.default_rng(seed)
    N = max(2 * F, 4)
    a = rng.integers(0, N, F)
    return np.stack([a, np.minimum(a + 1 + rng.integers(0, 3, F), N - 1), rng.integers(0, N, F)], 1).astype(np.int32), N


_SCENE = {}


def _plane_scene():
    """A real depth-grid mesh: pipeline.mesh_grid on a tilted plane of 2 views x 40 x 48 with a depth step down the middle, a
    speckled mask (seed 11, 22 % of the pixels off) and max_rtol 0.02, which cuts the step. The speckle leaves many small islands
    beside the two sheets of every view. Built once; the arrays are read-only."""
    if _SCENE:
        return _SCENE
    rng = np.random.default_rng(11)
    B, H, W = 2, 40, 48
    v, u = np.mgrid[0:H, 0:W].astype(f32)
    depth = np.stack([(2.0 + 0.004 * u + 0.003 * v + (u >= W // 2) * 0.8 + 0.1 * b).astype(f32) for b in range(B)])
    mask = rng.random((B, H, W)) >= 0.22
    mask[:, :, W // 2 - 1] &= rng.random((B, H)) >= 0.5
    pix = P.pixel_index(mask.astype(np.uint8))
    faces, face_count = P.mesh_grid(depth, pix, 1, 0.02)
    N = int(mask.sum())
    xyz = np.zeros((N, 3), f32)
    b, vv, uu = np.nonzero(mask)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = (uu - W / 2) * depth[b, vv, uu] / 50, (vv - H / 2) * depth[b, vv, uu] / 50, depth[b, vv, uu]
    _SCENE.update(faces=faces, face_counts=face_count[:-1].copy(), N=N, xyz=xyz, conf=rng.random(N).astype(f32),
                  rgb=rng.integers(0, 256, (N, 3)).astype(np.uint8), normals=rng.normal(size=(N, 3)).astype(f32), min_faces=6)
    for a in _SCENE.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return _SCENE


# ---- CPU: the reference against the per-face loop, clause by clause ------------------------------------------------------------

def test_a_single_triangle_is_one_component():
    r = _check_against_loop([[2, 0, 1]], 4)
    assert r.label.tolist() == [0, 0, 0, 3] and r.component_faces.tolist() == [1, 1, 1, 0]
    assert r.faces.tolist() == [[2, 0, 1]] and r.face_count.tolist() == [1, 1] and r.stats.tolist() == [0, 0, 0, 1, 1]


def test_two_triangles_that_share_one_vertex_only_are_one_component():
    r = _check_against_loop([[5, 6, 2], [2, 3, 4]], 7)
    assert r.label.tolist() == [0, 1, 2, 2, 2, 2, 2] and r.component_faces.tolist() == [0, 0, 2, 2, 2, 2, 2]
    assert r.stats.tolist() == [0, 0, 0, 1, 1]


def test_degenerate_faces_are_valid_and_join_what_they_name():
    r = _check_against_loop([[0, 1, 2], [4, 5, 6], [2, 2, 4], [8, 8, 8]], 9, min_faces=2)
    assert r.label.tolist() == [0, 0, 0, 3, 0, 0, 0, 7, 8] and r.component_faces[0] == 3 and r.component_faces[8] == 1
    assert r.face_index.tolist() == [0, 1, 2] and r.stats.tolist() == [0, 1, 0, 2, 1]


def test_corners_minus_one_and_n_are_invalid_and_join_nothing():
    faces = [[0, 1, 2], [2, 3, -1], [3, 4, 6], [4, 5, 5]]
    r = _check_against_loop(faces, 6)
    assert r.label.tolist() == [0, 0, 0, 3, 4, 4] and r.stats.tolist() == [2, 0, 0, 2, 2] and r.face_index.tolist() == [0, 3]
    assert r.component_faces.tolist() == [1, 1, 1, 0, 1, 1]


def test_rows_that_no_valid_face_names_are_their_own_component_with_no_face():
    r = _check_against_loop([[1, 3, 5]], 7)
    assert r.label.tolist() == [0, 1, 2, 1, 4, 1, 6] and r.component_faces.tolist() == [0, 1, 0, 1, 0, 1, 0]
    r = _check_against_loop(np.zeros((0, 3), np.int32), 3)
    assert r.label.tolist() == [0, 1, 2] and r.face_count.tolist() == [0, 0] and r.stats.tolist() == [0] * 5


def test_islands_of_one_to_eight_faces_at_min_faces_four():
    faces, N = _islands(64, shuffle=False)
    r = _check_against_loop(faces, N, min_faces=4)
    sizes = r.component_faces[faces[:, 0]]
    assert set(sizes.tolist()) == set(range(1, 9))
    assert np.array_equal(r.face_index, np.nonzero(sizes >= 4)[0]) and (sizes[r.face_index] >= 4).all()
    assert 4 in sizes[r.face_index] and 3 not in sizes[r.face_index]
    assert r.stats.tolist() == [0, int((sizes < 4).sum()), 0, 64, 40]


def test_a_shuffle_of_the_faces_changes_only_the_order_of_the_kept_faces():
    faces, N = _islands(200, shuffle=False)
    perm = np.random.default_rng(9).permutation(len(faces))
    a, b = _check_against_loop(faces, N, min_faces=5), _check_against_loop(faces[perm], N, min_faces=5)
    assert np.array_equal(a.label, b.label) and np.array_equal(a.component_faces, b.component_faces) and np.array_equal(a.stats, b.stats)
    assert sorted(perm[b.face_index].tolist()) == a.face_index.tolist()
    assert np.array_equal(b.faces, faces[perm][b.face_index])


def test_per_view_counts_follow_the_view_of_the_source_face():
    faces, N = _islands(100, seed=4)
    F = len(faces)
    r = _check_against_loop(faces, N, min_faces=3, face_counts=[100, 0, F - 150, 50])
    assert r.face_count[:-1].sum() == r.face_count[-1] == len(r.faces) and r.face_count[1] == 0
    r = _check_against_loop(faces, N, min_faces=3, face_counts=[F + 10, 5])  # counts beyond F are clamped
    assert r.face_count[1] == 0


def test_compact_with_remap_and_clipping_one_below_the_survivors():
    faces, N = _islands(100, seed=6)
    full = _check_against_loop(faces, N, min_faces=4, compact=True)
    M = len(full.index)
    assert 0 < M < N and (full.remap >= 0).sum() == M and full.stats[2] == 0
    assert np.array_equal(full.index[full.faces], faces[full.face_index])  # the faces go through remap, corners and winding unchanged
    assert set(np.unique(full.faces).tolist()) == set(range(M))            # no floater vertex: every survivor is named
    cut = _check_against_loop(faces, N, min_faces=4, compact=True, capacity=M - 1)
    assert cut.stats[2] >= 1 and cut.faces.max() < M - 1 and len(cut.faces) + cut.stats[2] == len(full.faces)
    assert np.array_equal(cut.index, full.index) and np.array_equal(cut.remap, full.remap)  # survival does not depend on clipping
    xyz = np.random.default_rng(1).normal(size=(N, 3)).astype(f32)
    r = P.mesh_components(faces, N, 4, compact=True, xyz=xyz)
    assert np.array_equal(r.xyz, xyz[full.index])


def test_face_capacity_below_the_total_cuts_the_rows_and_keeps_the_true_counts():
    faces, N = _islands(100, seed=6)
    full = _check_against_loop(faces, N, min_faces=4, face_counts=[200, len(faces) - 200])
    K = len(full.faces)
    for fcap in (K - 1, K // 2, 1, 0, K + 5):
        cut = _check_against_loop(faces, N, min_faces=4, face_counts=[200, len(faces) - 200], face_capacity=fcap)
        assert len(cut.faces) == len(cut.face_index) == min(fcap, K) and np.array_equal(cut.face_count, full.face_count)
        assert np.array_equal(cut.faces, full.faces[:fcap]) and np.array_equal(cut.stats, full.stats)
    cut = _check_against_loop(faces, N, min_faces=4, compact=True, face_capacity=7)
    assert len(cut.faces) == 7 and cut.face_count[-1] == K
    with pytest.raises(ValueError):
        P.mesh_components(faces, N, 4, face_capacity=-1)


def test_the_depth_grid_scene_has_islands_on_both_sides_of_min_faces():
    s = _plane_scene()
    r = _check_against_loop(s["faces"], s["N"], s["min_faces"], face_counts=s["face_counts"])
    assert r.stats[3] >= 3 and r.stats[4] >= 1 and r.stats[3] - r.stats[4] >= 1 and r.stats[1] >= 1
    assert r.face_count[0] > 0 and r.face_count[1] > 0 and r.face_count[:-1].sum() == r.face_count[-1]
    c = _check_against_loop(s["faces"], s["N"], s["min_faces"], compact=True)
    assert 0 < len(c.index) < s["N"]


def test_the_reference_refuses_what_the_contract_refuses():
    for bad in (dict(min_faces=0), dict(min_faces=-1), dict(compact=True, capacity=-1)):
        with pytest.raises(ValueError):
            P.mesh_components([[0, 1, 2]], 3, **{"min_faces": 1, **bad})


# ---- GPU: the operator against the reference, bit for bit -----------------------------------------------------------------------

def _run(dev, faces, N, min_faces, compact=False, capacity=None, face_capacity=None, xyz=None, conf=None, rgb=None, normals=None):
    """ops.mesh_components into outputs preset to a sentinel byte -> numpy dict (None fields left out)"""
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import PointCloud
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = len(faces)
    cap = N if capacity is None else capacity
    fcap = F if face_capacity is None else face_capacity
    z = _sentinel
    out = PointCloud(label=z((N,), torch.int32), component_faces=z((N,), torch.int32), faces=z((fcap, 3), torch.int32),
                     face_index=z((fcap,), torch.int32), face_count=z((2,), torch.int32), component_stats=z((5,), torch.int32))
    if compact:
        out.xyz, out.count, out.index, out.remap = z((cap, 3), torch.float32), z((2,), torch.int32), z((cap,), torch.int32), z((N,), torch.int32)
        out.conf = z((cap,), torch.float32) if conf is not None else None
        out.rgb = z((cap, 3), torch.uint8) if rgb is not None else None
        out.normals = z((cap, 3), torch.float32) if normals is not None else None
    ops.mesh_components(dev, _t(faces), N, min_faces, xyz=_t(xyz) if compact else None, conf=_t(conf), rgb=_t(rgb), normals=_t(normals),
                        compact=compact, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(out).items() if isinstance(v, torch.Tensor)}


def _sentinel(shape, dt):
    n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda").view(dt).reshape(shape)


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all()


def _assert_same(got, ref, what=""):
    """every output of the operator is the reference's, and the rows behind the written ones still hold the sentinel"""
    assert np.array_equal(got["label"], ref.label), what
    assert np.array_equal(got["component_faces"], ref.component_faces), what
    assert np.array_equal(got["component_stats"], ref.stats), (what, got["component_stats"], ref.stats)
    assert np.array_equal(got["face_count"], ref.face_count), (what, got["face_count"], ref.face_count)
    k = min(len(ref.faces), len(got["faces"]))
    assert np.array_equal(got["faces"][:k], ref.faces[:k]) and np.array_equal(got["face_index"][:k], ref.face_index[:k]), what
    assert _untouched(got["faces"][k:]) and _untouched(got["face_index"][k:]), what
    if ref.index is None:
        assert "remap" not in got and "index" not in got and "xyz" not in got
        return
    M = len(ref.index)
    m = min(M, len(got["index"]))
    assert got["count"].tolist() == [M, M] and np.array_equal(got["remap"], ref.remap), what
    assert np.array_equal(got["index"][:m], ref.index[:m]) and _untouched(got["index"][m:]), what
    for key in ("xyz", "conf", "rgb", "normals"):
        want = getattr(ref, key)
        assert (key in got) == (want is not None), (what, key)
        if want is not None:
            assert np.array_equal(got[key][:m].view(np.uint8), want[:m].view(np.uint8)) and _untouched(got[key][m:]), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [1, 63, 64, 65, 4095, 4096, 4097])
def test_wave_and_workgroup_edges_are_bit_identical_to_the_host_reference(dev, nf):
    faces, N = _random_faces(nf)
    ref = P.mesh_components(faces, N, 2)
    if nf >= 63:
        assert ref.stats[1] > 0 and ref.stats[4] > 0
    _assert_same(_run(dev, faces, N, 2), ref, nf)
    xyz = np.random.default_rng(nf).normal(size=(N, 3)).astype(f32)
    _assert_same(_run(dev, faces, N, 2, compact=True, xyz=xyz), P.mesh_components(faces, N, 2, compact=True, xyz=xyz), (nf, "compact"))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_strip_of_five_thousand_triangles_is_one_component_in_any_order(dev, order):
    faces, N = _strip(5000)
    faces = {"ascending": faces, "descending": faces[::-1], "shuffled": faces[np.random.default_rng(2).permutation(5000)]}[order]
    got = _run(dev, faces, N, 5000)
    _assert_same(got, P.mesh_components(faces, N, 5000), order)
    assert (got["label"] == 0).all() and (got["component_faces"] == 5000).all() and got["component_stats"].tolist() == [0, 0, 0, 1, 1]
    assert _run(dev, faces, N, 5001)["face_count"].tolist() == [0, 0]


@pytest.mark.gpu
def test_a_fan_of_ten_thousand_faces_around_one_vertex(dev):
    a = np.arange(10000, dtype=np.int32)
    faces = np.stack([np.zeros_like(a), a + 1, a + 2], 1)[np.random.default_rng(3).permutation(10000)]
    got = _run(dev, faces, 10002, 1)
    _assert_same(got, P.mesh_components(faces, 10002, 1))
    assert (got["label"] == 0).all() and (got["component_faces"] == 10000).all() and got["face_count"].tolist() == [10000, 10000]


@pytest.mark.gpu
@pytest.mark.parametrize("min_faces", [1, 4, 9])
def test_two_thousand_shuffled_islands(dev, min_faces):
    faces, N = _islands()
    ref = P.mesh_components(faces, N, min_faces)
    got = _run(dev, faces, N, min_faces)
    _assert_same(got, ref, min_faces)
    assert got["component_stats"][3] == 2000
    if min_faces == 9:
        assert got["face_count"].tolist() == [0, 0] and got["component_stats"][4] == 0 and _untouched(got["faces"])
    xyz = np.random.default_rng(7).normal(size=(N, 3)).astype(f32)
    _assert_same(_run(dev, faces, N, min_faces, compact=True, xyz=xyz), P.mesh_components(faces, N, min_faces, compact=True, xyz=xyz))


@pytest.mark.gpu
@pytest.mark.parametrize("compact,carried", [(False, False), (True, False), (True, True)])
def test_depth_grid_scene_with_and_without_compact_and_the_carried_rows(dev, compact, carried):
    s = _plane_scene()
    rows = dict(xyz=s["xyz"]) if compact else {}
    if carried:
        rows.update(conf=s["conf"], rgb=s["rgb"], normals=s["normals"])
    ref = P.mesh_components(s["faces"], s["N"], s["min_faces"], compact=compact, **rows)
    assert ref.stats[3] >= 3 and ref.stats[1] >= 1 and ref.stats[4] >= 1
    _assert_same(_run(dev, s["faces"], s["N"], s["min_faces"], compact=compact, **rows), ref, (compact, carried))


@pytest.mark.gpu
def test_capacities_below_the_outputs_keep_the_true_counts_and_clip(dev):
    s = _plane_scene()
    full = P.mesh_components(s["faces"], s["N"], s["min_faces"], compact=True, xyz=s["xyz"], rgb=s["rgb"])
    M, K = len(full.index), len(full.faces)
    for fcap in (K // 2, 1, 0, K - 1):
        got = _run(dev, s["faces"], s["N"], s["min_faces"], face_capacity=fcap)
        _assert_same(got, P.mesh_components(s["faces"], s["N"], s["min_faces"]), fcap)
        assert got["face_count"][-1] == K and len(got["faces"]) == fcap
    for cap in (M - 1, M // 2, 1, 0):
        ref = P.mesh_components(s["faces"], s["N"], s["min_faces"], compact=True, capacity=cap, xyz=s["xyz"], rgb=s["rgb"])
        assert ref.stats[2] >= 1 and len(ref.faces) + ref.stats[2] == K
        got = _run(dev, s["faces"], s["N"], s["min_faces"], compact=True, capacity=cap, face_capacity=K // 3, xyz=s["xyz"], rgb=s["rgb"])
        _assert_same(got, ref, cap)
        n = min(int(got["face_count"][-1]), K // 3)
        assert n == 0 or got["faces"][:n].max() < cap  # no written face names an unwritten row


@pytest.mark.gpu
def test_invalid_corners_join_nothing_and_are_counted(dev):
    faces, N = _random_faces(3000, seed=8)
    faces = faces.copy()
    faces[::7, 0], faces[3::11, 2], faces[5::13, 1] = -1, N, np.iinfo(np.int32).max
    faces[1::17] = np.iinfo(np.int32).min
    ref = P.mesh_components(faces, N, 3)
    assert ref.stats[0] > 600 and ref.stats[4] > 0
    _assert_same(_run(dev, faces, N, 3), ref)
    xyz = np.zeros((N, 3), f32)
    _assert_same(_run(dev, faces, N, 3, compact=True, xyz=xyz), P.mesh_components(faces, N, 3, compact=True, xyz=xyz))


@pytest.mark.gpu
def test_no_faces_and_no_rows(dev):
    none = np.zeros((0, 3), np.int32)
    got = _run(dev, none, 5, 1)
    _assert_same(got, P.mesh_components(none, 5, 1))
    assert got["label"].tolist() == [0, 1, 2, 3, 4] and got["face_count"].tolist() == [0, 0] and got["component_stats"].tolist() == [0] * 5
    _assert_same(_run(dev, none, 5, 1, compact=True, xyz=np.zeros((5, 3), f32)), P.mesh_components(none, 5, 1, compact=True, xyz=np.zeros((5, 3), f32)))
    got = _run(dev, [[0, 1, 2]], 0, 1)  # no rows: every face is invalid
    assert got["component_stats"].tolist() == [1, 0, 0, 0, 0] and got["face_count"].tolist() == [0, 0]


@pytest.mark.gpu
def test_two_runs_of_one_call_give_equal_bits(dev):
    faces, N = _islands(seed=12)
    xyz = np.random.default_rng(4).normal(size=(N, 3)).astype(f32)
    a, b = (_run(dev, faces, N, 4, compact=True, xyz=xyz) for _ in range(2))
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.gpu
def test_the_operator_refuses_before_any_launch(dev, lib):
    from burn_depth_amd import ops
    faces = _t(np.array([[0, 1, 2]], np.int32))
    for kw in (dict(min_faces=0), dict(min_faces=-3)):
        with pytest.raises(_lib.MdError) as e:
            ops.mesh_components(dev, faces, 3, **kw)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
    out = ops.mesh_components(dev, faces, 3, 1)
    for k, v in dict(remap=_sentinel((3,), torch.int32), index=_sentinel((3,), torch.int32), count=_sentinel((2,), torch.int32)).items():
        setattr(out, k, v)
        with pytest.raises(_lib.MdError) as e:  # a vertex-side output without compact
            ops.mesh_components(dev, faces, 3, 1, out=out)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG and _untouched(v.cpu().numpy())
        setattr(out, k, None)
    out.face_count = None
    with pytest.raises(_lib.MdError) as e:  # faces without face_count
        ops.mesh_components(dev, faces, 3, 1, out=out)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
