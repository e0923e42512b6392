"""DBSCAN / Euclidean clustering of a point list: md_op_cluster_points and its host reference pipeline.cluster_points.
include/mi_depth.h states the contract, DESIGN 12.12 the kernels. Every output is integers on a deterministic f32 predicate or a
selection among the input coordinates, so every comparison is bit for bit.

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
NEW_ENTRIES = ("md_op_cluster_points", "md_infer_points_clusters")
FIELDS = ["radius", "min_neighbours", "min_points", "max_points", "mode", "label", "cluster_size", "cluster", "table_label", "table_size", "box",
          "table_capacity", "stats", "index", "dropped"]
ROW_KEYS = ("label", "cluster_size", "cluster")


def _okey(v):
    b = int(np.asarray(v, f32).view(np.uint32))
    return (~b) & 0xFFFFFFFF if b & 0x80000000 else b ^ 0x80000000


def _brute(xyz, radius, k, min_points=1, max_points=0):
    """The contract applied literally, pair by pair in numpy scalars -> (label, cluster_size, cluster, table_label, table_size,
    box, stats, dropped): cells, predicate, core counts, components by repeated relabelling, the border rule."""
    pts = [tuple(f32(a) for a in p) for p in np.asarray(xyz, f32).reshape(-1, 3)]
    N, r = len(pts), f32(radius)
    r2, half = r * r, f32(1 << 20)
    with np.errstate(all="ignore"):
        cells = [tuple(np.floor(a / r) for a in p) for p in pts]
        ok = [all(np.isfinite(a) for a in p) and all(-half <= c < half for c in cs) for p, cs in zip(pts, cells)]
        nb = [[] for _ in range(N)]
        for i in range(N):
            for j in range(N):
                if i == j or not ok[i] or not ok[j] or any(abs(int(a) - int(b)) > 1 for a, b in zip(cells[i], cells[j])):
                    continue
                dx, dy, dz = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1], pts[j][2] - pts[i][2]
                if (dx * dx + dy * dy) + dz * dz <= r2:
                    nb[i].append(j)
    core = [ok[i] and len(nb[i]) >= k for i in range(N)]
    label = [i if core[i] else (-1 if ok[i] else -2) for i in range(N)]
    changed = True
    while changed:  # repeated relabelling: every core row takes the smallest label among its core neighbours
        changed = False
        for i in range(N):
            for j in nb[i]:
                if core[i] and core[j] and label[j] < label[i]:
                    label[i], changed = label[j], True
    for i in range(N):
        if ok[i] and not core[i]:
            near = [label[j] for j in nb[i] if core[j]]
            label[i] = min(near) if near else -1
    size = {l: label.count(l) for l in set(label) if l >= 0}
    kept = sorted(l for l, s in size.items() if s >= min_points and (max_points == 0 or s <= max_points))
    ids = {l: n for n, l in enumerate(kept)}
    cluster = [ids.get(l, -1) if l != -2 else -2 for l in label]
    box = np.zeros((len(kept), 6), f32)
    for n, l in enumerate(kept):
        rows = [i for i in range(N) if label[i] == l]
        for a in range(3):
            box[n, a] = min((pts[i][a] for i in rows), key=_okey)
            box[n, 3 + a] = max((pts[i][a] for i in rows), key=_okey)
    stats = [len(size), len(kept), label.count(-1), sum(size[l] for l in kept)]
    return (np.array(label, np.int32), np.array([size.get(l, 0) for l in label], np.int32), np.array(cluster, np.int32), np.array(kept, np.int32),
            np.array([size[l] for l in kept], np.int32), box, np.array(stats, np.int32), ok.count(False))


def _same_as_brute(got, want, what=""):
    for g, w, name in zip((got.label, got.cluster_size, got.cluster, got.table_label, got.table_size), want, ROW_KEYS + ("table_label", "table_size")):
        assert np.array_equal(g, w), (what, name, g, w)
    assert np.array_equal(_bits(got.box), _bits(want[5])), (what, got.box, want[5])
    assert got.stats.tolist() == want[6].tolist() and got.dropped == want[7], (what, got.stats, want[6])


def _blobs(n, seed, spread=4.0, centres=6):
    """n points around a few centres plus uniform speckle, with three rows that are out of the contract's range"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (centres, 3))
    x = np.concatenate([c[rng.integers(0, centres, n - n // 5)] + rng.normal(0, 0.25, (n - n // 5, 3)), rng.uniform(-spread, spread, (n // 5, 3))])
    x = x[rng.permutation(n)].astype(f32)
    if n > 20:
        x[[3, n // 2, n - 2]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 3e30]]
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_cluster_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    body = header[header.index("typedef struct md_points_clusters {"):header.index("} md_points_clusters;")]
    assert re.findall(r"^\s+[a-z0-9_]+\*? (?:\*)?([a-z_]+);", body, re.M) == FIELDS
    assert [n for n, _ in _lib.MdPointsClusters._fields_] == FIELDS
    # the model entry takes the plane entry's arguments with the cluster part in front of out_kind
    planes, clusters = _lib.SYMBOLS["md_infer_points_planes"][1], _lib.SYMBOLS["md_infer_points_clusters"][1]
    assert clusters[:-2] == planes[:-2] + [C.POINTER(_lib.MdPointsClusters)] and clusters[-2:] == planes[-2:]


@pytest.mark.parametrize("k", (0, 1, 3, 8))
@pytest.mark.parametrize("radius", (0.2, 0.45, 1.1))
def test_reference_against_brute_force(radius, k):
    for n, seed in ((60, 0), (400, 1)):
        xyz = _blobs(n, seed)
        for lim in (dict(), dict(min_points=3, max_points=40)):
            _same_as_brute(P.cluster_points(xyz, radius, k, **lim), _brute(xyz, radius, k, **lim), (n, radius, k, lim))


def test_inclusive_radius_and_one_ulp_beyond():
    r = f32(0.5)
    a = np.array([[0.25, 0.25, 0.25], [0.25 + 0.5, 0.25, 0.25]], f32)  # dx = 0.5 exactly: d2 == r2
    assert f32(a[1, 0] - a[0, 0]) == r
    assert P.cluster_points(a, r).label.tolist() == [0, 0]
    b = a.copy()
    b[1, 0] = np.nextafter(b[1, 0], f32(2))  # one ulp beyond
    assert f32(b[1, 0] - b[0, 0]) > r
    assert P.cluster_points(b, r).label.tolist() == [0, 1]
    _same_as_brute(P.cluster_points(b, r), _brute(b, r, 0))


def test_pair_two_cells_apart_is_no_edge():
    """the example of the outlier removal's contract: -1e-30 lies in cell -1, `radius` in cell 1, and dx rounds to the radius"""
    r = f32(0.5)
    a = np.array([[-1e-30, 0.1, 0.1], [0.5, 0.1, 0.1]], f32)
    assert f32(a[1, 0] - a[0, 0]) == r and np.floor(a[0, 0] / r) == -1 and np.floor(a[1, 0] / r) == 1
    got = P.cluster_points(a, r)
    assert got.label.tolist() == [0, 1] and got.stats.tolist() == [2, 2, 0, 2]
    assert P.cluster_points(a, r, 1).label.tolist() == [-1, -1]


def test_duplicates_are_neighbours_of_each_other():
    a = np.tile(np.array([[1.5, -2.0, 0.25]], f32), (5, 1))
    got = P.cluster_points(a, 0.1, 4)
    assert got.label.tolist() == [0] * 5 and got.cluster_size.tolist() == [5] * 5 and got.stats.tolist() == [1, 1, 0, 5]
    assert P.cluster_points(a, 0.1, 5).label.tolist() == [-1] * 5


def _two_clusters_and_a_border():
    """rows 1..4 around x = 0 and rows 5..8 around x = 2 are core at k = 3; row 0 at x = 1 sees one row of either and is border"""
    left = [[0.0, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1], [0.1, 0.0, 0.0]]
    right = [[2.0, 0.0, 0.0], [2.0, 0.1, 0.0], [2.0, 0.0, 0.1], [1.9, 0.0, 0.0]]
    return np.array([[1.0, 0.0, 0.0]] + left + right, f32)


def test_border_row_takes_the_smaller_label_and_merges_nothing():
    a = _two_clusters_and_a_border()
    got = P.cluster_points(a, 0.95, 3)
    assert got.label.tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5] and got.cluster_size.tolist() == [5] * 5 + [4] * 4
    assert got.table_label.tolist() == [1, 5] and got.stats.tolist() == [2, 2, 0, 9]
    _same_as_brute(got, _brute(a, 0.95, 3))
    swapped = a[[0, 5, 6, 7, 8, 1, 2, 3, 4]]  # the right cluster first: the border row still takes the smaller label
    assert P.cluster_points(swapped, 0.95, 3).label.tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5]
    assert P.cluster_points(a, 0.95, 0).label.tolist() == [0] * 9  # k = 0: the border row is core and joins them


def test_non_core_row_with_only_non_core_neighbours_is_noise():
    a = np.array([[0, 0, 0], [0.3, 0, 0], [5, 5, 5]], f32)
    got = P.cluster_points(a, 0.5, 2)
    assert got.label.tolist() == [-1, -1, -1] and got.cluster.tolist() == [-1, -1, -1] and got.stats.tolist() == [0, 0, 3, 0]
    assert got.cluster_size.tolist() == [0, 0, 0] and got.box.shape == (0, 6)


def test_size_filter_at_the_boundary_sizes():
    a = np.concatenate([np.tile([[0.0, 0, 0]], (3, 1)), np.tile([[5.0, 0, 0]], (4, 1)), np.tile([[9.0, 0, 0]], (5, 1))]).astype(f32)
    for lo, hi, want in ((1, 0, [0, 3, 7]), (4, 0, [3, 7]), (5, 0, [7]), (6, 0, []), (3, 3, [0]), (3, 4, [0, 3]), (4, 4, [3]), (1, 2, [])):
        got = P.cluster_points(a, 0.5, 0, lo, hi)
        assert got.table_label.tolist() == want and got.stats[0] == 3 and got.stats[1] == len(want), (lo, hi)
        assert got.label.tolist() == [0] * 3 + [3] * 4 + [7] * 5  # the label is the one before the filter
        assert sorted(set(got.cluster.tolist()) - {-1}) == list(range(len(want)))


def test_dense_ids_follow_ascending_label_after_a_shuffle():
    xyz = _blobs(300, 5)
    perm = np.random.default_rng(9).permutation(300)
    for x in (xyz, xyz[perm]):
        got = P.cluster_points(x, 0.45, 2, min_points=3)
        assert np.all(np.diff(got.table_label) > 0) and len(got.table_label) == got.stats[1] > 3
        for n, l in enumerate(got.table_label):
            assert set(got.cluster[got.label == l].tolist()) == {n} and got.label[l] == l
    a, b = P.cluster_points(xyz, 0.45, 2, min_points=3), P.cluster_points(xyz[perm], 0.45, 2, min_points=3)
    assert sorted(a.table_size.tolist()) == sorted(b.table_size.tolist()) and a.stats.tolist() == b.stats.tolist()


def test_boxes_order_minus_zero_below_plus_zero():
    a = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], f32)
    got = P.cluster_points(a, 4.0)
    assert got.table_label.tolist() == [0]
    assert _bits(got.box).tolist() == [_bits([[-0.0, -0.0, -1.0, 0.0, 0.0, 1.0]]).ravel().tolist()]
    _same_as_brute(got, _brute(a, 4.0, 0))


def test_stats_are_true_below_the_table_capacity():
    xyz = _blobs(300, 5)
    full = P.cluster_points(xyz, 0.45, 2, min_points=3)
    cut = P.cluster_points(xyz, 0.45, 2, min_points=3, table=2)
    assert cut.stats.tolist() == full.stats.tolist() and full.stats[1] > 2
    assert cut.table_label.tolist() == full.table_label[:2].tolist() and np.array_equal(_bits(cut.box), _bits(full.box[:2]))
    assert np.array_equal(cut.cluster, full.cluster)  # the ids of the rows do not depend on the table
    assert P.cluster_points(xyz, 0.45, 2, table=0).box.shape == (0, 6)


def test_mode_keep_and_per_view_counts():
    xyz = _blobs(300, 5)
    conf, rgb = np.arange(300, dtype=f32), (np.arange(900) % 251).astype(np.uint8).reshape(300, 3)
    got = P.cluster_points(xyz, 0.45, 2, min_points=3, mode=1, conf=conf, rgb=rgb, normals=xyz[::-1], counts=[100, 60, 140])
    index = np.nonzero(got.cluster >= 0)[0]
    assert np.array_equal(got.index, index) and got.count.tolist() == [(index < 100).sum(), ((index >= 100) & (index < 160)).sum(),
                                                                      (index >= 160).sum(), len(index)]
    assert len(index) == got.stats[3] and np.array_equal(_bits(got.xyz), _bits(xyz[index])) and np.array_equal(got.conf, conf[index])
    assert np.array_equal(got.rgb, rgb[index]) and np.array_equal(_bits(got.normals), _bits(xyz[::-1][index]))
    assert P.cluster_points(xyz, 0.45, 2).xyz is None


def test_reference_refusals():
    xyz = _blobs(30, 1)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(min_neighbours=-1), dict(min_neighbours=(1 << 20) + 1),
                dict(min_points=0), dict(max_points=-1), dict(min_points=5, max_points=4), dict(mode=2), dict(mode=-1), dict(table=-1)):
        with pytest.raises(ValueError):
            P.cluster_points(xyz, **dict(dict(radius=0.5), **bad))


def test_c_entries_refuse_before_touching_a_device(lib):
    """both entries with a null device / model: every refusal comes back as a code, nothing is dereferenced"""
    xyz = np.zeros((4, 3), f32)
    px = xyz.ctypes.data_as(C.c_void_p)
    outs = _lib.MdPointsOutputs()
    good = dict(radius=0.5, min_neighbours=0, min_points=1, max_points=0, mode=0, table_capacity=0)
    call = lambda clu, o=outs, n=4: lib.md_op_cluster_points(None, px, None, None, None, n, clu, C.byref(o), None, None)  # noqa: E731
    assert call(None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_cluster_points(None, px, None, None, None, 4, C.byref(_lib.MdPointsClusters(**good)), None, None, None) == _lib.MD_ERR_INVALID_ARG
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=float("nan")), dict(min_neighbours=-1),
                dict(min_neighbours=(1 << 20) + 1), dict(min_points=0), dict(max_points=-1), dict(min_points=5, max_points=4), dict(mode=2),
                dict(mode=-1), dict(table_capacity=-1), dict(index=px.value)):
        assert call(C.byref(_lib.MdPointsClusters(**dict(good, **bad)))) == _lib.MD_ERR_INVALID_ARG, bad
    clu = C.byref(_lib.MdPointsClusters(**good))
    assert call(clu, n=-1) == _lib.MD_ERR_INVALID_ARG and call(clu, n=1 << 30) == _lib.MD_ERR_SHAPE
    assert call(clu, _lib.MdPointsOutputs(capacity=-1)) == _lib.MD_ERR_INVALID_ARG
    assert call(clu, _lib.MdPointsOutputs(xyz=px.value, capacity=4)) == _lib.MD_ERR_INVALID_ARG  # a compacted output without count
    cnt = (C.c_int32 * 2)()
    with_list = _lib.MdPointsOutputs(xyz=px.value, count=C.cast(cnt, C.c_void_p).value, capacity=4)
    assert call(clu, with_list) == _lib.MD_ERR_INVALID_ARG  # ... or with mode 0
    keep = C.byref(_lib.MdPointsClusters(**dict(good, mode=1)))
    assert call(keep, _lib.MdPointsOutputs(rgb=px.value, count=C.cast(cnt, C.c_void_p).value, capacity=4)) == _lib.MD_ERR_INVALID_ARG  # no rgb row
    assert call(keep, with_list) == _lib.MD_ERR_INVALID_ARG  # everything is in order: the null device is the last refusal
    assert "device is null" in lib.md_last_error().decode()
    args = [None] * (len(_lib.SYMBOLS["md_infer_points_clusters"][1]) - 8)
    assert lib.md_infer_points_clusters(None, None, 1, 70, 70, _lib.MD_MEM_DEVICE, *args, _lib.MD_MEM_DEVICE, None) == _lib.MD_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the operator against pipeline.cluster_points
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(getattr(pc, k)) for k in ("xyz", "conf", "rgb", "normals", "index", "count")}
    d.update({k: g(getattr(pc.clusters, k)) for k in ROW_KEYS + ("table_label", "table_size", "box", "stats", "dropped")})
    return d


def _same_as_host(got, want, n, what=""):
    """got: _np of the operator's cloud; want: HostClusters of the same table capacity; n: the rows of the input"""
    for k in ROW_KEYS:
        assert np.array_equal(got[k][:n], getattr(want, k)), (what, k)
    assert got["stats"].tolist() == want.stats.tolist(), (what, got["stats"], want.stats)
    assert int(got["dropped"][0]) == want.dropped, what
    t = len(want.table_label)
    assert np.array_equal(got["table_label"][:t], want.table_label) and np.array_equal(got["table_size"][:t], want.table_size), what
    assert np.array_equal(got["box"][:t].view(np.uint32), _bits(want.box)), (what, got["box"][:t], want.box)
    if want.index is None:
        assert got["xyz"] is None and got["count"] is None
        return
    m = len(want.index)
    assert got["count"].tolist() == [m, m], what
    w = min(m, got["xyz"].shape[0])
    for k in ("xyz", "conf", "rgb", "normals", "index"):
        ref = getattr(want, k)
        assert (ref is None) == (got[k] is None), (what, k)
        if ref is not None:
            assert np.array_equal(got[k][:w].view(np.uint8), np.ascontiguousarray(ref[:w]).view(np.uint8)), (what, k)


def _check(dev, xyz, what="", **kw):
    from burn_depth_amd import ops
    got = _np(ops.cluster_points(dev, _t(xyz), **kw))
    want = P.cluster_points(xyz, **kw)
    _same_as_host(got, want, len(xyz), what)
    return got, want


@pytest.fixture(scope="module")
def seam_scene():
    """4097 rows of blobs and speckle with three rows out of range; computed once, never written"""
    xyz = _blobs(4097, 11, spread=5.0, centres=12)
    xyz.setflags(write=False)
    return xyz


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 4))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4095, 4096, 4097))
def test_operator_matches_the_reference_at_the_wave_and_tile_seams(dev, seam_scene, n, k):
    got, want = _check(dev, seam_scene[:n], (n, k), radius=0.3, min_neighbours=k, min_points=2 if n > 1 else 1, max_points=900)
    if n >= 4095:
        assert want.stats[1] > 10 and want.dropped >= 2 and (k > 0 or want.stats[0] > want.stats[1])  # clusters; at k = 0 some filtered out


CUBE = dict(radius=0.5, min_neighbours=30, min_points=10)


@pytest.fixture(scope="module")
def cube_scene():
    """5 000 points in the 8^3 cells of side 0.5 of [0, 4)^3: blobs on a checkerboard of 32 centres and 300 rows of speckle, in a
    seeded order. At the radius of the cells a speckle row close to a blob is core, one further out border or noise, and the seed
    is one where two blobs are bridged by such rows"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3), -1).reshape(-1, 3)
    c = g[g.sum(1) % 2 == 0] + 0.5
    x = np.concatenate([c[rng.integers(0, 32, 4700)] + rng.normal(0, 0.04, (4700, 3)), rng.uniform(0, 4, (300, 3))])
    x = np.clip(x, 0, np.nextafter(f32(4), f32(0)))[rng.permutation(5000)].astype(f32)
    x.setflags(write=False)
    return x


def test_cube_scene_has_the_clusters_its_gpu_test_needs(cube_scene):
    want = P.cluster_points(cube_scene, **CUBE)
    assert 20 <= want.stats[1] <= 200 and want.stats[2] > 100 and want.stats[1] == 31, want.stats
    cells = np.floor(cube_scene / f32(CUBE["radius"]))
    assert cells.max() == 7 and cells.min() == 0 and len(np.unique(cells, axis=0)) > 200  # 8^3 cells at the radius of the call


@pytest.mark.gpu
def test_many_clusters_with_noise(dev, cube_scene):
    from burn_depth_amd import ops
    got, want = _check(dev, cube_scene, "dbscan", **CUBE)
    assert 20 <= want.stats[1] <= 200 and want.stats[2] > 100
    _check(dev, cube_scene, "euclidean", radius=0.5 / 4, min_points=10)  # a quarter of the radius, k = 0: 32^3 cells, many small clusters
    again = _np(ops.cluster_points(dev, _t(cube_scene), **CUBE))
    kept = int(want.stats[1])
    for k in got:  # two runs of one call give equal bits; the table rows behind the kept clusters are not written, so not compared
        rows = kept if k in ("table_label", "table_size", "box") else None
        assert (got[k] is None and again[k] is None) or np.array_equal(got[k][:rows].view(np.uint8), again[k][:rows].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_one_chain_sees_the_deepest_trees(dev, order):
    x = np.zeros((5000, 3), f32)
    x[:, 0] = (np.arange(5000) * 0.9 * 0.01).astype(f32)
    x = {"ascending": x, "descending": x[::-1].copy(), "shuffled": x[np.random.default_rng(1).permutation(5000)]}[order]
    for k in (0, 2):
        got, want = _check(dev, x, (order, k), radius=0.01, min_neighbours=k)
        ends = {int(x[:, 0].argmin()), int(x[:, 0].argmax())}  # one neighbour each: border rows at k = 2, so not the label
        first = min(set(range(5000)) - ends) if k else 0
        assert want.stats.tolist() == [1, 1, 0, 5000] and got["table_size"][0] == 5000 and set(want.label.tolist()) == {first}
    got, want = _check(dev, x, (order, 3), radius=0.01, min_neighbours=3)  # no row of a chain has three neighbours
    assert want.stats.tolist() == [0, 0, 5000, 0]


@pytest.mark.gpu
def test_coincident_points_are_one_bucket_and_one_cluster(dev):
    x = np.tile(np.array([[0.3, -7.25, 2.0]], f32), (4097, 1))
    for k in (0, 4096):
        got, want = _check(dev, x, k, radius=0.05, min_neighbours=k)
        assert want.stats.tolist() == [1, 1, 0, 4097] and got["box"][0].tolist() == [x[0, 0], x[0, 1], x[0, 2]] * 2


@pytest.mark.gpu
def test_lone_points_and_the_table_clip(dev):
    from burn_depth_amd import ops
    g = np.arange(9, dtype=f32) * 10
    x = np.stack(np.meshgrid(g, g, g), -1).reshape(-1, 3)[np.random.default_rng(2).permutation(729)].astype(f32)
    got, want = _check(dev, x, "k0", radius=1.0, min_neighbours=0)
    assert want.stats.tolist() == [729, 729, 0, 729] and want.table_label.tolist() == list(range(729))
    assert _check(dev, x, "k1", radius=1.0, min_neighbours=1)[1].stats.tolist() == [0, 0, 729, 0]
    pc = ops.cluster_points(dev, _t(x), radius=1.0)
    for t in (pc.clusters.table_label, pc.clusters.table_size, pc.clusters.box):
        t.fill_(-7)
    torch.cuda.synchronize()
    got = _np(ops.cluster_points(dev, _t(x), radius=1.0, table=100, out=pc))  # ids >= 100 are not written
    _same_as_host(got, P.cluster_points(x, 1.0, table=100), 729, "clip")
    assert got["stats"].tolist() == [729, 729, 0, 729]
    assert (got["table_label"][100:] == -7).all() and (got["table_size"][100:] == -7).all() and (got["box"][100:] == -7).all()


@pytest.mark.gpu
def test_bridge_of_non_core_points(dev):
    rng = np.random.default_rng(4)
    blob = lambda c: (np.array(c) + rng.normal(0, 0.05, (200, 3))).astype(f32)  # noqa: E731
    bridge = np.stack([np.linspace(0.1, 1.9, 19), np.zeros(19), np.zeros(19)], 1).astype(f32)  # 0.1 apart: two neighbours each
    x = np.concatenate([bridge, blob([0, 0, 0]), blob([2, 0, 0])])[rng.permutation(419)]
    got, want = _check(dev, x, "k8", radius=0.15, min_neighbours=8)
    assert want.stats[1] == 2 and want.stats[2] > 0
    got, want = _check(dev, x, "k0", radius=0.15, min_neighbours=0, min_points=100)
    assert want.stats[1] == 1 and want.table_size[0] >= 419 - 10


@pytest.mark.gpu
def test_border_rule_on_the_device(dev):
    a = _two_clusters_and_a_border()
    got, want = _check(dev, a, "border", radius=0.95, min_neighbours=3)
    assert got["label"].tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 5]
    _check(dev, a[[0, 5, 6, 7, 8, 1, 2, 3, 4]], "border swapped", radius=0.95, min_neighbours=3)
    z = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], f32)
    _check(dev, z, "zeros", radius=4.0)


@pytest.mark.gpu
def test_mode_keep_carried_rows_and_capacity(dev, seam_scene):
    from burn_depth_amd import ops
    xyz = seam_scene
    n = len(xyz)
    rng = np.random.default_rng(6)
    conf, rgb, nrm = rng.random(n).astype(f32), rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.normal(size=(n, 3)).astype(f32)
    kw = dict(radius=0.3, min_neighbours=4, min_points=20, mode=1)
    want = P.cluster_points(xyz, conf=conf, rgb=rgb, normals=nrm, **kw)
    m = len(want.index)
    assert 500 < m < n - 500
    _same_as_host(_np(ops.cluster_points(dev, _t(xyz), conf=_t(conf), rgb=_t(rgb), normals=_t(nrm), **kw)), want, n, "all rows")
    _same_as_host(_np(ops.cluster_points(dev, _t(xyz), **kw)), P.cluster_points(xyz, **kw), n, "xyz only")
    _same_as_host(_np(ops.cluster_points(dev, _t(xyz), conf=_t(conf), **dict(kw, mode="keep"))), P.cluster_points(xyz, conf=conf, **kw), n, "by name")
    cap = m - 77
    short = ops.cluster_points(dev, _t(xyz), conf=_t(conf), normals=_t(nrm), capacity=cap + 9, **kw)
    for t in (short.xyz, short.conf, short.normals):
        t.fill_(POISON)
    short.index.fill_(-5)
    short.xyz, short.conf, short.normals, short.index = short.xyz[:cap + 5], short.conf[:cap + 3], short.normals[:cap + 5], short.index[:cap]
    keep = [t.clone() for t in (short.xyz, short.conf, short.normals)]
    got = _np(ops.cluster_points(dev, _t(xyz), conf=_t(conf), normals=_t(nrm), out=short, **kw))  # capacity = the shortest: cap < M
    assert got["count"].tolist() == [m, m]
    for k, ref in (("xyz", want.xyz), ("conf", want.conf), ("normals", want.normals), ("index", want.index)):
        assert np.array_equal(got[k][:cap].view(np.uint8), np.ascontiguousarray(ref[:cap]).view(np.uint8)), k
    for k, t in zip(("xyz", "conf", "normals"), keep):
        assert (got[k][cap:] == POISON).all() and (t[cap:].cpu().numpy() == POISON).all(), k  # the sentinels behind the capacity


@pytest.mark.gpu
def test_operator_refusals_and_the_empty_list(dev):
    from burn_depth_amd import ops
    x = _t(_blobs(64, 1))
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(min_neighbours=-1), dict(min_neighbours=(1 << 20) + 1),
                dict(min_points=0), dict(max_points=-1), dict(min_points=5, max_points=4), dict(mode=2), dict(table=-1)):
        with pytest.raises(_lib.MdError) as e:
            ops.cluster_points(dev, x, **dict(dict(radius=0.5), **bad))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
    got = _np(ops.cluster_points(dev, torch.zeros((0, 3), device="cuda"), radius=0.5, mode=1))
    assert got["stats"].tolist() == [0, 0, 0, 0] and got["count"].tolist() == [0, 0] and int(got["dropped"][0]) == 0
