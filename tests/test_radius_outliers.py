"""Radius outlier removal of a point list: md_op_radius_outliers and its host reference pipeline.radius_outliers.
include/mi_depth.h states the contract, DESIGN 12.7 the kernels. Selection: a row survives or it does not, on an integer count of
an f32 predicate, so every comparison is bit for bit.

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
NEW_ENTRIES = ("md_op_radius_outliers", "md_infer_points_outlier")
HALF = 1 << 20


def _brute(xyz, radius, k):
    """The contract applied literally, pair by pair in numpy scalars: cells, then the predicate -> (neighbours, dropped)."""
    r = f32(radius)
    r2 = r * r
    pts = [tuple(f32(a) for a in p) for p in np.asarray(xyz, f32).reshape(-1, 3)]
    cells = []
    with np.errstate(all="ignore"):
        for p in pts:
            c = [np.floor(a / r) for a in p]
            ok = all(np.isfinite(a) for a in p) and all(-HALF <= a < HALF for a in c)
            cells.append(tuple(int(a) for a in c) if ok else None)
        out = np.full(len(pts), -1, np.int32)
        for i, (pi, ci) in enumerate(zip(pts, cells)):
            if ci is None:
                continue
            n = 0
            for j, (pj, cj) in enumerate(zip(pts, cells)):
                if j == i or cj is None:
                    continue
                if abs(cj[0] - ci[0]) > 1 or abs(cj[1] - ci[1]) > 1 or abs(cj[2] - ci[2]) > 1:
                    continue
                dx, dy, dz = pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 <= r2:
                    n += 1
            out[i] = min(n, k)
    return out, sum(c is None for c in cells)


def _check_against_brute(xyz, radius, k):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    r = P.radius_outliers(xyz, radius, k)
    nb, dropped = _brute(xyz, radius, k)
    assert np.array_equal(r.neighbours, nb), (radius, k)
    assert r.dropped == dropped
    index = np.nonzero(nb == k)[0]
    assert np.array_equal(r.index, index) and r.index.dtype == np.int32 and r.neighbours.dtype == np.int32
    assert r.count.tolist() == [len(index), len(index)]
    assert np.array_equal(_bits(r.xyz), _bits(xyz[index]))
    return r


def _cloud(n, side, seed, cell=0.25):
    """n points uniform in a cube of `side`^3 cells of size `cell` around the origin: both signs of every coordinate"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-side / 2, side / 2, (n, 3)) * cell).astype(f32)


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n).astype(f32), rng.integers(0, 256, (n, 3), dtype=np.uint8), rng.normal(size=(n, 3)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_outlier_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "} md_points_outlier;" in header
    assert [n for n, _ in _lib.MdPointsOutlier._fields_] == ["radius", "min_neighbours", "neighbours", "index", "dropped"]


def test_reference_against_brute_force():
    for n, side, seed, radius, k in ((400, 4, 0, 0.25, 5), (200, 3, 1, 0.125, 1), (200, 2, 2, 0.5, 20), (150, 6, 3, 0.375, 3),
                                     (1, 1, 4, 0.25, 1), (300, 4, 5, 0.3, 1 << 20)):
        r = _check_against_brute(_cloud(n, side, seed), radius, k)
        assert (np.diff(r.index) > 0).all()
    r = P.radius_outliers(np.zeros((0, 3), f32), 1.0, 1)
    assert r.count.tolist() == [0, 0] and r.neighbours.shape == (0,) and r.dropped == 0


def test_reference_distance_is_inclusive_and_one_ulp_beyond_is_out():
    r = f32(0.3)
    r2 = r * r
    # a pair on one axis at exactly the radius: dx = r, d2 = r * r = r2
    on = np.array([[0.0, 0.0, 0.0], [r, 0.0, 0.0]], f32)
    assert f32(on[1, 0] - on[0, 0]) == r
    assert _check_against_brute(on, r, 1).neighbours.tolist() == [1, 1]
    # one ulp beyond in that coordinate: d2 > r2
    off = np.array([[0.0, 0.0, 0.0], [np.nextafter(r, f32(1)), 0.0, 0.0]], f32)
    assert f32(off[1, 0]) * f32(off[1, 0]) > r2
    assert _check_against_brute(off, r, 1).neighbours.tolist() == [0, 0]
    # off the axes: the sum of the three rounded squares decides, in the contract's order
    rng = np.random.default_rng(6)
    d = rng.normal(size=(200, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * float(r)).astype(f32)  # on the sphere, up to rounding
    inside = 0
    for row in d:
        pair = np.array([[0, 0, 0], row], f32)
        want = int((row[0] * row[0] + row[1] * row[1]) + row[2] * row[2] <= r2)
        assert P.radius_outliers(pair, r, 1).neighbours.tolist() == [want, want]  # symmetric
        inside += want
    assert 0 < inside < 200  # both sides of the rounding occur


def test_reference_pair_two_cells_apart_is_not_a_neighbour_pair():
    """The cell condition is part of the definition. A pair can pass d2 <= r2 and sit two cells apart only through the rounded
    difference: p_i just below 0 lies in cell -1, p_j = radius in cell 1, and dx = radius - p_i.x rounds to the radius. (A
    quotient that rounds up to an integer moves a point one cell up, but a search over 10^7 radii and cells found no pair that
    then also passes the distance test: the rows are at least one ulp of the radius too far apart.)"""
    for r in (f32(0.3), f32(1.0), f32(0.013)):
        pair = np.array([[-1e-30, 0.0, 0.0], [r, 0.0, 0.0]], f32)
        c = np.floor(pair[:, 0] / r)
        assert c.tolist() == [-1.0, 1.0]
        dx = f32(pair[1, 0] - pair[0, 0])
        assert dx == r and dx * dx <= r * r  # the pure radius test would count the pair
        nb, _ = _brute(pair, r, 1)
        assert nb.tolist() == [0, 0]
        assert P.radius_outliers(pair, r, 1).neighbours.tolist() == [0, 0]
        # a third point in the cell between them is within reach of both
        three = np.concatenate([pair, np.array([[r * f32(0.5), 0.0, 0.0]], f32)])
        assert _check_against_brute(three, r, 2).neighbours.tolist() == [1, 1, 2]
    # the largest float below 1 and 2.0 at radius 1: cells 0 and 2, dx = 1 + 2^-24 rounds to 1
    pair = np.array([[np.nextafter(f32(1), f32(0)), 0, 0], [2, 0, 0]], f32)
    assert f32(pair[1, 0] - pair[0, 0]) == f32(1)
    assert _check_against_brute(pair, 1.0, 1).neighbours.tolist() == [0, 0]
    # a quotient that rounds up to an integer: b < 5 r exactly, yet b / r == 5 in f32, so b lies in cell 5 and not in cell 4. A
    # row in cell 3 within the radius of b would be such a pair, and there is none: the reference and the literal loop agree on
    # every row of a line of floats from cell 3 up to b.
    r = f32(0.1)
    b = f32(0.5)
    assert float(b) < 5 * float(r) and f32(b / r) == f32(5) and np.floor(f32(b / r)) == 5
    a = [np.nextafter(f32(0.4), f32(0))]
    while len(a) < 6:
        a.append(np.nextafter(a[-1], f32(1)))  # across the face between cells 3 and 4
    cells = np.floor(np.array(a, f32) / r)
    assert cells.min() == 3 and cells.max() == 4
    line = np.array([[v, 0, 0] for v in a] + [[b, 0, 0], [0.55, 0, 0]], f32)
    got = _check_against_brute(line, r, 1 << 20)
    pure = sum(bool(f32(b - v) * f32(b - v) <= r * r) for v in a)  # rows the pure radius test would give b
    assert got.neighbours[len(a)] == 1 + sum(bool(f32(b - v) * f32(b - v) <= r * r) for v, c in zip(a, cells) if c == 4) <= 1 + pure


def test_reference_duplicates_count_each_other_and_a_row_never_counts_itself():
    one = np.array([[0.1, -0.2, 0.3]], f32)
    assert P.radius_outliers(one, 0.5, 1).neighbours.tolist() == [0]
    assert P.radius_outliers(one, 0.5, 1).count.tolist() == [0, 0]
    dup = np.repeat(one, 5, 0)
    r = _check_against_brute(dup, 0.5, 4)
    assert r.neighbours.tolist() == [4] * 5 and r.index.tolist() == [0, 1, 2, 3, 4]  # the four others, not itself
    assert _check_against_brute(dup, 0.5, 5).index.tolist() == []
    # duplicates beside a lone point: equal coordinates are neighbours, the lone one has none
    mixed = np.concatenate([dup[:3], np.array([[5, 5, 5]], f32)])
    assert _check_against_brute(mixed, 0.5, 2).neighbours.tolist() == [2, 2, 2, 0]


def test_reference_count_saturates_at_k():
    xyz = _cloud(300, 2, 7)  # dense: every row has dozens of neighbours
    full = P.radius_outliers(xyz, 0.25, 1 << 20).neighbours
    assert full.max() > 20 and full.min() >= 0
    for k in (1, 7, 20):
        r = _check_against_brute(xyz, 0.25, k)
        assert np.array_equal(r.neighbours, np.minimum(full, k))
        assert np.array_equal(r.index, np.nonzero(full >= k)[0])
    assert P.radius_outliers(xyz, 0.25, 1 << 20).count.tolist() == [0, 0]  # k above every count: nobody survives


def test_reference_negative_cells_and_the_sign_boundary():
    v = f32(0.375)
    ks = np.arange(-5, 6)
    faces = np.array([[k * v, -k * v, 0.0] for k in ks] + [[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], f32)
    assert np.array_equal(np.floor(faces[:len(ks), 0] / v).astype(int), ks)  # k v lies in cell k, -k v in cell -k
    _check_against_brute(faces, v, 1)
    below = np.nextafter(faces[:len(ks)], f32(-np.inf)).astype(f32)
    _check_against_brute(np.concatenate([faces, below]), v, 2)
    # -0.1 lies in cell -1, 0.1 in cell 0: neighbours across the boundary
    r = _check_against_brute(np.array([[-0.1, 0, 0], [0.1, 0, 0], [-0.9, 0, 0], [0.95, 0, 0]], f32), 1.0, 1)
    assert r.neighbours.tolist() == [1, 1, 1, 1]
    _check_against_brute(_cloud(250, 2, 8), 0.25, 4)  # a cloud around the origin, eight octants


def test_reference_rows_outside_the_grid_get_minus_one_and_are_counted():
    edge = np.array([[-HALF, 0, 0], [HALF - 1, 0, 0], [0, HALF - 0.5, -HALF], [HALF, 0, 0], [-HALF - 1, 0, 0], [0, 0, 3e38], [np.nan, 0, 0],
                     [0, np.inf, 0], [0, 0, -np.inf], [1, 2, 3], [1, 2, 3.5], [-HALF + 0.5, 0, 0]], f32)
    r = _check_against_brute(edge, 1.0, 1)
    assert r.neighbours.tolist() == [1, 0, 0, -1, -1, -1, -1, -1, -1, 1, 1, 1] and r.dropped == 6
    assert r.index.tolist() == [0, 9, 10, 11]  # the rows at the lower edge of the grid look at cells outside it: skipped
    r = _check_against_brute(edge, 1e-3, 1)  # p / radius leaves the grid for all but the rows near the origin
    assert r.dropped == 10 and r.neighbours.tolist() == [-1] * 9 + [0, 0, -1]
    _check_against_brute(np.array([[3e38, 0, 0], [1, 1, 1], [1, 1, 1]], f32), 1e-3, 1)  # the quotient overflows to inf


def test_reference_shuffle_keeps_the_same_points_and_counts_per_view():
    xyz = _cloud(900, 5, 9)
    a = P.radius_outliers(xyz, 0.25, 22)
    assert 0.2 < len(a.index) / 900 < 0.8
    perm = np.random.default_rng(10).permutation(900)
    b = P.radius_outliers(xyz[perm], 0.25, 22)
    assert np.array_equal(np.sort(perm[b.index]), a.index)
    assert np.array_equal(b.neighbours, a.neighbours[perm])
    conf, rgb, nrm = _rows(900, 11)
    r = P.radius_outliers(xyz, 0.25, 22, conf, rgb, nrm, counts=[200, 0, 450, 250])
    bd = np.array([0, 200, 200, 650, 900])
    assert r.count.tolist() == [int(((r.index >= bd[i]) & (r.index < bd[i + 1])).sum()) for i in range(4)] + [len(r.index)]
    assert r.count[1] == 0 and np.array_equal(r.index, a.index)
    assert np.array_equal(_bits(r.conf), _bits(conf[a.index])) and np.array_equal(r.rgb, rgb[a.index])
    assert np.array_equal(_bits(r.normals), _bits(nrm[a.index]))


def test_reference_refusals():
    xyz = _cloud(10, 2, 12)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.radius_outliers(xyz, bad, 1)
    for bad in (0, -3, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError):
            P.radius_outliers(xyz, 0.5, bad)
    P.radius_outliers(xyz, 0.5, 1 << 20)


def test_outlier_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched: with a null device the valid call is refused last, for the device."""
    buf = (C.c_float * 64)()
    px = C.cast(buf, C.c_void_p)
    listed = _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, 4, None)
    no_count = _lib.MdPointsOutputs(None, None, None, None, None, None, 4, None)
    O = _lib.MdPointsOutlier

    def why(outl, out=listed, N=4, code=_lib.MD_ERR_INVALID_ARG, xyz=px, normals_out=None):
        rc = lib.md_op_radius_outliers(None, xyz, None, None, None, N, C.byref(outl) if outl else None, C.byref(out) if out else None,
                                       normals_out, None)
        assert rc == code, rc
        return lib.md_last_error().decode()

    for bad in (float("nan"), float("inf"), -0.5, 0.0):
        assert "radius" in why(O(bad, 3, None, None, None)), bad
    for bad in (0, -1, (1 << 20) + 1):
        assert "min_neighbours" in why(O(0.5, bad, None, None, None)), bad
    assert "need `count`" in why(O(0.5, 3, None, px.value, None), no_count)  # index
    assert "need `count`" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(None, None, px.value, None, None, None, 4, None))
    assert "device is null" in why(O(0.5, 3, px.value, None, px.value), no_count)  # neighbours and dropped alone need no list
    assert "negative" in why(O(0.5, 3, None, None, None), N=-1)
    assert "negative" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, -1, None))
    assert "2^30" in why(O(0.5, 3, None, None, None), N=1 << 30, code=_lib.MD_ERR_SHAPE)
    assert "confidence row" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(None, None, px.value, None, px.value, px.value, 4, None))
    assert "rgb row" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(None, None, px.value, px.value, None, px.value, 4, None))
    assert "normals row" in why(O(0.5, 3, None, None, None), normals_out=px)
    assert "dense" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(px.value, None, px.value, None, None, px.value, 4, None))
    assert "dense" in why(O(0.5, 3, None, None, None), _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, 4, px.value))
    assert "xyz pointer is null" in why(O(0.5, 3, None, None, None), xyz=None)
    assert "options are null" in why(None)
    assert "outputs are null" in why(O(0.5, 3, None, None, None), out=None)
    assert "device is null" in why(O(0.5, 1 << 20, px.value, px.value, px.value))
    # the model call: the outlier part is checked with the other arguments (here: refused for the null model first)
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    outl = O(-1.0, 1, None, None, None)
    rc = lib.md_infer_points_outlier(None, px, 1, 2, 2, 1, None, None, None, C.byref(o), C.byref(listed), None, None, None, None, None,
                                     C.byref(outl), 1, None)
    assert rc == _lib.MD_ERR_INVALID_ARG and "model is null" in lib.md_last_error().decode()
    assert (np.frombuffer(buf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0
CANARY = 16  # elements behind the end of every output buffer
FILLS = dict(xyz=POISON, conf=POISON, rgb=77, normals=POISON, index=-7, neighbours=-7, count=-5, dropped=-5)


def _fresh(n, cap, conf, rgb, normals):
    from burn_depth_amd.depth_pro import PointCloud
    out, stores = PointCloud(), {}

    def put(name, shape, dtype=torch.float32):
        size = int(np.prod(shape))
        stores[name] = torch.full((size + CANARY,), FILLS[name], dtype=dtype, device="cuda")
        setattr(out, name, stores[name][:size].view(shape))

    put("xyz", (cap, 3))
    put("index", (cap,), torch.int32)
    put("neighbours", (n,), torch.int32)
    put("count", (2,), torch.int32)
    put("dropped", (1,), torch.int32)
    if conf:
        put("conf", (cap,))
    if rgb:
        put("rgb", (cap, 3), torch.uint8)
    if normals:
        put("normals", (cap, 3))
    return out, stores


def _run(dev, xyz, radius, k, conf=None, rgb=None, normals=None, capacity=None):
    """ops.radius_outliers on poisoned, guarded outputs -> numpy dict"""
    from burn_depth_amd import ops
    cap = len(xyz) if capacity is None else capacity
    out, stores = _fresh(len(xyz), cap, conf is not None, rgb is not None, normals is not None)
    ops.radius_outliers(dev, _t(xyz), radius, k, conf=_t(conf), rgb=_t(rgb), normals=_t(normals), out=out)
    torch.cuda.synchronize()
    for name, store in stores.items():
        assert (store[-CANARY:] == FILLS[name]).all(), name
    return {k_: v.cpu().numpy() for k_, v in vars(out).items() if v is not None}


def _assert_same(got, ref, what=""):
    assert got["count"].tolist() == [int(ref.count[-1])] * 2, (what, got["count"], ref.count)
    assert int(got["dropped"][0]) == ref.dropped, what
    assert np.array_equal(got["neighbours"], ref.neighbours), what
    cap = got["xyz"].shape[0]
    n = min(int(ref.count[-1]), cap)
    for k in ("xyz", "conf", "normals"):
        if k in got:
            assert np.array_equal(_bits(got[k][:n]), _bits(getattr(ref, k)[:n])), (what, k)
            assert (got[k][n:] == f32(POISON)).all(), (what, k)  # the rows behind the survivors stay untouched
    if "rgb" in got:
        assert np.array_equal(got["rgb"][:n], ref.rgb[:n]) and (got["rgb"][n:] == 77).all(), what
    assert np.array_equal(got["index"][:n], ref.index[:n]) and (got["index"][n:] == -7).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_wave_and_workgroup_edges_are_bit_identical_to_the_host_reference(dev, n):
    side = max(2, int(round((n / 2.5) ** (1 / 3))))  # about 2.5 points per cell at every size: about 10 within the radius
    xyz = _cloud(n, side, 20 + n)
    conf, rgb, nrm = _rows(n, n)
    ref = P.radius_outliers(xyz, 0.25, 6, conf, rgb, nrm)
    if n > 1:
        assert 0 < ref.count[-1] < n
    _assert_same(_run(dev, xyz, 0.25, 6, conf, rgb, nrm), ref, n)


@pytest.mark.gpu
def test_dense_grid_where_about_half_survive(dev):
    n = 5000
    xyz = _cloud(n, 8, 4)  # 8^3 = 512 cells: about 10 points each, long buckets on the 16384-slot table's few keys
    ref = P.radius_outliers(xyz, 0.25, 35)
    assert 0.2 <= ref.count[-1] / n <= 0.8, ref.count  # the rows near the faces of the cube have fewer neighbours
    got = _run(dev, xyz, 0.25, 35)
    _assert_same(got, ref, "bare")
    assert "conf" not in got and "rgb" not in got and "normals" not in got
    conf, rgb, nrm = _rows(n, 5)
    _assert_same(_run(dev, xyz, 0.25, 35, conf, rgb, nrm), P.radius_outliers(xyz, 0.25, 35, conf, rgb, nrm), "rows")
    _assert_same(_run(dev, xyz, 0.25, 35, None, rgb), P.radius_outliers(xyz, 0.25, 35, None, rgb), "rgb only")


@pytest.mark.gpu
def test_coincident_points_all_survive(dev):
    n, k = 10000, 8
    xyz = np.tile(np.array([[0.3, -1.7, 2.2]], f32), (n, 1))
    got = _run(dev, xyz, 0.05, k)
    assert got["count"].tolist() == [n, n] and (got["neighbours"] == k).all() and np.array_equal(got["index"], np.arange(n))
    assert np.array_equal(_bits(got["xyz"]), _bits(xyz))
    _assert_same(got, P.radius_outliers(xyz, 0.05, k))


@pytest.mark.gpu
def test_every_point_alone_in_a_far_cell_leaves_nothing(dev):
    n = 5000
    cells = np.random.default_rng(2).permutation(40 ** 3)[:n]
    r = f32(0.5)
    xyz = ((np.stack([cells % 40, cells // 40 % 40, cells // 1600], 1) - 20) * 3 + 0.5).astype(f32) * r  # every third cell
    got = _run(dev, xyz, r, 1)
    assert got["count"].tolist() == [0, 0] and (got["neighbours"] == 0).all() and got["dropped"][0] == 0
    assert (got["xyz"] == f32(POISON)).all() and (got["index"] == -7).all()
    _assert_same(got, P.radius_outliers(xyz, r, 1))


@pytest.mark.gpu
def test_planted_isolated_points_are_exactly_the_ones_removed(dev):
    rng = np.random.default_rng(3)
    g = np.arange(60) * 0.01
    patch = np.stack(list(np.meshgrid(g, g, indexing="ij")) + [np.zeros((60, 60))], -1).reshape(-1, 3)
    patch = patch + rng.uniform(-0.001, 0.001, patch.shape)
    patch[:, 2] = 0.02 * np.sin(7 * patch[:, 0]) + patch[:, 2]  # a gently curved surface through the sign boundary of z
    planted = np.stack([rng.uniform(0, 0.6, 50), rng.uniform(0, 0.6, 50), 0.3 + 0.1 * np.arange(50)], 1)  # 0.1 apart, far above
    xyz = np.concatenate([patch, planted]).astype(f32)
    where = rng.permutation(len(xyz))
    xyz = xyz[where]
    is_planted = where >= len(patch)
    ref = P.radius_outliers(xyz, 0.025, 4)
    assert np.array_equal(ref.index, np.nonzero(~is_planted)[0])  # every surface row has four neighbours, corners included
    assert (ref.neighbours[is_planted] == 0).all()
    got = _run(dev, xyz, 0.025, 4)
    _assert_same(got, ref)
    assert got["count"][0] == len(patch) and np.array_equal(got["index"][:len(patch)], np.nonzero(~is_planted)[0])


@pytest.mark.gpu
def test_k_of_one_k_above_every_count_and_rows_outside_the_grid(dev):
    v = f32(0.375)
    xyz = _cloud(3000, 10, 6, cell=float(v))
    rng = np.random.default_rng(7)
    bad = rng.permutation(3000)[:300]
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:200], rng.integers(0, 3, 100)] = np.array([np.inf, -np.inf], f32)[rng.integers(0, 2, 100)]
    xyz[bad[200:], rng.integers(0, 3, 100)] = f32(HALF) * v * f32(1.5)  # beyond the grid
    a = np.arange(-20, 21)
    faces = np.array([[i * v, -i * v, b] for i in a for b in (-0.0, 0.0)], f32)  # on the faces of the cells, both zeros
    xyz = np.concatenate([xyz, faces, np.nextafter(faces, f32(-np.inf)).astype(f32)])
    ref = P.radius_outliers(xyz, v, 1)
    assert ref.dropped == 300 and (ref.neighbours[bad] == -1).all() and 0 < ref.count[-1] <= len(xyz) - 300
    _assert_same(_run(dev, xyz, v, 1), ref, "k = 1")
    top = P.radius_outliers(xyz, v, 1 << 20)
    assert top.count[-1] == 0 and top.neighbours.max() > 2
    got = _run(dev, xyz, v, 1 << 20)
    _assert_same(got, top, "k = 2^20")  # nothing saturates: neighbours is the full count of every row
    edge = np.array([[-HALF, 0, 0], [HALF - 1, 0, 0], [0, HALF - 0.5, -HALF], [HALF, 0, 0], [-HALF - 1, 0, 0], [1, 2, 3], [1, 2, 3.5],
                     [-HALF + 0.5, 0, 0]], f32)
    got = _run(dev, edge, 1.0, 1)  # rows at the edge of the grid look at cells outside it
    assert got["neighbours"].tolist() == [1, 0, 0, -1, -1, 1, 1, 1] and got["dropped"][0] == 2
    pair = np.array([[-1e-30, 0.0, 0.0], [0.3, 0.0, 0.0]], f32)  # within the radius after rounding, two cells apart
    assert _run(dev, pair, f32(0.3), 1)["neighbours"].tolist() == [0, 0]
    everything = _run(dev, np.full((70, 3), np.nan, f32), 1.0, 1)
    assert everything["count"].tolist() == [0, 0] and everything["dropped"][0] == 70 and (everything["neighbours"] == -1).all()


@pytest.mark.gpu
def test_capacity_below_the_survivors_keeps_the_true_count(dev):
    n = 9000
    xyz = _cloud(n, 12, 8)
    conf, rgb, nrm = _rows(n, 9)
    ref = P.radius_outliers(xyz, 0.25, 20, conf, rgb, nrm)
    total = int(ref.count[-1])
    assert 3000 < total < n
    for cap in (total // 2, 1, 0, total - 1):
        got = _run(dev, xyz, 0.25, 20, conf, rgb, nrm, capacity=cap)  # _run checks the sentinels behind row `cap`
        assert got["xyz"].shape[0] == cap
        _assert_same(got, ref, cap)


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_and_a_shuffle_the_same_points(dev):
    xyz = _cloud(8000, 10, 10)
    conf, rgb, nrm = _rows(8000, 11)
    a = _run(dev, xyz, 0.25, 28, conf, rgb, nrm)
    b = _run(dev, xyz, 0.25, 28, conf, rgb, nrm)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    n = int(a["count"][0])
    assert 0.2 < n / 8000 < 0.8
    perm = np.random.default_rng(12).permutation(8000)
    c = _run(dev, xyz[perm], 0.25, 28)
    assert c["count"][0] == n and np.array_equal(np.sort(perm[c["index"][:n]]), a["index"][:n])
    assert np.array_equal(c["neighbours"], a["neighbours"][perm])


@pytest.mark.gpu
def test_outlier_refusals_leave_the_outputs_untouched(dev):
    from burn_depth_amd import ops
    xyz = _cloud(500, 4, 12)
    conf = _rows(500, 13)[0]

    def refused(code, radius=0.25, k=3, strip=()):
        out, stores = _fresh(500, 500, True, False, False)
        for name in strip:
            setattr(out, name, None)
        with pytest.raises(_lib.MdError) as e:
            ops.radius_outliers(dev, _t(xyz), radius, k, conf=_t(conf), out=out)
        assert e.value.code == code
        torch.cuda.synchronize()
        for name, store in stores.items():
            assert (store == FILLS[name]).all(), name

    for bad in (float("nan"), float("inf"), -0.25, 0.0):
        refused(_lib.MD_ERR_INVALID_ARG, radius=bad)
    for bad in (0, (1 << 20) + 1):
        refused(_lib.MD_ERR_INVALID_ARG, k=bad)
    refused(_lib.MD_ERR_INVALID_ARG, strip=("count",))  # index and the list without count
    out, _ = _fresh(500, 500, False, False, False)
    out.conf = torch.empty(500, device="cuda")
    with pytest.raises(_lib.MdError) as e:  # a conf output without a confidence row
        ops.radius_outliers(dev, _t(xyz), 0.25, 3, out=out)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    # an empty list is not an error
    got = ops.radius_outliers(dev, torch.empty((0, 3), device="cuda"), 0.25, 3)
    torch.cuda.synchronize()
    assert got.count.tolist() == [0, 0] and got.dropped.item() == 0 and got.neighbours.shape == (0,)
