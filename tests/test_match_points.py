"""The nearest row of a reference cloud for every row of a point list: md_op_match_points and its host reference
pipeline.match_points. include/mi_depth.h states the contract, DESIGN 12.13 the kernels. Every output is a selection on a
deterministic f32 value, so every comparison is bit for bit.

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
NEW_ENTRIES = ("md_op_match_points", "md_infer_points_match")
FIELDS = ["radius", "target", "target_rows", "target_kind", "mode", "tol", "nearest", "dist2", "stats", "index", "dropped"]
INF_BITS = 0x7F800000
RADII = (0.1, 0.125, 0.15)  # at these between 0.2 and 0.8 of the in-range rows of the scenes below have a counterpart


def _brute(xyz, target, radius, tol=()):
    """The contract applied literally, pair by pair in numpy scalars -> (nearest, dist2 bits, stats, dropped)."""
    src = [tuple(f32(a) for a in p) for p in np.asarray(xyz, f32).reshape(-1, 3)]
    tgt = [tuple(f32(a) for a in p) for p in np.asarray(target, f32).reshape(-1, 3)]
    r = f32(radius)
    r2, half = r * r, f32(1 << 20)

    def cell(p):
        with np.errstate(all="ignore"):
            cs = tuple(np.floor(a / r) for a in p)
        return cs if all(np.isfinite(a) for a in p) and all(-half <= c < half for c in cs) else None

    sc, tc = [cell(p) for p in src], [cell(p) for p in tgt]
    nearest, bits = [], []
    for i, p in enumerate(src):
        if sc[i] is None:
            nearest.append(-2)
            bits.append(INF_BITS)
            continue
        best = None
        for j, q in enumerate(tgt):
            if tc[j] is None or any(abs(int(a) - int(b)) > 1 for a, b in zip(sc[i], tc[j])):
                continue
            with np.errstate(all="ignore"):
                dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
                d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= r2:
                key = (int(f32(d2).view(np.uint32)) << 32) | j
                best = key if best is None or key < best else best
        nearest.append(-1 if best is None else best & 0xFFFFFFFF)
        bits.append(INF_BITS if best is None else best >> 32)
    nearest, bits = np.array(nearest, np.int64).astype(np.int32), np.array(bits, np.uint32)
    stats = [sum(c is not None for c in sc), int((nearest >= 0).sum()), sum(c is not None for c in tc), 0, 0, 0, 0, 0]
    for t, v in enumerate(tol):
        if f32(v) > 0:
            stats[4 + t] = int(((nearest >= 0) & (bits.view(f32) <= f32(v) * f32(v))).sum())
    return nearest, bits, np.array(stats, np.int32), sum(c is None for c in sc)


def _blobs(n, seed, spread=4.0, centres=6):
    """n points around a few centres plus uniform speckle, with three rows that are out of the contract's range"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (centres, 3))
    x = np.concatenate([c[rng.integers(0, centres, n - n // 5)] + rng.normal(0, 0.25, (n - n // 5, 3)), rng.uniform(-spread, spread, (n // 5, 3))])
    x = x[rng.permutation(n)].astype(f32)
    if n > 20:
        x[[3, n // 2, n - 2]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 3e30]]
    return x


def _pair(n, t, seed):
    """A source list of n rows and a target list of t rows: blobs plus speckle around the same centres, the target a jittered
    draw, each with a NaN, an inf and a 3e30 row (lists of more than 20 rows). Read-only."""
    a = _blobs(n, seed)
    rng = np.random.default_rng(seed + 100)
    b = _blobs(max(n, t), seed)[rng.permutation(max(n, t))[:t]].copy()
    ok = np.isfinite(b).all(1) & (np.abs(b) < 1e20).all(1)
    b[ok] += rng.normal(0, 0.08, (int(ok.sum()), 3)).astype(f32)
    if t > 20:
        b[[1, t // 3, t - 1]] = [[0, np.nan, 0], [np.inf, 0, 0], [0, 3e30, 0]]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _partly_matched(m):
    """the reference's own output: between 0.2 and 0.8 of the in-range rows have a counterpart"""
    return 0.2 * m.stats[0] <= m.stats[1] <= 0.8 * m.stats[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_match_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    body = header[header.index("typedef struct md_points_match {"):header.index("} md_points_match;")]
    assert re.findall(r"^\s+(?:const )?[a-z0-9_]+\*? (?:\*)?([a-z_0-9]+)(?:\[4\])?;", body, re.M) == FIELDS
    assert [n for n, _ in _lib.MdPointsMatch._fields_] == FIELDS
    # the model entry takes the cluster entry's arguments with the match part in front of out_kind
    clusters, match = _lib.SYMBOLS["md_infer_points_clusters"][1], _lib.SYMBOLS["md_infer_points_match"][1]
    assert match[:-2] == clusters[:-2] + [C.POINTER(_lib.MdPointsMatch)] and match[-2:] == clusters[-2:]


@pytest.mark.parametrize("tol", ((), (0.05, 0.0, 0.1)))
@pytest.mark.parametrize("radius", RADII)
def test_reference_against_brute_force(radius, tol):
    for (n, t), seed in (((60, 40), 0), ((400, 300), 1)):
        a, b = _pair(n, t, seed)
        nearest, bits, stats, dropped = _brute(a, b, radius, tol)
        for mode in (0, 1, 2):
            got = P.match_points(a, b, radius, tol=tol, mode=mode)
            assert _partly_matched(got), (n, radius, got.stats)
            assert np.array_equal(got.nearest, nearest) and np.array_equal(_bits(got.dist2), bits), (n, radius, mode)
            assert got.stats.tolist() == stats.tolist() and got.dropped == dropped == 3, (n, radius, got.stats, stats)
            if mode == 0:
                assert got.index is None and got.xyz is None and got.count is None
                continue
            index = np.nonzero(nearest >= 0 if mode == 1 else nearest == -1)[0]
            assert np.array_equal(got.index, index) and np.array_equal(_bits(got.xyz), _bits(a[index])) and got.count.tolist() == [len(index)] * 2


def _one(src, tgt, radius, **kw):
    return P.match_points(np.array(src, f32).reshape(-1, 3), np.array(tgt, f32).reshape(-1, 3), radius, **kw)


def test_pinned_radius_is_inclusive():
    r = f32(0.25)  # r*r is exact
    m = _one([[0, 0, 0]], [[r, 0, 0]], r)
    assert m.nearest.tolist() == [0] and _bits(m.dist2)[0] == _bits(r * r)[0]
    beyond = np.nextafter(r, f32(1))  # one ulp beyond: dx*dx rounds above r*r
    assert beyond * beyond > r * r
    m = _one([[0, 0, 0]], [[beyond, 0, 0]], r)
    assert m.nearest.tolist() == [-1] and _bits(m.dist2)[0] == INF_BITS and m.stats.tolist()[:3] == [1, 0, 1]


def test_pinned_pair_two_cells_apart_is_no_match():
    """a pair whose dx rounds to the radius but whose cells are two apart: the cell condition is part of the definition"""
    r = f32(1.0)
    s, t = f32(0.99999994), f32(2.0)  # cells 0 and 2; t - s = 1.00000006 rounds to 1.0 in f32
    assert f32(t - s) == r and np.floor(s / r) == 0 and np.floor(t / r) == 2
    m = _one([[s, 0.5, 0.5]], [[t, 0.5, 0.5]], r)
    assert m.nearest.tolist() == [-1] and m.stats.tolist()[:3] == [1, 0, 1]
    m = _one([[s, 0.5, 0.5]], [[t, 0.5, 0.5], [1.5, 0.5, 0.5]], r)  # the neighbour cell's row is one
    assert m.nearest.tolist() == [1]


def test_pinned_ties_and_duplicates_go_to_the_smaller_row():
    # two targets at equal d2 on either side: the smaller row wins, also when it lies in a later cell of the 27
    for tgt in ([[0.75, 0.5, 0.5], [0.25, 0.5, 0.5]], [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]]):
        assert _one([[0.5, 0.5, 0.5]], tgt, 1.0).nearest.tolist() == [0]
    later, earlier = [1.25, 0.5, 0.5], [-0.25, 0.5, 0.5]  # cells +1 and -1 on x: visited last and first
    m = _one([[0.5, 0.5, 0.5]], [later, earlier], 1.0)
    assert m.nearest.tolist() == [0] and m.dist2.tolist() == [0.5625]
    assert _one([[0.5, 0.5, 0.5]], [earlier, later], 1.0).nearest.tolist() == [0]
    m = _one([[0.5, 0.5, 0.5]], [[3, 3, 3], [0.5, 0.5, 0.75], [0.5, 0.5, 0.75], [0.5, 0.5, 0.75]], 1.0)  # duplicate target rows
    assert m.nearest.tolist() == [1]


def test_pinned_coincident_empty_and_out_of_range():
    m = _one([[0.3, -7.25, 2.0]], [[9, 9, 9], [0.3, -7.25, 2.0]], 0.05)
    assert m.nearest.tolist() == [1] and _bits(m.dist2)[0] == 0
    m = _one([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1]], np.zeros((0, 3)), 0.5, tol=(0.5,), mode=2)  # T = 0
    assert m.nearest.tolist() == [-1, -2, -1] and m.stats.tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and m.dropped == 1 and m.index.tolist() == [0, 2]
    assert (_bits(m.dist2) == INF_BITS).all()
    m = _one(np.zeros((0, 3)), [[0, 0, 0]], 0.5, mode=1)  # N = 0
    assert m.nearest.shape == (0,) and m.stats.tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and m.count.tolist() == [0, 0]
    m = _one([[100, 100, 100]], [[0, 0, 0], [1, 0, 0]], 0.5)  # in range, outside every occupied cell
    assert m.nearest.tolist() == [-1] and m.stats.tolist()[:3] == [1, 0, 2] and m.dropped == 0
    # a target row out of range is never returned, though it is the closest by its coordinates
    m = _one([[0, 0, 0], [3e30, 0, 0]], [[np.inf, 0, 0], [3e30, 0, 0], [0.25, 0, 0], [np.nan, 0, 0]], 0.5)
    assert m.nearest.tolist() == [2, -2] and m.stats.tolist()[:3] == [1, 1, 1] and m.dropped == 1


def test_pinned_tolerance_equal_to_the_radius_counts_every_match():
    a, b = _pair(400, 300, 1)
    for r in RADII:
        m = P.match_points(a, b, r, tol=(r, r / 2, 0.0, r))
        assert m.stats[4] == m.stats[1] == m.stats[7] and 0 < m.stats[5] < m.stats[1] and m.stats[6] == 0 and m.stats[3] == 0


def test_reference_refusals():
    a, b = _pair(60, 40, 0)
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=1e30),
                dict(tol=(-0.1,)), dict(tol=(0.6,)), dict(tol=(float("nan"),)), dict(tol=(0.1,) * 5), dict(mode=3), dict(mode=-1)):
        with pytest.raises(ValueError):
            P.match_points(a, b, **dict(dict(radius=0.5), **bad))


def test_refusals_before_any_launch(lib):
    """every refusal of the contract returns its code with a null device: the device is the last refusal, nothing is launched"""
    x = (C.c_float * 12)()
    px = C.cast(x, C.c_void_p)
    good = dict(radius=0.5, target=px.value, target_rows=4, target_kind=_lib.MD_MEM_DEVICE)
    tol = lambda *v: (C.c_float * 4)(*v)  # noqa: E731

    def call(mat, outs=None, n=4, xyz=px):
        return lib.md_op_match_points(None, xyz, None, None, None, n, mat, C.byref(outs if outs is not None else _lib.MdPointsOutputs()), None, None)

    assert call(None) == _lib.MD_ERR_INVALID_ARG
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=1e30),
                dict(tol=tol(-0.1)), dict(tol=tol(0, 0.6)), dict(tol=tol(0, 0, float("nan"))), dict(tol=tol(0, 0, 0, float("inf"))),
                dict(mode=3), dict(mode=-1), dict(target_rows=-1), dict(target=None), dict(target_kind=_lib.MD_MEM_HOST), dict(target_kind=7),
                dict(index=px.value)):
        assert call(C.byref(_lib.MdPointsMatch(**dict(good, **bad)))) == _lib.MD_ERR_INVALID_ARG, bad
    assert call(C.byref(_lib.MdPointsMatch(**dict(good, target_rows=1 << 30)))) == _lib.MD_ERR_SHAPE
    mat = C.byref(_lib.MdPointsMatch(**good))
    assert call(mat, n=-1) == _lib.MD_ERR_INVALID_ARG and call(mat, n=1 << 30) == _lib.MD_ERR_SHAPE
    assert call(mat, xyz=None) == _lib.MD_ERR_INVALID_ARG
    assert call(mat, _lib.MdPointsOutputs(capacity=-1)) == _lib.MD_ERR_INVALID_ARG
    assert call(mat, _lib.MdPointsOutputs(xyz=px.value, capacity=4)) == _lib.MD_ERR_INVALID_ARG  # a compacted output without count
    cnt = (C.c_int32 * 2)()
    with_list = _lib.MdPointsOutputs(xyz=px.value, count=C.cast(cnt, C.c_void_p).value, capacity=4)
    assert call(mat, with_list) == _lib.MD_ERR_INVALID_ARG  # ... or with mode 0
    assert call(mat, _lib.MdPointsOutputs(point_map=px.value)) == _lib.MD_ERR_INVALID_ARG  # a dense output
    for mode in (1, 2):
        keep = C.byref(_lib.MdPointsMatch(**dict(good, mode=mode)))
        assert call(keep, _lib.MdPointsOutputs(rgb=px.value, count=C.cast(cnt, C.c_void_p).value, capacity=4)) == _lib.MD_ERR_INVALID_ARG  # no rgb row
        assert call(keep, with_list) == _lib.MD_ERR_INVALID_ARG  # everything is in order: the null device is the last refusal
        assert "device is null" in lib.md_last_error().decode()
    empty = C.byref(_lib.MdPointsMatch(radius=0.5, target=None, target_rows=0, target_kind=_lib.MD_MEM_DEVICE))  # T = 0 is legal
    assert call(empty) == _lib.MD_ERR_INVALID_ARG and "device is null" in lib.md_last_error().decode()
    args = [None] * (len(_lib.SYMBOLS["md_infer_points_match"][1]) - 8)
    assert lib.md_infer_points_match(None, None, 1, 70, 70, _lib.MD_MEM_DEVICE, *args, _lib.MD_MEM_DEVICE, None) == _lib.MD_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the operator against pipeline.match_points
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0
TILE = 4096  # rows of one tile of tile_compact.h


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(getattr(pc, k)) for k in ("xyz", "conf", "rgb", "normals", "index", "count")}
    d.update({k: g(getattr(pc.match, k)) for k in ("nearest", "dist2", "stats", "dropped")})
    return d


def _same_as_host(got, want, n, what=""):
    """got: _np of the operator's cloud; want: HostMatch; n: the rows of the input"""
    assert np.array_equal(got["nearest"][:n], want.nearest), (what, "nearest")
    assert np.array_equal(got["dist2"][:n].view(np.uint32), _bits(want.dist2)), (what, "dist2")
    assert got["stats"].tolist() == want.stats.tolist(), (what, got["stats"], want.stats)
    assert int(got["dropped"][0]) == want.dropped, what
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


def _check(dev, xyz, target, what="", **kw):
    from burn_depth_amd import ops
    got = _np(ops.match_points(dev, _t(xyz), _t(target), **kw))
    want = P.match_points(xyz, target, **kw)
    _same_as_host(got, want, len(xyz), what)
    return got, want


@pytest.fixture(scope="module")
def scenes():
    """the pairs of the operator tests, computed once, never written"""
    return {(1, 1): (np.array([[0.5, 0.25, -1.0]], f32), np.array([[0.5, 0.3, -1.0]], f32)), (63, 65): _pair(63, 65, 4),
            (TILE + 1, 2049): _pair(TILE + 1, 2049, 3), (3000, 2000): _pair(3000, 2000, 2)}


def test_scenes_match_part_of_their_rows(scenes):
    for shape, (a, b) in scenes.items():
        m = P.match_points(a, b, 0.1, tol=(0.05, 0.1))
        assert shape == (1, 1) or (_partly_matched(m) and m.dropped == 3 and 0 < m.stats[2] <= shape[1] - 3), (shape, m.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("shape", ((1, 1), (63, 65), (TILE + 1, 2049), (3000, 2000)))
def test_operator_matches_the_reference(dev, scenes, shape, mode):
    a, b = scenes[shape]
    n = len(a)
    got, want = _check(dev, a, b, (shape, mode), radius=0.1, tol=(0.05, 0.1), mode=mode)
    if shape == (1, 1):
        assert want.nearest.tolist() == [0]
    rng = np.random.default_rng(6)
    conf, rgb, nrm = rng.random(n).astype(f32), rng.integers(0, 256, (n, 3)).astype(np.uint8), rng.normal(size=(n, 3)).astype(f32)
    from burn_depth_amd import ops
    kw = dict(radius=0.1, tol=(0.1, 0.0, 0.025), mode=mode)
    full = _np(ops.match_points(dev, _t(a), _t(b), conf=_t(conf), rgb=_t(rgb), normals=_t(nrm), **kw))
    _same_as_host(full, P.match_points(a, b, conf=conf, rgb=rgb, normals=nrm, **kw), n, (shape, mode, "all rows"))
    by_name = dict(kw, mode=("label", "matched", "unmatched")[mode])
    _same_as_host(_np(ops.match_points(dev, _t(a), _t(b), conf=_t(conf), **by_name)), P.match_points(a, b, conf=conf, **kw), n, "by name")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 2))
def test_capacity_below_the_kept_count(dev, scenes, mode):
    from burn_depth_amd import ops
    xyz, target = scenes[(TILE + 1, 2049)]
    n = len(xyz)
    rng = np.random.default_rng(7)
    conf, nrm = rng.random(n).astype(f32), rng.normal(size=(n, 3)).astype(f32)
    kw = dict(radius=0.1, mode=mode)
    want = P.match_points(xyz, target, conf=conf, normals=nrm, **kw)
    m = len(want.index)
    assert 500 < m < n - 500
    cap = m - 77
    short = ops.match_points(dev, _t(xyz), _t(target), conf=_t(conf), normals=_t(nrm), capacity=cap + 9, **kw)
    for t in (short.xyz, short.conf, short.normals):
        t.fill_(POISON)
    short.index.fill_(-5)
    short.xyz, short.conf, short.normals, short.index = short.xyz[:cap + 5], short.conf[:cap + 3], short.normals[:cap + 5], short.index[:cap]
    keep = [t.clone() for t in (short.xyz, short.conf, short.normals)]
    got = _np(ops.match_points(dev, _t(xyz), _t(target), conf=_t(conf), normals=_t(nrm), out=short, **kw))  # capacity = the shortest: cap < M
    assert got["count"].tolist() == [m, m]
    for k, ref in (("xyz", want.xyz), ("conf", want.conf), ("normals", want.normals), ("index", want.index)):
        assert np.array_equal(got[k][:cap].view(np.uint8), np.ascontiguousarray(ref[:cap]).view(np.uint8)), k
    for k, t in zip(("xyz", "conf", "normals"), keep):
        assert (got[k][cap:] == POISON).all() and (t[cap:].cpu().numpy() == POISON).all(), k  # the sentinels behind the capacity
    assert np.array_equal(got["nearest"], want.nearest)


@pytest.mark.gpu
def test_every_output_skipped_in_turn(dev, lib, scenes):
    a, b = scenes[(63, 65)]
    n = len(a)
    want = P.match_points(a, b, 0.1, tol=(0.05,), mode=1)
    xyz, tgt = _t(a), _t(b)
    for skip in ("nearest", "dist2", "stats", "index", "dropped", "xyz"):
        o = dict(nearest=torch.full((n,), -9, dtype=torch.int32, device="cuda"), dist2=torch.full((n,), POISON, device="cuda"),
                 stats=torch.full((8,), -9, dtype=torch.int32, device="cuda"), index=torch.full((n,), -9, dtype=torch.int32, device="cuda"),
                 dropped=torch.full((1,), -9, dtype=torch.int32, device="cuda"), xyz=torch.full((n, 3), POISON, device="cuda"))
        count = torch.full((2,), -9, dtype=torch.int32, device="cuda")
        p = lambda k: None if k == skip else o[k].data_ptr()  # noqa: E731
        mat = _lib.MdPointsMatch(0.1, tgt.data_ptr(), len(b), _lib.MD_MEM_DEVICE, 1, (C.c_float * 4)(0.05), p("nearest"), p("dist2"), p("stats"),
                                 p("index"), p("dropped"))
        outs = _lib.MdPointsOutputs(xyz=p("xyz"), count=count.data_ptr(), capacity=n)
        _lib.check(lib.md_op_match_points(dev.handle, xyz.data_ptr(), None, None, None, n, C.byref(mat), C.byref(outs), None,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        m = len(want.index)
        ref = dict(nearest=want.nearest, dist2=want.dist2, stats=want.stats, dropped=np.array([want.dropped], np.int32))
        for k, t in o.items():
            got = t.cpu().numpy()
            if k == skip:
                assert (got == (POISON if got.dtype == f32 else -9)).all(), (skip, k)  # untouched
            elif k in ("index", "xyz"):
                assert np.array_equal(got[:m].view(np.uint8), np.ascontiguousarray(getattr(want, k)).view(np.uint8)), (skip, k)
            else:
                assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(ref[k]).view(np.uint8)), (skip, k)
        assert count.cpu().tolist() == [m, m]


@pytest.mark.gpu
def test_operator_refusals_and_the_empty_lists(dev):
    from burn_depth_amd import ops
    a, b = (_t(v) for v in _pair(63, 65, 4))
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=1e30), dict(tol=(-0.1,)),
                dict(tol=(0.0, 0.6)), dict(tol=(float("nan"),)), dict(mode=3), dict(mode=-1)):
        with pytest.raises(_lib.MdError) as e:
            ops.match_points(dev, a, b, **dict(dict(radius=0.5), **bad))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
    none = torch.zeros((0, 3), device="cuda")
    got = _np(ops.match_points(dev, none, b, radius=0.5, mode=1))  # N = 0
    src, tgt = _pair(63, 65, 4)
    in_grid = int(P.match_points(src, tgt, 0.5).stats[2])
    assert got["count"].tolist() == [0, 0] and got["stats"].tolist() == [0, 0, in_grid, 0, 0, 0, 0, 0] and got["dropped"].tolist() == [0]
    got = _np(ops.match_points(dev, a, none, radius=0.5, tol=(0.5,), mode=2))  # T = 0: every in-range row is unmatched
    _same_as_host(got, P.match_points(src, np.zeros((0, 3), f32), 0.5, tol=(0.5,), mode=2), 63, "T = 0")
    assert got["count"].tolist() == [60, 60] and got["stats"].tolist() == [60, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.gpu
def test_pinned_cases_on_the_device(dev):
    r = f32(0.25)
    beyond = np.nextafter(r, f32(1))
    src = np.array([[0, 0, 0], [0, 8, 0], [20.5, 0.5, 0.5], [30.99999994, 0.5, 0.5], [40.3, -7.25, 2.0], [100, 100, 100]], f32)
    tgt = np.array([[r, 0, 0], [beyond, 8, 0], [20.75, 0.5, 0.5], [20.25, 0.5, 0.5], [40.3, -7.25, 2.0], [40.3, -7.25, 2.0],
                    [np.inf, 0, 0]], f32)
    got, want = _check(dev, src, tgt, "pinned", radius=r, tol=(r,))
    assert want.nearest.tolist() == [0, -1, 2, -1, 4, -1] and _bits(want.dist2)[4] == 0 and want.stats[4] == want.stats[1] == 3
    s, t = f32(0.99999994), f32(2.0)  # two cells apart, dx rounds to the radius
    got, want = _check(dev, np.array([[s, 0.5, 0.5]], f32), np.array([[t, 0.5, 0.5]], f32), "two cells", radius=1.0)
    assert want.nearest.tolist() == [-1]
    later, earlier = [1.25, 0.5, 0.5], [-0.25, 0.5, 0.5]
    got, want = _check(dev, np.array([[0.5, 0.5, 0.5]], f32), np.array([later, earlier], f32), "tie across cells", radius=1.0)
    assert want.nearest.tolist() == [0]


@pytest.mark.gpu
def test_swapped_call_and_cloud_distance(dev, scenes):
    from burn_depth_amd import ops
    a, b = scenes[(3000, 2000)]
    tol = (0.05, 0.1)
    ab, _ = _check(dev, a, b, "a -> b", radius=0.1, tol=tol)
    ba, want = _check(dev, b, a, "b -> a", radius=0.1, tol=tol)
    assert want.stats[2] == ab["stats"][0] and ba["stats"][0] == ab["stats"][2] and ba["nearest"].shape == (2000,)
    d = ops.cloud_distance(dev, _t(a), _t(b), 0.1, tol)
    assert d["stats_ab"] == ab["stats"].tolist() and d["stats_ba"] == ba["stats"].tolist()
    assert d["precision"] == [int(ab["stats"][4 + t]) / 3000 for t in range(2)] and d["recall"] == [int(ba["stats"][4 + t]) / 2000 for t in range(2)]
    assert all(0 < f < 1 for f in d["fscore"])
    both = [np.sqrt(m["dist2"][m["nearest"] >= 0].astype(np.float64)).mean() for m in (ab, ba)]
    assert abs(d["chamfer"] - sum(both)) < 1e-6  # a float mean: outside the bit contract
