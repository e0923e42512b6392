"""RANSAC plane extraction from a point list: md_op_fit_planes and its host reference pipeline.fit_planes. include/mi_depth.h states
the contract, DESIGN 12.11 the kernels. The decision is an integer inlier count of an f32 predicate and the winner an arg-max
with a fixed tie rule, so every comparison is bit for bit.

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
NEW_ENTRIES = ("md_op_fit_planes", "md_infer_points_planes")
FIELDS = ["planes", "hypotheses", "tol", "min_inliers", "seed", "normal_min_cos", "axis", "axis_min_cos", "mode", "plane", "plane_count",
          "hypothesis", "label", "index", "dropped"]
MASK = (1 << 64) - 1
_OPS_H = open(os.path.join(ROOT, "burn_depth_amd", "csrc", "kernels", "ops.h")).read()
# kPlaneCountChunk: hypotheses of one trip of the count kernel's loop, a tail loop takes the rest
COUNT_CHUNK = int(re.search(r"constexpr int kPlaneCountChunk = (\d+);", _OPS_H).group(1))
# 256 threads x kPlaneCountRows: live rows of one pass of a count workgroup
COUNT_ROWS = 256 * int(re.search(r"constexpr int kPlaneCountRows = (\d+);", _OPS_H).group(1))


def _mix64(x):
    x &= MASK
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def _brute(xyz, planes, hypotheses, tol, min_inliers, seed=0, normals=None, normal_min_cos=0.0, axis=(0, 0, 0), axis_min_cos=0.0):
    """The contract applied literally, row by row in numpy scalars and Python integers -> (plane, plane_count, hypothesis, label,
    dropped)."""
    pts = [tuple(f32(a) for a in p) for p in np.asarray(xyz, f32).reshape(-1, 3)]
    nrm = None if normals is None else [tuple(f32(a) for a in p) for p in np.asarray(normals, f32).reshape(-1, 3)]
    ax = tuple(f32(a) for a in axis)
    tol, ncos, acos = f32(tol), f32(normal_min_cos), f32(axis_min_cos)
    label = [-1 if all(np.isfinite(a) for a in p) else -2 for p in pts]
    plane, plane_count, hypothesis = np.zeros((planes, 4), f32), np.zeros(planes + 1, np.int32), np.full(planes, -1, np.int32)
    with np.errstate(all="ignore"):
        for r in range(planes):
            live = [i for i, l in enumerate(label) if l == -1]
            M = len(live)
            if M < 3:
                break
            best, best_h, best_w = 0, -1, None
            for h in range(hypotheses):
                rows = [live[_mix64((seed << 32) | (r << 28) | (h << 2) | j) % M] for j in range(3)]
                if len(set(rows)) < 3:
                    continue
                p0, p1, p2 = (pts[i] for i in rows)
                e1 = tuple(b - a for a, b in zip(p0, p1))
                e2 = tuple(b - a for a, b in zip(p0, p2))
                nx = e1[1] * e2[2] - e1[2] * e2[1]
                ny = e1[2] * e2[0] - e1[0] * e2[2]
                nz = e1[0] * e2[1] - e1[1] * e2[0]
                len2 = (nx * nx + ny * ny) + nz * nz
                if not np.isfinite(len2) or not len2 > f32(1e-30):
                    continue
                s = np.sqrt(len2)
                nx, ny, nz = nx / s, ny / s, nz / s
                d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
                if d < 0 or (d == 0 and next((c for c in (nx, ny, nz) if c != 0), f32(0)) < 0):
                    nx, ny, nz, d = -nx, -ny, -nz, -d
                if acos > 0 and not abs((nx * ax[0] + ny * ax[1]) + nz * ax[2]) >= acos:
                    continue
                count = 0
                for i in live:
                    q = pts[i]
                    inl = abs(((nx * q[0] + ny * q[1]) + nz * q[2]) + d) <= tol
                    if inl and ncos > 0:
                        inl = abs((nx * nrm[i][0] + ny * nrm[i][1]) + nz * nrm[i][2]) >= ncos
                    count += bool(inl)
                if count > best:
                    best, best_h, best_w = count, h, (nx, ny, nz, d)
            if best < min_inliers:
                break
            plane[r], plane_count[r], hypothesis[r], plane_count[planes] = best_w, best, best_h, r + 1
            nx, ny, nz, d = best_w
            for i in live:
                q = pts[i]
                inl = abs(((nx * q[0] + ny * q[1]) + nz * q[2]) + d) <= tol
                if inl and ncos > 0:
                    inl = abs((nx * nrm[i][0] + ny * nrm[i][1]) + nz * nrm[i][2]) >= ncos
                if inl:
                    label[i] = r
    return plane, plane_count, hypothesis, np.array(label, np.int32).reshape(-1), sum(l == -2 for l in label)


def _same_planes(r, want, what=""):
    plane, plane_count, hypothesis, label, dropped = want
    assert np.array_equal(_bits(r.plane), _bits(plane)), (what, r.plane, plane)
    assert np.array_equal(r.plane_count, plane_count), (what, r.plane_count, plane_count)
    assert np.array_equal(r.hypothesis, hypothesis), what
    assert np.array_equal(r.label, label), what
    assert r.dropped == dropped, what


def _scene(n_planes, per_plane, clutter, seed, noise=0.002):
    """noisy planes in general position in front of the origin plus uniform clutter, shuffled -> (xyz f32 [N,3], normals f32 [N,3])"""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for k in range(n_planes):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = np.cross(n, [1.0, 0.3, 0.1])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        c = n * (1.5 + k)
        ab = rng.uniform(-1, 1, (per_plane, 2))
        pts.append(c + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0, noise, (per_plane, 1)) * n)
        nrm.append(np.repeat(n[None], per_plane, 0) + rng.normal(0, 0.02, (per_plane, 3)))
    pts.append(rng.uniform(-2, 4, (clutter, 3)))
    nrm.append(rng.normal(size=(clutter, 3)))
    order = rng.permutation(n_planes * per_plane + clutter)
    return np.concatenate(pts)[order].astype(f32), np.concatenate(nrm)[order].astype(f32)


def _lattice(side, z=0.0):
    g = np.arange(side, dtype=f32)
    x, y = np.meshgrid(g, g)
    return np.stack([x.ravel(), y.ravel(), np.full(side * side, z, f32)], 1).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_plane_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    body = header[header.index("typedef struct md_points_planes {"):header.index("} md_points_planes;")]
    assert re.findall(r"^\s+[a-z0-9_]+\*? (?:\*)?([a-z_]+)(?:\[3\])?;", body, re.M) == FIELDS
    assert [n for n, _ in _lib.MdPointsPlanes._fields_] == FIELDS
    # the model entry takes the widest entry's arguments with the plane part in front of out_kind
    smooth, planes = _lib.SYMBOLS["md_infer_points_smooth"][1], _lib.SYMBOLS["md_infer_points_planes"][1]
    assert planes[:-2] == smooth[:-2] + [C.POINTER(_lib.MdPointsPlanes)] and planes[-2:] == smooth[-2:]


@pytest.mark.parametrize("hyp", (1, 7, 64))
@pytest.mark.parametrize("planes", (1, 2, 3))
def test_reference_against_brute_force(planes, hyp):
    for n_planes, per, clutter, seed in ((2, 15, 10, 0), (3, 40, 30, 1), (3, 90, 30, 2)):
        xyz, _ = _scene(n_planes, per, clutter, seed)
        kw = dict(planes=planes, hypotheses=hyp, tol=0.01, min_inliers=5, seed=seed + 11)
        _same_planes(P.fit_planes(xyz, **kw), _brute(xyz, **kw), (n_planes, per, seed))


def test_reference_finds_the_planes_of_a_scene():
    xyz, _ = _scene(3, 90, 30, 5)
    r = P.fit_planes(xyz, planes=3, hypotheses=64, tol=0.01, min_inliers=30, seed=3)
    assert r.plane_count[3] == 3 and (r.plane_count[:3] >= 85).all() and sorted(set(r.label.tolist())) == [-1, 0, 1, 2]
    assert np.allclose(np.linalg.norm(r.plane[:, :3], axis=1), 1, atol=1e-6) and (r.plane[:, 3] > 0).all()  # unit, facing the origin


def test_tolerance_is_inclusive_and_one_ulp_beyond_is_out():
    tol = f32(0.3)
    base = _lattice(4)
    for z, want in ((tol, 0), (np.nextafter(tol, f32(1)), -1), (-tol, 0), (np.nextafter(-tol, f32(-1)), -1)):
        xyz = np.concatenate([base, [[0.5, 0.5, z]]]).astype(f32)
        kw = dict(planes=1, hypotheses=256, tol=tol, min_inliers=16, seed=0)
        r = P.fit_planes(xyz, **kw)
        _same_planes(r, _brute(xyz, **kw), z)
        # seed 0 draws a lattice triple first among the valid ones: n = (0,0,+-1), d = 0 exactly, so |z| against tol decides the row
        assert _bits(np.abs(r.plane[0])).tolist() == _bits(f32([0, 0, 1, 0])).tolist(), z
        assert r.label[-1] == want and r.plane_count[0] == 16 + (want == 0), z
    # the decision at the off-lattice row, with a seed whose winner is a lattice triple
    for seed in range(8):
        xyz = np.concatenate([base, [[0.5, 0.5, tol]], [[0.5, 1.5, np.nextafter(tol, f32(1))]]]).astype(f32)
        r = P.fit_planes(xyz, planes=1, hypotheses=8, tol=tol, min_inliers=16, seed=seed)
        if r.plane_count[0] == 17 and r.plane[0, 2] == 1 and r.plane[0, 3] == 0:
            assert r.label[-2] == 0 and r.label[-1] == -1
            break
    else:
        raise AssertionError("no seed drew a lattice triple")


def test_coplanar_rows_tie_and_the_smallest_valid_hypothesis_wins():
    xyz = _lattice(5)
    for seed in range(6):
        kw = dict(planes=1, hypotheses=32, tol=0.001, min_inliers=25, seed=seed)
        r = P.fit_planes(xyz, **kw)
        b = _brute(xyz, **kw)
        _same_planes(r, b, seed)
        assert r.plane_count.tolist() == [25, 1] and (r.label == 0).all()
        # the hypotheses in front of the winner are invalid: a repeated row or a collinear triple
        for h in range(r.hypothesis[0]):
            rows = [_mix64((seed << 32) | (h << 2) | j) % 25 for j in range(3)]
            p0, p1, p2 = (xyz[i].astype(np.float64) for i in rows)
            assert len(set(rows)) < 3 or not np.cross(p1 - p0, p2 - p0).any(), (seed, h)


def test_orientation_faces_the_origin_and_the_zero_offset_rule():
    r = P.fit_planes(_lattice(4, -2.0), planes=1, hypotheses=16, tol=0.01, min_inliers=16, seed=1)
    assert r.plane[0].tolist() == [0, 0, 1, 2]  # as values: the sign of a zero component follows the triple drawn
    r = P.fit_planes(_lattice(4, 2.0), planes=1, hypotheses=16, tol=0.01, min_inliers=16, seed=1)
    assert r.plane[0].tolist() == [0, 0, -1, 2]
    # d == 0: the first non-zero component of n is positive, whichever way round the triple is drawn
    for seed in range(6):
        r = P.fit_planes(_lattice(4), planes=1, hypotheses=16, tol=0.01, min_inliers=16, seed=seed)
        assert r.plane[0, 2] == 1 and r.plane[0, 3] == 0, (seed, r.plane)
    # ... on the other axes too: the plane x = 0, y = 0
    for perm in ((2, 0, 1), (0, 2, 1)):
        xyz = np.ascontiguousarray(_lattice(4)[:, perm])
        for seed in range(4):
            kw = dict(planes=1, hypotheses=16, tol=0.01, min_inliers=16, seed=seed)
            r = P.fit_planes(xyz, **kw)
            _same_planes(r, _brute(xyz, **kw))
            n = r.plane[0, :3]
            assert n[np.nonzero(n)[0][0]] == 1 and r.plane[0, 3] == 0


def test_degenerate_triples_never_win_and_rows_that_are_not_finite_are_dropped():
    line = np.stack([np.arange(30, dtype=f32), 2 * np.arange(30, dtype=f32), np.zeros(30, f32)], 1)  # collinear: every triple
    r = P.fit_planes(line, planes=2, hypotheses=64, tol=0.5, min_inliers=3, seed=0)
    assert r.plane_count.tolist() == [0, 0, 0] and r.hypothesis.tolist() == [-1, -1] and not r.plane.any() and (r.label == -1).all()
    same = np.ones((20, 3), f32)  # equal coordinates on different rows: a zero cross product
    assert P.fit_planes(same, planes=1, hypotheses=64, tol=0.5, min_inliers=3).plane_count.tolist() == [0, 0]
    three = _lattice(2)[:3]  # M = 3: most triples repeat a row, the valid ones are the plane
    kw = dict(planes=1, hypotheses=64, tol=0.01, min_inliers=3, seed=2)
    _same_planes(P.fit_planes(three, **kw), _brute(three, **kw))
    assert P.fit_planes(three, **kw).plane_count.tolist() == [3, 1]
    xyz = np.concatenate([_lattice(4), [[np.nan, 0, 0]]]).astype(f32)
    kw = dict(planes=1, hypotheses=32, tol=0.01, min_inliers=16, seed=0)
    r = P.fit_planes(xyz, **kw)
    _same_planes(r, _brute(xyz, **kw))
    assert r.label[-1] == -2 and r.dropped == 1 and r.plane_count.tolist() == [16, 1]
    for n in (0, 1, 2):
        r = P.fit_planes(_lattice(2)[:n], planes=2, hypotheses=8, tol=0.1, min_inliers=3)
        assert r.plane_count.tolist() == [0, 0, 0] and r.label.tolist() == [-1] * n and r.dropped == 0


def test_a_failed_round_ends_the_call():
    xyz, _ = _scene(1, 60, 12, 7)
    kw = dict(planes=3, hypotheses=64, tol=0.01, min_inliers=20, seed=4)
    r = P.fit_planes(xyz, **kw)
    _same_planes(r, _brute(xyz, **kw))
    assert r.plane_count[3] == 1 and r.plane_count[1:3].tolist() == [0, 0] and r.hypothesis[1:].tolist() == [-1, -1]
    assert r.plane[0].any() and not r.plane[1:].any() and set(r.label.tolist()) == {-1, 0}


def test_the_normals_and_the_axis_predicate_each_change_the_winner():
    # a large plane z = 2 whose rows carry normals along x, a smaller one x = 1.5 with matching normals
    big, small = _lattice(8, 2.0), np.ascontiguousarray(_lattice(5)[:, (2, 0, 1)] + f32([1.5, 0, 0]))
    xyz = np.concatenate([big, small]).astype(f32)
    nrm = np.tile(f32([1, 0, 0]), (len(xyz), 1))
    kw = dict(planes=1, hypotheses=256, tol=0.01, min_inliers=10, seed=0)
    plain = P.fit_planes(xyz, **kw)
    assert plain.plane_count[0] == 64 + 5 and abs(plain.plane[0, 2]) == 1  # and the five rows of the small plane at z = 2
    with_n = P.fit_planes(xyz, normals=nrm, normal_min_cos=0.9, **kw)
    _same_planes(with_n, _brute(xyz, normals=nrm, normal_min_cos=0.9, **kw))
    assert with_n.plane_count[0] == 25 and abs(with_n.plane[0, 0]) == 1
    zero = P.fit_planes(xyz, normals=np.zeros_like(nrm), normal_min_cos=0.5, **kw)  # an all-zero normal fails
    assert zero.plane_count.tolist() == [0, 0]
    with_a = P.fit_planes(xyz, axis=(1, 0, 0), axis_min_cos=0.9, **kw)
    _same_planes(with_a, _brute(xyz, axis=(1, 0, 0), axis_min_cos=0.9, **kw))
    assert with_a.plane_count[0] == 25 and abs(with_a.plane[0, 0]) == 1 and with_a.hypothesis[0] != plain.hypothesis[0]


def test_modes_and_the_seed():
    """pipeline.fit_planes has no capacity (as radius_outliers has none): it returns every survivor. A capacity below the
    survivors is the first `capacity` rows of that, which the last assertion of the mode loop states; the device side of it,
    with the memory behind the rows untouched, is test_operator_modes_carry_the_rows_and_respect_the_capacity."""
    xyz, nrm = _scene(2, 50, 25, 9)
    rng = np.random.default_rng(0)
    conf, rgb = rng.random(len(xyz)).astype(f32), rng.integers(0, 256, (len(xyz), 3), dtype=np.uint8)
    kw = dict(planes=2, hypotheses=64, tol=0.01, min_inliers=20, seed=5)
    lab = P.fit_planes(xyz, **kw)
    assert lab.xyz is None and lab.index is None and lab.plane_count[2] == 2
    for mode, keep in ((1, lab.label == -1), ("keep", lab.label >= 0)):
        r = P.fit_planes(xyz, mode=mode, conf=conf, rgb=rgb, normals=nrm, counts=[40, 85], **kw)
        idx = np.nonzero(keep)[0]
        assert np.array_equal(r.index, idx) and np.array_equal(r.label, lab.label)
        assert r.count.tolist() == [int((idx < 40).sum()), int((idx >= 40).sum()), len(idx)]
        assert np.array_equal(_bits(r.xyz), _bits(xyz[idx])) and np.array_equal(_bits(r.conf), _bits(conf[idx]))
        assert np.array_equal(r.rgb, rgb[idx]) and np.array_equal(_bits(r.normals), _bits(nrm[idx]))
        cap = len(idx) // 2  # below the survivors: the count stays the total, the rows are the first `cap` survivors in input order
        assert 0 < cap < r.count[-1] and np.array_equal(r.index[:cap], idx[:cap]) and np.array_equal(_bits(r.xyz[:cap]), _bits(xyz[idx[:cap]]))
    other = P.fit_planes(xyz, **dict(kw, seed=6))
    _same_planes(other, _brute(xyz, **dict(kw, seed=6)))
    assert other.hypothesis.tolist() != lab.hypothesis.tolist() or not np.array_equal(_bits(other.plane), _bits(lab.plane))
    assert other.plane_count[2] == 2 and abs(int(other.plane_count[0]) - int(lab.plane_count[0])) <= 10  # the same planes, other samples
    for bad in (dict(planes=0), dict(planes=9), dict(hypotheses=0), dict(hypotheses=4097), dict(tol=0.0), dict(tol=np.inf), dict(min_inliers=2),
                dict(normal_min_cos=0.5), dict(axis_min_cos=0.5, axis=(np.nan, 0, 0)), dict(axis_min_cos=1.5), dict(mode=3)):
        with pytest.raises(ValueError):
            P.fit_planes(xyz, **dict(kw, **bad))


def test_ply_label_column_is_optional(tmp_path):
    xyz = _lattice(3)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    P.write_ply(a, xyz)
    P.write_ply(b, xyz, label=None)
    assert open(a, "rb").read() == open(b, "rb").read() and b"label" not in open(a, "rb").read() and P.read_ply_label(a) is None
    label = np.arange(9, dtype=np.int32) - 2
    P.write_ply(b, xyz, rgb=np.zeros((9, 3), np.uint8), label=label)
    assert np.array_equal(P.read_ply_label(b), label) and np.array_equal(_bits(P.read_ply(b)[0]), _bits(xyz))


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the operator against pipeline.fit_planes
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(getattr(pc, k)) for k in ("xyz", "conf", "rgb", "normals", "index", "count")}
    d.update({k: g(getattr(pc.planes, k)) for k in ("plane", "plane_count", "hypothesis", "label", "dropped")})
    return d


def _same_as_host(got, want, n, what=""):
    """got: _np of the operator's cloud; want: HostPlanes; n: the rows of the input"""
    assert np.array_equal(got["plane"].view(np.uint32), _bits(want.plane)), (what, got["plane"], want.plane)
    assert np.array_equal(got["plane_count"], want.plane_count), (what, got["plane_count"], want.plane_count)
    assert np.array_equal(got["hypothesis"], want.hypothesis), what
    assert np.array_equal(got["label"][:n], want.label[:n]), what
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


@pytest.fixture(scope="module")
def big_scene():
    """2 * 4096 + 5 rows: three planes and clutter, with three rows that are not finite; computed once, never written"""
    xyz, nrm = _scene(3, 2200, 2 * 4096 + 5 - 6600, 21)
    xyz[[5, 4100, 8000]] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    xyz.setflags(write=False)
    nrm.setflags(write=False)
    return xyz, nrm


@pytest.mark.gpu
@pytest.mark.parametrize("n", (0, 1, 3, 2047, 2048, 2049, 4095, 4096, 4097, 2 * 4096 + 5))
def test_operator_matches_the_reference_at_the_tile_seams(dev, big_scene, n):
    """one tile of the ballot layout is 4096 rows, one pass of a count workgroup COUNT_ROWS; with three planes the later rounds
    run on a live index shorter than the list"""
    from burn_depth_amd import ops
    assert {COUNT_ROWS - 1, COUNT_ROWS, COUNT_ROWS + 1} <= {2047, 2048, 2049}  # the sizes below straddle one pass
    xyz = big_scene[0][:n]
    kw = dict(planes=3, hypotheses=65, tol=0.01, min_inliers=3 if n < 100 else 50, seed=n)
    got = _np(ops.fit_planes(dev, _t(xyz), **kw))
    _same_as_host(got, P.fit_planes(xyz, **kw), n, n)
    if n > 4000:
        assert got["plane_count"][3] == 3  # the scene's planes are found: every round ran on the device


@pytest.mark.gpu
@pytest.mark.parametrize("hyp", (1, 3, 4, 5, 63, 64, 65, 255, 256, 257))
def test_operator_matches_the_reference_around_the_hypothesis_chunks(dev, big_scene, hyp):
    """COUNT_CHUNK hypotheses per trip and a tail loop; 64 a wave of the hypothesis kernel; 256 its workgroup and the stride of the
    count kernel's LDS counters and of the winner's arg-max"""
    from burn_depth_amd import ops
    assert {COUNT_CHUNK - 1, COUNT_CHUNK, COUNT_CHUNK + 1} <= {1, 3, 4, 5, 63, 64, 65, 255, 256, 257}  # the sizes straddle one trip
    xyz = big_scene[0][:4097]
    kw = dict(planes=2, hypotheses=hyp, tol=0.01, min_inliers=30, seed=1000 + hyp)
    _same_as_host(_np(ops.fit_planes(dev, _t(xyz), **kw)), P.fit_planes(xyz, **kw), len(xyz), hyp)


@pytest.mark.gpu
@pytest.mark.parametrize("planes", (1, 3, 8))
@pytest.mark.parametrize("form", ("plain", "normals", "axis", "both"))
def test_operator_planes_and_predicates(dev, big_scene, planes, form):
    from burn_depth_amd import ops
    xyz, nrm = big_scene[0][:5000], big_scene[1][:5000]
    kw = dict(planes=planes, hypotheses=64, tol=0.01, min_inliers=40, seed=planes)
    if form in ("normals", "both"):
        kw.update(normal_min_cos=0.9)
    if form in ("axis", "both"):
        first = P.fit_planes(xyz, planes=1, hypotheses=64, tol=0.01, min_inliers=40, seed=0).plane[0, :3]
        kw.update(axis=tuple(float(a) for a in first), axis_min_cos=0.7)
    want = P.fit_planes(xyz, normals=nrm, **kw)
    assert want.plane_count[planes] >= 1
    _same_as_host(_np(ops.fit_planes(dev, _t(xyz), normals=_t(nrm), **kw)), want, len(xyz), (planes, form))


@pytest.mark.gpu
def test_operator_lattice_cases_are_exact(dev):
    from burn_depth_amd import ops
    tol = f32(0.3)
    xyz = np.concatenate([_lattice(4), [[0.5, 0.5, tol]], [[0.5, 1.5, np.nextafter(tol, f32(1))]], [[np.nan, 1, 1]]]).astype(f32)
    for seed in range(8):
        kw = dict(planes=2, hypotheses=8, tol=float(tol), min_inliers=16, seed=seed)
        _same_as_host(_np(ops.fit_planes(dev, _t(xyz), **kw)), P.fit_planes(xyz, **kw), len(xyz), seed)
    for z in (-2.0, 0.0, 2.0):
        kw = dict(planes=1, hypotheses=16, tol=0.01, min_inliers=16, seed=1)
        _same_as_host(_np(ops.fit_planes(dev, _t(_lattice(4, z)), **kw)), P.fit_planes(_lattice(4, z), **kw), 16, z)
    line = np.stack([np.arange(30, dtype=f32), 2 * np.arange(30, dtype=f32), np.zeros(30, f32)], 1)
    kw = dict(planes=2, hypotheses=64, tol=0.5, min_inliers=3)
    got = _np(ops.fit_planes(dev, _t(line), **kw))
    _same_as_host(got, P.fit_planes(line, **kw), 30, "collinear")
    assert got["plane_count"].tolist() == [0, 0, 0] and got["hypothesis"].tolist() == [-1, -1] and not got["plane"].any()


@pytest.mark.gpu
def test_operator_modes_carry_the_rows_and_respect_the_capacity(dev, big_scene):
    from burn_depth_amd import ops
    xyz, nrm = big_scene
    n = len(xyz)
    rng = np.random.default_rng(3)
    conf, rgb = rng.random(n).astype(f32), rng.integers(0, 256, (n, 3), dtype=np.uint8)
    kw = dict(planes=3, hypotheses=64, tol=0.01, min_inliers=100, seed=2)
    for mode in ("drop", "keep"):
        want = P.fit_planes(xyz, mode=mode, conf=conf, rgb=rgb, normals=nrm, **kw)
        m = len(want.index)
        assert 500 < m < n - 500
        out = ops.fit_planes(dev, _t(xyz), mode=mode, conf=_t(conf), rgb=_t(rgb), normals=_t(nrm), **kw)
        _same_as_host(_np(out), want, n, mode)
        # a capacity below the survivors: the true count, the first rows only, the memory behind them untouched
        cap = m // 2
        out = ops.fit_planes(dev, _t(xyz), mode=mode, conf=_t(conf), normals=_t(nrm), capacity=cap + 7, **kw)
        for t in (out.xyz, out.conf, out.normals):
            t.fill_(POISON)
        out.index.fill_(-7)
        short = type(out)(xyz=out.xyz[:cap], conf=out.conf[:cap], normals=out.normals[:cap], index=out.index[:cap], count=out.count, planes=out.planes)
        got = _np(ops.fit_planes(dev, _t(xyz), mode=mode, conf=_t(conf), normals=_t(nrm), out=short, **kw))
        assert got["count"].tolist() == [m, m] and got["xyz"].shape[0] == cap
        assert np.array_equal(got["xyz"].view(np.uint32), _bits(want.xyz[:cap])) and np.array_equal(got["index"], want.index[:cap])
        torch.cuda.synchronize()
        assert (out.xyz[cap:] == POISON).all() and (out.conf[cap:] == POISON).all() and (out.normals[cap:] == POISON).all()
        assert (out.index[cap:] == -7).all()


@pytest.mark.gpu
def test_operator_second_call_after_a_larger_one_and_refusals(dev, big_scene):
    from burn_depth_amd import ops
    xyz = big_scene[0]
    big = dict(planes=3, hypotheses=257, tol=0.01, min_inliers=100, seed=8)
    small = dict(planes=2, hypotheses=5, tol=0.02, min_inliers=10, seed=9)
    _same_as_host(_np(ops.fit_planes(dev, _t(xyz), **big)), P.fit_planes(xyz, **big), len(xyz), "large")
    _same_as_host(_np(ops.fit_planes(dev, _t(xyz[:300]), **small)), P.fit_planes(xyz[:300], **small), 300, "small behind large")
    _same_as_host(_np(ops.fit_planes(dev, _t(xyz), **big)), P.fit_planes(xyz, **big), len(xyz), "large again")
    x = _t(xyz[:64])
    for bad in (dict(planes=0), dict(planes=9), dict(hypotheses=0), dict(hypotheses=4097), dict(tol=0.0), dict(tol=float("nan")),
                dict(min_inliers=2), dict(normal_min_cos=0.5), dict(normal_min_cos=-0.1), dict(axis_min_cos=0.5, axis=(float("inf"), 0, 0)),
                dict(axis_min_cos=1.5), dict(mode=3)):
        with pytest.raises(_lib.MdError) as e:
            ops.fit_planes(dev, x, **dict(small, **bad))
        assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
