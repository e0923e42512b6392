"""Voxel thinning of a point list: md_op_voxel_thin and its host reference pipeline.voxel_thin. include/mi_depth.h states the
contract, DESIGN 12.3 the kernels. Selection, not averaging: the output is a subset of the input rows, so every comparison
is bit for bit.

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
NEW_ENTRIES = ("md_op_voxel_thin", "md_infer_points_voxel")
HALF = 1 << 20


def _dict_thin(xyz, voxel, conf=None):
    """The contract once more, point by point with a dictionary: -> (index, weight, dropped)."""
    vs = f32(voxel)
    best, size, dropped = {}, {}, 0
    for i, p in enumerate(np.asarray(xyz, f32)):
        with np.errstate(all="ignore"):
            c = [np.floor(f32(a) / vs) for a in p]
        if not all(np.isfinite(a) for a in p) or not all(-HALF <= a < HALF for a in c):
            dropped += 1
            continue
        key = tuple(int(a) for a in c)
        w = f32(0)
        if conf is not None and np.isfinite(conf[i]) and conf[i] >= 0:
            w = f32(conf[i]) + f32(0)  # -0 + 0 = +0
        size[key] = size.get(key, 0) + 1
        if key not in best or w > best[key][0]:  # strictly larger: among equals the first stays
            best[key] = (w, i)
    win = sorted((i, size[k]) for k, (_, i) in best.items())
    return np.array([i for i, _ in win], np.int32), np.array([n for _, n in win], np.int32), dropped


def _check_against_dict(xyz, voxel, conf=None):
    r = P.voxel_thin(xyz, voxel, conf)
    index, weight, dropped = _dict_thin(xyz, voxel, conf)
    assert np.array_equal(r.index, index) and np.array_equal(r.weight, weight) and r.dropped == dropped
    assert r.count.tolist() == [len(index), len(index)]
    assert np.array_equal(_bits(r.xyz), _bits(np.asarray(xyz, f32)[index]))
    if conf is not None:
        assert np.array_equal(_bits(r.conf), _bits(np.asarray(conf, f32)[index]))
    assert r.weight.sum() + r.dropped == len(xyz)
    return r


def _cloud(n, side, seed, spread=1.0):
    """n points uniform in a cube of `side`^3 voxels of size 0.25 around the origin, distinct confidences in (0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-side / 2, side / 2, (n, 3)) * 0.25 * spread).astype(f32)
    conf = (0.5 + rng.permutation(n) / n).astype(f32)
    return xyz, conf


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_voxel_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "} md_points_voxel;" in header
    assert [n for n, _ in _lib.MdPointsVoxel._fields_] == ["voxel", "index", "weight", "dropped"]


def test_reference_against_the_dictionary_restatement():
    for n, side, seed in ((1, 4, 0), (300, 4, 1), (2000, 8, 2), (500, 64, 3)):
        xyz, conf = _cloud(n, side, seed)
        r = _check_against_dict(xyz, 0.25, conf)
        _check_against_dict(xyz, 0.25)  # no confidence: the first point of every voxel
        assert len(r.index) <= min(n, side ** 3) and (np.diff(r.index) > 0).all()
    # without a confidence row the survivor of a voxel is its first point
    xyz, _ = _cloud(400, 3, 4)
    r = P.voxel_thin(xyz, 0.25)
    seen = {}
    for i, p in enumerate(xyz):
        seen.setdefault(tuple(np.floor(p / f32(0.25)).astype(int)), i)
    assert sorted(seen.values()) == r.index.tolist()
    assert P.voxel_thin(np.zeros((0, 3), f32), 1.0).count.tolist() == [0, 0]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.voxel_thin(xyz, bad)


def test_reference_ties_and_odd_confidences():
    rng = np.random.default_rng(5)
    xyz = (rng.uniform(-0.5, 0.5, (600, 3))).astype(f32)  # 4^3 voxels of 0.25: about 9 points each
    # ties: three confidence levels only
    conf = rng.choice(np.array([0.25, 0.5, 0.75], f32), 600)
    r = _check_against_dict(xyz, 0.25, conf)
    assert (r.conf == f32(0.75)).mean() > 0.9
    # -0.0, NaN, inf and negative confidences all rank as 0: among themselves the first wins, any positive beats them
    odd = np.array([-0.0, np.nan, np.inf, -np.inf, -1.0, 0.0], f32)
    conf = odd[rng.integers(0, len(odd), 600)]
    r = _check_against_dict(xyz, 0.25, conf)
    assert np.array_equal(r.index, P.voxel_thin(xyz, 0.25).index)  # every weight is 0: the order alone decides
    conf[rng.permutation(600)[:100]] = f32(1e-30)
    _check_against_dict(xyz, 0.25, conf)
    one = np.zeros((4, 3), f32)
    assert P.voxel_thin(one, 1.0, np.array([-0.0, 0.0, -0.0, 0.0], f32)).index.tolist() == [0]
    assert P.voxel_thin(one, 1.0, np.array([np.nan, -2.0, 1e-38, 0.0], f32)).index.tolist() == [2]
    assert P.voxel_thin(one, 1.0, np.array([np.inf, 3.0, 3.0, 1.0], f32)).index.tolist() == [1]  # inf is not finite: weight 0


def test_reference_cell_faces_negative_coordinates_and_the_range():
    v = f32(0.375)
    ks = np.arange(-5, 6)
    faces = np.array([[k * v, -k * v, 0.0] for k in ks] + [[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]], f32)
    r = _check_against_dict(faces, v)
    cells = np.floor(faces / v).astype(int)
    assert np.array_equal(cells[:len(ks), 0], ks) and np.array_equal(cells[:len(ks), 1], -ks)  # k v lies in cell k, -k v in cell -k
    assert r.index.tolist() == list(range(len(ks)))  # -0.0 and 0.0 share cell (0, 0, 0) with k = 0
    assert r.weight[5] == 3
    # just below a face
    below = np.nextafter(faces[:len(ks)], f32(-np.inf)).astype(f32)
    _check_against_dict(np.concatenate([faces, below]), v)
    # a negative coordinate goes down: -0.1 / 1 lies in cell -1
    assert P.voxel_thin(np.array([[-0.1, 0, 0], [-0.9, 0, 0], [0.1, 0, 0]], f32), 1.0).weight.tolist() == [2, 1]
    # the range: cells -2^20 .. 2^20 - 1 are in, the next ones and non-finite points are out
    edge = np.array([[-HALF, 0, 0], [HALF - 1, 0, 0], [0, HALF - 0.5, -HALF], [HALF, 0, 0], [-HALF - 1, 0, 0], [0, 0, 3e38], [np.nan, 0, 0],
                     [0, np.inf, 0], [0, 0, -np.inf], [1, 2, 3]], f32)
    r = _check_against_dict(edge, 1.0)
    assert r.index.tolist() == [0, 1, 2, 9] and r.dropped == 6
    r = _check_against_dict(edge, 1e-3)  # p / voxel overflows the grid for all but the origin-near rows
    assert r.dropped == 9
    _check_against_dict(np.array([[3e38, 0, 0], [1, 1, 1]], f32), 1e-3)  # the quotient overflows to inf


def test_reference_per_view_counts():
    xyz, conf = _cloud(900, 6, 6)
    r = P.voxel_thin(xyz, 0.25, conf, counts=[200, 0, 450, 250])
    b = np.array([0, 200, 200, 650, 900])
    assert r.count.tolist() == [int(((r.index >= b[i]) & (r.index < b[i + 1])).sum()) for i in range(4)] + [len(r.index)]
    assert r.count[1] == 0


def test_voxel_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched: with a null device the valid call is refused last, for the device."""
    buf = (C.c_float * 64)()
    px = C.cast(buf, C.c_void_p)
    listed = _lib.MdPointsOutputs(None, None, px.value, None, None, px.value, 4, None)
    no_count = _lib.MdPointsOutputs(None, None, None, None, None, None, 4, None)

    def why(vox, out=listed, N=4, code=_lib.MD_ERR_INVALID_ARG, conf=None, normals_out=None):
        rc = lib.md_op_voxel_thin(None, px, conf, None, None, N, C.byref(vox) if vox else None, C.byref(out), normals_out, None)
        assert rc == code, rc
        return lib.md_last_error().decode()

    for bad in (float("nan"), float("inf"), -0.5, 0.0):
        assert "voxel" in why(_lib.MdPointsVoxel(bad, None, None, None)), bad
    assert "need `count`" in why(_lib.MdPointsVoxel(0.5, px.value, None, None), no_count)
    assert "need `count`" in why(_lib.MdPointsVoxel(0.5, None, px.value, None), no_count)
    assert "negative" in why(_lib.MdPointsVoxel(0.5, None, None, None), N=-1)
    assert "2^30" in why(_lib.MdPointsVoxel(0.5, None, None, None), N=1 << 30, code=_lib.MD_ERR_SHAPE)
    assert "confidence row" in why(_lib.MdPointsVoxel(0.5, None, None, None), _lib.MdPointsOutputs(None, None, px.value, None, px.value, px.value, 4, None))
    assert "normals row" in why(_lib.MdPointsVoxel(0.5, None, None, None), normals_out=px)
    assert "dense" in why(_lib.MdPointsVoxel(0.5, None, None, None), _lib.MdPointsOutputs(px.value, None, px.value, None, None, px.value, 4, None))
    assert "options are null" in why(None)
    assert "device is null" in why(_lib.MdPointsVoxel(0.5, px.value, px.value, px.value))
    # the model call: voxel and its outputs are checked with the other arguments (here: refused for the null model first)
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    vox = _lib.MdPointsVoxel(-1.0, None, None, None)
    assert lib.md_infer_points_voxel(None, px, 1, 2, 2, 1, None, None, None, C.byref(o), C.byref(listed), None, C.byref(vox), 1, None) == _lib.MD_ERR_INVALID_ARG
    assert "model is null" in lib.md_last_error().decode()
    assert (np.frombuffer(buf, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
POISON = 123456.0
CANARY = 16  # elements behind the end of every output buffer
FILLS = dict(xyz=POISON, conf=POISON, rgb=77, normals=POISON, index=-7, weight=-7, count=-5, dropped=-5)


def _fresh(cap, conf, rgb, normals):
    from burn_depth_amd.depth_pro import PointCloud
    out, stores = PointCloud(), {}

    def put(name, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        stores[name] = torch.full((n + CANARY,), FILLS[name], dtype=dtype, device="cuda")
        setattr(out, name, stores[name][:n].view(shape))

    put("xyz", (cap, 3))
    put("index", (cap,), torch.int32)
    put("weight", (cap,), torch.int32)
    put("count", (2,), torch.int32)
    put("dropped", (1,), torch.int32)
    if conf:
        put("conf", (cap,))
    if rgb:
        put("rgb", (cap, 3), torch.uint8)
    if normals:
        put("normals", (cap, 3))
    return out, stores


def _run(dev, xyz, voxel, conf=None, rgb=None, normals=None, capacity=None):
    """ops.voxel_thin on poisoned, guarded outputs -> numpy dict"""
    from burn_depth_amd import ops
    cap = len(xyz) if capacity is None else capacity
    out, stores = _fresh(cap, conf is not None, rgb is not None, normals is not None)
    ops.voxel_thin(dev, _t(xyz), voxel, conf=_t(conf), rgb=_t(rgb), normals=_t(normals), out=out)
    torch.cuda.synchronize()
    for name, store in stores.items():
        assert (store[-CANARY:] == FILLS[name]).all(), name
    return {k: v.cpu().numpy() for k, v in vars(out).items() if v is not None}


def _assert_same(got, ref, what=""):
    assert got["count"].tolist() == [int(ref.count[-1])] * 2, (what, got["count"], ref.count)
    assert int(got["dropped"][0]) == ref.dropped, what
    cap = got["xyz"].shape[0]
    n = min(int(ref.count[-1]), cap)
    for k in ("xyz", "conf", "normals"):
        if k in got:
            assert np.array_equal(_bits(got[k][:n]), _bits(getattr(ref, k)[:n])), (what, k)
            assert (got[k][n:] == f32(POISON)).all(), (what, k)  # the rows behind the survivors stay untouched
    if "rgb" in got:
        assert np.array_equal(got["rgb"][:n], ref.rgb[:n]) and (got["rgb"][n:] == 77).all(), what
    for k in ("index", "weight"):
        assert np.array_equal(got[k][:n], getattr(ref, k)[:n]) and (got[k][n:] == -7).all(), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097])
def test_wave_and_workgroup_edges_are_bit_identical_to_the_host_reference(dev, n):
    xyz, conf = _cloud(n, 12, 20 + n)  # up to 1728 voxels: duplicates and singletons at every size
    rng = np.random.default_rng(n)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(f32)
    ref = P.voxel_thin(xyz, 0.25, conf, rgb, nrm)
    assert 0 < ref.count[-1] <= n
    _assert_same(_run(dev, xyz, 0.25, conf, rgb, nrm), ref, n)


@pytest.mark.gpu
def test_one_voxel_takes_every_point(dev):
    n = 10000
    rng = np.random.default_rng(1)
    xyz = rng.uniform(0.01, 0.99, (n, 3)).astype(f32)
    conf = (1 + rng.permutation(n)).astype(f32)  # distinct
    got = _run(dev, xyz, 1.0, conf)
    _assert_same(got, P.voxel_thin(xyz, 1.0, conf), "distinct")
    assert got["count"][0] == 1 and got["index"][0] == int(conf.argmax()) and got["weight"][0] == n
    got = _run(dev, xyz, 1.0, np.full(n, 0.5, f32))
    assert got["count"][0] == 1 and got["index"][0] == 0 and got["weight"][0] == n
    assert np.array_equal(_bits(got["xyz"][0]), _bits(xyz[0]))


@pytest.mark.gpu
def test_every_point_in_its_own_voxel_is_the_identity(dev):
    n = 5000
    cells = np.random.default_rng(2).permutation(40 ** 3)[:n]
    xyz = (np.stack([cells % 40, cells // 40 % 40, cells // 1600], 1) - 20 + 0.5).astype(f32) * f32(0.5)
    conf = np.random.default_rng(3).random(n).astype(f32)
    got = _run(dev, xyz, 0.5, conf)
    assert got["count"][0] == n and (got["weight"] == 1).all() and np.array_equal(got["index"], np.arange(n))
    assert np.array_equal(_bits(got["xyz"]), _bits(xyz)) and np.array_equal(_bits(got["conf"]), _bits(conf))
    _assert_same(got, P.voxel_thin(xyz, 0.5, conf))


@pytest.mark.gpu
def test_dense_grid_without_confidence_carries_rgb_and_normals(dev):
    n = 5000
    xyz, conf = _cloud(n, 8, 4)  # 8^3 = 512 voxels: about 10 points each, long probe chains on the 16384-slot table's few keys
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(f32)
    ref = P.voxel_thin(xyz, 0.25, None, rgb, nrm)
    assert 400 < ref.count[-1] <= 512
    got = _run(dev, xyz, 0.25, None, rgb, nrm)
    _assert_same(got, ref, "no conf")
    assert "conf" not in got
    _assert_same(_run(dev, xyz, 0.25, conf, rgb, nrm), P.voxel_thin(xyz, 0.25, conf, rgb, nrm), "conf")
    # ties and odd confidences on the device
    odd = np.array([-0.0, np.nan, np.inf, -1.0, 0.0, 0.5, 0.5], f32)[rng.integers(0, 7, n)]
    _assert_same(_run(dev, xyz, 0.25, odd), P.voxel_thin(xyz, 0.25, odd), "odd")


@pytest.mark.gpu
def test_dropped_points_are_counted_and_faces_land_in_their_cells(dev):
    v = f32(0.375)
    xyz, conf = _cloud(3000, 8, 6)
    rng = np.random.default_rng(7)
    bad = rng.permutation(3000)[:300]
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:200], rng.integers(0, 3, 100)] = np.array([np.inf, -np.inf], f32)[rng.integers(0, 2, 100)]
    xyz[bad[200:], rng.integers(0, 3, 100)] = f32(HALF) * v * f32(1.5)  # beyond the grid
    k = np.arange(-20, 21)
    faces = np.array([[a * v, -a * v, b] for a in k for b in (-0.0, 0.0)], f32)
    xyz = np.concatenate([xyz, faces, np.nextafter(faces, f32(-np.inf)).astype(f32)])
    conf = np.concatenate([conf, np.ones(2 * len(faces), f32)])
    ref = P.voxel_thin(xyz, v, conf)
    assert ref.dropped == 300
    _assert_same(_run(dev, xyz, v, conf), ref)
    edge = np.array([[-HALF, 0, 0], [HALF - 1, 0, 0], [0, HALF - 0.5, -HALF], [HALF, 0, 0], [-HALF - 1, 0, 0], [1, 2, 3]], f32)
    got = _run(dev, edge, 1.0)
    assert got["index"][:4].tolist() == [0, 1, 2, 5] and got["dropped"][0] == 2
    everything = _run(dev, np.full((70, 3), np.nan, f32), 1.0)  # nothing survives
    assert everything["count"].tolist() == [0, 0] and everything["dropped"][0] == 70


@pytest.mark.gpu
def test_capacity_below_the_survivors_keeps_the_true_count(dev):
    xyz, conf = _cloud(9000, 16, 8)
    rgb = np.random.default_rng(9).integers(0, 256, (9000, 3), dtype=np.uint8)
    ref = P.voxel_thin(xyz, 0.25, conf, rgb)
    total = int(ref.count[-1])
    assert total > 3000
    for cap in (total // 2, 1, 0, total - 1):
        got = _run(dev, xyz, 0.25, conf, rgb, capacity=cap)  # _run checks the sentinels behind row `cap`
        assert got["xyz"].shape[0] == cap
        _assert_same(got, ref, cap)


@pytest.mark.gpu
def test_more_tiles_than_scan_threads_with_a_capacity_inside_the_list(dev):
    """256 * 4096 + 1 rows are 257 tiles, one more than the one-workgroup scan has threads: every thread of scan_tile_counts
    (kernels/tile_compact.h) sums and writes a chunk of two tile counts, the branch the cases up to 4097 rows (two tiles) never
    take. About a ninth of the rows survive; half the survivors as capacity ends inside a tile near the middle of the list, so
    that tile takes the per-row capacity check and every tile behind it the early-out. One view: md_op_voxel_thin takes no
    per-view input counts (only the model call has them; test_points_voxel.py checks its three-view counts at its own sizes)."""
    n = 256 * 4096 + 1
    xyz, conf = _cloud(n, 47, 13)  # 48^3 = 110592 cells
    ref = P.voxel_thin(xyz, 0.25, conf)
    total = int(ref.count[-1])
    assert n // 12 < total < n // 8
    _assert_same(_run(dev, xyz, 0.25, conf), ref, "whole")  # the offsets of all 257 tiles
    cap = total // 2
    assert 0 < ref.index[cap] % 4096 and ref.index[cap] // 4096 < 256  # the capacity ends inside a tile, tiles lie behind it
    _assert_same(_run(dev, xyz, 0.25, conf, capacity=cap), ref, "half")


@pytest.mark.gpu
def test_survivor_set_is_invariant_under_a_shuffle_and_runs_repeat(dev):
    xyz, conf = _cloud(8000, 10, 10)  # distinct confidences
    a = _run(dev, xyz, 0.25, conf)
    b = _run(dev, xyz, 0.25, conf)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k  # two runs, the same bits
    perm = np.random.default_rng(11).permutation(8000)
    c = _run(dev, xyz[perm], 0.25, conf[perm])
    n = int(a["count"][0])
    assert c["count"][0] == n
    assert np.array_equal(np.sort(perm[c["index"][:n]]), a["index"][:n])  # the same input points survive
    order = np.argsort(perm[c["index"][:n]])
    assert np.array_equal(c["weight"][:n][order], a["weight"][:n])
    assert np.array_equal(_bits(c["xyz"][:n][order]), _bits(a["xyz"][:n]))


@pytest.mark.gpu
def test_voxel_refusals_leave_the_outputs_untouched(dev):
    from burn_depth_amd import ops
    xyz, conf = _cloud(500, 4, 12)

    def refused(code, voxel=0.25, strip=(), **kw):
        out, stores = _fresh(500, True, False, False)
        for name in strip:
            setattr(out, name, None)
        with pytest.raises(_lib.MdError) as e:
            ops.voxel_thin(dev, _t(xyz), voxel, conf=_t(conf), out=out, **kw)
        assert e.value.code == code
        torch.cuda.synchronize()
        for name, store in stores.items():
            assert (store == FILLS[name]).all(), name

    for bad in (float("nan"), float("inf"), -0.25, 0.0):
        refused(_lib.MD_ERR_INVALID_ARG, voxel=bad)
    refused(_lib.MD_ERR_INVALID_ARG, strip=("count",))  # index / weight / the list without count
    out, _ = _fresh(500, False, False, False)
    out.conf = torch.empty(500, device="cuda")
    with pytest.raises(_lib.MdError) as e:  # a conf output without a confidence row
        ops.voxel_thin(dev, _t(xyz), 0.25, out=out)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    # an empty list is not an error
    got = ops.voxel_thin(dev, torch.empty((0, 3), device="cuda"), 0.25)
    torch.cuda.synchronize()
    assert got.count.tolist() == [0, 0] and got.dropped.item() == 0
