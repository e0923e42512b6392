"""Rigid ICP registration of a point list onto a reference cloud: md_op_register_points against its host reference
pipeline.register_points. include/mi_depth.h states the contract, kernels/register_math.h its arithmetic, DESIGN 12.14 the kernels.
The sums have a fixed tree shape and the solve uses correctly rounded operations only, so every comparison is bit for bit:
transform, pairs, sum_d2, stats, dropped, the moved rows, the rotated normals, nearest and dist2.

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
from points_util import _t, dev, lib  # noqa: E402,F401
from test_register_host import _motion, _move, _surface, cases  # noqa: E402

f32, f64 = np.float32, np.float64
FIELDS = ["radius", "target", "target_rows", "target_kind", "iterations", "min_pairs", "apply", "rot_eps", "trans_eps", "init", "transform",
          "pairs", "sum_d2", "stats", "dropped", "nearest", "dist2"]


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, ref, what, N):
    """the operator's `PointRegistration` holds the reference's bits"""
    g = {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(got).items()}
    assert np.array_equal(g["stats"], ref.stats), (what, g["stats"], ref.stats)
    assert np.array_equal(g["pairs"], ref.pairs), (what, g["pairs"], ref.pairs)
    assert np.array_equal(_u(g["sum_d2"]), _u(ref.sum_d2)), (what, g["sum_d2"], ref.sum_d2)
    assert np.array_equal(_u(g["transform"]), _u(ref.transform)), (what, g["transform"], ref.transform)
    assert int(g["dropped"][0]) == ref.dropped, what
    assert np.array_equal(g["nearest"], ref.nearest), what
    assert np.array_equal(_u(g["dist2"]), _u(ref.dist2)), what
    if g["xyz"] is not None:
        assert np.array_equal(_u(g["xyz"].reshape(N, 3)), _u(ref.xyz)), what
    if g["normals"] is not None:
        assert np.array_equal(_u(g["normals"]), _u(ref.normals)), what


def _both(dev, xyz, target, radius, K, init=None, min_pairs=3, rot_eps=0.0, trans_eps=0.0, normals=None, what=""):
    from burn_depth_amd import ops
    ref = P.register_points(xyz, target, radius, iterations=K, init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps, normals=normals)
    got = ops.register_points(dev, _t(np.asarray(xyz, f32).reshape(-1, 3)), _t(np.asarray(target, f32).reshape(-1, 3)), radius, iterations=K,
                              init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps, normals=_t(normals), apply=True)
    _same(got, ref, what, len(xyz))
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_register_entry(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    assert "md_op_register_points" in declared and hasattr(raw, "md_op_register_points") and "md_op_register_points" in _lib.SYMBOLS
    body = re.search(r"typedef struct md_points_register \{(.*?)\} md_points_register;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == FIELDS == [f[0] for f in _lib.MdPointsRegister._fields_]


def test_register_kernels_compile_without_contraction_and_share_the_grid_header():
    csrc = os.path.join(ROOT, "burn_depth_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    nocontract = re.search(r"^NOCONTRACT = (.*?)\n\$", make, re.S | re.M).group(1)
    assert "kernels/register.hip" in nocontract and "kernels/register.hip" in make.split("OBJS =")[0]
    for name in ("match.hip", "register.hip"):
        assert '#include "match_grid.h"' in open(os.path.join(csrc, "kernels", name)).read()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in cases()])
def test_operator_equals_the_reference_on_the_seeded_cases(dev, name):
    """K = 1 and K = 8, an init away from the identity, early convergence, too few pairs, rows that are NaN, infinite or out of
    range on both lists, duplicate target rows at equal distance, T = 0 and N = 0, a planar cloud."""
    _, xyz, target, radius, K, init, min_pairs, rot_eps, trans_eps = next(c for c in cases() if c[0] == name)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(len(xyz), 3)).astype(f32)
    if len(xyz) > 4:
        normals[1] = [np.nan, 0, 1]
    got, ref = _both(dev, xyz, target, radius, K, init, min_pairs, rot_eps, trans_eps, normals, name)
    if name == "stops early":
        assert ref.stats[1] == 1 and 0 < ref.stats[0] < K and not ref.pairs[ref.stats[0]:K].any() and ref.pairs[K] > 0
    if name == "too few pairs":
        assert ref.stats[1] == 2 and np.array_equal(_u(got.transform.cpu().numpy()), _u(np.asarray(init, f64)))
    if name == "no target":
        assert ref.stats[1] == 2 and ref.stats[4] == 0
    if name == "duplicate targets":
        assert (ref.nearest[:100] == np.arange(100)).all()  # rows 200.. repeat rows 0..200 at equal distance: the smallest row wins


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 257, 4095, 4096, 4097, 2 * 4096 + 1])
@pytest.mark.parametrize("T", [1, 64, 3000])
def test_row_counts_at_the_seams_of_the_tree(dev, N, T):
    A = _motion([1, 2, 3], 2.0, [0.02, -0.01, 0.02])
    src, tgt = _surface(N, 20 + N % 7), _move(A, _surface(max(N, T), 20 + N % 7))[:T]
    for K in (1, 8):
        _both(dev, src, tgt, 0.3, K, what=(N, T, K))


@pytest.mark.gpu
def test_moved_rows_may_overwrite_the_input(dev):
    from burn_depth_amd import ops
    _, xyz, target, radius, K, *_ = next(c for c in cases() if c[0] == "bad rows")
    ref = P.register_points(xyz, target, radius, iterations=K)
    rows = _t(xyz)
    got = ops.register_points(dev, rows, _t(target), radius, iterations=K, xyz_out=rows)
    assert got.xyz.data_ptr() == rows.data_ptr()
    _same(got, ref, "in place", len(xyz))


@pytest.mark.gpu
def test_more_than_256_tiles_fold_in_the_second_level(dev):
    """N = 257 * 4096 + 1 with K = 1 and a small target: thread 0 of the reduce folds tile 0 and tile 256, thread 1 tile 1 and the
    one-row tile 257. Only the first and the last four tiles lie near the target (the others are 50 away and find empty cells),
    which keeps the numpy side cheap; a fold that loses or misplaces a tile beyond 255 still shows."""
    N = 257 * 4096 + 1
    src = np.tile(_surface(4096, 31), (258, 1))[:N].copy()
    src[4 * 4096:254 * 4096] += f32(50)
    tgt = _move(_motion([0, 0, 1], 1.0, [0.01, 0.0, 0.0]), _surface(300, 32))
    got, ref = _both(dev, src, tgt, 0.15, 1, what="258 tiles")
    near = ref.nearest >= 0
    assert near[:4096].any() and near[256 * 4096:257 * 4096].any() and near[257 * 4096] and ref.stats[0] == 1


@pytest.mark.gpu
def test_refusals_before_any_launch(dev, lib):
    xyz, tgt = _t(_surface(10, 1)), _t(_surface(10, 2))
    out = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")

    def call(n=10, xyz_p=xyz.data_ptr(), normals_out=None, **kw):
        f = dict(radius=0.3, target=tgt.data_ptr(), target_rows=10, target_kind=_lib.MD_MEM_DEVICE, iterations=2, min_pairs=3, apply=0, rot_eps=0.0,
                 trans_eps=0.0, init=None, transform=out.data_ptr(), pairs=None, sum_d2=None, stats=None, dropped=None, nearest=None, dist2=None)
        f.update(kw)
        reg = _lib.MdPointsRegister(*[f[k] for k in FIELDS])
        return lib.md_op_register_points(dev.handle, C.c_void_p(xyz_p), None, n, C.byref(reg), None, C.c_void_p(normals_out), None)

    nan12 = (C.c_double * 12)(*([1.0] * 11 + [float("nan")]))
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=1e30), dict(target_rows=-1), dict(target=None),
           dict(target_kind=_lib.MD_MEM_HOST), dict(iterations=0), dict(iterations=65), dict(min_pairs=2), dict(rot_eps=-1e-9),
           dict(trans_eps=float("nan")), dict(rot_eps=float("inf")), dict(init=C.cast(nan12, C.c_void_p)), dict(n=-1), dict(xyz_p=0),
           dict(normals_out=out.data_ptr())]
    for kw in bad:
        assert call(**kw) == _lib.MD_ERR_INVALID_ARG, kw
    assert call(n=1 << 30) == _lib.MD_ERR_SHAPE and call(target_rows=1 << 30) == _lib.MD_ERR_SHAPE
    assert lib.md_op_register_points(dev.handle, C.c_void_p(xyz.data_ptr()), None, 10, None, None, None, None) == _lib.MD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out.cpu() == 7.0).all()  # nothing was launched
    assert call() == _lib.MD_OK
