"""md_op_register_points_plane (point-to-plane ICP against the target's normals, kernels/register.hip) against the host reference
`pipeline.register_points(target_normals=)`, bit for bit in every output. include/mi_depth.h states the contract, DESIGN 12.15
the kernels. The GPU tests run with `-m gpu` on an MI355X; tests/test_register_plane_host.py holds the CPU side."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from burn_depth_amd import _lib  # noqa: E402
from burn_depth_amd import pipeline as P  # noqa: E402
from points_util import _t, dev, lib  # noqa: E402,F401
from test_register_host import _motion, _move  # noqa: E402
from test_register_plane_host import _bumpy, _turn, cases  # noqa: E402
from test_register_points import FIELDS, _same, _u  # noqa: E402

f32, f64 = np.float32, np.float64
PLANE_FIELDS = ["target_normals", "sum_r2"]


def _same_plane(got, ref, what, N):
    _same(got, ref, what, N)
    assert np.array_equal(_u(got.sum_r2.cpu().numpy()), _u(ref.sum_r2)), (what, got.sum_r2, ref.sum_r2)


def _both(dev, xyz, target, tn, radius, K, init=None, min_pairs=6, rot_eps=0.0, trans_eps=0.0, normals=None, what=""):
    from burn_depth_amd import ops
    ref = P.register_points(xyz, target, radius, iterations=K, init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps, normals=normals,
                            target_normals=tn)
    got = ops.register_points(dev, _t(np.asarray(xyz, f32).reshape(-1, 3)), _t(np.asarray(target, f32).reshape(-1, 3)), radius, iterations=K,
                              init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps, normals=_t(normals), apply=True,
                              target_normals=_t(np.asarray(tn, f32).reshape(-1, 3)))
    _same_plane(got, ref, what, len(xyz))
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_plane_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in ("md_op_register_points_plane", "md_infer_points_register_plane"):
        assert name in declared and hasattr(raw, name) and name in _lib.SYMBOLS, name
    body = re.search(r"typedef struct md_points_register_plane \{(.*?)\} md_points_register_plane;", header, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == PLANE_FIELDS == [f[0] for f in _lib.MdPointsRegisterPlane._fields_]
    # the plane part rides behind the register part: the widest entry takes one pointer more
    assert len(_lib.SYMBOLS["md_infer_points_register_plane"][1]) == len(_lib.SYMBOLS["md_infer_points_register"][1]) + 1
    assert len(_lib.SYMBOLS["md_op_register_points_plane"][1]) == len(_lib.SYMBOLS["md_op_register_points"][1]) + 1


def test_plane_kernels_compile_without_contraction_beside_the_point_form():
    csrc = os.path.join(ROOT, "burn_depth_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    nocontract = re.search(r"^NOCONTRACT = (.*?)\n\$", make, re.S | re.M).group(1)
    assert "kernels/register.hip" in nocontract
    src = open(os.path.join(csrc, "kernels", "register.hip")).read()
    for kernel in ("register_plane_step_kernel", "register_plane_reduce_kernel", "register_step_kernel", "register_reduce_kernel"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\(", src), kernel
    math = open(os.path.join(csrc, "kernels", "register_math.h")).read()
    assert "reg_add_plane_leaves" in math and "reg_solve_plane" in math and "reg_add_plane_leaves" in src and "reg_solve_plane" in src
    assert not re.search(r"\bfma\s*\(|__fma_rn|atomicAdd\s*\(\s*\(?\s*(float|double)", src + math)


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in cases()])
def test_operator_equals_the_reference_on_the_seeded_cases(dev, name):
    """The cases of the CPU test: K = 1 and K = 8, an init, early convergence, too few pairs, rows that are NaN, infinite or out
    of range on both lists, NaN / infinite / zero normals, duplicate target rows, one normal direction, T = 1, T = 0 and N = 0."""
    _, xyz, target, tn, radius, K, init, min_pairs, rot_eps, trans_eps = next(c for c in cases() if c[0] == name)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=(len(xyz), 3)).astype(f32)
    if len(xyz) > 4:
        normals[1] = [np.nan, 0, 1]
    got, ref = _both(dev, xyz, target, tn, radius, K, init, min_pairs, rot_eps, trans_eps, normals, name)
    if name == "stops early":
        assert ref.stats[1] == 1 and 0 < ref.stats[0] < K and not ref.sum_r2[ref.stats[0]:K].any() and ref.pairs[K] > 0
    if name == "too few pairs":
        assert ref.stats[1] == 2 and np.array_equal(_u(got.transform.cpu().numpy()), _u(np.asarray(init, f64)))
    if name in ("single direction", "one target row"):
        assert ref.stats[1] == 3 and ref.stats[0] == 0 and not ref.sum_r2[1:K].any() and ref.sum_r2[K] == ref.sum_r2[0]
    if name == "unusable normals":
        assert 6 <= ref.pairs[0] < (ref.nearest >= 0).sum()  # pairs count the usable ones, nearest reports all
    if name == "no target":  # no row of normals either: the address is null, which is the point-to-point entry: status 2 alike
        assert ref.stats[1] == 2 and ref.stats[4] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 257, 4095, 4096, 4097, 2 * 4096 + 1])
@pytest.mark.parametrize("T", [1, 64, 3000])
def test_row_counts_at_the_seams_of_the_tree(dev, N, T):
    """T = 1 with the normal (0,0,1): status 3 on the device from N = 6 rows on, status 2 below"""
    A = _motion([1, 2, 3], 2.0, [0.02, -0.01, 0.02])
    src = _bumpy(N, 20 + N % 7)[0]
    tgt, tgt_n = _bumpy(max(N, T), 20 + N % 7)
    tgt, tgt_n = _move(A, tgt)[:T], _turn(A, tgt_n)[:T]
    if T == 1:
        tgt_n = np.array([[0, 0, 1]], f32)
    for K in (1, 8):
        _, ref = _both(dev, src, tgt, tgt_n, 0.3, K, what=(N, T, K))
        if T == 1 and ref.pairs[0] >= 6:
            assert ref.stats[1] == 3


@pytest.mark.gpu
def test_more_than_256_tiles_fold_in_the_second_level(dev):
    """N = 258 * 4096 + 5 with K = 1 and a small target: the threads 0 and 1 of the reduce fold two tile sums each. Only the
    first and the last four tiles lie near the target (the others are 50 away and find empty cells), which keeps the numpy side
    cheap; a fold that loses or misplaces a tile beyond 255 still shows."""
    N = 258 * 4096 + 5
    src = np.tile(_bumpy(4096, 31)[0], (259, 1))[:N].copy()
    src[4 * 4096:254 * 4096] += f32(50)
    A = _motion([0, 0, 1], 1.0, [0.01, 0.0, 0.0])
    tgt, tgt_n = _bumpy(300, 32)
    got, ref = _both(dev, src, _move(A, tgt), _turn(A, tgt_n), 0.15, 1, what="259 tiles")
    near = ref.nearest >= 0
    assert near[:4096].any() and near[256 * 4096:257 * 4096].any() and near[258 * 4096:].any() and ref.stats[0] == 1


@pytest.mark.gpu
def test_moved_rows_may_overwrite_the_input_and_normals_turn(dev):
    from burn_depth_amd import ops
    _, xyz, target, tn, radius, K, *_ = next(c for c in cases() if c[0] == "bad rows")
    normals = np.random.default_rng(6).normal(size=(len(xyz), 3)).astype(f32)
    ref = P.register_points(xyz, target, radius, iterations=K, normals=normals, target_normals=tn)
    rows = _t(xyz)
    got = ops.register_points(dev, rows, _t(target), radius, iterations=K, xyz_out=rows, normals=_t(normals), target_normals=_t(tn))
    assert got.xyz.data_ptr() == rows.data_ptr() and got.normals is not None
    _same_plane(got, ref, "in place", len(xyz))


def _plane_call(lib, dev, xyz, n, reg, plane, xyz_out=None, normals_out=None):
    return lib.md_op_register_points_plane(dev.handle, C.c_void_p(xyz), None, n, C.byref(reg) if reg is not None else None,
                                           C.byref(plane) if plane is not None else None, C.c_void_p(xyz_out), C.c_void_p(normals_out), None)


@pytest.mark.gpu
def test_without_the_plane_part_the_entry_is_the_point_to_point_operator(dev, lib):
    from burn_depth_amd import ops
    _, xyz, target, tn, radius, K, *_ = next(c for c in cases() if c[0] == "other draw")
    want = ops.register_points(dev, _t(xyz), _t(target), radius, iterations=K, apply=True)
    src, tgt = _t(xyz), _t(target)
    for plane in (None, _lib.MdPointsRegisterPlane(None, None)):
        got = ops.register_points(dev, src, tgt, radius, iterations=K, apply=True)  # fresh tensors of the right sizes
        for t in (got.transform, got.sum_d2, got.xyz):
            t.fill_(7.0)
        reg = _lib.MdPointsRegister(radius, tgt.data_ptr(), len(target), _lib.MD_MEM_DEVICE, K, 3, 0, 0.0, 0.0, None, got.transform.data_ptr(),
                                    got.pairs.data_ptr(), got.sum_d2.data_ptr(), got.stats.data_ptr(), got.dropped.data_ptr(),
                                    got.nearest.data_ptr(), got.dist2.data_ptr())
        assert _plane_call(lib, dev, src.data_ptr(), len(xyz), reg, plane, xyz_out=got.xyz.data_ptr()) == _lib.MD_OK
        torch.cuda.synchronize()
        for k in ("transform", "pairs", "sum_d2", "stats", "dropped", "nearest", "dist2", "xyz"):
            assert np.array_equal(_u(getattr(got, k).cpu().numpy()), _u(getattr(want, k).cpu().numpy())), (plane is None, k)


@pytest.mark.gpu
def test_refusals_before_any_launch(dev, lib):
    xyz, (tgt, tn) = _t(_bumpy(10, 1)[0]), (_t(a.astype(f32)) for a in _bumpy(10, 2))
    out = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    r2 = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")

    def call(n=10, xyz_p=xyz.data_ptr(), normals_out=None, normals_p=tn.data_ptr(), **kw):
        f = dict(radius=0.3, target=tgt.data_ptr(), target_rows=10, target_kind=_lib.MD_MEM_DEVICE, iterations=2, min_pairs=6, apply=0, rot_eps=0.0,
                 trans_eps=0.0, init=None, transform=out.data_ptr(), pairs=None, sum_d2=None, stats=None, dropped=None, nearest=None, dist2=None)
        f.update(kw)
        reg = _lib.MdPointsRegister(*[f[k] for k in FIELDS])
        return _plane_call(lib, dev, xyz_p, n, reg, _lib.MdPointsRegisterPlane(normals_p, r2.data_ptr()), normals_out=normals_out)

    nan12 = (C.c_double * 12)(*([1.0] * 11 + [float("nan")]))
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")), dict(radius=1e30), dict(target_rows=-1), dict(target=None),
           dict(target=None, target_rows=0), dict(target_kind=_lib.MD_MEM_HOST), dict(iterations=0), dict(iterations=65), dict(min_pairs=2),
           dict(min_pairs=3), dict(min_pairs=5), dict(rot_eps=-1e-9), dict(trans_eps=float("nan")), dict(rot_eps=float("inf")),
           dict(init=C.cast(nan12, C.c_void_p)), dict(n=-1), dict(xyz_p=0), dict(normals_out=out.data_ptr())]
    for kw in bad:
        assert call(**kw) == _lib.MD_ERR_INVALID_ARG, kw
    assert call(n=1 << 30) == _lib.MD_ERR_SHAPE and call(target_rows=1 << 30) == _lib.MD_ERR_SHAPE
    assert _plane_call(lib, dev, xyz.data_ptr(), 10, None, _lib.MdPointsRegisterPlane(tn.data_ptr(), None)) == _lib.MD_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out.cpu() == 7.0).all() and (r2.cpu() == 7.0).all()  # nothing was launched
    assert call(min_pairs=3, normals_p=None) == _lib.MD_OK  # without normals the point form's bound holds, and sum_r2 stays
    torch.cuda.synchronize()
    assert (r2.cpu() == 7.0).all() and not (out.cpu() == 7.0).all()
    assert call() == _lib.MD_OK
    torch.cuda.synchronize()
    assert not (r2.cpu() == 7.0).any()
