"""The view filter in front of the point path: md_op_filter_views (an exact confidence percentile over all candidates of the call,
then the cross-view support count, on the device), md_infer_points_filtered (the model, the filter, the unprojection in one call)
and their host reference pipeline.filter_views.

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import functools
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
from points_util import _bits, _cloud_np, _da3, _da3_subset, _image, _pro, _same_cloud, _t, dev, lib  # noqa: E402,F401

f32 = np.float32
NEW_ENTRIES = ("md_view_filter_opts_default", "md_op_filter_views", "md_infer_points_filtered")
POISON = 123456.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the synthetic scene: B cameras on an arc look at the plane n . X = 4; a share of the pixels carries a wrong depth
# ---------------------------------------------------------------------------------------------------------------------------------
PLANE_N, PLANE_C = np.array([0.1, -0.05, 1.0]), 4.0


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) if axis == "x" else np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


@functools.lru_cache(maxsize=None)
def _scene(B, H, W, off, outliers=0.3):
    """-> (depth f32 [B,H,W], conf f32, K f32 [B,3,3], E f32 [B,3,4], outlier mask). f64 construction, rounded once."""
    K = np.zeros((B, 3, 3))
    E = np.zeros((B, 3, 4))
    depth = np.zeros((B, H, W))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    for b in range(B):
        K[b] = [[0.9 * W + b, 0, W / 2 + 0.3], [0, 0.8 * W + 2 * b, H / 2 - 0.7], [0, 0, 1]]
        R = _rot("y", 0.06 * (b - (B - 1) / 2)) @ _rot("x", 0.03 * b)
        t = np.array([0.25 * (b - (B - 1) / 2), 0.05 * b, 0.1 * b])
        E[b, :, :3], E[b, :, 3] = R, t
        # X = R^T (d r - t) on the plane: d (R n) . r = c + (R n) . t
        rn = R @ PLANE_N
        ray = np.stack([(u + off - K[b, 0, 2]) / K[b, 0, 0], (v + off - K[b, 1, 2]) / K[b, 1, 1], np.ones_like(u)], -1)
        depth[b] = (PLANE_C + rn @ t) / (ray @ rn)
    rng = np.random.default_rng(11)
    bad = rng.random((B, H, W)) < outliers
    factor = np.where(rng.random((B, H, W)) < 0.5, 0.7, 1.35)
    depth = np.where(bad, depth * factor, depth)
    conf = 1 + 2 * rng.random((B, H, W))
    out = tuple(a.astype(f32) for a in (depth, conf, K, E)) + (bad,)
    for a in out:
        a.setflags(write=False)
    return out


# (B, H, W, min_views): a partial single tile; a shape that crosses a 4096-pixel tile, with one and with two views required
SCENE_CASES = [(3, 37, 53, 1), (4, 70, 70, 1), (4, 70, 70, 2)]
RTOL = 0.02
# 30 % of the pixels carry a wrong depth, except where the f32 reference would leave the coverage band with it: with the
# percentile on top, two supporting views out of three are rare (each needs a landing pixel that survived and is no outlier),
# and the reference keeps 0.10-0.11 of each view; with 10 % it keeps 0.20-0.23
OUTLIERS = {(4, 70, 70, 2, 40): 0.1}

@functools.lru_cache(maxsize=None)
def _reference(B, H, W, min_views, q, off):
    """The scene and pipeline.filter_views on it, computed once and shared (read-only)."""
    d, c, K, E, bad = _scene(B, H, W, off, OUTLIERS.get((B, H, W, min_views, q), 0.3))
    ref = P.filter_views(d, c, intrinsics=K, extrinsics=E, pixel_offset=off, conf_percentile=q, view_rtol=RTOL, min_views=min_views)
    for a in ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return (d, c, K, E, bad), ref


def _assert_covered(ref, lo, hi=0.75):
    """Asserted on the reference: each view keeps a share in [lo, hi], so a comparison cannot pass on an (almost) empty or full map."""
    B = ref[0].shape[0]
    share = ref[3][:B] / ref[0][0].size
    assert ((share >= lo) & (share <= hi)).all(), share


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_filter_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^(?:int|long|void|const char\*)\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)  # test_host_abi's equality still holds
    for s in ("md_view_filter_opts", "md_view_filter_outputs"):
        assert f"}} {s};" in header
    o = _lib.MdViewFilterOpts(9, 9, 9, 9, 9, 9)
    lib.md_view_filter_opts_default(C.byref(o))
    assert (o.pixel_offset, o.depth_min, o.depth_max, o.conf_percentile, o.view_rtol, o.min_views) == (0, 0, 0, 0, 0, 0)
    assert C.sizeof(_lib.MdViewFilterOpts) == 24 and C.sizeof(_lib.MdViewFilterOutputs) == 32
    # the existing structs stay byte for byte
    assert C.sizeof(_lib.MdPointsOpts) == 28 and C.sizeof(_lib.MdPointsCameras) == 24 and C.sizeof(_lib.MdPointsOutputs) == 64


def test_reference_identical_views_support_each_other():
    rng = np.random.default_rng(5)
    H, W = 12, 17
    d1 = rng.uniform(1, 3, (H, W)).astype(f32)
    d1[3, 4], d1[5, 6], d1[0, 0] = 0, np.nan, np.inf
    d = np.stack([d1, d1])
    K = np.array([[[40, 0, 8.25], [0, 37, 6.5], [0, 0, 1]]] * 2, f32)
    E = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]] * 2, f32)
    for off in (0.0, 0.5):
        out, sup, tau, kept = P.filter_views(d, intrinsics=K, extrinsics=E, pixel_offset=off, view_rtol=1e-3, min_views=1)
        cand = np.isfinite(d) & (d > 0)
        assert np.array_equal(sup, cand.astype(np.uint8)) and tau == 0
        assert np.array_equal(_bits(out), _bits(np.where(cand, d, 0))) and kept.tolist() == [H * W - 3, H * W - 3, 2 * (H * W - 3)]


def test_reference_shifted_camera_closed_form():
    """A fronto-parallel plane d = 2, fx = fy = 64, integer principal point; the second camera is translated by (sx, sy) pixels'
    worth: t = (sx, sy, 0) * d / f, exact in f32. A pixel (v, u) of view 0 lands on (v + sy, u + sx) of view 1 and back."""
    H, W, sx, sy = 9, 14, 3, -2
    d = np.full((2, H, W), 2, f32)
    K = np.array([[[64, 0, 7], [0, 64, 4], [0, 0, 1]]] * 2, f32)
    E = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, sx / 32], [0, 1, 0, sy / 32], [0, 0, 1, 0]]], f32)
    out, sup, tau, kept = P.filter_views(d, intrinsics=K, extrinsics=E, view_rtol=1e-6, min_views=1)
    v, u = np.mgrid[0:H, 0:W]
    want0 = (u + sx >= 0) & (u + sx < W) & (v + sy >= 0) & (v + sy < H)
    want1 = (u - sx >= 0) & (u - sx < W) & (v - sy >= 0) & (v - sy < H)
    assert np.array_equal(sup[0], want0.astype(np.uint8)) and np.array_equal(sup[1], want1.astype(np.uint8))
    assert kept.tolist() == [want0.sum(), want1.sum(), want0.sum() + want1.sum()]
    assert np.array_equal(out, np.where(np.stack([want0, want1]), f32(2), f32(0)))
    # the landing pixel must itself be a survivor: knock one out in view 1 and its source in view 0 loses its support
    d2 = d.copy()
    d2[1, 5 + sy, 6 + sx] = 0
    sup2 = P.filter_views(d2, intrinsics=K, extrinsics=E, view_rtol=1e-6, min_views=1)[1]
    assert sup2[0, 5, 6] == 0 and sup2[1, 5 + sy, 6 + sx] == 0 and (sup2 != sup).sum() == 2
    # a depth that disagrees by more than the tolerance: 2 against 2.1 is 5 % of the smaller
    d3 = d.copy()
    d3[1] = f32(2.1)
    E3 = E.copy()
    E3[1, :2, 3] = 0
    assert P.filter_views(d3, intrinsics=K, extrinsics=E3, view_rtol=0.04, min_views=1)[3][-1] == 0
    assert P.filter_views(d3, intrinsics=K, extrinsics=E3, view_rtol=0.06, min_views=1)[3][-1] == 2 * H * W


def test_reference_percentile_is_the_sorted_order_statistic():
    rng = np.random.default_rng(9)
    d = rng.uniform(0.5, 2, (2, 11, 13)).astype(f32)
    c = (1 + 2 * rng.random((2, 11, 13))).astype(f32)
    d[0, 0, :5], c[1, 2, :4], c[1, 3, 0] = 0, np.nan, -1
    cand = (d > 0) & np.isfinite(c) & (c >= 0)
    N = int(cand.sum())
    assert N == 2 * 11 * 13 - 10
    for q in (1, 40, 99):
        out, sup, tau, kept = P.filter_views(d, c, conf_percentile=q)
        want = np.sort(c[cand])[(N - 1) * q // 100]
        assert tau == want and tau.dtype == f32
        assert kept[-1] == (c[cand] >= want).sum() and not sup.any()
        assert np.array_equal(out != 0, cand & (c >= want))
    out, sup, tau, kept = P.filter_views(np.zeros((2, 4, 5), f32), np.ones((2, 4, 5), f32), conf_percentile=40)  # N = 0
    assert tau == 0 and not kept.any() and not out.any()
    with pytest.raises(ValueError):
        P.filter_views(d, conf_percentile=40)
    with pytest.raises(ValueError):
        P.filter_views(d, c, min_views=1)


def test_reference_rejects_the_injected_outliers_where_decidable():
    """float64 on the synthetic scene. A pixel is decidable when every pixel it lands on in the other views carries the true
    plane depth: then a true pixel is supported by exactly the views it lands in (neighbouring plane depths differ by far less
    than 2 %), and a wrong one (off by 30 % / 35 %) by none."""
    B, H, W, off = 4, 70, 70, 0.5
    d, c, K, E, bad = (a.astype(np.float64) if a.dtype == f32 else a for a in _scene(B, H, W, off))
    out, sup, tau, kept = P.filter_views(d, None, intrinsics=K, extrinsics=E, pixel_offset=off, view_rtol=RTOL, min_views=1, dtype=np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    checked = 0
    for i in range(B):
        ray = np.stack([(u + off - K[i, 0, 2]) / K[i, 0, 0], (v + off - K[i, 1, 2]) / K[i, 1, 1], np.ones_like(u)], -1)
        X = (ray * d[i][..., None] - E[i, :, 3]) @ E[i, :, :3]  # R^T (p_c - t)
        inside_n = np.zeros((H, W), int)
        decidable = np.ones((H, W), bool)
        for j in range(B):
            if j == i:
                continue
            p = X @ E[j, :, :3].T + E[j, :, 3]
            uf, vf = K[j, 0, 0] * p[..., 0] / p[..., 2] + K[j, 0, 2] - off + 0.5, K[j, 1, 1] * p[..., 1] / p[..., 2] + K[j, 1, 2] - off + 0.5
            near_edge = (np.abs(uf - np.round(uf)) < 1e-6) | (np.abs(vf - np.round(vf)) < 1e-6)
            uu, vv = np.floor(uf).astype(int), np.floor(vf).astype(int)
            inside = (p[..., 2] > 0) & (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            lands_on_bad = bad[j][np.clip(vv, 0, H - 1), np.clip(uu, 0, W - 1)] & inside
            decidable &= ~lands_on_bad & ~near_edge
            inside_n += inside
        good = decidable & ~bad[i]
        wrong = decidable & bad[i]
        assert np.array_equal(sup[i][good], inside_n[good]) and not sup[i][wrong].any()
        assert (out[i][wrong] == 0).all() and np.array_equal(out[i][good] != 0, inside_n[good] >= 1)
        checked += int(good.sum()) + int(wrong.sum())
        assert good.sum() > 0.1 * H * W and wrong.sum() > 0.03 * H * W  # the condition is not vacuous
    assert checked > 0.2 * B * H * W


def _c_call(lib, devh, depth, conf, B, H, W, cam, o, out, no_o=False, no_out=False):
    return lib.md_op_filter_views(devh, depth, conf, B, H, W, C.byref(cam) if cam is not None else None, None if no_o else C.byref(o),
                                  None if no_out else C.byref(out), None)


def _refusals(lib, devh, depth, conf, cams, B, H, W, outs):
    """Every documented refusal of md_op_filter_views -> the list of (what, got, want)."""
    K, E = cams
    INV, SHAPE = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
    full = _lib.MdPointsCameras(K, E, None)
    ok = _lib.MdViewFilterOpts(0, 0, 0, 40, 0.02, 1)
    rows = []

    def case(what, want, o=ok, out=outs, cam=full, depth_=depth, conf_=conf, B_=B, H_=H, W_=W, **kw):
        rows.append((what, _c_call(lib, devh, depth_, conf_, B_, H_, W_, cam, o, out, **kw), want))

    V = _lib.MdViewFilterOpts
    case("null opts", INV, no_o=True)
    case("null outputs", INV, no_out=True)
    case("every output null", INV, out=_lib.MdViewFilterOutputs(None, None, None, None))
    case("q = 100", INV, o=V(0, 0, 0, 100, 0, 0))
    case("q = -1", INV, o=V(0, 0, 0, -1, 0, 0))
    case("q > 0 without a confidence map", INV, o=V(0, 0, 0, 40, 0, 0), conf_=None)
    for bad in (float("nan"), float("inf"), -0.5):
        case(f"view_rtol {bad}", INV, o=V(0, 0, 0, 0, bad, 1))
        case(f"depth_min {bad}", INV, o=V(0, bad, 0, 0, 0, 0))
    case("pixel_offset nan", INV, o=V(float("nan"), 0, 0, 0, 0, 0))
    case("depth_max < depth_min", INV, o=V(0, 2, 1, 0, 0, 0))
    case("min_views without view_rtol", INV, o=V(0, 0, 0, 0, 0, 1))
    case("view_rtol without min_views", INV, o=V(0, 0, 0, 0, 0.02, 0))
    case("min_views > B - 1", INV, o=V(0, 0, 0, 0, 0.02, B))
    case("view_rtol without extrinsics", INV, cam=_lib.MdPointsCameras(K, None, None))
    case("view_rtol without cameras", INV, cam=None)
    case("view_rtol without intrinsics or focal", INV, cam=_lib.MdPointsCameras(None, E, None))
    case("depth_out is the input", INV, out=_lib.MdViewFilterOutputs(depth, None, None, None))
    case("B = 65 with view_rtol", SHAPE, B_=65, H_=1, W_=1)
    case("B = 1 with view_rtol", SHAPE, B_=1)
    case("H = 0", SHAPE, H_=0)
    case("B H W = 2^31", SHAPE, o=V(0, 0, 0, 0, 0, 0), B_=2, H_=32768, W_=32768)
    return rows


def test_filter_argument_errors_without_a_gpu(lib):
    """Every refusal happens before the device is touched: with a null device the valid call is refused last."""
    buf = (C.c_float * 64)()
    buf2 = (C.c_float * 64)()
    px, px2 = C.cast(buf, C.c_void_p).value, C.cast(buf2, C.c_void_p).value
    outs = _lib.MdViewFilterOutputs(px2, None, None, px2)
    for what, got, want in _refusals(lib, None, px, px, (px, px), 2, 2, 2, outs):
        assert got == want, (what, got, want)
    # the null device, after everything else passed; focal_px stands in for intrinsics; B = 1 is fine without view_rtol
    assert _c_call(lib, None, px, px, 2, 2, 2, _lib.MdPointsCameras(None, px, px), _lib.MdViewFilterOpts(0, 0, 0, 40, 0.02, 1), outs) == _lib.MD_ERR_INVALID_ARG
    assert b"device is null" in lib.md_last_error()
    assert _c_call(lib, None, px, None, 1, 2, 2, None, _lib.MdViewFilterOpts(0, 0, 0, 0, 0, 0), outs) == _lib.MD_ERR_INVALID_ARG
    assert b"device is null" in lib.md_last_error()
    # the model entry refuses a null model and null options before anything else
    o = _lib.MdPointsOpts(0, 0, 0, 0, 0, 1, 0)
    po = _lib.MdPointsOutputs()
    fo = _lib.MdViewFilterOpts(0, 0, 0, 0, 0, 0)
    assert lib.md_infer_points_filtered(None, px, 1, 2, 2, 1, None, None, C.byref(fo), C.byref(o), C.byref(po), 1, None) == _lib.MD_ERR_INVALID_ARG
    assert (np.frombuffer(buf, f32) == 0).all() and (np.frombuffer(buf2, f32) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the operator
# ---------------------------------------------------------------------------------------------------------------------------------


def _poisoned(B, H, W):
    return dict(depth=torch.full((B, H, W), POISON, device="cuda"), support=torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda"),
                tau=torch.full((1,), POISON, device="cuda"), kept=torch.full((B + 1,), -5, dtype=torch.int32, device="cuda"))


def _run_filter(dev, d, c=None, K=None, E=None, focal=None, **opts):
    """ops.filter_views on poisoned outputs -> numpy (depth, support, tau, kept)."""
    from burn_depth_amd import ops
    out = _poisoned(*d.shape)
    ops.filter_views(dev, _t(d), _t(c), intrinsics=_t(K), extrinsics=_t(E), focal_px=_t(focal), out=out, **opts)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("depth", "support", "tau", "kept"))


def _assert_same(got, ref, what=""):
    print(what, "tau", float(got[2][0]), "kept", got[3].tolist(), "reference", float(ref[2]), ref[3].tolist())
    assert _bits(got[2])[0] == _bits(np.array([ref[2]], f32))[0], (what, got[2], ref[2])
    assert np.array_equal(got[3], ref[3]), (what, got[3], ref[3])
    assert np.array_equal(got[1], ref[1]), (what, "support", int((got[1] != ref[1]).sum()))
    assert np.array_equal(_bits(got[0]), _bits(ref[0])), (what, "depth", int((_bits(got[0]) != _bits(ref[0])).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0.0, 0.5])
@pytest.mark.parametrize("q", [0, 40])
@pytest.mark.parametrize("B,H,W,min_views", SCENE_CASES)
def test_filter_views_is_bit_identical_to_the_host_reference(dev, B, H, W, min_views, q, off):
    (d, c, K, E, _), ref = _reference(B, H, W, min_views, q, off)
    _assert_covered(ref, 0.15 if q else 0.25)
    got = _run_filter(dev, d, c, K, E, pixel_offset=off, conf_percentile=q, view_rtol=RTOL, min_views=min_views)
    _assert_same(got, ref, f"{(B, H, W)} min_views {min_views} q {q} off {off}")
    assert got[1].max() >= min_views and (got[1][ref[0] != 0] >= min_views).all()


@pytest.mark.gpu
def test_filter_views_focal_form_depth_bounds_and_optional_outputs(dev):
    """K = (f, f, W/2, H/2) from focal_px; explicit depth bounds; no confidence map; any output may be left out."""
    from burn_depth_amd import ops
    B, H, W = 3, 37, 53
    d, c, K, E, _ = _scene(B, H, W, 0.0)
    focal = np.array([0.9 * W + b for b in range(B)], f32)
    kw = dict(depth_min=3.5, depth_max=5.0, view_rtol=0.05, min_views=1)
    ref = P.filter_views(d, None, focal_px=focal, extrinsics=E, **kw)
    assert 0.1 * d.size < ref[3][-1] < 0.9 * d.size
    _assert_same(_run_filter(dev, d, None, None, E, focal, **kw), ref, "focal form")
    for only in ("depth", "support", "tau", "kept"):
        out = {only: _poisoned(B, H, W)[only]}
        ops.filter_views(dev, _t(d), _t(c), intrinsics=_t(K), extrinsics=_t(E), out=out, conf_percentile=40, view_rtol=RTOL, min_views=1)
        torch.cuda.synchronize()
        want = dict(zip(("depth", "support", "tau", "kept"), _reference(B, H, W, 1, 40, 0.0)[1]))[only]
        assert np.array_equal(out[only].cpu().numpy().reshape(-1).view(np.uint8), np.asarray(want).reshape(-1).view(np.uint8)), only


def _selection_maps():
    """name -> (depth, conf) of B = 2, 70 x 70 (crosses a 4096-pixel tile): the edge cases of the radix select."""
    rng = np.random.default_rng(21)
    shape = (2, 70, 70)
    n = int(np.prod(shape))
    ones = np.ones(shape, f32)
    maps = {"all equal": (ones, np.full(shape, 1.75, f32))}
    maps["lowest byte only"] = (ones, (np.uint32(0x3FC00000) + rng.integers(0, 256, shape).astype(np.uint32)).view(f32))
    maps["top byte only"] = (ones, (rng.integers(0x01, 0x7F, shape).astype(np.uint32) << np.uint32(24)).view(f32))
    single = np.zeros(shape, f32)
    single[1, 33, 44] = 2.0
    maps["one candidate"] = (single, (1 + rng.random(shape)).astype(f32))
    maps["no candidate"] = (np.zeros(shape, f32), ones)
    d, c = rng.uniform(1, 2, shape).astype(f32), (3 * rng.random(shape)).astype(f32)
    kind = rng.integers(0, 10, shape)  # kinds 0..4 spoil the pixel: half the map
    d = np.where(kind == 0, 0, np.where(kind == 1, np.inf, np.where(kind == 2, np.nan, d))).astype(f32)
    c = np.where(kind == 3, np.nan, np.where(kind == 4, -c - f32(0.5), c)).astype(f32)
    c.reshape(-1)[rng.choice(n, 40, replace=False)] = f32(-0.0)  # -0 is a candidate and counts as +0
    c.reshape(-1)[rng.choice(n, 40, replace=False)] = f32(0.0)
    c.reshape(-1)[rng.choice(n, 40, replace=False)] = f32(1e-42)  # a denormal
    maps["half non-candidates"] = (d, c)
    maps["uniform"] = (ones, (1 + 2 * rng.random(shape)).astype(f32))
    return maps


@pytest.mark.gpu
def test_percentile_selection_edge_cases(dev):
    for name, (d, c) in _selection_maps().items():
        cand = np.isfinite(d) & (d > 0) & np.isfinite(c) & (c >= 0)
        if name == "half non-candidates":
            assert 0.4 < cand.mean() < 0.6
        for q in (1, 40, 99):
            ref = P.filter_views(d, c, conf_percentile=q)
            if cand.any():
                assert ref[2] == np.sort(np.where(c[cand] == 0, f32(0), c[cand]))[(int(cand.sum()) - 1) * q // 100]
            _assert_same(_run_filter(dev, d, c, conf_percentile=q), ref, f"{name} q {q}")
    # q = 0: a pass-through of the candidates, tau = 0
    d, c = _selection_maps()["half non-candidates"]
    got = _run_filter(dev, d, c)
    _assert_same(got, P.filter_views(d, c), "pass-through")
    cand = np.isfinite(d) & (d > 0) & np.isfinite(c) & (c >= 0)
    assert got[3][-1] == cand.sum() and got[2][0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,min_views", SCENE_CASES[1:])
def test_unproject_of_the_filtered_depth_equals_the_host_composition(dev, B, H, W, min_views):
    from burn_depth_amd import ops
    off, q = 0.5, 40
    (d, c, K, E, _), ref = _reference(B, H, W, min_views, q, off)
    fd = ops.filter_views(dev, _t(d), _t(c), intrinsics=_t(K), extrinsics=_t(E), pixel_offset=off, conf_percentile=q, view_rtol=RTOL,
                          min_views=min_views)[0]
    pc = ops.unproject(dev, fd, intrinsics=_t(K), extrinsics=_t(E), conf=_t(c), pixel_offset=off, world=True)
    torch.cuda.synchronize()
    want = P.unproject_depth(ref[0], intrinsics=K, extrinsics=E, conf=c, pixel_offset=off, world=True)
    assert np.array_equal(pc.count.cpu().numpy(), want.count) and np.array_equal(want.count, ref[3]) and want.count[-1] > 0
    n = int(want.count[-1])
    assert np.array_equal(pc.mask.cpu().numpy(), want.mask)
    assert np.array_equal(_bits(pc.point_map.cpu().numpy()), _bits(want.point_map))
    assert np.array_equal(_bits(pc.xyz.cpu().numpy()[:n]), _bits(want.xyz))
    assert np.array_equal(_bits(pc.conf.cpu().numpy()[:n]), _bits(want.conf))


@pytest.mark.gpu
def test_filter_refusals_leave_the_outputs_untouched(dev, lib):
    B, H, W = 2, 37, 53
    d, c, K, E, _ = _scene(3, H, W, 0.0)
    td, tc, tk, te = _t(d), _t(c), _t(K), _t(E)
    out = _poisoned(B, H, W)
    outs = _lib.MdViewFilterOutputs(out["depth"].data_ptr(), out["support"].data_ptr(), out["tau"].data_ptr(), out["kept"].data_ptr())
    rows = _refusals(lib, dev.handle, td.data_ptr(), tc.data_ptr(), (tk.data_ptr(), te.data_ptr()), B, H, W, outs)
    torch.cuda.synchronize()
    for what, got, want in rows:
        assert got == want, (what, got, want)
    assert (out["depth"] == POISON).all() and (out["support"] == 77).all() and (out["tau"] == POISON).all() and (out["kept"] == -5).all()
    # and the call the refusals were variations of goes through
    assert _c_call(lib, dev.handle, td.data_ptr(), tc.data_ptr(), B, H, W, _lib.MdPointsCameras(tk.data_ptr(), te.data_ptr(), None),
                   _lib.MdViewFilterOpts(0, 0, 0, 40, 0.02, 1), outs) == 0
    torch.cuda.synchronize()
    assert 0 < int(out["kept"][-1]) < B * H * W and not (out["depth"] == POISON).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: the model call
# ---------------------------------------------------------------------------------------------------------------------------------


def _composition(dev, depth, conf, intr, extr, fkw, pkw, focal=None):
    """ops.filter_views -> ops.unproject on the model's own tensors -> (cloud dict with the filtered depth, kept)."""
    from burn_depth_amd import ops
    off = pkw.get("pixel_offset", 0.0)
    fd, _, _, kept = ops.filter_views(dev, depth, conf, intrinsics=intr, extrinsics=extr, focal_px=focal, pixel_offset=off, **fkw)
    want = _cloud_np(ops.unproject(dev, fd, intrinsics=intr, extrinsics=extr, focal_px=focal, conf=conf, **pkw))
    want["depth"] = fd.cpu().numpy()
    return want, kept.cpu().numpy()


@pytest.mark.gpu
def test_infer_points_filtered_da3_equals_the_composition(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        depth, conf, extr, intr = _da3_subset(m, x)
        cand = int((torch.isfinite(depth) & (depth > 0) & torch.isfinite(conf) & (conf >= 0)).sum())
        assert cand > 0.9 * depth.numel()
        pkw = dict(pixel_offset=0.5, world=True)
        # the percentile alone: 60 % of the candidates stay (ties can only add)
        want, kept = _composition(dev, depth, conf, intr, extr, dict(conf_percentile=40), pkw)
        got = _cloud_np(m.infer_points(x, conf_percentile=40, **pkw))
        print("percentile: kept", kept.tolist(), "of", cand)
        assert 0.5 * cand <= kept[-1] <= 0.7 * cand and np.array_equal(want["count"], kept)
        _same_cloud(want, got, "percentile")
        assert np.array_equal(got["depth"] != 0, got["mask"] != 0)
        # conf_min still works on top of tau, and the other point options apply afterwards
        cmin = float(conf.quantile(0.7))
        pkw2 = dict(pkw, conf_min=cmin, stride=2, edge_rtol=0.5)
        want2, _ = _composition(dev, depth, conf, intr, extr, dict(conf_percentile=40), pkw2)
        assert 0 < want2["count"][-1] < want["count"][-1]
        _same_cloud(want2, _cloud_np(m.infer_points(x, conf_percentile=40, **pkw2)), "percentile + point options")
        # the cross-view test through the model's own cameras, alone and with the percentile
        for fkw in (dict(view_rtol=0.5, min_views=1), dict(view_rtol=0.5, min_views=2, conf_percentile=40)):
            want3, kept3 = _composition(dev, depth, conf, intr, extr, fkw, pkw)
            print(fkw, "kept", kept3.tolist())
            _same_cloud(want3, _cloud_np(m.infer_points(x, **fkw, **pkw)), str(fkw))
        # the caller's cameras replace the model's, camera-space output included (the filter still needs the extrinsics)
        K, E = (np.array(a) for a in _scene(3, 70, 70, 0.5)[2:4])  # copies: the shared scene is read-only
        fkw = dict(view_rtol=0.5, min_views=1)
        want4, _ = _composition(dev, depth, conf, _t(K), _t(E), fkw, dict(pixel_offset=0.5))
        _same_cloud(want4, _cloud_np(m.infer_points(x, intrinsics=K, extrinsics=E, pixel_offset=0.5, **fkw)), "caller cameras")
        # refusals
        for kw in (dict(conf_percentile=100), dict(view_rtol=0.5), dict(min_views=1), dict(view_rtol=0.5, min_views=3)):
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, kw
        # the option structs must agree on pixel_offset and the depth bounds
        from burn_depth_amd.points import _points_cameras, _points_opts, _points_outputs, _view_filter_opts
        res, outs = _points_outputs(x.device, 3, 70, 70, True, True, None, 1, False, True, True, None)
        cam, _ = _points_cameras(x.device, 3)
        for fo in (_view_filter_opts(0.5, 0, 0, 40), _view_filter_opts(0, 1.0, 0, 40), _view_filter_opts(0, 0, 9.0, 40)):
            o = _points_opts()
            assert _lib.load().md_infer_points_filtered(m._h, C.c_void_p(x.data_ptr()), 3, 70, 70, 1, None, C.byref(cam), C.byref(fo), C.byref(o),
                                                        C.byref(outs), 1, None) == _lib.MD_ERR_INVALID_ARG
    finally:
        m.destroy()


@pytest.mark.gpu
def test_infer_points_filtered_graph_replay_and_allocations(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        kw = dict(conf_percentile=40, view_rtol=0.5, min_views=1, pixel_offset=0.5, world=True)
        eager = _cloud_np(m.infer_points(x, **kw))
        assert 0 < eager["count"][-1] < 3 * 70 * 70
        m.enable_graph(True)
        out = m.infer_points(x, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (2, 3, 4):  # 2: capture, 3 and 4: replay
            for t in (out.xyz, out.point_map, out.depth):
                t.fill_(POISON)
            out = m.infer_points(x, out=out, **kw)
            torch.cuda.synchronize()
            _same_cloud(eager, _cloud_np(out), f"graph call {call}")
        assert m.query("allocs") == allocs
        # a replay reads the inputs at run time, and another filter option takes another graph
        x2 = _image(3, 70, seed=1).cuda()
        m.enable_graph(False)
        want2 = _cloud_np(m.infer_points(x2, **kw))
        want3 = _cloud_np(m.infer_points(x2, **dict(kw, conf_percentile=80)))
        assert want3["count"][-1] < want2["count"][-1]
        m.enable_graph(True)
        x.copy_(x2)
        _same_cloud(want2, _cloud_np(m.infer_points(x, out=out, **kw)), "replay on new pixels")
        for _ in range(3):
            out = m.infer_points(x, out=out, **dict(kw, conf_percentile=80))
        torch.cuda.synchronize()
        _same_cloud(want3, _cloud_np(out), "another percentile")
        assert m.query("allocs") == allocs
        # the unfiltered call is the old entry and still its own graph
        m.enable_graph(False)
        plain = _cloud_np(m.infer_points(x, pixel_offset=0.5, world=True))
        assert plain["count"][-1] > want2["count"][-1]
    finally:
        m.enable_graph(False)
        m.destroy()


@pytest.mark.gpu
def test_infer_points_filtered_depth_pro(dev):
    m = _pro(dev)
    try:
        x = _image(2, 512).cuda()
        with pytest.raises(_lib.MdError) as e:  # Depth Pro has no confidence map
            m.infer_points(x, conf_percentile=40)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        with pytest.raises(_lib.MdError) as e:  # and predicts no extrinsics
            m.infer_points(x, view_rtol=0.1, min_views=1)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        ref = m.infer(x)
        E = np.array(_scene(2, 37, 53, 0.0)[3])
        fkw = dict(view_rtol=0.1, min_views=1)
        for pkw in (dict(pixel_offset=0.5, world=True, stride=2), dict()):
            want, kept = _composition(dev, ref.depth, None, None, _t(E), fkw, pkw, focal=ref.focallength_px)
            print("depth pro", pkw, "kept", kept.tolist())
            assert 0 < kept[-1] < 2 * 512 * 512
            _same_cloud(want, _cloud_np(m.infer_points(x, extrinsics=E, **fkw, **pkw)), str(pkw))
    finally:
        m.destroy()
