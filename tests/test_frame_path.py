"""The frame path: md_process_frame (u8 RGB frames in, a displayable depth map out, in one device call), its stand-alone operators
md_op_resize_catmull_rom / md_op_depth_display, the host tap builder md_catmull_rom_taps, and their host references in
burn_depth_amd/pipeline.py (prepare_input_frame, depth_to_display; the viewer's process_frame, crates/bevy_burn_depth/src/lib.rs).

The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import importlib.util
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

f32 = np.float32
NEW_ENTRIES = ("md_frame_geometry", "md_process_frame", "md_catmull_rom_taps", "md_op_resize_catmull_rom", "md_op_depth_display")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _taps(lib, n, new):
    """[(left, weights f32)] of every output of an n -> new pass, from the library."""
    out = []
    buf = (C.c_float * (4 * n // new + 8))()
    for o in range(new):
        l, c = C.c_int(), C.c_int()
        assert lib.md_catmull_rom_taps(n, new, o, C.byref(l), C.byref(c), buf) == 0
        out.append((l.value, np.frombuffer(buf, f32)[:c.value].copy()))
    return out


_libm = C.CDLL("libm.so.6")
_libm.powf.restype, _libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]


def _catmull_rom_glibc(x):
    """pipeline._catmull_rom with a ** 3 through glibc's powf (numpy's f32 power dispatches to a vector library on AVX-512
    hosts, whose last bit differs from glibc's): the tap builder's arithmetic contract."""
    a = np.abs(x).astype(f32)
    a3 = np.array([_libm.powf(float(v), 3.0) for v in a], f32)
    k = np.where(a < 1, f32(9) * a3 + f32(-15) * (a * a) + f32(6),
                 np.where(a < 2, f32(-3) * a3 + f32(15) * (a * a) + f32(-24) * a + f32(12), f32(0)))
    return (k / 6).astype(f32)


def _windows_ref(n, new):
    """pipeline._sample_axis's windows and weights, the sum taken left to right."""
    ratio = f32(n) / f32(new)
    sratio = max(ratio, f32(1.0))
    support = f32(2.0) * sratio
    res = []
    for o in range(new):
        centre = (f32(o) + f32(0.5)) * ratio
        left = int(min(max(np.floor(centre - support), 0), n - 1))
        right = int(min(max(np.ceil(centre + support), left + 1), n))
        w = _catmull_rom_glibc((np.arange(left, right, dtype=f32) - (centre - f32(0.5))) / sratio)
        s = f32(0)
        for v in w:
            s = f32(s + v)
        res.append((left, (w / s).astype(f32)))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_frame_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^int\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS
    assert "MD_FRAME_U8_GRAY" in header and "MD_FRAME_RGBA_F32" in header


@pytest.mark.parametrize("n,new", [(1080, 518), (1920, 921), (360, 518), (518, 518), (7, 3), (720, 518), (1280, 921), (1, 518)])
def test_catmull_rom_taps_match_the_host_resampler(lib, n, new):
    got = _taps(lib, n, new)
    want = _windows_ref(n, new)
    for o, ((gl, gw), (wl, ww)) in enumerate(zip(got, want)):
        assert gl == wl and len(gw) == len(ww), (o, gl, wl, len(gw), len(ww))
        assert (gw.view(np.uint32) == ww.view(np.uint32)).all(), (o, gw, ww)
    # the windows and weights of pipeline._sample_axis itself: one pass over the identity image puts output o's weights at
    # columns [left, right) of row o (its own weight sum, and numpy's power, may differ in the last bit)
    eye = np.eye(n, dtype=f32)[:, :, None]
    m = P._sample_axis(eye, new, 0)[:, :, 0]
    for o, (gl, gw) in enumerate(got):
        nz = np.nonzero(m[o])[0]
        assert nz.min() >= gl and nz.max() < gl + len(gw), (o, nz, gl, len(gw))
        np.testing.assert_allclose(m[o, gl:gl + len(gw)], gw, rtol=2e-6, atol=1e-6)


def test_prepare_input_frame_align_down():
    rng = np.random.default_rng(0)
    ps = 14
    # (w, h) -> crop size: below one patch the size stays, between one and four patches a multiple of the patch, from four
    # patches on a multiple of four patches
    for (w, h), (cw, ch) in {(10, 13): (10, 13), (30, 50): (28, 42), (56, 112): (56, 112), (100, 57): (56, 56),
                             (1920, 1080): (1904, 1064), (14, 28): (14, 28), (55, 200): (42, 168)}.items():
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = P.prepare_input_frame(rgb, ps, None)
        assert (p.width, p.height) == (cw, ch) and p.rgb.shape == (ch, cw, 3)
        ox, oy = (w - cw) // 2, (h - ch) // 2
        assert (p.rgb == rgb[oy:oy + ch, ox:ox + cw]).all()
    rgb = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    p = P.prepare_input_frame(rgb, ps, 28)
    assert (p.rgb == P.prepare_depth_anything3_image(rgb, 28).rgb).all()
    assert P.prepare_input_frame(rgb, ps, 5).width == 14  # the target is raised to the patch size


def _planted_field(rng, h, w, lo=0.5, hi=20.0):
    d = rng.uniform(lo, hi, (h, w)).astype(f32)
    d[1, 2], d[3, 1], d[h - 1, w - 1] = np.inf, -np.inf, np.nan
    return d


def test_depth_to_display_u8_equals_depth_to_u8():
    rng = np.random.default_rng(1)
    d = _planted_field(rng, 30, 40)
    for crop, dims in ((None, None), (None, (57, 33)), (P.ImageCropRegion(3, 2, 30, 20), (80, 50)), (P.ImageCropRegion(3, 2, 30, 20), None)):
        assert (P.depth_to_display(d, crop, dims, True, "u8") == P.depth_to_u8(d, crop, dims)).all()
    rgba = P.depth_to_display(d[None], None, None, True, "rgba")
    assert rgba.shape == (1, 30, 40, 4) and rgba.dtype == np.float32 and (rgba[..., 3] == 1).all()
    assert np.array_equal(np.floor(rgba[0, ..., 0] * f32(255) + f32(0.5)).astype(np.uint8), P.depth_to_u8(d))
    raw = P.depth_to_display(d, None, None, False, "rgba")
    assert np.array_equal(raw[..., 1], d, equal_nan=True)
    with pytest.raises(ValueError):
        P.depth_to_display(d, None, None, False, "u8")


def test_frame_argument_errors_without_a_gpu(lib):
    o = _lib.MdFrameOpts(0, 1, 1, _lib.MD_FRAME_U8_GRAY)
    outs = _lib.MdFrameOutputs()
    buf = (C.c_uint8 * 12)()
    px = C.cast(buf, C.c_void_p)
    pf = lambda m, rgb, B, w, h, opts: lib.md_process_frame(m, rgb, B, w, h, _lib.MD_MEM_HOST, C.byref(opts), C.byref(outs), _lib.MD_MEM_HOST, None)
    assert pf(None, None, 1, 2, 2, o) == _lib.MD_ERR_INVALID_ARG
    assert pf(None, px, 1, 0, 2, o) == _lib.MD_ERR_SHAPE
    assert pf(None, px, 1, 2, -1, o) == _lib.MD_ERR_SHAPE
    assert pf(None, px, 0, 2, 2, o) == _lib.MD_ERR_SHAPE
    assert pf(None, px, 1, 2, 2, _lib.MdFrameOpts(0, 1, 1, 7)) == _lib.MD_ERR_INVALID_ARG        # unknown format
    assert pf(None, px, 1, 2, 2, _lib.MdFrameOpts(0, 1, 0, _lib.MD_FRAME_U8_GRAY)) == _lib.MD_ERR_INVALID_ARG  # u8 without normalise
    assert pf(None, px, 1, 2, 2, o) == _lib.MD_ERR_INVALID_ARG                                   # null model
    i = [C.c_int() for _ in range(4)]
    assert lib.md_frame_geometry(None, 2, 2, C.byref(o), *(C.byref(x) for x in i)) == _lib.MD_ERR_INVALID_ARG
    l, c = C.c_int(), C.c_int()
    assert lib.md_catmull_rom_taps(0, 5, 0, C.byref(l), C.byref(c), None) == _lib.MD_ERR_SHAPE
    assert lib.md_catmull_rom_taps(5, 3, 3, C.byref(l), C.byref(c), None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_resize_catmull_rom(None, px, 1, 2, 2, 4, 4, 0, 0, 4, 4, px, None, None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_resize_catmull_rom(None, px, 1, 2, 2, 4, 4, 1, 0, 4, 4, px, None, None) == _lib.MD_ERR_SHAPE  # crop outside
    assert lib.md_op_depth_display(None, px, 1, 2, 2, 0, 0, 0, 0, 2, 2, 1, 0, px, None, None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_depth_display(None, px, 1, 2, 2, 0, 0, 0, 0, 2, 2, 0, 0, px, None, None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_depth_display(None, px, 1, 2, 2, 0, 0, 0, 0, 2, 2, 1, 9, px, None, None) == _lib.MD_ERR_INVALID_ARG
    assert lib.md_op_depth_display(None, px, 1, 2, 2, 1, 1, 2, 2, 2, 2, 1, 0, px, None, None) == _lib.MD_ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    d = Device(0)
    yield d


def _da3_geometry(w, h, t):
    if w == t and h == t:
        return w, h, 0, 0
    s = f32(t) / f32(max(min(w, h), 1))
    sw, sh = max(int(np.round(f32(w) * s)), t), max(int(np.round(f32(h) * s)), t)
    return sw, sh, (sw - t) // 2, (sh - t) // 2


def _sequential_resize(lib, rgb, sw, sh, cx, cy, tw, th):
    """The separable resampler in the kernels' order: taps left to right, f32 multiply then add, vertical pass first."""
    h, w = rgb.shape[:2]
    src = rgb.astype(f32)
    if (sw, sh) == (w, h):
        return rgb[cy:cy + th, cx:cx + tw].copy()
    tv, th_ = _taps(lib, h, sh), _taps(lib, w, sw)
    tmp = np.empty((th, w, 3), f32)
    for oy in range(th):
        left, wt = tv[cy + oy]
        acc = np.zeros((w, 3), f32)
        for k, wk in enumerate(wt):
            acc = (acc + wk * src[left + k]).astype(f32)
        tmp[oy] = acc
    out = np.empty((th, tw, 3), f32)
    for ox in range(tw):
        left, wt = th_[cx + ox]
        acc = np.zeros((th, 3), f32)
        for k, wk in enumerate(wt):
            acc = (acc + wk * tmp[:, left + k]).astype(f32)
        out[:, ox] = acc
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1920, 1080), (1280, 720), (360, 540), (518, 518), (1, 1)])
def test_resize_catmull_rom_kernel(lib, dev, w, h):
    from burn_depth_amd.depth_pro import _stream_ptr
    t = 518
    rng = np.random.default_rng(w * 7 + h)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    sw, sh, cx, cy = _da3_geometry(w, h, t)
    x = torch.from_numpy(rgb).cuda()
    u8 = torch.empty((1, t, t, 3), dtype=torch.uint8, device="cuda")
    nchw = torch.empty((1, 3, t, t), dtype=torch.float32, device="cuda")
    _lib.check(lib.md_op_resize_catmull_rom(dev.handle, C.c_void_p(x.data_ptr()), 1, h, w, sw, sh, cx, cy, t, t, C.c_void_p(u8.data_ptr()),
                                            C.c_void_p(nchw.data_ptr()), _stream_ptr(0)))
    got = u8[0].cpu().numpy()
    want = _sequential_resize(lib, rgb, sw, sh, cx, cy, t, t)
    assert np.array_equal(got, want), int((got != want).sum())
    host = P.prepare_depth_anything3_image(rgb, t).rgb
    d = np.abs(got.astype(np.int32) - host.astype(np.int32))
    assert d.max() <= 1 and (d == 0).mean() >= 0.999, (int(d.max()), float((d == 0).mean()))
    ref = torch.empty_like(nchw)
    _lib.check(lib.md_op_rgb_to_input(dev.handle, C.c_void_p(u8.data_ptr()), t * t * 3, t, t, C.c_void_p(ref.data_ptr()), _stream_ptr(0)))
    torch.cuda.synchronize()
    assert torch.equal(nchw.view(torch.int32), ref.view(torch.int32))


@pytest.mark.gpu
def test_resize_catmull_rom_batch_and_crop_only(lib, dev):
    from burn_depth_amd.depth_pro import _stream_ptr
    rng = np.random.default_rng(5)
    B, h, w = 3, 90, 130  # odd row length in bytes: the byte-load form
    rgb = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    x = torch.from_numpy(rgb).cuda()
    for (sw, sh, cx, cy, tw, th) in ((w, h, 9, 5, 112, 84), (101, 70, 15, 0, 70, 70)):
        u8 = torch.empty((B, th, tw, 3), dtype=torch.uint8, device="cuda")
        _lib.check(lib.md_op_resize_catmull_rom(dev.handle, C.c_void_p(x.data_ptr()), B, h, w, sw, sh, cx, cy, tw, th,
                                                C.c_void_p(u8.data_ptr()), None, _stream_ptr(0)))
        got = u8.cpu().numpy()
        for b in range(B):
            assert np.array_equal(got[b], _sequential_resize(lib, rgb[b], sw, sh, cx, cy, tw, th)), (sw, sh, b)


def _display(lib, dev, d, crop, ow, oh, normalize, fmt):
    from burn_depth_amd.depth_pro import _stream_ptr
    B, h, w = d.shape
    x = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    out = torch.empty((B, oh, ow), dtype=torch.uint8, device="cuda") if fmt == "u8" else torch.empty((B, oh, ow, 4), device="cuda")
    rng_ = torch.empty((B, 2), device="cuda")
    cx, cy, cw, ch = (crop.x, crop.y, crop.width, crop.height) if crop else (0, 0, 0, 0)
    _lib.check(lib.md_op_depth_display(dev.handle, C.c_void_p(x.data_ptr()), B, h, w, cx, cy, cw, ch, ow, oh, int(normalize),
                                       _lib.MD_FRAME_U8_GRAY if fmt == "u8" else _lib.MD_FRAME_RGBA_F32, C.c_void_p(out.data_ptr()),
                                       C.c_void_p(rng_.data_ptr()), _stream_ptr(0)))
    return out.cpu().numpy(), rng_.cpu().numpy()


@pytest.mark.gpu
def test_depth_display_kernel_on_planted_fields(lib, dev):
    rng = np.random.default_rng(3)
    B, h, w = 3, 61, 83
    d = np.stack([_planted_field(rng, h, w, 0.1, 3.0), _planted_field(rng, h, w, 5.0, 700.0), _planted_field(rng, h, w, -4.0, 4.0)])
    allbad = np.full((1, h, w), np.nan, f32)
    allbad[0, :5] = np.inf
    const = np.full((1, h, w), 2.5, f32)
    crop = P.ImageCropRegion(7, 4, 60, 45)
    cases = [(d, None, w, h), (d, crop, 150, 97), (d, crop, 31, 20), (d, None, 1, 1), (allbad, None, w, h), (const, crop, 90, 70)]
    for field, cr, ow, oh in cases:
        dims = (ow, oh)
        u8, rg = _display(lib, dev, field, cr, ow, oh, True, "u8")
        for b in range(field.shape[0]):
            assert np.array_equal(u8[b], P.depth_to_u8(field[b], cr, dims)), (b, cr, dims)
        rgba, _ = _display(lib, dev, field, cr, ow, oh, True, "rgba")
        assert np.array_equal(rgba, P.depth_to_display(field, cr, dims, True, "rgba")), (cr, dims)
        raw, _ = _display(lib, dev, field, cr, ow, oh, False, "rgba")
        assert np.array_equal(raw, P.depth_to_display(field, cr, dims, False, "rgba"), equal_nan=True), (cr, dims)
        for b in range(field.shape[0]):
            v = field[b] if cr is None else P.crop_depth_field(field[b], cr)
            v = P.resize_depth_field(v, ow, oh)
            fin = np.isfinite(v)
            want = (v[fin].min(), v[fin].max()) if fin.any() else (0.0, 1.0)
            assert tuple(rg[b]) == tuple(np.float32(want)), (b, rg[b], want)


def _seeded_da3(dev, variant, max_batch=1):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = {"tiny": DepthAnything3Config.tiny_test, "small": DepthAnything3Config.small, "metric_large": DepthAnything3Config.metric_large}[variant]()
    cfg.max_batch = max_batch
    return DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _seeded_pro(dev):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthProConfig
    from burn_depth_amd.depth_pro import DepthPro
    return DepthPro.new(dev, DepthProConfig.tiny_test(), seed=0, init_scheme=Wt.INIT_PARITY)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("variant,w,h,B", [("tiny", 150, 100, 2), ("small", 1280, 720, 1), ("metric_large", 700, 900, 1)])
def test_process_frame_da3_end_to_end(dev, variant, w, h, B):
    from burn_depth_amd.inference import rgb_to_input_tensor
    m = _seeded_da3(dev, variant, max_batch=B)
    try:
        rng = np.random.default_rng(11)
        rgb = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
        r = m.process_frame(rgb, target=0, restore=True, normalize=True, fmt="u8")
        t = m.img_size()
        assert tuple(r.depth.shape) == (B, t, t) and tuple(r.display.shape) == (B, h, w)
        for b in range(B):
            prep = r.prepared[b].cpu().numpy()
            assert np.array_equal(prep, _sequential_resize(_lib.load(), rgb[b], *_da3_geometry(w, h, t), t, t))
            ref = m.infer(rgb_to_input_tensor(prep.tobytes(), t, t, dev)).depth
            assert torch.equal(_bits(r.depth[b]), _bits(ref[0])), variant
            depth = r.depth[b].cpu().numpy()
            assert np.array_equal(r.display[b].cpu().numpy(), P.depth_to_display(depth, None, (w, h), True, "u8"))
        # the viewer's call: model resolution, RGBA texture
        v = P.AnyDepthModel(P.DepthModelKind.DEPTH_ANYTHING3, m).process_frame(torch.from_numpy(rgb).cuda())
        assert torch.equal(_bits(v.depth), _bits(r.depth))
        assert np.array_equal(v.display.cpu().numpy(), P.depth_to_display(r.depth.cpu().numpy(), None, None, True, "rgba"))
        # patch-aligned crop, no resize
        c = m.process_frame(rgb, target=-1, restore=False, normalize=False, fmt="rgba")
        p0 = P.prepare_input_frame(rgb[0], m.patch_size(), None)
        assert np.array_equal(c.prepared[0].cpu().numpy(), p0.rgb)
        ref = m.infer(rgb_to_input_tensor(p0.rgb.tobytes(), p0.width, p0.height, dev)).depth
        assert torch.equal(_bits(c.depth[0]), _bits(ref[0]))
        assert np.array_equal(c.display[0].cpu().numpy(), P.depth_to_display(c.depth[0].cpu().numpy(), None, None, False, "rgba"))
    finally:
        m.destroy()


@pytest.mark.gpu
def test_process_frame_depth_pro_matches_infer_from_rgb(dev):
    m = _seeded_pro(dev)
    try:
        rng = np.random.default_rng(12)
        h, w = 400, 600
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        r = m.process_frame(rgb, target=0, restore=True, normalize=True, fmt="u8")
        ref = m.infer_from_rgb(rgb.tobytes(), w, h)
        assert torch.equal(_bits(r.depth), _bits(ref.depth))
        assert torch.equal(_bits(r.focallength_px), _bits(ref.focallength_px))
        assert torch.equal(_bits(r.fovy_rad), _bits(ref.fovy_rad))
        assert np.array_equal(r.prepared[0].cpu().numpy(), rgb)
        assert np.array_equal(r.display[0].cpu().numpy(), P.depth_to_u8(ref.depth.cpu().numpy()))
        # a fork gives the same bits on the same frame
        f = m.fork()
        try:
            rf = f.process_frame(rgb, target=0, restore=True, normalize=True, fmt="u8")
            assert torch.equal(_bits(rf.depth), _bits(r.depth)) and torch.equal(rf.display.cpu(), r.display.cpu())
        finally:
            f.destroy()
        # errors on a live model
        with pytest.raises(_lib.MdError) as e:
            m.process_frame(rgb, target=518)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        with pytest.raises(_lib.MdError) as e:
            m.process_frame(np.stack([rgb, rgb]))
        assert e.value.code == _lib.MD_ERR_SHAPE
    finally:
        m.destroy()


@pytest.mark.gpu
def test_process_frame_errors_on_a_live_da3_model(dev):
    m = _seeded_da3(dev, "tiny")
    try:
        rgb = np.zeros((50, 60, 3), np.uint8)
        for kw, code in (({"target": 100}, _lib.MD_ERR_SHAPE), ({"fmt": "u8", "normalize": False}, _lib.MD_ERR_INVALID_ARG)):
            with pytest.raises(_lib.MdError) as e:
                m.process_frame(rgb, **kw)
            assert e.value.code == code, kw
        with pytest.raises(_lib.MdError) as e:
            m.process_frame(np.zeros((2, 50, 60, 3), np.uint8))
        assert e.value.code == _lib.MD_ERR_SHAPE
        with pytest.raises(_lib.MdError) as e:  # the patch-aligned crop of a frame below one patch
            m.process_frame(np.zeros((10, 60, 3), np.uint8), target=-1)
        assert e.value.code == _lib.MD_ERR_SHAPE
    finally:
        m.destroy()


@pytest.mark.gpu
def test_process_frame_graph_replay_and_allocations(dev):
    m = _seeded_da3(dev, "tiny", max_batch=2)
    try:
        rng = np.random.default_rng(13)
        frames = [rng.integers(0, 256, (2, 120, 160, 3), dtype=np.uint8) for _ in range(3)]
        eager = [m.process_frame(f, target=0, restore=True, normalize=True, fmt="rgba") for f in frames]
        eager = [(e.display.clone(), e.depth.clone(), e.depth_range.clone()) for e in eager]
        buf = torch.empty((2, 120, 160, 3), dtype=torch.uint8, device="cuda")
        m.enable_graph(True)
        out = None
        for rep in range(2):
            for f, (disp, depth, rng_) in zip(frames, eager):
                buf.copy_(torch.from_numpy(f))
                out = m.process_frame(buf, target=0, restore=True, normalize=True, fmt="rgba", out=out)
                torch.cuda.synchronize()
                assert torch.equal(_bits(out.display), _bits(disp)) and torch.equal(_bits(out.depth), _bits(depth)), rep
                assert torch.equal(_bits(out.depth_range), _bits(rng_))
        allocs = m.query("allocs")
        for f in frames:  # host frames stage through the grow-only pinned buffer
            m.process_frame(f, target=0, restore=True, normalize=True, fmt="rgba", out=out)
        allocs_host = m.query("allocs")
        for f in frames:
            r = m.process_frame(f, target=0, restore=True, normalize=True, fmt="rgba", out=out)
        torch.cuda.synchronize()
        assert m.query("allocs") == allocs_host
        assert torch.equal(_bits(r.display), _bits(eager[-1][0]))
        assert allocs_host - allocs <= 2  # the staging buffers of the first host frame, nothing more
    finally:
        m.enable_graph(False)
        m.destroy()


@pytest.mark.gpu
def test_infer_cli_on_device_writes_the_default_png(dev, tmp_path):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
    spec = importlib.util.spec_from_file_location("infer_cli", os.path.join(ROOT, "tools", "infer.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = DepthAnything3Config.small()
    ck = str(tmp_path / "da3_small.safetensors")
    Wt.save_container(ck, Wt.generate_da3_weights(cfg, 0, Wt.INIT_PARITY), dtype="F16")
    rgb = np.random.default_rng(14).integers(0, 256, (360, 640, 3), dtype=np.uint8)
    prep = P.prepare_depth_anything3_image(rgb, 518).rgb
    # fed the prepared frame, nothing is resized: the same PNG bytes. Fed the original frame, the two resizes differ by one grey
    # level on a few input pixels (the host's tensordot sums in BLAS order); the parity mode (f32) keeps that from growing
    # through the seeded network, whose bf16 mode amplifies it to several levels
    for name, img, prec in (("prep", prep, "bf16"), ("orig", rgb, "f32")):
        path = str(tmp_path / f"{name}.npy")
        np.save(path, img)
        a, b = str(tmp_path / f"{name}_host.png"), str(tmp_path / f"{name}_dev.png")
        args = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", path, "--precision", prec]
        assert cli.main(args + ["--output", a]) == 0
        assert cli.main(args + ["--output", b, "--on-device"]) == 0
        if name == "prep":
            assert open(a, "rb").read() == open(b, "rb").read()
        else:
            d = np.abs(P.read_gray_png(a).astype(np.int32) - P.read_gray_png(b).astype(np.int32))
            assert (d <= 1).mean() >= 0.999, (int(d.max()), float((d <= 1).mean()))
