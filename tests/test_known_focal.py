"""Depth Pro with a known focal length: md_depth_pro_infer_with_focal / md_infer_from_rgb_with_focal / md_op_focal_to_fov and
their Python mirror (`DepthPro.infer(x, f_px)`, Apple ml-depth-pro's `infer(x, f_px)`).

With the caller's f_px the FOV encoder and head do not run; focallength_px is f_px, fovx = 2 atan(W / 2 f_px), fovy comes from that
fovx through the reference's `fovy_from_fovx_rad` (depth_pro/mod.rs:370-414), and depth follows mod.rs:330-363 with ratio = W / f_px.
The CPU tests need no GPU; the others run with `-m gpu` on an MI355X."""
import ctypes as C
import math
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
from oracle import depth_pro_ref as R  # noqa: E402

NEW_ENTRIES = ("md_depth_pro_infer_with_focal", "md_infer_from_rgb_with_focal", "md_op_focal_to_fov")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_known_focal_entries(lib):
    header = open(os.path.join(ROOT, "include", "mi_depth.h")).read()
    declared = set(re.findall(r"^int\s+(md_[a-z0-9_]+)\s*\(", header, re.M))
    raw = C.CDLL(os.path.join(ROOT, "burn_depth_amd", "libmi_depth.so"))
    for name in NEW_ENTRIES:
        assert name in declared, f"include/mi_depth.h does not declare {name}"
        assert hasattr(raw, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS


def _focal_to_fov(lib, f, h, w):
    fx, fy = C.c_float(), C.c_float()
    code = lib.md_op_focal_to_fov(C.c_float(f), h, w, C.byref(fx), C.byref(fy))
    return code, fx.value, fy.value


def test_focal_to_fov_against_fp64_and_the_oracle(lib):
    for h, w in [(512, 512), (360, 540), (540, 360), (1536, 1536), (1, 4000)]:
        for f in (1.0, 37.5, 0.3 * w, 0.87 * w, float(w), 2.5 * w, 40.0 * w):
            code, fovx, fovy = _focal_to_fov(lib, f, h, w)
            assert code == 0
            want = 2.0 * math.atan(0.5 * w / float(np.float32(f))) * 180.0 / math.pi
            assert abs(fovx - want) <= 2e-6 * abs(want), (f, h, w, fovx, want)
            # fovy: the reference's approximation of 2 atan((H/W) tan(fovx/2)) on this fovx, to the tolerance of the predicting path's
            # tail test (tests/test_host_abi.py::test_fov_scalar_tail_matches_oracle)
            fx = torch.tensor([fovx], dtype=torch.float32) * torch.tensor(math.pi / 180.0, dtype=torch.float32)
            ref = R.fovy_from_fovx_rad(fx, h, w).item()
            assert abs(fovy - ref) <= 1e-6, (f, h, w, fovy, ref)
    # the inverse of md_op_fov_to_focal
    for deg in (30.0, 56.4, 75.5, 100.0):
        focal, _ = C.c_float(), C.c_float()
        assert lib.md_op_fov_to_focal(C.c_float(deg), 512, 512, C.byref(focal), None) == 0
        _, fovx, _ = _focal_to_fov(lib, focal.value, 512, 512)
        assert abs(fovx - deg) <= 1e-5 * deg


def test_focal_to_fov_rejects_bad_values(lib):
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        code, _, _ = _focal_to_fov(lib, bad, 512, 512)
        assert code == _lib.MD_ERR_INVALID_ARG, bad
    assert _focal_to_fov(lib, 100.0, 0, 512)[0] == _lib.MD_ERR_SHAPE


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def _tiny_no_fov_vit():
    from burn_depth_amd.config import DepthProConfig, TINY16_128
    return DepthProConfig(TINY16_128, TINY16_128, 64, None, None)  # a FOV head without its own ViT (fov.rs:118-155)


def _model(dev, cfg, precision, B):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.depth_pro import DepthPro
    cfg.precision = precision
    cfg.max_batch = B
    return DepthPro.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _input(B, H, W, seed=0):
    torch.manual_seed(seed)
    return (torch.rand(B, 3, H, W) - torch.tensor(R.MEAN).view(1, 3, 1, 1)) / torch.tensor(R.STD).view(1, 3, 1, 1)


def _rel(a, b):
    return ((a - b).abs() / b.abs()).max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["tiny", "small", "tiny_no_fov_vit"])
@pytest.mark.parametrize("precision", [1, 0, 3, 4])
def test_known_focal_round_trip_is_bit_identical(dev, preset, precision):
    """f_px = the predicted focal length -> the predicting call's depth and focal length, bit for bit (the ViT without the FOV row
    group computes the same bits for the other groups; ratio = W / f is the same division)."""
    from burn_depth_amd.config import DepthProConfig
    cfg = {"tiny": DepthProConfig.tiny_test, "small": DepthProConfig.small_test, "tiny_no_fov_vit": _tiny_no_fov_vit}[preset]()
    m = _model(dev, cfg, precision, 2)
    S = m.img_size()
    try:
        for H, W in ((S, S), (360, 540)):
            x = _input(2, H, W, seed=H).cuda()
            a = m.infer(x)
            b = m.infer(x, f_px=a.focallength_px)
            torch.cuda.synchronize()
            assert torch.equal(b.depth, a.depth), (H, W)
            assert torch.equal(b.focallength_px, a.focallength_px)
            assert _rel(b.fovx_deg, a.fovx_deg) <= 1e-5 and _rel(b.fovy_rad, a.fovy_rad) <= 1e-5
    finally:
        m.destroy()


def _oracle_known_focal(x, W, cfg, f_px):
    """mod.rs:330-363 with the caller's focal length: canonical x W / f_px, resize back, clamp, reciprocal."""
    B, _, H, Wd = x.shape
    S = cfg.img_size()
    xin = R.resize_bilinear(x, (S, S), cfg.interpolation) if (H, Wd) != (S, S) else x
    with torch.no_grad():
        canonical = R.forward_debug(xin, W, cfg)["canonical"]
    f = torch.as_tensor(f_px, dtype=torch.float32).reshape(B)
    ratio = (torch.ones_like(f) * float(Wd)) / f
    inv = canonical * ratio.reshape(B, 1, 1, 1)
    if (H, Wd) != (S, S):
        inv = R.resize_bilinear(inv, (H, Wd), cfg.interpolation)
    return (1.0 / inv.clamp(1e-4, 1e4)).squeeze(1)


def _weights(cfg):
    from burn_depth_amd import weights as Wt
    return R.weights_to_torch(Wt.generate_depth_pro_weights(cfg, 0, Wt.INIT_PARITY))


E2E_F32_MAX_REL = 1e-3  # the tiny fp32 end-to-end bar (tools/gpu_diag.py E2E_TOL[F32])


@pytest.mark.gpu
def test_known_focal_against_the_oracle(dev):
    from burn_depth_amd.config import DepthProConfig
    cfg = DepthProConfig.tiny_test()
    m = _model(dev, cfg, 1, 2)
    try:
        x = _input(2, 360, 540, seed=5)
        pred = m.infer(x.cuda()).focallength_px.cpu()
        f_px = torch.stack([pred[0] * 0.5, pred[1] * 3.0])
        out = m.infer(x.cuda(), f_px=f_px.cuda())
        want = _oracle_known_focal(x, _weights(cfg), cfg, f_px)
        assert _rel(out.depth.cpu(), want) < E2E_F32_MAX_REL
        assert torch.equal(out.focallength_px.cpu(), f_px)
        fovx = 2.0 * torch.atan(540.0 * 0.5 / f_px.double()) * 180.0 / math.pi
        assert _rel(out.fovx_deg.cpu().double(), fovx) <= 2e-6
    finally:
        m.destroy()


@pytest.mark.gpu
def test_model_without_fov_head_infers_with_a_known_focal_length(dev):
    from burn_depth_amd.config import DepthProConfig
    cfg = DepthProConfig.tiny_test()
    cfg.use_fov_head = False
    m = _model(dev, cfg, 1, 2)
    try:
        x = _input(2, 360, 540, seed=6)
        with pytest.raises(_lib.MdError) as e:
            m.infer(x.cuda())
        assert e.value.code == _lib.MD_ERR_NO_FOV
        f_px = [420.0, 1300.0]
        out = m.infer(x.cuda(), f_px=f_px)
        want = _oracle_known_focal(x, _weights(cfg), cfg, f_px)
        assert _rel(out.depth.cpu(), want) < E2E_F32_MAX_REL
        assert out.focallength_px.cpu().tolist() == f_px
    finally:
        m.destroy()


@pytest.mark.gpu
def test_known_focal_schedule_leaves_out_the_fov_network(dev):
    from burn_depth_amd.config import DepthProConfig
    m = _model(dev, DepthProConfig.tiny_test(), 0, 2)
    try:
        x = _input(2, 512, 512).cuda()
        m.infer(x)  # warm (index tables, first launches)
        m.enable_timing(True)

        def order(f_px=None):
            m.infer(x, f_px=f_px)
            torch.cuda.synchronize()
            names = m.read_launch_order()
            m.read_timing()  # clears the record
            return names

        plain = order()
        known = order(300.0)
        plain2 = order()
        m.enable_timing(False)
    finally:
        m.destroy()
    assert "fov_post" in plain and any(n.startswith("fov_") and n != "fov_post" for n in plain)
    assert not [n for n in known if n.startswith("fov")], known
    assert known.count("focal_post") == 1 and "focal_post" not in plain
    assert plain2 == plain
    # the same launches otherwise: the ViT's row groups run in the same launches, one group fewer
    assert [n for n in known if n != "focal_post"] == [n for n in plain if not n.startswith("fov_")]


@pytest.mark.gpu
def test_known_focal_from_host_memory(dev):
    from burn_depth_amd.config import DepthProConfig
    m = _model(dev, DepthProConfig.tiny_test(), 0, 2)
    lib = _lib.load()
    B, H, W = 2, 360, 540
    x = _input(B, H, W, seed=7).numpy()
    fh = np.array([333.0, 777.0], np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(f):
        depth = np.full((B, H, W), -1.0, np.float32)
        focal, fovx, fovy = (np.zeros(B, np.float32) for _ in range(3))
        code = lib.md_depth_pro_infer_with_focal(m._h, p(x), B, H, W, _lib.MD_MEM_HOST, p(f), p(depth), p(focal), p(fovx), p(fovy),
                                                 _lib.MD_MEM_HOST, None)
        return code, depth, focal, fovx, fovy

    try:
        code, d0, f, fx, fy = call(fh)
        assert code == 0
        want = m.infer(torch.from_numpy(x).cuda(), f_px=torch.from_numpy(fh).cuda())
        assert np.array_equal(d0, want.depth.cpu().numpy()) and np.array_equal(f, fh)
        assert np.array_equal(fx, want.fovx_deg.cpu().numpy()) and np.array_equal(fy, want.fovy_rad.cpu().numpy())
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            code, d, *_ = call(np.array([500.0, bad], np.float32))
            assert code == _lib.MD_ERR_INVALID_ARG, bad
            assert (d == -1.0).all()
        allocs = m.query("allocs")
        for i in range(3):
            code, d2, *_ = call(fh * np.float32(1 + i))
            assert code == 0
        assert m.query("allocs") == allocs, "a repeated host-pointer known-focal call must not allocate"
        assert np.array_equal(call(fh)[1], d0)
    finally:
        m.destroy()


@pytest.mark.gpu
def test_known_focal_graph_replay_reads_the_focal_buffer_at_run_time(dev):
    from burn_depth_amd.config import DepthProConfig
    g = _model(dev, DepthProConfig.tiny_test(), 0, 2)
    e = _model(dev, DepthProConfig.tiny_test(), 0, 2)
    try:
        x = _input(2, 512, 512, seed=8).cuda()
        v1 = torch.tensor([250.0, 600.0], device="cuda")
        v2 = torch.tensor([900.0, 180.0], device="cuda")
        f = v1.clone()
        bufs = [torch.empty(2, 512, 512, device="cuda")] + [torch.empty(2, device="cuda") for _ in range(3)]
        pbufs = [torch.empty(2, 512, 512, device="cuda")] + [torch.empty(2, device="cuda") for _ in range(3)]
        g.enable_graph(True)
        want1, want2, want_plain = e.infer(x, f_px=v1), e.infer(x, f_px=v2), e.infer(x)
        assert not torch.equal(want1.depth, want2.depth)
        for _ in range(2):  # eager, then captured
            g.infer_into(x, *bufs, f_px=f)
        torch.cuda.synchronize()
        assert torch.equal(bufs[0], want1.depth) and torch.equal(bufs[1], v1)
        f.copy_(v2)
        g.infer_into(x, *bufs, f_px=f)  # replayed: reads v2
        torch.cuda.synchronize()
        assert torch.equal(bufs[0], want2.depth) and torch.equal(bufs[1], v2)
        assert torch.equal(bufs[2], want2.fovx_deg) and torch.equal(bufs[3], want2.fovy_rad)
        for i in range(3):  # plain and known-focal calls alternating on one graph-enabled model
            g.infer_into(x, *pbufs)
            g.infer_into(x, *bufs, f_px=f)
            torch.cuda.synchronize()
            assert torch.equal(pbufs[0], want_plain.depth) and torch.equal(pbufs[1], want_plain.focallength_px), i
            assert torch.equal(bufs[0], want2.depth), i
    finally:
        g.destroy()
        e.destroy()


@pytest.mark.gpu
def test_known_focal_rgb_path_and_forks(dev):
    from burn_depth_amd.config import DepthProConfig
    from burn_depth_amd.inference import infer_from_rgb, rgb_to_input_tensor
    m = _model(dev, DepthProConfig.tiny_test(), 0, 2)
    fork = m.fork()
    try:
        w, h = 54, 36
        rgb = bytes(np.random.RandomState(3).randint(0, 256, size=w * h * 3, dtype=np.uint8).tolist())
        a = m.infer_from_rgb(rgb, w, h, f_px=48.5)
        b = m.infer(rgb_to_input_tensor(rgb, w, h, dev), f_px=48.5)
        torch.cuda.synchronize()
        assert torch.equal(a.depth, b.depth) and torch.equal(a.focallength_px, b.focallength_px)
        assert torch.equal(a.fovy_rad, b.fovy_rad) and a.focallength_px.item() == 48.5
        p = infer_from_rgb(m, rgb, w, h, f_px=48.5)
        assert torch.equal(p.depth, a.depth) and p.focallength_px.item() == 48.5
        x = _input(2, 512, 512, seed=9).cuda()
        fa = fork.infer(x, f_px=[300.0, 410.0])
        ra = m.infer(x, f_px=[300.0, 410.0])
        torch.cuda.synchronize()
        assert torch.equal(fa.depth, ra.depth) and torch.equal(fa.fovx_deg, ra.fovx_deg)
    finally:
        fork.destroy()
        m.destroy()


@pytest.mark.gpu
def test_known_focal_taps_do_not_report_an_earlier_fov(dev):
    from burn_depth_amd.config import DepthProConfig
    m = _model(dev, DepthProConfig.tiny_test(), 1, 1)
    try:
        x = _input(1, 512, 512).cuda()
        m.enable_taps(True)
        m.infer(x)
        assert m.read_tap("fov_deg").size == 1
        m.infer(x, f_px=200.0)
        with pytest.raises(_lib.MdError) as e:
            m.read_tap("fov_deg")
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        m.read_tap("canonical_inverse_depth")
        m.enable_taps(False)
    finally:
        m.destroy()


@pytest.mark.gpu
def test_attention_redo_list_survives_a_known_focal_call(dev):
    """A known-focal call runs 36 of the 37 sequences of B = 1 through the ViT. The assembly attention kernel's compacted redo list
    must not land on flag slots of the FOV sequence, which a later plain call would read as raised (re-running those units in the
    running-maximum body, another count and other bits)."""
    from burn_depth_amd.config import DepthProConfig
    lib = _lib.load()
    m = _model(dev, DepthProConfig(), 0, 1)
    try:
        D = 1024
        for name in ("encoder.image_encoder.blocks.0.attn.qkv.weight", "encoder.image_encoder.blocks.0.attn.qkv.bias"):
            n = 3 * D * D if name.endswith("weight") else 3 * D
            w = m.get_tensor(name, n).copy()
            w[: 2 * (n // 3)] *= np.float32(16.0)  # q and k: logits x 256, far outside the fast body's range
            m.set_tensor(name, w)
        m.commit_weights()
        x = _input(1, 1536, 1536, seed=10).cuda()
        assert lib.md_debug_attention_redo_units(dev.handle, 1) >= 0, "the assembly kernel's code object is not loaded"
        a = m.infer(x)
        n1 = int(lib.md_debug_attention_redo_units(dev.handle, 1))
        k = m.infer(x, f_px=a.focallength_px)
        n2 = int(lib.md_debug_attention_redo_units(dev.handle, 1))
        b = m.infer(x)
        n3 = int(lib.md_debug_attention_redo_units(dev.handle, 1))
        assert n1 > 0 and n2 > 0, (n1, n2)
        assert n3 == n1, (n1, n2, n3)
        assert torch.equal(b.depth, a.depth) and torch.equal(b.focallength_px, a.focallength_px)
        assert torch.equal(k.depth, a.depth)
    finally:
        m.destroy()
