"""GPU tests of multi-view Depth-Anything-v3 `small` (`md_da3_infer_views`) against the fp32 restatement
tests/da3_multiview_ref.py: parity in the three 16-bit modes with the tolerances run_da3 (tools/gpu_diag.py) applies to the single-view
`small` run of each mode, V = 1 against md_da3_infer_ex, scene independence, graph replay and the error returns.

Shapes: 2 scenes x 3 views at 126 x 154 (9 x 11 patches + cls = 100 tokens per view: two key tiles per view, the second partial, the
view boundary inside a tile's over-read). tests/test_da3_multiview_ref.py shows that the views change the depth by 1.3e-1 max-rel /
2.0e-2 mean-rel at these seeds, above every bound below."""
import ctypes as C
import functools

import pytest
import torch

import da3_multiview_ref as MV
from oracle import depth_pro_ref as R

pytestmark = pytest.mark.gpu

H, W, SCENES, VIEWS = 126, 154, 2, 3
N = SCENES * VIEWS
FIELDS = ("depth", "depth_confidence", "aux", "aux_confidence", "pose_encoding", "extrinsics", "intrinsics")


@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def small_cfg(precision, max_batch=N):
    from burn_depth_amd.config import DepthAnything3Config
    cfg = DepthAnything3Config.small()
    cfg.image_size, cfg.image_width = H, W
    cfg.precision, cfg.max_batch = precision, max_batch
    return cfg


def new_model(dev, precision, f16_weights=False, max_batch=N):
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.depth_anything3 import DepthAnything3
    m = DepthAnything3.new(dev, small_cfg(precision, max_batch), seed=0, init_scheme=Wt.INIT_PARITY)
    return m.round_weights_to_f16() if f16_weights else m


def seeded_views():
    torch.manual_seed(1)
    return torch.randn(SCENES, VIEWS, 3, H, W)


@functools.lru_cache(maxsize=None)
def reference(f16_weights):
    """One fp32 frame per weight set, shared by the precisions that use it."""
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import Precision
    cfg = small_cfg(Precision.F32)
    Wd = R.weights_to_torch(Wt.generate_da3_weights(cfg, 0, Wt.INIT_PARITY))
    if f16_weights:
        Wd = {k: R.f16_round(v) for k, v in Wd.items()}
    with torch.no_grad():
        return MV.infer_views(seeded_views(), Wd, cfg)


def same(a, b):  # bit-identical, NaN (unused intrinsics entries) at the same places
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=1.0), torch.nan_to_num(b, nan=1.0))


@pytest.mark.parametrize("mode", ["f16x2", "f16", "bf16"])
def test_views_parity_against_the_fp32_restatement(dev, mode):
    """Tolerances: run_da3's for the single-view `small` run of the mode (tools/gpu_diag.py:841-865) -- depth max-rel / mean-rel
    bf16 8e-2 / 1e-2, f16 1.2e-2 / 1.5e-3, f16x2 1e-3 / 1e-4 and the reference's own bar (max-abs 5e-3, mean-abs 1e-3, max-rel 1e-2);
    confidences max-rel and aux max-abs 8e-2 k (k = 1 bf16, 0.15 f16) or 1e-3 (f16x2); pose / extrinsics max-abs and intrinsics rel
    3e-2 k or 2e-4. f16x2 runs on f16-rounded weights (what the reference's records hold), on both sides."""
    from burn_depth_amd.config import Precision
    prec = {"f16x2": Precision.F16X2, "f16": Precision.F16, "bf16": Precision.BF16}[mode]
    f16w = mode == "f16x2"
    model = new_model(dev, prec, f16_weights=f16w)
    try:
        out = model.infer_views(seeded_views().cuda())
        torch.cuda.synchronize()
    finally:
        model.destroy()
    ref = reference(f16w)
    d, rd = out.depth.cpu(), ref["depth"]
    assert d.shape == (N, H, W) and bool(torch.isfinite(d).all())
    rel = (d - rd).abs() / rd.abs()
    tol = {"bf16": (8e-2, 1e-2), "f16": (1.2e-2, 1.5e-3)}.get(mode, (1e-3, 1e-4))
    print(f"da3 views {mode}: depth max-rel {rel.max().item():.3e} (bound {tol[0]:.1e}) mean-rel {rel.mean().item():.3e} (bound {tol[1]:.1e}) "
          f"max-abs {(d - rd).abs().max().item():.3e} mean-abs {(d - rd).abs().mean().item():.3e}")
    assert rel.max().item() <= tol[0]
    assert rel.mean().item() <= tol[1]
    if mode == "f16x2":
        assert (d - rd).abs().max().item() <= 5e-3 and (d - rd).abs().mean().item() <= 1e-3 and rel.max().item() <= 1e-2
    k = {"bf16": 1.0, "f16": 0.15}.get(mode, 0.0)
    t_rel, t_abs, t_pose = (8e-2 * k or 1e-3), (8e-2 * k or 1e-3), (3e-2 * k or 2e-4)
    for name, rt, at in (("depth_confidence", t_rel, 0.0), ("aux_confidence", t_rel, 0.0), ("aux", 0.0, t_abs), ("pose_encoding", 0.0, t_pose),
                         ("extrinsics", 0.0, t_pose)):
        g, w = getattr(out, name).cpu(), ref[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        err = ((g - w).abs() / w.abs()).max().item() if rt else (g - w).abs().max().item()
        print(f"da3 views {mode}: {name} {'max-rel' if rt else 'max-abs'} {err:.3e} (bound {rt or at:.1e})")
        assert err <= (rt or at), name
    g, w = out.intrinsics.cpu(), ref["intrinsics"]
    fin = torch.isfinite(w)
    assert torch.equal(torch.isfinite(g), fin)
    assert ((g[fin] - w[fin]).abs().max() / (w[fin].abs().max() + 1e-12)).item() <= t_pose


@pytest.fixture(scope="module")
def f16x2_model(dev):
    from burn_depth_amd.config import Precision
    m = new_model(dev, Precision.F16X2, f16_weights=True)
    yield m
    m.destroy()


def test_one_view_per_scene_is_infer_ex(f16x2_model):
    x = seeded_views().reshape(N, 3, H, W).cuda()
    a = f16x2_model.infer_views(x.reshape(N, 1, 3, H, W))
    b = f16x2_model.infer(x)
    for f in FIELDS:
        assert same(getattr(a, f), getattr(b, f)), f


def test_views_differ_from_separate_scenes_and_scenes_are_independent(f16x2_model):
    x = seeded_views().cuda()
    a = f16x2_model.infer_views(x)
    per_image = f16x2_model.infer(x.reshape(N, 3, H, W))
    assert ((a.depth - per_image.depth).abs() / per_image.depth.abs()).max().item() > 1e-2
    y = x.clone()
    torch.manual_seed(7)
    y[1] = torch.randn(VIEWS, 3, H, W).cuda()
    b = f16x2_model.infer_views(y)
    for f in FIELDS:
        assert same(getattr(a, f)[:VIEWS], getattr(b, f)[:VIEWS]), f
    assert not torch.equal(a.depth[VIEWS:], b.depth[VIEWS:])


def test_graph_replay_equals_eager_and_allocates_nothing(dev):
    from burn_depth_amd import _lib
    from burn_depth_amd.config import Precision
    eager, graph = new_model(dev, Precision.BF16), new_model(dev, Precision.BF16)
    try:
        graph.enable_graph(True)
        x = seeded_views().cuda()
        want = eager.infer_views(x)
        f = lambda *s: torch.empty(s, device="cuda")  # noqa: E731
        depth, conf, pose, extr, intr = f(N, H, W), f(N, H, W), f(N, 1, 9), f(N, 1, 3, 4), f(N, 1, 3, 3)
        o = _lib.MdDa3Outputs(depth.data_ptr(), conf.data_ptr(), None, None, pose.data_ptr(), extr.data_ptr(), intr.data_ptr())

        def run(V):
            _lib.check(_lib.load().md_da3_infer_views(graph._h, C.c_void_p(x.data_ptr()), N // V, V, H, W, _lib.MD_MEM_DEVICE, C.byref(o),
                                                      _lib.MD_MEM_DEVICE, None))
            torch.cuda.synchronize()
        run(VIEWS)  # eager
        allocs = graph.query("allocs")
        for step in range(3):  # capture, replay, replay
            depth.fill_(-1.0)
            run(VIEWS)
            assert torch.equal(depth, want.depth) and torch.equal(conf, want.depth_confidence) and torch.equal(pose, want.pose_encoding), step
            assert same(extr, want.extrinsics) and same(intr, want.intrinsics), step
            assert graph.query("allocs") == allocs, step
        # the same pointers with another grouping are another graph: V is part of the replay key
        run(1)
        assert torch.equal(depth, eager.infer(x.reshape(N, 3, H, W)).depth)
        run(VIEWS)
        assert torch.equal(depth, want.depth)
    finally:
        eager.destroy()
        graph.destroy()


def test_error_returns(dev, f16x2_model):
    from burn_depth_amd import _lib, weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    x = torch.zeros(SCENES + 1, VIEWS, 3, H, W, device="cuda")
    with pytest.raises(_lib.MdError) as e:  # 9 images, max_batch 6
        f16x2_model.infer_views(x)
    assert e.value.code == _lib.MD_ERR_SHAPE
    with pytest.raises(_lib.MdError) as e:  # caller cameras: one encoder token per image, not per view
        f16x2_model.infer_views(x[:2], extrinsics=torch.zeros(2, 1, 3, 4), intrinsics=torch.zeros(2, 1, 3, 3))
    assert e.value.code == _lib.MD_ERR_UNSUPPORTED
    f32 = new_model(dev, Precision.F32)
    try:
        with pytest.raises(_lib.MdError) as e:  # the fp32 parity mode attends through its own three-launch path
            f32.infer_views(x[:2])
        assert e.value.code == _lib.MD_ERR_UNSUPPORTED
        assert f32.infer_views(x[:2].reshape(N, 1, 3, H, W)).depth.shape == (N, H, W)  # one view per scene is plain infer
    finally:
        f32.destroy()
    mcfg = DepthAnything3Config.metric_large()  # the mono head: no global blocks
    mcfg.image_size = 70
    mcfg.max_batch = 2
    mono = DepthAnything3.new(dev, mcfg, seed=0, init_scheme=Wt.INIT_PARITY)
    try:
        s = mcfg.image_size
        with pytest.raises(_lib.MdError) as e:
            mono.infer_views(torch.zeros(1, 2, 3, s, s, device="cuda"))
        assert e.value.code == _lib.MD_ERR_UNSUPPORTED
        assert mono.infer_views(torch.zeros(2, 1, 3, s, s, device="cuda")).depth.shape == (2, s, s)
    finally:
        mono.destroy()
