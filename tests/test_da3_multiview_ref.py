"""CPU checks of tests/da3_multiview_ref.py, the fp32 restatement of multi-view Depth-Anything-v3 `small`.

* With one view per scene it is oracle.da3_ref's `small` inference, bit for bit.
* With several views the cross-view attention and the per-view camera token change the result by far more than any precision mode's
  tolerance, so a GPU parity test against it (tests/test_da3_views.py) cannot pass on an engine that runs the views as separate scenes.
"""
import functools

import pytest
import torch

import da3_multiview_ref as MV
from burn_depth_amd import weights as Wt
from burn_depth_amd.config import DepthAnything3Config
from oracle import da3_ref as D3
from oracle import depth_pro_ref as R

H, W = 126, 154          # 9 x 11 patches + cls = 100 tokens per view
SCENES, VIEWS = 2, 3
SEED_W, SEED_X = 0, 1    # seeded `small` weights (INIT_PARITY) and input; the margins below hold for this pair
# run_da3 (tools/gpu_diag.py) holds the f16x2 depth of `small` to max-rel 1e-3 and mean-rel 1e-4 against the fp32 oracle
F16X2_DEPTH_MAX_REL, F16X2_DEPTH_MEAN_REL = 1e-3, 1e-4
FIELDS = ("depth", "depth_confidence", "aux", "aux_confidence", "pose_encoding", "extrinsics", "intrinsics")


def small_cfg():
    cfg = DepthAnything3Config.small()
    cfg.image_size, cfg.image_width = H, W
    return cfg


@functools.lru_cache(maxsize=None)
def frames():
    cfg = small_cfg()
    Wd = R.weights_to_torch(Wt.generate_da3_weights(cfg, SEED_W, Wt.INIT_PARITY))
    torch.manual_seed(SEED_X)
    x = torch.randn(SCENES, VIEWS, 3, H, W)
    with torch.no_grad():
        dbg = {}
        multi = MV.infer_views(x, Wd, cfg, debug=dbg)
        single = D3.infer(x.reshape(SCENES * VIEWS, 3, H, W), Wd, cfg)
        one_view = MV.infer_views(x.reshape(SCENES * VIEWS, 1, 3, H, W), Wd, cfg)
    return cfg, x, multi, single, one_view, dbg


def same(a, b):  # bit-identical, a NaN (the intrinsics' unused entries may hold none or some) at the same places
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def test_one_view_per_scene_is_the_single_view_oracle():
    _, _, _, single, one_view, _ = frames()
    for f in FIELDS:
        assert same(one_view[f], single[f]), f


def test_views_change_the_depth_far_beyond_the_f16x2_tolerance():
    _, _, multi, single, _, _ = frames()
    assert multi["depth"].shape == (SCENES * VIEWS, H, W)
    rel = (multi["depth"] - single["depth"]).abs() / single["depth"].abs()
    print(f"multi-view vs per-image depth: max-rel {rel.max().item():.3e} mean-rel {rel.mean().item():.3e}")
    assert rel.max().item() > 10 * F16X2_DEPTH_MAX_REL
    assert rel.mean().item() > 10 * F16X2_DEPTH_MEAN_REL
    for v in range(SCENES * VIEWS):  # every view, the reference views included (they see the other views' keys)
        assert rel[v].max().item() > 10 * F16X2_DEPTH_MAX_REL, v


def test_reference_and_source_views_carry_different_camera_tokens():
    cfg, _, _, _, _, dbg = frames()
    t0 = dbg["tok0_block_out"]
    assert t0.shape == (SCENES * VIEWS, cfg.vit().embed_dim)
    for s in range(SCENES):
        assert not torch.equal(t0[s * VIEWS], t0[s * VIEWS + 1])
        assert (t0[s * VIEWS] - t0[s * VIEWS + 1]).abs().max().item() > 1e-3


def test_scenes_do_not_see_each_other():
    cfg, x, multi, _, _, _ = frames()
    Wd = R.weights_to_torch(Wt.generate_da3_weights(cfg, SEED_W, Wt.INIT_PARITY))
    with torch.no_grad():
        alone = MV.infer_views(x[:1], Wd, cfg)
    assert torch.allclose(alone["depth"], multi["depth"][:VIEWS], rtol=1e-5, atol=0)


def test_mono_variant_is_rejected():
    with pytest.raises(ValueError):
        MV.infer_views(torch.zeros(1, 2, 3, 14, 14), {}, DepthAnything3Config.tiny_test())
