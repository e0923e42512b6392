"""Multi-view Depth-Anything-v3 `small` in fp32 torch: the restatement the multi-view engine path is tested against.

PARITY STATUS: like the single-view backbone extras of oracle/da3_ref.py this is **unpinned**: the reference tree sets burn_dino's
switches and only ever passes one view, so what several views mean is restated from the public Depth-Anything-3 model definition:

  * input [B, V, 3, H, W]; view 0 of a scene is its reference view (no reference-view reordering);
  * patch embedding, cls + position embedding, the blocks before `ext_block_start` and the LOCAL blocks run per view (B*V sequences),
    exactly as oracle.da3_ref.backbone_hooks_ext runs them;
  * entering block `ext_block_start`, token 0 of view 0 becomes camera_token[:, 0], token 0 of views 1 .. V-1 camera_token[:, 1];
  * in a GLOBAL block (odd index >= ext_block_start) every query of a view attends over the V * N tokens of all views of its scene,
    taken in view order, with one softmax over all of them; q/k-norm and the "no-diff" RoPE positions stay per token (cls slot (0, 0),
    patches (1, 1)), and so do LayerNorm, QKV, proj, the MLP and the hook rules (local_x, cat, final norm on the second half);
  * the dual head and the camera decoder run per view: every output is [B*V, ...] in (scene, view) order.

With V = 1 every statement below is the statement oracle.da3_ref.backbone_hooks_ext executes, so the results are equal bit for bit
(tests/test_da3_multiview_ref.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import da3_ref as R
from oracle.depth_pro_ref import identity, interpolate_pos_encoding, linear_quantisers, round_q_prescaled


def backbone_hooks_views(x, W, cfg, views: int, q=identity, debug=None):
    """x [B*V, 3, H, W] scene-major -> (hooks: 4 x [B*V, P, 2D], camera feature [B*V, 2D]) as oracle.da3_ref.backbone_hooks_ext.
    debug (a dict): "tok0_block_out" = the token-0 rows [B*V, D] behind block `ext_block_start`."""
    qn, qo, qh, qw = linear_quantisers(q, False)
    v = cfg.vit()
    bp = "backbone.pretrained"
    p = lambda n: W[f"{bp}.{n}"]
    BV = x.shape[0]
    V = int(views)
    assert V >= 1 and BV % V == 0
    B = BV // V
    D, Hn, hd = v.embed_dim, v.num_heads, v.head_dim
    gh, gw = x.shape[2] // v.patch_size, x.shape[3] // v.patch_size
    tok = F.conv2d(q(x), q(p("patch_embed.proj.weight")), p("patch_embed.proj.bias"), stride=v.patch_size).flatten(2).transpose(1, 2)
    xs = torch.cat([p("cls_token").expand(BV, 1, D), tok], 1) + interpolate_pos_encoding(p("pos_embed"), gh, gw)
    N = xs.shape[1]
    yy, xx = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    pos_l = torch.cat([torch.zeros(1, 2, dtype=torch.long), torch.stack([yy.reshape(-1), xx.reshape(-1)], 1) + 1], 0)
    pos_g = torch.cat([torch.zeros(1, 2, dtype=torch.long), torch.ones(gh * gw, 2, dtype=torch.long)], 0)
    start = cfg.ext_block_start
    local_x = xs
    raw = {}

    def scene_keys(t):
        """[B*V, heads, N, hd] -> every view sees its scene's V*N rows in view order: [B*V, heads, V*N, hd]."""
        if V == 1:
            return t
        s = t.reshape(B, V, Hn, N, hd).permute(0, 2, 1, 3, 4).reshape(B, 1, Hn, V * N, hd)
        return s.expand(B, V, Hn, V * N, hd).reshape(BV, Hn, V * N, hd)

    for i in range(v.depth):
        b = f"blocks.{i}"
        ext = start >= 0 and i >= start
        if ext and i == start:
            if V == 1:
                cam_tok = p("camera_token")[:, :1].expand(BV, 1, D)
            else:  # slot 0 for the reference view, slot 1 for every other view
                ct = p("camera_token")
                per_scene = torch.cat([ct[:, :1], ct[:, 1:2].expand(1, V - 1, D)], 1)  # [1, V, D]
                cam_tok = per_scene.expand(B, V, D).reshape(BV, 1, D)
            xs = torch.cat([cam_tok, xs[:, 1:]], 1)
        is_global = ext and i % 2 == 1
        xn = qn(F.layer_norm(xs, (D,), p(f"{b}.norm1.gamma"), p(f"{b}.norm1.beta"), v.ln_eps))
        qkv = F.linear(xn, qw(p(f"{b}.attn.qkv.weight")), p(f"{b}.attn.qkv.bias"))
        qkv = qkv.reshape(BV, N, 3, Hn, hd).permute(2, 0, 3, 1, 4)
        qq, kk, vv = round_q_prescaled(qkv[0], q), q(qkv[1]), q(qkv[2])
        if ext:
            pos = pos_g if is_global else pos_l
            qq = F.layer_norm(qq, (hd,), p(f"{b}.attn.q_norm.gamma"), p(f"{b}.attn.q_norm.beta"), cfg.qk_norm_eps)
            kk = F.layer_norm(kk, (hd,), p(f"{b}.attn.k_norm.gamma"), p(f"{b}.attn.k_norm.beta"), cfg.qk_norm_eps)
            qq, kk = round_q_prescaled(R.rope2d(qq, pos, cfg.rope_frequency), q), q(R.rope2d(kk, pos, cfg.rope_frequency))
        if is_global:
            kk, vv = scene_keys(kk), scene_keys(vv)
        sc = (qq @ kk.transpose(-2, -1)) * hd ** -0.5
        pu = torch.exp(sc - sc.amax(-1, keepdim=True))
        o = (q(pu) @ vv) / pu.sum(-1, keepdim=True)
        o = qo(o.transpose(1, 2).reshape(BV, N, D))
        xs = xs + p(f"{b}.ls1.gamma") * F.linear(o, qw(p(f"{b}.attn.proj.weight")), p(f"{b}.attn.proj.bias"))
        xn = qn(F.layer_norm(xs, (D,), p(f"{b}.norm2.gamma"), p(f"{b}.norm2.beta"), v.ln_eps))
        h = qh(F.gelu(F.linear(xn, qw(p(f"{b}.mlp.fc1.weight")), p(f"{b}.mlp.fc1.bias"))))
        xs = xs + p(f"{b}.ls2.gamma") * F.linear(h, qw(p(f"{b}.mlp.fc2.weight")), p(f"{b}.mlp.fc2.bias"))
        if debug is not None and ext and i == start:
            debug["tok0_block_out"] = xs[:, 0].clone()
        if not is_global:
            local_x = xs
        if i in cfg.hook_block_ids:
            raw[i] = torch.cat([local_x, xs], -1)
    hooks, cam = [], None
    for i in cfg.hook_block_ids:
        r = raw[i]
        hooks.append(torch.cat([r[..., :D], F.layer_norm(r[..., D:], (D,), p("norm.gamma"), p("norm.beta"), v.ln_eps)], -1)[:, 1:])
        cam = r[:, 0]
    return hooks, cam


def infer_views(x, W, cfg, q=identity, debug=None):
    """x [B, V, 3, H, W] -> the dict of oracle.da3_ref.infer with every entry [B*V, ...] in (scene, view) order."""
    if not cfg.dual_head:
        raise ValueError("multi-view inference needs the extended backbone (the `small` variant)")
    B, V, _, H, Wd = x.shape
    ps = cfg.patch_size
    if H % ps or Wd % ps:
        raise ValueError(f"Input {H}x{Wd} must be divisible by patch size {ps}")
    hooks, cam = backbone_hooks_views(x.reshape(B * V, 3, H, Wd), W, cfg, V, q, debug)
    out = R.dual_head_forward(hooks, H, Wd, W, cfg, q, None)
    out.update(R.camera_decode(cam, W, H, Wd))
    return out
