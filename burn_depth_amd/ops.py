"""Stand-alone operators of libmi_depth.so on torch device tensors (used by the parity tests and
bench.py; each wraps one ``md_op_*`` entry point of include/mi_depth.h)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from .depth_pro import Device, _stream_ptr
from .points import (FittedPlanes, PointCloud, PointRegistration, RasterisedMesh, RenderedPoints, SmoothedMesh, _cluster_mode_of, _clusters_struct, _f32, _i32, _lattice,
                     _match_mode_of, _match_struct, _new_clusters, _new_match, _new_registration, _plane_mode, _planes_struct, _points_cameras, _points_request, _ptr,
                     _raster_request, _register_plane_struct, _register_struct, _render_request, _u8, _view_filter_opts)


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32c(t: torch.Tensor) -> torch.Tensor:
    assert t.is_cuda, "operators take device tensors"
    return t.contiguous().to(torch.float32)


def resize_bilinear(dev: Device, x: torch.Tensor, out_hw: Tuple[int, int], method: int = 0, post: int = 0) -> torch.Tensor:
    """post = 1: the final-depth step 1 / clamp(blend, 1e-4, 1e4) of the last resize (md_op_resize_bilinear_ex)."""
    x = _f32c(x)
    B, Cn, H, W = x.shape
    out = torch.empty((B, Cn, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_resize_bilinear_ex(dev.handle, _p(x), B, Cn, H, W, _p(out), int(out_hw[0]), int(out_hw[1]),
                                                    int(method), int(post), _stream_ptr(dev.ordinal)))
    return out


def resize_bilinear_into(dev: Device, x: torch.Tensor, out: torch.Tensor, method: int = 0) -> None:
    """Allocation-free form (bench.py): fp32 NCHW x -> out, both contiguous device tensors."""
    B, Cn, H, W = x.shape
    _lib.check(_lib.load().md_op_resize_bilinear(dev.handle, _p(x), B, Cn, H, W, _p(out), int(out.shape[2]), int(out.shape[3]),
                                                 int(method), _stream_ptr(dev.ordinal)))


_NHWC_PREC = {torch.bfloat16: 0, torch.float32: 1, torch.float16: 3}


def resize_nhwc_into(dev: Device, x: torch.Tensor, out: torch.Tensor, method: int = 1) -> None:
    """NHWC bilinear resize of the Depth-Anything-v3 head (md_op_resize_nhwc): x [B,H,W,C] -> out [B,OH,OW,C]."""
    assert x.is_cuda and out.is_cuda and x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype
    B, H, W, Cn = x.shape
    _lib.check(_lib.load().md_op_resize_nhwc(dev.handle, _p(x), B, H, W, Cn, _p(out), int(out.shape[1]), int(out.shape[2]), int(method),
                                             _NHWC_PREC[x.dtype], _stream_ptr(dev.ordinal)))


def resize_nhwc(dev: Device, x: torch.Tensor, out_hw: Tuple[int, int], method: int = 1) -> torch.Tensor:
    out = torch.empty((x.shape[0], int(out_hw[0]), int(out_hw[1]), x.shape[3]), dtype=x.dtype, device=x.device)
    resize_nhwc_into(dev, x.contiguous(), out, method)
    return out


def resize_nhwc_ex(dev: Device, x: torch.Tensor, Cn: int, out: torch.Tensor, method: int, precision: int,
                   addend: Optional[torch.Tensor] = None) -> torch.Tensor:
    """md_op_resize_nhwc_ex on raw storage: x [B, H, W, ld_in (x 2 for split-half)] -> a copy of the pre-filled raw buffer `out`
    [B, OH, OW, ld_out (x 2)] with channels 0 .. Cn of every pixel written; addend: fp32 [OH, OW, Cn] or None."""
    planes = 2 if precision == 4 else 1
    assert x.is_cuda and out.is_cuda and x.is_contiguous() and x.dtype == out.dtype == _RAW_DTYPE[precision]
    assert x.shape[3] % planes == 0 and out.shape[3] % planes == 0 and out.shape[0] == x.shape[0]
    out = out.contiguous().clone()
    B, H, W, _ = x.shape
    OH, OW = int(out.shape[1]), int(out.shape[2])
    if addend is not None:
        addend = _f32c(addend)
        assert tuple(addend.shape) == (OH, OW, Cn)
    _lib.check(_lib.load().md_op_resize_nhwc_ex(dev.handle, _p(x), B, H, W, Cn, x.shape[3] // planes, _p(out), OH, OW, out.shape[3] // planes,
                                                int(method), _p(addend), precision, _stream_ptr(dev.ordinal)))
    return out



def pyramid_patchify(dev: Device, x: torch.Tensor, window: int, patch: int = 16, method: int = 0, precision: int = 1,
                     force_generic: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pyramid + sliding-window split + patch extraction of DepthProEncoder::forward (encoder.rs:326-344) as the A matrix
    of the patch-embed GEMM (md_op_pyramid_patchify): x [B,3,S,S] fp32, S = 4 * window -> [35B * (window/patch)^2, 3 * patch^2]."""
    x = _f32c(x)
    B, _, S, _ = x.shape
    rows, cols = C.c_int(), C.c_int()
    lib = _lib.load()
    _lib.check(lib.md_op_pyramid_patchify(dev.handle, None, B, S, window, patch, method, precision, 0, None, C.byref(rows), C.byref(cols), None))
    if out is None:
        out = _raw_empty((rows.value,), cols.value, precision, x.device)   # split-half rows: [hi: cols | lo: cols]
    _lib.check(lib.md_op_pyramid_patchify(dev.handle, _p(x), B, S, window, patch, method, precision, int(force_generic), _p(out),
                                          C.byref(rows), C.byref(cols), _stream_ptr(dev.ordinal)))
    return out


def resize_output_size(H: int, W: int, scale: Tuple[float, float]) -> Tuple[int, int]:
    oh, ow = C.c_int(), C.c_int()
    _lib.check(_lib.load().md_op_resize_output_size(H, W, C.c_float(scale[0]), C.c_float(scale[1]), C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def resize_bilinear_scale(dev: Device, x: torch.Tensor, scale: Tuple[float, float], method: int = 0) -> torch.Tensor:
    return resize_bilinear(dev, x, resize_output_size(x.shape[2], x.shape[3], scale), method)


def split(dev: Device, x: torch.Tensor, window: int, overlap: float) -> Tuple[torch.Tensor, int]:
    x = _f32c(x)
    B, Cn, S, _ = x.shape
    steps = C.c_int()
    _lib.check(_lib.load().md_op_split(dev.handle, _p(x), B, Cn, S, window, C.c_float(overlap), C.c_void_p(0), C.byref(steps), None))
    out = torch.empty((steps.value * steps.value * B, Cn, window, window), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_split(dev.handle, _p(x), B, Cn, S, window, C.c_float(overlap), _p(out), C.byref(steps),
                                       _stream_ptr(dev.ordinal)))
    return out, steps.value


def merge(dev: Device, tiles: torch.Tensor, batch: int, padding: int) -> torch.Tensor:
    tiles = _f32c(tiles)
    n, Cn, h, w = tiles.shape
    oh, ow = C.c_int(), C.c_int()
    _lib.check(_lib.load().md_op_merge(dev.handle, C.c_void_p(0), n, Cn, h, w, batch, padding, C.c_void_p(0), C.byref(oh), C.byref(ow), None))
    out = torch.empty((batch, Cn, oh.value, ow.value), dtype=torch.float32, device=tiles.device)
    _lib.check(_lib.load().md_op_merge(dev.handle, _p(tiles), n, Cn, h, w, batch, padding, _p(out), C.byref(oh), C.byref(ow),
                                       _stream_ptr(dev.ordinal)))
    return out


def layernorm(dev: Device, x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float) -> torch.Tensor:
    x = _f32c(x)
    rows, D = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().md_op_layernorm(dev.handle, _p(x), _p(gamma), _p(beta), rows, D, C.c_float(eps), _p(out),
                                           _stream_ptr(dev.ordinal)))
    return out


STORAGE_OUT = 0x100  # MD_OP_STORAGE_OUT: result through the engine's storage type (bf16) instead of the fp32 store


def linear(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int = 0, precision: int = 0,
           tile: int = _lib.TILE_AUTO, storage_out: bool = False) -> torch.Tensor:
    precision |= STORAGE_OUT if storage_out else 0
    x, w = _f32c(x), _f32c(w)
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_linear_tile(dev.handle, _p(x), _p(w), _p(bias), M, N, K, act, precision, tile, _p(out),
                                             _stream_ptr(dev.ordinal)))
    return out


POISON_PAD = 0x200  # MD_OP_POISON_PAD: the attention staging's padding holds a large finite value instead of zero


def attention(dev: Device, qkv: torch.Tensor, heads: int, precision: int = 0) -> torch.Tensor:
    qkv = _f32c(qkv)
    T, N, _ = qkv.shape
    out = torch.empty((T, N, heads * 64), dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.load().md_op_attention(dev.handle, _p(qkv), T, N, heads, precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def attention_views(dev: Device, qkv: torch.Tensor, views: int, heads: int, precision: int = 0, poison_pad: bool = False) -> torch.Tensor:
    """`md_op_attention_views`: qkv [T, N, 3*heads*64], the T sequences in groups of `views`; every query attends over the
    views * N keys of its group (one softmax). views = 1 is `attention`."""
    precision |= POISON_PAD if poison_pad else 0
    qkv = _f32c(qkv)
    T, N, _ = qkv.shape
    out = torch.empty((T, N, heads * 64), dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.load().md_op_attention_views(dev.handle, _p(qkv), T, int(views), N, heads, precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def attention_ex(dev: Device, qkv: torch.Tensor, heads: int, precision: int = 0, *, views: int = 1, seq_stride: int = 0, kpad: int = 0,
                 out_fp8_inv: float = 0.0, small: int = -1, poison_pad: bool = False) -> torch.Tensor:
    """`md_op_attention_ex`: `attention` / `attention_views` with the launch parameters of the descriptor (include/mi_depth.h
    md_attention_op). out_fp8_inv > 0: the e4m3-output form, returned as the raw bytes, uint8 [T, N, heads*64]."""
    qkv = _f32c(qkv)
    T, N, _ = qkv.shape
    out = torch.empty((T, N, heads * 64), dtype=torch.uint8 if out_fp8_inv > 0 else torch.float32, device=qkv.device)
    d = _lib.MdAttentionOp(T, int(views), N, heads, precision, int(seq_stride), int(kpad), float(out_fp8_inv), int(small), int(poison_pad),
                           qkv.data_ptr(), out.data_ptr())
    _lib.check(_lib.load().md_op_attention_ex(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))
    return out


def attention_last_form() -> dict:
    """md_debug_attention_last_form: what this thread's last attention launch ran -- form (a name of _lib.ATTN_FORMS), grid, QW, KS."""
    v = (C.c_int * 4)()
    _lib.check(_lib.load().md_debug_attention_last_form(C.byref(v)))
    return {"form": _lib.ATTN_FORMS[v[0]], "grid": v[1], "QW": v[2], "KS": v[3]}


def conv3x3(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], pre_relu: bool = False,
            precision: int = 0, storage_out: bool = False) -> torch.Tensor:
    precision |= STORAGE_OUT if storage_out else 0
    x, w = _f32c(x), _f32c(w)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    out = torch.empty((B, Cout, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_conv3x3(dev.handle, _p(x), _p(w), _p(bias), B, Cin, H, W, Cout, int(pre_relu), precision,
                                         _p(out), _stream_ptr(dev.ordinal)))
    return out


def deconv2x2(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], precision: int = 0,
              storage_out: bool = False) -> torch.Tensor:
    precision |= STORAGE_OUT if storage_out else 0
    x, w = _f32c(x), _f32c(w)
    B, Cin, H, W = x.shape
    Cout = w.shape[1]
    out = torch.empty((B, Cout, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_deconv2x2(dev.handle, _p(x), _p(w), _p(bias), B, Cin, H, W, Cout, precision, _p(out),
                                           _stream_ptr(dev.ordinal)))
    return out


def conv2d_direct(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], stride: int, pad: int,
                  relu: bool) -> torch.Tensor:
    x, w = _f32c(x), _f32c(w)
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, Cout, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_conv2d_direct(dev.handle, _p(x), _p(w), _p(bias), B, Cin, H, W, Cout, k, stride, pad,
                                               int(relu), _p(out), _stream_ptr(dev.ordinal)))
    return out


def qkv_norm_rope(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, q_gamma: torch.Tensor, q_beta: torch.Tensor,
                  k_gamma: torch.Tensor, k_beta: torch.Tensor, n_tokens: int, S: int, pw: int, global_pos: bool = False,
                  rope_frequency: float = 100.0, eps: float = 1e-5, precision: int = 0, tile: int = _lib.TILE_AUTO,
                  form: int = 1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """md_op_qkv_norm_rope: x [T*S, K], w [3D, K] -> (q' [T*S, D], k' [T*S, D], V [T, S, D]); form 0 = QKV GEMM + the stand-alone
    q/k-norm + RoPE kernel, form 1 = the GEMM's fused epilogue. V is read back from the V^T layout the epilogue writes."""
    x, w = _f32c(x), _f32c(w)
    rows, K = x.shape
    D = w.shape[0] // 3
    T, heads, kpad = rows // S, D // 64, (S + 63) // 64 * 64
    assert rows == T * S and w.shape == (3 * D, K)
    qk = torch.empty((rows, 2 * D), dtype=torch.float32, device=x.device)
    vt = torch.empty((T, heads, 64, kpad), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().md_op_qkv_norm_rope(dev.handle, _p(x), _p(w), _p(_f32c(bias)), _p(_f32c(q_gamma)), _p(_f32c(q_beta)),
                                               _p(_f32c(k_gamma)), _p(_f32c(k_beta)), T, S, n_tokens, K, D, pw, int(global_pos),
                                               C.c_float(rope_frequency), C.c_float(eps), precision, tile, form, _p(qk), _p(vt),
                                               _stream_ptr(dev.ordinal)))
    v = vt[..., :S].permute(0, 3, 1, 2).reshape(T, S, D).contiguous()
    return qk[:, :D].contiguous(), qk[:, D:].contiguous(), v


def qk_norm_rope(dev: Device, qk: torch.Tensor, q_gamma: torch.Tensor, q_beta: torch.Tensor, k_gamma: torch.Tensor,
                 k_beta: torch.Tensor, n_tokens: int, S: int, pw: int, global_pos: bool = False, rope_frequency: float = 100.0,
                 eps: float = 1e-5, precision: int = 0) -> torch.Tensor:
    """md_op_qk_norm_rope: the stand-alone kernel on rows qk [T*S, 2D] = q | k (q pre-scaled by the mode's softmax scale)."""
    qk = _f32c(qk)
    rows, D2 = qk.shape
    out = torch.empty_like(qk)
    _lib.check(_lib.load().md_op_qk_norm_rope(dev.handle, _p(qk), _p(_f32c(q_gamma)), _p(_f32c(q_beta)), _p(_f32c(k_gamma)),
                                              _p(_f32c(k_beta)), rows // S, S, n_tokens, D2 // 2, pw, int(global_pos),
                                              C.c_float(rope_frequency), C.c_float(eps), precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def hook_cat_ln(dev: Device, x_local: torch.Tensor, x: torch.Tensor, n_tokens: int, S: int, norm_g: torch.Tensor, norm_b: torch.Tensor,
                eps_final: float, head_g: torch.Tensor, head_b: torch.Tensor, eps_head: float, precision: int, out: torch.Tensor,
                with_cam: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """md_op_hook_cat_ln: x_local, x [T*S, D] -> (hook [T*S, 2D], camera feature [T, 2D] or None). `out` holds the rows the kernel
    must leave alone (t >= n_tokens); a copy of it is updated and returned."""
    x_local, x, out = _f32c(x_local), _f32c(x), _f32c(out).clone()
    rows, D = x.shape
    T = rows // S
    cam = torch.zeros((T, 2 * D), dtype=torch.float32, device=x.device) if with_cam else None
    _lib.check(_lib.load().md_op_hook_cat_ln(dev.handle, _p(x_local), _p(x), T, S, n_tokens, D, _p(_f32c(norm_g)), _p(_f32c(norm_b)),
                                             C.c_float(eps_final), _p(_f32c(head_g)), _p(_f32c(head_b)), C.c_float(eps_head), precision,
                                             _p(out), _p(cam), _stream_ptr(dev.ordinal)))
    return out, cam


def patchify(dev: Device, x: torch.Tensor, ps: int, Kp: int, precision: int, cls_x: Optional[torch.Tensor] = None, S: int = 0,
             cls: Optional[torch.Tensor] = None, pos0: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """md_op_patchify: x [B,3,H,W] -> (patch rows [B * ph * pw, Kp], the updated copy of cls_x [B*S, D] or None)."""
    x = _f32c(x)
    B, _, H, W = x.shape
    n_tokens = 1 + (H // ps) * (W // ps)
    out = torch.empty((B * (n_tokens - 1), Kp), dtype=torch.float32, device=x.device)
    D = 0
    if cls_x is not None:
        cls_x = _f32c(cls_x).clone()
        D = cls_x.shape[1]
        cls, pos0 = _f32c(cls), _f32c(pos0)
    _lib.check(_lib.load().md_op_patchify(dev.handle, _p(x), B, H, W, ps, Kp, precision, _p(out), _p(cls_x), S, n_tokens, D, _p(cls),
                                          _p(pos0), _stream_ptr(dev.ordinal)))
    return out, cls_x


def set_token0(dev: Device, x: torch.Tensor, S: int, src: torch.Tensor, src_stride: int) -> torch.Tensor:
    """md_op_set_token0 on a copy of x [nseq*S, D]: row 0 of every sequence <- src[b * src_stride, :D]."""
    x, src = _f32c(x).clone(), _f32c(src)
    rows, D = x.shape
    _lib.check(_lib.load().md_op_set_token0(dev.handle, _p(x), rows // S, S, D, _p(src), src_stride, _stream_ptr(dev.ordinal)))
    return x


def border_bias_fix(dev: Device, fmap: torch.Tensor, C_: int, bias9: torch.Tensor, precision: int) -> torch.Tensor:
    """md_op_border_bias_fix on a copy of the NHWC map [B,H,W,ld] (channels 0 .. C_-1 are corrected)."""
    fmap = _f32c(fmap).clone()
    B, H, W, ld = fmap.shape
    _lib.check(_lib.load().md_op_border_bias_fix(dev.handle, _p(fmap), B, H, W, C_, ld, _p(_f32c(bias9)), precision,
                                                 _stream_ptr(dev.ordinal)))
    return fmap


_COMPOSE_SHAPES = {  # kind -> (first weight, second weight, product) of (cin, cmid, cout)
    _lib.COMPOSE_DECONV_CONV: (lambda i, m, o: (i, m, 2, 2), lambda i, m, o: (o, m), lambda i, m, o: (i, o, 2, 2)),
    _lib.COMPOSE_DECONV_PAIR: (lambda i, m, o: (i, m, 2, 2), lambda i, m, o: (m, o, 2, 2), lambda i, m, o: (i, o, 4, 4)),
    _lib.COMPOSE_C1C3: (lambda i, m, o: (m, i), lambda i, m, o: (o, m, 3, 3), lambda i, m, o: (o, i, 3, 3)),
    _lib.COMPOSE_HEAD: (lambda i, m, o: (i, m, 2, 2), lambda i, m, o: (o, m, 3, 3), lambda i, m, o: (4 * o, i, 3, 3)),
}


def compose_weights(dev: Device, kind: int, cin: int, cmid: int, cout: int, w_first: torch.Tensor, w_second: torch.Tensor,
                    bias_first: Optional[torch.Tensor] = None, bias_second: Optional[torch.Tensor] = None, tail: int = 0, fill: float = 0.0):
    """md_op_compose_weights: the fp32 weight product of two layers as the commit composes it (kind = _lib.COMPOSE_*) -> (product, bias9
    [9, cout] or None). With biases (C1C3, HEAD) the nine position-class bias vectors come with it. `tail` extra elements behind both
    outputs hold `fill`, as does every element the launch does not write: the caller checks that they come back."""
    first, second, prod = (f(cin, cmid, cout) for f in _COMPOSE_SHAPES[kind])
    w_first, w_second = _f32c(w_first), _f32c(w_second)
    assert tuple(w_first.shape) == first and tuple(w_second.shape) == second, "weight shapes"
    n = cin * cout * {0: 4, 1: 16, 2: 9, 3: 36}[kind]
    out = torch.full((n + tail,), fill, dtype=torch.float32, device=w_first.device)
    with_bias = bias_first is not None or bias_second is not None
    if with_bias:
        bias_first, bias_second = _f32c(bias_first), _f32c(bias_second)
        assert bias_first.numel() == cmid and bias_second.numel() == cout, "bias shapes"
    b9 = torch.full((9 * cout + tail,), fill, dtype=torch.float32, device=w_first.device) if with_bias else None
    _lib.check(_lib.load().md_op_compose_weights(dev.handle, kind, cin, cmid, cout, _p(w_first), _p(w_second), _p(bias_first), _p(bias_second),
                                                 _p(out), _p(b9), _stream_ptr(dev.ordinal)))
    if tail:
        return out, b9
    return out.reshape(prod), (b9.reshape(9, cout) if b9 is not None else None)


# ---- the kernels that write MFMA operands, alone: outputs are the STORED bytes (bf16 / f16 / fp32 tensors, split-half rows as f16
# [.., 2 * width] = hi | lo, e4m3 as uint8) ----
_RAW_DTYPE = {0: torch.bfloat16, 1: torch.float32, 2: torch.uint8, 3: torch.float16, 4: torch.float16}


def _raw_empty(shape, width: int, precision: int, device) -> torch.Tensor:
    """Storage rows of logical shape [..., width]."""
    return torch.empty((*shape, width * (2 if precision == 4 else 1)), dtype=_RAW_DTYPE.get(precision, torch.uint8), device=device)


def layernorm_ex(dev: Device, x: torch.Tensor, S: int, groups, eps: float, precision: int, out_f32: bool = False,
                 fp8_inv_scale: float = 1.0, tok0: Optional[torch.Tensor] = None, tok0_stride: int = 0):
    """md_op_layernorm_ex: x [rows, D]; groups = [(seq0, nseq, gamma or None, beta or None), ...] -> (raw output rows, the rewritten
    copy of x when tok0 is given, else None)."""
    x = _f32c(x).clone()
    rows, D = x.shape
    n = len(groups)
    keep = [(None if g is None else _f32c(g), None if b is None else _f32c(b)) for _, _, g, b in groups]
    seq0, nseq = (C.c_int * n)(*[int(g[0]) for g in groups]), (C.c_int * n)(*[int(g[1]) for g in groups])
    ga = (C.c_void_p * n)(*[t[0].data_ptr() if t[0] is not None else None for t in keep])
    be = (C.c_void_p * n)(*[t[1].data_ptr() if t[1] is not None else None for t in keep])
    if tok0 is not None:
        tok0 = _f32c(tok0)
        assert tok0.numel() >= ((rows + S - 1) // S - 1) * tok0_stride + D, "tok0 is shorter than the sequences read from it"
    out = torch.empty((rows, D), dtype=torch.float32, device=x.device) if out_f32 else _raw_empty((rows,), D, precision, x.device)
    _lib.check(_lib.load().md_op_layernorm_ex(dev.handle, _p(x), rows, D, S, n, seq0, nseq, ga, be, C.c_float(eps), precision, int(out_f32),
                                              C.c_float(fp8_inv_scale), _p(tok0), tok0_stride, _p(out), _stream_ptr(dev.ordinal)))
    del keep
    return out, (x if tok0 is not None else None)


def store_rows(dev: Device, x: torch.Tensor, width: int, precision: int) -> torch.Tensor:
    """md_op_store_rows: fp32 [count] -> raw rows [count / width, width] of the storage type."""
    x = _f32c(x).reshape(-1)
    out = _raw_empty((x.numel() // max(width, 1),), width, precision, x.device) if width else _raw_empty((), x.numel(), precision, x.device)
    _lib.check(_lib.load().md_op_store_rows(dev.handle, _p(x), x.numel(), width, precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def load_rows(dev: Device, raw: torch.Tensor, count: int, width: int, precision: int) -> torch.Tensor:
    """md_op_load_rows: raw storage -> fp32 [count]."""
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == _RAW_DTYPE[precision] and raw.numel() == count * (2 if precision == 4 else 1)
    out = torch.empty(count, dtype=torch.float32, device=raw.device)
    _lib.check(_lib.load().md_op_load_rows(dev.handle, _p(raw), count, width, precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def f32_to_fp8(dev: Device, x: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """md_op_f32_to_fp8: e4m3 bytes (uint8) of clamp(x * inv_scale, +-448)."""
    x = _f32c(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().md_op_f32_to_fp8(dev.handle, _p(x), x.numel(), C.c_float(inv_scale), _p(out), _stream_ptr(dev.ordinal)))
    return out


def pack_fp8_rows(dev: Device, w: torch.Tensor, Kp: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """md_op_pack_fp8_rows: w [N, K] -> (e4m3 bytes [N, Kp] uint8, scale [N])."""
    w = _f32c(w)
    N, K = w.shape
    out = torch.full((N, max(Kp, 0)), 0x55, dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().md_op_pack_fp8_rows(dev.handle, _p(w), N, K, Kp, _p(out), _p(scale), _stream_ptr(dev.ordinal)))
    return out, scale


def nchw_to_nhwc(dev: Device, x: torch.Tensor, precision: int, relu: bool, ld: int, out: torch.Tensor) -> torch.Tensor:
    """md_op_nchw_to_nhwc into a copy of the pre-filled raw buffer `out` [B, H, W, ld (x 2 for split-half)]."""
    x, out = _f32c(x), out.contiguous().clone()
    B, Cn, H, W = x.shape
    assert out.is_cuda and out.dtype == _RAW_DTYPE[precision] and out.numel() == B * H * W * (ld or Cn) * (2 if precision == 4 else 1)
    _lib.check(_lib.load().md_op_nchw_to_nhwc(dev.handle, _p(x), B, Cn, H, W, precision, int(relu), ld, _p(out), _stream_ptr(dev.ordinal)))
    return out


def nhwc_to_nchw(dev: Device, raw: torch.Tensor, Cn: int, ld: int, coff: int, precision: int) -> torch.Tensor:
    """md_op_nhwc_to_nchw: raw [B, H, W, ld (x 2 for split-half)], channels coff .. coff + Cn -> fp32 [B, Cn, H, W]."""
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype == _RAW_DTYPE[precision] and raw.shape[3] == ld * (2 if precision == 4 else 1)
    B, H, W, _ = raw.shape
    out = torch.empty((B, Cn, H, W), dtype=torch.float32, device=raw.device)
    _lib.check(_lib.load().md_op_nhwc_to_nchw(dev.handle, _p(raw), B, Cn, H, W, ld, coff, precision, _p(out), _stream_ptr(dev.ordinal)))
    return out


def ln_fold_vectors(dev: Device, w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor],
                    precision: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """md_op_ln_fold_vectors: w [N, K] -> (c [N], d [N])."""
    w, gamma, beta = _f32c(w), _f32c(gamma), _f32c(beta)
    bias = _f32c(bias) if bias is not None else None
    N, K = w.shape
    c, d = torch.empty(N, dtype=torch.float32, device=w.device), torch.empty(N, dtype=torch.float32, device=w.device)
    _lib.check(_lib.load().md_op_ln_fold_vectors(dev.handle, _p(w), _p(gamma), _p(beta), _p(bias), N, K, precision, _p(c), _p(d),
                                                 _stream_ptr(dev.ordinal)))
    return c, d


def ln_finish(dev: Device, parts: torch.Tensor, inv_n: float, eps: float) -> torch.Tensor:
    """md_op_ln_finish: parts [rows, 4, 2] -> ab [rows, 2]."""
    parts = _f32c(parts)
    rows = parts.shape[0]
    assert parts.shape == (rows, 4, 2)
    ab = torch.empty((rows, 2), dtype=torch.float32, device=parts.device)
    _lib.check(_lib.load().md_op_ln_finish(dev.handle, _p(parts), rows, C.c_float(inv_n), C.c_float(eps), _p(ab), _stream_ptr(dev.ordinal)))
    return ab


def vit_gemm(dev: Device, kind: int, a: torch.Tensor, groups, precision: int, tile: int = _lib.TILE_AUTO, *, x: Optional[torch.Tensor] = None,
             x_out: Optional[torch.Tensor] = None, ln_out: Optional[torch.Tensor] = None, ln_stats_out: Optional[torch.Tensor] = None,
             ln_stats: Optional[torch.Tensor] = None, ln_raw: bool = False, ln_eps: float = 0.0, ln_inv_n: float = 0.0, S: int = 0, D: int = 0,
             P: int = 0, qk: Optional[torch.Tensor] = None, vT: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> None:
    """md_op_vit_gemm: one GEMM form of the ViT token stream (kind = _lib.VIT_GEMM_*) on the CALLER's buffers -- contiguous fp32 device
    tensors, updated in place; nothing is pre-filled. a [a_rows, K]; groups = dicts with row0, rows, arow0, w [N, K], bias [N] and, by
    kind, scale, gamma_next, c, pos."""
    tensors = [a, x, x_out, ln_out, ln_stats_out, ln_stats, qk, vT, out] + [g.get(k) for g in groups for k in ("w", "bias", "scale", "gamma_next", "c", "pos")]
    for t in tensors:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32), "vit_gemm takes contiguous fp32 device tensors"
    d = _lib.MdVitGemm()
    d.kind, d.precision, d.tile = kind, precision, tile
    d.N, d.K = groups[0]["w"].shape
    d.a_rows, d.a, d.ngroups = a.shape[0], a.data_ptr(), len(groups)
    assert a.shape[1] == d.K and 1 <= len(groups) <= 4
    for i, g in enumerate(groups):
        assert g["w"].shape == (d.N, d.K) and g["bias"].shape == (d.N,)
        d.g[i].row0, d.g[i].rows, d.g[i].arow0 = g["row0"], g["rows"], g.get("arow0", g["row0"])
        for k in ("w", "bias", "scale", "gamma_next", "c", "pos"):
            setattr(d.g[i], k, g[k].data_ptr() if g.get(k) is not None else None)
    first = next(t for t in (x, qk, out) if t is not None)
    d.out_rows = first.shape[0]
    for name, t, cols in (("x", x, d.N), ("x_out", x_out, d.N), ("ln_out", ln_out, d.N), ("out", out, d.N), ("qk", qk, 2 * D)):
        assert t is None or t.shape == (d.out_rows, cols), name
        setattr(d, name, t.data_ptr() if t is not None else None)
    assert ln_stats_out is None or ln_stats_out.shape == (d.out_rows, d.N // 256, 2)
    assert ln_stats is None or ln_stats.shape == ((d.out_rows, 4, 2) if ln_raw else (d.out_rows, 2))
    assert vT is None or vT.shape == (d.out_rows // S, D // 64, 64, (S + 63) // 64 * 64)
    d.ln_stats_out = ln_stats_out.data_ptr() if ln_stats_out is not None else None
    d.ln_stats = ln_stats.data_ptr() if ln_stats is not None else None
    d.vT = vT.data_ptr() if vT is not None else None
    d.ln_raw, d.ln_eps, d.ln_inv_n, d.S, d.D, d.P = int(ln_raw), ln_eps, ln_inv_n, S, D, P
    _lib.check(_lib.load().md_op_vit_gemm(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))


def gemm_last_form() -> dict:
    """md_debug_gemm_last_form + md_debug_gemm_last_launch: what this thread's last 256 x 256 GEMM launch ran (family -1: the operator
    entry took another tile), and the tile, the pixel-shuffle form and the contraction length (`tile`, `ps_fast`, `K`) launch_gemm resolved
    for the entry's launch."""
    v, n = (C.c_int * 8)(), (C.c_int * 4)()
    _lib.check(_lib.load().md_debug_gemm_last_form(C.byref(v)))
    _lib.check(_lib.load().md_debug_gemm_last_launch(C.byref(n)))
    return dict(zip(("family", "ek", "fold", "qkv", "conv", "diag", "blocks", "grid", "tile", "ps_fast", "K"), list(v) + list(n)[:3]))


def decoder_gemm(dev: Device, kind: int, x: torch.Tensor, w, bias, precision: int, tile: int = _lib.TILE_AUTO, *, B: int, H: int, W: int, Cin: int,
                 Cin_p: int, Cout: int, out: Optional[torch.Tensor] = None, ldo: int = 0, act: int = 0, res1: Optional[torch.Tensor] = None,
                 res2: Optional[torch.Tensor] = None, res_mod: int = 0, out2: Optional[torch.Tensor] = None, in_shared: bool = False,
                 res1_shared: bool = False, out_f32: bool = False, ps_f: int = 2, ps_coff: int = 0, head=None, head_w: Optional[torch.Tensor] = None,
                 head_b: float = 0.0, head_act: int = 0, Cmid: int = 0, w2: Optional[torch.Tensor] = None, bias2: Optional[torch.Tensor] = None) -> None:
    """md_op_decoder_gemm: one GEMM form of the convolutional decoders / heads (kind = _lib.DECODER_GEMM_*) on the CALLER's buffers,
    updated in place. x, res1, res2, out, out2: raw storage tensors (`store_rows` / `nchw_to_nhwc`), fp32 where the form stores fp32;
    w, bias: fp32 masters, lists of two for two weight groups; head: dicts with w [32], b, act, out (fp32), bstride."""
    ws = list(w) if isinstance(w, (list, tuple)) else [w]
    bs = list(bias) if isinstance(bias, (list, tuple)) else [bias] * len(ws)
    G, xm, raw = len(ws), (2 if precision == 4 else 1), _RAW_DTYPE.get(precision)
    conv, s2, ps, hd, up2 = (kind == k for k in range(5))
    assert 1 <= G <= 2 and len(bs) == G and (G == 1 or conv)
    OH, OW = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if s2 else ((ps_f * H, ps_f * W) if ps else (H, W))
    f32s = [t for t in ws + bs + [head_w, w2, bias2] if t is not None]
    for t in f32s:
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32, "weights and biases are contiguous fp32 device tensors"
    taps = ps_f * ps_f if ps else (4 if up2 else 9)
    for t in ws:
        assert t.numel() == Cin * (Cmid if up2 else Cout) * taps, "weight shape"
    for t in bs:
        assert t is None or t.numel() == (Cmid if up2 else Cout), "bias shape"

    def holds(t, elems, dtype, what):   # (an output may be longer: rows behind the launch's are the caller's)
        ok = t.numel() >= elems if what.startswith("out") else t.numel() == elems
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and ok, f"{what}: {tuple(t.shape)} {t.dtype}, expected {elems} of {dtype}"

    holds(x, (1 if in_shared else G) * B * H * W * Cin_p * xm, raw, "x")
    d = _lib.MdDecoderGemm()
    d.kind, d.precision, d.tile, d.B, d.H, d.W, d.Cin, d.Cin_p, d.Cout, d.ngroups = kind, precision, tile, B, H, W, Cin, Cin_p, Cout, G
    d.in_shared, d.res1_shared, d.act, d.res_mod, d.ldo, d.out_f32, d.ps_f, d.ps_coff = int(in_shared), int(res1_shared), act, res_mod, ldo, int(out_f32), ps_f, ps_coff
    for g in range(G):
        d.w[g], d.bias[g] = ws[g].data_ptr(), (bs[g].data_ptr() if bs[g] is not None else None)
    d.in_ = x.data_ptr()
    if conv or s2 or ps:
        if out_f32:
            holds(out, B * OH * OW * Cout, torch.float32, "out")
        else:
            assert ldo >= (ps_coff if ps else 0) + Cout
            holds(out, G * B * OH * OW * ldo * xm, raw, "out")
        if out2 is not None:
            holds(out2, G * B * OH * OW * ldo * xm, raw, "out2")
        if res1 is not None:
            holds(res1, (res_mod if res_mod else (1 if res1_shared else G) * B * OH * OW) * ldo * xm, raw, "res1")
        if res2 is not None:
            holds(res2, G * B * OH * OW * ldo * xm, raw, "res2")
        d.out, d.out2 = out.data_ptr(), (out2.data_ptr() if out2 is not None else None)
        d.res1, d.res2 = (res1.data_ptr() if res1 is not None else None), (res2.data_ptr() if res2 is not None else None)
    elif hd:
        chans = list(head or [])
        d.head_nch = len(chans)
        assert len(chans) <= 8
        for i, c in enumerate(chans):
            o, stride = c["out"], int(c["bstride"])
            assert o.is_cuda and o.dtype == torch.float32 and stride >= H * W and c["w"].numel() == 32 and c["w"].dtype == torch.float32 and c["w"].is_cuda
            assert o.numel() >= (B - 1) * stride + H * W, "head plane outside its tensor"   # (a view into a wider tensor: storage behind it is the caller's)
            d.ch[i].w, d.ch[i].b, d.ch[i].act, d.ch[i].out, d.ch[i].bstride = c["w"].data_ptr(), float(c["b"]), int(c["act"]), o.data_ptr(), stride
        if not chans:
            holds(out, B * H * W, torch.float32, "out")
            assert head_w is not None and head_w.numel() == 32
            d.head_w, d.head_b, d.head_act = head_w.data_ptr(), float(head_b), head_act
        d.out = out.data_ptr() if out is not None else chans[0]["out"].data_ptr()
    else:
        holds(out, B * 4 * H * W, torch.float32, "out")
        assert head_w.numel() == 32 and w2.numel() == 32 * Cmid * 9 and bias2.numel() == 32
        d.out, d.head_w, d.head_b, d.Cmid, d.w2, d.bias2 = out.data_ptr(), head_w.data_ptr(), float(head_b), Cmid, w2.data_ptr(), bias2.data_ptr()
    _lib.check(_lib.load().md_op_decoder_gemm(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))


def _index_table(entry, *args) -> torch.Tensor:
    """A host-only table entry: the count first (out = NULL), then the entries into an int32 host tensor."""
    n = entry(*args, None, 0)
    _lib.check(min(n, 0))
    out = torch.empty(n, dtype=torch.int32)
    assert entry(*args, C.c_void_p(out.data_ptr()), n) == n
    return out


def merge_index_table(B: int, g: int, steps: int, pad: int, SS: int, seq0: int = 0) -> torch.Tensor:
    """md_op_merge_index_table (no device): the gather table [B * E * E] of the merged map of g x g token tiles."""
    return _index_table(_lib.load().md_op_merge_index_table, B, g, steps, pad, SS, seq0)


def token_index_table(B: int, P: int, SS: int, seq0: int = 0) -> torch.Tensor:
    """md_op_token_index_table (no device): the patch rows (seq0 + b) SS + 1 + p of B sequences."""
    return _index_table(_lib.load().md_op_token_index_table, B, P, SS, seq0)


def indexed_gemm(dev: Device, kind: int, a: torch.Tensor, index: Optional[torch.Tensor], w: torch.Tensor, bias: Optional[torch.Tensor], precision: int,
                 tile: int = _lib.TILE_AUTO, *, out: torch.Tensor, ldo: int, M: Optional[int] = None, out_f32: bool = False,
                 res1: Optional[torch.Tensor] = None, res_mod: int = 0, B: int = 0, ph: int = 0, pw: int = 0, ps_f: int = 2, ps_coff: int = 0) -> None:
    """md_op_indexed_gemm: one gathered-row GEMM form (kind = _lib.INDEXED_GEMM_*) on the CALLER's contiguous fp32 device tensors; `out`
    [rows, ldo] is updated in place. a [rows_a, K]; index int32 [M] (None: the dense launch over a [M, K]); w [N, K], for the pixel
    shuffle [K, N, f, f]; res1 [res_mod, ldo]."""
    for t in (a, w, bias, res1, out):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32), "indexed_gemm takes contiguous fp32 device tensors"
    assert index is None or (index.is_cuda and index.is_contiguous() and index.dtype == torch.int32 and index.dim() == 1)
    ps = kind == _lib.INDEXED_GEMM_PIXSHUF
    d = _lib.MdIndexedGemm()
    d.kind, d.precision, d.tile = kind, precision, tile
    d.rows_a, d.K = a.shape
    d.M = index.numel() if index is not None else (a.shape[0] if M is None else M)
    d.N = w.shape[1] if ps else w.shape[0]
    assert a.dim() == 2 and (w.shape == (d.K, d.N, ps_f, ps_f) if ps else w.shape == (d.N, d.K)), "weight shape"
    assert bias is None or bias.shape == (d.N,)
    assert res1 is None or res1.shape == (res_mod, ldo)
    assert out.dim() == 2 and out.shape[1] == ldo
    d.a, d.index, d.w, d.bias, d.res1, d.out = a.data_ptr(), (index.data_ptr() if index is not None else None), w.data_ptr(), \
        (bias.data_ptr() if bias is not None else None), (res1.data_ptr() if res1 is not None else None), out.data_ptr()
    d.res_mod, d.out_rows, d.ldo, d.out_f32 = res_mod, out.shape[0], ldo, int(out_f32)
    d.B, d.ph, d.pw, d.ps_f, d.ps_coff = B, ph, pw, (ps_f if ps else 0), (ps_coff if ps else 0)
    _lib.check(_lib.load().md_op_indexed_gemm(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))


def _f32_dev(*tensors) -> None:
    for t in tensors:
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32), "the camera entries take contiguous fp32 device tensors"


def camera_encode(dev: Device, extr: torch.Tensor, intr: torch.Tensor, top, blocks, *, heads: int, H: int, W: int, eps_tok: float, eps_blk: float,
                  out: torch.Tensor, pose_out: Optional[torch.Tensor] = None, V: Optional[int] = None, depth: Optional[int] = None) -> None:
    """md_op_camera_encode: extr [B, V, 3, 4], intr [B, V, 3, 3] -> out [B, D] (+ pose_out [B, V, 9]), the CALLER's tensors, written in
    place. top: the 8 tensors of md_camera_encode.w in its order; blocks: per trunk block the 14 tensors of md_camera_encode.blk.
    V / depth: what the descriptor states when it is not what the tensors have (the refusal tests)."""
    _f32_dev(extr, intr, out, pose_out, *top, *(t for b in blocks for t in b))
    d = _lib.MdCameraEncode()
    d.B, d.V, d.D, d.heads, d.depth = out.shape[0], (extr.shape[1] if V is None else V), out.shape[1], heads, (len(blocks) if depth is None else depth)
    d.H, d.W, d.eps_tok, d.eps_blk = H, W, eps_tok, eps_blk
    assert len(top) == 8 and len(blocks) <= 8 and all(len(b) == 14 for b in blocks)
    for i, t in enumerate(top):
        d.w[i] = t.data_ptr()
    for i, b in enumerate(blocks):
        for j, t in enumerate(b):
            d.blk[i][j] = t.data_ptr()
    d.extr, d.intr, d.out, d.pose_out = extr.data_ptr(), intr.data_ptr(), out.data_ptr(), (pose_out.data_ptr() if pose_out is not None else None)
    _lib.check(_lib.load().md_op_camera_encode(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))


def camera_decode(dev: Device, cam: torch.Tensor, weights, H: int, W: int, pose: torch.Tensor, extr: Optional[torch.Tensor] = None,
                  intr: Optional[torch.Tensor] = None, *, B: Optional[int] = None) -> None:
    """md_op_camera_decode: cam [B, din] -> pose [B, 9] (+ extr [B, 12], intr [B, 9]), the CALLER's tensors, written in place. weights:
    the 10 tensors of md_camera_decode.w in its order. B: what the descriptor states when it is not cam's row count (the refusal tests)."""
    _f32_dev(cam, pose, extr, intr, *weights)
    assert len(weights) == 10
    d = _lib.MdCameraDecode()
    d.B, d.din, d.H, d.W = (cam.shape[0] if B is None else B), cam.shape[1], H, W
    for i, t in enumerate(weights):
        d.w[i] = t.data_ptr()
    d.cam, d.pose = cam.data_ptr(), pose.data_ptr()
    d.extr, d.intr = (extr.data_ptr() if extr is not None else None), (intr.data_ptr() if intr is not None else None)
    _lib.check(_lib.load().md_op_camera_decode(dev.handle, C.byref(d), _stream_ptr(dev.ordinal)))


def pose_to_camera(dev: Device, pose: torch.Tensor, H: int, W: int, extr: Optional[torch.Tensor] = None, intr: Optional[torch.Tensor] = None,
                   *, B: Optional[int] = None) -> None:
    """md_op_pose_to_camera: pose [B, 9] -> extr [B, 12] world-to-camera, intr [B, 9] (either may be None), written in place."""
    _f32_dev(pose, extr, intr)
    _lib.check(_lib.load().md_op_pose_to_camera(dev.handle, _p(pose), pose.shape[0] if B is None else B, H, W, _p(extr), _p(intr),
                                                _stream_ptr(dev.ordinal)))


def conv2d_direct_ex(dev: Device, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], add: Optional[torch.Tensor], stride: int,
                     pad: int, relu: bool, in_precision: int, out_ld: int, out: torch.Tensor) -> torch.Tensor:
    """md_op_conv2d_direct_ex: x [B, Cin, H, W], w [Cout, Cin, k, k], add fp32 NHWC or None -> a copy of the pre-filled fp32
    `out` [B, OH, OW, out_ld or Cout] with the first Cout columns of every pixel written."""
    x, w, out = _f32c(x), _f32c(w), _f32c(out).clone()
    B, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    assert out.shape == (B, OH, OW, out_ld or Cout) and (add is None or add.shape == (B, H, W, Cin))
    add = _f32c(add) if add is not None else None
    bias = _f32c(bias) if bias is not None else None
    _lib.check(_lib.load().md_op_conv2d_direct_ex(dev.handle, _p(x), _p(w), _p(bias), _p(add), B, Cin, H, W, Cout, k, stride, pad, int(relu),
                                                  in_precision, out_ld, _p(out), _stream_ptr(dev.ordinal)))
    return out


def unproject(dev: Device, depth: torch.Tensor, intrinsics=None, extrinsics=None, focal_px=None, conf: Optional[torch.Tensor] = None,
              rgb: Optional[torch.Tensor] = None, dense: bool = True, compact: bool = True, capacity: Optional[int] = None,
              out: Optional[PointCloud] = None, normals: bool = False, normal_min_cos: float = 0.0, mesh=None, **opts) -> PointCloud:
    """md_op_unproject_mesh: depth [B,H,W] (+ conf [B,H,W], + u8 rgb [B,H,W,3]) and pinhole cameras (intrinsics [B,3,3] or focal_px
    [B]; extrinsics [B,3,4] world-to-camera for world=True) -> `PointCloud`. opts: the fields of `md_points_opts`. normals /
    normal_min_cos (or an `out` that carries normal tensors): the surface normals beside the points and the grazing-angle test;
    without them the entry gets NULL normals, which is md_op_unproject. mesh: True, or a dict with any of max_rtol, face_capacity,
    pixel_index (or an `out` that carries mesh tensors): `faces`, `face_count` and `pixel_index` of the depth grid over the list's
    rows; without it the entry gets a NULL mesh, which is md_op_unproject_normals. Bit-identical to `pipeline.unproject_depth`,
    `pipeline.pixel_index` and `pipeline.mesh_grid`."""
    depth = _f32c(depth)
    B, H, W = (int(v) for v in depth.shape)
    conf = _f32c(conf) if conf is not None else None
    rgb = rgb.contiguous() if rgb is not None else None
    assert rgb is None or (rgb.is_cuda and rgb.dtype == torch.uint8)
    rq = _points_request(depth.device, B, H, W, want_rgb=rgb is not None, want_conf=conf is not None, want_depth=False, intrinsics=intrinsics,
                         extrinsics=extrinsics, focal_px=focal_px, dense=dense, compact=compact, capacity=capacity, out=out, normals=normals,
                         normal_min_cos=normal_min_cos, mesh=mesh, opts=opts)
    _lib.check(_lib.load().md_op_unproject_mesh(dev.handle, _p(depth), _p(conf), _p(rgb), B, H, W, C.byref(rq.cam), C.byref(rq.opts), C.byref(rq.outs),
                                                C.byref(rq.nrm) if rq.nrm is not None else None, C.byref(rq.msh) if rq.msh is not None else None,
                                                _stream_ptr(dev.ordinal)))
    return rq.cloud


def filter_views(dev: Device, depth: torch.Tensor, conf: Optional[torch.Tensor] = None, intrinsics=None, extrinsics=None, focal_px=None,
                 out: Optional[dict] = None, **opts):
    """md_op_filter_views: depth [B,H,W] (+ conf [B,H,W]) and the cameras of `unproject` -> (depth_out [B,H,W], support u8 [B,H,W],
    tau [1], kept int32 [B+1]). opts: the fields of `md_view_filter_opts`. `out`: a dict with any of the keys depth, support, tau,
    kept -> the tensors to write into (None = that output is skipped); default: four fresh tensors. Bit-identical to
    `pipeline.filter_views`."""
    depth = _f32c(depth)
    B, H, W = (int(v) for v in depth.shape)
    conf = _f32c(conf) if conf is not None else None
    if out is None:
        f = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=depth.device)  # noqa: E731
        out = dict(depth=f(B, H, W), support=f(B, H, W, dt=torch.uint8), tau=f(1), kept=f(B + 1, dt=torch.int32))
    o = _view_filter_opts(**opts)
    outs = _lib.MdViewFilterOutputs(*((out[k].data_ptr() if out.get(k) is not None else None) for k in ("depth", "support", "tau", "kept")))
    cam, keep = _points_cameras(depth.device, B, intrinsics, extrinsics, focal_px)
    _lib.check(_lib.load().md_op_filter_views(dev.handle, _p(depth), _p(conf), B, H, W, C.byref(cam), C.byref(o), C.byref(outs),
                                              _stream_ptr(dev.ordinal)))
    del keep
    return out.get("depth"), out.get("support"), out.get("tau"), out.get("kept")


def _list_inputs(xyz, faces=None, conf=None, rgb=None, normals=None, n_rows: Optional[int] = None, standin: bool = False):
    """What the list operators take, checked and staged -> (xyz, faces, conf, rgb, normals, N, F): xyz f32 [N,3], faces int32 [F,3],
    conf [N], u8 rgb [N,3], normals [N,3]. n_rows: `mesh_components` names its rows and has checked xyz, which may be None.
    standin: for N == 0 one row that is never read stands for the rgb input."""
    if n_rows is None:
        assert xyz.is_cuda and xyz.dim() == 2 and xyz.shape[1] == 3, "xyz is a device tensor [N,3]"
    if faces is not None:
        assert faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3, "faces is a device int32 tensor [F,3]"
        faces = faces.contiguous()
    xyz = _f32c(xyz) if xyz is not None else None
    N, F = int(xyz.shape[0]) if n_rows is None else int(n_rows), int(faces.shape[0]) if faces is not None else 0
    conf = _f32c(conf).reshape(N) if conf is not None else None
    normals = _f32c(normals).reshape(N, 3) if normals is not None else None
    rgb = rgb.contiguous() if rgb is not None else None
    assert rgb is None or (rgb.is_cuda and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (N, 3))
    if standin and rgb is not None and N == 0:  # an empty tensor has no address
        rgb = torch.zeros((1, 3), dtype=torch.uint8, device=xyz.device)
    return xyz, faces, conf, rgb, normals, N, F


def _list_outputs(out: Optional[PointCloud], dev, cap: int, conf, rgb, normals, carried=("index",), vertex: bool = True, **i32):
    """The outputs of a list operator -> (`out`, or a fresh PointCloud; its md_points_outputs). Fresh: every `i32` keyword is an
    int32 tensor of that shape and, with `vertex`, the list rows [cap, ..] of the inputs given come with count [2] and index [cap].
    The capacity is the fewest rows among the list rows and the `carried` tensors that the PointCloud has."""
    if out is None:
        out = PointCloud(**{k: _i32(dev, *shape) for k, shape in i32.items()})
        if vertex:
            out.xyz, out.count, out.index = _f32(dev, cap, 3), _i32(dev, 2), _i32(dev, cap)
            out.conf = _f32(dev, cap) if conf is not None else None
            out.rgb = _u8(dev, cap, 3) if rgb is not None else None
            out.normals = _f32(dev, cap, 3) if normals is not None else None
    rows = [int(t.shape[0]) for t in (out.xyz, out.conf, out.rgb, out.normals, *(getattr(out, k) for k in carried)) if t is not None]
    return out, _lib.MdPointsOutputs(None, None, _ptr(out.xyz), _ptr(out.rgb), _ptr(out.conf), _ptr(out.count), min(rows) if rows else 0, None)


def voxel_thin(dev: Device, xyz: torch.Tensor, voxel: float, conf: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None,
               normals: Optional[torch.Tensor] = None, capacity: Optional[int] = None, out: Optional[PointCloud] = None) -> PointCloud:
    """md_op_voxel_thin: a point list xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) -> `PointCloud` with one input row per
    occupied voxel of side `voxel`, in input order: xyz / conf / rgb / normals [capacity, ..], index and weight int32 [capacity],
    count int32 [2] (the survivors, twice: one view), dropped int32 [1]. capacity defaults to N. `out`: a PointCloud of an
    earlier call to write into again. Bit-identical to `pipeline.voxel_thin`."""
    xyz, _, conf, rgb, normals, N, _ = _list_inputs(xyz, None, conf, rgb, normals)
    cap = N if capacity is None else int(capacity)
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, ("index", "weight"), weight=(cap,), dropped=(1,))
    vox = _lib.MdPointsVoxel(float(voxel), _ptr(out.index), _ptr(out.weight), _ptr(out.dropped))
    _lib.check(_lib.load().md_op_voxel_thin(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, C.byref(vox), C.byref(outs),
                                            _p(out.normals), _stream_ptr(dev.ordinal)))
    return out


def radius_outliers(dev: Device, xyz: torch.Tensor, radius: float, min_neighbours: int, conf: Optional[torch.Tensor] = None,
                    rgb: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                    out: Optional[PointCloud] = None) -> PointCloud:
    """md_op_radius_outliers: a point list xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) -> `PointCloud` with the rows that have
    at least min_neighbours other rows within radius, in input order: xyz / conf / rgb / normals [capacity, ..], index int32
    [capacity], neighbours int32 [N] (min(neighbours, min_neighbours) of every input row, -1 outside the grid), count int32 [2] (the
    survivors, twice: one view), dropped int32 [1]. capacity defaults to N. `out`: a PointCloud of an earlier call to write into
    again. Bit-identical to `pipeline.radius_outliers`."""
    xyz, _, conf, rgb, normals, N, _ = _list_inputs(xyz, None, conf, rgb, normals)
    cap = N if capacity is None else int(capacity)
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, neighbours=(N,), dropped=(1,))
    assert out.neighbours is None or int(out.neighbours.shape[0]) >= N, "neighbours covers the input rows"
    outl = _lib.MdPointsOutlier(float(radius), int(min_neighbours), _ptr(out.neighbours), _ptr(out.index), _ptr(out.dropped))
    _lib.check(_lib.load().md_op_radius_outliers(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, C.byref(outl), C.byref(outs),
                                                 _p(out.normals), _stream_ptr(dev.ordinal)))
    return out


def fit_planes(dev: Device, xyz: torch.Tensor, planes: int = 1, hypotheses: int = 256, tol: float = 0.0, min_inliers: int = 3, seed: int = 0,
               normals: Optional[torch.Tensor] = None, normal_min_cos: float = 0.0, axis=(0.0, 0.0, 0.0), axis_min_cos: float = 0.0,
               mode=0, conf: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None, out: Optional[PointCloud] = None,
               capacity: Optional[int] = None) -> PointCloud:
    """md_op_fit_planes: a point list xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) -> `PointCloud` whose `planes`
    (`FittedPlanes`) holds up to `planes` RANSAC planes of `hypotheses` triples each (plane f32 [P,4], plane_count int32 [P+1],
    hypothesis int32 [P]), label int32 [N] (the plane of every input row, -1 none, -2 not finite) and dropped int32 [1]. mode
    "label" / 0: nothing else. "drop" / 1, "keep" / 2: also the rows without / of a plane in input order, xyz / conf / rgb /
    normals [capacity, ..], index int32 [capacity] and count int32 [2]; capacity defaults to N. `out`: a PointCloud of an earlier
    call to write into again. Bit-identical to `pipeline.fit_planes`."""
    xyz, _, conf, rgb, normals, N, _ = _list_inputs(xyz, None, conf, rgb, normals)
    opts = dict(planes=planes, hypotheses=hypotheses, tol=tol, min_inliers=min_inliers, seed=seed, normal_min_cos=normal_min_cos, axis=axis,
                axis_min_cos=axis_min_cos, mode=mode)
    cut = _plane_mode(opts) != 0
    cap = N if capacity is None else int(capacity)
    fresh = out is None
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, vertex=cut)
    if fresh:
        P = max(int(planes), 0)
        out.planes = FittedPlanes(plane=_f32(xyz.device, P, 4), plane_count=_i32(xyz.device, P + 1), hypothesis=_i32(xyz.device, P),
                                  label=_i32(xyz.device, N), dropped=_i32(xyz.device, 1))
    assert out.planes is not None and (out.planes.label is None or int(out.planes.label.shape[0]) >= N), "label covers the input rows"
    pln = _planes_struct(opts, out.planes, out.index)
    _lib.check(_lib.load().md_op_fit_planes(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, C.byref(pln), C.byref(outs),
                                            _p(out.normals) if cut else None, _stream_ptr(dev.ordinal)))
    return out


def cluster_points(dev: Device, xyz: torch.Tensor, radius: float, min_neighbours: int = 0, min_points: int = 1, max_points: int = 0, mode=0,
                   table: Optional[int] = None, conf: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None,
                   normals: Optional[torch.Tensor] = None, out: Optional[PointCloud] = None, capacity: Optional[int] = None) -> PointCloud:
    """md_op_cluster_points: a point list xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) -> `PointCloud` whose `clusters`
    (`PointClusters`) holds the DBSCAN clusters of the rows (min_neighbours 0: Euclidean cluster extraction): label, cluster_size
    and cluster int32 [N], the table of kept clusters (table rows, default N; the first min(stats[1], table) are written), stats
    int32 [4] and dropped int32 [1]. mode "label" / 0: nothing else. "keep" / 1: also the rows of kept clusters in input order,
    xyz / conf / rgb / normals [capacity, ..], index int32 [capacity] and count int32 [2]; capacity defaults to N. `out`: a
    PointCloud of an earlier call to write into again. Bit-identical to `pipeline.cluster_points`."""
    xyz, _, conf, rgb, normals, N, _ = _list_inputs(xyz, None, conf, rgb, normals)
    opts = dict(radius=radius, min_neighbours=min_neighbours, min_points=min_points, max_points=max_points, mode=mode)
    if table is not None:
        opts["table"] = table
    cut = _cluster_mode_of(mode) != 0
    cap = N if capacity is None else int(capacity)
    fresh = out is None
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, vertex=cut)
    if fresh:
        out.clusters = _new_clusters(xyz.device, N, N if table is None else table)
    assert out.clusters is not None and (out.clusters.label is None or int(out.clusters.label.shape[0]) >= N), "label covers the input rows"
    clu = _clusters_struct(opts, out.clusters, out.index)
    _lib.check(_lib.load().md_op_cluster_points(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, C.byref(clu), C.byref(outs),
                                                _p(out.normals) if cut else None, _stream_ptr(dev.ordinal)))
    return out


def match_points(dev: Device, xyz: torch.Tensor, target: torch.Tensor, radius: float, tol=(), mode=0, conf: Optional[torch.Tensor] = None,
                 rgb: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, out: Optional[PointCloud] = None,
                 capacity: Optional[int] = None) -> PointCloud:
    """md_op_match_points: a point list xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) and a reference cloud target [T,3], both
    on the device -> `PointCloud` whose `match` (`PointMatch`) holds, for every row, the nearest target row within `radius`
    (nearest int32 [N]: -1 none, -2 dropped; dist2 f32 [N]), stats int32 [8] (in-range rows, matched rows, target rows in the
    grid, 0, rows within each of up to four tolerances `tol`) and dropped int32 [1]. mode "label" / 0: nothing else. "matched" /
    1, "unmatched" / 2: also the rows with / without a counterpart in input order, xyz / conf / rgb / normals [capacity, ..],
    index int32 [capacity] and count int32 [2]; capacity defaults to N. `out`: a PointCloud of an earlier call to write into
    again. Bit-identical to `pipeline.match_points`."""
    xyz, _, conf, rgb, normals, N, _ = _list_inputs(xyz, None, conf, rgb, normals)
    target = target.to(device=xyz.device, dtype=torch.float32).contiguous().reshape(-1, 3)
    cut = _match_mode_of(mode) != 0
    cap = N if capacity is None else int(capacity)
    fresh = out is None
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, vertex=cut)
    if fresh:
        out.match = _new_match(xyz.device, N)
    assert out.match is not None and (out.match.nearest is None or int(out.match.nearest.shape[0]) >= N), "nearest covers the input rows"
    out.match.index = out.index if cut else None
    mat = _match_struct(dict(radius=radius, tol=tol, mode=mode), _p(target), int(target.shape[0]), _lib.MD_MEM_DEVICE, out.match, out.index)
    _lib.check(_lib.load().md_op_match_points(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, C.byref(mat), C.byref(outs),
                                              _p(out.normals) if cut else None, _stream_ptr(dev.ordinal)))
    return out


def register_points(dev: Device, xyz: torch.Tensor, target: torch.Tensor, radius: float, iterations: int = 10, init=None,
                    min_pairs: Optional[int] = None, rot_eps: float = 0.0, trans_eps: float = 0.0, normals: Optional[torch.Tensor] = None, apply: bool = False,
                    xyz_out: Optional[torch.Tensor] = None, target_normals: Optional[torch.Tensor] = None) -> PointRegistration:
    """md_op_register_points: rigid point-to-point ICP of the list xyz [N,3] onto the reference cloud target [T,3], both on the
    device, pairing within `radius` for `iterations` rounds from the transform `init` (twelve f64, R row-major then t, or a 3x4 /
    4x4 matrix; None: the identity) -> `PointRegistration`: transform f64 [12], the per-pass pairs / sum_d2 histories, stats,
    dropped, nearest / dist2 under the final transform. rot_eps / trans_eps > 0 stop the rounds once a solve changes R and t by no
    more than that. apply: also xyz, the moved rows, and (with normals=) the rotated normals; xyz_out: the tensor the moved rows
    go to, which may be `xyz` itself. target_normals [T,3] on the device: the point-to-plane form (`md_op_register_points_plane`):
    the residual of a pair is measured along its target normal, pairs with a normal that is not finite or all zero are left out,
    min_pairs is at least 6 (the default then), status 3 is a degenerate system and `sum_r2` holds the squared residuals of every pass.
    Bit-identical to `pipeline.register_points`."""
    xyz, _, _, _, normals, N, _ = _list_inputs(xyz, None, None, None, normals)
    target = target.to(device=xyz.device, dtype=torch.float32).contiguous().reshape(-1, 3)
    K = int(iterations)
    d = xyz.device
    res = _new_registration(d, N, K)
    if xyz_out is not None:
        assert xyz_out.is_cuda and xyz_out.dtype == torch.float32 and xyz_out.is_contiguous() and xyz_out.numel() == 3 * N, "xyz_out is f32 [N,3]"
        res.xyz = xyz_out
    elif apply:
        res.xyz = _f32(d, N, 3)
    if (apply or xyz_out is not None) and normals is not None:
        res.normals = _f32(d, N, 3)
    keep: list = []
    reg = _register_struct(dict(radius=radius, iterations=K, init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps,
                                target_normals=target_normals), _p(target),
                           int(target.shape[0]), _lib.MD_MEM_DEVICE, res, keep)
    if target_normals is None:
        _lib.check(_lib.load().md_op_register_points(dev.handle, _p(xyz), _p(normals), N, C.byref(reg), _p(res.xyz), _p(res.normals),
                                                     _stream_ptr(dev.ordinal)))
        return res
    target_normals = target_normals.to(device=xyz.device, dtype=torch.float32).contiguous().reshape(-1, 3)
    plane = _register_plane_struct(d, target_normals, int(target.shape[0]), _lib.MD_MEM_DEVICE, res, keep)
    _lib.check(_lib.load().md_op_register_points_plane(dev.handle, _p(xyz), _p(normals), N, C.byref(reg), C.byref(plane), _p(res.xyz),
                                                       _p(res.normals), _stream_ptr(dev.ordinal)))
    return res


def cloud_distance(dev: Device, a: torch.Tensor, b: torch.Tensor, radius: float, tol=()) -> dict:
    """Precision, recall, F-score and Chamfer distance of cloud a [N,3] against the reference b [T,3] within `radius`: two
    `match_points` calls, a against b and b against a. -> dict(stats_ab, stats_ba: the two int32 [8] count sets as lists;
    precision, recall, fscore: one float per tolerance, precision = rows of a within tol of b / N, recall = rows of b within tol
    of a / T; chamfer: the mean distance of the matched rows of a plus that of b (nan for a direction without a match)). The
    counts are the operator's and bit-identical to the host reference; the Chamfer mean is a torch float reduction over sqrt(dist2)
    and lies outside the bit contract."""
    ab = match_points(dev, a, b, radius, tol=tol).match
    ba = match_points(dev, b, a, radius, tol=tol).match
    sa, sb = ab.stats.cpu().tolist(), ba.stats.cpu().tolist()
    N, T = int(ab.nearest.shape[0]), int(ba.nearest.shape[0])
    precision = [sa[4 + t] / N if N else 0.0 for t in range(len(tol))]
    recall = [sb[4 + t] / T if T else 0.0 for t in range(len(tol))]
    fscore = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)]
    mean = lambda m: float(m.dist2[m.nearest >= 0].double().sqrt().mean()) if bool((m.nearest >= 0).any()) else float("nan")  # noqa: E731
    return dict(stats_ab=sa, stats_ba=sb, precision=precision, recall=recall, fscore=fscore, chamfer=mean(ab) + mean(ba))


def decimate_mesh(dev: Device, xyz: torch.Tensor, faces: torch.Tensor, voxel: float, conf: Optional[torch.Tensor] = None,
                  rgb: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                  face_capacity: Optional[int] = None, out: Optional[PointCloud] = None) -> PointCloud:
    """md_op_decimate_mesh: vertices xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) and faces int32 [F,3] over them -> `PointCloud`
    with one vertex per occupied voxel of side `voxel` (every vertex output is `voxel_thin`'s), remap int32 [N], the kept faces
    int32 [face_capacity,3] over the output rows with face_index int32 [face_capacity], face_count int32 [2] and faces_dropped
    int32 [3] (invalid, degenerate, duplicate). capacity defaults to N, face_capacity to F. `out`: a PointCloud of an earlier call
    to write into again. Bit-identical to `pipeline.decimate_mesh`."""
    xyz, faces, conf, rgb, normals, N, F = _list_inputs(xyz, faces, conf, rgb, normals)
    cap, fcap = N if capacity is None else int(capacity), F if face_capacity is None else int(face_capacity)
    out, outs = _list_outputs(out, xyz.device, cap, conf, rgb, normals, ("index", "weight"), weight=(cap,), dropped=(1,), remap=(N,),
                              faces=(fcap, 3), face_index=(fcap,), face_count=(2,), faces_dropped=(3,))
    assert out.remap is None or int(out.remap.shape[0]) >= N, "remap covers the input rows"
    frows = [int(t.shape[0]) for t in (out.faces, out.face_index) if t is not None]
    dec = _lib.MdPointsDecimate(float(voxel), _ptr(out.index), _ptr(out.weight), _ptr(out.dropped), _ptr(out.remap), _ptr(out.faces),
                                _ptr(out.face_index), _ptr(out.face_count), min(frows) if frows else 0, _ptr(out.faces_dropped))
    _lib.check(_lib.load().md_op_decimate_mesh(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, _p(faces), F, C.byref(dec),
                                               C.byref(outs), _p(out.normals), _stream_ptr(dev.ordinal)))
    return out


def mesh_components(dev: Device, faces: torch.Tensor, n_rows: int, min_faces: int, xyz: Optional[torch.Tensor] = None,
                    conf: Optional[torch.Tensor] = None, rgb: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                    compact: bool = False, capacity: Optional[int] = None, face_capacity: Optional[int] = None,
                    out: Optional[PointCloud] = None) -> PointCloud:
    """md_op_mesh_components: faces int32 [F,3] over n_rows vertex rows -> `PointCloud` with label int32 [N] (the smallest row of
    every row's component), component_faces int32 [N], the faces of the components with at least min_faces faces, int32
    [face_capacity,3], with face_index int32 [face_capacity], face_count int32 [2] and component_stats int32 [5] (invalid, dropped,
    clipped faces, components with a face, components kept). compact: the rows those faces name are compacted too, in ascending
    order: xyz [N,3] (+ conf [N], u8 rgb [N,3], normals [N,3]) -> the rows of the survivors, index int32 [capacity], count int32 [2],
    remap int32 [N], and the faces are written through remap. capacity defaults to N, face_capacity to F. `out`: a PointCloud of an
    earlier call to write into again. Bit-identical to `pipeline.mesh_components`."""
    assert faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3, "faces is a device int32 tensor [F,3]"
    N = int(n_rows)
    if not compact:
        assert xyz is None and conf is None and rgb is None and normals is None and capacity is None, "vertex rows are carried only with compact"
    else:
        assert xyz is not None and xyz.is_cuda and tuple(xyz.shape) == (N, 3), "compact needs xyz, a device tensor [n_rows,3]"
    xyz, faces, conf, rgb, normals, _, F = _list_inputs(xyz, faces, conf, rgb, normals, n_rows=N)  # xyz, when there is one, is checked above
    cap, fcap = N if capacity is None else int(capacity), F if face_capacity is None else int(face_capacity)
    out, outs = _list_outputs(out, faces.device, cap, conf, rgb, normals, vertex=compact, label=(N,), component_faces=(N,), faces=(fcap, 3),
                              face_index=(fcap,), face_count=(2,), component_stats=(5,), **(dict(remap=(N,)) if compact else {}))
    for t in (out.label, out.component_faces, out.remap):
        assert t is None or int(t.shape[0]) >= N, "label / component_faces / remap cover the input rows"
    frows = [int(t.shape[0]) for t in (out.faces, out.face_index) if t is not None]
    comp = _lib.MdPointsComponents(int(min_faces), 1 if compact else 0, _ptr(out.label), _ptr(out.component_faces), _ptr(out.index), _ptr(out.remap),
                                   _ptr(out.faces), _ptr(out.face_index), _ptr(out.face_count), min(frows) if frows else 0,
                                   _ptr(out.component_stats))
    _lib.check(_lib.load().md_op_mesh_components(dev.handle, _p(xyz), _p(conf), _p(rgb), _p(normals), N, _p(faces), F, C.byref(comp),
                                                 C.byref(outs), _p(out.normals), _stream_ptr(dev.ordinal)))
    return out


def smooth_mesh(dev: Device, xyz: torch.Tensor, faces: torch.Tensor, step: float, iterations: int, lam: float, mu: float = 0.0,
                pin_boundary: bool = True, normals: bool = False, capacity: Optional[int] = None,
                out: Optional[SmoothedMesh] = None) -> SmoothedMesh:
    """md_op_smooth_mesh: xyz f32 [N,3] and faces int32 [F,3] over its rows -> `SmoothedMesh`: Taubin (lam | mu) or, with mu == 0,
    Laplacian smoothing on the integer lattice of side `step`, 2 * iterations (iterations) Jacobi steps, rows with an open fan
    pinned with pin_boundary; xyz f32 [capacity,3], with normals=True the area-weighted vertex normals f32 [capacity,3] of the
    smoothed faces, stats int32 [5] (invalid and degenerate faces, rows not in range, open rows, moved rows). capacity defaults to
    N: rows behind it are not written. `out`: a SmoothedMesh of an earlier call to write into again. Bit-identical to
    `pipeline.smooth_mesh`."""
    xyz, faces, _, _, _, N, F = _list_inputs(xyz, faces)
    if out is None:
        cap = N if capacity is None else int(capacity)
        out = SmoothedMesh(xyz=torch.empty((max(cap, 0), 3), dtype=torch.float32, device=xyz.device),
                           normals=torch.empty((max(cap, 0), 3), dtype=torch.float32, device=xyz.device) if normals else None,
                           stats=torch.empty(5, dtype=torch.int32, device=xyz.device))
    else:
        cap = min(int(t.shape[0]) for t in (out.xyz, out.normals) if t is not None) if capacity is None else int(capacity)
    smooth = _lib.MdPointsSmooth(float(step), float(lam), float(mu), int(iterations), 1 if pin_boundary else 0, _p(out.xyz), _p(out.normals),
                                 _p(out.stats))
    _lib.check(_lib.load().md_op_smooth_mesh(dev.handle, _p(xyz), N, _p(faces), F, C.byref(smooth), cap, _stream_ptr(dev.ordinal)))
    return out


def render_points(dev: Device, xyz: torch.Tensor, H: int, W: int, intrinsics=None, extrinsics=None, focal_px=None,
                  rgb: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, *, pixel_offset: float = 0.0, z_near: float = 0.0,
                  z_far: float = 0.0, radius: int = 0, out: Optional[RenderedPoints] = None) -> RenderedPoints:
    """md_op_render_points: a point list xyz [N,3] (+ u8 rgb [N,3]) z-buffered into T target cameras (intrinsics [T,3,3] or focal_px
    [T]; extrinsics [T,3,4] world-to-camera, None = the points are in the camera's frame) -> `RenderedPoints` of H x W images.
    count: a device int32 tensor whose first word is the number of rows to render (what `unproject` / `voxel_thin` left in
    `count[-1:]`), read on the device. `out`: a RenderedPoints to write into again; a None field skips that output. Bit-identical
    to `pipeline.render_points`."""
    xyz, _, _, rgb, _, N, _ = _list_inputs(xyz, rgb=rgb, standin=True)
    assert count is None or (count.is_cuda and count.dtype == torch.int32 and count.is_contiguous() and count.numel() >= 1)
    T, cam, o, out, outs, keep = _render_request(xyz.device, int(H), int(W), intrinsics, extrinsics, focal_px, pixel_offset=pixel_offset,
                                                 z_near=z_near, z_far=z_far, radius=radius, want_rgb=rgb is not None, out=out)
    _lib.check(_lib.load().md_op_render_points(dev.handle, _p(xyz), _p(rgb), N, _p(count), T, int(H), int(W), C.byref(cam), C.byref(o),
                                               C.byref(outs), _stream_ptr(dev.ordinal)))
    del keep
    return out


def mesh_grid(dev: Device, depth: torch.Tensor, pixel_index: torch.Tensor, stride: int = 1, max_rtol: float = 0.0, vertex_limit: int = 0,
              face_capacity: Optional[int] = None, faces: Optional[torch.Tensor] = None, face_count: Optional[torch.Tensor] = None):
    """md_op_mesh_grid: depth f32 [B,H,W] and a map pixel_index int32 [B,H,W] (the list row of a pixel, -1 = none) -> (faces int32
    [face_capacity,3], face_count int32 [B+1]): the triangles of the strided lattice whose corners have an index in
    [0, vertex_limit) (0 = no limit) and whose edges pass the max_rtol test, in (view, row, column, triangle) order.
    face_capacity defaults to two faces per quad; `faces` / `face_count`: tensors to write into again. Bit-identical to
    `pipeline.mesh_grid`."""
    assert depth.is_cuda and depth.dim() == 3 and pixel_index.is_cuda and pixel_index.dtype == torch.int32
    depth, pixel_index = _f32c(depth), pixel_index.contiguous()
    B, H, W = (int(v) for v in depth.shape)
    assert tuple(pixel_index.shape) == (B, H, W)
    if faces is None:
        cap = _lattice(B, H, W, stride)[2] if face_capacity is None else int(face_capacity)
        faces = torch.empty((max(cap, 0), 3), dtype=torch.int32, device=depth.device)
    else:
        cap = int(faces.shape[0]) if face_capacity is None else int(face_capacity)
    if face_count is None:
        face_count = torch.empty(B + 1, dtype=torch.int32, device=depth.device)
    msh = _lib.MdPointsMesh(float(max_rtol), _p(faces) if faces.numel() else None, _p(face_count), cap, None)
    _lib.check(_lib.load().md_op_mesh_grid(dev.handle, _p(depth), _p(pixel_index), B, H, W, int(stride), int(vertex_limit), C.byref(msh),
                                           _stream_ptr(dev.ordinal)))
    return faces, face_count


def render_mesh(dev: Device, xyz: torch.Tensor, faces: torch.Tensor, H: int, W: int, intrinsics=None, extrinsics=None, focal_px=None,
                rgb: Optional[torch.Tensor] = None, face_count: Optional[torch.Tensor] = None, *, pixel_offset: float = 0.0,
                z_near: float = 0.0, z_far: float = 0.0, cull: int = 0, max_extent: int = 0,
                out: Optional[RasterisedMesh] = None) -> RasterisedMesh:
    """md_op_render_mesh: the faces int32 [F,3] over the rows of xyz [N,3] (+ u8 rgb [N,3]) rasterised into T target cameras
    (intrinsics [T,3,3] or focal_px [T]; extrinsics [T,3,4] world-to-camera, None = the points are in the camera's frame) ->
    `RasterisedMesh` of H x W images. face_count: a device int32 tensor whose first word is the number of faces to draw (what
    `mesh_grid` / `unproject(mesh=)` left in `face_count[-1:]`), read on the device. `out`: a RasterisedMesh to write into again; a
    None field skips that output. Bit-identical to `pipeline.render_mesh`."""
    xyz, faces, _, rgb, _, N, F = _list_inputs(xyz, faces, rgb=rgb, standin=True)
    assert face_count is None or (face_count.is_cuda and face_count.dtype == torch.int32 and face_count.is_contiguous() and face_count.numel() >= 1)
    T, cam, o, out, outs, keep = _raster_request(xyz.device, int(H), int(W), intrinsics, extrinsics, focal_px, pixel_offset=pixel_offset,
                                                 z_near=z_near, z_far=z_far, cull=cull, max_extent=max_extent, want_rgb=rgb is not None, out=out)
    _lib.check(_lib.load().md_op_render_mesh(dev.handle, _p(xyz) if N else None, _p(rgb), N, _p(faces) if F else None, F, _p(face_count), T,
                                             int(H), int(W), C.byref(cam), C.byref(o), C.byref(outs), _stream_ptr(dev.ordinal)))
    del keep
    return out


def raster_inline_pixels() -> int:
    """md_raster_inline_pixels: the largest box, in pixels, that the setup kernel of `render_mesh` draws in the face's own thread."""
    return int(_lib.load().md_raster_inline_pixels())


def fov_to_focal(fovx_deg: float, H: int, W: int) -> Tuple[float, float]:
    f, y = C.c_float(), C.c_float()
    _lib.check(_lib.load().md_op_fov_to_focal(C.c_float(fovx_deg), H, W, C.byref(f), C.byref(y)))
    return f.value, y.value
