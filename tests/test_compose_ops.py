"""Operator tests of the layer compositions `model_commit` runs (burn_depth_amd/csrc/md_engine.hip), through `ops.compose_weights`
(md_op_compose_weights: the commit's own host functions compose_deconv_conv / compose_deconv_pair / compose_c1c3 / compose_head /
compose_head_bias on the caller's fp32 tensors), at two levels:

(A) the composed fp32 tensor against fp64 (test_composed_tensors_*). The reference applies the two LAYERS, uncomposed, in fp64 to unit impulses:
    DECONV_CONV conv2d_1x1(conv_transpose2d(delta)), DECONV_PAIR conv_transpose2d(conv_transpose2d(delta)), C1C3 the flipped impulse response
    of conv2d_3x3(conv2d_1x1(delta)); HEAD and the nine bias classes are `compose_head` / `bias_classes` of tests/test_compose_algebra.py (that
    file checks them against the layers). Bound, per element, derived: the kernels form a left-to-right fp32 sum of n products,
    |got - ref| <= n 2^-24 sum_m |a_m| |b_m| (sum of magnitudes in fp64: the same reference on |weights|), n = cmid (DECONV_CONV, DECONV_PAIR,
    C1C3), 4 cmid (a HEAD tap folds at most four taps of the 3x3), 9 cmid + 1 (a bias class: the second bias and at most nine taps). A
    contracted fma removes roundings. No max|ref| term: an element whose products are all absent (five of the nine HEAD taps per parity) must
    be exactly 0. Shapes: three pairwise different channel counts that are no multiple of 4, cmid = 1, and per kernel one case of more than
    4096 x 256 elements with cmid <= 8 -- the kernels launch min(total / 256, 4096) blocks and stride over the rest, which no model size but
    the full one reaches; its last elements are asserted on their own. Elements behind the tensors come back as the caller's fill.

(B) each composition as the engine launches it (test_launched_*): the composed weight of (A) into `ops.decoder_gemm` -- DECONV_CONV as
    MD_DECODER_GEMM_PIXSHUF f = 2, DECONV_PAIR f = 4, C1C3 as MD_DECODER_GEMM_CONV3 with bias9[4] followed by `ops.border_bias_fix(bias9)`
    (run_decoder of md_engine.hip) -- against the two layers in fp64 torch on the activations as the storage type holds them. HEAD is covered
    by test_decoder_gemm_ops.py (EPI_HEAD_UP2). How the 1x1's bias rides through DECONV_CONV (include/mi_depth.h, md_op_compose_weights): the
    deconvolution has no bias, so out_conv's bias is not composed; the engine passes it unchanged as the pixel-shuffle launch's bias.
    Bound per element = close_check's 0.5 ulp_T(ref) (+ tie slack) + A_MFMA max|acc + bias|, plus the derived terms
      conv(|x|, 0.5 ulp_T |Wc|)   the fp32 product rounded to the operand type (22 bits for the three-term split-half form, absent for f32),
      conv(|x|, E)                the fp32 composition, E = the element bound of (A) (+ E of the bias class for C1C3),
      ulp_T(ref) on C1C3's border pixels: border_bias_fix reads the stored value, adds bias9[class] - bias9[4] and rounds AGAIN. The stored
                                  value's half ulp is an ulp of the interior-class value v = ref - (bias9[class] - bias9[4]), so this term is a
                                  bound only while ulp_T(v) <= 2 ulp_T(ref); the C1C3 cases carry a 3x3 bias of about 4.5 that keeps every
                                  value of the map inside two binades, and the CPU test asserts that premise on every border element.
    `conv` is the launch's own operation (conv_transpose2d with stride f, conv2d pad 1) in fp64. The derived terms are as large as the
    half-ulp on every bf16 element, so the tie slack's users are counted beyond them (close_check `slack_beyond_extra`) and stay under 1 %.
    F16X2 must take the three-term form (a product is never f16-exact): asserted from the launch record's K = terms x padded channels.
    Maps, B = 2: 2 x 2 (all border, four corners), 3 x 5 (one interior row), 17 x 19 (646 rows: tile boundaries at 256 and 512, the image
    boundary at 323). Cin = 64 in pixels of Cin_p = 128 channels.

No bound is taken from a GPU result: the CPU tests evaluate every formula in fp32 with torch and must pass the same bounds; they reject the
mutants below, and `MUTANT_ACTIVE` says where a mutant is the identity (asserted in both directions):
  wo_cmid_cout    DECONV_CONV: Wo read as [cmid, cout]                       identity when cmid == 1 or cout == 1
  cico_strides    ci / co strides exchanged in the output (all four kinds)  identity when cin == 1 or cout == 1 (none here)
  q_transposed    DECONV_CONV: q taken as 2 dx + dy                          never
  qa_qb           DECONV_PAIR: qa and qb exchanged                           never
  wb_cout_cmid    DECONV_PAIR: Wb read as [cout, cmid]                       identity when cmid == 1 or cout == 1
  dydx            HEAD: dy / dx exchanged                                    never
  parity          HEAD: parity group q = 2 px + py                           never
  a_trunc         HEAD: a by truncating instead of floor division            never (py = 0, u = 0 moves from a = -1 to a = 0)
  tap_transposed  C1C3: tap (u, v) transposed                                never
  ryrx, valid_inverted, b_out_left_out, all_interior   bias classes: ry / rx exchanged; `ry == 0` drops u == 2; the second layer's bias (the
                  kernel's `b1`) left out; the first layer's bias counted through outside taps as well (all classes = interior)   never
                  (b_out_left_out would be the identity for a zero bias)
  level (B): border_all_interior (no border fix), fix_absolute (the fix adds bias9[class], not the difference to class 4), bias1_dropped (the
                  1x1's bias dropped: DECONV_CONV's launch bias, C1C3's first bias)   never; the first two are C1C3's alone."""
import ctypes as C
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import close_check
from close_check import A_MFMA, BF16, F16X2, F32, PNAME, ROUND, ulp_T
from test_compose_algebra import bias_classes, class_map, compose_head
from test_decoder_gemm_ops import CONV3, PIXSHUF, TAIL, canary, conv_gather, last_form, rows_of, stage, stage_nchw, unstage

from burn_depth_amd import _lib

DC, PAIR, C1C3, HEAD = _lib.COMPOSE_DECONV_CONV, _lib.COMPOSE_DECONV_PAIR, _lib.COMPOSE_C1C3, _lib.COMPOSE_HEAD
KNAME = {DC: "deconv_conv", PAIR: "deconv_pair", C1C3: "c1c3", HEAD: "head"}
U = 2.0 ** -24
FILL = 7.25
GRID_ELEMS = 4096 * 256   # the compose kernels' capped grid: an element count beyond it makes the grid-stride loop repeat
# position constants: every tap / parity of a weight is scaled by its own factor, so a transposed or swapped tap changes the values
TAP2A = torch.tensor([[1.0, 1.5], [0.5, 2.0]])
TAP2B = torch.tensor([[0.75, 1.25], [1.75, 0.25]])
TAP3 = (0.6 + 0.1 * torch.arange(9.0)).reshape(3, 3)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=32)
def weights_of(kind, cin, cmid, cout, seed=0, w2_scale=1.0, b_out_mean=0.0):
    """-> (first weight, second weight, first bias or None, second bias or None), fp32, in the layouts of md_op_compose_weights."""
    g = gen(1000 * kind + 31 * cin + 7 * cmid + cout + seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if kind == DC:
        return rn(cin, cmid, 2, 2) / cin ** 0.5 * TAP2A, rn(cout, cmid) / cmid ** 0.5 * w2_scale, None, None
    if kind == PAIR:
        return rn(cin, cmid, 2, 2) / cin ** 0.5 * TAP2A, rn(cmid, cout, 2, 2) / cmid ** 0.5 * TAP2B * w2_scale, None, None
    first = rn(cmid, cin) / cin ** 0.5 if kind == C1C3 else rn(cin, cmid, 2, 2) / cin ** 0.5 * TAP2A
    return first, rn(cout, cmid, 3, 3) / (9 * cmid) ** 0.5 * TAP3 * w2_scale, rn(cmid) * 0.5, rn(cout) * 0.5 + b_out_mean


def compose_ref(kind, a, b):
    """The composed weight from the LAYERS (dtype of a, b): the response of layer 2 (layer 1 (unit impulses)). Bilinear with non-negative
    coefficients, so the same call on |a|, |b| is the sum of the products' magnitudes."""
    cin = a.shape[1] if kind == C1C3 else a.shape[0]
    eye = torch.eye(cin, dtype=a.dtype)
    if kind == DC:
        return F.conv2d(F.conv_transpose2d(eye[:, :, None, None], a, stride=2), b[:, :, None, None])
    if kind == PAIR:
        return F.conv_transpose2d(F.conv_transpose2d(eye[:, :, None, None], a, stride=2), b, stride=2)
    if kind == C1C3:   # out[co, y, x] = sum Wc[co, ci, u, v] in[ci, y + u - 1, x + v - 1]: an impulse at (1, 1) of channel ci answers Wc[co, ci, 2 - y, 2 - x]
        d = torch.zeros(cin, cin, 3, 3, dtype=a.dtype)
        d[:, :, 1, 1] = eye
        return F.conv2d(F.conv2d(d, a[:, :, None, None]), b, padding=1).flip(2, 3).permute(1, 0, 2, 3).contiguous()
    return compose_head(a, b)


def n_products(kind, cmid):
    return 4 * cmid if kind == HEAD else cmid


def swap_cico(out):
    """The buffer a kernel leaves when it writes element (c0, c1, tap) at (c1 * n0 + c0) * taps + tap."""
    return out.permute(1, 0, 2, 3).contiguous().reshape(out.shape)


def compose_eval(kind, a, b, mut=None):
    """The composed weight as index arithmetic in the dtype of a, b (the fp32 evaluation of the CPU tests), with the mutants."""
    if kind == DC:
        cout, cmid = b.shape
        wo = b.reshape(cmid, cout).t() if mut == "wo_cmid_cout" else b
        wd = a.transpose(2, 3) if mut == "q_transposed" else a
        out = torch.einsum("imyx,om->ioyx", wd, wo)
    elif kind == PAIR:
        cmid, cout = b.shape[:2]
        wb = b.reshape(cout, cmid, 2, 2).permute(1, 0, 2, 3) if mut == "wb_cout_cmid" else b
        # tap (ty, tx) = (2 dy1 + dy2, 2 dx1 + dx2): Wa at (dy1, dx1) = (p, r), Wb at (dy2, dx2) = (s, t)
        eq = "imst,mopr->iopsrt" if mut == "qa_qb" else "impr,most->iopsrt"
        out = torch.einsum(eq, a, wb).reshape(a.shape[0], cout, 4, 4)
    elif kind == C1C3:
        out = torch.einsum("omuv,mi->oiuv", b.transpose(2, 3) if mut == "tap_transposed" else b, a)
    else:
        cin, cout = a.shape[0], b.shape[0]
        out = torch.zeros(4 * cout, cin, 3, 3, dtype=a.dtype)
        half = (lambda t: int(t / 2)) if mut == "a_trunc" else (lambda t: t // 2)
        for py in range(2):
            for px in range(2):
                q = 2 * px + py if mut == "parity" else 2 * py + px
                for u in range(3):
                    for v in range(3):
                        ty, tx = py + u - 1, px + v - 1   # the deconvolution pixel, relative to (2y, 2x)
                        dy, dx = (tx & 1, ty & 1) if mut == "dydx" else (ty & 1, tx & 1)
                        out[q * cout:(q + 1) * cout, :, half(ty) + 1, half(tx) + 1] += torch.einsum("om,im->oi", b[:, :, u, v], a[:, :, dy, dx])
    return swap_cico(out) if mut == "cico_strides" else out


def bias_eval(w3, b_in, b_out, mut=None):
    """[9, cout] bias classes in the dtype of the inputs: b_out + b_in through the taps inside the map, with the mutants."""
    out = torch.zeros(9, w3.shape[0], dtype=w3.dtype)
    lo, hi = (2, 0) if mut == "valid_inverted" else (0, 2)
    for ry in range(3):
        for rx in range(3):
            acc = torch.zeros_like(b_out) if mut == "b_out_left_out" else b_out.clone()
            for u in range(3):
                for v in range(3):
                    outside = (ry == 0 and u == lo) or (ry == 2 and u == hi) or (rx == 0 and v == lo) or (rx == 2 and v == hi)
                    if outside and mut != "all_interior":
                        continue
                    acc = acc + w3[:, :, u, v] @ b_in
            out[3 * rx + ry if mut == "ryrx" else 3 * ry + rx] = acc
    return out


W_MUTANTS = {  # mutant -> (kinds it belongs to, is it something else than the identity at (cin, cmid, cout)?)
    "wo_cmid_cout": ((DC,), lambda cin, cmid, cout: cmid > 1 and cout > 1),
    "cico_strides": ((DC, PAIR, C1C3, HEAD), lambda cin, cmid, cout: cin > 1 and cout > 1),
    "q_transposed": ((DC,), lambda *s: True),
    "qa_qb": ((PAIR,), lambda *s: True),
    "wb_cout_cmid": ((PAIR,), lambda cin, cmid, cout: cmid > 1 and cout > 1),
    "dydx": ((HEAD,), lambda *s: True),
    "parity": ((HEAD,), lambda *s: True),
    "a_trunc": ((HEAD,), lambda *s: True),
    "tap_transposed": ((C1C3,), lambda *s: True),
}
B_MUTANTS = ("ryrx", "valid_inverted", "b_out_left_out", "all_interior")


def MUTANT_ACTIVE(mut, cin, cmid, cout):
    return mut in B_MUTANTS or W_MUTANTS[mut][1](cin, cmid, cout)


@functools.lru_cache(maxsize=32)
def tensor_case(kind, cin, cmid, cout):
    """-> the fp64 references and element bounds of (A), computed once and shared: (w, ref, E, ref9, E9), the last two None without biases."""
    a, b, b_in, b_out = w = weights_of(kind, cin, cmid, cout)
    ref = compose_ref(kind, a.double(), b.double())
    E = n_products(kind, cmid) * U * compose_ref(kind, a.double().abs(), b.double().abs())
    if b_in is None:
        return w, ref, E, None, None
    ref9 = bias_classes(b.double(), b_in.double(), b_out.double())
    E9 = (9 * cmid + 1) * U * bias_classes(b.double().abs(), b_in.double().abs(), b_out.double().abs())
    return w, ref, E, ref9, E9


def outside(got, ref, bound):
    return int(((got.double() - ref).abs() > bound).sum())


SMALL = [(5, 3, 7), (12, 20, 9), (6, 1, 5)]   # three different counts, none a multiple of 4; cmid = 1
LARGE = {DC: (517, 3, 509), PAIR: (259, 5, 254), C1C3: (343, 6, 341), HEAD: (169, 7, 173)}   # just beyond 4096 x 256 elements, cmid <= 8
TAPS = {DC: 4, PAIR: 16, C1C3: 9, HEAD: 36}


def test_the_large_cases_make_the_grid_stride_loop_repeat():
    for kind, (cin, cmid, cout) in LARGE.items():
        n = cin * cout * TAPS[kind]
        assert GRID_ELEMS < n < GRID_ELEMS + 8192 and cmid <= 8, (KNAME[kind], n)


@pytest.mark.parametrize("shape", SMALL + ["large"], ids=lambda s: s if isinstance(s, str) else "%d_%d_%d" % s)
@pytest.mark.parametrize("kind", [DC, PAIR, C1C3, HEAD], ids=KNAME.get)
def test_fp32_composition_is_inside_the_bound_and_mutants_are_not(kind, shape):
    cin, cmid, cout = LARGE[kind] if shape == "large" else shape
    (a, b, b_in, b_out), ref, E, ref9, E9 = tensor_case(kind, cin, cmid, cout)
    assert tuple(ref.shape) == {DC: (cin, cout, 2, 2), PAIR: (cin, cout, 4, 4), C1C3: (cout, cin, 3, 3), HEAD: (4 * cout, cin, 3, 3)}[kind]
    # the two formulations of the definition agree in fp64 (layers on impulses against index arithmetic)
    assert torch.allclose(compose_eval(kind, a.double(), b.double()), ref, rtol=0, atol=1e-13)
    got = compose_eval(kind, a, b)
    assert got.dtype == torch.float32 and outside(got, ref, E) == 0, f"{KNAME[kind]} {shape}: fp32 evaluation outside n u sum|a||b|"
    if kind == HEAD:   # five of the nine taps of a parity group have no product: bound 0, value 0
        assert (E == 0).sum() == 5 * 4 * cout * cin and (got[E == 0] == 0).all()
    if shape == "large":
        return
    for mut, (kinds, _) in W_MUTANTS.items():
        if kind in kinds:
            bad = compose_eval(kind, a, b, mut)
            assert (outside(bad, ref, E) > 0) == MUTANT_ACTIVE(mut, cin, cmid, cout), (mut, KNAME[kind], shape)
    if ref9 is not None:
        assert torch.allclose(bias_eval(b.double(), b_in.double(), b_out.double()), ref9, rtol=0, atol=1e-13)
        assert outside(bias_eval(b, b_in, b_out), ref9, E9) == 0, f"{KNAME[kind]} {shape}: fp32 bias classes outside the bound"
        for mut in B_MUTANTS:
            assert outside(bias_eval(b, b_in, b_out, mut), ref9, E9) > 0, (mut, KNAME[kind], shape)


def test_refusals_come_before_any_launch():
    """Each refusal is the entry's own error and needs no device: the handle and the pointers below are never dereferenced."""
    lib = _lib.load()
    dev, p, null = C.c_void_p(1), C.c_void_p(64), C.c_void_p(0)

    def err(kind, cin, cmid, cout, w1=p, w2=p, b1=null, b2=null, out=p, b9=null):
        code = lib.md_op_compose_weights(dev, kind, cin, cmid, cout, w1, w2, b1, b2, out, b9, None)
        return code, lib.md_last_error().decode()

    for kw in (dict(w1=null), dict(w2=null), dict(out=null)):
        assert err(DC, 4, 4, 4, **kw) == (_lib.MD_ERR_INVALID_ARG, "compose_weights: null argument")
    for kind in (-1, 4):
        code, msg = err(kind, 4, 4, 4)
        assert code == _lib.MD_ERR_INVALID_ARG and msg == f"compose_weights: kind {kind}"
    for chans in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        code, msg = err(C1C3, *chans)
        assert code == _lib.MD_ERR_SHAPE and msg == "compose_weights: channels %d -> %d -> %d" % chans
    for kind in (DC, PAIR):
        for kw in (dict(b9=p), dict(b1=p), dict(b1=p, b2=p, b9=p)):
            code, msg = err(kind, 4, 4, 4, **kw)
            assert code == _lib.MD_ERR_INVALID_ARG and msg.startswith(f"compose_weights: kind {kind} has no bias classes")
    for kind in (C1C3, HEAD):
        for kw in (dict(b9=p), dict(b9=p, b1=p), dict(b9=p, b2=p), dict(b1=p, b2=p)):
            code, msg = err(kind, 4, 4, 4, **kw)
            assert code == _lib.MD_ERR_INVALID_ARG and msg == "compose_weights: the bias classes need both layers' biases and bias9_out"


def test_header_symbols_and_library_agree_on_the_entry(repo_root):
    header = open(os.path.join(repo_root, "include", "mi_depth.h")).read()
    assert "md_op_compose_weights" in re.findall(r"^int\s+(md_[a-z0-9_]+)\s*\(", header, re.M)
    raw = C.CDLL(os.path.join(repo_root, "burn_depth_amd", "libmi_depth.so"))
    assert hasattr(raw, "md_op_compose_weights") and len(_lib.SYMBOLS["md_op_compose_weights"][1]) == 12
    m = re.search(r"typedef enum md_compose_kind \{([^}]*)\}", header)
    assert [s.strip() for s in m.group(1).split(",")] == [f"MD_COMPOSE_{n} = {v}" for n, v in (("DECONV_CONV", DC), ("DECONV_PAIR", PAIR), ("C1C3", C1C3), ("HEAD", HEAD))]


# ---------------------------------------------------------------------------------------------
# (B) the composition as the engine launches it
# ---------------------------------------------------------------------------------------------
MODES = [BF16, F16X2, F32]
MAPS = [(2, 2), (3, 5), (17, 19)]
B_, CIN, CIN_P = 2, 64, 128
LAUNCH = {DC: dict(cmid=48, cout=40, f=2, coff=8, pad=8), PAIR: dict(cmid=24, cout=36, f=4, coff=0, pad=4), C1C3: dict(cmid=48, cout=40, pad=8)}
L_MUTANTS = {DC: ("bias1_dropped",), PAIR: (), C1C3: ("border_all_interior", "fix_absolute", "bias1_dropped")}


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=32)
def launch_case(kind, H, W, prec):
    """The fp64 reference of the two uncomposed layers on the stored activations, and the per-element bound's terms, computed once."""
    k = LAUNCH[kind]
    cmid, cout = k["cmid"], k["cout"]
    # C1C3: a small 3x3 weight and a 3x3 bias around 4.5 keep the map inside [2, 8) (module docstring: the read-modify-write term)
    a, b, b_in, b_out = weights_of(kind, CIN, cmid, cout, 5, **(dict(w2_scale=0.3, b_out_mean=4.5) if kind == C1C3 else {}))
    g = gen(97 * kind + 13 * H + W + prec)
    x = ROUND[prec](torch.randn(B_, CIN, H, W, generator=g))
    bo = torch.randn(cout, generator=g) if kind == DC else None   # out_conv's bias: the launch's own
    a64, b64, x64, ax = a.double(), b.double(), x.double(), x.double().abs()
    Wc = compose_ref(kind, a64, b64)
    E = n_products(kind, cmid) * U * compose_ref(kind, a64.abs(), b64.abs())
    w_err = 0.5 * ulp_T(Wc.abs(), prec) + E
    c = dict(kind=kind, H=H, W=W, prec=prec, cmid=cmid, cout=cout, a=a, b=b, b_in=b_in, b_out=b_out, bo=bo, x=x, **{n: k[n] for n in ("f", "coff", "pad") if n in k})
    if kind == C1C3:
        ref = F.conv2d(F.conv2d(x64, a64[:, :, None, None], b_in.double()), b64, b_out.double(), padding=1)
        b9 = bias_classes(b64, b_in.double(), b_out.double())
        E9 = (9 * cmid + 1) * U * bias_classes(b64.abs(), b_in.double().abs(), b_out.double().abs())
        cls = class_map(H, W)
        pre = F.conv2d(x64, Wc, b9[4], padding=1)   # what the GEMM stores: the interior class everywhere
        border = (cls != 4)[None, :, :, None].expand(B_, H, W, cout)
        extra = nhwc(F.conv2d(ax, w_err, padding=1)) + E9[cls][None] + ulp_T(nhwc(ref).abs(), prec) * border
        c.update(border=border, v=nhwc(pre), cls=cls)
    else:
        f = k["f"]
        ref = F.conv_transpose2d(x64, a64, None, stride=2)
        ref = F.conv2d(ref, b64[:, :, None, None], bo.double()) if kind == DC else F.conv_transpose2d(ref, b64, None, stride=2)
        pre = ref
        extra = nhwc(F.conv_transpose2d(ax, w_err, stride=f))
    c.update(ref=nhwc(ref), extra=extra, a32=A_MFMA * pre.abs().max().item() / ref.abs().max().item())
    return c


def launch_eval(c, mut=None):
    """The launch in fp32 on the CPU: the fp32 product rounded to the operand type, the launch's operation, ONE rounding to T, and for
    C1C3 the border pixels' read-modify-write with its second rounding -> NHWC [B, OH, OW, cout]."""
    kind, prec, R = c["kind"], c["prec"], ROUND[c["prec"]]
    Wr = R(compose_eval(kind, c["a"], c["b"]))
    if kind != C1C3:
        bias = torch.zeros(c["cout"]) if (kind == PAIR or mut == "bias1_dropped") else c["bo"]
        return R(nhwc(F.conv_transpose2d(c["x"], Wr, bias, stride=c["f"])))
    b9 = bias_eval(c["b"], torch.zeros_like(c["b_in"]) if mut == "bias1_dropped" else c["b_in"], c["b_out"])
    v = R(conv_gather(c["x"], Wr) + b9[4]).reshape(B_, c["H"], c["W"], c["cout"])
    if mut == "border_all_interior":
        return v
    fix = (b9 if mut == "fix_absolute" else b9 - b9[4])[c["cls"]][None]
    return torch.where(c["border"], R(v + fix), v)


def launch_report(c, got):
    return close_check.close_report(got, c["ref"], c["prec"], c["a32"], c["extra"], slack_beyond_extra=True)


def launch_assert(c, got, what):
    return close_check.assert_close_in(got, c["ref"], c["prec"], c["a32"], extra=c["extra"], what=what, tag="compose_ops", slack_beyond_extra=True)


@pytest.mark.parametrize("prec", MODES, ids=PNAME.get)
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", [DC, PAIR, C1C3], ids=KNAME.get)
def test_launch_checker_accepts_fp32_and_rejects_mutants(kind, hw, prec):
    c = launch_case(kind, hw[0], hw[1], prec)
    what = f"fp32 evaluation, {KNAME[kind]} {hw}"
    assert launch_assert(c, launch_eval(c), what)["slack_share"] < 0.01
    assert c["cout"] % 4 == 0 and c["cout"] not in (CIN, c["cmid"]) and CIN_P > CIN
    if kind == C1C3:   # the premise of the read-modify-write term, on every border element, from the fp64 values alone
        v, ref, m = c["v"].abs(), c["ref"].abs(), c["border"]
        assert m.sum() == B_ * (hw[0] * hw[1] - max(hw[0] - 2, 0) * max(hw[1] - 2, 0)) * c["cout"]
        assert (ulp_T(v, BF16)[m] <= 2 * ulp_T(ref, BF16)[m]).all() and ref.min() >= 1.0
    for mut in L_MUTANTS[kind]:
        r = launch_report(c, launch_eval(c, mut))
        assert r["n_bad"] > 0 or r["slack_share"] >= 0.01, (mut, what)


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL + ["large"], ids=lambda s: s if isinstance(s, str) else "%d_%d_%d" % s)
@pytest.mark.parametrize("kind", [DC, PAIR, C1C3, HEAD], ids=KNAME.get)
def test_composed_tensors_against_fp64(dev, kind, shape):
    """The four compose kernels and compose_head_bias_kernel per element inside n u sum|a||b|; nothing written behind the tensors."""
    from burn_depth_amd import ops
    cin, cmid, cout = LARGE[kind] if shape == "large" else shape
    (a, b, b_in, b_out), ref, E, ref9, E9 = tensor_case(kind, cin, cmid, cout)
    n = ref.numel()
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    flat, flat9 = ops.compose_weights(dev, kind, cin, cmid, cout, a.cuda(), b.cuda(), cu(b_in), cu(b_out), tail=TAIL, fill=FILL)
    flat = flat.cpu()
    assert torch.isfinite(flat).all() and (flat[n:] == FILL).all(), "elements behind the product"
    got = flat[:n].reshape(ref.shape)
    ratio = ((got.double() - ref).abs() / E.clamp_min(1e-300)).max().item()
    print(f"[compose_ops] {KNAME[kind]} {shape}: {n} elements, worst err/bound {ratio:.3f}")
    assert outside(got, ref, E) == 0, f"{KNAME[kind]} {shape}: {outside(got, ref, E)} of {n} elements outside the bound, worst err/bound {ratio:.3f}"
    if shape == "large":   # the elements of the loop's second trip (the last n - 4096 x 256) and the very last ones
        assert n > GRID_ELEMS
        tail_got, tail_ref, tail_E = got.reshape(-1)[GRID_ELEMS:], ref.reshape(-1)[GRID_ELEMS:], E.reshape(-1)[GRID_ELEMS:]
        assert outside(tail_got, tail_ref, tail_E) == 0 and tail_got.abs().max() > 0 and tail_ref[-TAPS[kind]:].abs().max() > 0
        assert outside(got.reshape(-1)[-TAPS[kind]:], ref.reshape(-1)[-TAPS[kind]:], E.reshape(-1)[-TAPS[kind]:]) == 0
    if ref9 is None:
        assert flat9 is None
        return
    flat9 = flat9.cpu()
    assert torch.isfinite(flat9).all() and (flat9[9 * cout:] == FILL).all(), "elements behind bias9"
    got9 = flat9[:9 * cout].reshape(9, cout)
    assert outside(got9, ref9, E9) == 0, f"{KNAME[kind]} {shape}: bias classes, worst err/bound {((got9.double() - ref9).abs() / E9).max().item():.3f}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [C1C3, HEAD], ids=KNAME.get)
def test_composed_weight_alone_leaves_no_bias(dev, kind):
    """Without the three bias pointers the entry composes the weight alone, to the same bits as with them."""
    from burn_depth_amd import ops
    a, b, b_in, b_out = weights_of(kind, 5, 3, 7)
    w0, none = ops.compose_weights(dev, kind, 5, 3, 7, a.cuda(), b.cuda())
    w1, b9 = ops.compose_weights(dev, kind, 5, 3, 7, a.cuda(), b.cuda(), b_in.cuda(), b_out.cuda())
    assert none is None and b9.shape == (9, 7) and torch.equal(w0, w1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES, ids=PNAME.get)
@pytest.mark.parametrize("kind", [DC, PAIR], ids=KNAME.get)
def test_launched_deconvolution_products_against_the_uncomposed_layers(dev, kind, prec):
    """compose_deconv_conv / compose_deconv_pair -> MD_DECODER_GEMM_PIXSHUF f = 2 | 4 (deconv2() of run_decoder / the encoder's latent chains)
    against conv_transpose2d -> conv2d 1x1 (+ bias) | conv_transpose2d in fp64; columns outside the slice and rows behind the map stay canary."""
    from burn_depth_amd import ops
    for H, W in MAPS:
        c = launch_case(kind, H, W, prec)
        f, coff, cout = c["f"], c["coff"], c["cout"]
        ldo, rows = coff + cout + c["pad"], B_ * f * f * H * W
        wc, _ = ops.compose_weights(dev, kind, CIN, c["cmid"], cout, c["a"].cuda(), c["b"].cuda())
        bias = c["bo"].cuda() if kind == DC else torch.zeros(cout).cuda()   # DECONV_PAIR's layers are bias-free: the launch form wants a vector
        xr = stage_nchw(dev, c["x"], CIN_P, prec)
        x0 = xr.clone()
        out = stage(dev, canary(rows + TAIL, ldo), ldo, prec)
        ops.decoder_gemm(dev, PIXSHUF, xr, wc.contiguous(), bias, prec, B=B_, H=H, W=W, Cin=CIN, Cin_p=CIN_P, Cout=cout, out=out, ldo=ldo, ps_f=f, ps_coff=coff)
        fm = last_form()
        assert fm["K"] == CIN_P * (3 if prec == F16X2 else 1), fm   # split-half: three terms
        assert torch.equal(x0.view(torch.uint8), xr.view(torch.uint8))
        what = f"{KNAME[kind]} as pixel shuffle f{f} {H}x{W}"
        got = unstage(dev, out, rows + TAIL, ldo, prec)
        can = canary(rows + TAIL, ldo)
        assert torch.equal(got[rows:], can[rows:]), what + ": rows behind the map"
        keep = torch.ones(ldo, dtype=torch.bool)
        keep[coff:coff + cout] = False
        assert torch.equal(got[:rows][:, keep], can[:rows][:, keep]), what + ": columns outside the slice"
        launch_assert(c, got[:rows, coff:coff + cout].reshape(c["ref"].shape), what)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", MODES, ids=PNAME.get)
def test_launched_conv1x1_conv3x3_product_against_the_uncomposed_layers(dev, prec):
    """compose_c1c3 + compose_head_bias -> MD_DECODER_GEMM_CONV3 with bias9[4] -> border_bias_fix(bias9), as run_decoder launches head.conv0 on the
    product path, against conv2d 1x1 (+ bias) -> conv2d 3x3 pad 1 (+ bias) in fp64: every border class, the four corners, interior untouched."""
    from burn_depth_amd import ops
    for H, W in MAPS:
        c = launch_case(C1C3, H, W, prec)
        cout, M = c["cout"], B_ * H * W
        ldo = cout + c["pad"]
        wc, b9 = ops.compose_weights(dev, C1C3, CIN, c["cmid"], cout, c["a"].cuda(), c["b"].cuda(), c["b_in"].cuda(), c["b_out"].cuda())
        xr = stage_nchw(dev, c["x"], CIN_P, prec)
        x0 = xr.clone()
        out = stage(dev, canary(M + TAIL, ldo), ldo, prec)
        ops.decoder_gemm(dev, CONV3, xr, wc.contiguous(), b9[4].contiguous(), prec, B=B_, H=H, W=W, Cin=CIN, Cin_p=CIN_P, Cout=cout, out=out, ldo=ldo)
        fm = last_form()
        assert fm["K"] == 9 * CIN_P * (3 if prec == F16X2 else 1), fm
        assert torch.equal(x0.view(torch.uint8), xr.view(torch.uint8))
        what = f"c1c3 as conv3 + border fix {H}x{W}"
        mid = unstage(dev, out, M + TAIL, ldo, prec)
        can = canary(M + TAIL, ldo)
        assert torch.equal(mid[M:], can[M:]) and torch.equal(mid[:, cout:], can[:, cout:]), what + ": rows behind M / pad columns"
        fixed = ops.border_bias_fix(dev, mid[:M].reshape(B_, H, W, ldo).cuda(), cout, b9, prec).cpu()
        assert torch.equal(fixed[..., cout:], can[:M].reshape(B_, H, W, ldo)[..., cout:]), what + ": pad columns behind the border fix"
        inner = ~c["border"]
        assert torch.equal(fixed[..., :cout][inner], mid[:M, :cout].reshape(B_, H, W, cout)[inner]), what + ": interior pixels changed"
        launch_assert(c, fixed[..., :cout], what)
