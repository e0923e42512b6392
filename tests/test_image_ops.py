"""Operator tests of the image-space resampling kernels (kernels/ops.hip) in the forms the engines launch: the NHWC bilinear resize with
padded pixel strides, the shared fp32 addend table and split-half storage (md_op_resize_nhwc_ex), the fused pyramid + split + patch
extraction in every storage type (md_op_pyramid_patchify), the final-depth post step of the NCHW resize and of its identity-size copy
(md_op_resize_bilinear_ex, post = 1), and split / merge at further geometries. The conventions are those of tests/test_operand_writers.py.

The reference. The tap indices and fractions (i0, i1, d) of an axis are part of the operation's DEFINITION (interpolate.rs:29-41, fp32) and
are computed in numpy float32 exactly as `axis_tap` computes them: one correctly rounded fp32 quotient for the scale; method 0
(MD_INTERP_CUSTOM) src = (o + .5) * scale - .5, floor, clamp; method 1 (MD_INTERP_BURN, align-corners) src = o * scale, 0 when out == 1.
Real-number coordinates are NOT the reference (at a width of 2048 the fp32 src is already 2^-12 from the real one). The blend
tl (1 - dx) + tr dx, ... is then evaluated in fp64 from the operand values as the storage type holds them (hi + lo for f16x2), the fp32
addend is added in fp64, and post = 1 applies 1 / clamp(., 1e-4f, 1e4f) in fp64.

Where the bounds come from (none is taken from a GPU result):

* Typed NHWC outputs, per element with `close_check.assert_close_in`: 0.5 ulp_T (1 + tie slack) + A_LN max|ref|, tie-slack users under 1 %.
  The blend is at most nine fp32 roundings (two subtractions 1 - d, six products, three sums: counted generously) of magnitudes
  <= max|in|, plus one for the addend: 10 * 2^-24 = 6e-7 of max|ref| against A_LN = 2e-6. The three-`fma` form of the 16-bit types has six.
  The CPU test evaluates BOTH forms in fp32 for every type and case and they pass with the slack share under 1 %.
* f32, method 0: bit-exact against `oracle.depth_pro_ref.resize_bilinear` (+ the addend, one fp32 addition), the project's standard.
* Identity-size cases, all types and both methods: d = 0 and v * 1 + w * 0 = v exactly for finite v, w, so the output must be
  round_T(fp32(in + addend)) (round_T(in) without an addend) bit for bit. No inf / NaN inputs; no -0 arises from seeded normal values.
* Pad columns (ld > C): the output buffer is pre-filled and columns C .. ld of every plane must come back byte-identical; the input's
  pad columns hold 1234, far from every value.
* Pyramid: tolerance 0. The expected bytes are `expect_store(want_f32)` (torch's casts) of the oracle's resize + split + patch extraction,
  for the block kernel and for the generic kernel each (not one against the other: both share the store helpers).
* post = 1: inside a constant plateau whose value the clamp replaces (0, -3, 5e-5 below; 3e4 above) every blend is the value or a value on
  the same side of the clamp, so the result is exactly fp32(1 / 1e-4f) or fp32(1 / 1e4f). A plateau AT a clamp bound (1e-4, 1e4) blends to
  v (1 - d) + v d, which fp32 may leave one ulp inside the open interval, so the exact check covers those two at identity size (where the
  blend is the value) and the checks below cover them elsewhere. f32 method 0: bit-exact against the oracle's fp32 resize with the same
  post step in fp32. Both methods, per element against fp64: A_LN max|ref| + 2^-23 |ref| + A_LN max|taps| / blend^2 -- the reciprocal's
  rounding and the blend's error (bounded as above) carried through d(1/r)/dr = 1 / r^2. max|taps| is the largest of the element's four
  taps, never more than max|in|. Inputs >= 0.05 keep the last term small.

CPU tests (no device): the fp32 evaluation of every case passes its bound, and each mutant is rejected wherever it is not the identity
(`nhwc_mutant_active`, `post_mutant_active`). Where the mutants ARE the identity:

* method swapped: equal input and output size (both give src = o, d = 0) and a one-pixel input.
* i1 left unclamped at the far edge of x (reads the first pixel of the next row): everywhere but method 0 with OW > W > 1. A 2:1 downscale
  never reaches the last pixel's successor; under method 1 the last src is W - 1 or a rounding residue next to it (d <= 2^-17, below every
  bound), which the test neither requires nor forbids to be rejected when it is not exactly 0.
* d taken from the clamped i0 instead of floor(src): EVERYWHERE within a rounding. i0 differs from floor(src) only where src < 0 (method 0,
  the near edge), and there i0 = i1 = 0: v (1 - d) + v d = v for any d. A bound cannot see it; it is listed because the issue lists it.
* addend read with stride ld: ld == C, no addend, or a 1 x 1 output.
* addend offset by the batch index: B == 1 or no addend.
* lo plane of the input dropped: every type but f16x2.
* addend added to the top-left tap before the blend: no addend, or every d = 0 (identity size; the 1 x 1 output, whose src is an integer
  under both methods; the one-pixel input under method 1, whose scale is 0).
* scale in / out under method 1: method 0; equal sizes; a 1 x 1 output (src = 0); a one-pixel input (every tap is that pixel).
* post: clamp after the reciprocal -- identity unless a blend is negative (every input here plants the -3 plateau); bounds 1e-3 / 1e3 --
  never the identity (every input has a clamped plateau); post on the taps before the blend -- identity at equal sizes (d = 0).
"""
import functools
import os

import numpy as np
import pytest
import torch

import close_check
from close_check import A_LN, BF16, F16, F16X2, F32, PNAME, rejects
from oracle import depth_pro_ref as R
from test_operand_writers import assert_bits, expect_load, expect_store, prefill

assert_close_in = functools.partial(close_check.assert_close_in, tag="image_ops")
STORE_PRECS = [BF16, F16, F32, F16X2]
F = np.float32
PAD_IN = 1234.0   # what the pad columns of the input hold


# ---------------------------------------------------------------------------------------------
# taps: the definition, in numpy float32
# ---------------------------------------------------------------------------------------------
def axis_taps(in_size, out_size, method, mut=None):
    """(i0, i1, d) of every output index of one axis, as `axis_tap` computes them (int64, int64, float32)."""
    o = np.arange(out_size, dtype=np.float32)
    if mut == "method_swapped":
        method = 1 - method
    if method == 0:
        scale = F(in_size) / F(out_size)
        src = (o + F(0.5)) * scale - F(0.5)
        f0 = np.floor(src)
        i0 = np.maximum(f0, F(0.0)).astype(np.int64)
        i1 = (f0 + F(1.0) if mut == "i1_unclamped" else np.minimum(f0 + F(1.0), F(in_size - 1))).astype(np.int64)
    else:
        if mut == "scale_in_over_out":
            scale = F(in_size) / F(out_size)
        else:
            scale = F(in_size - 1) / F(out_size - 1) if out_size > 1 else F(0.0)
        src = o * scale
        f0 = np.floor(src)
        i0 = np.clip(f0.astype(np.int64), 0, in_size - 1)
        i1 = i0 + 1 if mut == "i1_unclamped" else np.minimum(i0 + 1, in_size - 1)
    d = src - (i0.astype(np.float32) if mut == "d_from_clamped_i0" else f0)
    assert src.dtype == np.float32 and d.dtype == np.float32
    return i0, i1, d


def fma32(a, b, c):
    """fp32 fma (the product of two fp32 is exact in fp64; the double rounding of the sum is a self-test's concern only)."""
    return (a.double() * b.double() + c.double()).float()


def gather_taps(val, OH, OW, method, mut=None):
    """val [B, H, W, C] -> (tl, tr, bl, br) [B, OH, OW, C], dx [1, 1, OW, 1], dy [1, OH, 1, 1] (fp32). An unclamped i1 walks the flat
    pixel list into the next row (wrapping at the end of the tensor)."""
    B, H, W, C = val.shape
    y0, y1, dy = axis_taps(H, OH, method, None if mut == "i1_unclamped" else mut)
    x0, x1, dx = axis_taps(W, OW, method, mut)
    flat = val.reshape(B * H * W, C)
    bb = torch.arange(B).view(B, 1, 1)
    pick = lambda yy, xx: flat[((bb * H + torch.from_numpy(yy).view(1, OH, 1)) * W + torch.from_numpy(xx).view(1, 1, OW)) % (B * H * W)]  # noqa: E731
    return (pick(y0, x0), pick(y0, x1), pick(y1, x0), pick(y1, x1)), torch.from_numpy(dx).view(1, 1, OW, 1), torch.from_numpy(dy).view(1, OH, 1, 1)


def blend(taps, dx, dy, dtype, form):
    tl, tr, bl, br = (t.to(dtype) for t in taps)
    dx, dy = dx.to(dtype), dy.to(dtype)
    if form == "fma":  # the 16-bit types' three fused lerps (fp32 only)
        top = fma32(dx, tr - tl, tl)
        bottom = fma32(dx, br - bl, bl)
        return fma32(dy, bottom - top, top)
    top = tl * (1.0 - dx) + tr * dx
    bottom = bl * (1.0 - dx) + br * dx
    return top * (1.0 - dy) + bottom * dy


def addend_lookup(addend, filler, B, OH, OW, C, ld, mut):
    """The addend of every output element [B or 1, OH, OW, C]; the two indexing mutants read on into `filler` (what lies behind the table)."""
    if mut not in ("addend_stride_ld", "addend_batch_offset"):
        return addend.view(1, OH, OW, C)
    ext = torch.cat([addend.reshape(-1), filler])
    pix = (torch.arange(OH).view(1, OH, 1, 1) * OW + torch.arange(OW).view(1, 1, OW, 1))
    idx = pix * (ld if mut == "addend_stride_ld" else C) + torch.arange(C).view(1, 1, 1, C)
    if mut == "addend_batch_offset":
        idx = idx + torch.arange(B).view(B, 1, 1, 1) * (OH * OW * C)
    return ext[idx]


def nhwc_eval(val, OH, OW, method, addend=None, filler=None, ld=0, dtype=torch.float64, form="separate", mut=None):
    """[B, OH, OW, C] in `dtype` arithmetic from the operand values val [B, H, W, C] (fp32)."""
    B, _, _, C = val.shape
    tmut = mut if mut in ("method_swapped", "i1_unclamped", "d_from_clamped_i0", "scale_in_over_out") else None
    taps, dx, dy = gather_taps(val, OH, OW, method, tmut)
    a = None if addend is None else addend_lookup(addend, filler, B, OH, OW, C, ld or C, mut).to(dtype)
    if mut == "addend_before_blend" and a is not None:
        taps = (taps[0].to(dtype) + a, taps[1], taps[2], taps[3])
        return blend(taps, dx, dy, dtype, form)
    out = blend(taps, dx, dy, dtype, form)
    return out if a is None else out + a


def store_T(y32, prec):
    """fp32 values -> what the output holds, widened back."""
    C = y32.shape[-1]
    return expect_load(expect_store(y32.reshape(-1, C), prec, C), prec, C).reshape(y32.shape)


# ---------------------------------------------------------------------------------------------
# NHWC cases
# ---------------------------------------------------------------------------------------------
NHWC_CASES = [   # B, H, W, C, OH, OW
    (2, 5, 7, 8, 11, 13),        # C8 = 1, upscale
    (2, 6, 11, 24, 13, 29),      # C8 = 3: the division path
    (1, 37, 37, 64, 74, 74),     # the shift path, 1:2
    (1, 74, 74, 64, 37, 37),     # 2:1
    (1, 9, 40, 256, 20, 300),    # 9600 channel groups per row: more than one pass of the capped grid
    (2, 16, 12, 32, 16, 12),     # identity size: the aux-head form ("add the table")
    (1, 5, 9, 8, 1, 1),          # out == 1
    (1, 1, 1, 8, 3, 4),          # a one-pixel input
]
NHWC_ID = lambda c: "%dx%dx%dx%d-%dx%d" % c  # noqa: E731
NHWC_MUTANTS = ["method_swapped", "i1_unclamped", "d_from_clamped_i0", "addend_stride_ld", "addend_batch_offset", "lo_dropped",
                "addend_before_blend", "scale_in_over_out"]


def is_identity_size(case):
    return (case[1], case[2]) == (case[4], case[5])


@functools.lru_cache(maxsize=None)
def nhwc_input(case, prec):
    """(stored rows [B*H*W, planes * C] of seeded normal values, their fp32 values [B, H, W, C], the values of the hi plane alone)."""
    B, H, W, C, _, _ = case
    g = torch.Generator().manual_seed(sum(case) * 7 + prec)
    x = torch.randn(B * H * W, C, generator=g)   # every batch item its own values
    st = expect_store(x, prec, C)
    return st, expect_load(st, prec, C).reshape(B, H, W, C), st[:, :C].float().reshape(B, H, W, C)


@functools.lru_cache(maxsize=None)
def nhwc_addend(case):
    """(fp32 table [OH, OW, C], what the indexing mutants find behind it)."""
    B, _, _, C, OH, OW = case
    g = torch.Generator().manual_seed(sum(case) * 11 + 1)
    return torch.randn(OH, OW, C, generator=g) * 0.7 + 0.3, torch.randn(OH * OW * max(C + 8, B * C), generator=g) * 0.7 - 0.3


def far_edge_d(case, method):
    """The fraction at the last output column where its unclamped i1 leaves the row, else None."""
    _, _, W, _, _, OW = case
    _, i1, d = axis_taps(W, OW, method, "i1_unclamped")
    over = i1 > W - 1
    return float(d[over].max()) if over.any() else None


def nhwc_mutant_active(mut, case, prec, method, ld, with_addend):
    """True / False: the mutant must / must not be rejected; None: a rounding residue decides (module docstring)."""
    B, H, W, C, OH, OW = case
    same, one_in, one_out = is_identity_size(case), (H, W) == (1, 1), (OH, OW) == (1, 1)
    if mut == "method_swapped":
        return not same and not one_in
    if mut == "i1_unclamped":
        if method == 0:
            return OW > W > 1
        d = far_edge_d(case, method)
        return False if (d is None or d == 0.0 or W == 1) else None
    if mut == "d_from_clamped_i0":
        return False
    if mut == "addend_stride_ld":
        return with_addend and ld > C and OH * OW > 1
    if mut == "addend_batch_offset":
        return with_addend and B > 1
    if mut == "lo_dropped":
        return prec == F16X2
    if mut == "addend_before_blend":
        dmax = max(axis_taps(H, OH, method)[2].max(), axis_taps(W, OW, method)[2].max())
        assert dmax == 0.0 or dmax > 1e-3
        return with_addend and dmax > 0.0
    if mut == "scale_in_over_out":
        return method == 1 and not same and not one_in and not one_out
    raise KeyError(mut)


def test_axis_taps_are_the_oracles():
    """The numpy taps are the oracle's (method 0: `_axis_taps`) and obey the definition's edge rules."""
    for (i, o) in [(7, 13), (74, 37), (40, 300), (1, 4), (9, 1), (12, 12), (2048, 1500)]:
        a0, a1, ad = axis_taps(i, o, 0)
        b0, b1, bd = R._axis_taps(i, o)
        assert np.array_equal(a0, b0.numpy()) and np.array_equal(a1, b1.numpy()) and np.array_equal(ad, bd.numpy())
        for m in (0, 1):
            i0, i1, d = axis_taps(i, o, m)
            assert i0.min() >= 0 and i1.max() <= i - 1 and ((i1 == i0) | (i1 == i0 + 1)).all() and d.min() >= 0 and d.max() < 1
    assert np.array_equal(axis_taps(9, 1, 1)[0], [0]) and axis_taps(9, 1, 1)[2][0] == 0
    assert np.array_equal(axis_taps(9, 1, 0)[0], [4]) and axis_taps(9, 1, 0)[2][0] == 0
    x = torch.randn(2, 3, 6, 11, generator=torch.Generator().manual_seed(0))
    for m in (0, 1):   # the fp32 evaluation of the reference formula IS the oracle's resize, bit for bit
        got = nhwc_eval(x.permute(0, 2, 3, 1).contiguous(), 13, 29, m, dtype=torch.float32)
        assert torch.equal(got, R.resize_bilinear(x, (13, 29), m).permute(0, 2, 3, 1))


@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case", NHWC_CASES, ids=NHWC_ID)
def test_nhwc_checker_accepts_fp32_and_rejects_mutants(case, prec):
    B, H, W, C, OH, OW = case
    _, val, hi_only = nhwc_input(case, prec)
    table, filler = nhwc_addend(case)
    for method in (0, 1):
        for addend in (None, table):
            what = f"fp32 evaluation {NHWC_ID(case)} m{method} addend={addend is not None}"
            ref = nhwc_eval(val, OH, OW, method, addend)
            for form in ("separate", "fma"):
                got = store_T(nhwc_eval(val, OH, OW, method, addend, dtype=torch.float32, form=form), prec)
                assert_close_in(got, ref, prec, A_LN, what=f"{what} {form}")
                if is_identity_size(case):
                    want = val if addend is None else val + addend
                    assert torch.equal(got, store_T(want, prec)), what
            for mut in NHWC_MUTANTS:
                for ld in ((C, C + 8) if mut == "addend_stride_ld" else (C,)):
                    active = nhwc_mutant_active(mut, case, prec, method, ld, addend is not None)
                    if active is None:
                        continue
                    src = hi_only if mut == "lo_dropped" else val
                    got = store_T(nhwc_eval(src, OH, OW, method, addend, filler, ld, torch.float32, mut=mut), prec)
                    assert rejects(got, ref, prec, A_LN) == active, (mut, what, ld)


# ---------------------------------------------------------------------------------------------
# pyramid cases
# ---------------------------------------------------------------------------------------------
PYRAMID_CASES = [   # S, window, patch, method, the block kernel accepts it
    (256, 64, 16, 0, True),      # the smallest block geometry: 4 * 48 + 64 = 256, 2 * 32 + 64 = 128
    (192, 48, 16, 0, False),     # strides 36 and 24: off the patch grid
    (128, 32, 8, 0, False),      # patch 8
    (256, 64, 16, 1, False),     # align-corners taps leave the 64-pixel block
]
PYRAMID_ID = lambda c: "S%d-w%d-p%d-m%d" % c[:4]  # noqa: E731
PYRAMID_B = 2
REFUSED_PYRAMID = (160, 40, 8)   # stride0 = 30: level-0 rows would be read at 8-byte alignment


def pyramid_geometry(S, win):
    (s0, n0), (s1, n1) = R.split_geometry(S, win, 0.25), R.split_geometry(S // 2, win, 0.5)
    return s0, n0, s1, n1


@functools.lru_cache(maxsize=None)
def pyramid_case(S, win, ps, method):
    """(x [2, 3, S, S], want fp32 [rows, 3 ps^2]): the oracle's resize + split + patch extraction (encoder.rs:326-344). The input mixes
    magnitudes from 1e-3 to beyond the f16 range (finite: a blend with an infinity has no defined value)."""
    g = torch.Generator().manual_seed(S + win + ps + method)
    x = torch.randn(PYRAMID_B, 3, S, S, generator=g) * torch.tensor([1e-3, 0.05, 1.0, 30.0, 600.0])[torch.randint(0, 5, (PYRAMID_B, 3, S, S), generator=g)]
    x.view(-1)[torch.randint(0, x.numel(), (64,), generator=g)] = torch.tensor([1e5, -1e5, 65520.0, -65504.0] * 16)
    x1, x2 = R.resize_bilinear_scale(x, (0.5, 0.5), method), R.resize_bilinear_scale(x, (0.25, 0.25), method)
    tiles = torch.cat([R.split(x, win, 0.25)[0], R.split(x1, win, 0.5)[0], x2], 0)
    gp = win // ps
    want = tiles.reshape(-1, 3, gp, ps, gp, ps).permute(0, 2, 4, 1, 3, 5).reshape(-1, 3 * ps * ps)
    return x, want.contiguous()


def test_pyramid_geometries():
    """The cases are what their comments say: which kernel serves them, 16-byte aligned level-0 reads, and the refused stride."""
    for S, win, ps, method, blocks in PYRAMID_CASES:
        s0, n0, s1, n1 = pyramid_geometry(S, win)
        assert S == 4 * win and win % ps == 0 and ps % 8 == 0 and s0 % 4 == 0
        assert (n0 - 1) * s0 + win == S and (n1 - 1) * s1 + win == S // 2
        ok = method == 0 and ps == 16 and S % 64 == 0 and s0 % 16 == 0 and s1 % 16 == 0
        assert ok == blocks, (S, win, ps, method)
    assert pyramid_geometry(192, 48)[::2] == (36, 24)
    S, win, ps = REFUSED_PYRAMID
    s0, n0, s1, n1 = pyramid_geometry(S, win)
    assert s0 == 30 and S == 4 * win and win % ps == 0 and (n0 - 1) * s0 + win == S   # a valid split that only the 16-byte reads rule out
    x, want = pyramid_case(128, 32, 8, 0)
    for prec in (F16, F16X2):   # the input reaches the f16 saturation and a non-zero lo plane
        st = expect_store(want, prec, want.shape[1])
        assert (st[:, :want.shape[1]].float().abs() == 65504.0).any()
    assert (expect_store(want, F16X2, want.shape[1])[:, want.shape[1]:] != 0).any()


# ---------------------------------------------------------------------------------------------
# post = 1 cases
# ---------------------------------------------------------------------------------------------
LO_F, HI_F = F(1e-4), F(1e4)
R_LO, R_HI = float(F(1.0) / LO_F), float(F(1.0) / HI_F)   # fp32(1 / 1e-4f), fp32(1 / 1e4f)
PLATEAU_VALUES = [0.0, -3.0, 5e-5, 1e-4, 1e4, 3e4]
POST_CASES = [   # (B, C, H, W), (OH, OW), input variants
    ((1, 2, 7, 5), (13, 17), 2),          # four 3 x 3 plateaus fit: two inputs carry the six values
    ((1, 1, 33, 1300), (50, 2100), 1),    # three 1024-column chunks
    ((2, 1, 9, 9), (9, 9), 1),            # identity size: copy_post_kernel
]
POST_ID = lambda c: "%dx%dx%dx%d-%dx%d" % (c[0] + c[1])  # noqa: E731
POST_MUTANTS = ["clamp_after_reciprocal", "bounds_1e-3_1e3", "post_before_blend"]


@functools.lru_cache(maxsize=None)
def post_input(shape, variant):
    """(x uniform in [0.05, 20] with planted constant plateaus, [(value, plane, y0, x0, h, w)])."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + variant)
    x = torch.rand(B * C, H, W, generator=g) * 19.95 + 0.05
    if shape == (1, 2, 7, 5):
        slots = [(p, y, xx, 3, 3) for p in range(2) for (y, xx) in ((0, 0), (4, 2))]
        values = [[0.0, -3.0, 5e-5, 1e-4], [-3.0, 1e4, 3e4, 0.0]][variant]
    elif shape == (1, 1, 33, 1300):
        slots = [(0, 2 + 5 * k, 60 + 244 * k, 4, 7) for k in range(6)]    # spread over the three column chunks of the output
        values = PLATEAU_VALUES
    else:
        slots = [(p, y, xx, 3, 3) for p in range(2) for (y, xx) in ((0, 0), (0, 5), (5, 1))]
        values = PLATEAU_VALUES
    plateaus = []
    for v, (p, y, xx, h, w) in zip(values, slots):
        x[p, y:y + h, xx:xx + w] = v
        plateaus.append((float(F(v)), p, y, xx, h, w))
    return x.reshape(B, C, H, W), plateaus


def post_step(r, mut=None):
    lo, hi = (1e-3, 1e3) if mut == "bounds_1e-3_1e3" else (float(LO_F), float(HI_F))
    lo, hi = torch.tensor(lo, dtype=r.dtype), torch.tensor(hi, dtype=r.dtype)   # (fp32: rounds 1e-3 / 1e3 as the literal would)
    if mut == "clamp_after_reciprocal":
        return torch.minimum(torch.maximum(1.0 / r, lo), hi)
    return 1.0 / torch.minimum(torch.maximum(r, lo), hi)


def post_eval(x, out_hw, method, dtype=torch.float64, mut=None):
    """-> (1 / clamp(blend) [B, C, OH, OW], the blend, the largest |tap| of every element), NCHW planes as one-channel NHWC images."""
    B, C, H, W = x.shape
    taps, dx, dy = gather_taps(x.reshape(B * C, H, W, 1), out_hw[0], out_hw[1], method)
    tapmax = torch.stack([t.abs() for t in taps]).amax(0).double()
    if mut == "post_before_blend":
        taps = tuple(post_step(t.to(dtype)) for t in taps)
        out = b = blend(taps, dx, dy, dtype, "separate")
    else:
        b = blend(taps, dx, dy, dtype, "separate")
        out = post_step(b, mut)
    shp = (B, C, out_hw[0], out_hw[1])
    return out.reshape(shp), b.reshape(shp), tapmax.reshape(shp)


def post_bound_extra(ref, blend64, tapmax):
    """2^-23 |ref| + A_LN max|taps| / blend^2; four zero taps blend to an exact zero (no term), a zero blend of non-zero taps has no bound."""
    return 2.0 ** -23 * ref.abs() + torch.where(tapmax == 0, torch.zeros_like(tapmax), A_LN * tapmax / (blend64 * blend64).clamp_min(1e-300))


def plateau_interior(x_shape, out_hw, method, plateau):
    """Output elements whose four taps all lie inside the plateau -> bool [B*C, OH, OW]."""
    B, C, H, W = x_shape
    _, p, y, xx, h, w = plateau
    y0, y1, _ = axis_taps(H, out_hw[0], method)
    x0, x1, _ = axis_taps(W, out_hw[1], method)
    my = torch.from_numpy((y0 >= y) & (y1 <= y + h - 1))
    mx = torch.from_numpy((x0 >= xx) & (x1 <= xx + w - 1))
    m = torch.zeros(B * C, out_hw[0], out_hw[1], dtype=torch.bool)
    m[p] = my[:, None] & mx[None, :]
    return m


def plateau_expectation(v, same_size):
    """The exact result inside a plateau of value v, or None where fp32 leaves it open (a value AT a clamp bound, blended)."""
    if v < float(LO_F) or (same_size and v == float(LO_F)):
        return R_LO
    if v > float(HI_F) or (same_size and v == float(HI_F)):
        return R_HI
    return None


def post_oracle_fp32(x, out_hw, method):
    return post_step(R.resize_bilinear(x, out_hw, method))


def post_mutant_active(mut, shape, out_hw):
    return not (mut == "post_before_blend" and tuple(shape[2:]) == tuple(out_hw))


def check_post(got, x, plateaus, out_hw, method, what):
    """Everything a post = 1 result is held to; `got` fp32 [B, C, OH, OW]. -> the close_check report."""
    same = tuple(x.shape[2:]) == tuple(out_hw)
    ref, b64, tapmax = post_eval(x, out_hw, method)
    flat = got.reshape(-1, *out_hw)
    for pl in plateaus:
        m = plateau_interior(x.shape, out_hw, method, pl)
        assert m.sum() >= 4, (what, pl)
        want = plateau_expectation(pl[0], same)
        if want is not None:
            assert (flat[m] == want).all(), f"{what}: plateau {pl[0]} is not exactly {want}"
    if method == 0:
        assert_bits(got, post_oracle_fp32(x, out_hw, 0), f"{what} against the oracle's fp32 evaluation")
    return assert_close_in(got, ref, F32, A_LN, extra=post_bound_extra(ref, b64, tapmax), what=what)


def test_post_constants():
    assert R_LO == 10000.0 and abs(R_HI - 1e-4) < 1e-11   # fp32(1 / 1e-4f) is 1e4 exactly
    assert plateau_expectation(float(LO_F), False) is None and plateau_expectation(float(LO_F), True) == R_LO
    assert plateau_expectation(float(HI_F), False) is None and plateau_expectation(float(HI_F), True) == R_HI
    assert plateau_expectation(float(F(5e-5)), False) == R_LO and plateau_expectation(-3.0, False) == R_LO and plateau_expectation(3e4, False) == R_HI
    seen = set()
    for shape, out_hw, variants in POST_CASES:
        for v in range(variants):
            x, pls = post_input(shape, v)
            seen |= {round(p[0], 9) for p in pls}
            assert any(p[0] == -3.0 for p in pls) and x.min() == -3.0 and x.max() <= 3e4
            rest = torch.ones_like(x.reshape(-1, *shape[2:]), dtype=torch.bool)
            for _, p, y, xx, h, w in pls:
                assert h >= 3 and w >= 3
                rest[p, y:y + h, xx:xx + w] = False
            assert rest.any() and x.reshape(-1, *shape[2:])[rest].min() >= 0.05
    assert seen == {round(float(F(v)), 9) for v in PLATEAU_VALUES}
    assert (2100 + 1023) // 1024 == 3


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("case", POST_CASES, ids=POST_ID)
def test_post_checker_accepts_fp32_and_rejects_mutants(case, method):
    shape, out_hw, variants = case
    for v in range(variants):
        x, pls = post_input(shape, v)
        what = f"fp32 evaluation post {POST_ID(case)} m{method} input {v}"
        got = post_oracle_fp32(x, out_hw, method)
        assert torch.equal(got, post_eval(x, out_hw, method, torch.float32)[0])
        check_post(got, x, pls, out_hw, method, what)
        ref, b64, tapmax = post_eval(x, out_hw, method)
        extra = post_bound_extra(ref, b64, tapmax)
        for mut in POST_MUTANTS:
            bad = post_eval(x, out_hw, method, torch.float32, mut)[0]
            assert rejects(bad, ref, F32, A_LN, extra=extra) == post_mutant_active(mut, shape, out_hw), (mut, what)


# ---------------------------------------------------------------------------------------------
# split / merge cases
# ---------------------------------------------------------------------------------------------
SPLIT_CASES = [((3, 1, 64, 64), 64, 0.25), ((1, 2, 96, 96), 32, 0.5), ((1, 2, 104, 104), 32, 0.25)]   # shape, window, overlap
SPLIT_UNTILED = ((1, 2, 96, 96), 32, 0.25)   # stride 24, 4 steps: 3 * 24 + 32 = 104 > 96 -- no tiling, in the reference either
MERGE_CASES = [((18, 3, 8, 12), 2, 1), ((4, 2, 6, 6), 1, 0), ((25, 1, 10, 10), 1, 2)]                  # tiles, batch, padding


def arange_like(shape):
    n = int(np.prod(shape))
    assert n < 2 ** 24   # every index its own fp32 value
    return torch.arange(n, dtype=torch.float32).reshape(shape)


def test_split_merge_cases_are_what_they_claim():
    assert R.split_geometry(64, 64, 0.25)[1] == 1
    assert R.split_geometry(96, 32, 0.5) == (16, 5) and R.split_geometry(104, 32, 0.25) == (24, 4)
    stride, steps = R.split_geometry(96, 32, 0.25)
    assert (steps - 1) * stride + 32 > 96
    with pytest.raises(RuntimeError):   # the last tiles are cut short: the oracle cannot stack them (the reference's slice panics)
        R.split(arange_like(SPLIT_UNTILED[0]), 32, 0.25)
    (n, c, h, w), batch, pad = MERGE_CASES[2]
    out = R.merge(arange_like((n, c, h, w)), batch, pad)
    assert out.shape == (1, 1, 10 + 4 * 6, 10 + 4 * 6)   # the last `pad` rows / columns lie past steps * interior: the clamp j <= steps - 1
    assert R.merge(arange_like(MERGE_CASES[0][0]), 2, 1).shape == (2, 3, 8 + 2 * 6, 12 + 2 * 10)


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


RECORD = {}  # (kernel, precision name) -> [worst error / bound, largest slack-user share, elements] or a bit-exact element count


def record(kernel, pname, r):
    old = RECORD.setdefault((kernel, pname), [0.0, 0.0, 0])
    old[0], old[1], old[2] = max(old[0], r["worst_ratio"]), max(old[1], r["slack_share"]), old[2] + r["n"]


def record_exact(kernel, pname, n):
    RECORD[(kernel, pname)] = RECORD.get((kernel, pname), 0) + n


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    """With IMAGE_OPS_ERRORS=<path> the worst error / bound per (kernel, precision) and the slack-user share are written there."""
    yield
    path = os.environ.get("IMAGE_OPS_ERRORS")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("kernel precision | worst error / bound over all elements | largest share of tie-slack users | elements compared\n")
            for (k, p), v in sorted(RECORD.items()):
                if isinstance(v, list):
                    f.write(f"{k:32s} {p:8s} | {v[0]:.3f} | {v[1]:.2e} | {v[2]}\n")
                else:
                    f.write(f"{k:32s} {p:8s} | bit-exact | - | {v}\n")


def raw_pixels(st, C, ld, fill):
    """Stored rows [n, planes * C] -> pixels [n, planes * ld] with `fill` in the pad columns of every plane."""
    planes = st.shape[1] // C
    raw = fill.clone()
    assert raw.shape == (st.shape[0], planes * ld) and raw.dtype == st.dtype
    for p in range(planes):
        raw[:, p * ld: p * ld + C] = st[:, p * C: (p + 1) * C]
    return raw


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case", NHWC_CASES, ids=NHWC_ID)
def test_resize_nhwc_forms_against_fp64(dev, case, prec):
    """Both methods x ld in {C, C + 8} x with / without the addend table [OH, OW, C]: every element within the derived bound, the pad
    columns of the output untouched, f32 method 0 bit-exact against the oracle, identity size bit-exact in every type."""
    from burn_depth_amd import ops
    B, H, W, C, OH, OW = case
    st, val, _ = nhwc_input(case, prec)
    table, _ = nhwc_addend(case)
    planes = 2 if prec == F16X2 else 1
    name = "resize_nhwc identity" if is_identity_size(case) else "resize_nhwc"
    for method in (0, 1):
        for addend in (None, table):
            ref = nhwc_eval(val, OH, OW, method, addend)
            exact = None
            if is_identity_size(case):
                exact = val if addend is None else val + addend
            elif prec == F32 and method == 0:
                exact = R.resize_bilinear(val.permute(0, 3, 1, 2), (OH, OW), 0).permute(0, 2, 3, 1)
                exact = exact if addend is None else exact + addend
            for ld in (C, C + 8):
                what = f"resize_nhwc {NHWC_ID(case)} m{method} ld={ld} addend={addend is not None}"
                xin = raw_pixels(st, C, ld, torch.full((B * H * W, planes * ld), PAD_IN, dtype=st.dtype)).reshape(B, H, W, planes * ld)
                fill = prefill((B * OH * OW, planes * ld), st.dtype)
                got = ops.resize_nhwc_ex(dev, xin.cuda(), C, fill.reshape(B, OH, OW, planes * ld).cuda(), method, prec,
                                         None if addend is None else addend.cuda()).cpu().reshape(B * OH * OW, planes * ld)
                pad = torch.ones(planes * ld, dtype=torch.bool)
                for p in range(planes):
                    pad[p * ld: p * ld + C] = False
                assert_bits(got[:, pad], fill[:, pad], f"{what}: pad columns")
                rows = torch.cat([got[:, p * ld: p * ld + C] for p in range(planes)], 1)
                record(name, PNAME[prec], assert_close_in(expect_load(rows, prec, C).reshape(B, OH, OW, C), ref, prec, A_LN, what=what))
                if exact is not None:
                    assert_bits(rows, expect_store(exact.reshape(-1, C), prec, C), f"{what}: stored bytes")
                    record_exact(name + " (bits)", PNAME[prec], rows.numel())


@pytest.mark.gpu
def test_resize_nhwc_ex_argument_checks(dev):
    from burn_depth_amd import _lib, ops
    x = torch.zeros(1, 2, 2, 16).cuda()
    out = torch.zeros(1, 3, 3, 16).cuda()
    lib = _lib.load()
    call = lambda C, ld_in, ld_out, method, prec: lib.md_op_resize_nhwc_ex(dev.handle, ops._p(x), 1, 2, 2, C, ld_in, ops._p(out), 3, 3, ld_out,  # noqa: E731
                                                                            method, None, prec, None)
    assert call(8, 8, 8, 1, F32) == 0
    assert call(16, 8, 16, 1, F32) == _lib.MD_ERR_INVALID_ARG and call(16, 16, 8, 1, F32) == _lib.MD_ERR_INVALID_ARG   # ld < C
    assert call(4, 8, 8, 1, F32) == _lib.MD_ERR_UNSUPPORTED and call(8, 12, 8, 1, F32) == _lib.MD_ERR_UNSUPPORTED     # C % 8, ld % 8
    assert call(8, 8, 8, 2, F32) == _lib.MD_ERR_INVALID_ARG
    for prec in (2, 5):   # e4m3 has no NHWC maps
        assert call(8, 8, 8, 1, prec) == _lib.MD_ERR_INVALID_ARG
    with pytest.raises(_lib.MdError) as e:   # the plain entry keeps its three types
        _lib.check(lib.md_op_resize_nhwc(dev.handle, ops._p(x), 1, 2, 2, 8, ops._p(out), 3, 3, 1, F16X2, None))
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    with pytest.raises(_lib.MdError) as e:
        ops.resize_bilinear(dev, torch.zeros(1, 1, 4, 4).cuda(), (5, 5), 0, post=2)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case", PYRAMID_CASES, ids=PYRAMID_ID)
def test_pyramid_patchify_stored_bytes(dev, case, prec):
    """The block kernel (where the geometry admits it) and the generic kernel, each against the expected stored bytes."""
    from burn_depth_amd import ops
    S, win, ps, method, blocks = case
    x, want = pyramid_case(S, win, ps, method)
    expect = expect_store(want, prec, want.shape[1])
    xc = x.cuda()
    for force_generic in (False, True):   # (without the flag a generic-only geometry runs the generic kernel too)
        got = ops.pyramid_patchify(dev, xc, win, ps, method, prec, force_generic=force_generic)
        assert_bits(got, expect, f"pyramid_patchify {PYRAMID_ID(case)} {PNAME[prec]} generic={force_generic}")
        record_exact("pyramid_patchify " + ("generic" if force_generic or not blocks else "blocks"), PNAME[prec], expect.numel())


@pytest.mark.gpu
def test_pyramid_patchify_refuses_a_misaligned_level0_stride(dev):
    """S = 160, window 40, patch 8: stride0 = 30. Refused before any launch (the output keeps its pre-fill); no such geometry is run."""
    from burn_depth_amd import _lib, ops
    S, win, ps = REFUSED_PYRAMID
    x = torch.zeros(1, 3, S, S).cuda()
    for prec in STORE_PRECS:
        for method in (0, 1):
            rows = (25 + 9 + 1) * (win // ps) ** 2
            out = torch.full((rows, 3 * ps * ps * (2 if prec == F16X2 else 1)), 7.0, dtype=ops._RAW_DTYPE[prec]).cuda()
            with pytest.raises(_lib.MdError) as e:
                ops.pyramid_patchify(dev, x, win, ps, method, prec, out=out)
            assert e.value.code == _lib.MD_ERR_UNSUPPORTED
            torch.cuda.synchronize()
            assert (out == 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("case", POST_CASES, ids=POST_ID)
def test_resize_bilinear_post_step(dev, case, method):
    """post = 1 (the final depth): plateaus exact, method 0 bit-exact against the oracle, both methods within the derived bound; and
    post = 0 of the same launch still is the plain resize."""
    from burn_depth_amd import ops
    shape, out_hw, variants = case
    same = tuple(shape[2:]) == tuple(out_hw)
    for v in range(variants):
        x, pls = post_input(shape, v)
        got = ops.resize_bilinear(dev, x.cuda(), out_hw, method, post=1).cpu()
        r = check_post(got, x, pls, out_hw, method, f"resize_bilinear post=1 {POST_ID(case)} m{method} input {v}")
        record("copy_post" if same else "resize_bilinear post=1 m%d" % method, "f32", r)
        plain = ops.resize_bilinear(dev, x.cuda(), out_hw, method, post=0).cpu()
        if method == 0 or same:
            assert_bits(plain, R.resize_bilinear(x, out_hw, method), "post = 0")


@pytest.mark.gpu
def test_split_and_merge_bit_exact(dev):
    from burn_depth_amd import _lib, ops
    for shape, win, overlap in SPLIT_CASES:
        x = arange_like(shape)
        want, steps, _ = R.split(x, win, overlap)
        got, gsteps = ops.split(dev, x.cuda(), win, overlap)
        assert gsteps == steps
        assert_bits(got, want.contiguous(), f"split {shape} window {win} overlap {overlap}")
        record_exact("split", "f32", want.numel())
    shape, win, overlap = SPLIT_UNTILED
    with pytest.raises(_lib.MdError) as e:
        ops.split(dev, arange_like(shape).cuda(), win, overlap)
    assert e.value.code == _lib.MD_ERR_SHAPE
    for shape, batch, pad in MERGE_CASES:
        t = arange_like(shape)
        want = R.merge(t, batch, pad)
        got = ops.merge(dev, t.cuda(), batch, pad)
        assert_bits(got, want.contiguous(), f"merge {shape} batch {batch} padding {pad}")
        record_exact("merge", "f32", want.numel())
