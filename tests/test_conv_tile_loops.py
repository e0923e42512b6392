"""The decoder's two 3 x 3 convolution tile loops (gemm_impl.h: gemm256p_kernel<T, false, true, true>, the lean bias + ReLU form, and
gemm256r_kernel<T, false, true>, the form with residual inputs and a relu'd second output) through `ops.decoder_gemm`, at the smallest
launches that reach them: 1024 tiles of N = 256 with 9 or 36 k-tiles (gemm256_form: loop_ok).

* Each loop against the one-tile kernel bit for bit (`md_debug_gemm_persistent` 15 against 7; `ops.gemm_last_form()` must name the loop in
  the first half and the one-tile kernel in the second, so a moved threshold cannot make the comparison vacuous).
  [1, 512, 512, C], C = 64 | 256: exactly 1024 tiles, tile rows aligned with image rows, one and four channel blocks per tap.
  [2, 363, 363, 64]: 1030 tiles, the last one partial (114 rows); tiles straddle image rows and the boundary between the two images, so every
  combination of the border flags occurs inside a wave's 32 staged rows and the rows clamped behind M are read.
* Both loops against an fp64 convolution summed tap by tap from the definition at [2, 363, 363, 64], every element, and once more on the
  first and last row and column of each image alone: two kernels that share a wrong tap table agree with each other, not with this.

Bounds (tests/test_decoder_gemm_ops.py, EPI_STORE; u = 2^-24): 0.5 ulp_T with tie slack + A_MFMA max|acc + bias|, and for the residual form
u (|pre + res1| + |pre + res1 + res2|) for the two fp32 additions. out2 = relu(out) as values, tolerance 0."""
import functools

import pytest
import torch

import close_check
from close_check import A_MFMA, BF16, F16, PNAME

CONV3, T256 = 0, 0
EK_STORE = 2
ONE_TILE, LOOP_P, LOOP_R = 0, 1, 2
U = 2.0 ** -24
STRADDLE = (2, 363, 363, 64)
LEAN_SHAPES = [(1, 512, 512, 64), (1, 512, 512, 256), STRADDLE]
DT = {BF16: torch.bfloat16, F16: torch.float16}


@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


@functools.lru_cache(maxsize=2)
def operands(shape, prec, residual):
    B, H, W, C = shape
    M, dt = B * H * W, DT[prec]
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H + C + prec)
    x = torch.randn(M, C, generator=g, device="cuda").to(dt)
    w = (torch.randn(256, C, 3, 3, generator=g, device="cuda") / (9 * C) ** 0.5).to(dt).float()
    b = torch.randn(256, generator=g, device="cuda")
    r1, r2 = ((torch.randn(M, 256, generator=g, device="cuda").to(dt) for _ in range(2)) if residual else (None, None))
    return x, w, b, r1, r2


@functools.lru_cache(maxsize=2)
def both_forms(dev, shape, prec, residual):
    """-> [(out, out2 | None) of the tile loop, the same of the one-tile kernel]; asserts which kernel ran each."""
    from burn_depth_amd import _lib, ops
    lib = _lib.load()
    B, H, W, C = shape
    M, dt = B * H * W, DT[prec]
    x, w, b, r1, r2 = operands(shape, prec, residual)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid, tiles = max(cus & ~7, 8), -(-M // 256)
    assert tiles >= 1024
    res = []
    prev = lib.md_debug_gemm_persistent(15)
    try:
        for mask in (15, 7):
            lib.md_debug_gemm_persistent(mask)
            out = torch.full((M, 256), 3.0, device="cuda", dtype=dt)
            out2 = torch.full((M, 256), 5.0, device="cuda", dtype=dt) if residual else None
            ops.decoder_gemm(dev, CONV3, x, w, b, prec, T256, B=B, H=H, W=W, Cin=C, Cin_p=C, Cout=256, out=out, ldo=256, act=0 if residual else 1, res1=r1,
                             res2=r2, out2=out2)
            f = ops.gemm_last_form()
            assert f["tile"] == T256 and f["blocks"] == tiles, f
            if mask == 15:
                assert (f["family"], f["conv"], f["grid"]) == (LOOP_R if residual else LOOP_P, 1, grid), f
            else:
                assert (f["family"], f["ek"], f["grid"]) == (ONE_TILE, EK_STORE, tiles), f
            res.append((out, out2))
    finally:
        lib.md_debug_gemm_persistent(prev)
    return res


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", LEAN_SHAPES, ids=lambda s: "B%d_%dx%d_C%d" % s)
def test_lean_convolution_tile_loop_is_bit_identical_to_the_one_tile_kernel(dev, shape, prec):
    (loop, _), (one, _) = both_forms(dev, shape, prec, False)
    assert same_bits(loop, one)
    assert float(loop.float().max()) > 1.0 and float(loop.float().min()) == 0.0   # (bias + ReLU ran: not the fill value, nothing negative)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_residual_convolution_tile_loop_is_bit_identical_at_straddling_tiles(dev, prec):
    (loop, loop2), (one, one2) = both_forms(dev, STRADDLE, prec, True)
    assert same_bits(loop, one) and same_bits(loop2, one2)
    assert torch.equal(loop2.float(), torch.relu(loop.float())) and float(loop.float().abs().max()) > 1.0


def conv_fp64(shape, x, w, b):
    """pre = conv3x3(x, pad 1) + bias as rows [M, 256] in fp64, summed tap by tap from the definition."""
    B, H, W, C = shape
    xp = torch.zeros(B, H + 2, W + 2, C, dtype=torch.float64, device="cuda")
    xp[:, 1:H + 1, 1:W + 1] = x.double().reshape(B, H, W, C)
    pre = b.double().expand(B * H * W, 256).clone()
    for dy in range(3):
        for dx in range(3):
            pre += xp[:, dy:dy + H, dx:dx + W].reshape(B * H * W, C) @ w[:, :, dy, dx].double().t()
    return pre


def border_rows(shape):
    B, H, W, _ = shape
    y, x = torch.arange(H, device="cuda")[:, None], torch.arange(W, device="cuda")[None, :]
    edge = ((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).reshape(-1)
    return edge.repeat(B).nonzero().reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("residual", [False, True], ids=["lean", "residual"])
def test_convolution_tile_loops_against_fp64(dev, residual, prec):
    (got, got2), _ = both_forms(dev, STRADDLE, prec, residual)
    x, w, b, r1, r2 = operands(STRADDLE, prec, residual)
    pre = conv_fp64(STRADDLE, x, w, b)
    if residual:
        s1 = pre + r1.double()
        ref = s1 + r2.double()
        extra = U * (s1.abs() + ref.abs())
    else:
        ref, extra = torch.relu(pre), None
    amax = A_MFMA * pre.abs().max().item()
    what = "conv3 %s tile loop %s" % ("residual" if residual else "lean", PNAME[prec])
    close_check.assert_close_in(got.double(), ref, prec, amax / ref.abs().max().item(), extra=extra, what=what, tag="conv_tile_loops")
    rows = border_rows(STRADDLE)
    assert rows.numel() == 2 * (2 * 363 + 2 * 361)
    close_check.assert_close_in(got[rows].double(), ref[rows], prec, amax / ref[rows].abs().max().item(), extra=None if extra is None else extra[rows],
                                what=what + " image borders", tag="conv_tile_loops")
    if residual:
        assert torch.equal(got2.float(), torch.relu(got.float()))
