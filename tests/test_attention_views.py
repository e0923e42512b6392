"""GPU operator tests of `md_op_attention_views` (cross-view keys, kernels/attention.hip MV form) against an fp64 softmax over the
concatenated keys of a scene's views.

Reference: tools/gpu_diag.py `attn_ref` with the key set widened -- q rounded after the softmax scale is folded in, k and v as stored,
P rounded to the operand type before P.V, everything else fp64. Bounds: the ones `check_attention` / `check_f16x2` (tools/gpu_diag.py)
hold `md_op_attention` to -- max error relative to the largest output, and the mean error: bf16 8e-3 / 2.5e-3, f16 1e-3 / 4e-4,
f16x2 2e-5 / 3e-6 (planted outliers in f16x2: 5e-4, gpu_diag's "late keys" bound). The per-key arithmetic is the same; the key counts
here (74 .. 258) are below the 577 .. 4096 those bounds were set on.
"""
import functools

import pytest
import torch

from oracle import depth_pro_ref as R

pytestmark = pytest.mark.gpu

BF16, F16, F16X2 = 0, 3, 4
PNAME = {BF16: "bf16", F16: "f16", F16X2: "f16x2"}
ROUND = {BF16: R.bf16_round, F16: R.f16_round, F16X2: R.identity}
TOL_MAX = {BF16: 8e-3, F16: 1e-3, F16X2: 2e-5}
TOL_MEAN = {BF16: 2.5e-3, F16: 4e-4, F16X2: 3e-6}
TOL_OUTLIER = {BF16: 8e-3, F16: 1e-3, F16X2: 5e-4}
# (T sequences, V views, N tokens, heads)
SHAPES = [(4, 2, 70, 2),    # last tile holds 6 valid keys per view
          (6, 3, 64, 2),    # exact tile
          (2, 2, 129, 6),   # three tiles, one key in the last
          (3, 3, 37, 2)]    # less than a tile
PRECS = [BF16, F16, F16X2]


@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape and bool(torch.isfinite(a).all())
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def mean_rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().mean() / (b.abs().mean() + 1e-12)).item()


def attn_views_ref(qkv, V, heads, quant):
    """fp64: the queries of sequence g*V + i against the keys of sequences g*V .. g*V + V-1 in that order, one softmax."""
    T, N, _ = qkv.shape
    G = T // V
    q, k, v = qkv.reshape(T, N, 3, heads, 64).permute(2, 0, 3, 1, 4)  # [T, heads, N, 64]
    q, k, v = R.round_q_prescaled(q, quant).double(), quant(k).double(), quant(v).double()
    cat = lambda t: t.reshape(G, V, heads, N, 64).permute(0, 2, 1, 3, 4).reshape(G, 1, heads, V * N, 64).expand(G, V, heads, V * N, 64).reshape(T, heads, V * N, 64)
    k, v = cat(k), cat(v)
    s = (q @ k.transpose(-2, -1)) * 0.125
    pu = torch.exp(s - s.amax(-1, keepdim=True))
    o = (quant(pu.float()).double() @ v) / pu.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(T, N, heads * 64).float()


@functools.lru_cache(maxsize=None)
def inputs(shape):
    T, V, N, heads = shape
    g = torch.Generator().manual_seed(1000 + 7 * T + 3 * V + N + heads)
    qkv = torch.randn(T, N, 3 * heads * 64, generator=g)
    qkv[..., :heads * 64] *= 2.0
    return qkv


@functools.lru_cache(maxsize=None)
def reference(shape, prec):
    return attn_views_ref(inputs(shape), shape[1], shape[3], ROUND[prec])


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_V%d_N%d_h%d" % s)
def test_attention_views_against_fp64(dev, shape, prec):
    from burn_depth_amd import ops
    T, V, N, heads = shape
    got = ops.attention_views(dev, inputs(shape).cuda(), V, heads, prec)
    want = reference(shape, prec)
    e_max, e_mean = rel_err(got, want), mean_rel(got, want)
    print(f"attention_views {PNAME[prec]} {shape}: max {e_max:.3e} (bound {TOL_MAX[prec]:.1e}) mean {e_mean:.3e} (bound {TOL_MEAN[prec]:.1e})")
    assert e_max <= TOL_MAX[prec]
    assert e_mean <= TOL_MEAN[prec]
    # a view that ignored the other views' keys would be the single-view result: far outside the bound
    from_one_view = ops.attention(dev, inputs(shape).cuda(), heads, prec)
    assert rel_err(from_one_view, want) > 10 * TOL_MAX[prec]


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_V%d_N%d_h%d" % s)
def test_poisoned_padding_changes_no_bit(dev, shape, prec):
    """The rows between N and the sequence stride, the slack rows and the V^T columns past N hold a large finite value (8192 as a half,
    1.6e29 as bf16): behind a view's last valid key the kernel reads the padding rows and then the NEXT view's rows, and must mask both."""
    from burn_depth_amd import ops
    T, V, N, heads = shape
    x = inputs(shape).cuda()
    clean = ops.attention_views(dev, x, V, heads, prec)
    dirty = ops.attention_views(dev, x, V, heads, prec, poison_pad=True)
    assert bool(torch.isfinite(dirty).all())
    assert torch.equal(clean, dirty)


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("shape", SHAPES + [(2, 1, 577, 2)], ids=lambda s: "T%d_N%d_h%d" % (s[0], s[2], s[3]))
def test_one_view_is_md_op_attention(dev, shape, prec):
    from burn_depth_amd import ops
    T, _, N, heads = shape
    x = inputs(shape).cuda()
    assert torch.equal(ops.attention_views(dev, x, 1, heads, prec), ops.attention(dev, x, heads, prec))


@pytest.mark.parametrize("prec", PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("nat", [60.0, 95.0], ids=["60nat", "95nat"])
def test_outlier_in_the_last_views_second_tile(dev, prec, nat):
    """One query of the scene's FIRST view meets a key in the LAST view's second tile worth `nat` natural logit units, everything else
    being O(1) (the pattern of test_attention_assembly_kernel_on_heavy_tailed_logits). 60 nat = 87 log2 units: inside the bf16 fast
    body's range (p = 2^87 in fp32), beyond what an f16 P holds; 95 nat = 137 log2 units overflows the fp32 row sum. Whatever the first
    tile's range check saw, the row sums show it and the workgroup runs again in the running-maximum body."""
    from burn_depth_amd import ops
    T, V, N, heads = 4, 2, 129, 2
    D = heads * 64
    qkv = inputs((T, V, N, heads)).clone()
    seq_q, seq_k, qi, ki, h = 2, 3, 11, 64 + 5, 1
    qrow = qkv[seq_q, qi, h * 64:(h + 1) * 64]
    qkv[seq_k, ki, D + h * 64:D + (h + 1) * 64] = qrow * (8.0 * nat / float(qrow.square().sum()))
    want = attn_views_ref(qkv, V, heads, ROUND[prec])
    got = ops.attention_views(dev, qkv.cuda(), V, heads, prec)
    assert bool(torch.isfinite(got).all())
    row_g, row_w = got[seq_q, qi, h * 64:(h + 1) * 64], want[seq_q, qi, h * 64:(h + 1) * 64]
    print(f"attention_views outlier {PNAME[prec]} {nat} nat: all {rel_err(got, want):.3e} row {rel_err(row_g, row_w):.3e} (bound {TOL_OUTLIER[prec]:.1e})")
    assert rel_err(got, want) <= TOL_OUTLIER[prec]
    assert rel_err(row_g, row_w) <= TOL_OUTLIER[prec]  # the planted row: essentially that key's v
    # the other scene never sees the planted key
    plain = ops.attention_views(dev, inputs((T, V, N, heads)).cuda(), V, heads, prec)
    assert torch.equal(got[:2], plain[:2])


def test_shape_and_mode_errors(dev):
    from burn_depth_amd import _lib, ops
    x = torch.randn(3, 40, 3 * 64, device="cuda")
    with pytest.raises(_lib.MdError) as e:
        ops.attention_views(dev, x, 2, 1, BF16)   # 3 sequences in groups of 2
    assert e.value.code == _lib.MD_ERR_SHAPE
    with pytest.raises(_lib.MdError) as e:
        ops.attention_views(dev, x, 3, 1, 1)      # the fp32 mode attends through its own three-launch path
    assert e.value.code == _lib.MD_ERR_UNSUPPORTED
