"""Operator tests of the kernels that WRITE the MFMA operands both models share: the typed LayerNorm in the forms the engines launch
(bf16 / f16 / split-half / e4m3 / fp32 rows, two to four sequence groups, the token-0 replacement with write-back, more rows than
waves), the row and layout converters, the two e4m3 packers, the LayerNorm-fold kernels and the typed direct convolution. Every other
test of the suite rounds its operands in Python and assumes the device stores exactly those values; these tests check the stores.
References are plain torch fp64 (or torch's own casts, for the bit-exact part), written from each operation's definition.

Where the tolerances come from (none is taken from a GPU result):

* Pure conversions (`store_rows`, `load_rows`, `nchw_to_nhwc`, `nhwc_to_nchw`, `f32_to_fp8`, `pack_fp8_rows`): tolerance 0, the stored
  bytes against torch's casts: bf16 `.bfloat16()`; f16 `clamp(+-65504).half()`; split-half hi = that half, lo = half(clamp(v - float(hi))),
  rows [hi: width | lo: width]; e4m3 `(x * inv).clamp(+-448).to(float8_e4m3fn)` with the fp32 multiply first; `pack_fp8_rows`
  scale = amax * fp32(1/448) (1 for an all-zero row), inv = 1 / scale in fp32, columns K .. Kp zero. The input block carries, in every
  lane slot of a 4-vector, exact ties of each type in both parities, f16 subnormals and values below 2^-25, +-65504 and just above,
  +-inf, +-0, values whose lo plane is subnormal, 448 / 449 / 464 and the smallest e4m3 subnormal and half of it; no NaN. -0 is left
  out of the relu = 1 layout cases only (max(-0, 0) has no defined sign). `f32_to_fp8` converts four values per thread, so its
  second grid-stride pass needs 4 * 2^19 + 48 values (8 MB), the largest buffer of this file.
* LayerNorm, per element against fp64 with `close_check.assert_close_in`: 0.5 ulp_T (1 + tie slack) + A_LN max|ref|, A_LN = 2e-6 (what
  tools/gpu_diag.py check_layernorm uses), tie-slack users under 1 %. e4m3: the reference is scaled by fp8_inv_scale and clamped to
  +-448. Inputs are of check_layernorm's class (randn * 3 + 0.5); the fp32 two-pass evaluation of that class is 1.6e-7 max|ref| from
  fp64 on the CPU. The large-mean class (mean 30, std 1) gains one derived term. The kernel forms mean = fp32(sum / D) and normalises
  c_j = x_j - mean (exact here: x and the mean are multiples of 2^-19 below 32, the difference is below 8, so it has at most 22 bits).
  An error dm in the mean moves every c_j by -dm, moves the variance only in second order (sum c_j = 0), and therefore moves the
  output y_j = c_j rstd gamma_j + beta_j by |dm| rstd |gamma_j|. One fp32 rounding of the mean is up to one ulp of it:
  ulp_fp32(m) <= 2^-23 |m| (half an ulp from the last addition of the sum, half from the division). The term is therefore
  2^-23 |mean| rstd |gamma_j| per element (times fp8_inv_scale for e4m3), with mean and rstd of the fp64 reference. The roundings of the
  earlier, smaller partial sums are left to A_LN. The CPU test confirms that the fp32 evaluation passes with it.
* `ln_fold_vectors`: the kernel sums in fp64, so only the final fp32 rounding shows: 0.5 ulp_fp32(|ref|) + 1e-12 max|ref| (the fp64
  summation order) against c[n] = sum_k gamma[k] Wr[n][k], d[n] = bias[n] + sum_k beta[k] Wr[n][k], Wr = the weight as the operand holds it.
* `ln_finish`: 4 fp32 ulp on rstd and on -mu rstd against the fp64 Chan combination of the same fp32 parts. Roundings on the way to rstd,
  each at most half an ulp = 2^-24 relative: two additions deep in the sum of the four M2, one for adding the between-tile term, halved by
  the square root (1.5), the product with inv_n and the addition of eps, halved (1), the square root (1), the division (1): 4.5 * 2^-24
  relative when every one of them is at its worst and of the same sign, which is between 2.25 and 4.5 ulp of the result; -mu rstd adds
  the three additions of mu and one product. The check is the 4 ulp the kernel's header states; tile means of this input class carry
  little of M2 (under 1 %), so the roundings inside the between-tile term do not count.
* `conv_direct`: fp32 products and sums of exactly representable inputs: the suite's A_MFMA = 2e-5 max|ref| (accumulation order).

CPU tests (no device): for every checked kernel the reference formula is evaluated in fp32, rounded as the type rounds, and accepted;
then each mutant is rejected on every case where it is not the identity (`MUTANT_ACTIVE` says where): unbiased variance; gamma / beta of
the neighbouring group; the previous row's sequence index (the stale prefetch hand-over); token 0 written back but the old row
normalised; truncation for round-to-nearest-even; lo = half(v) - hi for half(v - hi); an f16 cast that does not saturate; an e4m3 cast
without the clamp; the fp8 scale applied after the rounding; `pack_fp8_rows` with inv = 448 / amax; `ln_finish` without the between-tile
term; `ln_fold_vectors` with the unrounded W. What the per-element LayerNorm check can NOT reject at these shapes, and where it is
caught instead: truncation in the split-half mode (one 22-bit ulp, 4.8e-7 at 1, is below A_LN max|ref| = 2e-5: the bit-exact converter
tests catch a truncating split). `pack_fp8_rows` with inv = 448 / amax differs from the kernel's inv by one fp32 rounding and flips a
byte only next to an e4m3 tie, so `pack_input` plants such values (`pack_tie_values`); seeded rows alone would not tell the two apart.
"""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import close_check
from close_check import A_LN, A_MFMA, BF16, F16, F16X2, F32, FP8, PNAME, ROUND, rejects

assert_close_in = functools.partial(close_check.assert_close_in, tag="operand_writers")
STORE_PRECS = [BF16, F16, F32, F16X2]
FP8_INV = 448.0 / 8.0   # the engine's static LayerNorm-output scale


# ---------------------------------------------------------------------------------------------
# expected bits of the pure conversions (torch's casts)
# ---------------------------------------------------------------------------------------------
def sat_half(v):
    return v.clamp(-65504.0, 65504.0).half()


def expect_store(x, prec, width, mut=None):
    """The stored rows of fp32 x [rows, width]: bf16 / f16 / f32 [rows, width], split-half f16 [rows, 2 * width] = hi | lo."""
    x = x.float().contiguous()
    half = (lambda v: v.half()) if mut == "f16_no_saturation" else sat_half
    if mut == "truncate":
        half = lambda v: trunc_half(v.clamp(-65504.0, 65504.0))  # noqa: E731
    if prec == F32:
        return x.clone()
    if prec == BF16:
        return trunc_bf16(x) if mut == "truncate" else x.bfloat16()
    hi = half(x)
    if prec == F16:
        return hi
    lo = (half(x) - hi) if mut == "lo_of_rounded" else half(x - hi.float())
    return torch.cat([hi, lo], -1)


def expect_load(raw, prec, width):
    if prec == F16X2:
        return raw[..., :width].float() + raw[..., width:].float()
    return raw.float()


def trunc_bf16(x):
    return (x.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def trunc_half(x):
    """fp32 -> f16 rounding toward zero (finite inputs within +-65504)."""
    h = x.half()
    over = h.float().abs() > x.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)  # sign-magnitude: one step toward zero


def expect_fp8(x, inv, mut=None):
    """e4m3 bytes (uint8) of fp32 x on the scale 1 / inv."""
    x = x.float()
    if mut == "scale_after_rounding":
        v = x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * torch.tensor(inv, dtype=torch.float32)
        return v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    v = x * torch.tensor(inv, dtype=torch.float32)
    if mut != "no_clamp":
        v = v.clamp(-448.0, 448.0)
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def expect_pack_fp8(w, Kp, mut=None):
    w = w.float()
    N, K = w.shape
    amax = w.abs().amax(1)
    scale = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    inv = torch.tensor(448.0, dtype=torch.float32) / amax.clamp_min(1e-30) if mut == "inv_direct" else 1.0 / scale
    inv = torch.where(amax > 0, inv, torch.ones_like(inv))
    out = torch.zeros(N, Kp, dtype=torch.uint8)
    out[:, :K] = (w * inv[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return out, scale


P2 = lambda e: 2.0 ** e  # noqa: E731
EDGES = [
    1 + P2(-8), 1 + 3 * P2(-8), -(1 + P2(-8)), -(1 + 3 * P2(-8)),                    # bf16 ties, even and odd neighbour below
    1 + P2(-11), 1 + 3 * P2(-11), -(1 + P2(-11)), -(1 + 3 * P2(-11)),                # f16 ties
    1 + P2(-12) + P2(-23), 1 + P2(-12) + 3 * P2(-23), -(1 + P2(-12) + P2(-23)),      # ties of the lo plane (hi = 1)
    1 + P2(-4), 1 + 3 * P2(-4), -(1 + P2(-4)), -(1 + 3 * P2(-4)),                    # e4m3 ties
    P2(-24), 3 * P2(-24), 1.5 * P2(-24), 2.5 * P2(-24), -1.5 * P2(-24),              # f16 subnormals and their ties
    P2(-25), P2(-25) * (1 + P2(-10)), -P2(-25), P2(-26), P2(-30), -P2(-40),          # the tie to zero, just above, below 2^-25
    65504.0, -65504.0, 65504.0 * (1 + P2(-20)), 65520.0, -65520.0, 65536.0, 1e5, -1e5, 3e38, -3e38,
    float("inf"), float("-inf"), 0.0, -0.0,
    0.1, -0.1, 0.01, 0.003, P2(-3) - P2(-20), P2(-14) + P2(-30),                     # lo plane subnormal (|v| < 2^-3)
    448.0, 449.0, 464.0, 465.0, 480.0, -448.0, -449.0, -464.0, 432.0, 440.0,         # the e4m3 clamp, the last tie before it
    P2(-9), P2(-10), -P2(-9), -P2(-10), 1.5 * P2(-9), 2.5 * P2(-9), 3 * P2(-10), P2(-11),  # e4m3 subnormals, half of the smallest
]
while len(EDGES) % 4 != 1:  # position of the i-th placed value is 5 i + 3, its lane slot (i + 3) % 4: four passes over a list of
    EDGES.append(1.0)       # length = 1 mod 4 put every value into every slot


@functools.lru_cache(maxsize=None)
def conversion_block(count, seed=5):
    """fp32 [count]: seeded values over the ranges of the types, the edge values at positions 5 i + 3 (four passes: every slot)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(count, generator=g) * torch.tensor([1e-3, 0.05, 1.0, 30.0, 600.0])[torch.randint(0, 5, (count,), generator=g)]
    e = torch.tensor(EDGES * 4, dtype=torch.float32)
    pos = 5 * torch.arange(e.numel()) + 3
    assert pos[-1] < count
    x[pos] = e
    return x


def edge_slots():
    """edge value index -> the set of 4-vector lane slots it lands in."""
    n = len(EDGES)
    return [{(5 * (i + r * n) + 3) % 4 for r in range(4)} for i in range(n)]


SMALL_COUNT = 5 * 4 * len(EDGES) + 20  # a few hundred elements (a multiple of 20: split-half width 20)
BIG_COUNT = 2 ** 19 + 12               # above 256 * 2048 threads: the grid-stride loop takes a second pass (width 100 divides it)
FP8_BIG_COUNT = 4 * 2 ** 19 + 48       # the same for the four-values-per-thread e4m3 converter
CONV_SIZES = [(SMALL_COUNT, 20), (BIG_COUNT, 100)]
FP8_INVS = [1.0, 0.25, FP8_INV]
PACK_CASES = [(5, 100, 128), (64, 70, 72), (8200, 12, 16)]  # N, K, Kp; the last: more rows than the 8192 waves of a capped grid


def pack_invs(amax):
    """(the kernel's inv = 1 / (amax * fp32(1/448)), the mutant's 448 / amax), both fp32."""
    return 1.0 / (amax * torch.tensor(1.0 / 448.0, dtype=torch.float32)), torch.tensor(448.0, dtype=torch.float32) / amax


def pack_tie_values(amax):
    """Weights below amax whose product with the kernel's inv and with 448 / amax fall on different sides of an e4m3 tie (the two
    reciprocals are one fp32 rounding apart on most rows); empty where the two agree."""
    inv1, inv2 = pack_invs(amax)
    if inv1 == inv2:
        return torch.zeros(0)
    ties = torch.tensor([(1 + (2 * m + 1) / 16) * 2.0 ** k for k in range(-5, 8) for m in range(8)], dtype=torch.float32)
    base = (ties / inv1).view(torch.int32)
    cand = torch.cat([(base + o).view(torch.float32) for o in range(-3, 4)])
    cand = cand[cand.abs() < amax]
    q = lambda inv: (cand * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)  # noqa: E731
    return cand[q(inv1) != q(inv2)]


@functools.lru_cache(maxsize=None)
def pack_input(N, K):
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) * torch.rand(N, 1, generator=g) * 3
    w[1] = 0.0                                # an all-zero row: scale 1
    w[2, : min(K, 8)] = torch.tensor([448.0, -449.0, 464.0, 1 + P2(-4), P2(-9), P2(-10), -0.0, 1e-30])[: min(K, 8)]
    for n in range(3, min(N, 40)):            # values that tell inv = 1 / scale from inv = 448 / amax
        kmax = int(w[n].abs().argmax())
        while pack_tie_values(w[n, kmax].abs()).numel() == 0:   # the two reciprocals agree for this amax: take the next one up
            w[n, kmax] = torch.nextafter(w[n, kmax], w[n, kmax] * 2)
        amax = w[n].abs().amax()
        t = pack_tie_values(amax)[:4]
        free = [k for k in range(K) if w[n, k].abs() != amax][: t.numel()]
        w[n, free] = t
    return w


def test_conversion_block_covers_every_lane_slot():
    assert SMALL_COUNT % 20 == 0 and BIG_COUNT % 100 == 0 and BIG_COUNT > 256 * 2048 and FP8_BIG_COUNT // 4 > 256 * 2048
    assert all(s == {0, 1, 2, 3} for s in edge_slots())
    x = conversion_block(SMALL_COUNT)
    assert not torch.isnan(x).any() and torch.isinf(x).sum() == 8
    for prec in STORE_PRECS:  # the casts themselves never produce a NaN from this block
        assert not torch.isnan(expect_load(expect_store(x.reshape(-1, 20), prec, 20), prec, 20)).any()


def test_conversion_mutants_change_the_expected_bits():
    """The bit-exact tests compare with `expect_*`; a device that did what a mutant does would differ on this input block."""
    x = conversion_block(SMALL_COUNT).reshape(-1, 20)
    differs = lambda a, b: not torch.equal(a.view(torch.int16) if a.dtype != torch.float32 else a, b.view(torch.int16) if b.dtype != torch.float32 else b)  # noqa: E731
    for prec in (BF16, F16, F16X2):
        assert differs(expect_store(x, prec, 20, "truncate"), expect_store(x, prec, 20))
    for prec in (F16, F16X2):
        assert differs(expect_store(x, prec, 20, "f16_no_saturation"), expect_store(x, prec, 20))
    assert differs(expect_store(x, F16X2, 20, "lo_of_rounded"), expect_store(x, F16X2, 20))
    assert not differs(expect_store(x, F16X2, 20, "lo_of_rounded")[:, :20], expect_store(x, F16X2, 20)[:, :20])  # hi plane: identity
    flat = x.reshape(-1)
    for inv in FP8_INVS:
        for mut in ("no_clamp", "scale_after_rounding"):
            identity = mut == "scale_after_rounding" and inv == 1.0
            assert torch.equal(expect_fp8(flat, inv, mut), expect_fp8(flat, inv)) == identity, (mut, inv)
        nan = expect_fp8(flat, inv, "no_clamp") & 0x7f == 0x7f
        assert nan.any() and not (expect_fp8(flat, inv) & 0x7f == 0x7f).any()
    for N, K, Kp in PACK_CASES:
        (b0, s0), (b1, s1) = expect_pack_fp8(pack_input(N, K), Kp), expect_pack_fp8(pack_input(N, K), Kp, "inv_direct")
        assert torch.equal(s0, s1) and not torch.equal(b0, b1), (N, K)   # `pack_input` plants values that tell the two reciprocals apart
        assert (b0[:, K:] == 0).all() and s0[1] == 1.0 and (b0[1] == 0).all()


# ---------------------------------------------------------------------------------------------
# LayerNorm: cases, reference, mutants
# ---------------------------------------------------------------------------------------------
LN_KINDS = [(BF16, 0), (F16, 0), (F32, 0), (F16X2, 0), (FP8, 0), (BF16, 1)]  # (precision, out_f32)
LN_KIND_ID = lambda k: PNAME[k[0]] + ("_outf32" if k[1] else "")  # noqa: E731
LN_DS = [64, 260, 384, 512, 772, 1024]   # NV = 1, 2 (one lane of the second vector), 2, 2, 4 (one lane of the fourth), 4
LN_SS = [1, 5, 37]
LN_T = 7
GROUP_KINDS = ["one", "three", "mixed"]
LN_EPS = 1e-6


def out_prec(kind):
    return F32 if kind[1] else kind[0]


@functools.lru_cache(maxsize=None)
def ln_params(D, gkind, seed=0):
    """[(seq0, nseq, gamma, beta)] over LN_T = 7 sequences; the groups' gammas / betas lie clearly apart."""
    g = torch.Generator().manual_seed(100 + D + seed)
    ga = lambda s: (torch.rand(D, generator=g) + 0.5) * s          # noqa: E731
    be = lambda o: torch.randn(D, generator=g) * 0.1 + o           # noqa: E731
    if gkind == "one":
        return [(0, LN_T, ga(1.0), be(0.0))]
    if gkind == "three":
        return [(0, 1, ga(1.0), be(0.0)), (1, 4, ga(2.0), be(1.0)), (5, 2, ga(0.5), be(-1.0))]
    return [(0, 3, None, None), (3, 4, ga(1.5), be(0.5))]          # a non-affine group beside an affine one


@functools.lru_cache(maxsize=None)
def ln_input(rows, D, cls="plain", seed=0):
    g = torch.Generator().manual_seed(7 + rows + D + seed)
    if cls == "plain":
        return torch.randn(rows, D, generator=g) * 3 + 0.5
    return torch.randn(rows, D, generator=g) + 30.0                # the large-mean class


def ln_row_params(rows, D, S, groups, dtype, mut=None):
    """gamma, beta per row [rows, D] (ones / zeros where non-affine)."""
    seq = torch.arange(rows) // S
    if mut == "stale_seq":
        seq = (torch.arange(rows) - 1).clamp_min(0) // S
    gi = torch.zeros(rows, dtype=torch.long)
    for i, (s0, _, _, _) in enumerate(groups):
        gi[seq >= s0] = i
    if mut == "neighbour_group":
        gi = (gi + 1) % len(groups)
    G = torch.stack([torch.ones(D) if g[2] is None else g[2] for g in groups]).to(dtype)[gi]
    Bt = torch.stack([torch.zeros(D) if g[3] is None else g[3] for g in groups]).to(dtype)[gi]
    return G, Bt


def ln_eval(x, S, groups, eps=LN_EPS, dtype=torch.float64, tok0=None, stride=0, mut=None, scale=1.0):
    """(y [rows, D], x after the token-0 write-back, the bound's large-mean term per element)."""
    rows, D = x.shape
    xw = x.clone()
    if tok0 is not None:
        nseq = (rows + S - 1) // S
        xw[torch.arange(nseq) * S] = torch.stack([tok0.reshape(-1)[s * stride: s * stride + D] for s in range(nseq)])
    xin = (x if mut == "tok0_old_row" else xw).to(dtype)
    G, Bt = ln_row_params(rows, D, S, groups, dtype, mut)
    mean = xin.mean(-1, keepdim=True)
    c = xin - mean
    var = (c * c).sum(-1, keepdim=True) / ((D - 1) if mut == "unbiased" else D)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = c * rstd * G + Bt
    mean_term = 2.0 ** -23 * mean.abs() * rstd * G.abs() * scale
    return y * scale, xw, mean_term


def ln_store(y32, kind, mut=None):
    """fp32 values -> what the output rows hold, widened back (e4m3: on the scaled, clamped axis)."""
    prec = out_prec(kind)
    if prec == FP8:
        if mut == "truncate":
            v = y32.clamp(-448.0, 448.0)
            r = v.to(torch.float8_e4m3fn)
            over = r.float().abs() > v.abs()
            return torch.where(over, (r.view(torch.uint8) - 1).view(torch.float8_e4m3fn).float(), r.float())
        if mut == "no_clamp":
            return y32.to(torch.float8_e4m3fn).float()
        return ROUND[FP8](y32)
    if prec == F32:
        return y32
    w = y32.shape[-1]
    return expect_load(expect_store(y32, prec, w, mut), prec, w)


def ln_scale(kind):
    return FP8_INV if out_prec(kind) == FP8 else 1.0


def ln_ref(x, S, groups, kind, **kw):
    y, xw, mt = ln_eval(x, S, groups, scale=ln_scale(kind), **kw)
    return (y.clamp(-448.0, 448.0) if out_prec(kind) == FP8 else y), xw, mt


def ln_fp32(x, S, groups, kind, mut=None, **kw):
    """The formula in fp32 arithmetic, stored as the type stores."""
    emut = mut if mut in ("unbiased", "neighbour_group", "stale_seq", "tok0_old_row") else None
    y, _, _ = ln_eval(x, S, groups, dtype=torch.float32, mut=emut, **kw)
    if out_prec(kind) == FP8:
        if mut == "scale_after_rounding":
            return ROUND[FP8](y) * FP8_INV
        y = y * torch.tensor(FP8_INV, dtype=torch.float32)
    return ln_store(y, kind, mut if mut in ("truncate", "lo_of_rounded", "no_clamp") else None)


def ln_case_rows(S):
    return LN_T * S


LN_MUTANTS = ["unbiased", "neighbour_group", "stale_seq", "tok0_old_row", "truncate", "lo_of_rounded", "scale_after_rounding"]


def MUTANT_ACTIVE(mut, kind, gkind, S, with_tok0):
    """Is the mutant something other than the identity on this case (and within the per-element check's reach)?"""
    prec = out_prec(kind)
    if mut == "neighbour_group":
        return gkind != "one"
    if mut == "stale_seq":       # only the first row of a group reads another group's parameters
        return gkind != "one"
    if mut == "tok0_old_row":
        return with_tok0
    if mut == "truncate":        # split-half: one 22-bit ulp is below A_LN max|ref| (module docstring)
        return prec not in (F32, F16X2)
    if mut == "lo_of_rounded":
        return prec == F16X2
    if mut == "scale_after_rounding":
        return prec == FP8
    return True


@pytest.mark.parametrize("kind", LN_KINDS, ids=LN_KIND_ID)
@pytest.mark.parametrize("D", [64, 384, 772, 1024])
def test_layernorm_checker_accepts_fp32_and_rejects_mutants(D, kind):
    prec = out_prec(kind)
    for S in (5, 37):
        for gkind in GROUP_KINDS:
            for with_tok0 in (False, True):
                groups = ln_params(D, gkind)
                x = ln_input(ln_case_rows(S), D)
                tok0 = ln_input(LN_T, D, seed=9) * 0.7 - 1.0 if with_tok0 else None
                kw = dict(tok0=tok0, stride=D)
                ref, xw, _ = ln_ref(x, S, groups, kind, **kw)
                what = f"fp32 evaluation D={D} S={S} {gkind} tok0={with_tok0}"
                assert_close_in(ln_fp32(x, S, groups, kind, **kw), ref, prec, A_LN, what=what)
                for mut in LN_MUTANTS:
                    got = ln_fp32(x, S, groups, kind, mut=mut, **kw)
                    assert rejects(got, ref, prec, A_LN) == MUTANT_ACTIVE(mut, kind, gkind, S, with_tok0), (mut, what)


@pytest.mark.parametrize("kind", LN_KINDS, ids=LN_KIND_ID)
@pytest.mark.parametrize("D", [64, 772, 1024])
def test_layernorm_large_mean_term_holds_for_the_fp32_evaluation(D, kind):
    """Mean 30, std 1: the fp32 evaluation passes with the derived term 2^-23 |mean| rstd |gamma_j| (module docstring), and the term
    does not hide the mutants."""
    prec, S = out_prec(kind), 5
    groups = ln_params(D, "three")
    x = ln_input(ln_case_rows(S), D, cls="large_mean")
    ref, _, mt = ln_ref(x, S, groups, kind)
    assert_close_in(ln_fp32(x, S, groups, kind), ref, prec, A_LN, extra=mt, what=f"fp32 evaluation, large mean, D={D}")
    for mut in ("unbiased", "neighbour_group", "stale_seq"):
        assert rejects(ln_fp32(x, S, groups, kind, mut=mut), ref, prec, A_LN, extra=mt), mut


def ln_saturating(D=512, S=5):
    """gamma = 8 / 2.576: about 1 % of a unit normal lies beyond 2.576, so about 1 % of the outputs exceed 8 = 448 / fp8_inv_scale."""
    return ln_input(ln_case_rows(S), D, seed=3), [(0, LN_T, torch.full((D,), 8.0 / 2.576), torch.zeros(D))], S


def test_fp8_saturation_case_and_the_unclamped_cast():
    x, groups, S = ln_saturating()
    ref, _, _ = ln_eval(x, S, groups, scale=FP8_INV)
    over = ref.abs() > 448.0
    assert 0.005 < over.double().mean().item() < 0.02
    kind = (FP8, 0)
    good = ln_fp32(x, S, groups, kind)
    assert torch.isfinite(good).all() and (good[over].abs() == 448.0).all()
    assert_close_in(good, ref.clamp(-448.0, 448.0), FP8, A_LN, what="fp32 evaluation, saturating e4m3")
    assert torch.isnan(ln_fp32(x, S, groups, kind, mut="no_clamp")).any()   # the mutant stores NaN bytes: assert_close_in's first line


# ---------------------------------------------------------------------------------------------
# fold kernels: references and mutants
# ---------------------------------------------------------------------------------------------
FOLD_CASES = [(5, 64), (130, 1024), (7, 100)]


@functools.lru_cache(maxsize=None)
def fold_inputs(N, K):
    g = torch.Generator().manual_seed(N * 3 + K)
    return (torch.randn(N, K, generator=g) / K ** 0.5, torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2,
            torch.randn(N, generator=g) * 0.3)


def fold_eval(W, gamma, beta, bias, prec, rounded=True, order=None):
    """fp64 (c, d); `order`: a permutation of k (another summation order)."""
    Wr = (ROUND[prec](W) if rounded else W).double()
    tc, td = gamma.double() * Wr, beta.double() * Wr
    if order is not None:
        tc, td = tc[:, order], td[:, order]
        c, d = torch.zeros(W.shape[0], dtype=torch.float64), torch.zeros(W.shape[0], dtype=torch.float64)
        for k in range(tc.shape[1]):
            c, d = c + tc[:, k], d + td[:, k]
    else:
        c, d = tc.sum(1), td.sum(1)
    return c, d + (bias.double() if bias is not None else 0.0)


def ulp_f32(a):
    _, ex = torch.frexp(a.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a, dtype=torch.float64), ex - 24)


def fold_bad(got, ref):
    """Elements outside 0.5 ulp_fp32(|ref|) + 1e-12 max|ref|."""
    return int(((got.double() - ref).abs() > 0.5 * ulp_f32(ref) + 1e-12 * ref.abs().max()).sum())


@pytest.mark.parametrize("N,K", FOLD_CASES)
def test_fold_vectors_checker(N, K):
    W, gamma, beta, bias = fold_inputs(N, K)
    order = torch.randperm(K, generator=torch.Generator().manual_seed(1))
    for prec in STORE_PRECS:
        for b in (bias, None):
            ref = fold_eval(W, gamma, beta, b, prec)
            got = fold_eval(W, gamma, beta, b, prec, order=order)
            assert fold_bad(got[0].float(), ref[0]) == 0 and fold_bad(got[1].float(), ref[1]) == 0
            mut = fold_eval(W, gamma, beta, b, prec, rounded=False)
            caught = fold_bad(mut[0].float(), ref[0]) + fold_bad(mut[1].float(), ref[1]) > 0
            assert caught == (prec != F32), (PNAME[prec], b is None)   # f32 operands hold W unrounded: the identity


FINISH_ROWS = [1, 255, 257, 1000]
FINISH_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def finish_parts():
    """parts [1000, 4, 2] fp32 = (mean, centred sum of squares) of the four 256-column tiles of real rows, computed in fp64.
    Row 1: four equal tiles (equal tile means); row 2: every tile constant (M2 = 0, the between-tile term is everything)."""
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(1000, 4, 256, generator=g) * 3 + 0.5).double()
    x[1] = x[1, 0]
    x[2] = torch.tensor([1.0, 2.0, 3.0, 4.5], dtype=torch.float64)[:, None]
    mean = x.mean(-1)
    m2 = ((x - mean[..., None]) ** 2).sum(-1)
    parts = torch.stack([mean, m2], -1).float()
    assert torch.equal(parts[1, :, 0], parts[1, :1, 0].expand(4)) and (parts[2, :, 1] == 0).all()
    return parts


def finish_eval(parts, dtype=torch.float64, mut=None):
    """Chan: mu = mean of the tile means, M2 = sum M2_t + 256 sum (mean_t - mu)^2; ab = (rstd, -mu rstd), n = 1024."""
    p = parts.to(dtype)
    mu = p[:, :, 0].sum(1) * 0.25
    m2 = p[:, :, 1].sum(1)
    if mut != "no_between_term":
        m2 = m2 + 256.0 * ((p[:, :, 0] - mu[:, None]) ** 2).sum(1)
    rstd = 1.0 / torch.sqrt(m2 * torch.tensor(1.0 / 1024.0, dtype=torch.float32).to(dtype) + FINISH_EPS)
    return torch.stack([rstd, -mu * rstd], 1)


def finish_bad(got, ref):
    """Rows with rstd or -mu rstd more than 4 fp32 ulp from the reference."""
    return ((got.double() - ref).abs() > 4 * ulp_f32(ref)).any(1)


def test_ln_finish_checker():
    parts = finish_parts()
    ref = finish_eval(parts)
    assert not finish_bad(finish_eval(parts, torch.float32), ref).any()
    bad = finish_bad(finish_eval(parts, torch.float32, "no_between_term"), ref)
    assert not bad[1] and bad[2] and bad[0] and bad.double().mean() > 0.99   # identity on the equal-means row only
    for rows in FINISH_ROWS:
        assert finish_bad(finish_eval(parts[:rows], torch.float32, "no_between_term"), ref[:rows]).any()


# ---------------------------------------------------------------------------------------------
# conv_direct: cases and reference
# ---------------------------------------------------------------------------------------------
CONV_CASES = [(1, 8, 6, 6, 1, 6, 1, 0), (2, 16, 9, 7, 8, 3, 2, 1), (1, 6, 5, 5, 3, 3, 1, 1)]  # B, Cin, H, W, Cout, k, stride, pad


@functools.lru_cache(maxsize=None)
def conv_inputs(case, prec):
    B, Cin, H, W, Cout, k, stride, pad = case
    g = torch.Generator().manual_seed(sum(case) + prec)
    x = ROUND[prec](torch.randn(B, Cin, H, W, generator=g))       # exact in the input type
    return (x, torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5, torch.randn(Cout, generator=g) * 0.3,
            torch.randn(B, H, W, Cin, generator=g) * 0.5)


def conv_eval(case, x, w, bias, add, relu, dtype=torch.float64):
    """NHWC [B, OH, OW, Cout]: conv2d(x + add) + bias, optional relu."""
    _, _, _, _, _, _, stride, pad = case
    xin = x.to(dtype) + (add.to(dtype).permute(0, 3, 1, 2) if add is not None else 0.0)
    y = F.conv2d(xin, w.to(dtype), bias.to(dtype), stride=stride, padding=pad)
    return (y.relu() if relu else y).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_direct_checker_accepts_the_fp32_evaluation(case):
    for prec in STORE_PRECS:
        x, w, bias, add = conv_inputs(case, prec)
        assert torch.equal(ROUND[prec](x), x)
        for a in (None, add):
            for relu in (False, True):
                ref = conv_eval(case, x, w, bias, a, relu)
                assert_close_in(conv_eval(case, x, w, bias, a, relu, torch.float32), ref, F32, A_MFMA, what=f"fp32 evaluation conv {case}")
                if not relu:  # the add left out, or added where there is none
                    assert rejects(conv_eval(case, x, w, bias, None if a is not None else add, relu, torch.float32), ref, F32, A_MFMA)


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
    """With OPERAND_WRITERS_ERRORS=<path> the worst error / bound per (kernel, precision) and the slack-user share are written there."""
    yield
    path = os.environ.get("OPERAND_WRITERS_ERRORS")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("kernel precision | worst error / bound over all elements | largest share of tie-slack users | elements compared\n")
            for (k, p), v in sorted(RECORD.items()):
                if isinstance(v, list):
                    f.write(f"{k:28s} {p:12s} | {v[0]:.3f} | {v[1]:.2e} | {v[2]}\n")
                else:
                    f.write(f"{k:28s} {p:12s} | bit-exact | - | {v}\n")


def bits(t):
    """A view in which torch.equal compares bit patterns (-0 / +0 and the two infinities told apart)."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def assert_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
    ne = bits(got) != bits(want)
    assert not ne.any(), f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at {ne.nonzero()[0].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("count,width", CONV_SIZES)
def test_store_rows_and_load_rows_bit_exact(dev, count, width, prec):
    from burn_depth_amd import ops
    x = conversion_block(count)
    want = expect_store(x.reshape(-1, width), prec, width)
    raw = ops.store_rows(dev, x.cuda(), width, prec)
    assert_bits(raw, want, f"store_rows {PNAME[prec]} {count}")
    back = ops.load_rows(dev, want.cuda(), count, width, prec)
    assert_bits(back, expect_load(want, prec, width).reshape(-1), f"load_rows {PNAME[prec]} {count}")
    record_exact("store_rows", PNAME[prec], count)
    record_exact("load_rows", PNAME[prec], count)


@pytest.mark.gpu
def test_store_rows_argument_checks(dev):
    from burn_depth_amd import _lib, ops
    x = conversion_block(SMALL_COUNT).cuda()
    for width in (0, 7):  # split-half needs the width, and rows of it
        with pytest.raises(_lib.MdError) as e:
            ops.store_rows(dev, x, width, F16X2)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
    with pytest.raises(_lib.MdError) as e:
        ops.store_rows(dev, x, 20, FP8)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    with pytest.raises(_lib.MdError) as e:
        ops.f32_to_fp8(dev, x[:6], 1.0)
    assert e.value.code == _lib.MD_ERR_UNSUPPORTED
    with pytest.raises(_lib.MdError) as e:
        ops.pack_fp8_rows(dev, x[:40].reshape(4, 10), 8)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("inv", FP8_INVS)
@pytest.mark.parametrize("count", [SMALL_COUNT, FP8_BIG_COUNT])
def test_f32_to_fp8_bit_exact(dev, count, inv):
    from burn_depth_amd import ops
    x = conversion_block(count)
    got = ops.f32_to_fp8(dev, x.cuda(), inv)
    assert_bits(got, expect_fp8(x, inv), f"f32_to_fp8 inv={inv} {count}")
    record_exact("f32_to_fp8", "fp8", count)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,Kp", PACK_CASES)
def test_pack_fp8_rows_bit_exact(dev, N, K, Kp):
    from burn_depth_amd import ops
    w = pack_input(N, K)
    want, scale = expect_pack_fp8(w, Kp)
    got, gs = ops.pack_fp8_rows(dev, w.cuda(), Kp)
    assert_bits(gs, scale, f"pack_fp8_rows scales {N}x{K}")
    assert_bits(got, want, f"pack_fp8_rows {N}x{K}->{Kp}")
    record_exact("pack_fp8_rows", "fp8", N * Kp)


LAYOUT_CASES = [(1, 8, 3, 5), (2, 20, 4, 3)]


def layout_input(B, C, H, W, relu):
    x = conversion_block(SMALL_COUNT)[torch.randperm(SMALL_COUNT, generator=torch.Generator().manual_seed(C))[: B * C * H * W]].reshape(B, C, H, W).clone()
    if relu:
        x[x == 0] = 0.0   # max(-0, 0): no defined sign
    return x


def prefill(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) % 97 + 3).float() * 0.25).to(dtype).reshape(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("B,C,H,W", LAYOUT_CASES)
def test_nchw_to_nhwc_bit_exact(dev, B, C, H, W, prec):
    """relu and ld > C as the decoder runs it: the padding columns keep their pre-fill, the lo plane sits ld elements behind hi."""
    from burn_depth_amd import ops
    planes = 2 if prec == F16X2 else 1
    for ld in (C, C + 12):
        for relu in (0, 1):
            x = layout_input(B, C, H, W, relu)
            v = (x.clamp_min(0.0) if relu else x).permute(0, 2, 3, 1).reshape(-1, C)
            st = expect_store(v, prec, C)
            want = prefill((B * H * W, planes * ld), st.dtype)
            for p in range(planes):
                want[:, p * ld: p * ld + C] = st[:, p * C: (p + 1) * C]
            got = ops.nchw_to_nhwc(dev, x.cuda(), prec, bool(relu), ld, prefill((B, H, W, planes * ld), st.dtype).cuda())
            assert_bits(got.reshape(B * H * W, planes * ld), want, f"nchw_to_nhwc {PNAME[prec]} ld={ld} relu={relu}")
            record_exact("nchw_to_nhwc", PNAME[prec], B * C * H * W)
    got0 = ops.nchw_to_nhwc(dev, x.cuda(), prec, True, 0, prefill((B, H, W, planes * C), st.dtype).cuda())   # ld = 0 means C
    assert_bits(got0.reshape(B * H * W, planes * C), st, "nchw_to_nhwc ld=0")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("B,C,H,W", LAYOUT_CASES)
def test_nhwc_to_nchw_bit_exact(dev, B, C, H, W, prec):
    from burn_depth_amd import _lib, ops
    for ld in (C, C + 12):
        raw = expect_store(layout_input(B, ld, H, W, 0).permute(0, 2, 3, 1).reshape(-1, ld), prec, ld).reshape(B, H, W, -1)
        val = expect_load(raw, prec, ld)
        for coff in (0, 4):
            got = ops.nhwc_to_nchw(dev, raw.cuda(), C - coff, ld, coff, prec)
            assert_bits(got, val[..., coff:C].permute(0, 3, 1, 2).contiguous(), f"nhwc_to_nchw {PNAME[prec]} ld={ld} coff={coff}")
            record_exact("nhwc_to_nchw", PNAME[prec], B * (C - coff) * H * W)
    with pytest.raises(_lib.MdError) as e:
        ops.nhwc_to_nchw(dev, raw.cuda(), C + 12, ld, 4, prec)   # channels past the pixel
    assert e.value.code == _lib.MD_ERR_INVALID_ARG


def ln_run(dev, x, S, groups, kind, tok0=None, stride=0):
    """-> (the output rows widened on the CPU, the raw rows, x after the call or None)."""
    from burn_depth_amd import ops
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    prec = out_prec(kind)
    raw, xw = ops.layernorm_ex(dev, x.cuda(), S, [(a, b, cu(g), cu(be)) for a, b, g, be in groups], LN_EPS, kind[0], bool(kind[1]),
                               FP8_INV if kind[0] == FP8 else 1.0, cu(tok0), stride)
    raw = raw.cpu()
    D = x.shape[1]
    if prec == FP8:
        assert raw.dtype == torch.uint8 and raw.shape == x.shape
        val = raw.view(torch.float8_e4m3fn).float()
    else:
        assert raw.dtype == {BF16: torch.bfloat16, F16: torch.float16, F16X2: torch.float16, F32: torch.float32}[prec]
        assert raw.shape == (x.shape[0], D * (2 if prec == F16X2 else 1))
        val = expect_load(raw, prec, D)
    return val, raw, (xw.cpu() if xw is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LN_KINDS, ids=LN_KIND_ID)
@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_forms_against_fp64(dev, D, kind):
    """Every output type x NV = 1..4 with a partial last vector x S in {1, 5, 37} x one / three / mixed (non-affine + affine) groups."""
    prec = out_prec(kind)
    for S in LN_SS:
        for gkind in GROUP_KINDS:
            groups = ln_params(D, gkind)
            x = ln_input(ln_case_rows(S), D)
            ref, _, _ = ln_ref(x, S, groups, kind)
            val, _, xw = ln_run(dev, x, S, groups, kind)
            assert xw is None
            record("layernorm", LN_KIND_ID(kind), assert_close_in(val, ref, prec, A_LN, what=f"layernorm D={D} S={S} {gkind}"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LN_KINDS, ids=LN_KIND_ID)
@pytest.mark.parametrize("D", [64, 772, 1024])
def test_layernorm_large_mean_against_fp64(dev, D, kind):
    """Mean 30, std 1: the bound carries the derived term 2^-23 |mean| rstd |gamma_j| (module docstring)."""
    prec, S = out_prec(kind), 5
    groups = ln_params(D, "three")
    x = ln_input(ln_case_rows(S), D, cls="large_mean")
    ref, _, mt = ln_ref(x, S, groups, kind)
    val, _, _ = ln_run(dev, x, S, groups, kind)
    record("layernorm large mean", LN_KIND_ID(kind), assert_close_in(val, ref, prec, A_LN, extra=mt, what=f"layernorm large mean D={D}"))


GS_ROWS, GS_D, GS_S = 16389, 64, 37   # 2 * 8192 + 5 rows over a grid capped at 8192 waves: every wave runs two or three rows


@functools.lru_cache(maxsize=None)
def grid_stride_case():
    nseq = (GS_ROWS + GS_S - 1) // GS_S                    # 443, the last sequence partial
    g = torch.Generator().manual_seed(77)
    ga = lambda s: (torch.rand(GS_D, generator=g) + 0.5) * s   # noqa: E731
    be = lambda o: torch.randn(GS_D, generator=g) * 0.1 + o    # noqa: E731
    groups = [(0, 100, ga(1.0), be(0.0)), (100, 250, ga(2.0), be(1.0)), (350, nseq - 350, ga(0.5), be(-1.0))]
    x = torch.randn(GS_ROWS, GS_D, generator=g) * 3 + 0.5
    tok0 = torch.randn(nseq, GS_D, generator=g) * 2 - 1.5
    return x, groups, tok0, nseq


def test_grid_stride_case_reaches_the_prefetched_rows():
    x, groups, tok0, nseq = grid_stride_case()
    first = torch.arange(nseq) * GS_S
    assert (first < 8192).any() and ((first >= 8192) & (first < 16384)).any()   # replaced rows in a wave's first iteration and in prefetched ones
    assert GS_ROWS == 2 * 8192 + 5 and first[-1] < GS_ROWS
    for stride in (0, GS_D):
        ref, xw, _ = ln_eval(x, GS_S, groups, tok0=tok0, stride=stride)
        for mut in ("stale_seq", "tok0_old_row", "neighbour_group"):
            assert rejects(ln_eval(x, GS_S, groups, dtype=torch.float32, tok0=tok0, stride=stride, mut=mut)[0], ref, F32, A_LN), mut


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LN_KINDS, ids=LN_KIND_ID)
@pytest.mark.parametrize("stride", [0, GS_D])
def test_layernorm_grid_stride_tok0_and_groups(dev, stride, kind):
    """More rows than waves: the prefetch hand-over (row, sequence index, replacement flag) with three groups and the token-0
    replacement; the written-back x is bit-equal to tok0 on the rows seq * S and untouched elsewhere."""
    prec = out_prec(kind)
    x, groups, tok0, nseq = grid_stride_case()
    ref, xw_ref, _ = ln_ref(x, GS_S, groups, kind, tok0=tok0, stride=stride)
    val, _, xw = ln_run(dev, x, GS_S, groups, kind, tok0=tok0, stride=stride)
    assert_bits(xw, xw_ref, "x after the token-0 write-back")
    first = torch.arange(nseq) * GS_S
    assert torch.equal(xw[first], tok0 if stride else tok0[:1].expand(nseq, GS_D))
    record("layernorm grid-stride tok0", LN_KIND_ID(kind), assert_close_in(val, ref, prec, A_LN, what=f"layernorm grid-stride stride={stride}"))


@pytest.mark.gpu
def test_layernorm_fp8_saturates(dev):
    x, groups, S = ln_saturating()
    ref, _, _ = ln_eval(x, S, groups, scale=FP8_INV)
    val, raw, _ = ln_run(dev, x, S, groups, (FP8, 0))
    assert not ((raw & 0x7f) == 0x7f).any(), "NaN bytes"
    over = ref.abs() > 448.0 * (1 + 1e-5)
    assert over.any() and torch.equal(val[over], 448.0 * ref[over].sign().float())
    record("layernorm saturating", "fp8", assert_close_in(val, ref.clamp(-448.0, 448.0), FP8, A_LN, what="layernorm saturating e4m3"))


@pytest.mark.gpu
def test_layernorm_ex_argument_checks(dev):
    from burn_depth_amd import _lib, ops
    g1 = lambda D: [(0, 2, torch.ones(D).cuda(), torch.zeros(D).cuda())]  # noqa: E731
    for D, code in ((66, _lib.MD_ERR_UNSUPPORTED), (1028, _lib.MD_ERR_UNSUPPORTED)):
        with pytest.raises(_lib.MdError) as e:
            ops.layernorm_ex(dev, torch.zeros(2, D).cuda(), 1, g1(D), LN_EPS, BF16)
        assert e.value.code == code
    x = torch.zeros(4, 64).cuda()
    with pytest.raises(_lib.MdError) as e:   # groups that do not cover the rows
        ops.layernorm_ex(dev, x, 1, g1(64), LN_EPS, BF16)
    assert e.value.code == _lib.MD_ERR_SHAPE
    with pytest.raises(_lib.MdError) as e:   # groups that do not follow each other
        ops.layernorm_ex(dev, x, 1, [(0, 2, None, None), (3, 2, None, None)], LN_EPS, BF16)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG
    with pytest.raises(_lib.MdError) as e:
        ops.layernorm_ex(dev, x, 1, [(0, 4, None, None)], LN_EPS, 7)
    assert e.value.code == _lib.MD_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("N,K", FOLD_CASES)
def test_ln_fold_vectors_against_fp64(dev, N, K, prec):
    from burn_depth_amd import ops
    W, gamma, beta, bias = fold_inputs(N, K)
    for b in (bias, None):
        ref = fold_eval(W, gamma, beta, b, prec)
        c, d = ops.ln_fold_vectors(dev, W.cuda(), gamma.cuda(), beta.cuda(), b.cuda() if b is not None else None, prec)
        for name, got, r in (("c", c.cpu(), ref[0]), ("d", d.cpu(), ref[1])):
            bound = 0.5 * ulp_f32(r) + 1e-12 * r.abs().max()
            ratio = ((got.double() - r).abs() / bound).max().item()
            print(f"[operand_writers] ln_fold_vectors {name} {N}x{K} {PNAME[prec]} bias={b is not None}: worst err/bound {ratio:.3f}")
            record("ln_fold_vectors " + name, PNAME[prec], {"worst_ratio": ratio, "slack_share": 0.0, "n": N})
            assert fold_bad(got, r) == 0, f"{name}: {fold_bad(got, r)} of {N} outside the final fp32 half-ulp, worst {ratio:.3f}"


@pytest.mark.gpu
@pytest.mark.parametrize("rows", FINISH_ROWS)
def test_ln_finish_against_fp64(dev, rows):
    from burn_depth_amd import ops
    parts = finish_parts()[:rows]
    ref = finish_eval(parts)
    ab = ops.ln_finish(dev, parts.cuda(), 1.0 / 1024.0, FINISH_EPS).cpu()
    ratio = ((ab.double() - ref).abs() / (4 * ulp_f32(ref))).max().item()
    print(f"[operand_writers] ln_finish rows={rows}: worst err / (4 ulp) {ratio:.3f}")
    record("ln_finish", "f32", {"worst_ratio": ratio, "slack_share": 0.0, "n": 2 * rows})
    assert not finish_bad(ab, ref).any(), f"{int(finish_bad(ab, ref).sum())} of {rows} rows beyond 4 ulp, worst {ratio:.3f} of the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", STORE_PRECS, ids=lambda p: PNAME[p])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_direct_typed_against_fp64(dev, case, prec):
    """The FOV head's forms: input held in the mode's storage type, the fused add, out_ld > Cout (padding columns untouched)."""
    from burn_depth_amd import ops
    B, Cin, H, W, Cout, k, stride, pad = case
    x, w, bias, add = conv_inputs(case, prec)
    for a in (None, add):
        for relu in (False, True):
            ref = conv_eval(case, x, w, bias, a, relu)
            for out_ld in (0, Cout + 5):
                fill = prefill((*ref.shape[:3], out_ld or Cout), torch.float32)
                got = ops.conv2d_direct_ex(dev, x.cuda(), w.cuda(), bias.cuda(), a.cuda() if a is not None else None, stride, pad, relu, prec,
                                           out_ld, fill.cuda()).cpu()
                assert_bits(got[..., Cout:], fill[..., Cout:], "conv_direct padding columns")
                record("conv_direct", PNAME[prec], assert_close_in(got[..., :Cout], ref, F32, A_MFMA, what=f"conv_direct {case} {PNAME[prec]} add={a is not None} relu={relu} ld={out_ld}"))
