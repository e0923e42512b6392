"""Operator tests of the kernels that exist only for Depth-Anything-v3: the per-head q/k LayerNorm(64) + 2-D RoPE in its two
forms (form 0: the plain QKV GEMM followed by `qk_norm_rope_kernel`; form 1: the QKV GEMM's fused epilogue), `hook_cat_ln`,
`patchify` with the cls rows, `set_token0` and `border_bias_fix`, each against a plain fp64 torch reference written from the
operation's definition (oracle/da3_ref.py states the definition; the CPU tests hold the two together).

Tolerances are derived, none is taken from what the GPU produced. One checker, `assert_close_in(got, ref64, prec, a32)`, holds
every element to

    |got - ref| <= 0.5 * ulp_T(|ref|) * (1 + slack) + a32 * max|ref|

* ulp_T = the spacing of the storage type at |ref|: 2^(e-7) for bf16 (8 significant bits), 2^(e-10) for f16 (11 bits; never below
  the subnormal spacing 2^-24), 2^(e-21) for the split-half f16x2 (hi + lo, 22 bits; lo is an f16, same floor), absent for f32;
  2^e <= |ref| < 2^(e+1). A correctly rounded store is half of it away from the value it rounds.
* a32 = the fp32-arithmetic allowance this suite already uses: 2e-5 behind an MFMA contraction (tests/test_gpu_parity.py header:
  "MFMA kernels ... fp32 accumulate: 2e-5 (accumulation order)") and 2e-6 for LayerNorm-only kernels (tools/gpu_diag.py
  check_layernorm), both relative to the largest reference magnitude of the tensor compared.
* slack = 1 only where `ref` lies within a32 * max|ref| of a rounding boundary of T (the kernel's fp32 value and the fp64 value may
  fall on different sides of the tie), 0 elsewhere. Elements that need it (error above the slack-free bound) are counted and their
  share must stay under 1 % -- a condition of the test, checked on the CPU for the fp32 evaluation of the reference formula too.
* form 0 rounds the LayerNorm input to T before the norm (the stored q | k rows; what oracle/da3_ref.py emulates). Its reference
  rounds the same way, so an input within a32 * max|input| of a rounding boundary of T may come out one ulp_T(input) away in the
  kernel's fp32; that ulp is carried through the LayerNorm to first order (`flip_allowance`: the element, its RoPE partner and,
  through the row's mean and variance, the rest of its head row) and added to the bound; elements that need it count as slack users.
* distance between the two forms (rows t < n_tokens): f32 mode a32 * max|ref| (nothing rounds in between). In the 2-byte and
  split-half modes the forms differ by the rounding of the LayerNorm input. The bound is computed per element from the fp64
  reference: the propagated half-ulp of the rounded input, 0.5 * ulp_T(|y|) * rstd * |gamma|, summed over the rotation's two terms,
  plus the output half-ulp. Taken literally (own element only, one output rounding) that bound is missed by the reference
  arithmetic itself -- fp32 evaluation of both forms on the CPU, bf16, DA3-small grid: 3.06 times the bound, at elements whose own
  input is small -- because a rounded row also moves its mean and its variance, and because each form rounds its output. So the
  propagated term is the full first-order one, rstd * |gamma_j| * (h_j + mean(h) + |c^_j| * mean(|c^| h)) with h = 0.5 * ulp_T(|y|)
  and c^ the normalised row, and both outputs' half-ulps and both forms' fp32 allowances are added. The LayerNorm amplifies an
  input error by rstd, hence the premise on the inputs: every (row, head) of the LayerNorm input has a standard deviation above
  0.25 (checked on the CPU; the weights are drawn so that it is about 1).

The mutant tests (CPU) evaluate the reference formula in fp32, round to T and show the checker accepts it, then show that it
rejects each subtly wrong variant on every case where the variant is not the identity. A dropped eps is NOT caught at these input
scales (row variance O(1), eps 1e-5: 5e-6 relative, below the bound) and is not among the mutants. The eps of the stand-alone
kernel's q rows IS caught: they arrive scaled by s = 0.125 * log2(e), and normalising them with the plain eps is LN(y; eps / s^2),
1.5e-4 / var relative -- above the f16 and f16x2 bounds (mutant `q_eps_on_scaled_rows`; the kernel scales eps by s^2 for q).

The 64x64 and 128x64 tiles run the same k order and the same row-statistics exchange (two waves per row, `row_total` in
gemm_impl.h), so form 1 is asserted bit-identical across the two tiles.
"""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import close_check
from close_check import A_LN, A_MFMA, BF16, F16, F16X2, F32, PNAME, PRECS, ROUND, near_boundary, rejects, ulp_T  # noqa: F401
from oracle import da3_ref

assert_close_in = functools.partial(close_check.assert_close_in, tag="da3_token_ops")
ATTN_QSCALE = 0.125 * 1.4426950408889634
ROPE_BASE, QK_EPS = 100.0, 1e-5
TILE_128x64, TILE_64x64, TILE_256x256 = 3, 4, 0


def qscale_of(prec):
    return 1.0 if prec == F32 else ATTN_QSCALE


# ---------------------------------------------------------------------------------------------
# q/k LayerNorm(64) + 2-D RoPE: cases, reference, mutants
# ---------------------------------------------------------------------------------------------
# name: (D, K, ph, pw, S, T)
QK_CASES = {
    "small_37x74": (384, 384, 37, 74, 2739, 1),   # DA3-small, landscape grid; S = n_tokens (odd): the 2739 x 1152 x 384 GEMM
    "small_74x37": (384, 384, 74, 37, 2740, 1),   # portrait; S rounded up to 4 as the engine does
    "partial_5x7": (384, 384, 5, 7, 40, 3),       # partial last m-tile (120 rows), padding rows
    "heads16_9x4": (1024, 1024, 9, 4, 40, 2),     # 16 heads, long contraction
    "column_6x1": (128, 64, 6, 1, 8, 1),
    "row_1x6": (128, 64, 1, 6, 8, 1),
}
QK_ROWS = [(c, g) for c in QK_CASES for g in (0, 1)]
# mutant -> does it change anything on (case, global_pos)? The position mutants are hidden by global blocks (every patch at (1, 1)).
LOCAL_ONLY = lambda case, glob: glob == 0  # noqa: E731
GLOBAL_ONLY = lambda case, glob: glob == 1  # noqa: E731
ALWAYS = lambda case, glob: True  # noqa: E731
QK_MUTANTS = {
    "sin_sign": ALWAYS,
    "swap_row_col": LOCAL_ONLY,
    "patch_pos_from_0": LOCAL_ONLY,
    "row_divisor_ph": LOCAL_ONLY,
    "token0_at_1_1": ALWAYS,
    "k_scaled_too": lambda case, glob: True,  # (identity in f32 mode, where the scale is 1: the mutant tests run the 2-byte modes)
    "q_gamma_for_k": ALWAYS,
    "pair_j_j1": ALWAYS,
    "global_ignored": GLOBAL_ONLY,
}


def token_positions(n_tokens, S, ph, pw, glob, mut=None):
    """[S, 2] (row, column): token 0 and the padding rows t >= n_tokens at (0, 0), patch t at (1 + (t-1) / pw, 1 + (t-1) % pw),
    global blocks: every patch at (1, 1)."""
    pos = torch.zeros(S, 2, dtype=torch.long)
    pi = torch.arange(n_tokens - 1)
    if glob and mut != "global_ignored":
        pos[1:n_tokens] = 1
    else:
        first = 0 if mut == "patch_pos_from_0" else 1
        py = pi // (ph if mut == "row_divisor_ph" else pw)
        pos[1:n_tokens, 0] = first + py
        pos[1:n_tokens, 1] = first + pi % pw
        if mut == "swap_row_col":
            pos = pos.flip(1)
    if mut == "token0_at_1_1":
        pos[0] = 1
    return pos


def rope_angles(pos, base):
    """[S, 2, 16] fp32: angle = fp32(pos) * fp32(base^(-2f/32)), formed in fp32 as the oracle and the engine's table form it."""
    inv = 1.0 / torch.pow(torch.tensor(base, dtype=torch.float32), torch.arange(16, dtype=torch.float32) * 2 / 32)
    return pos.to(torch.float32)[:, :, None] * inv[None, None, :]


def qk_eval(yq, yk, par, geom, glob, qscale, dtype=torch.float64, mut=None, q_eps=None):
    """q' | k' from the LayerNorm inputs y = acc + bias [T, S, heads, 64]: LN_64(y) * gamma + beta, each 32-column half rotated in
    pairs (j, j + 16) by the row (first half) / column (second half) angle, q times the softmax scale. Everything after the fp32
    angle in `dtype`. Returns ([T*S, D], [T*S, D])."""
    ph, pw, S, n_tokens = geom
    ang = rope_angles(token_positions(n_tokens, S, ph, pw, glob, mut), ROPE_BASE).to(dtype)  # [S, 2, 16]
    cs, sn = ang.cos()[None, :, None], ang.sin()[None, :, None]                              # [1, S, 1, 2, 16]
    if mut == "sin_sign":
        sn = -sn
    out = []
    for which, y in enumerate((yq, yk)):
        y = y.to(dtype)
        g, b = par["gq" if (which == 0 or mut == "q_gamma_for_k") else "gk"].to(dtype), par["bk" if which else "bq"].to(dtype)
        eps = QK_EPS if (which or q_eps is None) else q_eps
        mean = y.mean(-1, keepdim=True)
        c = y - mean
        u = c / torch.sqrt((c * c).mean(-1, keepdim=True) + eps) * g + b
        T, S_, H, _ = u.shape
        if mut == "pair_j_j1":
            h = u.reshape(T, S_, H, 2, 16, 2)
            a, bb = h[..., 0], h[..., 1]
            o = torch.stack([a * cs - bb * sn, bb * cs + a * sn], -1).reshape(T, S_, H, 64)
        else:
            h = u.reshape(T, S_, H, 2, 2, 16)
            a, bb = h[..., 0, :], h[..., 1, :]
            o = torch.stack([a * cs - bb * sn, bb * cs + a * sn], -2).reshape(T, S_, H, 64)
        if which == 0 or mut == "k_scaled_too":
            o = o * qscale
        out.append(o.reshape(T * S_, H * 64))
    return out[0], out[1]


@functools.lru_cache(maxsize=16)
def qk_inputs(case, prec):
    """Operands representable in the mode's storage type; gammas of q and k drawn apart, betas and bias non-zero."""
    D, K, ph, pw, S, T = QK_CASES[case]
    g = torch.Generator().manual_seed(1000 + 17 * list(QK_CASES).index(case) + prec)
    rnd = ROUND[prec]
    x = rnd(torch.randn(T * S, K, generator=g))
    w = rnd(torch.randn(3 * D, K, generator=g) / math.sqrt(K))
    par = {"bias": torch.randn(3 * D, generator=g) * 0.3,
           "gq": torch.rand(64, generator=g) + 0.5, "gk": torch.rand(64, generator=g) + 0.5,
           "bq": torch.randn(64, generator=g) * 0.2, "bk": torch.randn(64, generator=g) * 0.2}
    y = x.double() @ w.double().T + par["bias"].double()
    H = D // 64
    yq, yk, v = (y[:, i * D:(i + 1) * D].reshape(T, S, H, 64) for i in range(3))
    return x, w, par, yq, yk, v.reshape(T, S, D)


def geom_of(case):
    D, K, ph, pw, S, T = QK_CASES[case]
    return ph, pw, S, ph * pw + 1


def form0_inputs(yq, yk, prec):
    """The stored rows the stand-alone kernel reads: q scaled by the softmax scale, both rounded to T (from the fp32 value)."""
    s = qscale_of(prec)
    return ROUND[prec]((yq * s).float()).double() / s, ROUND[prec](yk.float()).double()


def ln_gain(y, g):
    """rstd * |gamma| of the per-head LayerNorm, [T, S, H, 64] (fp64)."""
    c = y - y.mean(-1, keepdim=True)
    return (1.0 / torch.sqrt((c * c).mean(-1, keepdim=True) + QK_EPS)) * g.double().abs()


def ln_first_order(yq, yk, par, prec, h_of):
    """First-order reach of errors |e_i| <= h_i in the LayerNorm input, per output element and summed over the rotation's two terms
    (element j and its partner j +- 16); q in its scaled domain. The normalised row c^ = (y - mean) * rstd moves by
    rstd * (e_j - mean(e) - c^_j * mean(c^ e)), so |d LN_j| <= rstd * |gamma_j| * (h_j + mean(h) + |c^_j| * mean(|c^| h)): the element's
    own error, the row mean's and the row variance's. h_of(y_scaled) -> h. ([T*S, D], [T*S, D])"""
    out = []
    for which, (y, g) in enumerate(((yq, par["gq"]), (yk, par["gk"]))):
        s = 1.0 if which else qscale_of(prec)
        h = h_of(y * s)   # the scaled domain throughout: (h / s) * rstd * |gamma| * s
        c = y - y.mean(-1, keepdim=True)
        chat = (c / torch.sqrt((c * c).mean(-1, keepdim=True) + QK_EPS)).abs()
        p = ln_gain(y, g) * (h + h.mean(-1, keepdim=True) + chat * (chat * h).mean(-1, keepdim=True))
        T, S, H, _ = p.shape
        hh = p.reshape(T, S, H, 2, 2, 16)
        out.append((hh + hh.flip(-2)).reshape(T * S, H * 64))
    return out[0], out[1]


def propagated_input_ulp(yq, yk, par, prec, weight):
    """`weight` ulps of the LayerNorm input's storage rounding carried through the LayerNorm and the rotation."""
    return ln_first_order(yq, yk, par, prec, lambda ys: weight * ulp_T(ys.abs(), prec))


def flip_allowance(yq, yk, par, prec):
    """form 0: one input ulp, carried the same way, for every LayerNorm input that sits within the fp32 allowance of a rounding
    boundary of T -- the GEMM's fp32 value may round to the other neighbour, which moves the element, its RoPE partner and (through
    the row's mean and variance) the other elements of its head row."""
    return ln_first_order(yq, yk, par, prec, lambda ys: ulp_T(ys.abs(), prec) * near_boundary(ys, prec, A_MFMA * ys.abs().max()))


def valid_rows(case):
    D, K, ph, pw, S, T = QK_CASES[case]
    return (torch.arange(T * S) % S) < ph * pw + 1


# ---- CPU tests -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,glob", QK_ROWS)
def test_reference_agrees_with_the_oracle(case, glob):
    """The fp64 reference of this file against oracle.da3_ref.rope2d + F.layer_norm in fp32 on the same inputs (scale 1): the
    reference the operator tests use and the oracle the end-to-end tests use cannot drift apart."""
    x, w, par, yq, yk, _ = qk_inputs(case, F32)
    ph, pw, S, n_tokens = geom_of(case)
    rq, rk = qk_eval(yq, yk, par, geom_of(case), glob, 1.0)
    pos = token_positions(n_tokens, S, ph, pw, glob)
    for y, gam, bet, ref in ((yq, par["gq"], par["bq"], rq), (yk, par["gk"], par["bk"], rk)):
        t = F.layer_norm(y.float().permute(0, 2, 1, 3), (64,), gam, bet, QK_EPS)     # [T, heads, S, 64]
        o = da3_ref.rope2d(t, pos, ROPE_BASE).permute(0, 2, 1, 3).reshape(ref.shape)
        assert (o.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


@pytest.mark.parametrize("case", list(QK_CASES))
def test_input_premise_every_head_row_has_spread(case):
    for prec in PRECS:
        _, _, _, yq, yk, _ = qk_inputs(case, prec)
        for y in (yq, yk) + form0_inputs(yq, yk, prec):
            assert y.std(-1, unbiased=False).min().item() > 0.25


@pytest.mark.parametrize("case,glob", QK_ROWS)
def test_checker_accepts_the_fp32_evaluation(case, glob):
    """The reference formula evaluated in fp32 and rounded to T passes `assert_close_in` (tie-slack share under 1 % included), for
    form 1 (unrounded LayerNorm input) and form 0 (rounded input), and the two evaluations keep the form-distance bound."""
    for prec in PRECS:
        x, w, par, yq, yk, _ = qk_inputs(case, prec)
        s, geom, rnd = qscale_of(prec), geom_of(case), ROUND[prec]
        ref1 = qk_eval(yq, yk, par, geom, glob, s)
        got1 = [rnd(t) for t in qk_eval(yq, yk, par, geom, glob, s, torch.float32)]
        for g1, r1 in zip(got1, ref1):
            assert_close_in(g1, r1, prec, A_MFMA, what=f"fp32 evaluation, form 1, {case} g{glob}")
        y0 = form0_inputs(yq, yk, prec)
        ref0 = qk_eval(*y0, par, geom, glob, s)
        got0 = [rnd(t) for t in qk_eval(*y0, par, geom, glob, s, torch.float32)]
        for g0, r0 in zip(got0, ref0):
            assert_close_in(g0, r0, prec, A_MFMA, what=f"fp32 evaluation, form 0, {case} g{glob}")
        assert_forms_within_distance(got0, got1, ref0, ref1, yq, yk, par, prec, valid_rows(case), f"fp32 evaluation, {case} g{glob}")


def assert_forms_within_distance(f0, f1, ref0, ref1, yq, yk, par, prec, rows, what):
    prop = propagated_input_ulp(yq, yk, par, prec, 0.5)
    for name, a, b, r0, r, p in zip("qk", f0, f1, ref0, ref1, prop):
        bound = p + 0.5 * ulp_T(r0.abs(), prec) + 0.5 * ulp_T(r.abs(), prec) + 2 * A_MFMA * r.abs().max()
        d = (a.double() - b.double()).abs()
        ratio = (d / bound)[rows]
        print(f"[da3_token_ops] {what} {PNAME[prec]} {name}: form distance max {d[rows].max().item():.3e}, worst distance/bound {ratio.max().item():.3f}")
        assert (d <= bound)[rows].all(), f"{what} {PNAME[prec]} {name}: forms {ratio.max().item():.3f} of the derived distance apart"


@pytest.mark.parametrize("mutant", list(QK_MUTANTS))
@pytest.mark.parametrize("case,glob", QK_ROWS)
def test_checker_rejects_qk_mutants(case, glob, mutant):
    """Each wrong variant, evaluated in fp32 and rounded like the real thing, is outside the bound -- in the loosest storage type
    (bf16) on every case, in all of them on the small case. Where the variant is the identity (position mutants under global
    blocks, `global_ignored` on local blocks) it must be ACCEPTED: the parametrisation says which is which."""
    precs = [BF16, F16, F16X2] + ([F32] if mutant != "k_scaled_too" else []) if case == "partial_5x7" else [BF16]
    for prec in precs:
        x, w, par, yq, yk, _ = qk_inputs(case, prec)
        s, geom = qscale_of(prec), geom_of(case)
        ref = qk_eval(yq, yk, par, geom, glob, s)
        got = [ROUND[prec](t) for t in qk_eval(yq, yk, par, geom, glob, s, torch.float32, mut=mutant)]
        rejected = any(rejects(g, r, prec, A_MFMA) for g, r in zip(got, ref))
        assert rejected == QK_MUTANTS[mutant](case, glob), f"{mutant} on {case} global={glob} {PNAME[prec]}"


@pytest.mark.parametrize("prec", [F16, F16X2])
def test_checker_rejects_plain_eps_on_the_scaled_q_rows(prec):
    """`q_eps_on_scaled_rows`: the stand-alone kernel reads q rows that carry the softmax scale s; LayerNorm with the plain eps on
    them is LN(y; eps / s^2). Caught in f16 and f16x2 (bf16's half-ulp hides it) -- the case that showed the kernel's defect."""
    case, glob = "partial_5x7", 0
    x, w, par, yq, yk, _ = qk_inputs(case, prec)
    s, geom = qscale_of(prec), geom_of(case)
    y0 = form0_inputs(yq, yk, prec)
    ref = qk_eval(*y0, par, geom, glob, s)
    got = qk_eval(*y0, par, geom, glob, s, torch.float32, q_eps=QK_EPS / (s * s))
    assert rejects(ROUND[prec](got[0]), ref[0], prec, A_MFMA)
    assert not rejects(ROUND[prec](got[1]), ref[1], prec, A_MFMA)


# ---------------------------------------------------------------------------------------------
# hook_cat_ln, border_bias_fix: references and mutants
# ---------------------------------------------------------------------------------------------
EPS_FINAL, EPS_HEAD = 1e-6, 1e-5


def hook_inputs(D, T, S, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return {"xl": r(T * S, D) * 1.5 + 0.3, "x": r(T * S, D) * 2.0 - 0.4, "ng": torch.rand(D, generator=g) + 0.5, "nb": r(D) * 0.2,
            "hg": torch.rand(2 * D, generator=g) + 0.5, "hb": r(2 * D) * 0.2}


def hook_eval(p, dtype=torch.float64, mut=None):
    """LayerNorm_head(cat(x_local, LayerNorm_final(x))) -> [rows, 2D]."""
    xl, x = p["xl"].to(dtype), p["x"].to(dtype)
    D = x.shape[1]
    ln = lambda t, g, b, eps: (t - t.mean(-1, keepdim=True)) / torch.sqrt(t.var(-1, unbiased=False, keepdim=True) + eps) * g.to(dtype) + b.to(dtype)  # noqa: E731
    if mut == "final_norm_on_wrong_half":
        cat = torch.cat([ln(xl, p["ng"], p["nb"], EPS_FINAL), x], -1)
    else:
        cat = torch.cat([xl, ln(x, p["ng"], p["nb"], EPS_FINAL)], -1)
    if mut == "head_stats_over_D":
        return torch.cat([ln(cat[:, :D], p["hg"][:D], p["hb"][:D], EPS_HEAD), ln(cat[:, D:], p["hg"][D:], p["hb"][D:], EPS_HEAD)], -1)
    return ln(cat, p["hg"], p["hb"], EPS_HEAD)


HOOK_CASES = [(64, 2, 12, 9), (384, 3, 40, 36), (1024, 2, 20, 17)]  # D, T, S, n_tokens


@pytest.mark.parametrize("D,T,S,n_tokens", HOOK_CASES)
def test_checker_on_hook_cat_ln_evaluations(D, T, S, n_tokens):
    p = hook_inputs(D, T, S, 40 + D)
    ref = hook_eval(p)
    for prec in PRECS:
        assert_close_in(ROUND[prec](hook_eval(p, torch.float32)), ref, prec, A_LN, what=f"fp32 evaluation, hook_cat_ln D={D}")
        for mut in ("head_stats_over_D", "final_norm_on_wrong_half"):
            assert rejects(ROUND[prec](hook_eval(p, torch.float32, mut)), ref, prec, A_LN), (mut, PNAME[prec])


def border_inputs(B, H, W, C_, ld, prec, seed):
    g = torch.Generator().manual_seed(seed)
    return ROUND[prec](torch.randn(B, H, W, ld, generator=g)), torch.randn(9, C_, generator=g) * 0.5


def border_eval(fmap, bias9, C_, dtype=torch.float64, mut=None):
    """map[b, y, x, :C] += bias9[3 * ry + rx] - bias9[4]; ry / rx: 0 first, 2 last, 1 interior row / column."""
    B, H, W, _ = fmap.shape
    hh, ww = (H - 1, W - 1) if mut == "last_row_col_missed" else (H, W)
    cls = lambda i, n: torch.where(i == 0, 0, torch.where(i == n - 1, 2, 1))  # noqa: E731
    ry, rx = cls(torch.arange(H), hh)[:, None].expand(H, W), cls(torch.arange(W), ww)[None, :].expand(H, W)
    if mut == "corners_as_edges":  # a corner takes its row's edge class
        rx = torch.where((ry != 1) & (rx != 1), 1, rx)
    b9 = bias9.to(dtype)
    out = fmap.to(dtype).clone()
    out[..., :C_] += (b9[3 * ry + rx] - b9[4])[None]
    return out


BORDER_CASES = [(2, 2), (2, 9), (37, 37)]


@pytest.mark.parametrize("H,W", BORDER_CASES)
def test_checker_on_border_bias_fix_evaluations(H, W):
    for prec in PRECS:
        fmap, b9 = border_inputs(2, H, W, 24, 32, prec, 7 + H)
        ref = border_eval(fmap, b9, 24)
        assert_close_in(ROUND[prec](border_eval(fmap, b9, 24, torch.float32)), ref, prec, A_LN, what=f"fp32 evaluation, border {H}x{W}")
        for mut in ("corners_as_edges", "last_row_col_missed"):
            assert rejects(ROUND[prec](border_eval(fmap, b9, 24, torch.float32, mut)), ref, prec, A_LN), (mut, PNAME[prec])


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


RECORD = {}  # (operator, precision, form) -> (largest error, its bound, worst error / bound)


def record(key, r):
    old = RECORD.get(key)
    if old is None or r["worst_ratio"] > old[2]:
        RECORD[key] = (r["max_err"], r["bound_at_max"], r["worst_ratio"])


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    """With DA3_TOKEN_OPS_ERRORS=<path> the largest error per (operator, precision, form) is written next to its bound."""
    yield
    path = os.environ.get("DA3_TOKEN_OPS_ERRORS")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("operator precision form | largest |got - ref| | derived bound at that element | worst error / bound over all elements\n")
            for (op, prec, form), (e, b, ratio) in sorted(RECORD.items()):
                f.write(f"{op:24s} {PNAME[prec]:6s} {form:8s} | {e:.3e} | {b:.3e} | {ratio:.3f}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,glob", QK_ROWS)
def test_qkv_norm_rope_forms_against_fp64(dev, case, glob, prec):
    """Both forms, both 64-column tiles: each form per element against fp64 (form 1 on every row -- the padding rows sit at
    (0, 0) --, form 0 on the rows t < n_tokens); V of form 1 bit-identical to V of form 0 and equal to the fp64 projection rounded
    to T; form 1 bit-identical across the tiles; the forms within their derived distance of each other."""
    from burn_depth_amd import ops
    D, K, ph, pw, S, T = QK_CASES[case]
    x, w, par, yq, yk, v64 = qk_inputs(case, prec)
    s, geom, rows = qscale_of(prec), geom_of(case), valid_rows(case)
    ref1 = qk_eval(yq, yk, par, geom, glob, s)
    y0 = form0_inputs(yq, yk, prec)
    ref0 = qk_eval(*y0, par, geom, glob, s)
    extra0 = flip_allowance(yq, yk, par, prec)
    cu = lambda t: t.cuda()  # noqa: E731
    run = lambda tile, form: [t.cpu() for t in ops.qkv_norm_rope(  # noqa: E731
        dev, cu(x), cu(w), cu(par["bias"]), cu(par["gq"]), cu(par["bq"]), cu(par["gk"]), cu(par["bk"]), geom[3], S, pw, bool(glob),
        ROPE_BASE, QK_EPS, prec, tile, form)]
    out = {(tile, form): run(tile, form) for tile in (TILE_64x64, TILE_128x64) for form in (0, 1)}
    for tile, tname in ((TILE_64x64, "64x64"), (TILE_128x64, "128x64")):
        q0, k0, v0 = out[(tile, 0)]
        q1, k1, v1 = out[(tile, 1)]
        for name, g1, r1 in (("q", q1, ref1[0]), ("k", k1, ref1[1])):
            record(("qkv_norm_rope " + name, prec, "1 fused"), assert_close_in(g1, r1, prec, A_MFMA, what=f"form 1 {tname} {case} g{glob} {name}"))
        for name, g0, r0, e0 in (("q", q0, ref0[0], extra0[0]), ("k", k0, ref0[1], extra0[1])):
            record(("qkv_norm_rope " + name, prec, "0 kernel"),
                   assert_close_in(g0[rows], r0[rows], prec, A_MFMA, extra=e0[rows], what=f"form 0 {tname} {case} g{glob} {name}"))
        assert torch.equal(v1, v0), f"{tname}: the q/k branch disturbed the V tiles"
        record(("qkv_norm_rope v", prec, "1 fused"), assert_close_in(v1.reshape(T * S, D), v64.reshape(T * S, D), prec, A_MFMA, what=f"V {tname} {case}"))
        if prec == F32:
            for a, b, r in ((q0, q1, ref1[0]), (k0, k1, ref1[1])):
                assert ((a - b).abs()[rows] <= A_MFMA * r.abs().max()).all()
        else:
            assert_forms_within_distance((q0, k0), (q1, k1), ref0, ref1, yq, yk, par, prec, rows, f"{tname} {case} g{glob}")
    for i, name in enumerate("qkv"):
        assert torch.equal(out[(TILE_64x64, 1)][i], out[(TILE_128x64, 1)][i]), f"form 1 {name}: the two tiles differ"


@pytest.mark.gpu
def test_qkv_norm_rope_refuses_a_tile_without_the_epilogue(dev):
    from burn_depth_amd import _lib, ops
    x, w, par, *_ = qk_inputs("column_6x1", BF16)
    with pytest.raises(_lib.MdError) as e:
        ops.qkv_norm_rope(dev, x.cuda(), w.cuda(), par["bias"].cuda(), par["gq"].cuda(), par["bq"].cuda(), par["gk"].cuda(), par["bk"].cuda(),
                          7, 8, 1, False, ROPE_BASE, QK_EPS, BF16, TILE_256x256, 1)
    assert e.value.code == _lib.MD_ERR_UNSUPPORTED


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,glob", [("partial_5x7", 0), ("partial_5x7", 1), ("heads16_9x4", 0), ("column_6x1", 0), ("row_1x6", 0), ("small_74x37", 0)])
def test_qk_norm_rope_kernel_alone(dev, case, glob, prec):
    """The stand-alone kernel on caller rows (exact in T, q carrying the softmax scale): fp64 per element on the rows t < n_tokens;
    the rows t >= n_tokens come back bit-equal to the input."""
    from burn_depth_amd import ops
    D, K, ph, pw, S, T = QK_CASES[case]
    x, w, par, yq, yk, _ = qk_inputs(case, prec)
    s, geom, rows = qscale_of(prec), geom_of(case), valid_rows(case)
    y0 = form0_inputs(yq, yk, prec)
    qk_in = torch.cat([(y0[0] * s).reshape(T * S, D), y0[1].reshape(T * S, D)], 1).float()
    assert torch.equal(ROUND[prec](qk_in), qk_in)
    ref = qk_eval(*y0, par, geom, glob, s)
    got = ops.qk_norm_rope(dev, qk_in.cuda(), par["gq"].cuda(), par["bq"].cuda(), par["gk"].cuda(), par["bk"].cuda(), geom[3], S, pw, bool(glob),
                           ROPE_BASE, QK_EPS, prec).cpu()
    for name, gt, r in (("q", got[:, :D], ref[0]), ("k", got[:, D:], ref[1])):
        record(("qk_norm_rope " + name, prec, "alone"), assert_close_in(gt[rows], r[rows], prec, A_LN, what=f"qk_norm_rope {case} g{glob} {name}"))
    assert (~rows).any() and torch.equal(got[~rows], qk_in[~rows])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("D,T,S,n_tokens", HOOK_CASES)
def test_hook_cat_ln(dev, D, T, S, n_tokens, prec):
    from burn_depth_amd import ops
    p = hook_inputs(D, T, S, 40 + D)
    ref = hook_eval(p)
    rows = (torch.arange(T * S) % S) < n_tokens
    keep = ROUND[prec](torch.randn(T * S, 2 * D, generator=torch.Generator().manual_seed(3)) * 7)
    c = {k: t.cuda() for k, t in p.items()}
    for with_cam in (True, False):
        out, cam = ops.hook_cat_ln(dev, c["xl"], c["x"], n_tokens, S, c["ng"], c["nb"], EPS_FINAL, c["hg"], c["hb"], EPS_HEAD, prec, keep.cuda(), with_cam)
        out = out.cpu()
        record(("hook_cat_ln", prec, "-"), assert_close_in(out[rows], ref[rows], prec, A_LN, what=f"hook_cat_ln D={D} cam={with_cam}"))
        assert torch.equal(out[~rows], keep[~rows]), "rows t >= n_tokens were written"
        if with_cam:
            assert torch.equal(cam.cpu(), torch.cat([p["xl"][::S], p["x"][::S]], 1))
        else:
            assert cam is None


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,W", [(70, 42), (518, 518), (14, 14)])
def test_patchify(dev, H, W, prec):
    """Pure data movement: the input value's exact rounding to T (bit-exact in f32), zero tail columns; with the cls rows the same
    launch writes cls + pos0 (one fp32 addition: exact against torch's) and zeroes the padding rows, and leaves the rest alone."""
    from burn_depth_amd import ops
    g = torch.Generator().manual_seed(H + W)
    B, ps, D = 2, 14, 128
    x = torch.randn(B, 3, H, W, generator=g)
    ph, pw = H // ps, W // ps
    n_tokens, S = ph * pw + 1, (ph * pw + 1 + 3) // 4 * 4 + 4
    want = x.reshape(B, 3, ph, ps, pw, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * ph * pw, 3 * ps * ps)
    cls, pos0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    stream = torch.randn(B * S, D, generator=g)
    for Kp in ((588 + 63) // 64 * 64, 704):  # the model's rounding of 3 * 14 * 14 and a larger row
        for with_cls in (False, True):
            out, cx = ops.patchify(dev, x.cuda(), ps, Kp, prec, stream.cuda() if with_cls else None, S, cls.cuda(), pos0.cuda())
            out = out.cpu()
            assert torch.equal(out[:, :588], ROUND[prec](want))
            assert torch.equal(out[:, 588:], torch.zeros(out.shape[0], Kp - 588))
            if with_cls:
                exp = stream.clone().reshape(B, S, D)
                exp[:, 0] = cls + pos0
                exp[:, n_tokens:] = 0
                assert torch.equal(cx.cpu(), exp.reshape(B * S, D))
            else:
                assert cx is None


@pytest.mark.gpu
@pytest.mark.parametrize("src_stride", [0, 192])
def test_set_token0(dev, src_stride):
    from burn_depth_amd import ops
    g = torch.Generator().manual_seed(11)
    nseq, S, D = 3, 40, 192
    x, src = torch.randn(nseq * S, D, generator=g), torch.randn(nseq, D, generator=g)
    exp = x.clone().reshape(nseq, S, D)
    exp[:, 0] = src if src_stride else src[0]
    assert torch.equal(ops.set_token0(dev, x.cuda(), S, src.cuda(), src_stride).cpu(), exp.reshape(nseq * S, D))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("H,W", BORDER_CASES)
def test_border_bias_fix(dev, H, W, prec):
    from burn_depth_amd import ops
    B, C_, ld = 2, 24, 32
    fmap, b9 = border_inputs(B, H, W, C_, ld, prec, 7 + H)
    ref = border_eval(fmap, b9, C_)
    got = ops.border_bias_fix(dev, fmap.cuda(), C_, b9.cuda(), prec).cpu()
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert torch.equal(got[:, ~border], fmap[:, ~border]), "interior pixels were written"
    assert torch.equal(got[..., C_:], fmap[..., C_:]), "padding columns were written"
    record(("border_bias_fix", prec, "-"), assert_close_in(got[:, border][..., :C_], ref[:, border][..., :C_], prec, A_LN, what=f"border {H}x{W}"))
