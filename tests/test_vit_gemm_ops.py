"""Operator tests of the GEMM forms the engines launch for the ViT token stream, through `ops.vit_gemm` (md_op_vit_gemm): the residual +
LayerScale update of proj / fc2 (EPI_RESID_LS: in place and out of place, grouped weights with aliased A rows, every tile), its
LayerNorm-fold producer part (`ln_out`, the per-tile statistics), the fold's consumer kinds of the QKV projection and fc1 (`ln_raw` 0 and
1, direct store on and off), the plain QKV store of the 256 x 256 kernel (q scaled before its one rounding, k, the transposed V^T), the
patch embedding, the producer -> consumer chain, and the tile loops against the one-tile kernel bit for bit. References are torch fp64
from each operation's definition on the operands as the device holds them (`close_check.ROUND`); every output buffer is the caller's and
filled with a canary, and what a launch must leave alone (rows between and behind the groups, rows 0 and 1 + P .. of a sequence, the key
columns S .. kpad of V^T) has to come back bit for bit. `ops.gemm_last_form()` says which kernel ran.

Where the bounds come from (u = 2^-24; none is taken from a GPU result; the CPU tests evaluate every reference formula in fp32 and must
pass, and reject the mutants listed at `MUTANTS`):

* resid, x_new = fma(ls, acc + b, x): the contraction gets the suite's allowance behind an MFMA, A_MFMA max|ls (acc + b)| (accumulation
  order of exact products; the rounding of acc + b, u |acc + b| |ls|, is far inside it), and the fma rounds once: u |x_new|. fp8: the
  reference quantises as the device does (activations * 448/8 in fp32, clamped, e4m3; weights per row with scale = amax * fp32(1/448)), so
  the same bound holds with the dequantising product acc * (ascale * wscale[n]) as one more fp32 rounding inside A_MFMA.
* ln_out: the kernel stores round_T(xnew * gamma_next) where xnew is the very fp32 vector it stores to x (gemm_impl.h, the EK_RMW_LN
  epilogue: `store4p(.., xnew * gam4)`), a lone fp32 product (nothing to contract it with). So ln_out == round_T(fp32(gamma_next[n] *
  x_new[m, n])) of the RETURNED x_new, bit for bit -- tolerance 0 -- for the one-plane types. Split-half: hi = f16(fp32 product) and
  lo = f16(product - hi), and that subtraction directly behind the product is free to contract into an fma (hipcc's default), so lo may
  be taken from the UNROUNDED product: the value is then within half a 22-bit ulp of gamma . x_new itself instead of within half an ulp
  of its fp32 rounding. Both are covered by 0.5 ulp_T + u |gamma . x_new| against the fp64 product, which is what the test holds the
  split-half ln_out to; the CPU test puts both evaluations (lo from the rounded and from the unrounded product) through it.
* per-tile statistics against fp64 statistics of the returned x_new. The kernel's tree: a lane adds its 4 columns (2 levels), 16 lanes
  add up (4 levels): the wave's mean over 64 columns carries |e_w| <= 6u A1_w (A1 = mean |x| over those columns; the factor 1/64 is
  exact); four wave means are averaged (2 levels): |e_t| <= 8u A1_t. M2: dl = x - mean_w (u), squares and their sums inside the lane
  (<= 3 roundings, fma or not), 4 lane levels, 3 levels over the waves and the between-wave term: every (non-negative) term carries a
  relative error of at most 12u. The tree sums deviations from the COMPUTED means, and sum_j (x_j - c)^2 about any c gives exactly
  Q = M2_t + 256 e_t^2 + 128 sum_w (mean_w' - mean_t') e_w (primes: computed). Hence
  |M2' - M2_t| <= 12u Q + 256 E_t^2 + 128 sum_w (|mean_w - mean_t| + E_w + E_t) E_w with E_w = 6u A1_w, E_t = 8u A1_t.
  Both input classes: for randn * 3 + 0.5 the first term dominates; for the ViT-like class (row mean of a few units, two channels
  of +-60 in different tiles) the wave that holds an outlier sits about 1 away from its tile mean and the last term is of the same
  order as the first. `stats_fp32_tree` evaluates that order in fp32 on the CPU.
* fold consumer: ref = rstd (A' Wr^T - mu c) + d (times qscale on q, through the exact-erf GELU for fc1), rstd and mu from the fp64
  Chan combination of the fp32 partials, c and d fp64 sums over Wr rounded to fp32. 0.5 ulp_T with tie slack + A_MFMA max|ref|, plus
  the cancellation term: the kernel forms acc * rstd + (c * (-mu rstd) + d); acc and mu c are each wrong by A_MFMA of their size
  (accumulation order; the fp32 Chan combination and the roundings of c and of the pair are u-sized) and then cancel, so the term is
  A_MFMA rstd_m (max_n |acc_mn| + |mu_m| max|c|), times qscale on q. It scales with |mu| and rstd, i.e. it is the same expression
  for both input classes (the ViT-like class has |mu| rstd of 0.5 - 1, the plain class 0.17). GELU: its slope is at most 1.13, so the
  pre-activation terms (A_MFMA max|pre| and the cancellation term) are multiplied by 1.13, and the polynomial's error is added as
  test_gelu_epilogue_pointwise_error_and_saturation states it: 1.05 * (8.5e-5 bf16, 6.6e-7 f16, 3.4e-7 split-half).
* plain qkv and patch_embed: 0.5 ulp_T with tie slack + A_MFMA max|ref| (fp32 rows for patch_embed).
* chain: the consumer's reference is built from the RETURNED x_new (fp64 statistics, A' = the returned ln_out); the device's statistics
  differ from those by the producer bounds above (relative 12u on M2, 8u A1 on a mean), three orders below the A_MFMA-sized relative
  freedom the cancellation term already gives mu and rstd, so the consumer bound is used unchanged.

What cannot be told apart at these shapes: `qscale_after_rounding` in f16x2 (a second rounding to 22 bits, 2.4e-7 relative, is below
A_MFMA max|ref|) and in f32 (qscale = 1: the identity, as is `qscale_on_k`); `vt_global_token_index` on one sequence. `c_from_unrounded_w`
is the identity here for bf16, f16 and split-half with f16-exact weights, because the weights of these tests are exact in the operand
type (as every operand is), and for split-half with fp32 weights it is a 22-bit rounding of W, below A_MFMA max|ref|: the CPU test
asserts that it is NOT rejected (and is the identity where it is one); tests/test_operand_writers.py (ln_fold_vectors on unrounded
weights, half an fp32 ulp against the operand-rounded W) is what catches it. The between-tile term belongs to the consumer (ln_raw = 1) and to ln_finish; the
producer's own statistics have the between-wave term."""
import functools
import math
import os

import pytest
import torch

import close_check
from close_check import A_MFMA, BF16, F16, F16X2, F32, FP8, PNAME, ROUND, rejects

assert_close_in = functools.partial(close_check.assert_close_in, tag="vit_gemm_ops")
RESID, QKV, FC1, PATCH = 0, 1, 2, 3
T256, T128, T64, TAUTO = 0, 1, 4, 99
EK_GENERIC, EK_RMW, EK_STORE, EK_RMW_LN, EK_QKV_LN, EK_GELU_LN, EK_GELU_LN_DS = 0, 1, 2, 5, 6, 7, 11
ONE_TILE, LOOP_P, LOOP_R = 0, 1, 2
ATTN_QSCALE = float(torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32))
U = 2.0 ** -24
LN_EPS = 1e-6
GELU_POLY = {BF16: 8.5e-5 * 1.05, F16: 6.6e-7 * 1.05, F16X2: 3.4e-7 * 1.05}
# (precision, weights): split-half runs with f16-exact weights (two MFMA terms) and with fp32 weights (three)
MODES = [(BF16, "w"), (F16, "w"), (F16X2, "w16"), (F16X2, "w32"), (F32, "w"), (FP8, "w")]
FOLD_MODES = [(BF16, "w"), (F16, "w"), (F16X2, "w16"), (F16X2, "w32")]
MODE_ID = lambda m: PNAME[m[0]] + ("" if m[1] == "w" else "_" + m[1])  # noqa: E731
CLASSES = ["plain", "vit"]


def qscale_of(prec):
    return 1.0 if prec == F32 else ATTN_QSCALE


def canary(*shape):
    """Values exact in every storage type (multiples of 1/4 below 32), no two neighbours equal."""
    n = math.prod(shape)
    return ((torch.arange(n) % 97 + 3).float() * 0.25).reshape(shape)


def round_w(W, mode):
    """The weight as the device's operand holds it."""
    prec, wk = mode
    if prec == FP8:
        return W
    return ROUND[F16](W) if wk == "w16" else ROUND[prec](W)


def stream(rows, D, cls, g):
    """fp32 residual-stream rows of the two input classes."""
    if cls == "plain":
        return torch.randn(rows, D, generator=g) * 3 + 0.5
    x = torch.randn(rows, D, generator=g) + (torch.rand(rows, 1, generator=g) * 4 + 1) * (torch.randint(0, 2, (rows, 1), generator=g) * 2 - 1)
    x[:, 7] += 60.0 + torch.randn(rows, generator=g)
    x[:, D - 200] -= 60.0 + torch.randn(rows, generator=g)   # another 256-column tile (D = 1024: tile 3)
    return x


# ---------------------------------------------------------------------------------------------
# groups
# ---------------------------------------------------------------------------------------------
def layout(sizes, gap=4, tail=7, alias=True):
    """[(row0, rows, arow0)], output rows, A rows: canary rows between the groups and behind the last; group 1 reads group 0's A rows."""
    out, r, a = [], 0, 0
    for i, n in enumerate(sizes):
        if alias and i == 1:
            out.append((r, n, 0))
        else:
            out.append((r, n, a))
            a += n
        r += n + gap
    return out, r - gap + tail, a


def row_index(groups, out_rows):
    """(group of every output row or -1, its A row)."""
    gi, ar = torch.full((out_rows,), -1, dtype=torch.long), torch.zeros(out_rows, dtype=torch.long)
    for i, (r0, n, a0) in enumerate(groups):
        gi[r0:r0 + n] = i
        ar[r0:r0 + n] = a0 + torch.arange(n)
    return gi, ar


def per_row(vecs, gi, mut_neighbour=False):
    """[rows, N] of the groups' vectors (zeros on canary rows)."""
    v = torch.stack(list(vecs))
    g = (gi + 1) % len(vecs) if mut_neighbour else gi
    return torch.where((gi >= 0)[:, None], v[g.clamp_min(0)], torch.zeros_like(v[0]))


# ---------------------------------------------------------------------------------------------
# case 1 / 2: resid (+ producer)
# ---------------------------------------------------------------------------------------------
# (sizes key, N, K, tile)
RESID_SHAPES = [(293, 1024, 1024, T256), (293, 1024, 4096, T256), (1370, 384, 384, TAUTO), (1370, 384, 384, T64), (1370, 384, 1536, TAUTO),
                (1370, 384, 1536, T64), (129, 132, 64, T128)]
THREE = (300, 37, 293)
FP8_XS = torch.tensor(8.0, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)


def q8(x, inv):
    return (x.float() * inv).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()


def q8_rows(w):
    amax = w.abs().amax(1, keepdim=True).float()
    sc = torch.where(amax > 0, amax * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(amax))
    return q8(w, 1.0 / sc), sc


@functools.lru_cache(maxsize=4)
def resid_case(sizes, N, K, mode, cls="plain", producer=False):
    """Inputs and the fp64 pieces of x_new = x + ls (A Wr^T + b) over the groups' rows."""
    prec = mode[0]
    g = torch.Generator().manual_seed(sum(sizes) + N + K + prec)
    groups, out_rows, a_rows = layout(sizes)
    gi, ar = row_index(groups, out_rows)
    A = torch.randn(a_rows, K, generator=g) * (1.5 if prec == FP8 else 1.0)
    A = A if prec == FP8 else ROUND[prec](A)
    Ws = [round_w(torch.randn(N, K, generator=g) / K ** 0.5, mode) for _ in sizes]
    bs = [torch.randn(N, generator=g) for _ in sizes]
    lss = [(torch.rand(N, generator=g) + 0.5) * (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float() for _ in sizes]
    gas = [torch.rand(N, generator=g) + 0.5 + 0.5 * i for i in range(len(sizes))]
    x = canary(out_rows, N)
    x[gi >= 0] = stream(int((gi >= 0).sum()), N, cls, g)
    acc = torch.zeros(out_rows, N, dtype=torch.float64)
    for i, (r0, n, a0) in enumerate(groups):
        if prec == FP8:
            wq, wsc = q8_rows(Ws[i])
            acc[r0:r0 + n] = (q8(A[a0:a0 + n], 1.0 / FP8_XS).double() @ wq.double().t()) * (FP8_XS * wsc.t()).double()
        else:
            acc[r0:r0 + n] = A[a0:a0 + n].double() @ ROUND[F16X2 if mode == (F16X2, "w32") else prec](Ws[i]).double().t()
    return dict(groups=groups, out_rows=out_rows, gi=gi, ar=ar, A=A, Ws=Ws, bs=bs, lss=lss, gas=gas, x=x, acc=acc, N=N, K=K)


def resid_eval(c, dtype=torch.float64, mut=None, src=None):
    """x_new over all output rows (canary rows unchanged). `src`: what the out-of-place form reads (the mutant: the output buffer)."""
    gi = c["gi"]
    b = per_row(c["bs"], gi, mut == "neighbour_bias").to(dtype)
    ls = per_row(c["lss"], gi, mut == "neighbour_ls").to(dtype)
    upd = ls * (c["acc"].to(dtype) + b)
    x = (c["x"] if src is None else src).to(dtype)
    return torch.where((gi >= 0)[:, None], x + upd, c["x"].to(dtype)), upd


def resid_report(got, ref, upd):
    """A_MFMA max|ls (acc + b)| + u |x_new| per element (module docstring)."""
    err = (got.double() - ref).abs()
    bound = A_MFMA * upd.abs().max() + U * ref.abs()
    return {"worst_ratio": (err / bound).max().item(), "n_bad": int((err > bound).sum()), "slack_share": 0.0, "n": err.numel()}


def assert_resid(got, ref, upd, what):
    assert torch.isfinite(got).all(), what
    r = resid_report(got, ref, upd)
    print(f"[vit_gemm_ops] {what}: worst err/bound {r['worst_ratio']:.3f}")
    assert r["n_bad"] == 0, f"{what}: {r['n_bad']} of {r['n']} outside the bound, worst {r['worst_ratio']:.3f}"
    return r


def ln_out_expect(x_new, c, prec, mut=None, x_old=None, gas_now=None):
    """round_T(fp32(gamma_next . x_new)) on the groups' rows."""
    ga = per_row(gas_now if mut == "ln_out_current_gamma" else c["gas"], c["gi"])
    return ROUND[prec]((x_old if mut == "ln_out_old_x" else x_new).float() * ga)


def stats_ref(x):
    """fp64 (mean, M2) per 256-column tile [rows, N / 256, 2] and the bound of the module docstring [rows, N / 256, 2]."""
    rows, N = x.shape
    xw = x.double().reshape(rows, N // 256, 4, 64)
    mw, a1w = xw.mean(-1), xw.abs().mean(-1)
    mt, a1t = mw.mean(-1), a1w.mean(-1)
    m2 = ((xw - mt[..., None, None]) ** 2).sum((-1, -2))
    Ew, Et = 6 * U * a1w, 8 * U * a1t
    cross = 128 * (((mw - mt[..., None]).abs() + Ew + Et[..., None]) * Ew).sum(-1)
    Q = m2 + 256 * Et ** 2 + cross
    return torch.stack([mt, m2], -1), torch.stack([Et * (1 + 2.0 ** -20), 12 * U * (1 + 2.0 ** -20) * Q + 256 * Et ** 2 + cross], -1)


def tree16(s):
    """row_sum16's pairing: lane i with i + 8, then i + 4, i + 2, i + 1 (rotations by 8, 4, 2, 1; fp32 addition commutes)."""
    for h in (8, 4, 2, 1):
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def stats_fp32_tree(x, mut=None):
    """The kernel's summation order in fp32: 4 columns per lane, 16 lanes (`tree16`), 4 waves."""
    rows, N = x.shape
    v = x.float().reshape(rows, N // 256, 4, 16, 4)
    if mut == "uncentred":
        return torch.stack([v.mean((-1, -2, -3)), (v * v).sum((-1, -2, -3))], -1)
    mw = tree16((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) * (1.0 / 64.0)
    dl = v - mw[..., None, None]
    sq = dl * dl
    m2w = tree16((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
    mt = ((mw[..., 0] + mw[..., 1]) + (mw[..., 2] + mw[..., 3])) * 0.25
    d = mw - mt[..., None]
    dd = d * d
    m2 = (m2w[..., 0] + m2w[..., 1]) + (m2w[..., 2] + m2w[..., 3])
    if mut != "no_between_wave":
        m2 = m2 + 64.0 * ((dd[..., 0] + dd[..., 1]) + (dd[..., 2] + dd[..., 3]))
    return torch.stack([mt, m2], -1)


def stats_bad(got, ref, bound):
    return int(((got.double() - ref).abs() > bound).sum()), ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


# ---------------------------------------------------------------------------------------------
# case 3: the fold's consumer part
# ---------------------------------------------------------------------------------------------
CONS_K = 1024
CONS_SIZES = {"one": (340,), "two": (200, 136)}   # multiples of 4 (token buffers), partial last m-tiles


def chan(parts):
    """fp64 Chan combination of fp32 partials [rows, 4, 2] -> (mu, rstd)."""
    p = parts.double()
    mu = p[:, :, 0].mean(1)
    m2 = p[:, :, 1].sum(1) + 256.0 * ((p[:, :, 0] - mu[:, None]) ** 2).sum(1)
    return mu, 1.0 / torch.sqrt(m2 / 1024.0 + LN_EPS)


def chan_fp32(parts, mut=None):
    """The consumer epilogue's (ln_finish's) arithmetic in fp32 -> (rstd, -mu rstd)."""
    p = parts.float()
    mu = ((p[:, 0, 0] + p[:, 1, 0]) + (p[:, 2, 0] + p[:, 3, 0])) * 0.25
    d = p[:, :, 0] - mu[:, None]
    m2 = (p[:, 0, 1] + p[:, 1, 1]) + (p[:, 2, 1] + p[:, 3, 1])
    if mut != "no_between_tile":
        m2 = m2 + 256.0 * ((d[:, 0] ** 2 + d[:, 1] ** 2) + (d[:, 2] ** 2 + d[:, 3] ** 2))
    rstd = 1.0 / torch.sqrt(m2 * torch.tensor(1.0 / 1024.0) + torch.tensor(LN_EPS))
    return rstd, (mu if mut == "pair_sign" else -mu) * rstd


def parts_of(z):
    zt = z.double().reshape(z.shape[0], 4, 256)
    mean = zt.mean(-1)
    return torch.stack([mean, ((zt - mean[..., None]) ** 2).sum(-1)], -1).float()


@functools.lru_cache(maxsize=4)
def cons_case(kind, gkey, mode, cls):
    """A fold consumer launch: synthetic statistics of a seeded stream z, A' = round_T(gamma . z)."""
    prec = mode[0]
    sizes = CONS_SIZES[gkey]
    N = 768 if kind == QKV else 512
    g = torch.Generator().manual_seed(31 + kind + len(sizes) + prec + (cls == "vit"))
    groups, out_rows, a_rows = layout(sizes, tail=4 if kind == FC1 else 0, alias=False)
    if kind == QKV:
        out_rows = (out_rows + 67) // 68 * 68 + 68   # whole sequences of S = 68, and one more behind the last group: canary rows of q | k and V^T
    gi, ar = row_index(groups, out_rows)
    z = stream(out_rows, CONS_K, cls, g)
    gam, beta = torch.rand(CONS_K, generator=g) + 0.5, torch.randn(CONS_K, generator=g) * 0.2
    A = ROUND[prec](z * gam)[gi >= 0]
    Ws = [round_w(torch.randn(N, CONS_K, generator=g) / CONS_K ** 0.5, mode) for _ in sizes]
    bs = [torch.randn(N, generator=g) for _ in sizes]
    return dict(kind=kind, groups=groups, out_rows=out_rows, gi=gi, ar=ar, A=A, Ws=Ws, bs=bs, gam=gam, beta=beta, parts=parts_of(z), N=N, prec=prec,
                mode=mode, D=256, S=68)


def fold_vectors(c, dtype=torch.float64, mut=None):
    """(c, d) per group, fp64 sums over the operand-rounded weight, rounded to fp32 as the device receives them."""
    out = []
    for i, (W, b) in enumerate(zip(c["Ws"], c["bs"])):
        Wr = (W if mut == "c_from_unrounded_w" else ROUND[F16X2 if c["mode"] == (F16X2, "w32") else c["prec"]](W)).double()
        gam = c["gams"][i] if "gams" in c else c["gam"]   # (the chain: every producer group has its own gamma_next)
        cv = (gam.double() * Wr).sum(1).float()
        dv = (b.double() + (0.0 if mut == "d_without_beta" else (c["beta"].double() * Wr).sum(1))).float()
        out.append((cv, dv))
    return out


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v / 2.0 ** 0.5))


def cons_acc(c, A=None):
    A = c["A"] if A is None else A
    acc = torch.zeros(c["out_rows"], c["N"], dtype=torch.float64)
    ai = 0
    for (r0, n, _), W in zip(c["groups"], c["Ws"]):
        Wr = ROUND[F16X2 if c["mode"] == (F16X2, "w32") else c["prec"]](W).double()
        acc[r0:r0 + n] = A[ai:ai + n].double() @ Wr.t()
        ai += n
    return acc


def cons_eval(c, acc, mu, rstd, cd, dtype=torch.float64, mut=None, pair=None):
    """(the pre-rounding output [rows, N], the extra bound term [rows, N]). q columns carry qscale; fc1 runs through the exact-erf GELU.
    `pair` = fp32 (rstd, -mu rstd): the kernel's own expression acc * rstd + (c * (-mu rstd) + d) in `dtype`."""
    gi, prec, N = c["gi"], c["prec"], c["N"]
    cv, dv = per_row([v[0] for v in cd], gi).to(dtype), per_row([v[1] for v in cd], gi).to(dtype)
    if pair is not None:
        pre = acc.to(dtype) * pair[0].to(dtype)[:, None] + (cv * pair[1].to(dtype)[:, None] + dv)
    else:
        pre = rstd.to(dtype)[:, None] * (acc.to(dtype) - mu.to(dtype)[:, None] * cv) + dv
    canc = A_MFMA * rstd.double()[:, None] * (acc.abs().amax(1, keepdim=True) + mu.double().abs()[:, None] * cv.double().abs().max())
    if c["kind"] == QKV:
        D, qs = c["D"], qscale_of(prec)
        scale = torch.ones(N, dtype=dtype)
        scale[:D] = qs
        if mut == "qscale_on_k":
            scale[D:2 * D] = qs
        if mut == "qscale_after_rounding":
            pre = torch.cat([ROUND[prec](pre[:, :D].float()).to(dtype) * qs, pre[:, D:]], 1)
        else:
            pre = pre * scale
        return pre, canc.expand(-1, N) * scale.double().clamp_max(1.0)
    extra = 1.13 * (canc + A_MFMA * pre.double().abs().max()) + GELU_POLY[prec]
    return gelu64(pre) if dtype == torch.float64 else torch.nn.functional.gelu(pre), extra.expand(-1, N)


def vt_layout(v, T, S, D, mut=None):
    """V [T * S, D] -> V^T [T, D / 64, 64, kpad]; key columns S .. kpad keep the canary (the kernel stores tokens of the sequence only)."""
    H, kpad = D // 64, (S + 63) // 64 * 64
    out = canary(T, H, 64, kpad).to(v.dtype)
    vv = v.reshape(T, S, H, 64)
    if mut == "vt_not_transposed":
        flat = out.reshape(T, H, 64 * kpad)
        flat[:, :, :S * 64] = vv.permute(0, 2, 1, 3).reshape(T, H, S * 64)
        return flat.reshape(T, H, 64, kpad)
    if mut == "vt_global_token_index":
        flat = out.reshape(-1).clone()
        t, i, h, d = torch.meshgrid(torch.arange(T), torch.arange(S), torch.arange(H), torch.arange(64), indexing="ij")
        pos = ((t * H + h) * 64 + d) * kpad + t * S + i
        ok = pos < flat.numel()
        flat[pos[ok]] = vv[ok]
        return flat.reshape(T, H, 64, kpad)
    out[..., :S] = vv.permute(0, 2, 3, 1)
    return out


def split_qkv(c, y, valid, mut=None, dtype=None):
    """Output rows [rows, 3 D] -> (qk [rows, 2 D], vT) with the canary where the launch writes nothing."""
    D, S, rows = c["D"], c["S"], c["out_rows"]
    qk = canary(rows, 2 * D).to(y.dtype)
    qk[valid] = y[valid, :2 * D]
    vt = vt_layout(y[:, 2 * D:], rows // S, S, D, mut)
    if not valid.all():   # tokens of rows outside every group keep the canary
        mask = vt_layout(-valid[:, None].expand(-1, D).to(y.dtype), rows // S, S, D)   # -1 where a group's row lands: no canary value
        vt = torch.where(mask == -1, vt, canary(*vt.shape).to(y.dtype))
    return qk, vt


# ---------------------------------------------------------------------------------------------
# case 4 / 5: plain qkv, patch embed
# ---------------------------------------------------------------------------------------------
QKV_CASES = {"S68": (3, 68, 256, 320, T256), "S580": (3, 580, 256, 320, T256), "auto_S1372": (1, 1372, 384, 384, TAUTO)}   # T, S, D, K, tile
QKV_MODES = [(BF16, "w"), (F16, "w"), (F16X2, "w16"), (F16X2, "w32"), (F32, "w")]


@functools.lru_cache(maxsize=2)
def qkv_case(name, mode):
    T, S, D, K, tile = QKV_CASES[name]
    prec = mode[0]
    g = torch.Generator().manual_seed(T + S + D + prec)
    rows = T * S
    A = ROUND[prec](torch.randn(rows, K, generator=g))
    W = round_w(torch.randn(3 * D, K, generator=g) / K ** 0.5, mode)
    b = torch.randn(3 * D, generator=g)
    gi = torch.cat([torch.zeros(rows, dtype=torch.long), torch.full((S,), -1, dtype=torch.long)])   # one canary sequence behind the last row
    c = dict(kind=QKV, groups=[(0, rows, 0)], out_rows=rows + S, gi=gi, A=A, Ws=[W], bs=[b], N=3 * D, prec=prec, mode=mode, D=D, S=S, tile=tile)
    c["acc"] = cons_acc(c)
    return c


def qkv_wrote(c):
    """(rows a group covers, the V^T elements the launch writes): everything else is canary and compared bit for bit."""
    valid = c["gi"] >= 0
    return valid, vt_layout(-valid[:, None].expand(-1, c["D"]).double(), c["out_rows"] // c["S"], c["S"], c["D"]) == -1   # (-1 is no canary value)


def qkv_eval(c, dtype=torch.float64, mut=None):
    prec, D = c["prec"], c["D"]
    y = c["acc"].to(dtype) + c["bs"][0].to(dtype)
    qs = qscale_of(prec)
    q = ROUND[prec](y[:, :D].float()).to(dtype) * qs if mut == "qscale_after_rounding" else y[:, :D] * qs
    k = y[:, D:2 * D] * (qs if mut == "qscale_on_k" else 1.0)
    return split_qkv(c, torch.cat([q, k, y[:, 2 * D:]], 1), c["gi"] >= 0, mut)


PE = dict(D=256, K0=588, P=9, S=12, seqs=(8, 3))
PE_MODES = [(BF16, "w"), (F16, "w"), (F32, "w"), (F16X2, "w16"), (F16X2, "w32")]


@functools.lru_cache(maxsize=2)
def pe_case(mode):
    prec = mode[0]
    D, K0, P, S = PE["D"], PE["K0"], PE["P"], PE["S"]
    ke = 32 if prec == F32 else 64
    K = (K0 + ke - 1) // ke * ke                      # the engine pads the patch vector to whole k-tiles with zeros
    g = torch.Generator().manual_seed(77 + prec)
    n0, n1 = PE["seqs"]
    groups = [(0, n0 * P, 0), (n0 * P, n1 * P, P)]    # the second group re-reads A rows of the first (another encoder on the same patches)
    A = torch.zeros(n0 * P, K)
    A[:, :K0] = ROUND[prec](torch.randn(n0 * P, K0, generator=g))
    Ws, bs, poss = [], [], []
    for _ in groups:
        W = torch.zeros(D, K)
        W[:, :K0] = round_w(torch.randn(D, K0, generator=g) / K0 ** 0.5, mode)
        Ws.append(W), bs.append(torch.randn(D, generator=g)), poss.append(torch.randn(1 + P, D, generator=g))
    return dict(groups=groups, A=A, Ws=Ws, bs=bs, poss=poss, nseq=n0 + n1, prec=prec, mode=mode, K=K)


def pe_eval(c, dtype=torch.float64, mut=None):
    D, P, S = PE["D"], PE["P"], PE["S"]
    x = canary(c["nseq"] * S, D).to(dtype)
    for (r0, n, a0), W, b, pos in zip(c["groups"], c["Ws"], c["bs"], c["poss"]):
        Wr = ROUND[F16X2 if c["mode"] == (F16X2, "w32") else c["prec"]](W)
        y = c["A"][a0:a0 + n].to(dtype) @ Wr.to(dtype).t() + b.to(dtype)
        m = r0 + torch.arange(n)
        seq, p = m // P, m % P
        y = y + pos.to(dtype)[p if mut == "pos_row_p" else 1 + p]
        x[seq * S + (p if mut == "rows_at_seq_s_plus_p" else 1 + p)] = y
    return x


# ---------------------------------------------------------------------------------------------
# CPU tests: the fp32 evaluation of every reference passes its bound, the mutants do not
# ---------------------------------------------------------------------------------------------
MUTANTS = ["neighbour_ls", "neighbour_bias", "oop_reads_output", "ln_out_old_x", "ln_out_current_gamma", "no_between_wave", "no_between_tile",
           "uncentred", "pair_sign", "c_from_unrounded_w", "d_without_beta", "qscale_after_rounding", "qscale_on_k", "vt_not_transposed",
           "vt_global_token_index", "rows_at_seq_s_plus_p", "pos_row_p"]


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
def test_resid_checker_accepts_fp32_and_rejects_mutants(mode):
    for sizes in ((293,), THREE):
        c = resid_case(sizes, 384, 384, mode)
        ref, upd = resid_eval(c)
        got, _ = resid_eval(c, torch.float32)
        assert resid_report(got, ref, upd)["n_bad"] == 0
        for mut in ("neighbour_ls", "neighbour_bias"):
            bad = resid_report(resid_eval(c, torch.float32, mut)[0], ref, upd)["n_bad"] > 0
            assert bad == (len(sizes) > 1), (mut, sizes)
        assert resid_report(resid_eval(c, torch.float32, src=canary(*c["x"].shape) * 1.5)[0], ref, upd)["n_bad"] > 0   # oop_reads_output


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("mode", FOLD_MODES, ids=MODE_ID)
def test_producer_checker_accepts_fp32_and_rejects_mutants(mode, cls):
    prec = mode[0]
    for sizes in ((293,), THREE):
        c = resid_case(sizes, 1024, 256, mode, cls, True)
        x_new = resid_eval(c, torch.float32)[0]
        want = ln_out_expect(x_new, c, prec)
        rows = c["gi"] >= 0
        assert not torch.equal(ln_out_expect(x_new, c, prec, "ln_out_old_x", x_old=c["x"])[rows], want[rows])
        now = [torch.rand(1024, generator=torch.Generator().manual_seed(i)) + 0.5 for i in range(len(sizes))]
        assert not torch.equal(ln_out_expect(x_new, c, prec, "ln_out_current_gamma", gas_now=now)[rows], want[rows])
        if prec == F16X2:   # the check the GPU test uses for split-half: both evaluations accepted, the mutants rejected
            v = (per_row(c["gas"], c["gi"]).double() * x_new.double())[rows]
            ext = U * v.abs()
            hi = ROUND[F16](want[rows])   # = f16(fp32 product)
            contracted = (hi.double() + ROUND[F16]((v - hi.double()).float()).double()).float()
            for name, got in (("rounded product", want[rows]), ("unrounded product", contracted)):
                assert assert_close_in(got, v, prec, 0.0, extra=ext, what=f"fp32 evaluation, ln_out from the {name}, {cls}")["slack_share"] < 0.01
            assert rejects(ln_out_expect(x_new, c, prec, "ln_out_old_x", x_old=c["x"])[rows], v, prec, 0.0, ext)
            assert rejects(ln_out_expect(x_new, c, prec, "ln_out_current_gamma", gas_now=now)[rows], v, prec, 0.0, ext)
        ref, bound = stats_ref(x_new[rows])
        n_bad, worst = stats_bad(stats_fp32_tree(x_new[rows]), ref, bound)
        print(f"[vit_gemm_ops] statistics, fp32 tree, {cls} {MODE_ID(mode)}: worst err/bound {worst:.3f}")
        assert n_bad == 0, (cls, worst)
        for mut in ("no_between_wave", "uncentred"):
            assert stats_bad(stats_fp32_tree(x_new[rows], mut), ref, bound)[0] > 0, (mut, cls)


def cons_mutant_active(mut, c):
    """qscale mutants: the identity where qscale = 1 is not reached here (no f32 fold); a second rounding shows in bf16 / f16 only."""
    return c["kind"] == QKV and (mut == "qscale_on_k" or c["prec"] in (BF16, F16))


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("mode", FOLD_MODES, ids=MODE_ID)
@pytest.mark.parametrize("kind", [QKV, FC1], ids=["qkv", "fc1"])
def test_consumer_checker_accepts_fp32_and_rejects_mutants(kind, mode, cls):
    prec = mode[0]
    c = cons_case(kind, "two", mode, cls)
    acc, (mu, rstd), cd = cons_acc(c), chan(c["parts"]), fold_vectors(c)
    valid = c["gi"] >= 0
    ref, extra = cons_eval(c, acc, mu, rstd, cd)
    got = ROUND[prec](cons_eval(c, acc.float(), mu, rstd, cd, torch.float32, pair=chan_fp32(c["parts"]))[0])
    r = assert_close_in(got[valid], ref[valid], prec, A_MFMA, extra=extra[valid], what=f"fp32 evaluation, consumer {kind} {cls}")
    assert r["slack_share"] < 0.01
    for mut in ("no_between_tile", "pair_sign"):
        bad = ROUND[prec](cons_eval(c, acc.float(), mu, rstd, cd, torch.float32, pair=chan_fp32(c["parts"], mut))[0])
        assert rejects(bad[valid], ref[valid], prec, A_MFMA, extra[valid]), (mut, cls)
    for mut in ("c_from_unrounded_w", "d_without_beta"):
        bad = ROUND[prec](cons_eval(c, acc.float(), mu, rstd, fold_vectors(c, mut=mut), torch.float32, pair=chan_fp32(c["parts"]))[0])
        rej = rejects(bad[valid], ref[valid], prec, A_MFMA, extra[valid])
        # c_from_unrounded_w: the identity on weights that are exact in the type (bf16, f16, w16), a 22-bit rounding for w32 (module docstring)
        assert rej == (mut == "d_without_beta"), (mut, cls)
        if mut == "c_from_unrounded_w" and mode != (F16X2, "w32"):
            assert torch.equal(bad, got), (mut, cls)
    if kind == QKV:
        for mut in ("qscale_after_rounding", "qscale_on_k"):
            bad = ROUND[prec](cons_eval(c, acc.float(), mu, rstd, cd, torch.float32, mut=mut, pair=chan_fp32(c["parts"]))[0].float())
            assert rejects(bad[valid], ref[valid], prec, A_MFMA, extra[valid]) == cons_mutant_active(mut, c), (mut, cls)


@pytest.mark.parametrize("mode", QKV_MODES, ids=MODE_ID)
def test_qkv_checker_accepts_fp32_and_rejects_mutants(mode):
    prec = mode[0]
    c = qkv_case("S68", mode)
    (qk, vt), (qk32, vt32) = qkv_eval(c), qkv_eval(c, torch.float32)
    valid, wrote = qkv_wrote(c)
    for r in (assert_close_in(ROUND[prec](qk32)[valid], qk[valid], prec, A_MFMA, what="fp32 evaluation, q | k"),
              assert_close_in(ROUND[prec](vt32)[wrote], vt[wrote], prec, A_MFMA, what="fp32 evaluation, V^T")):
        assert r["slack_share"] < 0.01
    assert wrote.sum() == 3 * 68 * 256 and valid.sum() == 3 * 68
    assert torch.equal(vt[..., 68:].float(), canary(*vt.shape)[..., 68:])
    assert torch.equal(vt[3].float(), canary(*vt.shape)[3]) and torch.equal(qk[3 * 68:].float(), canary(*qk.shape)[3 * 68:])   # the sequence behind the group
    for mut in ("qscale_after_rounding", "qscale_on_k"):
        active = prec != F32 and (mut == "qscale_on_k" or prec in (BF16, F16))
        assert rejects(ROUND[prec](qkv_eval(c, torch.float32, mut)[0].float())[valid], qk[valid], prec, A_MFMA) == active, mut
    for mut in ("vt_not_transposed", "vt_global_token_index"):
        assert rejects(ROUND[prec](qkv_eval(c, torch.float32, mut)[1])[wrote], vt[wrote], prec, A_MFMA), mut
    one = dict(c, out_rows=68, acc=c["acc"][:68], gi=c["gi"][:68])
    assert torch.equal(qkv_eval(one, mut="vt_global_token_index")[1], qkv_eval(one)[1])   # one sequence: the identity


@pytest.mark.parametrize("mode", PE_MODES, ids=MODE_ID)
def test_patch_embed_checker_accepts_fp32_and_rejects_mutants(mode):
    c = pe_case(mode)
    ref = pe_eval(c)
    assert assert_close_in(pe_eval(c, torch.float32), ref, F32, A_MFMA, what="fp32 evaluation, patch embed")["slack_share"] < 0.01
    S, P = PE["S"], PE["P"]
    keep = torch.ones(c["nseq"] * S, dtype=torch.bool)
    keep[(torch.arange(c["nseq"])[:, None] * S + 1 + torch.arange(P)[None]).reshape(-1)] = False
    assert torch.equal(ref[keep].float(), canary(c["nseq"] * S, PE["D"])[keep]) and keep.sum() == c["nseq"] * (S - P)
    for mut in ("rows_at_seq_s_plus_p", "pos_row_p"):
        assert rejects(pe_eval(c, torch.float32, mut), ref, F32, A_MFMA), mut


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


RECORD = {}


def record(form, mode, r):
    old = RECORD.setdefault((form, MODE_ID(mode)), [0.0, 0.0, 0])
    old[0], old[1], old[2] = max(old[0], r["worst_ratio"]), max(old[1], r["slack_share"]), old[2] + r["n"]


def record_exact(form, mode, n):
    RECORD[(form, MODE_ID(mode))] = RECORD.get((form, MODE_ID(mode)), 0) + n


@pytest.fixture(scope="module", autouse=True)
def _error_table():
    """With VIT_GEMM_OPS_ERRORS=<path> the worst error / bound per (kernel form, precision) and the slack-user share are written there."""
    yield
    path = os.environ.get("VIT_GEMM_OPS_ERRORS")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("kernel form, precision | worst error / bound over all elements | largest share of tie-slack users | elements compared\n")
            for (k, p), v in sorted(RECORD.items()):
                if isinstance(v, list):
                    f.write(f"{k:36s} {p:10s} | {v[0]:.3f} | {v[1]:.2e} | {v[2]}\n")
                else:
                    f.write(f"{k:36s} {p:10s} | bit-exact | - | {v}\n")


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def dev_groups(case, **extra):
    cu = lambda t: t.cuda().contiguous()  # noqa: E731
    out = []
    for i, (r0, n, a0) in enumerate(case["groups"]):
        g = dict(row0=r0, rows=n, arow0=a0, w=cu(case["Ws"][i]), bias=cu(case["bs"][i]))
        for k, vals in extra.items():
            g[k] = cu(vals[i])
        out.append(g)
    return out


def form():
    from burn_depth_amd import ops
    f = ops.gemm_last_form()
    return f["family"], f["ek"]


def run_resid(dev, c, mode, tile, oop=False, producer=False):
    """-> (x_new, the source buffer after the call, ln_out, stats), all on the CPU."""
    from burn_depth_amd import ops
    x = c["x"].cuda()
    x_out = (canary(*c["x"].shape) * 1.5).cuda() if oop else None
    N = c["N"]
    ln_out = canary(c["out_rows"], N).cuda() if producer else None
    stats = canary(c["out_rows"], N // 256, 2).cuda() if producer else None
    extra = dict(scale=c["lss"], gamma_next=c["gas"]) if producer else dict(scale=c["lss"])
    ops.vit_gemm(dev, RESID, c["A"].cuda(), dev_groups(c, **extra), mode[0], tile, x=x, x_out=x_out, ln_out=ln_out, ln_stats_out=stats)
    cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
    return cpu(x_out if oop else x), cpu(x), cpu(ln_out), cpu(stats)


# (e4m3 k-tiles are 128 elements: K = 64 is no fp8 launch, launch_gemm refuses it)
RESID_PARAMS = [pytest.param(s, m, id=f"M{s[0]}_N{s[1]}_K{s[2]}_tile{s[3]}-{MODE_ID(m)}") for s in RESID_SHAPES for m in MODES if not (m[0] == FP8 and s[2] % 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", RESID_PARAMS)
def test_resid_against_fp64(dev, shape, mode):
    """x_new = x + ls (A Wr^T + b), per element: one group and three groups (300, 37, 293) with the second reading the first's A rows,
    in place and out of place (the source bit-identical afterwards); canary rows between and behind the groups untouched."""
    from burn_depth_amd import _lib
    M, N, K, tile = shape
    # pick_ksplit: 16-bit operands, at most 512 tiles of 64 x 64, 2 - 4 groups that divide the k-tiles and keep five each
    KT = K * {"w": 1, "w16": 2, "w32": 3}[mode[1]] // 64
    ksplit_prec = mode[0] not in (F32, FP8) and any(KT % ks == 0 and KT // ks >= 5 for ks in (4, 3, 2))
    assert ksplit_prec or K != 1536 or mode[0] in (F32, FP8)
    for sizes in ((M,), THREE):
        c = resid_case(sizes, N, K, mode)
        ref, upd = resid_eval(c)
        quiet = c["gi"] < 0
        for oop in (False, True):
            before = _lib.load().md_gemm_ksplit_launches()
            got, src, _, _ = run_resid(dev, c, mode, tile, oop)
            split_ran = _lib.load().md_gemm_ksplit_launches() > before
            if tile != TAUTO:
                assert form() == ((ONE_TILE, EK_RMW) if tile == T256 else (-1, 0))
                assert split_ran == (ksplit_prec and tile == T64 and sum(-(-n // 64) for n in sizes) * -(-N // 64) <= 512), "k-split form"
            elif len(sizes) == 1 and _lib.load().md_gemm_pick_tile(M, N, K, mode[0]) == T64:   # DA3-small's fc2: the k-split form
                assert split_ran == ksplit_prec, "k-split form under TILE_AUTO"
            what = f"resid {MODE_ID(mode)} M{sizes} N{N} K{K} tile{tile} oop={oop}"
            if oop:
                assert bits_equal(src, c["x"]), what + ": the source changed"
                assert bits_equal(got[quiet], (canary(*c["x"].shape) * 1.5)[quiet]), what + ": canary rows of the output"
                got = torch.where(quiet[:, None], c["x"], got)
            assert bits_equal(got[quiet], c["x"][quiet]), what + ": canary rows"
            record(f"resid tile{tile}" + (" oop" if oop else ""), mode, assert_resid(got, ref, upd, what))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("mode", FOLD_MODES, ids=MODE_ID)
def test_fold_producer_against_fp64(dev, mode, cls):
    """EK_RMW_LN at N = 1024: x_new as in the resid test; ln_out bit-equal to round_T(fp32(gamma_next . x_new)) of the returned x_new; the
    (mean, M2) of every 256-column tile against fp64 statistics of the returned x_new within the summation-tree bound."""
    prec = mode[0]
    for sizes in ((293,), THREE):
        c = resid_case(sizes, 1024, 256, mode, cls, True)
        ref, upd = resid_eval(c)
        got, _, ln_out, stats = run_resid(dev, c, mode, T256, producer=True)
        assert form() == (ONE_TILE, EK_RMW_LN)
        rows, quiet = c["gi"] >= 0, c["gi"] < 0
        what = f"producer {MODE_ID(mode)} {cls} M{sizes}"
        assert bits_equal(got[quiet], c["x"][quiet]) and bits_equal(ln_out[quiet], canary(*ln_out.shape)[quiet]) and \
            bits_equal(stats[quiet], canary(*stats.shape)[quiet]), what + ": canary rows"
        record("producer x_new", mode, assert_resid(got, ref, upd, what))
        if prec == F16X2:   # lo = f16(gamma x - hi) may see the unrounded product (module docstring): half a 22-bit ulp + one fp32 rounding
            v = per_row(c["gas"], c["gi"]).double() * got.double()
            record("producer ln_out", mode, assert_close_in(ln_out[rows], v[rows], prec, 0.0, extra=U * v[rows].abs(), what=what + " ln_out"))
        else:
            want = ln_out_expect(got, c, prec)
            ne = ln_out[rows] != want[rows]
            assert not ne.any(), f"{what}: {int(ne.sum())} ln_out elements differ from round_T(fp32(gamma . x_new))"
            record_exact("producer ln_out", mode, int(rows.sum()) * 1024)
        sref, bound = stats_ref(got[rows])
        n_bad, worst = stats_bad(stats[rows], sref, bound)
        print(f"[vit_gemm_ops] {what}: statistics worst err/bound {worst:.3f}")
        record(f"producer statistics {cls}", mode, {"worst_ratio": worst, "slack_share": 0.0, "n": sref.numel()})
        assert n_bad == 0, f"{what}: {n_bad} statistics outside the bound, worst {worst:.3f}"


def run_consumer(dev, c, stats, raw, cd, tile=T256, A=None):
    """-> the fc1 output [rows, N] or (qk, vT), on the CPU."""
    from burn_depth_amd import ops
    groups = dev_groups(dict(c, bs=[v[1] for v in cd]), c=[v[0] for v in cd]) if cd is not None else dev_groups(c)
    kw = dict(ln_stats=stats.cuda().contiguous(), ln_raw=raw, ln_eps=LN_EPS, ln_inv_n=1.0 / 1024.0) if cd is not None else {}
    A = (c["A"] if A is None else A).cuda()
    if c["kind"] == FC1:
        out = canary(c["out_rows"], c["N"]).cuda()
        ops.vit_gemm(dev, FC1, A, groups, c["prec"], tile, out=out, **kw)
        return out.cpu()
    S, D = c["S"], c["D"]
    qk, vt = canary(c["out_rows"], 2 * D).cuda(), canary(c["out_rows"] // S, D // 64, 64, (S + 63) // 64 * 64).cuda()
    ops.vit_gemm(dev, QKV, A, groups, c["prec"], tile, qk=qk, vT=vt, S=S, D=D, **kw)
    return qk.cpu(), vt.cpu()


def check_consumer(dev, c, parts, acc, mu, rstd, cd, raw, what, tag, A=None, pairs=None):
    """One consumer launch per form against cons_eval: which kernel ran, the canary (rows between and behind the groups, their tokens'
    V^T columns, the key columns S .. kpad) bit for bit, the rest per element. `pairs`: the (rstd, -mu rstd) rows to hand over when not raw."""
    from burn_depth_amd import _lib
    prec, mode, valid = c["prec"], c["mode"], c["gi"] >= 0
    assert not valid[-4:].any(), "canary rows behind the last group"
    ref, extra = cons_eval(c, acc, mu, rstd, cd)
    stats = parts if raw else (pairs if pairs is not None else torch.stack([rstd, -mu * rstd], 1).float())
    if c["kind"] == FC1:
        for ds in (1, 0):
            prev = _lib.load().md_debug_gemm_direct_store(ds)
            try:
                got = run_consumer(dev, c, stats, raw, cd, A=A)
            finally:
                _lib.load().md_debug_gemm_direct_store(prev)
            assert form() == (ONE_TILE, EK_GELU_LN_DS if ds else EK_GELU_LN)
            assert bits_equal(got[~valid], canary(*got.shape)[~valid]), what + ": canary rows"
            record(f"{tag} fc1 raw{int(raw)} ds{ds}", mode, assert_close_in(got[valid], ref[valid], prec, A_MFMA, extra=extra[valid], what=f"{what} ds={ds}"))
        return
    qk, vt = run_consumer(dev, c, stats, raw, cd, A=A)
    assert form() == (ONE_TILE, EK_QKV_LN)
    qk_ref, vt_ref = split_qkv(c, ref, valid)
    qk_x, vt_x = split_qkv(c, extra, valid)
    wrote = qkv_wrote(c)[1]
    assert not wrote[-1].any() and not wrote[..., c["S"]:].any()   # the sequence behind the last group; the key columns S .. kpad
    assert bits_equal(qk[~valid], canary(*qk.shape)[~valid]) and bits_equal(vt[~wrote], canary(*vt.shape)[~wrote]), what + ": canary"
    record(f"{tag} qkv raw{int(raw)} qk", mode, assert_close_in(qk[valid], qk_ref[valid], prec, A_MFMA, extra=qk_x[valid], what=what + " q|k"))
    record(f"{tag} qkv raw{int(raw)} V^T", mode, assert_close_in(vt[wrote], vt_ref[wrote], prec, A_MFMA, extra=vt_x[wrote], what=what + " V^T"))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("mode", FOLD_MODES, ids=MODE_ID)
@pytest.mark.parametrize("kind", [QKV, FC1], ids=["qkv", "fc1"])
def test_fold_consumer_against_fp64(dev, kind, mode, cls):
    """EK_QKV_LN / EK_GELU_LN / EK_GELU_LN_DS at K = 1024, ln_raw 0 and 1, one and two groups, synthetic statistics."""
    for gkey in CONS_SIZES:
        c = cons_case(kind, gkey, mode, cls)
        acc, (mu, rstd), cd = cons_acc(c), chan(c["parts"]), fold_vectors(c)
        for raw in (False, True):
            check_consumer(dev, c, c["parts"], acc, mu, rstd, cd, raw, f"consumer {'qkv' if kind == QKV else 'fc1'} {MODE_ID(mode)} {cls} {gkey} raw={raw}", "consumer")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", QKV_MODES, ids=MODE_ID)
@pytest.mark.parametrize("name", list(QKV_CASES))
def test_plain_qkv_against_fp64(dev, name, mode):
    """EPI_QKV: q = (acc + b) qscale rounded once, k as is, V^T[seq][head][d][token]; the key columns S .. kpad keep the canary (the kernel
    stores the tokens of a sequence only; the engine zeroes them once at allocation), as do the q | k rows and the V^T block of one further
    sequence behind the group's last row (the row guard of the partial last m-tile)."""
    prec = mode[0]
    c = qkv_case(name, mode)
    qk_ref, vt_ref = qkv_eval(c)
    qk, vt = run_consumer(dev, c, None, False, None, tile=c["tile"])
    if c["tile"] == T256:
        assert form() == (ONE_TILE, EK_GENERIC if prec == F32 else EK_STORE)
    S = c["S"]
    valid, wrote = qkv_wrote(c)
    assert not valid[-S:].any() and not wrote[-1].any() and not wrote[..., S:].any()
    assert bits_equal(qk[~valid], canary(*qk.shape)[~valid]), "q | k rows of the sequence behind the group"
    assert bits_equal(vt[~wrote], canary(*vt.shape)[~wrote]), "key columns S .. kpad and the sequence behind the group"
    record(f"qkv {name} qk", mode, assert_close_in(qk[valid], qk_ref[valid], prec, A_MFMA, what=f"qkv {name} q|k"))
    record(f"qkv {name} V^T", mode, assert_close_in(vt[wrote], vt_ref[wrote], prec, A_MFMA, what=f"qkv {name} V^T"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", PE_MODES, ids=MODE_ID)
@pytest.mark.parametrize("tile", [TAUTO, T64, T256])
def test_patch_embed_against_fp64(dev, tile, mode):
    """x[seq * S + 1 + p] = A Wr^T + b + pos[1 + p]; two groups, the second on aliased A rows with its own table; rows seq * S and
    seq * S + 1 + P .. keep the canary (compared as part of the reference, whose untouched rows are the canary: tolerance 0 there)."""
    from burn_depth_amd import ops
    c = pe_case(mode)
    ref = pe_eval(c)
    x = canary(c["nseq"] * PE["S"], PE["D"]).cuda()
    ops.vit_gemm(dev, PATCH, c["A"].cuda(), dev_groups(c, pos=c["poss"]), mode[0], tile, x=x, S=PE["S"], P=PE["P"])
    assert form() == ((ONE_TILE, EK_GENERIC) if tile == T256 else (-1, 0))   # (99 rows: TILE_AUTO never takes the 256-row tile)
    x = x.cpu()
    keep = ref.float() == canary(*x.shape)
    assert bits_equal(x[keep], canary(*x.shape)[keep]), "rows outside the patches"
    record(f"patch_embed tile{tile}", mode, assert_close_in(x, ref, F32, A_MFMA, what=f"patch_embed {MODE_ID(mode)} tile{tile}"))


@pytest.mark.gpu
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("mode", [(BF16, "w"), (F16X2, "w16"), (F16X2, "w32")], ids=MODE_ID)
def test_producer_then_consumer_chain(dev, mode, cls):
    """proj-like producer -> (ln_finish | raw partials) -> fc1 and qkv consumers on the producer's own ln_out and statistics array, against
    fp64 LN(x_new) Wr^T + b of the returned x_new: pins the layout of the statistics between the two launches. Every consumer launch goes
    through check_consumer: kernel kind, canary rows, q | k, V^T and both fc1 store forms."""
    from burn_depth_amd import ops
    p = resid_case(CONS_SIZES["two"], 1024, 256, mode, cls, True)
    x_new, _, ln_out, stats = run_resid(dev, p, mode, T256, producer=True)
    assert form() == (ONE_TILE, EK_RMW_LN)
    prow = p["gi"] >= 0
    assert bits_equal(x_new[~prow], p["x"][~prow]) and bits_equal(stats[~prow], canary(*stats.shape)[~prow]), "producer canary rows"
    zt = x_new[prow].double()
    mu = zt.mean(1)
    rstd = 1.0 / torch.sqrt(((zt - mu[:, None]) ** 2).mean(1) + LN_EPS)
    finished = ops.ln_finish(dev, stats[prow].cuda(), 1.0 / 1024.0, LN_EPS).cpu()
    for kind in (FC1, QKV):
        c = dict(cons_case(kind, "two", mode, cls), gams=p["gas"])   # c of each group from that group's gamma_next
        valid = c["gi"] >= 0
        A = ln_out[prow]
        full = lambda v, fill: torch.full((c["out_rows"],), fill, dtype=torch.float64).index_put((valid.nonzero()[:, 0],), v)  # noqa: E731
        parts, pairs = canary(c["out_rows"], 4, 2), canary(c["out_rows"], 2)
        parts[valid], pairs[valid] = stats[prow], finished
        for raw in (True, False):
            check_consumer(dev, c, parts, cons_acc(c, A), full(mu, 0.0), full(rstd, 1.0), fold_vectors(c), raw,
                           f"chain {MODE_ID(mode)} {cls} {'fc1' if kind == FC1 else 'qkv'} raw={raw}", "chain", A=A, pairs=pairs)


# ---- tile loops: bit identity with the one-tile kernel (which the tests above hold to fp64) ----
def loop_pair(run, loop_family, one_tile_ek, fold):
    """run() under persist masks 15 and 0 -> the two result lists; asserts which kernel ran."""
    from burn_depth_amd import _lib, ops
    lib = _lib.load()
    prev = lib.md_debug_gemm_persistent(15)
    try:
        a = run()
        f = ops.gemm_last_form()
        assert (f["family"], f["fold"]) == (loop_family, int(fold)), f
        lib.md_debug_gemm_persistent(0)
        b = run()
        f0 = ops.gemm_last_form()
        assert (f0["family"], f0["ek"]) == (ONE_TILE, one_tile_ek) and f0["blocks"] == f["blocks"], f0
    finally:
        lib.md_debug_gemm_persistent(prev)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), "tile loop and one-tile kernel differ"
    return f


def loop_resid_inputs(M, N, K, mode):
    g = torch.Generator(device="cuda").manual_seed(M + K)
    rnd = (lambda t: t.bfloat16().float()) if mode[0] == BF16 else (lambda t: t.half().float())
    A = rnd(torch.randn(M, K, device="cuda", generator=g))
    W = rnd(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5)
    vec = lambda s: torch.randn(N, device="cuda", generator=g) * s  # noqa: E731
    return A, W, vec(1.0), vec(1.0), torch.rand(N, device="cuda", generator=g) + 0.5, torch.randn(M + 3, N, device="cuda", generator=g) * 3 + 0.5


def run_loop_resid(dev, inp, mode, producer, M):
    from burn_depth_amd import ops
    A, W, b, ls, gam, x0 = inp
    N = W.shape[0]

    def run():
        x = x0.clone()
        ln_out = torch.full((M + 3, N), 0.75, device="cuda") if producer else None
        stats = torch.full((M + 3, N // 256, 2), 0.75, device="cuda") if producer else None
        grp = dict(row0=0, rows=M, arow0=0, w=W, bias=b, scale=ls)
        if producer:
            grp["gamma_next"] = gam
        ops.vit_gemm(dev, RESID, A, [grp], mode[0], T256, x=x, ln_out=ln_out, ln_stats_out=stats)
        assert torch.equal(x[M:], x0[M:])
        return [x] + ([ln_out, stats] if producer else [])
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("producer", [False, True], ids=["rmw", "rmw_ln"])
@pytest.mark.parametrize("mode", [(BF16, "w"), (F16X2, "w16")], ids=MODE_ID)
def test_resid_tile_loop_bit_identical_to_one_tile(dev, mode, producer):
    """gemm256r_kernel against gemm256_kernel<EK_RMW / EK_RMW_LN> at M = 256 * 256 + 100, N = K = 1024: 1028 tiles."""
    M = 256 * 256 + 100
    inp = loop_resid_inputs(M, 1024, 1024, mode)
    f = loop_pair(run_loop_resid(dev, inp, mode, producer, M), LOOP_R, EK_RMW_LN if producer else EK_RMW, producer)
    assert f["blocks"] == 1028
    record_exact("loop resid" + (" + producer" if producer else ""), mode, M * 1024)


@pytest.mark.gpu
def test_resid_tile_loop_k4096_and_stagger(dev):
    """bf16: 64 k-tiles per tile, which selects the fc2 stagger slot -- but gemm256_form applies a start offset only from 2048 tiles, so at
    these 1028 tiles the slot is chosen and never takes effect (and its default is 0); then 2052 tiles of 16 k-tiles with the start offset
    of the proj slot at the value found (restored afterwards) and at 0."""
    from burn_depth_amd import _lib
    mode = (BF16, "w")
    M = 256 * 256 + 100
    loop_pair(run_loop_resid(dev, loop_resid_inputs(M, 1024, 4096, mode), mode, False, M), LOOP_R, EK_RMW, False)
    record_exact("loop resid K4096", mode, M * 1024)
    M = 512 * 256 + 100
    run = run_loop_resid(dev, loop_resid_inputs(M, 1024, 1024, mode), mode, True, M)
    f = loop_pair(run, LOOP_R, EK_RMW_LN, True)
    assert f["blocks"] == 2052
    lib = _lib.load()
    before = lib.md_debug_gemm_stagger_ticks(0)
    assert before > 0 and f["blocks"] >= 2048 and lib.md_debug_gemm_stagger_ticks(4) < 0   # (the default offset was in effect above)
    try:
        assert lib.md_debug_gemm_stagger(0, 0) == 0 and lib.md_debug_gemm_stagger_ticks(0) == 0
        f0 = loop_pair(run, LOOP_R, EK_RMW_LN, True)
    finally:
        lib.md_debug_gemm_stagger(0, before)
    assert lib.md_debug_gemm_stagger_ticks(0) == before
    assert f0["blocks"] == 2052
    record_exact("loop resid 2052 tiles both staggers", mode, 2 * M * 1024)


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "raw_fold"])
@pytest.mark.parametrize("mode", [(BF16, "w"), (F16, "w")], ids=MODE_ID)
def test_qkv_tile_loop_bit_identical_to_one_tile(dev, mode, fold):
    """The QKV form of gemm256p_kernel against gemm256_kernel<EK_STORE / EK_QKV_LN> at T = 29, S = 580, D = 1024: 66 x 12 = 792 tiles."""
    from burn_depth_amd import ops
    T, S, D, K = 29, 580, 1024, 1024
    rows = T * S
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = (lambda t: t.bfloat16().float()) if mode[0] == BF16 else (lambda t: t.half().float())
    A = rnd(torch.randn(rows, K, device="cuda", generator=g))
    W = rnd(torch.randn(3 * D, K, device="cuda", generator=g) / K ** 0.5)
    b, cvec = torch.randn(3 * D, device="cuda", generator=g), torch.randn(3 * D, device="cuda", generator=g)
    parts = torch.stack([torch.randn(rows + S, 4, device="cuda", generator=g), torch.rand(rows + S, 4, device="cuda", generator=g) * 2000 + 500], -1).contiguous()

    def run():
        qk = torch.full((rows + S, 2 * D), 0.75, device="cuda")          # one more sequence behind the group's last row
        vt = torch.full((T + 1, D // 64, 64, (S + 63) // 64 * 64), 0.75, device="cuda")
        grp = dict(row0=0, rows=rows, arow0=0, w=W, bias=b)
        kw = {}
        if fold:
            grp["c"] = cvec
            kw = dict(ln_stats=parts, ln_raw=True, ln_eps=LN_EPS, ln_inv_n=1.0 / 1024.0)
        ops.vit_gemm(dev, QKV, A, [grp], mode[0], T256, qk=qk, vT=vt, S=S, D=D, **kw)
        assert bool((vt[..., S:] == 0.75).all()) and bool((vt[T] == 0.75).all()) and bool((qk[rows:] == 0.75).all())
        return [qk, vt]
    f = loop_pair(run, LOOP_P, EK_QKV_LN if fold else EK_STORE, fold)
    assert f["blocks"] == 792 and f["qkv"] == 1
    record_exact("loop qkv" + (" + raw fold" if fold else ""), mode, rows * 3 * D)


@pytest.mark.gpu
def test_vit_gemm_argument_checks(dev):
    from burn_depth_amd import _lib, ops
    c = resid_case((293,), 1024, 256, (BF16, "w"), "plain", True)
    x = c["x"].cuda()
    grp = dev_groups(c, scale=c["lss"], gamma_next=c["gas"])
    with pytest.raises(_lib.MdError) as e:     # the fold lives in the 256 x 256 kernel only: never silently dropped
        ops.vit_gemm(dev, RESID, c["A"].cuda(), grp, BF16, T64, x=x, ln_out=x.clone(), ln_stats_out=canary(c["out_rows"], 4, 2).cuda())
    assert e.value.code == _lib.MD_ERR_UNSUPPORTED
    grp[0]["rows"] = c["out_rows"] + 1         # rows past the buffers
    with pytest.raises(_lib.MdError) as e:
        ops.vit_gemm(dev, RESID, c["A"].cuda(), grp, BF16, T256, x=x)
    assert e.value.code == _lib.MD_ERR_SHAPE
    assert bits_equal(x.cpu(), c["x"])
