"""Operator tests of the GEMM forms the engines launch for the convolutional decoders and heads, through `ops.decoder_gemm`
(md_op_decoder_gemm): the 3 x 3 convolution with residual inputs and a relu'd second output (EPI_STORE; one and two weight groups, the
shared input / residual with res_mod = M, the per-image residual table res_mod = P), the stride-2 convolution (T-typed and the fp32 +
ReLU form), the pixel shuffle into a channel slice (f = 2 | 4, fast and general form, second output), the head tails (EPI_HEAD with one
channel and with head_nch channels, EPI_HEAD_UP2) and the residual convolution's tile loop against the one-tile kernel bit for bit.
References are torch fp64 from each operation's definition (F.conv2d, F.conv_transpose2d, relu, sums, a dot with the head weights) on
operands that are exact in the operand type (`close_check.ROUND`); every output buffer is the caller's and filled with a canary, and what
a launch must leave alone (pad columns Cout .. ld, the columns outside [ps_coff, ps_coff + Cout), rows behind M, the planes of a
head_bstride layout that belong to no channel of the launch) has to come back bit for bit; inputs and residuals are compared bit for bit
afterwards. `ops.gemm_last_form()` says which kernel, tile and pixel-shuffle form ran.

Where the bounds come from (u = 2^-24; none is taken from a GPU result; the CPU tests evaluate every reference formula in fp32, summed
tap by tap as the kernels' k-loop walks the taps, and must pass; they reject the mutants of `MUTANT_ACTIVE`):

* EPI_STORE / EPI_PIXSHUF (gemm_impl.h epilogue4 and its 256 x 256 specialisations): v = acc + bias (+ res1 + res2), act, ONE rounding to
  T. 0.5 ulp_T with tie slack + A_MFMA max|acc + bias| (accumulation order of exact products behind the MFMA). The residuals are values
  exact in T added in fp32: each addition rounds once, u |partial sum| -- the extra term u (|pre + res1| + |pre + res1 + res2|). relu is
  exact. The fp32 store of the stride-2 form has no ulp_T term.
* out2 = relu(out) as VALUES, tolerance 0: the kernel stores round_T(relu(v)) beside round_T(v), rounding is monotone and keeps the sign,
  so round_T(relu(v)) == relu(round_T(v)); `torch.equal` (-0 == 0).
* heads (fp32 outputs). gemm_impl.h (the EPI_HEAD branch of gemm_kernel: `rl = fmaxf(acc + bv, 0.f)`, `part += rl * hw`) keeps the relu
  map in fp32 -- it is NOT rounded to T before the dot product, so no ulp_T(map) term exists. Pre-activation z_c = w_c . relu(conv + b1)
  + b_c: d = A_MFMA max|conv + b1| sum|w_c| (relu is 1-Lipschitz) + 12 u sum_j |w_cj| relu_j (the dot: 8 products summed in a lane, two
  cross-lane additions, the bias: at most 11 roundings of partial sums bounded by sum|w| relu, + the products') . acts 0 and 2: d.
  acts 1 and 3: |exp z| expm1(d) + the device expf error + (act 3) u |out| for the + 1. expf: 1 ulp = 2 u |exp z|, the figure of the HIP
  math API's accuracy table for expf; that document is not part of the ROCm tree this suite runs against, so the figure is quoted, not
  read from a file here. Pre-activations stay within +-4.
* EPI_HEAD_UP2: the reference is the definition (conv_transpose2d -> conv2d -> relu -> dot -> relu). The engine composes the two
  convolutions' weights in fp32 at commit and ROUNDS the product to the operand type (compose_head_kernel -> pack_kernel, md_engine.hip):
  a derived term per pre-activation p = conv(x, Wc) + bias9[class]: conv(|x|, 0.5 ulp_T |Wc|) for the operand rounding (ulp of the 22-bit
  split-half value for f16x2, none for f32) + 4 Cmid u conv(|x|, |W1| . |Wd|) for the fp32 sums of at most 4 Cmid products per composed
  weight + (9 Cmid + 1) u (max|b1| + max_co sum|W1| |bd|) for a bias class (compose_head_bias_kernel: b1 and at most 9 Cmid products in one
  fp32 chain) + A_MFMA (max conv(|x|, |Wc|) + max|bias9|), the last bracket being an upper bound of max|acc + bias|. These times sum|w|,
  plus the dot as in EPI_HEAD, 12 u (sum_c |w_c| relu(p_c) + |b|) with the relu map of the fp64 definition. The last relu is exact.

What cannot be told apart here: `res_after_act` is the identity without an activation or without residuals, `res1_row_m` without a wrap
(one group, no table), `f4_nested` at f = 2, `ps_coff_ignored` at ps_coff = 0, `img_dropped` needs B > 1 (all B >= 2 here),
`neighbour_act_bias` with one channel. `MUTANT_ACTIVE(mut, case)` states this per case and the CPU tests assert both directions through it.
The issue's list names the residual / activation order mutant in both directions; EPI_STORE has ONE definition, out = act(acc + bias +
res1 + res2) (gemm_impl.h epilogue4: the residual loads stand before `if (p.act == ACT_RELU)`), so only `res_after_act` (relu first, then
the residuals) is a mutant of it -- its reverse is the definition itself. The order of the nine
taps inside the k-loop and the k-split of the 64 x 64 kernel change last bits only (inside A_MFMA): no test here tells them apart, the
bit-identity tests of tests/test_gpu_parity.py pin them."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import close_check
from close_check import A_MFMA, BF16, F16, F16X2, F32, FP8, PNAME, ROUND, SIG_BITS, rejects, ulp_T

assert_close_in = functools.partial(close_check.assert_close_in, tag="decoder_gemm_ops")
CONV3, CONV3_S2, PIXSHUF, HEAD, HEAD_UP2 = range(5)
T256, T128, T256x32, T128x64, T64, TAUTO = 0, 1, 2, 3, 4, 99
EK_GENERIC, EK_STORE, EK_PIXSHUF = 0, 2, 3
ONE_TILE, LOOP_P, LOOP_R = 0, 1, 2
U = 2.0 ** -24
EXPF_ULPS = 1.0   # HIP math API accuracy table, expf (module docstring)
MODES = [(BF16, "w"), (F16, "w"), (F16X2, "w16"), (F16X2, "w32"), (F32, "w")]
MODE_ID = lambda m: PNAME[m[0]] + ("" if m[1] == "w" else "_" + m[1])  # noqa: E731


def canary(*shape):
    """Values exact in every storage type (multiples of 1/4 below 32), no two neighbours equal."""
    n = math.prod(shape)
    return ((torch.arange(n) % 97 + 3).float() * 0.25).reshape(shape)


def round_w(W, mode):
    """A master weight that is exact in the device's operand: f16 values for w16 (two terms), 22-bit hi + lo values for w32 (three)."""
    return ROUND[F16](W) if mode[1] == "w16" else ROUND[mode[0]](W)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows_of(t):
    """[n, C, H, W] -> NHWC rows [n H W, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_gather(x, Wt, stride=1, mut=None, dtype=torch.float32):
    """3 x 3, pad 1 convolution summed tap by tap in `dtype` -> rows [n OH OW, Co]. Mutants: `halo_neighbour` (an out-of-image tap reads the
    flat neighbour pixel -- the next row / image -- instead of the zero page), `s2_shift` (taps at +0 .. +2 instead of -1 .. +1)."""
    n, Cn, H, W = x.shape
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    flat = torch.cat([rows_of(x).to(dtype), torch.zeros(1, Cn, dtype=dtype)])
    img, oy, ox = torch.arange(n)[:, None, None], torch.arange(OH)[None, :, None], torch.arange(OW)[None, None, :]
    acc = torch.zeros(n * OH * OW, Wt.shape[0], dtype=dtype)
    sh = 0 if mut == "s2_shift" else -1
    for dy in range(3):
        for dx in range(3):
            yy, xx = oy * stride + dy + sh, ox * stride + dx + sh
            idx = ((img * H + yy) * W + xx).expand(n, OH, OW)
            ok = (idx >= 0) & (idx < n * H * W) if mut == "halo_neighbour" else ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).expand(n, OH, OW)
            acc += flat[torch.where(ok, idx, torch.full_like(idx, n * H * W)).reshape(-1)] @ Wt[:, :, dy, dx].to(dtype).t()
    return acc


def act_of(kind, z):
    return torch.relu(z) if kind == 0 else (torch.exp(z) if kind == 1 else (z if kind == 2 else torch.exp(z) + 1.0))


# ---------------------------------------------------------------------------------------------
# 3 x 3 convolution, stride 1 | 2: out = act(conv + bias + res1[m % res_mod] + res2), out2 = relu(out)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def conv_case(B, H, W, Cin, Cout, mode, G=1, shared=False, res=0, table=False, act=0, out2=False, stride=1, bias=True):
    """res: number of residual inputs; table: res1 is a per-image table (res_mod = P < M). shared: both groups read group 0's input / res1."""
    prec = mode[0]
    g = gen(B * 1000 + H * 37 + W + Cin + Cout + prec + G + res + stride)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * OH * OW
    x = ROUND[prec](torch.randn((1 if shared else G) * B, Cin, H, W, generator=g))
    Ws = [round_w(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, mode) for _ in range(G)]
    bs = [torch.randn(Cout, generator=g) if bias else None for _ in range(G)]
    res_mod = OH * OW if table else (M if (shared and G > 1 and res) else 0)
    r1 = ROUND[prec](torch.randn(res_mod or G * M, Cout, generator=g)) if res >= 1 else None
    r1_beyond = ROUND[prec](torch.randn(G * M, Cout, generator=g)) if res >= 1 else None   # what a launch that forgets the wrap would read
    if r1 is not None:
        r1_beyond[:r1.shape[0]] = r1
    r2 = ROUND[prec](torch.randn(G * M, Cout, generator=g)) if res >= 2 else None
    return dict(B=B, H=H, W=W, OH=OH, OW=OW, M=M, Cin=Cin, Cout=Cout, mode=mode, prec=prec, G=G, shared=shared, x=x, Ws=Ws, bs=bs, res_mod=res_mod, r1=r1,
                r1_beyond=r1_beyond, r2=r2, act=act, out2=out2, stride=stride)


def conv_eval(c, dtype=torch.float64, mut=None):
    """-> (out rows [G M, Cout], out2 rows, pre = acc + bias, the residual additions' partial sums |s1| + |s2|)."""
    G, B, M, s = c["G"], c["B"], c["M"], c["stride"]
    pre = []
    for g in range(G):
        xg = c["x"][:B] if c["shared"] else c["x"][g * B:(g + 1) * B]
        if dtype == torch.float64 and mut is None:
            acc = rows_of(F.conv2d(xg.double(), c["Ws"][g].double(), padding=1, stride=s))
        else:
            acc = conv_gather(xg, c["Ws"][g], s, mut, dtype)
        pre.append(acc + (c["bs"][g].to(dtype) if c["bs"][g] is not None else 0.0))
    pre = torch.cat(pre)
    m = torch.arange(G * M)
    v, sums = pre, torch.zeros_like(pre)
    relu_first = mut == "res_after_act" and c["act"] == 1
    if relu_first:
        v = torch.relu(v)
    if c["r1"] is not None:
        r1 = c["r1_beyond"][m] if mut == "res1_row_m" else c["r1"][m % c["res_mod"] if c["res_mod"] else m]
        v = v + r1.to(dtype)
        sums = sums + v.abs()
    if c["r2"] is not None and mut != "res2_dropped":
        v = v + c["r2"].to(dtype)
        sums = sums + v.abs()
    if c["act"] == 1 and not relu_first:
        v = torch.relu(v)
    out2 = torch.relu(pre if mut == "out2_pre_residual" else v) if c["out2"] else None
    return v, out2, pre, sums


def store_bad(got, ref, pre, sums, prec):
    a32 = A_MFMA * pre.abs().max().item() / max(ref.abs().max().item(), 1e-300)
    return rejects(got, ref, prec, a32, U * sums.double())


def store_assert(got, ref, pre, sums, prec, what):
    a32 = A_MFMA * pre.abs().max().item() / max(ref.abs().max().item(), 1e-300)
    return assert_close_in(got, ref, prec, a32, extra=U * sums.double(), what=what)


MUTANTS = {  # mutant -> is it something else than the identity on case c (a conv / ps / head / up2 case dict)?
    "res2_dropped": lambda c: c["r2"] is not None,                                                        # a second residual input
    "res1_row_m": lambda c: c["r1"] is not None and 0 < c["res_mod"] < c["G"] * c["M"],                    # a wrap below the launch's rows
    "res_after_act": lambda c: c["act"] == 1 and c["r1"] is not None,                                     # ACT_RELU with residual inputs
    "out2_pre_residual": lambda c: bool(c["out2"]) and c["r1"] is not None,                               # a second output with residual inputs
    "halo_neighbour": lambda c: True,
    "s2_shift": lambda c: c["stride"] == 2,
    "dydx_swapped": lambda c: True,
    "f4_nested": lambda c: c["f"] == 4,
    "ps_coff_ignored": lambda c: c["coff"] > 0,
    "parity_transposed": lambda c: True,
    "neighbour_act_bias": lambda c: len(c["acts"]) > 1,                                                   # more than one channel
    "img_dropped": lambda c: c["B"] > 1,
}


def MUTANT_ACTIVE(mut, c):
    return MUTANTS[mut](c)


CONV_CPU_CASES = {
    "unit2": dict(B=2, H=13, W=11, Cin=64, Cout=64, G=2, shared=True, res=2, out2=True),
    "table": dict(B=3, H=5, W=7, Cin=64, Cout=32, res=1, table=True, act=1, out2=True),
    "border": dict(B=1, H=2, W=2, Cin=64, Cout=32, res=2, out2=True),
    "s2_odd": dict(B=2, H=13, W=11, Cin=64, Cout=64, stride=2),
    "s2_even": dict(B=2, H=12, W=10, Cin=64, Cout=64, stride=2),
}


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("name", list(CONV_CPU_CASES))
def test_conv_checker_accepts_fp32_and_rejects_mutants(name, mode):
    c = conv_case(mode=mode, **CONV_CPU_CASES[name])
    prec = c["prec"]
    ref, ref2, pre, sums = conv_eval(c)
    got, got2, _, _ = conv_eval(c, torch.float32)
    assert store_assert(ROUND[prec](got), ref, pre, sums, prec, f"fp32 evaluation, conv {name}")["slack_share"] < 0.01
    if ref2 is not None:
        assert torch.equal(ROUND[prec](got2), torch.relu(ROUND[prec](got)))   # the out2 rule of the module docstring on the fp32 evaluation
    muts = ["res2_dropped", "res1_row_m", "res_after_act", "out2_pre_residual", "halo_neighbour"] + (["s2_shift"] if c["stride"] == 2 else [])
    for mut in muts:
        bad, bad2, _, _ = conv_eval(c, torch.float32, mut)
        rej = store_bad(ROUND[prec](bad), ref, pre, sums, prec)
        if mut == "out2_pre_residual":
            rej = bool(c["out2"]) and not torch.equal(ROUND[prec](bad2), torch.relu(ROUND[prec](bad)))
        assert rej == MUTANT_ACTIVE(mut, c), (mut, name)


# ---------------------------------------------------------------------------------------------
# pixel shuffle: ConvTranspose2d k = s = f into channels [coff, coff + Cout) of pixels of ldo
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def ps_case(B, H, W, Cin, Cout, mode, f=2, coff=0, pad=0, out2=False):
    prec = mode[0]
    g = gen(B + H * 31 + W + Cin + Cout + prec + f + coff)
    x = ROUND[prec](torch.randn(B, Cin, H, W, generator=g))
    Wt = round_w(torch.randn(Cin, Cout, f, f, generator=g) / Cin ** 0.5, mode)
    b = torch.randn(Cout, generator=g)
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, mode=mode, prec=prec, f=f, coff=coff, ldo=coff + Cout + pad, x=x, Wt=Wt, b=b, out2=out2)


def ps_eval(c, dtype=torch.float64, mut=None):
    """-> (out [B, fH, fW, ldo] with the canary where the launch writes nothing, the written mask, pre)."""
    B, H, W, f, Cout, coff = c["B"], c["H"], c["W"], c["f"], c["Cout"], c["coff"]
    out = canary(B, f * H, f * W, c["ldo"]).to(dtype)
    wrote = torch.zeros(out.shape, dtype=torch.bool)
    col = 0 if mut == "ps_coff_ignored" else coff
    if dtype == torch.float64 and mut is None:
        y = F.conv_transpose2d(c["x"].double(), c["Wt"].double(), c["b"].double(), stride=f).permute(0, 2, 3, 1)
        out[..., col:col + Cout] = y
    else:
        xr = c["x"].permute(0, 2, 3, 1).to(dtype)
        for t in range(f * f):   # GEMM column block t = ky * f + kx of the packed weight
            ky, kx = divmod(t, f)
            dy, dx = ky, kx
            if mut == "dydx_swapped":
                dy, dx = kx, ky
            if mut == "f4_nested" and f == 4:   # t read as (dy1, dx1, dy2, dx2): two nested f = 2 shuffles
                dy, dx = 2 * (t >> 3) + ((t >> 1) & 1), 2 * ((t >> 2) & 1) + (t & 1)
            out[:, dy::f, dx::f, col:col + Cout] = xr @ c["Wt"][:, :, ky, kx].to(dtype) + c["b"].to(dtype)
    wrote[..., col:col + Cout] = True
    return out, wrote, out[..., col:col + Cout]


def ps_bad(got, c, ref, wrote, pre):
    quiet = ~wrote
    if not torch.equal(got[quiet].float(), canary(*got.shape)[quiet]):
        return True
    return rejects(got[wrote], ref[wrote], c["prec"], A_MFMA * pre.abs().max().item() / ref[wrote].abs().max().item())


PS_CPU_CASES = {"f2": dict(B=2, H=5, W=7, Cin=64, Cout=32, f=2, coff=0), "f4_slice": dict(B=2, H=5, W=7, Cin=64, Cout=32, f=4, coff=72, pad=56),
                "f2_slice": dict(B=2, H=12, W=10, Cin=64, Cout=64, f=2, coff=64, pad=0, out2=True)}


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("name", list(PS_CPU_CASES))
def test_pixel_shuffle_checker_accepts_fp32_and_rejects_mutants(name, mode):
    c = ps_case(mode=mode, **PS_CPU_CASES[name])
    ref, wrote, pre = ps_eval(c)
    got = ROUND[c["prec"]](ps_eval(c, torch.float32)[0])
    assert not ps_bad(got, c, ref, wrote, pre), name
    assert wrote.sum() == c["B"] * c["f"] ** 2 * c["H"] * c["W"] * c["Cout"]
    for mut in ("dydx_swapped", "f4_nested", "ps_coff_ignored"):
        bad = ROUND[c["prec"]](ps_eval(c, torch.float32, mut)[0])
        assert ps_bad(bad, c, ref, wrote, pre) == MUTANT_ACTIVE(mut, c), (mut, name)


# ---------------------------------------------------------------------------------------------
# head tails
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def head_case(B, H, W, Cin, mode, acts=(), big_stride=True):
    """acts = (): the one-channel form (relu). Else channel i has acts[i]; planes live in one [B, nch + 1, H W] tensor (big_stride: bstride =
    (nch + 1) H W, the last plane belongs to no channel) or in a tensor [B, H W] per channel (bstride = the plane)."""
    prec = mode[0]
    g = gen(B + H * 29 + W + Cin + prec + len(acts))
    x = ROUND[prec](torch.randn(B, Cin, H, W, generator=g))
    W1 = round_w(torch.randn(32, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, mode)
    b1 = torch.randn(32, generator=g) * 0.5
    n = max(len(acts), 1)
    wc = torch.randn(n, 32, generator=g) * 0.35   # relu(N(0, 1.1)) . w: pre-activations of about +-1.5, inside +-4
    bc = torch.randn(n, generator=g) * 0.3
    return dict(B=B, H=H, W=W, Cin=Cin, mode=mode, prec=prec, acts=tuple(acts), big_stride=big_stride, x=x, W1=W1, b1=b1, wc=wc, bc=bc)


def head_eval(c, dtype=torch.float64, mut=None):
    """-> (planes [B, nch (+ 1), H W] with the canary where nothing is written, written mask, bound d-derived per element)."""
    B, HW, acts = c["B"], c["H"] * c["W"], c["acts"] or (0,)
    n = len(acts)
    if dtype == torch.float64:
        pre1 = rows_of(F.conv2d(c["x"].double(), c["W1"].double(), c["b1"].double(), padding=1))
    else:
        pre1 = conv_gather(c["x"], c["W1"], 1, None, dtype) + c["b1"].to(dtype)
    rl = torch.relu(pre1)
    planes = canary(B, n + 1, HW).to(dtype)
    wrote = torch.zeros(planes.shape, dtype=torch.bool)
    bound = torch.zeros(planes.shape, dtype=torch.float64)
    for i in range(n):
        j = (i + 1) % n if mut == "neighbour_act_bias" else i
        z = rl @ c["wc"][i].to(dtype) + c["bc"][j].to(dtype)
        o = act_of(acts[j], z).reshape(B, HW)
        d = A_MFMA * pre1.abs().max().double() * c["wc"][i].abs().sum().double() + 12 * U * (rl.double() @ c["wc"][i].abs().double())
        e = d if acts[i] in (0, 2) else o.reshape(-1).abs().double() * (torch.expm1(d) + 2 * U * EXPF_ULPS + U)
        if mut == "img_dropped":
            planes[0, i], wrote[0, i] = o[B - 1], True   # every image lands on image 0's plane: the last one stays
        else:
            planes[:, i], wrote[:, i] = o, True
        bound[:, i] = e.reshape(B, HW)
    return planes, wrote, bound


def head_bad(got, ref, wrote, bound):
    if not torch.equal(got[~wrote].float(), canary(*got.shape)[~wrote]) or not torch.isfinite(got).all():
        return True
    return bool(((got.double() - ref)[wrote].abs() > bound[wrote]).any())


def head_assert(got, ref, wrote, bound, what):
    assert torch.isfinite(got).all(), what
    assert torch.equal(got[~wrote].float(), canary(*got.shape)[~wrote]), what + ": planes / rows the launch does not own"
    ratio = ((got.double() - ref)[wrote].abs() / bound[wrote]).max().item()
    print(f"[decoder_gemm_ops] {what}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: worst err/bound {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("acts", [(), (1, 3), (2, 2, 2, 2, 2, 2, 3), (0, 1, 2, 3)], ids=["one", "depth_conf", "rays_conf", "all_acts"])
def test_head_checker_accepts_fp32_and_rejects_mutants(acts, mode):
    c = head_case(2, 6, 5, 64, mode, acts)
    ref, wrote, bound = head_eval(c)
    assert ref[wrote].abs().max() < 60 and not wrote[:, -1].any()
    assert not head_bad(head_eval(c, torch.float32)[0], ref, wrote, bound)
    for mut in ("neighbour_act_bias", "img_dropped"):
        assert head_bad(head_eval(c, torch.float32, mut)[0], ref, wrote, bound) == MUTANT_ACTIVE(mut, c), (mut, acts)


def compose_head(Wd, W1):
    """The composed 3 x 3 weight [4 Co, Cin, 3, 3] of deconv k2s2 [Cin, Cmid, 2, 2] -> conv 3 x 3 [Co, Cmid, 3, 3] on the deconvolution's input
    grid, column group q = 2 py + px = output parity: from the two definitions -- output pixel (2y + py, 2x + px) reads deconvolution pixels
    (2y + py + u - 1, ..), i.e. input pixel y + a, a = floor((py + u - 1) / 2), through deconvolution tap (py + u - 1) & 1."""
    Cin, Co = Wd.shape[0], W1.shape[0]
    out = torch.zeros(4, Co, Cin, 3, 3, dtype=Wd.dtype)
    for py in range(2):
        for px in range(2):
            for u in range(3):
                a, dy = (py + u + 1) // 2 - 1, (py + u + 1) & 1
                for v in range(3):
                    b, dx = (px + v + 1) // 2 - 1, (px + v + 1) & 1
                    out[2 * py + px, :, :, a + 1, b + 1] += torch.einsum("om,im->oi", W1[:, :, u, v], Wd[:, :, dy, dx])
    return out.reshape(4 * Co, Cin, 3, 3)


def compose_bias9(W1, bd, b1):
    out = torch.zeros(3, 3, W1.shape[0], dtype=W1.dtype)
    for ry in range(3):
        for rx in range(3):
            us = [u for u in range(3) if not ((ry == 0 and u == 0) or (ry == 2 and u == 2))]
            vs = [v for v in range(3) if not ((rx == 0 and v == 0) or (rx == 2 and v == 2))]
            out[ry, rx] = b1 + torch.einsum("omuv,m->o", W1[:, :, us][:, :, :, vs], bd)
    return out


@functools.lru_cache(maxsize=8)
def up2_case(B, H, W, Cin, Cmid, mode):
    prec = mode[0]
    g = gen(B + H * 23 + W + Cin + Cmid + prec)
    x = ROUND[prec](torch.randn(B, Cin, H, W, generator=g))
    Wd = torch.randn(Cin, Cmid, 2, 2, generator=g) / Cin ** 0.5
    bd = torch.randn(Cmid, generator=g) * 0.3
    W1 = torch.randn(32, Cmid, 3, 3, generator=g) / (9 * Cmid) ** 0.5
    b1 = torch.randn(32, generator=g) * 0.3
    return dict(B=B, H=H, W=W, Cin=Cin, Cmid=Cmid, mode=mode, prec=prec, x=x, Wd=Wd, bd=bd, W1=W1, b1=b1, w=torch.randn(32, generator=g) * 0.35,
                b=float(torch.randn(1, generator=g) * 0.3))


def up2_eval(c, dtype=torch.float64, mut=None):
    """-> (out [B, 2H, 2W], bound). fp64: the definition. Else the composed form as the engine runs it: the fp32 weight product rounded to T,
    one 3 x 3 convolution to 4 x 32 columns, the bias class of the output pixel, relu, dot, relu, parity group q -> pixel (2y + py, 2x + px)."""
    B, H, W, prec = c["B"], c["H"], c["W"], c["prec"]
    x64 = c["x"].double()
    Wc64, Wabs = compose_head(c["Wd"].double(), c["W1"].double()), compose_head(c["Wd"].double().abs(), c["W1"].double().abs())
    z = F.conv2d(F.conv_transpose2d(x64, c["Wd"].double(), c["bd"].double(), stride=2), c["W1"].double(), c["b1"].double(), padding=1)
    if dtype == torch.float64:
        out = torch.relu(torch.einsum("bchw,c->bhw", torch.relu(z), c["w"].double()) + c["b"])
    else:
        Wc = ROUND[prec](compose_head(c["Wd"].to(dtype), c["W1"].to(dtype)).float()).to(dtype)
        pre = conv_gather(c["x"], Wc, 1, None, dtype).reshape(B, H, W, 4, 32)
        b9 = compose_bias9(c["W1"].to(dtype), c["bd"].to(dtype), c["b1"].to(dtype))
        out = torch.zeros(B, 2 * H, 2 * W, dtype=dtype)
        cls = lambda n: torch.where(torch.arange(n) == 0, 0, torch.where(torch.arange(n) == n - 1, 2, 1))  # noqa: E731
        cy, cx = cls(2 * H), cls(2 * W)
        for q in range(4):
            py, px = (q & 1, q >> 1) if mut == "parity_transposed" else (q >> 1, q & 1)
            bq = b9[cy[py::2]][:, cx[px::2]]   # [H, W, 32]
            out[:, py::2, px::2] = torch.relu(torch.relu(pre[:, :, :, q] + bq) @ c["w"].to(dtype) + c["b"])
    # the derived terms of the module docstring, per pre-activation of parity group q, co -> times sum|w| (an upper bound over q, co per pixel)
    ax = x64.abs()
    e_round = F.conv2d(ax, 0.5 * ulp_T(Wc64.abs(), prec), padding=1) if prec != F32 else torch.zeros(B, 128, H, W, dtype=torch.float64)
    e_sum = 4 * c["Cmid"] * U * F.conv2d(ax, Wabs, padding=1)
    e_bias = (9 * c["Cmid"] + 1) * U * (c["b1"].double().abs().max() + (c["W1"].double().abs().sum((2, 3)) @ c["bd"].double().abs()).max())
    bias9_max = compose_bias9(c["W1"].double(), c["bd"].double(), c["b1"].double()).abs().max()
    pre_max = F.conv2d(ax, Wc64.abs(), padding=1).max() + bias9_max   # >= max|acc + bias|
    e = (e_round + e_sum).reshape(B, 4, 32, H, W).amax(2) + e_bias + A_MFMA * pre_max
    bound = torch.zeros(B, 2 * H, 2 * W, dtype=torch.float64)
    for q in range(4):
        bound[:, q >> 1::2, q & 1::2] = e[:, q]
    dot_abs = torch.einsum("bchw,c->bhw", torch.relu(z), c["w"].double().abs()) + abs(c["b"])
    return out, bound * c["w"].abs().sum().double() + 12 * U * dot_abs


@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("hw", [(6, 5), (13, 11)])
def test_head_up2_checker_accepts_fp32_and_rejects_mutants(hw, mode):
    c = up2_case(2, hw[0], hw[1], 64, 64, mode)
    ref, bound = up2_eval(c)
    got = up2_eval(c, torch.float32)[0]
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"[decoder_gemm_ops] fp32 evaluation, head_up2 {hw} {MODE_ID(mode)}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0
    bad = up2_eval(c, torch.float32, "parity_transposed")[0]
    assert bool(((bad.double() - ref).abs() > bound).any()) == MUTANT_ACTIVE("parity_transposed", c)


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def xm_of(prec):
    return 2 if prec == F16X2 else 1


def stage(dev, rows, ld, prec):
    """fp32 rows [n, ld] (exact in T) -> the raw storage tensor."""
    from burn_depth_amd import ops
    return ops.store_rows(dev, rows.cuda().contiguous(), ld, prec)


def unstage(dev, raw, n, ld, prec):
    from burn_depth_amd import ops
    return ops.load_rows(dev, raw.contiguous(), n * ld, ld, prec).reshape(n, ld).cpu()


def stage_nchw(dev, x, ld, prec):
    """NCHW fp32 -> raw NHWC pixels of ld channels through the engine's own layout kernel (pad columns zero)."""
    from burn_depth_amd import ops
    n, Cn, H, W = x.shape
    raw = stage(dev, torch.zeros(n * H * W, ld), ld, prec).reshape(n, H, W, ld * xm_of(prec))
    return ops.nchw_to_nhwc(dev, x.cuda(), prec, False, ld, raw)


def padded(rows, ld, tail):
    """rows [n, C] inside a canary buffer [n + tail, ld]."""
    out = canary(rows.shape[0] + tail, ld)
    out[:rows.shape[0], :rows.shape[1]] = rows
    return out


def last_form():
    from burn_depth_amd import ops
    return ops.gemm_last_form()


TAIL = 5


def run_conv(dev, c, tile=TAUTO, ld_pad=0, out_f32=False):
    """-> (out rows [G M + TAIL, ldo], out2 rows or None), on the CPU; asserts that the inputs came back bit for bit."""
    from burn_depth_amd import ops
    prec, Cout, GM = c["prec"], c["Cout"], c["G"] * c["M"]
    ldo = Cout + ld_pad
    xr = stage_nchw(dev, c["x"], c["Cin"], prec)
    keep = [xr.clone()]
    kw = {}
    for k in ("r1", "r2"):
        if c[k] is not None:
            kw[k] = stage(dev, padded(c[k], ldo, 0), ldo, prec)
            keep.append(kw[k].clone())
    if out_f32:
        out = canary(GM + TAIL, Cout).cuda()
    else:
        out = stage(dev, canary(GM + TAIL, ldo), ldo, prec)
    out2 = stage(dev, canary(GM + TAIL, ldo) * 0.5, ldo, prec) if c["out2"] else None
    ops.decoder_gemm(dev, CONV3_S2 if c["stride"] == 2 else CONV3, xr, [w.cuda() for w in c["Ws"]], [None if b is None else b.cuda() for b in c["bs"]], prec, tile,
                     B=c["B"], H=c["H"], W=c["W"], Cin=c["Cin"], Cin_p=c["Cin"], Cout=Cout, out=out, ldo=ldo, act=c["act"], res1=kw.get("r1"), res2=kw.get("r2"),
                     res_mod=c["res_mod"] if c["G"] == 1 else 0, out2=out2, in_shared=c["shared"], res1_shared=c["shared"], out_f32=out_f32)
    for a, b in zip(keep, [xr] + [kw[k] for k in ("r1", "r2") if k in kw]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input of the launch changed"
    if out_f32:
        return out.cpu(), None
    return unstage(dev, out, GM + TAIL, ldo, prec), (unstage(dev, out2, GM + TAIL, ldo, prec) if out2 is not None else None)


def check_conv(c, got, got2, ld_pad, what, f32_out=False):
    ref, ref2, pre, sums = conv_eval(c)
    GM, Cout = c["G"] * c["M"], c["Cout"]
    can = canary(GM + TAIL, Cout + ld_pad)
    assert torch.equal(got[GM:], can[GM:]) and torch.equal(got[:, Cout:], can[:, Cout:]), what + ": rows behind M / pad columns of out"
    r = store_assert(got[:GM, :Cout], ref, pre, sums, F32 if f32_out else c["prec"], what)
    if got2 is not None:
        assert torch.equal(got2[GM:], can[GM:] * 0.5) and torch.equal(got2[:, Cout:], can[:, Cout:] * 0.5), what + ": rows behind M / pad columns of out2"
        assert torch.equal(got2[:GM, :Cout], torch.relu(got[:GM, :Cout])), what + ": out2 != relu(out)"
    return r


def assert_conv_launch(f, c, tile, ldo, out_f32=False):
    """Which kernel ran a 3 x 3 launch of case c: the tile (the forced one, else the cost model's choice -- md_gemm_pick_tile on the summed
    rows: with every tile count of these shapes below the 256 CUs the model's cost does not depend on how the rows split into groups), and
    for the 256 x 256 kernel its form as gemm256_form chooses it: one tile per workgroup (all launches here are far below the loops' 1024
    tiles), the staged 2-byte store kind for 16-byte rows without a res1 wrap, else the generic epilogue (fp32 operands, res_mod > 0, a
    split-half launch with an fp32 output). Another tile leaves no 256 x 256 record (family -1): gemm_kernel<BM, BN> with epilogue4."""
    from burn_depth_amd import _lib
    prec, mode = c["prec"], c["mode"]
    K = 9 * c["Cin"] * {"w": 1, "w16": 2, "w32": 3}[mode[1]]
    want = tile if tile != TAUTO else _lib.load().md_gemm_pick_tile(c["G"] * c["M"], c["Cout"], K, prec)
    assert f["tile"] == want, (f, want)
    if f["tile"] == T256:
        store = prec != F32 and not c["res_mod"] and not (prec == F16X2 and out_f32) and ldo % 8 == 0 and c["Cout"] % 8 == 0
        assert (f["family"], f["ek"], f["conv"], f["fold"], f["qkv"]) == (ONE_TILE, EK_STORE if store else EK_GENERIC, 0, 0, 0), f
        assert f["blocks"] == f["grid"] == c["G"] * -(-c["M"] // 256) * -(-c["Cout"] // 256), f
    else:
        assert f["family"] == -1, f


# (B, H, W, Cin, Cout, ld_pad, tile): M = 286 = one full 256-row tile + 30 rows, the image boundary at row 143; the all-border map; interior tiles at 17 x 19
CONV_SHAPES = [(2, 13, 11, 64, 32, 0, TAUTO), (2, 13, 11, 64, 64, 8, TAUTO), (2, 13, 11, 128, 128, 0, TAUTO), (2, 13, 11, 64, 256, 8, TAUTO),
               (2, 13, 11, 64, 256, 0, T256), (2, 13, 11, 64, 128, 8, T128), (2, 13, 11, 64, 64, 0, T128x64), (2, 13, 11, 64, 64, 8, T64),
               (1, 2, 2, 64, 64, 0, TAUTO), (1, 17, 19, 64, 256, 0, T256), (1, 17, 19, 64, 64, 8, TAUTO)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "B%d_%dx%d_C%d_N%d_pad%d_tile%d" % s)
def test_conv3_residual_second_output_against_fp64(dev, shape, mode):
    """residual_unit's second convolution: out = conv + bias + res1 + res2, out2 = relu(out); and with ACT_RELU. f32: Cin 64 -> 96 (a k-tile of 32)."""
    B, H, W, Cin, Cout, ld_pad, tile = shape
    Cin = 96 if (mode[0] == F32 and Cin == 128) else Cin
    for act in (0, 1):
        c = conv_case(B, H, W, Cin, Cout, mode, res=2, act=act, out2=True)
        got, got2 = run_conv(dev, c, tile, ld_pad)
        assert_conv_launch(last_form(), c, tile, Cout + ld_pad)
        check_conv(c, got, got2, ld_pad, f"conv3 res2 out2 act{act} {shape} {MODE_ID(mode)}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("form", ["shared", "unshared", "table", "rn"])
def test_conv3_groups_and_residual_wrap_against_fp64(dev, form, mode):
    """Two weight groups with the shared input and the shared res1 (res_mod = M) and unshared; the per-image table res_mod = P < M at B = 3;
    the bias-free layerN_rn form with a second output only."""
    kw = {"shared": dict(B=2, H=13, W=11, G=2, shared=True, res=2, out2=True), "unshared": dict(B=2, H=13, W=11, G=2, shared=False, res=2, out2=True),
          "table": dict(B=3, H=13, W=11, res=1, table=True, out2=True), "rn": dict(B=2, H=13, W=11, out2=True, bias=False)}[form]
    for Cout, tile in ((64, TAUTO), (256, T256)):
        c = conv_case(Cin=64, Cout=Cout, mode=mode, **kw)
        assert c["res_mod"] == {"shared": c["M"], "unshared": 0, "table": 143, "rn": 0}[form]
        got, got2 = run_conv(dev, c, tile, 8)
        assert_conv_launch(last_form(), c, tile, Cout + 8)   # (res_mod > 0 takes the generic epilogue)
        check_conv(c, got, got2, 8, f"conv3 {form} N{Cout} {MODE_ID(mode)}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("hw", [(13, 11), (12, 10)])
def test_conv3_stride2_against_fp64(dev, hw, mode):
    """cstride = 2 with cOH / cOW: odd maps (the last tap on the pad row) and even maps (inside); the T-typed NHWC store and the fp32 + ReLU rows."""
    for out_f32, Cout, tile in ((False, 64, TAUTO), (False, 256, T256), (True, 32, TAUTO), (True, 128, T128)):
        c = conv_case(2, hw[0], hw[1], 64, Cout, mode, stride=2, act=1 if out_f32 else 0)
        assert (c["OH"], c["OW"]) == ((hw[0] + 1) // 2, (hw[1] + 1) // 2)
        got, _ = run_conv(dev, c, tile, 0 if out_f32 else 8, out_f32)
        assert_conv_launch(last_form(), c, tile, Cout + (0 if out_f32 else 8), out_f32)
        check_conv(c, got, None, 0 if out_f32 else 8, f"conv3 stride 2 {hw} f32out={out_f32} N{Cout} {MODE_ID(mode)}", out_f32)


PS_SHAPES = [(5, 7, 2, 0, 0), (5, 7, 2, 64, 56), (5, 7, 2, 72, 0), (12, 10, 2, 72, 56), (5, 7, 4, 0, 56), (12, 10, 4, 64, 0), (5, 7, 4, 72, 56)]   # H, W, f, coff, pad


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("shape", PS_SHAPES, ids=lambda s: "%dx%d_f%d_coff%d_pad%d" % s)
def test_pixel_shuffle_channel_slice_against_fp64(dev, shape, mode):
    """deconv2(): the scatter into channels [coff, coff + Cout) of pixels of ldo, with and without the relu'd second output. launch_gemm sets
    ps_fast for 2-byte outputs without a second output when psC, ldo and ps_coff are multiples of 8 -- asserted from the launch record."""
    from burn_depth_amd import ops
    H, W, f, coff, pad = shape
    prec = mode[0]
    for Cout, tile, with2 in ((64, TAUTO, False), (64, TAUTO, True), (64, T256, False), (36, T128, False)):
        c = ps_case(2, H, W, 64, Cout, mode, f, coff, pad, with2)
        ldo, rows = c["ldo"], 2 * f * f * H * W
        ref, wrote, pre = ps_eval(c)
        xr = stage_nchw(dev, c["x"], 64, prec)
        x0 = xr.clone()
        out = stage(dev, canary(rows + TAIL, ldo), ldo, prec)
        out2 = stage(dev, canary(rows + TAIL, ldo) * 0.5, ldo, prec) if with2 else None
        ops.decoder_gemm(dev, PIXSHUF, xr, c["Wt"].cuda(), c["b"].cuda(), prec, tile, B=2, H=H, W=W, Cin=64, Cin_p=64, Cout=Cout, out=out, ldo=ldo, out2=out2,
                         ps_f=f, ps_coff=coff)
        fm = last_form()
        fast = prec != F32 and not with2 and Cout % 8 == 0 and ldo % 8 == 0 and coff % 8 == 0
        assert fm["ps_fast"] == int(fast) and (tile == TAUTO or fm["tile"] == tile), fm
        if fm["tile"] == T256:   # split-half takes the pixel-shuffle kind in its fast form only
            assert fm["ek"] == (EK_PIXSHUF if (prec != F16X2 or fast) else EK_GENERIC), fm
        assert torch.equal(x0.view(torch.uint8), xr.view(torch.uint8))
        what = f"pixel shuffle {shape} N{Cout} tile{tile} out2={with2} {MODE_ID(mode)}"
        got = unstage(dev, out, rows + TAIL, ldo, prec)
        can = canary(rows + TAIL, ldo)
        assert torch.equal(got[rows:], can[rows:]), what + ": rows behind M"
        g4 = got[:rows].reshape(ref.shape)
        assert torch.equal(g4[~wrote], canary(*ref.shape)[~wrote]), what + ": columns outside the slice"
        assert_close_in(g4[wrote], ref[wrote], prec, A_MFMA * pre.abs().max().item() / ref[wrote].abs().max().item(), what=what)
        if with2:
            got2 = unstage(dev, out2, rows + TAIL, ldo, prec)
            assert torch.equal(got2[rows:], can[rows:] * 0.5) and torch.equal(got2[:rows].reshape(ref.shape)[~wrote], (canary(*ref.shape) * 0.5)[~wrote]), what
            assert torch.equal(got2[:rows].reshape(ref.shape)[wrote], torch.relu(g4[wrote])), what + ": out2 != relu(out)"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("acts", [(), (1, 3), (2, 2, 2, 2, 2, 2, 3), (0, 1, 2, 3)], ids=["one", "depth_conf", "rays_conf", "all_acts"])
def test_head_tail_against_fp64(dev, acts, mode):
    """EPI_HEAD on the 256 x 32 tile: the one-channel form and head_nch = 2 | 7 | 4 channels in one launch; B = 2 with the image boundary at row
    143 inside tile 0; bstride = (nch + 1) planes (a plane of no channel stays canary) and bstride = the plane (one tensor per channel)."""
    from burn_depth_amd import ops
    prec = mode[0]
    for big in ((True, False) if acts else (True,)):
        c = head_case(2, 13, 11, 64, mode, acts, big)
        B, HW, n = 2, 143, max(len(acts), 1)
        ref, wrote, bound = head_eval(c)
        xr = stage_nchw(dev, c["x"], 64, prec)
        x0 = xr.clone()
        planes = canary(B, n + 1, HW).cuda()
        kw = {}
        if not acts:
            flat = canary(B * HW + TAIL).cuda()
            kw = dict(out=flat, head_w=c["wc"][0].cuda(), head_b=float(c["bc"][0]), head_act=0)
        elif big:
            kw = dict(head=[dict(w=c["wc"][i].cuda(), b=float(c["bc"][i]), act=acts[i], out=planes[:, i], bstride=(n + 1) * HW) for i in range(n)])
        else:
            singles = [canary(B * HW + TAIL).cuda() for _ in range(n)]
            kw = dict(head=[dict(w=c["wc"][i].cuda(), b=float(c["bc"][i]), act=acts[i], out=singles[i], bstride=HW) for i in range(n)])
        if acts and big:   # a strided view: hand over the base pointer of the channel's first plane
            for i, h in enumerate(kw["head"]):
                h["out"] = planes.reshape(-1)[i * HW:]
        ops.decoder_gemm(dev, HEAD, xr, c["W1"].cuda(), c["b1"].cuda(), prec, B=B, H=13, W=11, Cin=64, Cin_p=64, Cout=32, **kw)
        f = last_form()
        assert f["tile"] == T256x32 and f["family"] == -1, f
        assert torch.equal(x0.view(torch.uint8), xr.view(torch.uint8))
        if not acts:
            got = flat.cpu()
            assert torch.equal(got[B * HW:], canary(B * HW + TAIL)[B * HW:]), "rows behind M"
            g = canary(B, 2, HW)
            g[:, 0] = got[:B * HW].reshape(B, HW)
        elif big:
            g = planes.cpu()
        else:
            g = canary(B, n + 1, HW)
            for i in range(n):
                assert torch.equal(singles[i].cpu()[B * HW:], canary(B * HW + TAIL)[B * HW:]), "rows behind the last plane"
                g[:, i] = singles[i].cpu()[:B * HW].reshape(B, HW)
        head_assert(g, ref, wrote, bound, f"head nch{len(acts)} acts{acts} bstride={'wide' if big else 'plane'} {MODE_ID(mode)}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_ID)
@pytest.mark.parametrize("hw", [(6, 5), (13, 11)])
def test_head_up2_against_fp64(dev, hw, mode):
    """EPI_HEAD_UP2 on the 128 x 128 tile against the DEFINITION (conv_transpose2d -> conv2d -> relu -> dot -> relu): the four parity groups on
    their pixels of the 2H x 2W map, the nine bias classes on the border; rows behind the map stay canary."""
    from burn_depth_amd import ops
    H, W = hw
    c = up2_case(2, H, W, 64, 64, mode)
    ref, bound = up2_eval(c)
    xr = stage_nchw(dev, c["x"], 64, mode[0])
    x0 = xr.clone()
    n = 2 * 4 * H * W
    out = canary(n + TAIL).cuda()
    ops.decoder_gemm(dev, HEAD_UP2, xr, c["Wd"].cuda(), c["bd"].cuda(), mode[0], B=2, H=H, W=W, Cin=64, Cin_p=64, Cout=32, out=out, head_w=c["w"].cuda(),
                     head_b=c["b"], Cmid=64, w2=c["W1"].cuda(), bias2=c["b1"].cuda())
    f = last_form()
    assert f["tile"] == T128 and f["family"] == -1, f
    assert torch.equal(x0.view(torch.uint8), xr.view(torch.uint8))
    assert torch.equal(out.cpu()[n:], canary(n + TAIL)[n:]), "rows behind the map"
    got = out.cpu()[:n].reshape(2, 2 * H, 2 * W)
    assert torch.isfinite(got).all()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print(f"[decoder_gemm_ops] head_up2 {hw} {MODE_ID(mode)}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"head_up2 {hw} {MODE_ID(mode)}: worst err/bound {ratio:.3f}"
    bad = up2_eval(c, torch.float32, "parity_transposed")[0]   # (the bound separates the groups' pixels at this very case)
    assert ((bad.double() - ref).abs() > bound).any()


@pytest.mark.gpu
def test_fp8_is_refused(dev):
    """The decoders do not run in fp8: the entry's own error, before any launch."""
    from burn_depth_amd import _lib, ops
    x = torch.zeros(2 * 2 * 64, dtype=torch.uint8).cuda()
    out = torch.zeros(4 * 32, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.MdError) as e:
        ops.decoder_gemm(dev, CONV3, x, torch.zeros(32, 64, 3, 3).cuda(), torch.zeros(32).cuda(), FP8, B=1, H=2, W=2, Cin=64, Cin_p=64, Cout=32, out=out, ldo=32)
    assert "decoder_gemm" in str(e.value) and "precision" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [BF16, F16], ids=["bf16", "f16"])
def test_residual_convolution_tile_loop_is_bit_identical_to_the_one_tile_kernel(dev, prec):
    """gemm256r_kernel<T, false, true> (persist bit 8) runs the 3 x 3 convolution with residual inputs and a second output from 1024 tiles of
    N = 256 (gemm256_form: loop_ok) on one workgroup per CU: the smallest launch with more tiles than workgroups is max(1024, grid + 1)
    tiles, here as a map of 509 columns. Same bits with the loop and with the one-tile kernel, out and out2."""
    from burn_depth_amd import _lib, ops
    lib = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = max(cus & ~7, 8)
    tiles = max(1024, grid + 1)
    W = 509
    H = -(-((tiles - 1) * 256 + 1) // W)
    M = H * W
    dt = torch.bfloat16 if prec == BF16 else torch.float16
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(M, 64, generator=g, device="cuda").to(dt)
    r1, r2 = (torch.randn(M, 256, generator=g, device="cuda").to(dt) for _ in range(2))
    w = (torch.randn(256, 64, 3, 3, generator=g, device="cuda") / 24.0).to(dt).float()
    b = torch.randn(256, generator=g, device="cuda")
    res = []
    prev = lib.md_debug_gemm_persistent(15)
    try:
        for mask in (15, 0):
            lib.md_debug_gemm_persistent(mask)
            out, out2 = torch.full((M, 256), 3.0, device="cuda", dtype=dt), torch.full((M, 256), 5.0, device="cuda", dtype=dt)
            ops.decoder_gemm(dev, CONV3, x, w, b, prec, T256, B=1, H=H, W=W, Cin=64, Cin_p=64, Cout=256, out=out, ldo=256, res1=r1, res2=r2, out2=out2)
            f = last_form()
            assert f["blocks"] == -(-M // 256) and f["blocks"] >= tiles and f["tile"] == T256
            if mask:
                assert (f["family"], f["conv"], f["grid"]) == (LOOP_R, 1, grid) and f["blocks"] > f["grid"], f
            else:
                assert (f["family"], f["ek"], f["grid"]) == (ONE_TILE, EK_STORE, f["blocks"]), f
            res.append((out, out2))
    finally:
        lib.md_debug_gemm_persistent(prev)
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16)) and torch.equal(res[0][1].view(torch.int16), res[1][1].view(torch.int16))
    assert torch.equal(res[0][1].float(), torch.relu(res[0][0].float())) and float(res[0][0].float().abs().max()) > 1.0
