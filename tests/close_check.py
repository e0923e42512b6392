"""The per-element checker the operator tests share (tests/test_da3_token_ops.py, tests/test_operand_writers.py): every element of a
kernel's output is held to

    |got - ref| <= 0.5 * ulp_T(|ref|) * (1 + slack) + a32 * max|ref|  (+ a derived extra term where a test states one)

against an fp64 reference. ulp_T = the spacing of the storage type at |ref|: 2^(e-7) for bf16 (8 significant bits), 2^(e-10) for f16
(11 bits; never below the subnormal spacing 2^-24), 2^(e-21) for the split-half f16x2 (hi + lo, 22 bits; lo is an f16, same floor),
2^(e-3) for OCP e4m3 (4 bits; never below the subnormal spacing 2^-9; the reference is already scaled and clamped to +-448), absent for
f32; 2^e <= |ref| < 2^(e+1). a32 = the fp32-arithmetic allowance of the suite: 2e-5 behind an MFMA contraction (A_MFMA), 2e-6 for
LayerNorm-only kernels (A_LN). slack = 1 only where `ref` lies within a32 * max|ref| of a rounding boundary of T; elements that need it
are counted and their share must stay under 1 %. The docstrings of the two test files say where each term comes from."""
import torch

from oracle.depth_pro_ref import f16x2_round

BF16, F32, FP8, F16, F16X2 = 0, 1, 2, 3, 4
PRECS = [BF16, F16, F32, F16X2]
PNAME = {BF16: "bf16", F32: "f32", FP8: "fp8", F16: "f16", F16X2: "f16x2"}
ROUND = {BF16: lambda t: t.bfloat16().float(), F32: lambda t: t, F16: lambda t: t.half().float(), F16X2: f16x2_round,
         FP8: lambda t: t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()}
SIG_BITS = {BF16: 8, F16: 11, F16X2: 22, FP8: 4}
ULP_FLOOR = {BF16: 2.0 ** -133, F16: 2.0 ** -24, F16X2: 2.0 ** -24, FP8: 2.0 ** -9}
A_MFMA, A_LN = 2e-5, 2e-6


def ulp_T(a, prec):
    """Spacing of the storage type at magnitude a (fp64 tensor, >= 0); zeros for f32 (the term is absent)."""
    if prec == F32:
        return torch.zeros_like(a)
    _, ex = torch.frexp(a.clamp_min(1e-300))  # a = m * 2^ex, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), ex - SIG_BITS[prec]).clamp_min(ULP_FLOOR[prec])


def near_boundary(v, prec, dist):
    """True where v lies within `dist` of a rounding boundary (the midpoint of two neighbouring values) of T."""
    if prec == F32:
        return torch.zeros_like(v, dtype=torch.bool)
    u = ulp_T(v.abs(), prec)
    t = v.abs() / u
    return ((t - t.floor()) - 0.5).abs() * u <= dist


def close_report(got, ref64, prec, a32, extra=None, slack_beyond_extra=False):
    """`slack_share`: the share of elements beyond 0.5 ulp + a32 max|ref| -- the elements that use the tie slack or `extra`. A caller
    whose `extra` is as large as the half-ulp on every element (tests/test_attention_ops.py) passes slack_beyond_extra=True: the share
    then counts the elements beyond 0.5 ulp + a32 max|ref| + extra, the tie slack's own users; `beyond_plain` keeps the former."""
    ref, got = ref64.double(), got.double()
    A = a32 * ref.abs().max()
    u = ulp_T(ref.abs(), prec)
    err = (got - ref).abs()
    plain = 0.5 * u + A
    bound = plain + 0.5 * u * near_boundary(ref, prec, A)
    if extra is not None:
        bound = bound + extra
    ratio = err / bound.clamp_min(1e-300)  # (a bound of 0 -- an exact zero reference in f32 -- admits only err = 0)
    beyond_plain = (err > plain).double().mean().item()
    slack_share = (err > plain + extra).double().mean().item() if slack_beyond_extra and extra is not None else beyond_plain
    return {"max_err": err.max().item(), "bound_at_max": bound.flatten()[err.argmax()].item(), "worst_ratio": ratio.max().item(),
            "n_bad": int((err > bound).sum()), "slack_share": slack_share, "beyond_plain": beyond_plain, "n": err.numel()}


def assert_close_in(got, ref64, prec, a32, extra=None, what="", tag="close_check", slack_beyond_extra=False):
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    r = close_report(got, ref64, prec, a32, extra, slack_beyond_extra)
    print(f"[{tag}] {what} {PNAME[prec]}: max err {r['max_err']:.3e} (bound there {r['bound_at_max']:.3e}), "
          f"worst err/bound {r['worst_ratio']:.3f}, slack users {r['slack_share']:.2e}")
    assert r["n_bad"] == 0, f"{what} {PNAME[prec]}: {r['n_bad']} of {r['n']} elements outside the bound, worst err/bound {r['worst_ratio']:.3f}"
    assert r["slack_share"] < 0.01, f"{what} {PNAME[prec]}: {r['slack_share']:.3%} of the elements need the tie slack"
    return r


def rejects(got, ref64, prec, a32, extra=None, slack_beyond_extra=False):
    r = close_report(got, ref64, prec, a32, extra, slack_beyond_extra)
    return r["n_bad"] > 0 or r["slack_share"] >= 0.01
