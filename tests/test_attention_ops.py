"""Operator tests of the fused attention kernel (kernels/attention.hip) per launch form, per element against fp64: the plain form
(bf16 / f16 / split-half), the small-launch key-split form (KS = 2, QW = 2), the e4m3-output form, the 577-token assembly kernel with its
HIP twin, the fp32 three-launch path, and enlarged strides. Every GPU test goes through `md_op_attention_ex` and asserts, from
`md_debug_attention_last_form`, that the launcher took the form the test means (a retuned kKeySplitMin / kKeySplitBlocks or assembly rule
fails the test instead of silently turning it into a second plain-form case).

Reference: plain torch fp64 softmax(q k^T / 8) v per (sequence, head) on the operands as the device stores them -- q rounded after the
softmax scale is folded in (oracle `round_q_prescaled`), k and v rounded to the type -- with P NOT rounded.

Bound per element (`close_check.assert_close_in`): 0.5 ulp_T(|ref|) (the output store) + A_MFMA max|ref| (fp32 accumulation order of
the two MFMA contractions, the suite's constant) + extra, extra[q, d] = u_P sum_k p_k |v_kd| / l from the reference's own probabilities:
the rounding of P to the type the P.V MFMA takes. u_P as the issue sets it: bf16 2^-9, f16 2^-12, split-half with P = hi + lo 2^-23.
NOTE: these are HALF the worst-case relative rounding error of the types (8, 11 and 22 significant bits: 2^-8, 2^-11, 2^-22). The term
is therefore not a worst-case bound. It holds where the roundings of many keys average, and is missed by correct arithmetic on rows
that one key dominates (below). f16 adds a floor: a p below 2^-14 lands on the subnormal grid, an absolute error of up to 2^-25 in the
units of the fixed offset m_g of its key group (the row maximum of the group's first tile; the fp64 logits give it). The groups meet at
mn = max_g m_g, so the floor term is 2^-25 sum_g 2^(m_g - mn) sum_{k in g} |v_kd| / sum_k 2^(s_k - mn) (split-half: the lo plane is an
f16 too). e4m3 output: the reference is clamp(ref * out_fp8_inv, +-448) with the e4m3 ulp, extra scaled by out_fp8_inv, + 2^-24 |ref|
for the fp32 rounding of the fused inv_l * out_fp8_inv; out_fp8_inv = 448 / 8 is the DA3 fp8 engine's (md_da3.hip kActScale). fp32 path:
A_MFMA alone. Tie-slack users stay under 1 %: close_check's cap, taken with `slack_beyond_extra=True`, i.e. over the elements beyond
0.5 ulp + A_MFMA max|ref| + extra. close_check's default counts every element beyond 0.5 ulp + A_MFMA max|ref| (its other callers' extra
terms are rare-event allowances). Here the P term is as large as the half-ulp on EVERY element (u_P sum p|v| / l against 2^-9 |ref| in
bf16, and sum p|v| >= |ref|), so correct arithmetic leaves that narrower band on a large share of them: the fp32 emulation on up to
40 % in bf16, 20 % in f16, 3 % in e4m3-out, none in split-half and fp32. `check` prints that share per case; it is no condition.

Inputs: standard normal q, k, v (logits of about one natural unit, the class the kernel header calls trained-ViT-like); every
(sequence, head) unit's V carries its own offset (0.25 apart), so a permuted unit fails per element.

CPU tests (no device). `emulate` is the kernel's arithmetic in fp32: exp2 of the pre-scaled logits against m = 0 (bf16) or the first
tile's row maximum (f16, split-half), P rounded to the type, row sums from the unrounded p per lane half, the two key groups merged at
the common offset, the e4m3 pack. It also evaluates the fast body's own checks (|m| <= 64, row sums below 2^100 / 57000) and the test
asserts that every case stays inside them: that is how the group-offset cases "reach the fast body" (it cannot be asserted on the
device without touching the kernel). Worst err/bound of the emulation, and of the MI355X run (equal to three digits on every form):
  plain      bf16 0.963   f16 0.818   f16x2 0.017 (GPU 0.042)
  key-split  bf16 0.652   f16 0.520   f16x2 0.014 (GPU 0.046)
  assembly   bf16 0.681   e4m3-out bf16 0.977   fp32 path 0.007 (GPU 0.025)
  group-offset case: key-split bf16 0.444, f16 0.590, f16x2 0.047; the same inputs in the plain form: bf16 0.444, f16 0.403, f16x2 0.011 (GPU 0.029).
Where u_P would be missed by correct arithmetic: on a row that ONE key dominates the output is v (1 + delta_P) with |delta_P| up to 2^-8
(bf16) / 2^-11 (f16) for a correctly rounded P, twice what u_P admits (with the planted keys' V rows at full scale the emulation and
the kernel alike gave err/bound 1.055 in bf16 and 1.126 in plain f16 on one planted row). The planted keys' V rows are therefore scaled
by 2^-10 (`_inputs`): the dominant key's rounding then weighs about 1e-5, below the P term of the other keys, and what the planted rows
check is the other keys' 2 % of the mass -- in f16 group 0's share of it, moved across 12 log2 units by the merge.
`test_spike_rows_carry_the_offsets_they_are_meant_to` shows that every element of the first-tile planted rows rejects a merge without
the common offset, and that most elements of the later-tile planted rows (and no other row) reject a P pack that saturates below their
p ~ 2^14: the planted key's own 2^-10-scaled v then arrives 8 times too small, about 1e-3 against a bound of about 3e-5. What the later-tile
rows can NOT reject is an error of the large P below about 3 % of it (the bound over |v| 2^-10).

Group-offset cases (N = 1089: 18 tiles, 9 + 9): four planted (query, key) pairs, one per query wave of two 64-query blocks; the key's
logit is 12 log2 units above the row's largest other logit. Two keys sit in group 1's FIRST tile (tile 9): f16 takes them as group 1's
offset, 12+ units above group 0's, so the merge scales group 0 by 2^-12 or less -- the fast body, offset path of the merge. Two sit in
LATER tiles (13, 14): p = 2^(12 + spread) ~ 2^14 < 57000 against group 1's first-tile offset -- the fast body with a large P.

Mutants (each rejected per element on every case where `MUTANT_ACTIVE` says it is not the identity, except the pairs of
`NOT_REJECTABLE`, which are asserted to pass): key N admitted -- the leaked key holding the poison value, a live k / v row (the next
unit's row 0), and the zero padding's value; the last-tile mask applied in the wrong key group (= every padding key of the last tile
admitted; the same three fillings); group 1's partial sums dropped; the merge without the common offset (f16, split-half); the row sum
without the cross-half exchange; q scaled without log2(e); bits 2 and 3 of the key index not swapped for sub-tile 1 (P meets the wrong
V rows); the XCD remap's permutation applied to the written blocks; query block 1 written at block 0's rows; e4m3 without the clamp,
with the scale applied after the rounding, with the bytes of one 4-vector reversed; the P pack saturating at 2^11 (group-offset cases).
A leaked LIVE key is rejected on every case, N = 37 .. 1089, in all three types: some query of the launch meets it with a logit a few
units above the mean and moves by far more than v / N.
What the per-element bound can NOT reject (`NOT_REJECTABLE`; asserted, both ways):
* ONE leaked ZERO-valued key (zero padding) at N >= 577 in bf16 and f16: p * 0 adds nothing to the output and 2^0 = 1 to a row sum of
  l = sum_k e^(s_k) ~ N e^(1/2) (unit-variance logits), so the row shrinks by about 1 / (1.65 N) of itself: 1.0e-3 at 577, 5.6e-4 at
  1089, against a half-ulp of 2^-9 .. 2^-8 (bf16) and a P term of 2^-12 sum p|v| ~ 2e-4 on outputs of a few 1e-2 (f16). Below 577,
  in split-half at every N, and with more than one leaked key (the wrong-group mask at N = 1025, 1089) it is rejected.
  `test_leaked_zero_key_is_caught_by_the_poison_bits` shows on the CPU that the same defect changes bits on every active case once
  the padding is poisoned, which is what the GPU test `test_poisoned_padding_changes_no_bit` compares, for every form but the fp32 path.
* the normaliser taken from the ROUNDED P, on every case: it differs from the kernel by the P rounding of the row sum, which is inside
  the P term by construction (the kernel header records it as numerically equivalent). The test asserts that the mutant changes bits
  and that no case rejects it; nothing else in the suite catches it either.
Known gaps: the redo scan kernel's `nunits > 1024` loop (about 0.5 GB of operands to reach); MD_ATTN_PTERMS = 1 (a DIAG-build matter);
which body (fast / safe) a launch ran cannot be asserted on the device.
"""
import functools

import pytest
import torch

import close_check
from close_check import A_MFMA, BF16, F16, F16X2, F32, FP8, PNAME, ROUND, rejects
from oracle import depth_pro_ref as R

# the P term is as large as the output's half-ulp on every element, so the tie-slack share counts the elements beyond it (opt-in)
assert_close_in = functools.partial(close_check.assert_close_in, tag="attention_ops", slack_beyond_extra=True)
LOG2E = 1.4426950408889634
QSCALE = torch.tensor(0.125 * LOG2E, dtype=torch.float32)   # kernels/ops.h kAttnQScale, as the fp32 constant the splitter multiplies by
FP8_INV = 448.0 / 8.0          # md_da3.hip kActScale = 8 / 448: the engine passes a_inv = 1 / kActScale to launch_attention
U_P = {BF16: 2.0 ** -9, F16: 2.0 ** -12, F16X2: 2.0 ** -23, F32: 0.0}
P_FLOOR = {BF16: 0.0, F16: 2.0 ** -25, F16X2: 2.0 ** -25, F32: 0.0}   # half the f16 subnormal spacing, per key (split-half: of the lo plane)
FAST_SUM_MAX = {BF16: 1.2676506e30, F16: 57000.0, F16X2: 57000.0}      # attention.hip kFastSumMax
POISON = {BF16: 1.6225927682921336e+29, F16: 8192.0, F16X2: 8192.0 + 8192.0}  # 0x7000 in every 16-bit slot (split-half: hi + lo)
OP_PRECS = [BF16, F16, F16X2]


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
class Case:
    def __init__(self, form, prec, T, heads, N, *, seq_stride=0, kpad=0, fp8_inv=0.0, small=-1, asm=True, kind="plain", vscale=1.0):
        self.form, self.prec, self.T, self.heads, self.N = form, prec, T, heads, N
        self.seq_stride, self.kpad, self.fp8_inv, self.small, self.asm, self.kind, self.vscale = seq_stride, kpad, fp8_inv, small, asm, kind, vscale

    @property
    def id(self):
        s = f"{self.form}-{PNAME[self.prec]}-T{self.T}h{self.heads}N{self.N}"
        s += f"-S{self.seq_stride}k{self.kpad}" if self.seq_stride or self.kpad else ""
        s += "-clamp" if self.vscale != 1.0 else ""
        return s + ("-spikes" if self.kind == "spikes" else "")

    def key(self):
        return (self.form, self.prec, self.T, self.heads, self.N, self.seq_stride, self.kpad, self.fp8_inv, self.small, self.asm, self.kind, self.vscale)

    def but(self, **kw):
        c = Case(self.form, self.prec, self.T, self.heads, self.N, seq_stride=self.seq_stride, kpad=self.kpad, fp8_inv=self.fp8_inv,
                 small=self.small, asm=self.asm, kind=self.kind, vscale=self.vscale)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    # launch geometry, as launch_attention derives it
    @property
    def qrows(self):
        return 64 if self.form == "key-split" else 128

    @property
    def qblocks(self):
        return (self.N + self.qrows - 1) // self.qrows

    @property
    def nwg(self):
        return self.qblocks * self.heads * self.T


# (T, heads, N): 128-query workgroups 1, 7, 17, 9, 15, 8, 16 -- nwg >> 3 = 0 and > 0, nwg & 7 = 0 and > 0
PLAIN_SHAPES = [(1, 1, 37), (7, 1, 64), (17, 1, 65), (3, 3, 127), (5, 3, 128), (2, 2, 129), (4, 2, 191)]
PLAIN = [Case("plain", p, T, h, N) for p in OP_PRECS for (T, h, N) in PLAIN_SHAPES]
STRIDES = [Case("plain" if p != F32 else "fp32-path", p, 2, 2, 65, seq_stride=192, kpad=192) for p in OP_PRECS + [F32]]
KS_NS = [1024, 1025, 1087, 1089]
KEYSPLIT = [Case("key-split", p, 1, h, N) for p in OP_PRECS for h in (1, 2) for N in KS_NS]
SPIKES = [Case("key-split", p, 1, 1, 1089, kind="spikes") for p in OP_PRECS]
FP8OUT = [Case("fp8-out", BF16, 2, 2, N, fp8_inv=FP8_INV) for N in (65, 129)] + [Case("fp8-out", BF16, 2, 2, 129, fp8_inv=FP8_INV, vscale=16.0)]
ASM = [Case("assembly", BF16, 2, h, 577, kpad=640) for h in (1, 2)]
F32PATH = [Case("fp32-path", F32, 2, 2, N) for N in (37, 65, 129)]
ASM_OFF = [c.but(form="plain", asm=False) for c in ASM]
KS_OFF = [c.but(form="plain", small=0) for c in KEYSPLIT + SPIKES]
ALL_CASES = PLAIN + STRIDES + KEYSPLIT + SPIKES + FP8OUT + ASM + F32PATH + ASM_OFF + KS_OFF
POISON_CASES = [c for c in PLAIN + STRIDES + KEYSPLIT + SPIKES + FP8OUT + ASM + ASM_OFF + KS_OFF if c.prec != F32]
cid = lambda c: c.id  # noqa: E731

SPIKE_ROWS = [(2 * 64 + 5, 9 * 64 + 3), (2 * 64 + 32 + 7, 13 * 64 + 40),     # (query, key): block 2: wave 0 -> group 1's first tile (tile 9 of
              (9 * 64 + 32 + 1, 9 * 64 + 60), (9 * 64 + 11, 14 * 64 + 17)]   # 18), wave 1 -> a later tile; block 9: the waves swapped
SPIKE_LOG2 = 12.0


@functools.lru_cache(maxsize=None)
def _inputs(T, heads, N, kind, vscale):
    D = heads * 64
    g = torch.Generator().manual_seed(4000 + 131 * T + 17 * heads + N)
    qkv = torch.randn(T, N, 3, heads, 64, generator=g)
    U = T * heads
    off = (torch.arange(U, dtype=torch.float32).reshape(T, 1, heads, 1) - (U - 1) / 2) * 0.25   # every unit's V on its own offset
    qkv[:, :, 2] += off
    qkv[:, :, 2] *= vscale
    if kind == "spikes":
        # the planted key is its query's direction, scaled so that its logit lies SPIKE_LOG2 log2 units above the row's largest other logit
        for qi, ki in SPIKE_ROWS:
            q = qkv[0, qi, 0, 0].double()
            others = (qkv[0, :, 1, 0].double() @ q) * 0.125 * LOG2E
            others[[k for _, k in SPIKE_ROWS]] = -1e30
            target = (others.max().item() + SPIKE_LOG2) / LOG2E
            qkv[0, ki, 1, 0] = (q * (8.0 * target / float(q.square().sum()))).float()
            # The planted key holds about 98 % of its row, so its ONE P rounding (up to 2^-8 / 2^-11 relative) would reach the output
            # whole, which the averaged u_P does not admit. Its V row is therefore small (an exact power-of-two scale): that rounding
            # then weighs |v| 2^-8 ~ 1e-5, below the P term of the other keys, and the row's output is the other keys' 2 % -- group 0's
            # share of it carried across the 12 log2 units of the merge, where a wrong factor shows in absolute terms.
            qkv[0, ki, 2, 0] *= 2.0 ** -10
    return qkv.reshape(T, N, 3 * D)


def inputs(c):
    return _inputs(c.T, c.heads, c.N, c.kind, c.vscale)


def operands(c, prec=None):
    """q (pre-scaled, log2 units; fp32 path: plain), k, v as the device stores them: fp32 tensors [T, heads, N, 64]."""
    prec = c.prec if prec is None else prec
    q, k, v = inputs(c).reshape(c.T, c.N, 3, c.heads, 64).permute(2, 0, 3, 1, 4)
    rnd = ROUND[prec]
    if prec == F32:
        return q.contiguous(), k.contiguous(), v.contiguous()
    return rnd(q * QSCALE), rnd(k.contiguous()), rnd(v.contiguous())


def key_groups(c):
    """[(first key, end key)] of the key groups of the launch: one, or the two halves of the key tiles."""
    NT = (c.N + 63) // 64
    if c.form != "key-split":
        return [(0, c.N)]
    per = (NT + 1) // 2
    return [(0, per * 64), (per * 64, c.N)]


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = Case(*key[:5], **dict(zip(("seq_stride", "kpad", "fp8_inv", "small", "asm", "kind", "vscale"), key[5:])))
    T, N, heads = c.T, c.N, c.heads
    if c.prec == F32:
        q, k, v = (t.double() for t in operands(c))
    else:
        qkv = inputs(c).reshape(T, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
        q = R.round_q_prescaled(qkv[0].contiguous(), ROUND[c.prec]).double()
        k, v = ROUND[c.prec](qkv[1].contiguous()).double(), ROUND[c.prec](qkv[2].contiguous()).double()
    s = (q @ k.transpose(-2, -1)) * 0.125
    p = torch.softmax(s, -1)
    ref = p @ v
    extra = U_P[c.prec] * (p @ v.abs())
    if P_FLOOR[c.prec]:
        # the f16 floor: a p below 2^-14 is rounded on the subnormal grid, an absolute error of up to 2^-25 in the units of the group's
        # fixed offset m_g (its first tile's row maximum). Moved to the common offset mn = max_g m_g it weighs 2^(m_g - mn), against
        # l = sum_k 2^(s_k - mn).
        s2 = s * LOG2E
        groups = key_groups(c)
        mg = [s2[..., a:min(a + 64, b)].amax(-1, keepdim=True) for a, b in groups]
        mn = functools.reduce(torch.maximum, mg)
        l = torch.exp2(s2 - mn).sum(-1, keepdim=True)
        fl = sum(torch.exp2(m - mn) * v[..., a:b, :].abs().sum(-2).unsqueeze(-2) for m, (a, b) in zip(mg, groups))
        extra = extra + P_FLOOR[c.prec] * fl / l
    to_rows = lambda t: t.transpose(1, 2).reshape(T, N, heads * 64)  # noqa: E731
    ref, extra = to_rows(ref), to_rows(extra)
    if c.fp8_inv:
        raw = ref * c.fp8_inv
        ref = raw.clamp(-448.0, 448.0)
        extra = extra * c.fp8_inv + 2.0 ** -24 * ref.abs()   # + the fp32 rounding of the fused inv_l * out_fp8_inv
        return ref, extra, raw
    return ref, extra, ref


def reference(c):
    """(fp64 reference [T, N, D], the bound's derived extra term, the unclamped scaled reference for the e4m3 form)."""
    return _reference(c.but(form="key-split" if c.form == "key-split" else "x", small=-1, asm=True).key())


def check(got, c, what):
    ref, extra, _ = reference(c)
    prec = FP8 if c.fp8_inv else c.prec
    r = assert_close_in(got.double().cpu(), ref, prec, A_MFMA, extra=extra if c.prec != F32 else None, what=what)
    print(f"[attention_ops] {what}: {r['beyond_plain']:.2%} of the elements lie beyond 0.5 ulp + A_MFMA max|ref| (inside the P term)")
    return r


def decode_fp8(b):
    return b.cpu().view(torch.float8_e4m3fn).float()


# ---------------------------------------------------------------------------------------------
# the kernel's arithmetic in fp32 (CPU), with the mutants
# ---------------------------------------------------------------------------------------------
P_CLAMP = 2.0 ** 11   # the `large_p_clamped` mutant: a pack that saturates where no ordinary row's p comes (they stay below 2^6)


def round_p(p, prec, mut=None):
    if mut == "large_p_clamped":
        p = p.clamp_max(P_CLAMP)
    if prec == BF16:
        return p.bfloat16().float()
    hi = p.half().float()                      # pack2_nosat: a plain conversion
    return hi if prec == F16 else hi + (p - hi).half().float()


def xcd_remap(nwg):
    q, r = nwg >> 3, nwg & 7
    return [(x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (b >> 3) for b in range(nwg) for x in [b & 7]]


def swap23(i):
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def emulate(c, mut=None, pad="zero"):
    """(the launch's output as the entry returns it, whether every row stayed inside the fast body's checks). `pad`: what a mutant that
    admits keys past N reads there -- "zero" / "poison": the staging's padding; "live": real k / v rows, the next (sequence, head)
    unit's first rows (what follows row N - 1 where the stride is exactly N; with one unit, fresh normal rows)."""
    T, N, heads, prec = c.T, c.N, c.heads, c.prec
    q, k, v = operands(c)
    if prec == F32:
        s = ((q.double() @ k.double().transpose(-2, -1)).float() * 0.125)
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = ((p / p.sum(-1, keepdim=True)).double() @ v.double()).float()
        return o.transpose(1, 2).reshape(T, N, heads * 64), True
    if mut == "q_scale_without_log2e":
        q = ROUND[prec](inputs(c).reshape(T, N, 3, heads, 64).permute(2, 0, 3, 1, 4)[0] * 0.125)
    groups = key_groups(c)
    leak = 0
    if mut == "key_N_admitted":
        leak = 1
    elif mut == "mask_in_wrong_group":
        leak = (-N) % 64
    if leak:  # the keys N .. N + leak of the last tile, with the padding's values
        if pad == "live" and T * heads > 1:
            kn, vn = (t.reshape(T * heads, N, 64).roll(-1, 0)[:, :leak].reshape(T, heads, leak, 64) for t in (k, v))
        elif pad == "live":
            g = torch.Generator().manual_seed(9000 + N)
            kn, vn = (ROUND[prec](torch.randn(1, 1, leak, 64, generator=g)) for _ in range(2))
        else:
            kn = vn = torch.full((T, heads, leak, 64), 0.0 if pad == "zero" else POISON[prec])
        k, v = torch.cat([k, kn], 2), torch.cat([v, vn], 2)
        groups = groups[:-1] + [(groups[-1][0], N + leak)]
    s = (q.double() @ k.double().transpose(-2, -1)).float()     # log2 units; the MFMA accumulates in fp32
    halves = ((torch.arange(s.shape[-1]) >> 3) & 1).bool()    # the lane half that holds a key: bit 3 of its index
    fast_ok, parts = True, []
    for a, b in groups:
        sg = s[..., a:b]
        m0 = sg[..., :64].amax(-1, keepdim=True)
        fast_ok = fast_ok and bool((m0.abs() <= 64.0).all())
        m = torch.zeros_like(m0) if prec == BF16 else m0
        p = torch.exp2(sg - m)
        pr = round_p(p, prec, mut)
        vg = v[..., a:b, :]
        if mut == "bits_2_3_not_swapped" and a == 0:   # sub-tile 1 of every tile of group 0: P of key i meets the V row of swap23(i)
            sw = torch.tensor([((i & ~31) | swap23(i & 31)) if (i & 32) else i for i in range(b - a)])
            vg = torch.where((sw < b - a)[:, None], vg[..., sw.clamp_max(b - a - 1), :], torch.zeros(()))
        o = (pr.double() @ vg.double()).float()
        src = pr if mut == "row_sum_of_rounded_p" else p
        hm = halves[a:b]
        l2 = torch.stack([src[..., ~hm].sum(-1), src[..., hm].sum(-1)], -1)   # [.., q, 2]: the two lane halves' row sums
        fast_ok = fast_ok and bool((l2 < FAST_SUM_MAX[prec]).all())
        parts.append((o, l2, m))
    o, l2, m = parts[0]
    if len(parts) == 2 and mut != "group_1_dropped":
        o1, l21, m1 = parts[1]
        if prec == BF16 or mut == "merge_without_common_offset":
            o, l2 = o + o1, l2 + l21
        else:
            mn = torch.maximum(m, m1)
            a_, b_ = torch.exp2(m - mn), torch.exp2(m1 - mn)
            o, l2 = o * a_ + o1 * b_, l2 * a_ + l21 * b_
    if mut == "no_cross_half_exchange":   # the lane half h writes the columns d with bit 2 = h
        l = l2[..., ((torch.arange(64) >> 2) & 1)]
    else:
        l = (l2[..., 0] + l2[..., 1]).unsqueeze(-1)
    inv_l = 1.0 / l
    if c.fp8_inv:
        inv8 = torch.tensor(c.fp8_inv, dtype=torch.float32)
        if mut == "e4m3_scale_after_rounding":
            y = (o * inv_l).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * inv8
        else:
            y = o * (inv_l * inv8)
        if mut != "e4m3_without_clamp":
            y = y.clamp(-448.0, 448.0)
        out = y.to(torch.float8_e4m3fn).view(torch.uint8)
        if mut == "e4m3_bytes_reversed":   # the 4-vector at columns 8 .. 11
            out = out.clone()
            out[..., 8:12] = out[..., 8:12].flip(-1)
    else:
        out = ROUND[prec](o * inv_l)
    out = out.transpose(1, 2).reshape(T, N, heads * 64)
    if mut in ("xcd_remap_identity", "query_block_1_at_block_0"):
        good, out = out, out.clone()
        rows, qb = c.qrows, c.qblocks
        items = [(u, b) for u in range(T * heads) for b in range(qb)]
        if mut == "xcd_remap_identity":
            moves = [(items[j], items[i]) for i, j in enumerate(xcd_remap(c.nwg))]      # block i's result lands where block j belongs
        else:
            moves = [((u, 1), (u, 0)) for u in range(T * heads)]
            out[:, rows:2 * rows] = 0.0
        for (us, bs), (ud, bd) in moves:
            n = min(N - bs * rows, N - bd * rows, rows)
            (ts, hs), (td, hd) = divmod(us, heads), divmod(ud, heads)
            out[td, bd * rows:bd * rows + n, hd * 64:(hd + 1) * 64] = good[ts, bs * rows:bs * rows + n, hs * 64:(hs + 1) * 64]
    return out, fast_ok


MUTANTS = ["key_N_admitted", "mask_in_wrong_group", "group_1_dropped", "merge_without_common_offset", "no_cross_half_exchange",
           "row_sum_of_rounded_p", "q_scale_without_log2e", "bits_2_3_not_swapped", "xcd_remap_identity", "query_block_1_at_block_0",
           "e4m3_without_clamp", "e4m3_scale_after_rounding", "e4m3_bytes_reversed", "large_p_clamped"]
_ks = lambda c: c.form == "key-split"  # noqa: E731
MUTANT_ACTIVE = {
    "key_N_admitted": lambda c: c.N % 64 != 0,                       # a full last tile has no key N
    "mask_in_wrong_group": lambda c: _ks(c) and c.N % 64 != 0,
    "group_1_dropped": _ks,
    "merge_without_common_offset": lambda c: _ks(c) and c.prec != BF16,
    "no_cross_half_exchange": lambda c: True,
    "row_sum_of_rounded_p": lambda c: True,
    "q_scale_without_log2e": lambda c: True,
    "bits_2_3_not_swapped": lambda c: c.N > 32,
    "xcd_remap_identity": lambda c: xcd_remap(c.nwg) != list(range(c.nwg)),
    "query_block_1_at_block_0": lambda c: c.qblocks > 1,
    "e4m3_without_clamp": lambda c: c.fp8_inv > 0 and c.vscale != 1.0,
    "e4m3_scale_after_rounding": lambda c: c.fp8_inv > 0,
    "e4m3_bytes_reversed": lambda c: c.fp8_inv > 0,
    "large_p_clamped": lambda c: c.kind == "spikes",                # only a planted key's p reaches the clamp
}
# Where the per-element bound cannot reject a mutant (the docstring says why, and what catches it instead). Both sides are asserted:
# the listed (mutant, case) pairs pass the bound, every other active pair is rejected.
LEAKS = ("key_N_admitted", "mask_in_wrong_group")
_one_zero_key_hides = lambda c: c.prec != F16X2 and c.N >= 577   # noqa: E731  (1 / (1.65 N) against the type's half-ulp + P term)
NOT_REJECTABLE = {
    ("key_N_admitted", "zero"): _one_zero_key_hides,
    ("mask_in_wrong_group", "zero"): lambda c: _one_zero_key_hides(c) and (-c.N) % 64 == 1,   # N = 1087: the whole leak is one key
    ("row_sum_of_rounded_p", None): lambda c: True,
}
CPU_CASES = [c for c in ALL_CASES if c.prec != F32 and (c.form != "plain" or (c.small == -1 and c.asm))]


def rejected(got, c):
    ref, extra, _ = reference(c)
    if got.dtype == torch.uint8:
        if bool(((got & 0x7F) == 0x7F).any()):
            return True
        got = decode_fp8(got)
    if not bool(torch.isfinite(got).all()):
        return True
    return rejects(got.double(), ref, FP8 if c.fp8_inv else c.prec, A_MFMA, extra, slack_beyond_extra=True)


@pytest.mark.parametrize("c", ALL_CASES, ids=cid)
def test_fp32_emulation_is_inside_the_bound(c):
    got, fast_ok = emulate(c)
    assert fast_ok, "the inputs leave the fast body's range: the launch would run the running-maximum body"
    if c.fp8_inv:
        assert not bool(((got & 0x7F) == 0x7F).any())
        got = decode_fp8(got)
    check(got, c, "emulation " + c.id)


def test_clamp_case_exceeds_the_e4m3_range_in_part():
    for c in FP8OUT:
        share = (reference(c)[2].abs() > 448.0).double().mean().item()
        assert (0.01 < share < 0.99) if c.vscale != 1.0 else share == 0.0, (c.id, share)


def test_spike_rows_carry_the_offsets_they_are_meant_to():
    """Group 1's fixed offset (f16) lies about SPIKE_LOG2 + the row's spread above group 0's on the first-tile rows, and the later-tile
    rows meet their key at an offset several log2 units below it -- all inside the fast body (asserted by the emulation test)."""
    c = SPIKES[1]
    q, k, _ = operands(c)
    s = (q[0, 0].double() @ k[0, 0].double().T)
    (a0, b0), (a1, b1) = key_groups(c)
    for i, (qi, ki) in enumerate(SPIKE_ROWS):
        assert a1 <= ki < b1 and s[qi].argmax().item() == ki
        m0, m1 = s[qi, a0:a0 + 64].max().item(), s[qi, a1:a1 + 64].max().item()
        top_others = s[qi][[j for j in range(c.N) if j != ki]].max().item()
        assert abs(s[qi, ki].item() - top_others - SPIKE_LOG2) < 0.25
        first_tile = ki < a1 + 64
        assert (m1 == s[qi, ki].item()) == first_tile and (i % 2 == 0) == first_tile
        assert (m1 - m0 > 8.0) if first_tile else (s[qi, ki].item() - m1 > 8.0)
    waves = {(qi // 64, (qi % 64) // 32) for qi, _ in SPIKE_ROWS}
    assert len(waves) == 4
    # the planted rows themselves (not only some row of the case) reject a merge that skips the common offset, in both half types;
    # the bound is the whole case's (A_MFMA on the case's max|ref|)
    for c in SPIKES[1:]:
        ref, extra, _ = reference(c)
        bound = 0.5 * close_check.ulp_T(ref.abs(), c.prec) * 2 + A_MFMA * ref.abs().max() + extra
        err = (emulate(c, "merge_without_common_offset")[0].double() - ref).abs()
        for qi, ki in SPIKE_ROWS[::2]:
            assert bool((err[0, qi] > bound[0, qi]).all()), (c.id, qi)
    # the later-tile planted rows themselves reject a P pack that mishandles their p ~ 2^14 (saturating at 2^11; the row sum is taken
    # from the unrounded p, as in the kernel): the planted key's own v, small as it is, then arrives 8 times too small. Most
    # elements of those rows fail (not all: an element whose planted |v| is below ~0.03 * 2^-10 stays inside the bound), no other row
    # does; in bf16 (offset 0) all four planted p reach the clamp.
    for c in SPIKES:
        ref, extra, _ = reference(c)
        bound = 0.5 * close_check.ulp_T(ref.abs(), c.prec) * 2 + A_MFMA * ref.abs().max() + extra
        bad = (emulate(c, "large_p_clamped")[0].double() - ref).abs() > bound
        large = SPIKE_ROWS if c.prec == BF16 else SPIKE_ROWS[1::2]
        for qi, _ in large:
            assert int(bad[0, qi].sum()) > 32, (c.id, qi)
        assert int(bad.sum()) == sum(int(bad[0, qi].sum()) for qi, _ in large), c.id


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_is_rejected_where_active(mut):
    """Every mutant on every case where it is not the identity: rejected per element, except on the (mutant, case) pairs of
    NOT_REJECTABLE, which are asserted to PASS the bound (so a change of either state is noticed). The two leak mutants run three
    times: the leaked keys hold the poison value, a live k / v row, and the zero padding's value."""
    active = [c for c in CPU_CASES if MUTANT_ACTIVE[mut](c)]
    assert active, mut
    clean = {c.id: emulate(c)[0] for c in active}
    for pad in (("poison", "live", "zero") if mut in LEAKS else (None,)):
        hidden = NOT_REJECTABLE.get((mut, pad), lambda c: False)
        blind = []
        for c in active:
            got, _ = emulate(c, mut, pad=pad) if pad else emulate(c, mut)
            assert not torch.equal(got, clean[c.id]), (mut, pad, c.id, "the mutant changes no bit: it is not active here")
            assert rejected(got, c) == (not hidden(c)), (mut, pad, c.id, "expected to pass the bound" if hidden(c) else "not rejected")
            blind += [c.id] if hidden(c) else []
        print(f"[attention_ops] {mut}{' / ' + pad if pad else ''}: active on {len(active)} cases, rejected on {len(active) - len(blind)}; "
              f"inside the bound, as listed, on {len(blind)}: {blind}")


@pytest.mark.parametrize("mut", LEAKS)
def test_leaked_zero_key_is_caught_by_the_poison_bits(mut):
    """A key admitted past N contributes p * 0 on zero padding: only the row sum grows, by 2^0 against l = sum_k e^(s_k) ~ 1.65 N, so
    the row moves by about 1 / (1.65 N) of itself (the module docstring). Where that is inside the bound (NOT_REJECTABLE, asserted
    above) the per-element check is blind. With the padding poisoned the same defect changes bits on EVERY active case (here: the
    emulation with poison against the emulation with zeros), which is what test_poisoned_padding_changes_no_bit compares on the device,
    and every such case is in POISON_CASES."""
    cases = [c for c in CPU_CASES if MUTANT_ACTIVE[mut](c)]
    assert any(NOT_REJECTABLE[(mut, "zero")](c) for c in cases)   # the gap is real
    poisoned = {c.id for c in POISON_CASES}
    for c in cases:
        assert c.id in poisoned, c.id
        zero, dirty = emulate(c, mut, pad="zero")[0], emulate(c, mut, pad="poison")[0]
        assert not torch.equal(zero, dirty), c.id


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def run(dev, c, poison=False):
    """One launch through md_op_attention_ex; asserts the form the launcher took."""
    from burn_depth_amd import _lib, ops
    lib = _lib.load()
    prev = lib.md_debug_attention_asm(1 if c.asm else 0)
    try:
        got = ops.attention_ex(dev, inputs(c).cuda(), c.heads, c.prec, seq_stride=c.seq_stride, kpad=c.kpad, out_fp8_inv=c.fp8_inv,
                               small=c.small, poison_pad=poison)
    finally:
        lib.md_debug_attention_asm(prev)
    f = ops.attention_last_form()
    assert f["form"] == c.form, (c.id, f)
    if c.form in ("plain", "fp8-out"):
        assert (f["grid"], f["QW"], f["KS"]) == (c.nwg, 4, 1), f
    elif c.form == "key-split":
        assert (f["grid"], f["QW"], f["KS"]) == (c.nwg, 2, 2), f
    return got


def check_gpu(dev, c):
    got = run(dev, c)
    if c.fp8_inv:
        assert got.dtype == torch.uint8 and not bool(((got & 0x7F) == 0x7F).any()), "an e4m3 NaN byte"
        ref, extra, raw = reference(c)
        b = got.cpu()
        sure = raw.abs() > 448.0 * (1 + 2.0 ** -4)   # beyond the last e4m3 tie: the clamp's value whatever the bound admits
        assert torch.equal(b[sure], torch.where(raw[sure] > 0, 0x7E, 0xFE).to(torch.uint8)), "the clamp must give +-448"
        got = decode_fp8(got)
    return check(got, c, c.id)


@pytest.mark.gpu
@pytest.mark.parametrize("c", PLAIN, ids=cid)
def test_plain_form(dev, c):
    check_gpu(dev, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", STRIDES, ids=cid)
def test_enlarged_strides(dev, c):
    check_gpu(dev, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", KEYSPLIT + SPIKES, ids=cid)
def test_key_split_form_and_plain_form_on_the_same_inputs(dev, c):
    check_gpu(dev, c)
    check_gpu(dev, c.but(form="plain", small=0))


@pytest.mark.gpu
@pytest.mark.parametrize("c", FP8OUT, ids=cid)
def test_e4m3_output_form(dev, c):
    check_gpu(dev, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", ASM, ids=cid)
def test_assembly_form_and_hip_kernel_at_577(dev, c):
    check_gpu(dev, c)
    check_gpu(dev, c.but(form="plain", asm=False))


@pytest.mark.gpu
@pytest.mark.parametrize("c", F32PATH, ids=cid)
def test_fp32_path(dev, c):
    check_gpu(dev, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", POISON_CASES, ids=cid)
def test_poisoned_padding_changes_no_bit(dev, c):
    clean, dirty = run(dev, c), run(dev, c, poison=True)
    assert torch.equal(clean, dirty)


@pytest.mark.gpu
def test_poison_flag_bit_is_the_descriptor_field(dev):
    from burn_depth_amd import ops
    c = PLAIN[0].but(T=2, heads=2, N=65)
    x = inputs(c).cuda()
    a = ops.attention_ex(dev, x, c.heads, c.prec | ops.POISON_PAD)
    assert torch.equal(a, ops.attention_ex(dev, x, c.heads, c.prec, poison_pad=True)) and torch.equal(a, ops.attention(dev, x, c.heads, c.prec))


@pytest.mark.gpu
def test_error_paths_of_the_descriptor_entry(dev):
    from burn_depth_amd import _lib, ops
    x = torch.randn(2, 70, 3 * 64, device="cuda")

    def fails(code, prec, **kw):
        with pytest.raises(_lib.MdError) as e:
            ops.attention_ex(dev, x, 1, prec, **kw)
        assert e.value.code == code, (prec, kw, e.value.code)

    fails(_lib.MD_ERR_UNSUPPORTED, F16, out_fp8_inv=FP8_INV)
    fails(_lib.MD_ERR_UNSUPPORTED, F16X2, out_fp8_inv=FP8_INV)
    fails(_lib.MD_ERR_INVALID_ARG, BF16, kpad=64)      # 70 keys need 128 columns
    fails(_lib.MD_ERR_INVALID_ARG, BF16, kpad=160)     # not a multiple of 64
    fails(_lib.MD_ERR_SHAPE, BF16, seq_stride=68)
    fails(_lib.MD_ERR_UNSUPPORTED, F32, poison_pad=True)
    fails(_lib.MD_ERR_UNSUPPORTED, F32 | ops.POISON_PAD)
