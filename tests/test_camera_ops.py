"""Operator tests of the Depth-Anything-v3 camera path alone: the one-workgroup-per-image camera encoder (`ops.camera_encode`,
md_op_camera_encode, with its pose encoding returned through `pose_out`), the three-launch camera decoder (`ops.camera_decode`) and the
pose -> matrices tail (`ops.pose_to_camera`), kernels/camera.hip, kernels/camera_math.h and pose_to_camera_kernel of kernels/ops.hip.
References are torch fp64 restatements of oracle/da3_ref.py (`pose_encoding`, `matrix_to_quaternion`, `approx_atan_positive`,
`camera_encode`, `camera_decode`) on the fp32 inputs widened; the kernel's fp32 literals (1e-6f, 0.2447f, 0.0663f, pi/4, pi/2) are
np.float32 values widened. The same functions evaluated in fp32 are the oracle bit for bit or to a last bit
(test_restatement_is_the_oracle) and carry the mutants. Every output buffer is the caller's and filled with a canary.

Where the bounds come from (u = 2^-24; none is taken from a GPU result):

* pose encoding, translation: -(m . t), a three-term fp32 dot in any order, fused or not: g3 sum_j |m_ij t_j|, g3 = 3u / (1 - 3u).
* pose encoding, quaternion, the branch the fp64 reference selects: arg = 1 +- m00 +- m11 +- m22 (three additions, error <= 3 u A,
  A = 1 + |m00| + |m11| + |m22|), s = 2 sqrt(arg) (sqrtf: 1 ulp = 2 u relative; the doubling is exact), so ds / s <= 1.5 u A / arg + 2 u
  = 6 u A / s^2 + 2 u. The component 0.25 s inherits that. A ratio component (a +- b) / (s + 1e-6): u for the numerator (ONE addition
  of two fp32 inputs, relative to its exact value, so an exact 0 stays 0), ds / s + u for the divisor, 2 u for the division: 6 u + 6 u A
  / s^2. Every component: |q| u (6 + 6 A / s^2). The masks multiply by exact 0 / 1 and the clamp keeps the unselected candidates finite.
  A rotation's selected branch has arg >= 1 (the four args sum to 4 and the selected one is the largest), s >= 2: the allowance is at
  most 12 u |q|. The seeded rotations keep |trace|, |m00 - m11|, |m00 - m22|, |m11 - m22| >= 1e-3, so fp32 and fp64 take the same branch;
  the threshold matrices are exact in fp32 (entries 0, +-1, or one circulant of three fp32 values), so the comparisons are exact in both
  and a kernel on the wrong side of a strict `>` differs by a whole quaternion (a sign flip of all four components).
* pose encoding, fov = 2 atan~(x), x = half / f (division: 2 u x), v = x on the small side, 1 / max(x, 1e-6) on the large side (a second
  division: 4 u v). f(v) = T1 - T2, T1 = pi/4 v (one rounding), T2 = v (v - 1)(0.2447 + 0.0663 v) (five roundings), one subtraction:
  u (|T1| + 5 |T2| + |f|), plus |f'| dv with |f'| <= pi/4 + 0.33 <= 1.12 on [0, 1], plus u |pi/2 - f| on the large side; times 2. At the
  seam both sides agree to second order in (x - 1) (f'(1) on either side), so a side picked differently one fp32 step from 1 costs
  ~1e-14. x = 0 (fx = inf) gives an exact 0: the clamp keeps the unselected side finite (mutant `atan_no_clamp`).
* encoder token [B, D]: a stack of fp32 LayerNorm / linear / softmax blocks has no useful derived constant. Per case, MEASURED ON THE
  CPU: a = max(8 max|oracle_fp32 - ref_fp64|, A_LN max|ref|). The 8 covers a second, independent summation order (lanes striding K
  with a butterfly reduction against torch's order), not a looser kernel; the CPU mutant test is the cap: every non-identity mutant
  lands outside a on at least one case. CPU-measured a per case (B, V, D, heads, depth):
    (1,1,8,1,0) 3.1e-06   (2,3,24,3,1) 3.4e-06   (3,5,40,5,1) 6.4e-06   (1,16,64,16,2) 5.2e-06   (1,16,136,68,1) 6.1e-06
    (1,7,384,6,1) 5.6e-06   (1,2,64,2,8) 6.1e-06 -- the floor A_LN max|ref| in every case (the fp32 oracle's error is 2.1e-7 .. 5.6e-7,
    times 8: 1.6e-6 .. 4.4e-6).
* decoder pose [B, 9]: two ReLU linears and three heads, the same rule with the floor A_MFMA max|ref|. CPU-measured a per case
  (B, din): (1,8) 2.0e-05, (2,40) 2.0e-05, (16,40) 3.1e-05, (17,40) 3.6e-05, (33,72) 4.5e-05, (2,768) 2.7e-05, zero_fov 2.0e-05 -- the floor
  in every case (the fp32 oracle's error is 2.6e-8 .. 4.8e-7).
* pose -> matrices (`#pragma clang fp contract(off)` in camera_math.h: the operation sequence is fixed), against fp64 OF THE RETURNED
  POSE: a rotation entry is 1 - 2 (a^2 + b^2) or 2 (ab +- cd): products u each, their sum u, the final subtraction u: u (4 Q + |R|), Q =
  x^2 + y^2 + z^2 + w^2 (a^2 + b^2 <= Q, |ab| + |cd| <= Q / 2). Translation -(r . t) on the ROUNDED r: sum_j |t_j| dR_j + g3 sum_j |r_j t_j|.
  Focal lengths half / (sin(a) / cos(a)), a = fov / 2 exact: sinf, cosf 1 ulp each (the HIP math API's accuracy table; quoted, that
  document is not part of this tree), two divisions: 8 u |ref|. fov = 0 gives sin / cos = 0 and a focal length of +inf in kernel and
  reference alike: the non-finite pattern must be equal, the finite elements within the bound.
* round trip pose_to_camera(pose_encode(E, K)) on the seeded rotations: the quaternion's 12 u |q| gives dR <= 48 u (diagonal: 4 (|y| dy
  + |z| dz)), the tail's own rounding 5 u, and E itself is a rotation ROUNDED to fp32 (entries off by u / 2, the extraction reads only
  some of them: dq <= 2 u, dR <= 16 u): 72 u per rotation entry, (72 + 8) u sum|t| for the translation column. K returns within the
  error of the atan polynomial: 1.5 x max |tan(atan~(x)) / x - 1| over the tested x in [0.25, 4], measured on the CPU in fp64 =
  1.5 x 3.96e-3 (ATAN_ROUND_TRIP below; it is computed, the figure is written here for the reader). A property of the reference's
  approximation, not of the kernel.

Mutants (fp32 on the CPU, through the checker the GPU results go through) and a case that rejects each:
  trace_ge: the cyclic permutation m01 = m12 = m20 = 1 (q_t = -q_z). m00_ge_m11 / m00_ge_m22 / m11_ge_m22: the 180 degree turns about
  (1,-1,0), (1,0,-1), (0,1,-1) / sqrt 2 (m00 = m11 > m22 etc.; the two candidates are each other's negative). On the matrices the issue
  names (identity, diag turns, cyclic permutations, 90 degree turns, 120 +- eps about (1,1,1)) these three mutants select a candidate
  that equals the reference's to ~1e-7 (|q| 1e-6 / s: the divisor's + 1e-6) or do not flip at all -- that is why the three face-diagonal
  turns are in the list. qx_sign / qy_sign / qz_sign: the seeded rotations of that branch. fov_swapped: every case (H != W, fx != fy).
  atan_lt: the IDENTITY (both sides give pi/4 at x = 1 exactly, 2 pi/4 = pi/2 in fp32 as in fp64) -- asserted NOT rejected.
  atan_no_clamp (an addition to the issue's list): fx = inf. ln_unbiased, no_softmax_scale, mean16, gelu_tanh, no_ls2, eps_swapped: the
  encoder cases with depth >= 1 (mean16: V != 16; no_softmax_scale: V > 1); `ENC_MUTANT_ACTIVE` states where each is the identity.
  no_fov_relu: the zero_fov decoder case. extr_R, t_not_negated, hw_swapped: every decoder case."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from close_check import A_LN, A_MFMA
from oracle import da3_ref

U = 2.0 ** -24
G3 = 3 * U / (1 - 3 * U)
c32 = lambda v: float(np.float32(v))  # noqa: E731 -- an fp32 literal of the kernel, widened
EPS6, C1, C2, PI4, PI2 = c32(1e-6), c32(0.2447), c32(0.0663), c32(math.pi / 4), c32(math.pi / 2)
CANARY = -7777.25
EPS_TOK, EPS_BLK = 1e-5, 1e-6


# ---------------------------------------------------------------------------------------------
# the definitions, in any dtype, with the mutants
# ---------------------------------------------------------------------------------------------
def atan_pos(x, mut=None):
    f = lambda v: PI4 * v - v * (v - 1.0) * (C1 + C2 * v)  # noqa: E731
    small, large = f(x), PI2 - f(1.0 / (x if mut == "atan_no_clamp" else torch.clamp_min(x, EPS6)))
    mk = ((x < 1.0) if mut == "atan_lt" else (x <= 1.0)).to(x.dtype)
    return small * mk + large * (1.0 - mk)


def quat_of(R, mut=None):
    """matrix_to_quaternion -> (q [N, 4] xyzw, branch [N] in 0..3 = t x y z, s [N] of the selected branch)"""
    m = lambda i, j: R[:, i, j]  # noqa: E731
    dt, one = R.dtype, torch.ones(R.shape[0], dtype=R.dtype)
    sg = lambda name: -1.0 if mut == name else 1.0  # noqa: E731
    gt = lambda a, b, name: ((a >= b) if mut == name else (a > b)).to(dt)  # noqa: E731
    trace = m(0, 0) + m(1, 1) + m(2, 2)
    s_t = torch.sqrt(torch.clamp_min(trace + one, EPS6)) * 2.0
    q_t = torch.stack([(m(2, 1) - m(1, 2)) / s_t, (m(0, 2) - m(2, 0)) / s_t, (m(1, 0) - m(0, 1)) / s_t, 0.25 * s_t], 1)
    s_x = torch.sqrt(torch.clamp_min(one + m(0, 0) - m(1, 1) - m(2, 2), EPS6)) * 2.0
    q_x = torch.stack([0.25 * s_x, (m(0, 1) + m(1, 0)) / (s_x + EPS6), (m(0, 2) + m(2, 0)) / (s_x + EPS6), (m(2, 1) - sg("qx_sign") * m(1, 2)) / (s_x + EPS6)], 1)
    s_y = torch.sqrt(torch.clamp_min(one + m(1, 1) - m(0, 0) - m(2, 2), EPS6)) * 2.0
    q_y = torch.stack([(m(0, 1) + m(1, 0)) / (s_y + EPS6), 0.25 * s_y, (m(1, 2) + m(2, 1)) / (s_y + EPS6), (m(0, 2) - sg("qy_sign") * m(2, 0)) / (s_y + EPS6)], 1)
    s_z = torch.sqrt(torch.clamp_min(one + m(2, 2) - m(0, 0) - m(1, 1), EPS6)) * 2.0
    q_z = torch.stack([(m(0, 2) + m(2, 0)) / (s_z + EPS6), (m(1, 2) + m(2, 1)) / (s_z + EPS6), 0.25 * s_z, (m(1, 0) - sg("qz_sign") * m(0, 1)) / (s_z + EPS6)], 1)
    mk_t = gt(trace, torch.zeros_like(trace), "trace_ge")
    mk_x = (one - mk_t) * gt(m(0, 0), m(1, 1), "m00_ge_m11") * gt(m(0, 0), m(2, 2), "m00_ge_m22")
    mk_y = (one - mk_t - mk_x) * gt(m(1, 1), m(2, 2), "m11_ge_m22")
    mk_z = one - mk_t - mk_x - mk_y
    q = q_t * mk_t[:, None] + q_x * mk_x[:, None] + q_y * mk_y[:, None] + q_z * mk_z[:, None]
    return q, (mk_x + 2 * mk_y + 3 * mk_z).long(), s_t * mk_t + s_x * mk_x + s_y * mk_y + s_z * mk_z


def pose_eval(extr, intr, H, W, dtype=torch.float64, mut=None):
    """pose_encoding: extr [N, 3, 4], intr [N, 3, 3] -> [N, 9]"""
    w2c, k = extr.to(dtype), intr.to(dtype)
    Rc2w = w2c[:, :, :3].transpose(1, 2)
    t = -(Rc2w @ w2c[:, :, 3:4])[:, :, 0]
    fov_w = atan_pos(c32(W / 2.0) / k[:, 0, 0], mut) * 2.0
    fov_h = atan_pos(c32(H / 2.0) / k[:, 1, 1], mut) * 2.0
    if mut == "fov_swapped":
        fov_h, fov_w = fov_w, fov_h
    return torch.cat([t, quat_of(Rc2w, mut)[0], fov_h[:, None], fov_w[:, None]], 1)


def pose_bound(extr, intr, H, W):
    """The derived allowance per element of pose_eval (module docstring), from fp64 quantities of the reference."""
    e = extr.double()
    m, t3 = e[:, :, :3].transpose(1, 2), e[:, :, 3]
    bt = G3 * (m.abs() @ t3.abs()[:, :, None])[:, :, 0]
    q, _, s = quat_of(m)
    A = 1.0 + m[:, 0, 0].abs() + m[:, 1, 1].abs() + m[:, 2, 2].abs()
    bq = q.abs() * (U * (6.0 + 6.0 * A / s ** 2))[:, None]

    def fov(x):
        small = x <= 1.0
        v = torch.where(small, x, 1.0 / torch.clamp_min(x, EPS6))
        T1, T2 = PI4 * v, v * (v - 1.0) * (C1 + C2 * v)
        f = T1 - T2
        b = 1.12 * torch.where(small, 2 * U * v, 4 * U * v) + U * (T1.abs() + 5 * T2.abs() + f.abs()) + torch.where(small, 0.0 * v, U * (PI2 - f).abs())
        return 2.0 * b

    k = intr.double()
    return torch.cat([bt, bq, fov(c32(H / 2.0) / k[:, 1, 1])[:, None], fov(c32(W / 2.0) / k[:, 0, 0])[:, None]], 1)


def enc_eval(extr, intr, Wd, c, dtype=torch.float64, mut=None):
    """camera_encode: extr [B, V, 3, 4], intr [B, V, 3, 3] -> [B, D]. c = (B, V, D, heads, depth, H, W)"""
    B, V, D, heads, depth, H, W = c
    hd = D // heads
    p = lambda n: Wd[f"camera_encoder.{n}"].to(dtype)  # noqa: E731
    lin = lambda n, t: F.linear(t, p(f"{n}.weight"), p(f"{n}.bias"))  # noqa: E731
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if mut == "gelu_tanh" else F.gelu
    eps_tok, eps_blk = (EPS_BLK, EPS_TOK) if mut == "eps_swapped" else (EPS_TOK, EPS_BLK)

    def ln(t, n, eps):
        if mut != "ln_unbiased":
            return F.layer_norm(t, (D,), p(f"{n}.gamma"), p(f"{n}.beta"), eps)
        cen = t - t.mean(-1, keepdim=True)
        return cen * torch.rsqrt((cen * cen).sum(-1, keepdim=True) / (D - 1) + eps) * p(f"{n}.gamma") + p(f"{n}.beta")

    pe = pose_eval(extr.reshape(B * V, 3, 4), intr.reshape(B * V, 3, 3), H, W, dtype).reshape(B, V, 9)
    x = ln(lin("pose_branch.fc2", gelu(lin("pose_branch.fc1", pe))), "token_norm", eps_tok)
    for i in range(depth):
        b = f"trunk.{i}"
        qkv = lin(f"{b}.attn.qkv", ln(x, f"{b}.norm1", eps_blk)).reshape(B, V, 3, heads, hd).permute(2, 0, 3, 1, 4)
        scale = 1.0 if mut == "no_softmax_scale" else hd ** -0.5
        a = torch.softmax((qkv[0] * scale) @ qkv[1].transpose(-1, -2), -1) @ qkv[2]
        x = x + p(f"{b}.ls1.gamma") * lin(f"{b}.attn.proj", a.transpose(1, 2).reshape(B, V, D))
        h = lin(f"{b}.mlp.fc2", gelu(lin(f"{b}.mlp.fc1", ln(x, f"{b}.norm2", eps_blk))))
        x = x + (h if mut == "no_ls2" else p(f"{b}.ls2.gamma") * h)
    x = ln(x, "trunk_norm", eps_tok)
    return x.sum(1) / 16.0 if mut == "mean16" else x.mean(1)


def p2c_eval(pose, H, W, dtype=torch.float64, mut=None):
    """pose_encoding_to_extri_intri: pose [B, 9] -> extr [B, 12] world-to-camera, intr [B, 9]"""
    pose = pose.to(dtype)
    t, (qx, qy, qz, qw), fov = pose[:, :3], pose[:, 3:7].unbind(1), pose[:, 7:9]
    R = torch.stack([torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)], 1),
                     torch.stack([2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)], 1),
                     torch.stack([2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], 1)], 1)
    Rt = R.transpose(1, 2)
    tr = Rt @ t[:, :, None]
    extr = torch.cat([R if mut == "extr_R" else Rt, tr if mut == "t_not_negated" else -tr], 2)
    tan_h = torch.sin(fov[:, 0] * 0.5) / torch.cos(fov[:, 0] * 0.5)
    tan_w = torch.sin(fov[:, 1] * 0.5) / torch.cos(fov[:, 1] * 0.5)
    h, w = (W, H) if mut == "hw_swapped" else (H, W)
    intr = torch.zeros(pose.shape[0], 3, 3, dtype=dtype)
    intr[:, 0, 0], intr[:, 0, 2] = (w / 2.0) / tan_w, w / 2.0
    intr[:, 1, 1], intr[:, 1, 2] = (h / 2.0) / tan_h, h / 2.0
    intr[:, 2, 2] = 1.0
    return extr.reshape(-1, 12), intr.reshape(-1, 9)


def p2c_bound(pose, H, W):
    """The derived allowances (extr [B, 12], intr [B, 9]) of the tail on `pose` (module docstring)."""
    p = pose.double()
    e, k = p2c_eval(pose, H, W)
    Q = (p[:, 3:7] ** 2).sum(1)
    R = e.reshape(-1, 3, 4)[:, :, :3]
    dR = U * (4.0 * Q[:, None, None] + R.abs())
    ta = p[:, :3].abs()
    dt = (dR * ta[:, None, :]).sum(2) + G3 * (R.abs() * ta[:, None, :]).sum(2)
    bk = 8 * U * torch.where(torch.isfinite(k), k.abs(), torch.zeros_like(k))
    bk[:, [1, 2, 3, 5, 6, 7, 8]] = 0.0
    return torch.cat([dR, dt[:, :, None]], 2).reshape(-1, 12), bk


def dec_eval(cam, Wd, H, W, dtype=torch.float64, mut=None):
    """camera_decode -> pose [B, 9]"""
    lin = lambda n, t: F.linear(t, Wd[f"camera_decoder.{n}.weight"].to(dtype), Wd[f"camera_decoder.{n}.bias"].to(dtype))  # noqa: E731
    h = F.relu(lin("backbone_2", F.relu(lin("backbone_1", cam.to(dtype)))))
    fov = lin("fc_fov", h)
    return torch.cat([lin("fc_t", h), lin("fc_qvec", h), fov if mut == "no_fov_relu" else F.relu(fov)], 1)


# ---------------------------------------------------------------------------------------------
# the checker (GPU results, the fp32 oracle and the mutants all go through it)
# ---------------------------------------------------------------------------------------------
def report(got, ref, bound):
    """bound: a tensor like ref, or a number. Non-finite reference elements must be matched exactly; the rest within the bound."""
    got, ref = got.double(), ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    fin = torch.isfinite(ref)
    pattern_ok = bool(torch.equal(torch.isfinite(got), fin) and torch.equal(got[~fin], ref[~fin]))
    err = torch.where(fin & torch.isfinite(got), (got - ref).abs(), torch.zeros_like(ref))
    bad = (err > bound) & fin
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return {"ok": pattern_ok and not bool(bad.any()), "max_err": err.max().item(), "worst_ratio": ratio.max().item(), "n_bad": int(bad.sum())}


def accept(got, ref, bound, what):
    r = report(got, ref, bound)
    print(f"[camera_ops] {what}: max err {r['max_err']:.3e}, worst err/bound {r['worst_ratio']:.3f}")
    assert r["ok"], f"{what}: {r['n_bad']} elements outside the bound (worst err/bound {r['worst_ratio']:.3f}) or a non-finite pattern that differs"
    return r


def rejects(got, ref, bound):
    return not report(got, ref, bound)["ok"]


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def quat_to_rot64(q):
    x, y, z, w = (q / q.norm(dim=1, keepdim=True)).double().unbind(1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def branch_margin(R):
    """The smallest of |trace|, |m00 - m11|, |m00 - m22|, |m11 - m22| (R fp32, evaluated in fp64)."""
    R = R.double()
    d0, d1, d2 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    return torch.stack([(d0 + d1 + d2).abs(), (d0 - d1).abs(), (d0 - d2).abs(), (d1 - d2).abs()], 1).min(1).values


_SEEDED = {}


def seeded_rotations(per_branch=50, seed=5):
    """Camera-to-world rotations (fp32) with every branch margin >= 1e-3, `per_branch` of each of the four branches, interleaved."""
    if (per_branch, seed) not in _SEEDED:
        g = torch.Generator().manual_seed(seed)
        R = quat_to_rot64(torch.randn(4000, 4, generator=g, dtype=torch.float64)).float()
        R = R[branch_margin(R) >= 1e-3]
        br = quat_of(R.double())[1]
        picks = [R[br == b][:per_branch] for b in range(4)]
        assert all(len(p) == per_branch for p in picks)
        _SEEDED[(per_branch, seed)] = torch.stack(picks, 1).reshape(-1, 3, 3)
    return _SEEDED[(per_branch, seed)]


def axis_turn(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    th = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def circulant_turn(deg):
    """A turn about (1,1,1)/sqrt 3 as ONE circulant of three fp32 values: its diagonals are equal bit for bit."""
    a, b, c = (float(np.float32(v)) for v in axis_turn((1, 1, 1), deg)[0])
    return torch.tensor([[a, b, c], [c, a, b], [b, c, a]], dtype=torch.float64)


def threshold_rotations():
    """name -> camera-to-world rotation exactly on a branch threshold, exact in fp32."""
    d = lambda *v: torch.diag(torch.tensor(v, dtype=torch.float64))  # noqa: E731
    P = torch.tensor([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=torch.float64)  # m02 = m10 = m21 = 1
    out = {"identity": d(1, 1, 1), "turn180_x": d(1, -1, -1), "turn180_y": d(-1, 1, -1), "turn180_z": d(-1, -1, 1),
           "cyclic_a": P, "cyclic_b": P.t().contiguous(),
           "turn90_x": axis_turn((1, 0, 0), 90).round(), "turn90_y": axis_turn((0, 1, 0), 90).round(), "turn90_z": axis_turn((0, 0, 1), 90).round(),
           "turn120_plus": circulant_turn(120 + 0.5), "turn120_minus": circulant_turn(120 - 0.5)}
    for name, axis in (("xy", (1, 1, 0)), ("x-y", (1, -1, 0)), ("xz", (1, 0, 1)), ("x-z", (1, 0, -1)), ("yz", (0, 1, 1)), ("y-z", (0, 1, -1))):
        out[f"turn180_{name}"] = axis_turn(axis, 180).round()   # m00 = m11 > m22 and its kin: the thresholds of the three `>` masks
    for R in out.values():
        assert torch.equal(R.float().double(), R)
    return {k: v.float() for k, v in out.items()}


def focal_specials(half):
    """Focal lengths around the seam x = half / f = 1 and on the far sides (fp32 values)."""
    h = np.float32(half)
    return [float(v) for v in (h, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1e9)), np.float32(2 * half) * np.float32(1e-3),
                               np.float32(2 * half) * np.float32(1e3), np.float32(2 * half) * np.float32(1e7))]


POSE_SIZES = [(48, 64), (37, 51)]  # H != W; the second: H * 0.5f and W * 0.5f are no integers


def pose_inputs(H, W):
    """-> names, extr [N, 3, 4] world-to-camera, intr [N, 3, 3]: the threshold rotations, the seeded ones, the intrinsics specials."""
    thr = threshold_rotations()
    Rc2w = torch.cat([torch.stack(list(thr.values())), seeded_rotations()])
    names = list(thr) + [f"seeded{i}" for i in range(len(Rc2w) - len(thr))]
    N = len(Rc2w)
    g = torch.Generator().manual_seed(17)
    t = torch.randn(N, 3, generator=g) * 2.0
    t[0] = 0.0
    fx = (torch.rand(N, generator=g) * 1.75 + 0.25) ** -1 * (W / 2.0)   # x = half / f in [0.25, 2]
    fy = (torch.rand(N, generator=g) * 3.75 + 0.25) ** -1 * (H / 2.0)   # x in [0.25, 4]
    sx, sy = focal_specials(W / 2.0), focal_specials(H / 2.0)
    fx[1:1 + len(sx)] = torch.tensor(sx)
    fy[2:2 + len(sy)] = torch.tensor(sy)
    fx[9] = math.inf                                                      # x = 0: the clamp keeps the large side finite
    extr = torch.cat([Rc2w.transpose(1, 2), t[:, :, None]], 2).contiguous()
    intr = torch.zeros(N, 3, 3)
    intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = fx, fy, W / 2.0, H / 2.0, 1.0
    return names, extr, intr


def seeded(shape, seed, kind="randn", k=1):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return torch.randn(*shape, generator=g) / math.sqrt(k)
    if kind == "gamma":
        return torch.rand(*shape, generator=g) + 0.5
    if kind == "ls":
        return torch.rand(*shape, generator=g) * 0.5 + 0.1
    return torch.randn(*shape, generator=g) * 0.1  # biases, betas


ENC_CASES = [(1, 1, 8, 1, 0), (2, 3, 24, 3, 1), (3, 5, 40, 5, 1), (1, 16, 64, 16, 2), (1, 16, 136, 68, 1), (1, 7, 384, 6, 1), (1, 2, 64, 2, 8)]
ENC_HW = (42, 70)
BLK_ORDER = ["norm1.gamma", "norm1.beta", "norm2.gamma", "norm2.beta", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
             "ls1.gamma", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias", "ls2.gamma"]
TOP_ORDER = ["pose_branch.fc1.weight", "pose_branch.fc1.bias", "pose_branch.fc2.weight", "pose_branch.fc2.bias", "token_norm.gamma", "token_norm.beta",
             "trunk_norm.gamma", "trunk_norm.beta"]
_ENC = {}


def enc_weights(D, depth, seed=100):
    shapes = {"pose_branch.fc1.weight": (D // 2, 9), "pose_branch.fc2.weight": (D, D // 2)}
    blk = {"attn.qkv.weight": (3 * D, D), "attn.proj.weight": (D, D), "mlp.fc1.weight": (4 * D, D), "mlp.fc2.weight": (D, 4 * D)}
    names = TOP_ORDER + [f"trunk.{i}.{n}" for i in range(depth) for n in BLK_ORDER]
    Wd = {}
    for j, n in enumerate(names):
        leaf = n.split(".", 2)[2] if n.startswith("trunk.") else n
        if n.endswith(".weight"):
            shp = shapes.get(leaf) or blk[leaf]
            Wd["camera_encoder." + n] = seeded(shp, seed + j, "randn", shp[1])
        elif n.endswith(".bias"):
            wshape = shapes.get(leaf[:-4] + "weight") or blk[leaf[:-4] + "weight"]
            Wd["camera_encoder." + n] = seeded((wshape[0],), seed + j, "bias")
        else:
            kind = "ls" if ".ls" in n else ("gamma" if n.endswith("gamma") else "bias")
            Wd["camera_encoder." + n] = seeded((D,), seed + j, kind)
    return Wd


def enc_case(case):
    """-> dict(c, Wd, extr, intr, ref fp64, oracle fp32, a): computed once per case, never changed."""
    if case not in _ENC:
        B, V, D, heads, depth = case
        H, W = ENC_HW
        Wd = enc_weights(D, depth)
        R = seeded_rotations()
        g = torch.Generator().manual_seed(1000 + B * 31 + V)
        idx = torch.randint(0, len(R), (B * V,), generator=g)
        t = torch.randn(B * V, 3, generator=g)
        extr = torch.cat([R[idx].transpose(1, 2), t[:, :, None]], 2).reshape(B, V, 3, 4).contiguous()
        intr = torch.zeros(B * V, 3, 3)
        intr[:, 0, 0] = (torch.rand(B * V, generator=g) * 1.75 + 0.25) ** -1 * (W / 2.0)
        intr[:, 1, 1] = (torch.rand(B * V, generator=g) * 1.75 + 0.25) ** -1 * (H / 2.0)
        intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = W / 2.0, H / 2.0, 1.0
        intr = intr.reshape(B, V, 3, 3)
        c = (B, V, D, heads, depth, H, W)
        ref = enc_eval(extr, intr, Wd, c)
        cfg = SimpleNamespace(vit=lambda: SimpleNamespace(embed_dim=D, ln_eps=EPS_BLK), cam_heads=heads, cam_ln_eps=EPS_TOK, cam_trunk_depth=depth)
        oracle = da3_ref.camera_encode(extr, intr, Wd, cfg, H, W)
        a = max(8.0 * (oracle.double() - ref).abs().max().item(), A_LN * ref.abs().max().item())
        _ENC[case] = dict(c=c, Wd=Wd, extr=extr, intr=intr, ref=ref, oracle=oracle, a=a)
    return _ENC[case]


DEC_CASES = [(1, 8), (2, 40), (16, 40), (17, 40), (33, 72), (2, 768), "zero_fov"]
DEC_HW = (45, 80)
DEC_ORDER = ["backbone_1.weight", "backbone_1.bias", "backbone_2.weight", "backbone_2.bias", "fc_t.weight", "fc_t.bias", "fc_qvec.weight", "fc_qvec.bias",
             "fc_fov.weight", "fc_fov.bias"]
_DEC = {}


def dec_case(case):
    """-> dict(Wd, cam, ref pose fp64, oracle dict fp32, a): computed once per case, never changed."""
    if case not in _DEC:
        zero = case == "zero_fov"
        B, din = (2, 40) if zero else case
        rows = {"backbone_1": din, "backbone_2": din, "fc_t": 3, "fc_qvec": 4, "fc_fov": 2}
        Wd = {}
        for j, (n, r) in enumerate(rows.items()):
            Wd[f"camera_decoder.{n}.weight"] = seeded((r, din), 300 + din + 2 * j, "randn", din)
            Wd[f"camera_decoder.{n}.bias"] = seeded((r,), 301 + din + 2 * j, "bias")
        Wd["camera_decoder.fc_fov.bias"] = torch.tensor([1.2, 0.9])     # fields of view around a radian
        if zero:  # the fov_h head far below zero with small weights: its ReLU gives exactly 0
            Wd["camera_decoder.fc_fov.weight"][0] *= 0.01
            Wd["camera_decoder.fc_fov.bias"][0] = -10.0
        cam = seeded((B, din), 400 + B + din)
        H, W = DEC_HW
        ref = dec_eval(cam, Wd, H, W)
        oracle = da3_ref.camera_decode(cam, Wd, H, W)
        opose = oracle["pose_encoding"][:, 0]
        a = max(8.0 * (opose.double() - ref).abs().max().item(), A_MFMA * ref.abs().max().item())
        _DEC[case] = dict(B=B, din=din, Wd=Wd, cam=cam, ref=ref, a=a,
                          oracle=(opose, oracle["extrinsics"][:, 0].reshape(B, 12), oracle["intrinsics"][:, 0].reshape(B, 9)))
    return _DEC[case]


def dec_check(pose, extr, intr, case, what, check=accept):
    """The decoder's checker: pose against fp64 within the case's allowance; extr / intr against fp64 of THAT pose within the tail's
    bound. check = accept (asserts) or rejects (-> True when any part is refused)."""
    d = dec_case(case)
    H, W = DEC_HW
    e64, k64 = p2c_eval(pose, H, W)
    be, bk = p2c_bound(pose, H, W)
    parts = [(pose, d["ref"], d["a"], "pose"), (extr, e64, be, "extr"), (intr, k64, bk, "intr")]
    res = [check(g, r, b, f"{what} {n}") if check is accept else check(g, r, b) for g, r, b, n in parts]
    return res if check is accept else any(res)


# ---------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------
def test_generator_reaches_every_branch():
    R = seeded_rotations()
    assert len(R) == 200 and (branch_margin(R) >= 1e-3).all()
    br64, br32 = quat_of(R.double())[1], quat_of(R)[1]
    assert torch.equal(br64, br32)
    assert all(int((br64 == b).sum()) >= 20 for b in range(4)), torch.bincount(br64)
    assert ((R.double() @ R.double().transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs() <= 4 * U).all()


def test_threshold_rotations_sit_on_the_thresholds():
    thr = threshold_rotations()
    br = {k: int(quat_of(v[None].double())[1]) for k, v in thr.items()}
    assert br["identity"] == 0 and (br["turn180_x"], br["turn180_y"], br["turn180_z"]) == (1, 2, 3)
    assert br["cyclic_a"] == br["cyclic_b"] == 3 and br["turn120_plus"] == 3 and br["turn120_minus"] == 0
    assert all(br[f"turn90_{a}"] == 0 for a in "xyz")
    for k in ("cyclic_a", "cyclic_b", "turn120_plus", "turn120_minus"):
        assert thr[k][0, 0] == thr[k][1, 1] == thr[k][2, 2]
    assert thr["cyclic_a"].diagonal().sum() == 0 and all(thr[f"turn90_{a}"].diagonal().sum() == 1 for a in "xyz")
    for k, eq in (("turn180_x-y", (0, 1)), ("turn180_x-z", (0, 2)), ("turn180_y-z", (1, 2))):
        assert thr[k][eq[0], eq[0]] == thr[k][eq[1], eq[1]] and thr[k].diagonal().sum() == -1


@pytest.mark.parametrize("H,W", POSE_SIZES)
def test_restated_pose_is_the_oracle(H, W):
    _, extr, intr = pose_inputs(H, W)
    assert torch.equal(pose_eval(extr, intr, H, W, torch.float32), da3_ref.pose_encoding(extr[None], intr[None], H, W)[0])


@pytest.mark.parametrize("case", ENC_CASES)
def test_restatement_is_the_oracle(case):
    d = enc_case(case)
    mine = enc_eval(d["extr"], d["intr"], d["Wd"], d["c"], torch.float32)
    assert (mine - d["oracle"]).abs().max() <= 4 * 2.0 ** -23 * d["oracle"].abs().max()


@pytest.mark.parametrize("case", DEC_CASES)
def test_restated_decoder_is_the_oracle(case):
    dd = dec_case(case)
    assert torch.equal(dec_eval(dd["cam"], dd["Wd"], *DEC_HW, torch.float32), dd["oracle"][0])
    e, k = p2c_eval(dd["oracle"][0], *DEC_HW, torch.float32)
    assert torch.equal(e, dd["oracle"][1]) and torch.equal(k, dd["oracle"][2])


@pytest.mark.parametrize("H,W", POSE_SIZES)
def test_checker_accepts_the_fp32_oracle_pose(H, W):
    _, extr, intr = pose_inputs(H, W)
    accept(da3_ref.pose_encoding(extr[None], intr[None], H, W)[0], pose_eval(extr, intr, H, W), pose_bound(extr, intr, H, W), f"oracle fp32 pose {H}x{W}")


@pytest.mark.parametrize("case", ENC_CASES)
def test_checker_accepts_the_fp32_oracle_encoder(case):
    d = enc_case(case)
    print(f"[camera_ops] encoder {case}: a = {d['a']:.3e} (max|ref| {d['ref'].abs().max():.3f})")
    accept(d["oracle"], d["ref"], d["a"], f"oracle fp32 encoder {case}")


@pytest.mark.parametrize("case", DEC_CASES)
def test_checker_accepts_the_fp32_oracle_decoder(case):
    d = dec_case(case)
    print(f"[camera_ops] decoder {case}: a = {d['a']:.3e} (max|ref| {d['ref'].abs().max():.3f})")
    dec_check(*d["oracle"], case, f"oracle fp32 decoder {case}")
    if case == "zero_fov":
        assert (d["oracle"][0][:, 7] == 0).all() and torch.isinf(d["oracle"][2][:, 4]).all() and (d["oracle"][2][:, 4] > 0).all()
        assert torch.isfinite(d["oracle"][2][:, 0]).all()


POSE_MUTANTS = {  # mutant -> a row of pose_inputs that must reject it (None: an identity, must NOT be rejected)
    "trace_ge": "cyclic_b", "m00_ge_m11": "turn180_x-y", "m00_ge_m22": "turn180_x-z", "m11_ge_m22": "turn180_y-z",
    "qx_sign": "seeded1", "qy_sign": "seeded2", "qz_sign": "seeded3", "fov_swapped": "seeded0", "atan_no_clamp": "turn120_plus", "atan_lt": None}   # (turn120_plus: the row with fx = inf)


@pytest.mark.parametrize("mutant", list(POSE_MUTANTS))
def test_checker_rejects_pose_mutants(mutant):
    """fp32 on the CPU. `atan_lt` (x < 1 for x <= 1) is the identity: both sides give pi/4 at x = 1 -- it is asserted NOT rejected."""
    for H, W in POSE_SIZES:
        names, extr, intr = pose_inputs(H, W)
        ref, bound = pose_eval(extr, intr, H, W), pose_bound(extr, intr, H, W)
        got = pose_eval(extr, intr, H, W, torch.float32, mutant)
        row = POSE_MUTANTS[mutant]
        if row is None:
            assert (intr[:, 0, 0] == W / 2.0).any() and (intr[:, 1, 1] == H / 2.0).any(), "the seam is not among the cases"
            assert not rejects(got, ref, bound), "atan_lt should be the identity: both sides give pi/4 at the seam"
        else:
            i = names.index(row)
            assert rejects(got[i:i + 1], ref[i:i + 1], bound[i:i + 1]), f"{mutant} passes on {row}"


ENC_MUTANTS = ["ln_unbiased", "no_softmax_scale", "mean16", "gelu_tanh", "no_ls2", "eps_swapped"]


def ENC_MUTANT_ACTIVE(mut, case):
    B, V, D, heads, depth = case
    if mut == "mean16":
        return V != 16
    if mut == "no_softmax_scale":
        return depth > 0 and V > 1 and D != heads   # one key: softmax = 1; hd = 1: the scale is 1
    if mut == "no_ls2":
        return depth > 0
    return True


@pytest.mark.parametrize("mutant", ENC_MUTANTS)
def test_checker_rejects_encoder_mutants(mutant):
    """fp32 on the CPU, per case: rejected wherever ENC_MUTANT_ACTIVE says the mutant is not the identity."""
    active = [c for c in ENC_CASES if ENC_MUTANT_ACTIVE(mutant, c)]
    assert active
    for case in ENC_CASES:
        d = enc_case(case)
        got = enc_eval(d["extr"], d["intr"], d["Wd"], d["c"], torch.float32, mutant)
        r = report(got, d["ref"], d["a"])
        print(f"[camera_ops] encoder mutant {mutant} {case}: err / a = {r['worst_ratio']:.1f}")
        assert r["ok"] != (case in active), f"{mutant} on {case}: rejected = {not r['ok']}"


@pytest.mark.parametrize("mutant", ["no_fov_relu", "extr_R", "t_not_negated", "hw_swapped"])
def test_checker_rejects_decoder_mutants(mutant):
    for case in DEC_CASES:
        d = dec_case(case)
        H, W = DEC_HW
        pose = dec_eval(d["cam"], d["Wd"], H, W, torch.float32, mutant)
        extr, intr = p2c_eval(pose, H, W, torch.float32, mutant)
        if mutant != "no_fov_relu" or case == "zero_fov":
            assert dec_check(pose, extr, intr, case, "", rejects), f"{mutant} passes on {case}"


def atan_round_trip_error():
    """max |tan(atan~(x)) / x - 1| over the tested x in [0.25, 4], fp64: the polynomial's own error, as a focal length sees it."""
    x = torch.linspace(0.25, 4.0, 30001, dtype=torch.float64)
    return (torch.tan(atan_pos(x)) / x - 1.0).abs().max().item()


ATAN_ROUND_TRIP = 1.5 * atan_round_trip_error()


def test_atan_round_trip_figure():
    print(f"[camera_ops] max |tan(atan~(x)) / x - 1| on [0.25, 4] = {ATAN_ROUND_TRIP / 1.5:.3e}")
    assert 1e-3 < ATAN_ROUND_TRIP / 1.5 < 1e-2


# ---------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def canary(*shape):
    return torch.full(shape, CANARY, device="cuda")


def enc_tensors(Wd, depth):
    top = [Wd["camera_encoder." + n].cuda() for n in TOP_ORDER]
    blocks = [[Wd[f"camera_encoder.trunk.{i}.{n}"].cuda() for n in BLK_ORDER] for i in range(depth)]
    return top, blocks


def run_encoder(dev, d, extr=None, intr=None, pose=False):
    from burn_depth_amd import ops
    B, V, D, heads, depth, H, W = d["c"]
    extr, intr = (d["extr"] if extr is None else extr), (d["intr"] if intr is None else intr)
    B = extr.shape[0]
    top, blocks = enc_tensors(d["Wd"], depth)
    out, pose_out = canary(B, D), (canary(B, V, 9) if pose else None)
    ops.camera_encode(dev, extr.cuda(), intr.cuda(), top, blocks, heads=heads, H=H, W=W, eps_tok=EPS_TOK, eps_blk=EPS_BLK, out=out, pose_out=pose_out)
    assert not (out == CANARY).any()
    return (out.cpu(), pose_out.cpu()) if pose else out.cpu()


def gpu_pose(dev, extr, intr, H, W):
    """The kernel's pose encoding of N cameras: images of 16 views through a width-8, depth-0 encoder."""
    N = extr.shape[0]
    assert N % 16 == 0
    d = dict(c=(N // 16, 16, 8, 1, 0, H, W), Wd=enc_weights(8, 0))
    out, pose = run_encoder(dev, d, extr.reshape(N // 16, 16, 3, 4), intr.reshape(N // 16, 16, 3, 3), pose=True)
    assert not (pose == CANARY).any()
    return pose.reshape(N, 9)


def padded16(extr, intr):
    n = (-extr.shape[0]) % 16
    return torch.cat([extr, extr[:n]]), torch.cat([intr, intr[:n]])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", POSE_SIZES)
def test_pose_encoding_against_fp64(dev, H, W):
    """Threshold rotations (the selected branch must be the fp64 reference's: the wrong one differs by a whole quaternion), the seeded
    rotations of every branch, the focal lengths at and around the atan seam and on the far sides."""
    names, extr, intr = pose_inputs(H, W)
    N = len(names)
    e, k = padded16(extr, intr)
    got = gpu_pose(dev, e, k, H, W)[:N]
    ref, bound = pose_eval(extr, intr, H, W), pose_bound(extr, intr, H, W)
    nthr = len(threshold_rotations())
    accept(got[:nthr], ref[:nthr], bound[:nthr], f"pose {H}x{W} threshold rotations")
    accept(got[nthr:], ref[nthr:], bound[nthr:], f"pose {H}x{W} seeded rotations")
    for part, sl in (("t", slice(0, 3)), ("quat", slice(3, 7)), ("fov", slice(7, 9))):
        accept(got[:, sl], ref[:, sl], bound[:, sl], f"pose {H}x{W} {part}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENC_CASES)
def test_encoder_against_fp64(dev, case):
    d = enc_case(case)
    got = run_encoder(dev, d)
    print(f"[camera_ops] encoder {case}: a = {d['a']:.3e}")
    accept(got, d["ref"], d["a"], f"encoder {case}")
    if case[4] == 0:  # no trunk: the mean over views of trunk_norm(token_norm(PoseBranch)), stated on its own
        B, V, D, heads, depth, H, W = d["c"]
        p = lambda n: d["Wd"]["camera_encoder." + n].double()  # noqa: E731
        pe = pose_eval(d["extr"].reshape(B * V, 3, 4), d["intr"].reshape(B * V, 3, 3), H, W).reshape(B, V, 9)
        x = F.linear(F.gelu(F.linear(pe, p("pose_branch.fc1.weight"), p("pose_branch.fc1.bias"))), p("pose_branch.fc2.weight"), p("pose_branch.fc2.bias"))
        x = F.layer_norm(F.layer_norm(x, (D,), p("token_norm.gamma"), p("token_norm.beta"), EPS_TOK), (D,), p("trunk_norm.gamma"), p("trunk_norm.beta"), EPS_TOK)
        accept(got, x.mean(1), d["a"], f"encoder {case} against the no-trunk formula")


@pytest.mark.gpu
def test_encoder_image_is_independent_of_its_batch(dev):
    """One image's token is bit-identical alone and as image 0, 1, 2 of a B = 3 call with the same views."""
    d = enc_case((3, 5, 40, 5, 1))
    e1, k1 = d["extr"][1:2], d["intr"][1:2]
    alone = run_encoder(dev, d, e1, k1)
    three = run_encoder(dev, d, e1.expand(3, -1, -1, -1).contiguous(), k1.expand(3, -1, -1, -1).contiguous())
    for i in range(3):
        assert torch.equal(three[i], alone[0]), f"image {i} of 3 differs from the image alone"
    assert torch.equal(run_encoder(dev, d)[1], alone[0])


def run_decoder(dev, case, rows=None, want=(True, True)):
    from burn_depth_amd import ops
    d = dec_case(case)
    cam = d["cam"] if rows is None else d["cam"][rows]
    B = cam.shape[0]
    w = [d["Wd"]["camera_decoder." + n].cuda() for n in DEC_ORDER]
    pose, extr, intr = canary(B, 9), canary(B, 12), canary(B, 9)
    ops.camera_decode(dev, cam.cuda().contiguous(), w, *DEC_HW, pose, extr if want[0] else None, intr if want[1] else None)
    assert not (pose == CANARY).any()
    for t, wanted in ((extr, want[0]), (intr, want[1])):
        assert not (t == CANARY).any() if wanted else bool((t == CANARY).all())
    return pose.cpu(), extr.cpu(), intr.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEC_CASES)
def test_decoder_against_fp64(dev, case):
    d = dec_case(case)
    pose, extr, intr = run_decoder(dev, case)
    print(f"[camera_ops] decoder {case}: a = {d['a']:.3e}")
    dec_check(pose, extr, intr, case, f"decoder {case}")
    if case == "zero_fov":  # relu gives exactly 0 -> sin / cos = 0 -> a focal length of +inf, in kernel and reference alike
        assert (pose[:, 7] == 0).all() and torch.isinf(intr[:, 4]).all() and (intr[:, 4] > 0).all() and torch.isfinite(intr[:, 0]).all()


@pytest.mark.gpu
def test_decoder_row_is_independent_of_its_batch(dev):
    """Row b of the B = 33 call (three chunks of the batch loop) is bit-identical to the B = 1 call on that row."""
    full = run_decoder(dev, (33, 72))
    for b in (0, 15, 16, 31, 32):
        one = run_decoder(dev, (33, 72), rows=slice(b, b + 1))
        for f, o, n in zip(full, one, ("pose", "extr", "intr")):
            assert torch.equal(f[b], o[0]), f"row {b}: {n} differs between B = 33 and B = 1"


@pytest.mark.gpu
def test_decoder_null_outputs(dev):
    full = run_decoder(dev, (2, 40))
    for want in ((True, False), (False, True), (False, False)):
        pose, extr, intr = run_decoder(dev, (2, 40), want=want)   # (asserts the skipped buffer's canary)
        assert torch.equal(pose, full[0])
        assert not want[0] or torch.equal(extr, full[1])
        assert not want[1] or torch.equal(intr, full[2])


def run_p2c(dev, pose, want=(True, True)):
    from burn_depth_amd import ops
    B = pose.shape[0]
    extr, intr = canary(B, 12), canary(B, 9)
    ops.pose_to_camera(dev, pose.cuda().contiguous(), *DEC_HW, extr if want[0] else None, intr if want[1] else None)
    for t, wanted in ((extr, want[0]), (intr, want[1])):
        assert not (t == CANARY).any() if wanted else bool((t == CANARY).all())
    return extr.cpu(), intr.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65])
def test_pose_to_camera_against_fp64(dev, B):
    """Random unnormalised quaternions; one thread per pose in blocks of 64."""
    g = torch.Generator().manual_seed(70 + B)
    pose = torch.cat([torch.randn(B, 3, generator=g) * 3, torch.randn(B, 4, generator=g) * 1.5, torch.rand(B, 2, generator=g) * 2.4 + 0.2], 1)
    extr, intr = run_p2c(dev, pose)
    e64, k64 = p2c_eval(pose, *DEC_HW)
    be, bk = p2c_bound(pose, *DEC_HW)
    accept(extr, e64, be, f"pose_to_camera B={B} extr")
    accept(intr, k64, bk, f"pose_to_camera B={B} intr")
    for want in ((True, False), (False, True), (False, False)):
        part = run_p2c(dev, pose, want)   # (asserts the skipped buffer's canary)
        assert not want[0] or torch.equal(part[0], extr)
        assert not want[1] or torch.equal(part[1], intr)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(33, 72), "zero_fov"])
def test_pose_to_camera_is_the_decoders_tail(dev, case):
    """kernels/ops.h: the stand-alone kernel and the decoder's tail "produce the same bits" (one device function, contraction off)."""
    pose, extr, intr = run_decoder(dev, case)
    e, k = run_p2c(dev, pose)
    assert torch.equal(e, extr) and torch.equal(k, intr)
    be, bk = p2c_bound(pose, *DEC_HW)
    e64, k64 = p2c_eval(pose, *DEC_HW)
    accept(e, e64, be, f"pose_to_camera on the decoder's poses {case} extr")
    accept(k, k64, bk, f"pose_to_camera on the decoder's poses {case} intr")


@pytest.mark.gpu
def test_pose_round_trip(dev):
    """pose_to_camera(pose_encode(E, K)) returns E within the quaternion bound and K within the atan polynomial's own error."""
    H, W = DEC_HW
    R = seeded_rotations()
    g = torch.Generator().manual_seed(23)
    N = len(R) // 16 * 16
    t = torch.randn(N, 3, generator=g) * 2.0
    extr = torch.cat([R[:N].transpose(1, 2), t[:, :, None]], 2).contiguous()
    intr = torch.zeros(N, 3, 3)
    intr[:, 0, 0] = (torch.rand(N, generator=g) * 3.75 + 0.25) ** -1 * (W / 2.0)   # x in [0.25, 4]: ATAN_ROUND_TRIP's range
    intr[:, 1, 1] = (torch.rand(N, generator=g) * 3.75 + 0.25) ** -1 * (H / 2.0)
    intr[:, 0, 2], intr[:, 1, 2], intr[:, 2, 2] = W / 2.0, H / 2.0, 1.0
    pose = gpu_pose(dev, extr, intr, H, W)
    e, k = run_p2c(dev, pose)
    be = torch.full((N, 3, 4), 72 * U, dtype=torch.float64)
    be[:, :, 3] = (72 + 8) * U * pose[:, :3].double().abs().sum(1)[:, None]
    accept(e, extr.reshape(N, 12), be.reshape(N, 12), "round trip extr")
    accept(k, intr.reshape(N, 9), ATAN_ROUND_TRIP * intr.reshape(N, 9).double().abs() * torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 0.0]), "round trip intr")


@pytest.mark.gpu
def test_refusals_start_no_work(dev):
    """The launchers' own codes; the outputs keep their canary."""
    from burn_depth_amd import _lib, ops
    d8, d64 = enc_case((1, 1, 8, 1, 0)), enc_case((1, 2, 64, 2, 8))

    def enc(d, D, heads, **kw):
        top, blocks = enc_tensors(d["Wd"], d["c"][4])
        out = canary(1, D)
        with pytest.raises(_lib.MdError) as e:
            ops.camera_encode(dev, d["extr"].cuda(), d["intr"].cuda(), top, blocks, heads=heads, H=42, W=70, eps_tok=EPS_TOK, eps_blk=EPS_BLK, out=out, **kw)
        assert (out == CANARY).all()
        return e.value.code

    assert enc(d8, 8, 1, V=0) == _lib.MD_ERR_UNSUPPORTED
    assert enc(d8, 8, 1, V=17) == _lib.MD_ERR_UNSUPPORTED
    assert enc(d8, 12, 1) == _lib.MD_ERR_INVALID_ARG          # D % 8
    assert enc(d8, 8, 3) == _lib.MD_ERR_INVALID_ARG           # D % heads
    assert enc(d64, 64, 2, depth=9) == _lib.MD_ERR_INVALID_ARG
    dd = dec_case((2, 40))
    w = [dd["Wd"]["camera_decoder." + n].cuda() for n in DEC_ORDER]
    for cam, kw in ((torch.zeros(2, 6, device="cuda"), {}), (dd["cam"].cuda(), {"B": 0})):   # din % 4, B = 0
        pose, extr, intr = canary(2, 9), canary(2, 12), canary(2, 9)
        with pytest.raises(_lib.MdError) as e:
            ops.camera_decode(dev, cam, w, *DEC_HW, pose, extr, intr, **kw)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        assert (pose == CANARY).all() and (extr == CANARY).all() and (intr == CANARY).all()
