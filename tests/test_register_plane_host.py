"""CPU-only: the point-to-plane form of the registration (`kernels/register_math.h`) before it meets a GPU.
  1. a host program (tests/native/register_plane_host.cpp) runs the header's lines sequentially, with a literal O(N T) nearest
     search and the fixed sum tree as literal loops, under the address and undefined-behaviour sanitizers: its bits are
     `pipeline.register_points(target_normals=)`'s.
  2. without target_normals the reference gives the bits it gave before the quaternion lines moved into a helper
     (tests/golden/register_point_form.json, recorded from the commit before the point-to-plane form).
  3. the Cholesky solve agrees with numpy.linalg.solve on the same system, and 64 composed increments stay orthonormal.
  4. on three perpendicular planes sampled at different places the plane metric recovers a motion the point metric does not.
  5. degenerate systems are status 3, too few usable pairs status 2.
  6. the refusals of the reference."""
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from burn_depth_amd import pipeline as P  # noqa: E402
from test_register_host import IDENTITY, _hex, _motion, _move  # noqa: E402
from test_register_host import cases as point_cases  # noqa: E402

f32, f64 = np.float32, np.float64
# Largest entry difference between the transform `register_solve_plane` composes and the one composed from numpy.linalg.solve's
# solution of the same M x = b, over the first-pass sums of the seeded cases below, as measured on the CPU (test 3 prints it);
# the test asserts 16 times it, the margin DESIGN 12.14 uses for its Jacobi solve. Both are f64 solves of one 6x6 system.
SOLVE_VS_NUMPY = 2.220e-16
# Largest |R^T R - I| entry after 64 composed increments of 0.5 degrees, measured the same way; asserted at 16 times it.
ORTHO_AFTER_64 = 2.232e-14
# Test 4's errors of the plane metric against the known motion, measured on the CPU (the test prints them): the largest entry
# difference of the rotation, and of the translation, after K = 20 rounds (the point metric on the same clouds: 2.178e-3 and
# 4.796e-3). What is left comes from pairs across the faces' edges, which no normal gate removes. Asserted at 16 times them.
CORNER_ROT_ERR = 2.441e-4
CORNER_TRANS_ERR = 7.591e-4


def _bumpy(n, seed):
    """n rows on test_register_host's bumpy height field over [-1, 1]^2 and their exact unit normals"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1, 1, (n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.3 * np.sin(2.1 * x) * np.cos(1.7 * y) + 0.2 * x * y
    fx = 0.63 * np.cos(2.1 * x) * np.cos(1.7 * y) + 0.2 * y
    fy = -0.51 * np.sin(2.1 * x) * np.sin(1.7 * y) + 0.2 * x
    nrm = np.stack([-fx, -fy, np.ones(n)], 1)
    return np.concatenate([xy, z[:, None]], 1).astype(f32), nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _turn(A, n):
    return (np.asarray(n, f64) @ A[:9].reshape(3, 3).T).astype(f32)


def cases():
    """(name, xyz, target, target_normals, radius, K, init, min_pairs, rot_eps, trans_eps), seeded; shared with the GPU tests.
    Read-only."""
    src, src_n = _bumpy(600, 1)
    A = _motion([1, 2, 3], 3.0, [0.03, -0.02, 0.04])
    moved, moved_n = _move(A, src), _turn(A, src_n)
    rng = np.random.default_rng(7)
    oth, oth_n = _bumpy(500, 2)
    other = _move(A, oth) + rng.normal(0, 0.01, (500, 3)).astype(f32)
    bad_src = np.concatenate([src[:300], [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 3e30], [-np.inf, 1, 1]]]).astype(f32)
    bad_tgt = np.concatenate([[[0, np.nan, 0], [np.inf, 0, 0], [0, 3e30, 0]], moved[:350]]).astype(f32)
    bad_tgt_n = np.concatenate([[[0, 0, 1]] * 3, moved_n[:350]]).astype(f32)
    holes = moved_n.copy()  # normals a pair cannot use: NaN, infinite, all zero (what the point path writes without a normal)
    holes[0::7] = [np.nan, 0, 1]
    holes[1::7] = [0, 0, 0]
    holes[2::49] = [0, np.inf, 0]
    holes[3::49] = [-0.0, 0.0, -0.0]
    dupes = np.concatenate([moved[:200], moved[:200], moved[100:150]]).astype(f32)
    dupes_n = np.concatenate([moved_n[:200], moved_n[:200], moved_n[100:150]]).astype(f32)
    up = np.tile(np.array([[0, 0, 1]], f32), (600, 1))
    out = [("moved copy", src, moved, moved_n, 0.3, 8, None, 6, 0.0, 0.0),
           ("other draw", src, other, _turn(A, oth_n), 0.25, 6, None, 6, 0.0, 0.0),
           ("one round", src, other, _turn(A, oth_n), 0.25, 1, None, 6, 0.0, 0.0),
           ("init", src, moved, moved_n, 0.2, 4, _motion([0, 1, 0], 2.0, [0.02, 0.0, 0.03]), 6, 0.0, 0.0),
           ("stops early", src, moved, moved_n, 0.3, 24, None, 6, 1e-7, 1e-7),
           ("too few pairs", src[:40], moved[:40], moved_n[:40], 0.3, 5, _motion([1, 0, 0], 1.0, [0.01, 0, 0]), 41, 0.0, 0.0),
           ("bad rows", bad_src, bad_tgt, bad_tgt_n, 0.3, 5, None, 6, 0.0, 0.0),
           ("unusable normals", src, moved, holes, 0.3, 5, None, 6, 0.0, 0.0),
           ("duplicate targets", src[:300], dupes, dupes_n, 0.3, 4, None, 6, 0.0, 0.0),
           ("single direction", src, moved, up, 0.3, 4, _motion([0, 0, 1], 1.0, [0.0, 0.01, 0.0]), 6, 0.0, 0.0),
           ("one target row", src[:80], moved[:1], up[:1], 2.0, 3, None, 6, 0.0, 0.0),
           ("no target", src[:50], np.zeros((0, 3), f32), np.zeros((0, 3), f32), 0.3, 2, None, 6, 0.0, 0.0),
           ("no rows", np.zeros((0, 3), f32), moved[:50], moved_n[:50], 0.3, 2, None, 6, 0.0, 0.0)]
    two, two_n = _bumpy(1500, 5)
    out.append(("two tiles", _bumpy(4097 + 300, 4)[0], _move(A, two), _turn(A, two_n), 0.2, 2, None, 6, 0.0, 0.0))
    for c in out:
        for a in c[1:4]:
            a.setflags(write=False)
    return out


def run_case(c, **kw):
    _, xyz, target, tn, radius, K, init, min_pairs, rot_eps, trans_eps = c
    return P.register_points(xyz, target, radius, iterations=K, init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps,
                             target_normals=tn, **kw)


# ---- 1 ----
def test_the_header_run_sequentially_on_the_host_equals_the_numpy_reference(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "burn_depth_amd", "csrc")
    exe = str(tmp_path / "register_plane_host")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + csrc, os.path.join(ROOT, "tests", "native", "register_plane_host.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    cs, paths = cases(), []
    for i, (_, xyz, target, tn, radius, K, init, min_pairs, rot_eps, trans_eps) in enumerate(cs):
        paths.append(str(tmp_path / f"clouds{i}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(np.array([len(xyz), len(target), K, min_pairs], np.int32).tobytes())
            f.write(np.array([radius], f32).tobytes())
            f.write(np.array([rot_eps, trans_eps], f64).tobytes())
            f.write(np.asarray(IDENTITY if init is None else init, f64).tobytes())
            f.write(np.ascontiguousarray(xyz, f32).tobytes())
            f.write(np.ascontiguousarray(target, f32).tobytes())
            f.write(np.ascontiguousarray(tn, f32).tobytes())
    run = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cs)
    seen = set()
    for line, c in zip(lines, cs):
        ref = run_case(c)
        seen.add(int(ref.stats[1]))
        head = (f"A {_hex(ref.transform)} pairs " + " ".join(str(v) for v in ref.pairs.tolist()) + f" sum_d2 {_hex(ref.sum_d2)} sum_r2 {_hex(ref.sum_r2)}"
                + " stats " + " ".join(str(v) for v in ref.stats.tolist()) + f" dropped {ref.dropped} rows")
        rows = "".join(f" {n} {d:08x} {x:08x} {y:08x} {z:08x}" for n, d, (x, y, z) in
                       zip(ref.nearest.tolist(), ref.dist2.view(np.uint32).tolist(), ref.xyz.view(np.uint32).tolist()))
        got_head = line[:len(head)]
        assert got_head == head, (c[0], got_head, head)
        assert line == head + rows, c[0]
    assert seen == {0, 1, 2, 3}  # the cases reach every status


# ---- 2 ----
def _record(r):
    """what tests/golden/register_point_form.json holds of one result"""
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()  # noqa: E731
    return dict(transform=_hex(r.transform), pairs=r.pairs.tolist(), sum_d2=_hex(r.sum_d2), stats=r.stats.tolist(), dropped=int(r.dropped),
                nearest=digest(r.nearest), dist2=digest(r.dist2), xyz=digest(r.xyz), normals=digest(r.normals))


def test_point_form_keeps_the_bits_it_had_before_the_quaternion_helper():
    """The golden file was written by this `_record` from the reference as it stood before the point-to-plane form, over
    test_register_host.py's cases with the seeded normals below."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "register_point_form.json")))
    cs = point_cases()
    assert sorted(golden) == sorted(c[0] for c in cs)
    for c in cs:
        _, xyz, target, radius, K, init, min_pairs, rot_eps, trans_eps = c
        normals = np.random.default_rng(5).normal(size=(len(xyz), 3)).astype(f32)
        r = P.register_points(xyz, target, radius, iterations=K, init=init, min_pairs=min_pairs, rot_eps=rot_eps, trans_eps=trans_eps, normals=normals)
        assert r.sum_r2 is None
        assert _record(r) == golden[c[0]], c[0]
        if c[0] in ("moved copy", "bad rows"):  # the default min_pairs is still 3
            d = P.register_points(xyz, target, radius, iterations=K, init=init, rot_eps=rot_eps, trans_eps=trans_eps, normals=normals)
            assert _record(d) == golden[c[0]], c[0]


# ---- 3 ----
def _first_pass_sums(c):
    """the usable pair count and the 29 sums of the first pass: one round's history and a solve-free read of the leaves"""
    _, xyz, target, tn, radius, _, init, *_ = c
    A = IDENTITY if init is None else np.asarray(init, f64)
    p, q, n = np.asarray(xyz, f32), np.asarray(target, f64), np.asarray(tn, f64)
    ref = P.register_points(xyz, target, radius, iterations=1, init=init, min_pairs=1 << 30, target_normals=tn)  # status 2: only the pass
    j = ref.nearest
    use = (j >= 0)
    use[use] = np.isfinite(tn[j[use]]).all(1) & (tn[j[use]] != 0).any(1)
    m = ref.xyz[use].astype(f64)
    nn, d = n[j[use]], q[j[use]] - m
    J = np.concatenate([np.cross(m, nn), nn], 1)
    r = (d * nn).sum(1)
    return int(use.sum()), J.T @ J, J.T @ r, A


def _compose(x, A):
    """the increment (w, tau) onto A, in plain numpy: the rotation of the quaternion (1, w/2) normalised"""
    q = np.concatenate([[1.0], 0.5 * x[:3]])
    w, a, b, c = q / np.linalg.norm(q)
    dR = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                   [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                   [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])
    return np.concatenate([(dR @ A[:9].reshape(3, 3)).reshape(9), dR @ A[9:] + x[3:]])


def _sums_of(M, b):
    S = np.zeros(29, f64)
    S[:21] = M[np.triu_indices(6)]
    S[21:27] = b
    return S


def test_cholesky_solve_agrees_with_numpy_and_stays_orthonormal():
    worst, used = 0.0, 0
    for c in cases():
        if c[0] in ("single direction", "one target row", "no target", "no rows"):  # singular by construction: test 5
            continue
        n, M, b, A = _first_pass_sums(c)
        if n < 6 or np.linalg.cond(M) > 1e6:
            continue
        used += 1
        got = P.register_solve_plane(n, _sums_of(M, b), A)
        assert got is not None, c[0]
        worst = max(worst, float(np.abs(got - _compose(np.linalg.solve(M, b), A)).max()))
    assert used >= 6
    print(f"largest |Cholesky - numpy.linalg.solve| entry of the composed transform over {used} seeded systems: {worst:.3e}")
    assert worst <= 16 * SOLVE_VS_NUMPY, worst
    # 64 composed increments of 0.5 degrees about a fixed axis and a small shift, each through the solve of an exact system
    rng = np.random.default_rng(3)
    J = rng.normal(size=(200, 6))
    M = J.T @ J
    k = np.array([2.0, -1.0, 3.0]) / np.sqrt(14.0)
    x = np.concatenate([2 * np.tan(np.deg2rad(0.5) / 2) * k, [0.001, -0.002, 0.0015]])
    A = IDENTITY.copy()
    for _ in range(64):
        A = P.register_solve_plane(200, _sums_of(M, M @ x), A)
    R = A[:9].reshape(3, 3)
    ortho = float(np.abs(R.T @ R - np.eye(3)).max())
    print(f"largest |R^T R - I| entry after 64 composed increments: {ortho:.3e}")
    assert ortho <= 16 * ORTHO_AFTER_64, ortho
    angle = np.rad2deg(np.arccos((np.trace(R) - 1) / 2))
    assert abs(angle - 32.0) < 1e-6, angle


# ---- 4 ----
def _corner(n, seed):
    """n rows on each of the three faces x = 0, y = 0, z = 0 of the corner [0, 2]^3 at seeded places, and the faces' normals"""
    rng = np.random.default_rng(seed)
    rows, nrm = [], []
    for axis in range(3):
        p = rng.uniform(0, 2, (n, 3))
        p[:, axis] = 0
        e = np.zeros(3)
        e[axis] = 1
        rows.append(p)
        nrm.append(np.tile(e, (n, 1)))
    return np.concatenate(rows).astype(f32), np.concatenate(nrm)


def test_plane_metric_recovers_a_motion_the_point_metric_does_not():
    src, _ = _corner(1200, 21)
    other, other_n = _corner(1500, 22)  # the same faces sampled elsewhere
    A = _motion([2, -1, 3], 4.0, [0.05, -0.03, 0.04])  # DESIGN 12.14's motion: 4 degrees; 2.5 % of the extent of 2
    tgt, tgt_n = _move(A, other), _turn(A, other_n)
    radius, K = 0.25, 20
    point = P.register_points(src, tgt, radius, iterations=K, min_pairs=6)
    plane = P.register_points(src, tgt, radius, iterations=K, min_pairs=6, target_normals=tgt_n)
    assert point.pairs[0] >= len(src) // 2 and plane.pairs[0] >= len(src) // 2, (point.pairs[0], plane.pairs[0])
    assert plane.stats[1] == 0 and plane.stats[0] == K and point.stats[1] == 0
    err = lambda r: (float(np.abs(r.transform[:9] - A[:9]).max()), float(np.abs(r.transform[9:] - A[9:]).max()))  # noqa: E731
    (pr, pt), (lr, lt) = err(point), err(plane)
    print(f"rotation / translation error after {K} rounds: point {pr:.3e} / {pt:.3e}, plane {lr:.3e} / {lt:.3e}")
    assert lr < pr and lt < pt
    assert lr <= 16 * CORNER_ROT_ERR and lt <= 16 * CORNER_TRANS_ERR, (lr, lt)
    assert plane.sum_r2[-1] < plane.sum_r2[0]


# ---- 5 ----
def test_degenerate_systems_are_status_3_and_leave_the_transform():
    c = next(c for c in cases() if c[0] == "single direction")
    r = run_case(c)
    assert r.stats[1] == 3 and r.stats[0] == 0
    assert np.array_equal(r.transform.view(np.uint64), np.asarray(c[6], f64).view(np.uint64))
    assert r.pairs[0] >= 6 and not r.pairs[1:-1].any() and not r.sum_d2[1:-1].any() and not r.sum_r2[1:-1].any()
    assert r.pairs[-1] == r.pairs[0] and r.sum_r2[-1] == r.sum_r2[0] > 0
    # T = 1: every row pairs with the one target row; its normal (0,0,1) makes column 2 of J exactly zero, so the pivot test,
    # which is exact and undamped, sees the deficiency whatever the rounding
    one = run_case(next(c for c in cases() if c[0] == "one target row"))
    assert one.pairs[0] == 80 and one.stats[1] == 3 and one.stats[0] == 0
    assert np.array_equal(one.transform, IDENTITY)


def test_fewer_than_six_usable_pairs_is_status_2():
    c = next(c for c in cases() if c[0] == "moved copy")
    tn = np.zeros_like(c[3])
    tn[:5] = c[3][:5]  # five target rows keep a normal: only pairs with them are usable
    r = P.register_points(c[1], c[2], c[4], iterations=3, target_normals=tn)
    usable = int(np.isin(r.nearest, np.arange(5)).sum())
    assert r.stats[1] == 2 and r.stats[0] == 0 and r.pairs[0] == usable < 6
    assert (r.nearest >= 0).sum() > 100  # nearest / dist2 report the pairs whatever their normals
    assert np.array_equal(r.transform, IDENTITY)


# ---- 6 ----
def test_refusals_of_the_reference():
    src, (tgt, tn) = _bumpy(10, 1)[0], _bumpy(10, 2)
    for kw in (dict(radius=0.0), dict(radius=np.inf), dict(radius=1e30), dict(iterations=0), dict(iterations=65), dict(min_pairs=5),
               dict(min_pairs=3), dict(rot_eps=-1.0), dict(trans_eps=np.nan), dict(init=[np.nan] * 12), dict(target_normals=tn[:9])):
        args = dict(radius=0.3, iterations=2, target_normals=tn)
        args.update(kw)
        with pytest.raises(ValueError):
            P.register_points(src, tgt, **args)
    assert P.register_points(src, tgt, 0.3, iterations=2, target_normals=tn).sum_r2 is not None
