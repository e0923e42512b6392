"""Taubin / Laplacian smoothing of a mesh and its vertex normals: md_op_smooth_mesh and its host reference pipeline.smooth_mesh
(include/mi_depth.h states the contract). The CPU half checks the vectorised reference against a plain Python loop
over rows and faces written here; the GPU half checks that the operator gives the reference's bits: positions, normals and
counters, on wave and workgroup edges, on a fan (one contended accumulator), on 10^5 seeded quotients and on a noisy depth-grid
scene."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402
from burn_depth_amd import pipeline as P  # noqa: E402
from points_util import _t, dev, lib  # noqa: E402,F401

f32 = np.float32
SENTINEL = 0xA5
M64 = (1 << 64) - 1
STEP = 1.0 / 1024.0


# ---- the plain loop restatement ----

def _mix(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & M64
    return x ^ (x >> 31)


def _s64(u):
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def _corners(a, b, c):
    return ((a, b, c), (b, c, a), (c, a, b))  # (corner, successor, predecessor)


def _loop_smooth(xyz, faces, step, iterations, lam, mu=0.0, pin_boundary=True, normals=False, capacity=None):
    """the contract of include/mi_depth.h row by row and face by face -> (xyz, normals or None, stats, lattice positions)"""
    p = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, np.int32).reshape(-1, 3).tolist()
    N, step = len(p), f32(step)
    lam, mu = float(f32(lam)), float(f32(mu))
    ok, k0 = [], []
    for i in range(N):
        with np.errstate(all="ignore"):
            q = np.rint(p[i] / step)
            good = bool(np.isfinite(p[i]).all() and (np.abs(q) <= f32(4194304.0)).all())
        ok.append(good)
        k0.append([int(v) for v in q] if good else [0, 0, 0])
    deg, opened, live, invalid, degenerate = [0] * N, [0] * N, [], 0, 0
    for a, b, c in fc:
        if not all(0 <= v < N and ok[v] for v in (a, b, c)):
            invalid += 1
            continue
        if a == b or b == c or a == c:
            degenerate += 1
            continue
        live.append((a, b, c))
        for v, n, q in _corners(a, b, c):
            deg[v] += 2
            opened[v] = (opened[v] + _mix(n) - _mix(q)) & M64
    pinned = [deg[i] == 0 or not ok[i] or (bool(pin_boundary) and opened[i] != 0) for i in range(N)]
    k = [row[:] for row in k0]
    for t in range(2 * iterations if mu != 0 else iterations):
        factor = mu if (mu != 0 and t & 1) else lam
        S = [[0, 0, 0] for _ in range(N)]
        for a, b, c in live:
            for v, n, q in _corners(a, b, c):
                for ax in range(3):
                    S[v][ax] += k[n][ax] + k[q][ax]
        new = [row[:] for row in k]
        for i in range(N):
            if pinned[i]:
                continue
            for ax in range(3):
                d = float(_s64(S[i][ax])) / float(deg[i]) - float(k[i][ax])
                r = float(np.rint(factor * d))
                r = max(min(r, 2.0 ** 62), -(2.0 ** 62))
                new[i][ax] = _s64(k[i][ax] + int(r))
        k = new
    out = p.copy()
    moved = 0
    for i in range(N):
        if k[i] != k0[i]:
            moved += 1
            out[i] = [f32(float(k[i][ax]) * float(step)) for ax in range(3)]
    nrm = None
    if normals:
        acc = [[0, 0, 0] for _ in range(N)]
        for a, b, c in live:
            u = [k[b][ax] - k[a][ax] for ax in range(3)]
            w = [k[c][ax] - k[a][ax] for ax in range(3)]
            x = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
            for v in (a, b, c):
                for ax in range(3):
                    acc[v][ax] = _s64(acc[v][ax] + x[ax])
        nrm = np.zeros((N, 3), f32)
        for i in range(N):
            if deg[i] == 0 or acc[i] == [0, 0, 0]:
                continue
            x, y, z = (float(v) for v in acc[i])
            length = math.sqrt((x * x + y * y) + z * z)
            nrm[i] = [f32(x / length), f32(y / length), f32(z / length)]
    cap = N if capacity is None else capacity
    stats = np.array([invalid, degenerate, N - sum(ok), sum(1 for i in range(N) if deg[i] > 0 and opened[i] != 0), moved], np.int32)
    return out[:cap], (nrm[:cap] if normals else None), stats, np.array(k, np.int64).reshape(N, 3)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_against_loop(xyz, faces, step, iterations, lam, **kw):
    ref = P.smooth_mesh(xyz, faces, step, iterations, lam, normals=True, **kw)
    want = _loop_smooth(xyz, faces, step, iterations, lam, normals=True, **kw)
    assert _same_bits(ref.xyz, want[0]) and _same_bits(ref.normals, want[1]), kw
    assert ref.stats.tolist() == want[2].tolist(), (ref.stats, want[2])
    return ref, want[3]


# ---- the scenes ----

def _octahedron(r=1.0):
    xyz = np.array([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]], f32)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)  # outward
    return xyz, faces


def _grid(n, noise=0.0, seed=1):
    """an n x n depth-grid mesh, two triangles per cell with one diagonal direction, spacing 1/32; z noisy"""
    j, i = np.meshgrid(np.arange(n), np.arange(n))
    xyz = np.stack([j.ravel() / 32.0, i.ravel() / 32.0, np.zeros(n * n)], 1).astype(f32)
    if noise:
        xyz[:, 2] = np.random.default_rng(seed).normal(scale=noise, size=n * n).astype(f32)
    v = (i[:-1, :-1] * n + j[:-1, :-1]).ravel()
    faces = np.concatenate([np.stack([v, v + n, v + 1], 1), np.stack([v + 1, v + n, v + n + 1], 1)]).astype(np.int32)
    return xyz, faces


def _rim(n):
    idx = np.arange(n * n).reshape(n, n)
    m = np.zeros((n, n), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m.ravel(), idx


def _strip(F, seed=2):
    """0-1-2, 2-1-3, ...: a strip of F faces with consistent winding over F + 2 noisy rows"""
    rng = np.random.default_rng(seed + F)
    t = np.arange(F + 2)
    xyz = np.stack([t // 2 / 16.0, (t % 2) / 16.0, np.zeros(F + 2)], 1) + rng.normal(scale=0.01, size=(F + 2, 3))
    f = np.arange(F)
    faces = np.where((f % 2 == 0)[:, None], np.stack([f, f + 1, f + 2], 1), np.stack([f + 1, f, f + 2], 1)).astype(np.int32)
    return xyz.astype(f32), faces


def _fan(F, seed=3):
    """F faces (0, f + 1, f + 2) around row 0: an open fan"""
    rng = np.random.default_rng(seed)
    a = np.arange(F + 1) * (2 * np.pi / (F + 1))
    rim = np.stack([np.cos(a), np.sin(a), rng.normal(scale=0.05, size=F + 1)], 1)
    xyz = np.concatenate([[[0.013, -0.02, 0.4]], rim]).astype(f32)
    f = np.arange(F)
    return xyz, np.stack([np.zeros(F, np.int64), f + 1, f + 2], 1).astype(np.int32)


def _small_fans(count, seed):
    """`count` independent open fans of 1..32 faces (deg 2..64 at the centre) over rows spread over the whole lattice range"""
    rng = np.random.default_rng(seed)
    nfaces = rng.integers(1, 33, count)
    rows = nfaces + 2  # the centre, then nfaces + 1 rim rows
    base = np.concatenate([[0], np.cumsum(rows)])[:-1]
    N = int(rows.sum())
    xyz = rng.uniform(-4000.0, 4000.0, size=(N, 3)).astype(f32)
    which = np.repeat(np.arange(count), nfaces)
    local = np.arange(len(which)) - np.repeat(np.concatenate([[0], np.cumsum(nfaces)])[:-1], nfaces)
    faces = np.stack([base[which], base[which] + 1 + local, base[which] + 2 + local], 1).astype(np.int32)
    return xyz, faces


def _lattice_volume(k, faces):
    a, b, c = (k[faces[:, j]].astype(object) for j in range(3))
    det = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) - a[:, 1] * (b[:, 0] * c[:, 2] - b[:, 2] * c[:, 0])
           + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]))
    return int(det.sum())  # six times the volume, in lattice units


# ---- CPU: the vectorised reference against the loop ----

def test_a_single_triangle_is_open_at_all_three_rows_pinned_or_free():
    xyz = np.array([[0, 0, 0], [1, 0, 0.25], [0, 1, -0.25]], f32)
    faces = np.array([[0, 1, 2]], np.int32)
    ref, _ = _check_against_loop(xyz, faces, STEP, 3, 0.5, pin_boundary=True)
    assert ref.stats.tolist() == [0, 0, 0, 3, 0] and _same_bits(ref.xyz, xyz)
    ref, _ = _check_against_loop(xyz, faces, STEP, 3, 0.5, pin_boundary=False)
    assert ref.stats.tolist() == [0, 0, 0, 3, 3] and not np.array_equal(ref.xyz, xyz)
    assert np.allclose(ref.normals, ref.normals[0]) and ref.normals[0, 2] > 0  # one face: one normal, along the winding
    _check_against_loop(xyz, faces, STEP, 2, 0.5, mu=-0.53, pin_boundary=False)


def test_a_closed_octahedron_has_no_open_row_and_shrinks_under_lambda_alone():
    xyz, faces = _octahedron()
    ref, k = _check_against_loop(xyz, faces, STEP, 2, 0.5)
    assert ref.stats.tolist() == [0, 0, 0, 0, 6]
    assert np.abs(ref.xyz).max() == 0.25  # every row halves its distance per step
    assert 0 < _lattice_volume(k, faces) < _lattice_volume(np.rint(xyz / STEP).astype(np.int64), faces)
    assert np.array_equal(np.sign(ref.normals), np.sign(xyz))  # outward, as the winding


def test_a_lattice_aligned_flat_grid_does_not_move_and_returns_its_input_bits():
    xyz, faces = _grid(9)
    xyz[:, 2] = -0.0
    xyz[0, 0] = -0.0
    for pin in (True, False):
        ref, _ = _check_against_loop(xyz, faces, f32(1.0 / 32.0), 4, 0.5, mu=-0.53, pin_boundary=pin)
        if pin:
            assert _same_bits(ref.xyz, xyz) and ref.stats[4] == 0
            assert np.signbit(ref.xyz[:, 2]).all() and np.signbit(ref.xyz[0, 0])
    # the interior of the free grid does not move either: the umbrella of a regular grid is centred on the row
    m, _ = _rim(9)
    assert _same_bits(ref.xyz[~m], xyz[~m])


def test_the_noisy_grid_keeps_its_rim_when_pinned_and_pulls_it_inward_when_free():
    xyz, faces = _grid(33, noise=0.01)
    m, _ = _rim(33)
    assert m.sum() == 128
    ref, _ = _check_against_loop(xyz, faces, STEP, 2, 0.5, pin_boundary=True)
    assert ref.stats[3] == 128 and _same_bits(ref.xyz[m], xyz[m])
    assert (ref.xyz[~m] != xyz[~m]).any(1).sum() > 900 and ref.stats[4] == (ref.xyz != xyz).any(1).sum()
    assert np.abs(ref.xyz[~m, 2]).std() < np.abs(xyz[~m, 2]).std()
    free, _ = _check_against_loop(xyz, faces, STEP, 2, 0.5, pin_boundary=False)
    assert free.stats[3] == 128 and free.xyz[m, 0].min() > xyz[m, 0].min() and free.xyz[m, 0].max() < xyz[m, 0].max()
    _check_against_loop(xyz, faces, STEP, 1, 0.5, mu=-0.53)


def test_taubin_keeps_the_volume_of_the_octahedron_where_lambda_alone_does_not():
    xyz, faces = _octahedron()
    v0 = _lattice_volume(np.rint(xyz / STEP).astype(np.int64), faces)
    _, k_taubin = _check_against_loop(xyz, faces, STEP, 1, 0.5, mu=-0.53)
    _, k_lambda = _check_against_loop(xyz, faces, STEP, 2, 0.5)  # the same two steps, both shrinking
    bound = _lattice_volume(k_taubin, faces)  # the loop's: 0.5 * 1.53 per axis
    got = P.smooth_mesh(xyz, faces, STEP, 1, 0.5, mu=-0.53).xyz.astype(np.float64)
    got_volume = _lattice_volume(np.rint(got / STEP).astype(np.int64), faces)
    assert got_volume == bound and abs(bound / v0 - (0.5 * 1.53) ** 3) < 0.01
    assert _lattice_volume(k_lambda, faces) < bound / 20


def test_degenerate_invalid_and_out_of_range_corners_are_counted_and_inert():
    xyz, faces = _grid(9, noise=0.01)
    N = len(xyz)
    clean = P.smooth_mesh(xyz, faces, STEP, 2, 0.5, normals=True)
    xyz2 = np.concatenate([xyz, [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 5000.0], [0.5, 0.5, 0.5]]]).astype(f32)  # 5000 / step > 2^22
    extra = np.array([[0, 1, -1], [0, 1, N + 4], [3, 3, 4], [5, 6, 5], [N, 1, 2], [N + 1, 1, 2], [N + 2, 1, 2], [7, 7, 7]], np.int32)
    ref, _ = _check_against_loop(xyz2, np.concatenate([extra[:4], faces, extra[4:]]), STEP, 2, 0.5)
    assert ref.stats[:3].tolist() == [5, 3, 3] and ref.stats[3:].tolist() == clean.stats[3:].tolist()
    assert _same_bits(ref.xyz[:N], clean.xyz) and _same_bits(ref.normals[:N], clean.normals)
    assert _same_bits(ref.xyz[N:], xyz2[N:]) and not ref.normals[N:].any()


def test_a_capacity_below_the_rows_cuts_the_outputs_only():
    xyz, faces = _grid(9, noise=0.01)
    full = P.smooth_mesh(xyz, faces, STEP, 2, 0.5, normals=True)
    ref, _ = _check_against_loop(xyz, faces, STEP, 2, 0.5, capacity=40)
    assert _same_bits(ref.xyz, full.xyz[:40]) and _same_bits(ref.normals, full.normals[:40]) and ref.stats.tolist() == full.stats.tolist()
    assert P.smooth_mesh(xyz, faces, STEP, 2, 0.5, capacity=0).xyz.shape == (0, 3)


def test_a_shuffle_of_the_faces_changes_no_output_bit():
    xyz, faces = _grid(33, noise=0.01)
    a = P.smooth_mesh(xyz, faces, STEP, 3, 0.5, mu=-0.53, normals=True)
    b = P.smooth_mesh(xyz, faces[np.random.default_rng(8).permutation(len(faces))], STEP, 3, 0.5, mu=-0.53, normals=True)
    assert _same_bits(a.xyz, b.xyz) and _same_bits(a.normals, b.normals) and a.stats.tolist() == b.stats.tolist()


def test_the_reference_refuses_what_the_contract_refuses():
    xyz, faces = _octahedron()
    for kw in (dict(step=0.0), dict(step=-1.0), dict(step=np.inf), dict(step=np.nan), dict(lam=0.0), dict(lam=1.5), dict(lam=np.nan),
               dict(mu=0.1), dict(mu=-1.5), dict(mu=np.nan), dict(iterations=0), dict(iterations=1025), dict(capacity=-1)):
        args = dict(step=STEP, iterations=1, lam=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            P.smooth_mesh(xyz, faces, **args)


# ---- GPU: the operator against the reference ----

def _sentinel(shape, dt):
    n = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda").view(dt).reshape(shape)


def _untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENTINEL).all()


def _run(dev, xyz, faces, step, iterations, lam, mu=0.0, pin_boundary=True, normals=False, capacity=None, rows=None):
    """ops.smooth_mesh into outputs of `rows` rows (default N) preset to a sentinel byte -> numpy dict"""
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import SmoothedMesh
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    rows = len(xyz) if rows is None else rows
    out = SmoothedMesh(xyz=_sentinel((rows, 3), torch.float32), normals=_sentinel((rows, 3), torch.float32) if normals else None,
                       stats=_sentinel((5,), torch.int32))
    ops.smooth_mesh(dev, _t(xyz), _t(faces), step, iterations, lam, mu=mu, pin_boundary=pin_boundary, normals=normals, capacity=capacity, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(out).items() if isinstance(v, torch.Tensor)}


def _assert_same(got, ref, what=""):
    """every output of the operator is the reference's, and the rows behind the written ones still hold the sentinel"""
    assert got["stats"].tolist() == ref.stats.tolist(), (what, got["stats"], ref.stats)
    m = len(ref.xyz)
    wrong = (got["xyz"][:m].view(np.uint32) != ref.xyz.view(np.uint32)).any(1)
    assert not wrong.any(), (what, int(wrong.sum()), got["xyz"][:m][wrong][:4], ref.xyz[wrong][:4])
    assert _untouched(got["xyz"][m:]), what
    assert ("normals" in got) == (ref.normals is not None), what
    if ref.normals is not None:
        wrong = (got["normals"][:m].view(np.uint32) != ref.normals.view(np.uint32)).any(1)
        assert not wrong.any(), (what, int(wrong.sum()), got["normals"][:m][wrong][:4], ref.normals[wrong][:4])
        assert _untouched(got["normals"][m:]), what


@pytest.mark.gpu
@pytest.mark.parametrize("nf", [63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_strips_at_wave_and_workgroup_edges_are_bit_identical_to_the_host_reference(dev, nf):
    xyz, faces = _strip(nf)
    for kw in (dict(pin_boundary=False), dict(mu=-0.53, pin_boundary=False), dict(pin_boundary=True)):
        ref = P.smooth_mesh(xyz, faces, STEP, 2, 0.5, normals=True, **kw)
        assert kw["pin_boundary"] or ref.stats[4] > nf // 2
        _assert_same(_run(dev, xyz, faces, STEP, 2, 0.5, normals=True, **kw), ref, (nf, kw))


@pytest.mark.gpu
def test_a_fan_of_ten_thousand_faces_around_one_vertex(dev):
    xyz, faces = _fan(10000)
    ref = P.smooth_mesh(xyz, faces, STEP, 3, 0.5, mu=-0.53, pin_boundary=False, normals=True)
    assert ref.stats.tolist()[:4] == [0, 0, 0, 10002] and (ref.xyz[0] != xyz[0]).any()
    _assert_same(_run(dev, xyz, faces, STEP, 3, 0.5, mu=-0.53, pin_boundary=False, normals=True), ref)
    closed = np.concatenate([faces, [[0, 10001, 1]]]).astype(np.int32)  # the fan closed: the centre is not open, the rim is
    ref = P.smooth_mesh(xyz, closed, STEP, 3, 0.5, pin_boundary=True, normals=True)
    assert ref.stats[3] == 10001 and ref.stats[4] == 1
    _assert_same(_run(dev, xyz, closed, STEP, 3, 0.5, pin_boundary=True, normals=True), ref)


@pytest.mark.gpu
def test_a_hundred_thousand_seeded_single_step_quotients(dev):
    """f64 division, int64 -> f64 conversion, product and round of one step, and the f64 sqrt and division of the normals: 10^5
    fan centres with deg 2..64 (and their rim rows) over the whole lattice range, five factors"""
    lams = [1.0, 0.5] + np.random.default_rng(77).uniform(1e-3, 1.0, 3).astype(f32).tolist()
    for i, lam in enumerate(lams):
        xyz, faces = _small_fans(20000, seed=100 + i)
        ref = P.smooth_mesh(xyz, faces, STEP, 1, lam, pin_boundary=False, normals=True)
        assert ref.stats[:3].tolist() == [0, 0, 0] and ref.stats[4] > 0.99 * len(xyz)
        _assert_same(_run(dev, xyz, faces, STEP, 1, lam, pin_boundary=False, normals=True), ref, lam)


@pytest.fixture(scope="module")
def scene():
    xyz, faces = _grid(33, noise=0.01)
    xyz.setflags(write=False)
    faces.setflags(write=False)
    return xyz, faces


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 10])
@pytest.mark.parametrize("mu", [0.0, -0.53])
@pytest.mark.parametrize("pin", [True, False])
def test_the_noisy_grid_scene(dev, scene, iterations, mu, pin):
    xyz, faces = scene
    for normals in (False, True):
        ref = P.smooth_mesh(xyz, faces, STEP, iterations, 0.5, mu=mu, pin_boundary=pin, normals=normals)
        assert ref.stats[3] == 128 and ref.stats[4] > 480  # the scene moves: more than half of its 961 interior rows
        _assert_same(_run(dev, xyz, faces, STEP, iterations, 0.5, mu=mu, pin_boundary=pin, normals=normals), ref, normals)


@pytest.mark.gpu
def test_the_same_faces_shuffled_give_the_same_bits(dev, scene):
    xyz, faces = scene
    ref = P.smooth_mesh(xyz, faces, STEP, 10, 0.5, mu=-0.53, normals=True)
    _assert_same(_run(dev, xyz, faces[np.random.default_rng(8).permutation(len(faces))], STEP, 10, 0.5, mu=-0.53, normals=True), ref)


@pytest.mark.gpu
def test_invalid_degenerate_and_out_of_range_corners_on_the_device(dev, scene):
    xyz, faces = scene
    N = len(xyz)
    xyz2 = np.concatenate([xyz, [[np.nan, 0, 0], [0, -np.inf, 0], [0, 0, -5000.0], [0.5, 0.5, 0.5]]]).astype(f32)
    extra = np.array([[0, 1, -1], [0, 1, N + 4], [3, 3, 4], [5, 6, 5], [N, 1, 2], [N + 1, 1, 2], [N + 2, 1, 2], [7, 7, 7]], np.int32)
    both = np.concatenate([extra[:4], faces, extra[4:]])
    ref = P.smooth_mesh(xyz2, both, STEP, 2, 0.5, mu=-0.53, normals=True)
    assert ref.stats[:3].tolist() == [5, 3, 3]
    _assert_same(_run(dev, xyz2, both, STEP, 2, 0.5, mu=-0.53, normals=True), ref)


@pytest.mark.gpu
def test_no_rows_and_no_faces(dev, scene):
    xyz, faces = scene
    none = np.zeros((0, 3), np.int32)
    got = _run(dev, xyz, none, STEP, 2, 0.5, normals=True)
    _assert_same(got, P.smooth_mesh(xyz, none, STEP, 2, 0.5, normals=True))
    assert _same_bits(got["xyz"], xyz) and not got["normals"].any() and got["stats"].tolist() == [0] * 5
    got = _run(dev, np.zeros((0, 3), f32), [[0, 1, 2]], STEP, 2, 0.5, normals=True, rows=4)  # no rows: every face is invalid
    assert got["stats"].tolist() == [1, 0, 0, 0, 0] and _untouched(got["xyz"]) and _untouched(got["normals"])
    got = _run(dev, np.zeros((0, 3), f32), none, STEP, 1, 0.5)
    assert got["stats"].tolist() == [0] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [0, 1, 700])
def test_sentinels_behind_the_capacity_stay_untouched(dev, scene, capacity):
    xyz, faces = scene
    ref = P.smooth_mesh(xyz, faces, STEP, 2, 0.5, normals=True, capacity=capacity)
    assert len(ref.xyz) == capacity
    _assert_same(_run(dev, xyz, faces, STEP, 2, 0.5, normals=True, capacity=capacity), ref)


@pytest.mark.gpu
def test_two_runs_of_one_call_give_equal_bits(dev):
    xyz, faces = _fan(5000, seed=9)
    a, b = (_run(dev, xyz, faces, STEP, 5, 0.6, mu=-0.63, pin_boundary=False, normals=True) for _ in range(2))
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.gpu
def test_the_operator_refuses_before_any_launch(dev, lib, scene):
    import ctypes as C
    xyz, faces = _t(scene[0]), _t(scene[1])
    N, F = xyz.shape[0], faces.shape[0]
    outs = [_sentinel((N, 3), torch.float32), _sentinel((N, 3), torch.float32), _sentinel((5,), torch.int32)]

    def call(step=STEP, lam=0.5, mu=-0.53, iterations=2, n=N, f=F, cap=N, x=xyz, fc=faces, d=dev.handle, null=False):
        s = _lib.MdPointsSmooth(step, lam, mu, iterations, 1, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
        rc = lib.md_op_smooth_mesh(d, x.data_ptr() if x is not None else None, n, fc.data_ptr() if fc is not None else None, f,
                                   None if null else C.byref(s), cap, None)
        torch.cuda.synchronize()
        assert rc == _lib.MD_OK or all(_untouched(t.cpu().numpy()) for t in outs)
        return rc

    nan, inf = float("nan"), float("inf")
    for kw in (dict(step=0.0), dict(step=-STEP), dict(step=inf), dict(step=nan), dict(lam=0.0), dict(lam=1.0001), dict(lam=nan),
               dict(mu=0.001), dict(mu=-1.0001), dict(mu=nan), dict(iterations=0), dict(iterations=-1), dict(iterations=1025), dict(n=-1),
               dict(f=-1), dict(cap=-1), dict(x=None), dict(fc=None), dict(d=None), dict(null=True)):
        assert call(**kw) == _lib.MD_ERR_INVALID_ARG, kw
    for kw in (dict(n=1 << 30), dict(f=1 << 30)):
        assert call(**kw) == _lib.MD_ERR_SHAPE, kw
    assert call() == _lib.MD_OK and not any(_untouched(t.cpu().numpy()) for t in outs)  # the same arguments unbroken are taken
