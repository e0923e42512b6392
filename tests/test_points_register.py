"""Model -> cloud registered onto a reference cloud in one call: `infer_points(register=...)` (md_infer_points_register) against
`infer_points()` followed by `ops.register_points` on its list, bit for bit: eagerly and under graph replay, a device target
changed between replays, a host target, apply with match= and clusters= against the three operators by hand, and the call
without the stage against the match entry. include/mi_depth.h states the contract, DESIGN 12.14 the kernels. Runs with `-m gpu`
on an MI355X, on the tiny DA3 variants."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402
from points_util import _da3, _image, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
LIST = ("xyz", "conf", "rgb", "normals")
REG = ("transform", "pairs", "sum_d2", "stats", "dropped")
K = 4


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _same_registration(got, want, n, what):
    """got: the model call's `PointRegistration`; want: the operator's on the list of `n` rows"""
    torch.cuda.synchronize()
    for k in REG:
        assert np.array_equal(_bytes(getattr(got, k)), _bytes(getattr(want, k))), (what, k, getattr(got, k), getattr(want, k))
    assert np.array_equal(_bytes(got.nearest[:n]), _bytes(want.nearest)) and np.array_equal(_bytes(got.dist2[:n]), _bytes(want.dist2)), what


def _scene(m):
    x, shifted = _image(2, 70).cuda(), torch.roll(_image(2, 70), (3, 2), (2, 3)).cuda()
    rgb = torch.randint(0, 256, (2, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(world=True, rgb=rgb, normals=True, **OPTS)
    full = m.infer_points(x, **kw)
    n = int(full.count[-1])
    ref = m.infer_points(shifted, **kw)
    target = ref.xyz[:int(ref.count[-1])].clone()
    radius = float(np.float32(0.05 * float((full.xyz[:n].max(0).values - full.xyz[:n].min(0).values).max())))
    return x, kw, full, n, target, radius


def test_register_in_the_call_equals_the_operator_on_the_list_of_the_call(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, radius = _scene(m)
        assert n > 500 and len(target) > 500
        init = [1, 0, 0, 0, 1, 0, 0, 0, 1, radius / 8, 0, -radius / 8]
        req = dict(radius=radius, iterations=K, init=init, min_pairs=3)
        want = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True)
        assert 3 <= int(want.pairs[0]) and int(want.stats[0]) == K  # the reference pairs rows and every round solves
        for tgt, name in ((target, "device target"), (target.cpu().numpy(), "host target")):
            got = m.infer_points(x, register=dict(target=tgt, **req), **kw)
            _same_registration(got.registration, want, n, name)
            for k in LIST:  # apply is off: the list is the one the stage read
                assert np.array_equal(_bytes(getattr(got, k)[:n]), _bytes(getattr(full, k)[:n])), (name, k)
            assert np.array_equal(_bytes(got.count), _bytes(full.count))
        # apply: the moved rows and the rotated normals replace the list's in place; conf and rgb stay
        got = m.infer_points(x, register=dict(target=target, apply=True, **req), **kw)
        _same_registration(got.registration, want, n, "apply")
        assert np.array_equal(_bytes(got.xyz[:n]), _bytes(want.xyz)) and np.array_equal(_bytes(got.normals[:n]), _bytes(want.normals))
        assert not np.array_equal(_bytes(got.xyz[:n]), _bytes(full.xyz[:n]))
        assert np.array_equal(_bytes(got.conf[:n]), _bytes(full.conf[:n])) and np.array_equal(_bytes(got.rgb[:n]), _bytes(full.rgb[:n]))
        # graph replay on the same pointers; a replay reads the target's current contents
        reg = dict(target=target, apply=True, **req)
        m.enable_graph(True)
        out = m.infer_points(x, register=reg, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            out.registration.transform.fill_(7.0)
            out.xyz.fill_(7.0)
            out = m.infer_points(x, out=out, register=reg, **kw)
            _same_registration(out.registration, want, n, f"graph call {call}")
            assert np.array_equal(_bytes(out.xyz[:n]), _bytes(want.xyz)), call
        saved = target.clone()
        target.add_(radius / 4)  # in place: the same address, other contents
        changed = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True)
        assert not np.array_equal(_bytes(changed.transform), _bytes(want.transform))
        out = m.infer_points(x, out=out, register=reg, **kw)
        _same_registration(out.registration, changed, n, "replay after the target changed")
        assert np.array_equal(_bytes(out.xyz[:n]), _bytes(changed.xyz))
        assert m.query("allocs") == allocs and m.query("register_overflow") == 0
        m.enable_graph(False)
        target.copy_(saved)
    finally:
        m.enable_graph(False)
        m.destroy()


def test_apply_in_front_of_match_and_clusters_equals_the_three_operators_by_hand(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, radius = _scene(m)
        req = dict(radius=radius, iterations=K)
        mat = dict(radius=radius / 2, tol=(radius / 4,), mode="unmatched")
        clu = dict(radius=radius / 2, min_neighbours=2, min_points=3, mode="keep", table=64)
        got = m.infer_points(x, register=dict(target=target, apply=True, **req), match=dict(target=target, **mat), clusters=clu, **kw)
        a = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True)
        b = ops.match_points(dev, a.xyz, target, **mat, conf=full.conf[:n], rgb=full.rgb[:n], normals=a.normals)
        nb = int(b.count[-1])
        c = ops.cluster_points(dev, b.xyz[:nb], conf=b.conf[:nb], rgb=b.rgb[:nb], normals=b.normals[:nb], **clu)
        nc = int(c.count[-1])
        assert 0 < nc < nb < n, (nc, nb, n)
        _same_registration(got.registration, a, n, "chain")
        assert int(got.count[-1]) == nc
        for k in LIST + ("index",):
            assert np.array_equal(_bytes(getattr(got, k)[:nc]), _bytes(getattr(c, k)[:nc])), k
        assert np.array_equal(_bytes(got.match.nearest[:n]), _bytes(b.match.nearest)) and np.array_equal(_bytes(got.match.stats), _bytes(b.match.stats))
        assert np.array_equal(_bytes(got.clusters.cluster[:nb]), _bytes(c.clusters.cluster[:nb]))
        assert np.array_equal(_bytes(got.clusters.stats), _bytes(c.clusters.stats))
    finally:
        m.destroy()


def test_the_call_without_the_stage_is_the_match_entry_and_the_refusals(dev):
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, radius = _scene(m)
        mat = dict(target=target, radius=radius / 2, tol=(radius / 4,), mode="matched")
        want = m.infer_points(x, match=mat, **kw)
        for off in (None, dict(target=target, radius=0.0)):
            got = m.infer_points(x, match=mat, register=off, **kw)
            assert got.registration is None
            kept = int(want.count[-1])  # behind the survivors the outputs are untouched memory
            assert 0 < kept < n and np.array_equal(_bytes(got.count), _bytes(want.count))
            for k in LIST + ("index",):
                assert np.array_equal(_bytes(getattr(got, k)[:kept]), _bytes(getattr(want, k)[:kept])), k
            assert np.array_equal(_bytes(got.match.nearest[:n]), _bytes(want.match.nearest[:n])) and np.array_equal(_bytes(got.match.stats), _bytes(want.match.stats))
        ok = dict(target=target, radius=radius, iterations=2)
        for bad in (dict(ok, radius=-1.0), dict(ok, iterations=0), dict(ok, iterations=65), dict(ok, min_pairs=2), dict(ok, rot_eps=-1.0),
                    dict(ok, trans_eps=float("nan")), dict(ok, init=[float("inf")] * 12)):
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, register=bad, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
        with pytest.raises(_lib.MdError):  # the stage needs the list
            m.infer_points(x, register=ok, compact=False, **kw)
        with pytest.raises(_lib.MdError):  # apply beside a mesh: its faces belong to the rows before they moved
            m.infer_points(x, register=dict(ok, apply=True), mesh=True, **kw)
        with pytest.raises(_lib.MdError):
            m.infer_points(x, register=dict(ok, sweeps=3), **kw)
        assert m.infer_points(x, register=ok, **kw).registration is not None
    finally:
        m.destroy()


def test_host_outputs_equal_device_outputs(dev):
    """Everything in host memory against the device-memory call, which the tests above tie to the operator: the stage's outputs
    travel through the host-output table, nearest / dist2 only below the rows of the list the stage read -- the call's list, or
    with the matching's mode 2 behind it the model's own list in front of the cut."""
    import ctypes as C
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev, max_batch=2)
    try:
        x = _image(2, 70)
        xd = x.cuda()
        kw = dict(world=True, **OPTS)
        first = m.infer_points(xd, **kw)
        n = int(first.count[-1])
        ref = m.infer_points(torch.roll(xd, (3, 2), (2, 3)), **kw)
        target = ref.xyz[:int(ref.count[-1])].cpu().numpy().copy()
        tgt = torch.from_numpy(target).cuda()
        radius = float(np.float32(0.05 * float((first.xyz[:n].max(0).values - first.xyz[:n].min(0).values).max())))
        B, S = 2, 70
        cap = B * 35 * 35
        o = _points_opts(world=True, **OPTS)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f, i32, POISON = np.float32, np.int32, 123456.0
        shapes = dict(xyz=((cap, 3), f, POISON), conf=((cap,), f, POISON), count=((B + 1,), i32, -7), transform=((12,), np.float64, POISON),
                      pairs=((K + 1,), i32, -7), sum_d2=((K + 1,), np.float64, POISON), stats=((8,), i32, -7), dropped=((1,), i32, -7),
                      nearest=((cap,), i32, -7), dist2=((cap,), f, POISON), m_nearest=((cap,), i32, -7), m_index=((cap,), i32, -7))
        init = (C.c_double * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, radius / 8, 0, 0)

        def run(host, apply, cut):
            t = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
            where = target.ctypes.data if host else tgt.data_ptr()
            outs = _lib.MdPointsOutputs(None, None, ptr("xyz"), None, ptr("conf"), ptr("count"), cap, None)
            reg = _lib.MdPointsRegister(radius, where, len(target), kind, K, 3, apply, 0.0, 0.0, C.cast(init, C.c_void_p), ptr("transform"), ptr("pairs"),
                                        ptr("sum_d2"), ptr("stats"), ptr("dropped"), ptr("nearest"), ptr("dist2"))
            mat = _lib.MdPointsMatch(radius=radius / 2, target=where, target_rows=len(target), target_kind=kind, mode=2, nearest=ptr("m_nearest"),
                                     index=ptr("m_index")) if cut else None
            px = x.numpy().ctypes.data if host else xd.data_ptr()
            rc = lib.md_infer_points_register(m._h, C.c_void_p(px), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None, None, None, None,
                                              None, None, None, None, None, None, None, C.byref(mat) if cut else None, C.byref(reg), kind,
                                              None if host else st)
            assert rc == _lib.MD_OK, (rc, lib.md_last_error().decode())
            torch.cuda.synchronize()
            return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        for apply, cut in ((0, False), (1, False), (1, True)):
            on_device, on_host = run(False, apply, cut), run(True, apply, cut)
            assert on_device["stats"][0] == K and on_device["pairs"][0] >= 3 and int(on_device["stats"][2] + on_device["dropped"][0]) == n
            for k in shapes:
                assert np.array_equal(on_host[k].view(np.uint8), on_device[k].view(np.uint8)), (apply, cut, k)
            kept = int(on_host["count"][-1])
            assert (0 < kept < n) if cut else kept == n
            assert (on_host["nearest"][:n] != -7).all() and (on_host["nearest"][n:] == -7).all()  # the rows of the list the stage read
            assert (on_host["xyz"][kept:] == f(POISON)).all()
            moved = not np.array_equal(on_host["xyz"][:kept].view(np.uint32), first.xyz[:n].cpu().numpy()[:kept].view(np.uint32))
            assert moved == bool(apply)
    finally:
        m.destroy()


def test_infer_cli_prints_the_transform_and_writes_the_aligned_cloud(dev, tmp_path, capsys):
    """tools/infer.py --ply --register-ply REF.ply --register-radius R: one image through the stage of the model call, --views
    through ops.register_points on the points of the file; --register-apply writes the moved rows, and the match step sees them"""
    import importlib.util
    from burn_depth_amd import ops
    from burn_depth_amd import pipeline as P
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
    spec = importlib.util.spec_from_file_location("infer_cli", os.path.join(ROOT, "tools", "infer.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ck = str(tmp_path / "da3_small.safetensors")
    Wt.save_container(ck, Wt.generate_da3_weights(DepthAnything3Config.small(), 0, Wt.INIT_PARITY), dtype="F16")
    rgb = np.load(os.path.join(ROOT, "tests", "golden", "test_jpg_rgb.npy"))
    img, flip = str(tmp_path / "img.npy"), str(tmp_path / "flip.npy")
    np.save(img, rgb)
    np.save(flip, np.ascontiguousarray(rgb[:, ::-1]))
    ply, ref_ply = str(tmp_path / "cloud.ply"), str(tmp_path / "ref.ply")
    one = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "4", "--edge-rtol", "0.5"]
    views = ["--model", "depth-anything-3", "--checkpoint", ck, "--views", img, flip, "--ply", ply, "--stride", "4", "--output", str(tmp_path / "d.png")]
    assert cli.main(one + ["--register-ply", ref_ply]) == 2  # without a radius
    assert cli.main(one + ["--register-ply", ref_ply, "--register-radius", "1", "--register-iterations", "65"]) == 2
    assert cli.main(one + ["--mesh", "--register-ply", ref_ply, "--register-radius", "1", "--register-apply"]) == 2
    assert cli.main(one + ["--register-apply"]) == 2
    for head in (one, views):
        assert cli.main(head) == 0
        xyz0, col0 = P.read_ply(ply)
        fin = xyz0[np.isfinite(xyz0).all(1)]
        extent = float(np.ptp(fin, axis=0).max())
        radius = float(np.float32(0.05 * extent))
        c, s = np.cos(0.01), np.sin(0.01)
        rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        ref = ((xyz0.astype(np.float64) - fin.mean(0)) @ rot.T + fin.mean(0) + 0.01 * extent).astype(np.float32)
        P.write_ply(ref_ply, ref, col0)
        src, tgt = torch.from_numpy(xyz0).cuda(), torch.from_numpy(P.read_ply(ref_ply)[0]).cuda()
        want = ops.register_points(dev, src, tgt, radius, iterations=6, apply=True)
        torch.cuda.synchronize()
        assert int(want.stats[0]) == 6 and float(want.sum_d2[-1]) < float(want.sum_d2[0])
        rows = ["  " + " ".join(f"{v:+.9e}" for v in row) for row in want.matrix().tolist()]
        opts = ["--register-ply", ref_ply, "--register-radius", repr(radius), "--register-iterations", "6"]
        capsys.readouterr()
        assert cli.main(head + opts) == 0
        said = capsys.readouterr().out.splitlines()
        at = said.index("Registration:")
        assert said[at + 1:at + 5] == rows, (said, rows)
        assert any(l.startswith(f"Registration: 6 solves (ran every round), {int(want.pairs[0])} -> {int(want.pairs[-1])} pairs") for l in said), said
        xyz1, _ = P.read_ply(ply)
        assert np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32))  # without --register-apply the cloud stays
        near = ops.match_points(dev, want.xyz, tgt, radius / 4).match
        capsys.readouterr()
        assert cli.main(head + opts + ["--register-apply", "--match-ply", ref_ply, "--match-radius", repr(radius / 4)]) == 0
        said = capsys.readouterr().out.splitlines()
        assert said[said.index("Registration:") + 1:][:4] == rows
        stats = near.stats.cpu().tolist()
        assert any(l.startswith(f"Match: {stats[0]} points in range, {stats[1]} with a counterpart") for l in said), said
        xyz2, col2 = P.read_ply(ply)
        assert np.array_equal(xyz2.view(np.uint32), want.xyz.cpu().numpy().view(np.uint32)) and np.array_equal(col2, col0)
