"""Model -> cloud registered onto a reference cloud by the point-to-plane metric in one call:
`infer_points(register=dict(..., target_normals=))` (md_infer_points_register_plane) against `infer_points()` followed by
`ops.register_points(..., target_normals=)` on its list, bit for bit: eagerly, with a host target and host normals, under graph
replay with the device normals changed between replays, apply with match= against the operators by hand, the call without the
keyword against the register entry, and tools/infer.py --register-metric plane. include/mi_depth.h states the contract, DESIGN
12.15 the kernels. Runs with `-m gpu` on an MI355X, on the tiny DA3 variants the other point-path tests use."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

from burn_depth_amd import _lib  # noqa: E402
from points_util import _da3, _image, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
LIST = ("xyz", "conf", "rgb", "normals")
REG = ("transform", "pairs", "sum_d2", "sum_r2", "stats", "dropped")
K = 4


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _same_registration(got, want, n, what, fields=REG):
    torch.cuda.synchronize()
    for k in fields:
        assert np.array_equal(_bytes(getattr(got, k)), _bytes(getattr(want, k))), (what, k, getattr(got, k), getattr(want, k))
    # below the n rows of the list: the model call's tensors cover its capacity, the operator's the n rows
    assert np.array_equal(_bytes(got.nearest[:n]), _bytes(want.nearest[:n])) and np.array_equal(_bytes(got.dist2[:n]), _bytes(want.dist2[:n])), what


def _scene(m):
    """the list of one call, and as reference cloud the list and the normals of a shifted image"""
    x, shifted = _image(2, 70).cuda(), torch.roll(_image(2, 70), (3, 2), (2, 3)).cuda()
    rgb = torch.randint(0, 256, (2, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    kw = dict(world=True, rgb=rgb, normals=True, **OPTS)
    full = m.infer_points(x, **kw)
    n = int(full.count[-1])
    ref = m.infer_points(shifted, **kw)
    t = int(ref.count[-1])
    target, normals = ref.xyz[:t].clone(), ref.normals[:t].clone()
    radius = float(np.float32(0.05 * float((full.xyz[:n].max(0).values - full.xyz[:n].min(0).values).max())))
    return x, kw, full, n, target, normals, radius


def test_plane_register_in_the_call_equals_the_operator_on_the_list_of_the_call(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, tn, radius = _scene(m)
        assert n > 500 and len(target) > 500
        init = [1, 0, 0, 0, 1, 0, 0, 0, 1, radius / 8, 0, -radius / 8]
        req = dict(radius=radius, iterations=K, init=init, min_pairs=6)
        want = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True, target_normals=tn)
        torch.cuda.synchronize()
        assert 6 <= int(want.pairs[0]) and int(want.stats[1]) in (0, 3)  # the reference pairs rows; whichever status, the call gives it too
        point = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True)
        assert int(want.stats[0]) == 0 or not np.array_equal(_bytes(want.transform), _bytes(point.transform))
        for tgt, nrm, name in ((target, tn, "device target"), (target.cpu().numpy(), tn.cpu().numpy(), "host target and normals")):
            got = m.infer_points(x, register=dict(target=tgt, target_normals=nrm, **req), **kw)
            _same_registration(got.registration, want, n, name)
            for k in LIST:  # apply is off: the list is the one the stage read
                assert np.array_equal(_bytes(getattr(got, k)[:n]), _bytes(getattr(full, k)[:n])), (name, k)
            assert np.array_equal(_bytes(got.count), _bytes(full.count))
        with pytest.raises(_lib.MdError):  # the normals lie where the target lies
            m.infer_points(x, register=dict(target=target, target_normals=tn.cpu().numpy(), **req), **kw)
        got = m.infer_points(x, register=dict(target=target, target_normals=tn, apply=True, **req), **kw)
        _same_registration(got.registration, want, n, "apply")
        assert np.array_equal(_bytes(got.xyz[:n]), _bytes(want.xyz)) and np.array_equal(_bytes(got.normals[:n]), _bytes(want.normals))
        assert np.array_equal(_bytes(got.conf[:n]), _bytes(full.conf[:n])) and np.array_equal(_bytes(got.rgb[:n]), _bytes(full.rgb[:n]))
        # graph replay on the same pointers; a replay reads the normals' current contents
        reg = dict(target=target, target_normals=tn, apply=True, **req)
        m.enable_graph(True)
        out = m.infer_points(x, register=reg, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            out.registration.transform.fill_(7.0)
            out.registration.sum_r2.fill_(7.0)
            out.xyz.fill_(7.0)
            out = m.infer_points(x, out=out, register=reg, **kw)
            _same_registration(out.registration, want, n, f"graph call {call}")
            assert np.array_equal(_bytes(out.xyz[:n]), _bytes(want.xyz)), call
        saved = tn.clone()
        tn.copy_(torch.roll(saved, 1, 1))  # in place: the same address, other normals
        changed = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True, target_normals=tn)
        assert not np.array_equal(_bytes(changed.sum_r2), _bytes(want.sum_r2))
        out = m.infer_points(x, out=out, register=reg, **kw)
        _same_registration(out.registration, changed, n, "replay after the normals changed")
        assert np.array_equal(_bytes(out.xyz[:n]), _bytes(changed.xyz))
        assert m.query("allocs") == allocs and m.query("register_overflow") == 0
        m.enable_graph(False)
        tn.copy_(saved)
    finally:
        m.enable_graph(False)
        m.destroy()


def test_apply_in_front_of_match_equals_the_operators_by_hand(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, tn, radius = _scene(m)
        req = dict(radius=radius, iterations=K)
        mat = dict(radius=radius / 2, tol=(radius / 4,), mode="unmatched")
        got = m.infer_points(x, register=dict(target=target, target_normals=tn, apply=True, **req), match=dict(target=target, **mat), **kw)
        a = ops.register_points(dev, full.xyz[:n], target, **req, normals=full.normals[:n], apply=True, target_normals=tn)
        b = ops.match_points(dev, a.xyz, target, **mat, conf=full.conf[:n], rgb=full.rgb[:n], normals=a.normals)
        nb = int(b.count[-1])
        assert 0 < nb < n, (nb, n)
        _same_registration(got.registration, a, n, "chain")
        assert int(got.count[-1]) == nb
        for k in LIST + ("index",):
            assert np.array_equal(_bytes(getattr(got, k)[:nb]), _bytes(getattr(b, k)[:nb])), k
        assert np.array_equal(_bytes(got.match.nearest[:n]), _bytes(b.match.nearest)) and np.array_equal(_bytes(got.match.stats), _bytes(b.match.stats))
    finally:
        m.destroy()


def test_the_call_without_the_keyword_is_the_register_entry_and_the_refusals(dev):
    m = _da3(dev, max_batch=2)
    try:
        x, kw, full, n, target, tn, radius = _scene(m)
        req = dict(target=target, radius=radius, iterations=K)
        want = m.infer_points(x, register=req, **kw)
        got = m.infer_points(x, register=dict(req, target_normals=None), **kw)
        assert got.registration.sum_r2 is None and want.registration.sum_r2 is None
        _same_registration(got.registration, want.registration, n, "no normals", fields=("transform", "pairs", "sum_d2", "stats", "dropped"))
        for k in LIST:
            assert np.array_equal(_bytes(getattr(got, k)[:n]), _bytes(getattr(want, k)[:n])), k
        ok = dict(req, target_normals=tn)
        for bad in (dict(ok, min_pairs=5), dict(ok, min_pairs=3), dict(ok, iterations=65), dict(ok, radius=-1.0)):
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, register=bad, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
        with pytest.raises(_lib.MdError):  # [T,3] beside the target
            m.infer_points(x, register=dict(ok, target_normals=tn[:-1]), **kw)
        assert m.infer_points(x, register=ok, **kw).registration.sum_r2 is not None
    finally:
        m.destroy()


def test_infer_cli_prints_the_operator_s_matrix_with_the_plane_metric(dev, tmp_path, capsys):
    """tools/infer.py --ply --register-ply REF.ply --register-metric plane: the normals of REF.ply through read_ply_normals; a
    file without them is refused"""
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
    img = str(tmp_path / "img.npy")
    np.save(img, np.load(os.path.join(ROOT, "tests", "golden", "test_jpg_rgb.npy")))
    ply, ref_ply, bare_ply = str(tmp_path / "cloud.ply"), str(tmp_path / "ref.ply"), str(tmp_path / "bare.ply")
    one = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "4", "--edge-rtol", "0.5"]
    assert cli.main(one + ["--normals"]) == 0
    xyz0, col0, nrm0 = P.read_ply_normals(ply)
    assert nrm0 is not None
    fin = xyz0[np.isfinite(xyz0).all(1)]
    extent = float(np.ptp(fin, axis=0).max())
    radius = float(np.float32(0.05 * extent))
    c, s = np.cos(0.01), np.sin(0.01)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    ref = ((xyz0.astype(np.float64) - fin.mean(0)) @ rot.T + fin.mean(0) + 0.01 * extent).astype(np.float32)
    P.write_ply(ref_ply, ref, col0, normals=(nrm0.astype(np.float64) @ rot.T).astype(np.float32))
    P.write_ply(bare_ply, ref, col0)
    opts = ["--register-radius", repr(radius), "--register-iterations", "6", "--register-metric", "plane"]
    assert cli.main(one + ["--register-ply", bare_ply] + opts) == 2  # no normals in the file
    assert cli.main(one + ["--register-metric", "plane"]) == 2  # without --register-ply
    tx, _, tnrm = P.read_ply_normals(ref_ply)
    assert cli.main(one) == 0  # the cloud the register step reads: the call without --normals
    src = torch.from_numpy(P.read_ply(ply)[0]).cuda()
    want = ops.register_points(dev, src, torch.from_numpy(tx).cuda(), radius, iterations=6, target_normals=torch.from_numpy(tnrm).cuda())
    torch.cuda.synchronize()
    rows = ["  " + " ".join(f"{v:+.9e}" for v in row) for row in want.matrix().tolist()]
    capsys.readouterr()
    assert cli.main(one + ["--register-ply", ref_ply] + opts) == 0
    said = capsys.readouterr().out.splitlines()
    at = said.index("Registration:")
    assert said[at + 1:at + 5] == rows, (said, rows)
    pairs, r2 = want.pairs.cpu().tolist(), want.sum_r2.cpu().tolist()
    rms = [float(np.sqrt(r2[k] / max(pairs[k], 1))) for k in (0, -1)]
    assert any(l.startswith(f"Registration (plane): status {int(want.stats[1])}, RMS point-to-plane residual {rms[0]:.6g} -> {rms[1]:.6g}") for l in said), said
