"""md_infer_points_decimate: the model -> point cloud -> mesh call with the vertex-clustering decimation behind the mesh stage
(DESIGN 12.8). The stage is md_op_decimate_mesh's launches on the model's own list and faces, so every comparison is bit for bit
against `ops.decimate_mesh` on the outputs of the same call without it. All tests need an MI355X (`-m gpu`)."""
import ctypes as C
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
from points_util import _da3, _image, _pro, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTS = dict(depth_min=1e-3, depth_max=1e6)
DEC_KEYS = ("xyz", "rgb", "conf", "index", "weight")
POISONS = dict(xyz=123456.0, rgb=77, conf=123456.0, index=-7, weight=-7, count=-5, dropped=-5, remap=-9, faces=-11, face_index=-11,
               face_count=-5, faces_dropped=-5)


def _np(pc):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in vars(pc).items()}


def _poison(pc):
    for k, fill in POISONS.items():
        if getattr(pc, k) is not None:
            getattr(pc, k).fill_(fill)


def _voxel_for(xyz, share):
    """a voxel side that leaves about `share` of the rows (host bisection on the reference)"""
    span = float((xyz.max(0) - xyz.min(0)).max())
    lo, hi = span * 2.0 ** -16, span
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        if P.voxel_thin(xyz, mid).count[-1] > share * len(xyz):
            lo = mid
        else:
            hi = mid
    return float(f32(hi))


def _operator(dev, full, voxel):
    """ops.decimate_mesh on the list and faces of the undecimated call, and the per-view counts from the host reference"""
    from burn_depth_amd import ops
    n, nf = int(full.count[-1].item()), int(full.face_count[-1].item())
    cut = lambda t: t[:n] if t is not None else None  # noqa: E731
    want = _np(ops.decimate_mesh(dev, full.xyz[:n], full.faces[:nf], voxel, conf=cut(full.conf), rgb=cut(full.rgb)))
    ref = P.decimate_mesh(full.xyz[:n].cpu().numpy(), full.faces[:nf].cpu().numpy(), voxel, None if full.conf is None else full.conf[:n].cpu().numpy(),
                          counts=full.count[:-1].cpu().numpy(), face_counts=full.face_count[:-1].cpu().numpy())
    return want, ref, n, nf


def _same_decimated(got, want, ref, n, what):
    m, k = int(want["count"][-1]), int(want["face_count"][-1])
    assert 0 < m < n and k > 0, what
    assert got["count"].tolist() == ref.vertices.count.tolist(), (what, got["count"], ref.vertices.count)
    assert got["face_count"].tolist() == ref.face_count.tolist(), (what, got["face_count"], ref.face_count)
    assert got["faces_dropped"].tolist() == want["faces_dropped"].tolist() and got["dropped"].tolist() == want["dropped"].tolist(), what
    for key in DEC_KEYS:
        if want[key] is not None:
            assert np.array_equal(got[key][:m].view(np.uint8), want[key][:m].view(np.uint8)), (what, key)
    assert np.array_equal(got["remap"][:n], want["remap"]) and (got["remap"][n:] == -1).all(), what
    assert np.array_equal(got["faces"][:k], want["faces"][:k]) and np.array_equal(got["face_index"][:k], want["face_index"][:k]), what
    assert (got["faces"][k:] == -11).all() and (got["xyz"][m:] == f32(123456.0)).all(), what  # the rows behind stay untouched


def _poisoned_call(m, x, **kw):
    out = m.infer_points(x, **kw)
    _poison(out)
    return m.infer_points(x, out=out, **kw)


@pytest.mark.parametrize("model", ["da3", "pro"])
def test_model_call_equals_the_operator_eagerly_and_under_graph_replay(dev, model):
    m = _da3(dev, max_batch=3) if model == "da3" else _pro(dev, "small")
    try:
        B, S = (3, 70) if model == "da3" else (1, 512)
        x = _image(B, S).cuda()
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=model == "da3", rgb=rgb, stride=1 if model == "da3" else 4, **OPTS)
        full = m.infer_points(x, mesh=True, **kw)
        n = int(full.count[-1].item())
        voxel = _voxel_for(full.xyz[:n].cpu().numpy(), 0.3)
        want, ref, n, nf = _operator(dev, full, voxel)
        assert (want["faces_dropped"][1:] > 0).all()
        dec = dict(voxel=voxel)
        got = _np(_poisoned_call(m, x, mesh=True, decimate=dec, **kw))
        _same_decimated(got, want, ref, n, (model, "eager"))
        # pixel_index names rows of the undecimated list; remap carries it over: the vertex lies in the pixel's voxel
        pix, pm = got["pixel_index"], got["point_map"]
        listed = pix >= 0
        assert np.array_equal(pix, _np(full)["pixel_index"]) and listed.sum() == n
        v = f32(voxel)
        assert np.array_equal(np.floor(got["xyz"][got["remap"][pix[listed]]] / v), np.floor(pm[listed] / v))
        # a capacity below the outputs: the true counts
        small = _np(m.infer_points(x, mesh=True, decimate=dict(voxel=voxel, face_capacity=5), **kw))
        assert small["face_count"].tolist() == got["face_count"].tolist() and np.array_equal(small["faces"], got["faces"][:5])
        m.enable_graph(True)
        out = m.infer_points(x, mesh=True, decimate=dec, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):
            _poison(out)
            out = m.infer_points(x, out=out, mesh=True, decimate=dec, **kw)
            _same_decimated(_np(out), want, ref, n, (model, "graph", call))
        assert m.query("allocs") == allocs
        assert m.query("decimate_overflow") == 0
    finally:
        m.enable_graph(False)
        m.destroy()


def test_render_and_raster_see_the_decimated_list_and_faces(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS)
        full = m.infer_points(x, mesh=True, **kw)
        n = int(full.count[-1].item())
        voxel = _voxel_for(full.xyz[:n].cpu().numpy(), 0.3)
        # two cameras that look at the cloud's centre from outside it (the reduced models' clouds have far outliers)
        pts = full.xyz[:n].cpu().numpy()
        c = pts.mean(0).astype(np.float64)
        d = 2.0 * float(np.percentile(np.linalg.norm(pts - c, axis=1), 80)) + 1e-3
        E = np.zeros((2, 3, 4), f32)
        E[:, :, :3], E[:, :, 3] = np.eye(3), np.array([0, 0, d]) - c
        E[1, 0, 3] += 0.1 * d
        cams = dict(H=48, W=56, focal_px=torch.tensor([40.0, 55.0]), extrinsics=torch.from_numpy(E))
        for graph in (False, True):
            m.enable_graph(graph)
            out = m.infer_points(x, mesh=True, decimate=dict(voxel=voxel), render=dict(radius=1, **cams), raster=dict(**cams), **kw)
            for _ in range(2 if graph else 1):
                out = m.infer_points(x, out=out, mesh=True, decimate=dict(voxel=voxel), render=dict(radius=1, **cams), raster=dict(**cams), **kw)
            torch.cuda.synchronize()
            mv = int(out.count[-1].item())
            assert 0 < mv < n
            pts = ops.render_points(dev, out.xyz, 48, 56, focal_px=cams["focal_px"], extrinsics=cams["extrinsics"].cuda(), rgb=out.rgb, count=out.count[-1:], radius=1)
            tri = ops.render_mesh(dev, out.xyz, out.faces, 48, 56, focal_px=cams["focal_px"], extrinsics=cams["extrinsics"].cuda(), rgb=out.rgb, face_count=out.face_count[-1:])
            torch.cuda.synchronize()
            for k in ("depth", "index", "rgb", "filled"):
                assert torch.equal(getattr(out.render, k), getattr(pts, k)), (graph, "render", k)
            for k in ("depth", "face", "rgb", "filled", "skipped"):
                assert torch.equal(getattr(out.raster, k), getattr(tri, k)), (graph, "raster", k)
            assert out.render.filled[-1].item() > 0 and out.raster.filled[-1].item() > 0
    finally:
        m.enable_graph(False)
        m.destroy()


def test_null_and_zero_voxel_are_the_call_without_it_and_the_refusals_leave_the_outputs_untouched(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, mesh=True, **OPTS)
        m.enable_timing(True)
        names, outs = {}, {}
        for what, extra in (("none", dict()), ("null", dict(decimate=None)), ("zero", dict(decimate=dict(voxel=0.0))), ("on", dict(decimate=dict(voxel=0.05)))):
            m.read_timing()
            outs[what] = _np(m.infer_points(x, **extra, **kw))
            names[what] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["none"] == names["null"] == names["zero"] and "points_mesh" in names["none"] and "points_decimate" not in names["none"]
        order = list(names["on"])
        assert order.index("points_mesh") < order.index("points_decimate")
        n, nf = int(outs["none"]["count"][-1]), int(outs["none"]["face_count"][-1])
        assert n > 0 and nf > 0
        for what in ("null", "zero"):
            for k, v in outs["none"].items():
                rows = n if k in ("xyz", "rgb", "conf") else nf if k == "faces" else None
                assert (v is None) == (outs[what][k] is None), (what, k)
                assert v is None or np.array_equal(v[:rows].view(np.uint8), outs[what][k][:rows].view(np.uint8)), (what, k)
        # refusals: nothing is written
        out = m.infer_points(x, decimate=dict(voxel=0.05), **kw)
        for bad, text in ((dict(decimate=dict(voxel=0.05), voxel=0.1), "two grids"),
                          (dict(decimate=dict(voxel=0.05), outlier=dict(radius=0.1, min_neighbours=2)), "outlier removal"),
                          (dict(decimate=dict(voxel=-1.0)), "voxel"), (dict(decimate=dict(voxel=float("nan"))), "voxel"),
                          (dict(decimate=dict(voxel=float("inf"))), "voxel")):
            _poison(out)
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, out=out, **bad, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG and text in str(e.value), bad
            torch.cuda.synchronize()
            for k, fill in POISONS.items():
                assert getattr(out, k) is None or (getattr(out, k) == fill).all(), (bad, k)
        with pytest.raises(_lib.MdError) as e:  # without a mesh request
            m.infer_points(x, decimate=dict(voxel=0.05), world=True, **OPTS)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
    finally:
        m.destroy()


def test_entries_through_ctypes_null_parts_refusals_and_host_memory(dev):
    """The narrower entries equal the widest with a null part; dec's pointers with voxel 0 and dec without a mesh are refused by the
    library itself; the host-memory call equals the device-memory one."""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S = 2, 70
        rows, fcap = B * S * S, 2 * B * 69 * 69
        x = _image(B, S)
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        xd, rd = x.cuda(), rgb.cuda()
        o = _points_opts(world=True, **OPTS)
        DEV, HOST = _lib.MD_MEM_DEVICE, _lib.MD_MEM_HOST
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        shapes = dict(xyz=((rows, 3), f32), rgb=((rows, 3), np.uint8), conf=((rows,), f32), count=((B + 1,), np.int32), index=((rows,), np.int32),
                      weight=((rows,), np.int32), dropped=((1,), np.int32), remap=((rows,), np.int32), faces=((fcap, 3), np.int32),
                      face_index=((fcap,), np.int32), face_count=((B + 1,), np.int32), faces_dropped=((3,), np.int32),
                      mesh_faces=((fcap, 3), np.int32), mesh_face_count=((B + 1,), np.int32), pixel_index=((B, S, S), np.int32))

        def call(entry, host=False, voxel=0.05, with_mesh=True, stray=False):
            t = {k: np.full(shape, POISONS.get(k, -3), dt) for k, (shape, dt) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            p = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, p("xyz"), p("rgb"), p("conf"), p("count"), rows, None)
            msh = _lib.MdPointsMesh(0.0, p("mesh_faces"), p("mesh_face_count"), fcap, p("pixel_index"))
            dec = _lib.MdPointsDecimate(voxel, p("index"), p("weight"), p("dropped"), p("remap"), p("faces"), p("face_index"), p("face_count"), fcap,
                                        p("faces_dropped"))
            if voxel == 0.0 and not stray:
                dec = _lib.MdPointsDecimate(0.0, None, None, None, None, None, None, None, 0, None)
            xin, cin = (x.numpy(), rgb.numpy()) if host else (xd, rd)
            px, pc = (xin.ctypes.data, cin.ctypes.data) if host else (xin.data_ptr(), cin.data_ptr())
            kind = HOST if host else DEV
            head = (m._h, C.c_void_p(px), B, S, S, kind, C.c_void_p(pc), None, None, C.byref(o), C.byref(outs), None, None, None,
                    C.byref(msh) if with_mesh else None, None)
            if entry == "raster":
                rc = lib.md_infer_points_raster(*head, kind, None if host else st)
            elif entry == "outlier":
                rc = lib.md_infer_points_outlier(*head, None, kind, None if host else st)
            else:
                rc = lib.md_infer_points_decimate(*head, None, C.byref(dec) if entry == "decimate" else None, kind, None if host else st)
            torch.cuda.synchronize()
            return rc, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        rc, widest = call("decimate-null")
        assert rc == 0
        n, nf = int(widest["count"][-1]), int(widest["mesh_face_count"][-1])
        assert n > 0 and nf > 0 and (widest["faces"] == -11).all()
        for what, (rc, other) in (("raster", call("raster")), ("outlier", call("outlier")), ("voxel 0", call("decimate", voxel=0.0))):
            assert rc == 0, what
            for k in widest:
                cut = n if k in ("xyz", "rgb", "conf") else nf if k == "mesh_faces" else None
                assert np.array_equal(widest[k][:cut].view(np.uint8), other[k][:cut].view(np.uint8)), (what, k)
        for kw in (dict(voxel=0.0, stray=True), dict(with_mesh=False)):  # pointers with voxel == 0; no mesh request
            rc, left = call("decimate", **kw)
            assert rc == _lib.MD_ERR_INVALID_ARG, kw
            for k, v in left.items():
                assert (v == np.asarray(POISONS.get(k, -3), v.dtype)).all(), (kw, k)
        (rc_d, on_device), (rc_h, on_host) = call("decimate"), call("decimate", host=True)
        assert rc_d == 0 and rc_h == 0
        mv, kf = int(on_device["count"][-1]), int(on_device["face_count"][-1])
        assert 0 < mv < n and 0 < kf < nf
        # the caller's mesh outputs still hold the undecimated mesh of the undecimated list
        assert np.array_equal(on_device["mesh_face_count"], widest["mesh_face_count"]) and np.array_equal(on_device["mesh_faces"][:nf], widest["mesh_faces"][:nf])
        for k in on_device:
            cut = mv if k in ("xyz", "rgb", "conf", "index", "weight") else kf if k in ("faces", "face_index") else nf if k == "mesh_faces" else None
            assert np.array_equal(on_device[k][:cut].view(np.uint8), on_host[k][:cut].view(np.uint8)), k
        assert (on_host["xyz"][mv:] == f32(123456.0)).all() and (on_host["faces"][kf:] == -11).all() and (on_host["face_index"][kf:] == -11).all()
    finally:
        m.destroy()


def test_infer_cli_decimates_the_mesh_of_one_image_and_of_views(dev, tmp_path):
    """tools/infer.py --ply --mesh --decimate V: one image through md_infer_points_decimate, --views through ops.decimate_mesh
    behind the per-view meshes; refused with --voxel, --outlier-radius and without --mesh."""
    import importlib.util
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
    from burn_depth_amd.depth_anything3 import DepthAnything3
    from burn_depth_amd.inference import rgb_to_input_tensor
    spec = importlib.util.spec_from_file_location("infer_cli", os.path.join(ROOT, "tools", "infer.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = DepthAnything3Config.small()
    ck = str(tmp_path / "da3_small.safetensors")
    Wt.save_container(ck, Wt.generate_da3_weights(cfg, 0, Wt.INIT_PARITY), dtype="F16")
    rgb = np.load(os.path.join(ROOT, "tests", "golden", "test_jpg_rgb.npy"))
    img, flip = str(tmp_path / "img.npy"), str(tmp_path / "flip.npy")
    np.save(img, rgb)
    np.save(flip, np.ascontiguousarray(rgb[:, ::-1]))
    ply = str(tmp_path / "mesh.ply")
    V = 0.05
    head = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "2", "--edge-rtol", "0.5"]
    mesh = ["--mesh", "--mesh-rtol", "0.1"]
    assert cli.main(head + mesh + ["--decimate", str(V), "--voxel", "0.1"]) == 2
    assert cli.main(head + mesh + ["--decimate", str(V), "--outlier-radius", "0.1"]) == 2
    assert cli.main(head + ["--decimate", str(V)]) == 2
    assert cli.main(head + mesh + ["--decimate", str(V)]) == 0
    xyz, col, _, faces = P.read_ply_faces(ply)
    m = DepthAnything3.load_file(dev, cfg, ck)
    try:
        prep = P.prepare_depth_anything3_image(rgb, 518).rgb
        x = rgb_to_input_tensor(prep.tobytes(), 518, 518, dev)
        pc = m.infer_points(x, rgb=torch.from_numpy(prep[None].copy()).cuda(), dense=False, stride=2, edge_rtol=0.5, world=True,
                            mesh=dict(max_rtol=0.1), decimate=dict(voxel=V))
        full = m.infer_points(x, dense=False, stride=2, edge_rtol=0.5, world=True)
        want_xyz, want_col, _ = pc.points()
        want = pc.faces[:int(pc.face_count[-1])].cpu().numpy()
        assert 0 < len(want_xyz) < int(full.count[-1])
    finally:
        m.destroy()
    assert len(faces) > 0 and faces.max() < len(xyz) and np.array_equal(faces, want)
    assert np.array_equal(xyz.view(np.uint32), want_xyz.cpu().numpy().view(np.uint32)) and np.array_equal(col, want_col.cpu().numpy())
    # --views: the undecimated file, then the decimated one: one vertex per occupied voxel, taken from the undecimated rows
    views = ["--model", "depth-anything-3", "--checkpoint", ck, "--views", img, flip, "--ply", ply, "--stride", "2", "--output", str(tmp_path / "d.png")]
    assert cli.main(views + mesh) == 0
    xyz0, _, _, faces0 = P.read_ply_faces(ply)
    assert cli.main(views + mesh + ["--decimate", str(V)]) == 0
    xyz1, _, _, faces1 = P.read_ply_faces(ply)
    cells = lambda p: {tuple(c) for c in np.floor(p / f32(V)).astype(np.int64).tolist()}  # noqa: E731
    assert 0 < len(xyz1) < len(xyz0) and 0 < len(faces1) < len(faces0) and faces1.min() >= 0 and faces1.max() < len(xyz1)
    assert len(cells(xyz1)) == len(xyz1) and cells(xyz1) == cells(xyz0)
    assert {tuple(r) for r in xyz1.view(np.uint32).tolist()} <= {tuple(r) for r in xyz0.view(np.uint32).tolist()}
    assert (faces1[:, 0] != faces1[:, 1]).all() and (faces1[:, 1] != faces1[:, 2]).all() and (faces1[:, 0] != faces1[:, 2]).all()
