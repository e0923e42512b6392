"""md_infer_points_components: the model -> point cloud -> mesh call with the island removal behind the mesh stage.
The stage is md_op_mesh_components' launches on the call's list and on all faces of it, so every comparison is bit for bit
against `ops.mesh_components` on the outputs of the same call without it. All tests need an MI355X (`-m gpu`)."""
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
POISONS = dict(label=-9, component_faces=-9, component_stats=-5, faces=-11, face_index=-11, face_count=-5)


def _np(pc):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in vars(pc).items()}


def _poison(pc):
    for k, fill in POISONS.items():
        if getattr(pc, k) is not None:
            getattr(pc, k).fill_(fill)


def _cut_for(m, x, kw):
    """(max_rtol, min_faces, the call without the stage): the first edge test of a fixed ladder whose mesh, by the host
    reference, has at least three components with a face; min_faces = the size of the second largest, so that at least two are
    kept and at least one is dropped whenever three sizes differ"""
    for rtol in (0.2, 0.1, 0.05, 0.02, 0.01, 0.005):
        full = m.infer_points(x, mesh=dict(max_rtol=rtol), **kw)
        n, nf = int(full.count[-1].item()), int(full.face_count[-1].item())
        ref = P.mesh_components(full.faces[:nf].cpu().numpy(), n, 1)
        sizes = np.sort(ref.component_faces[ref.label == np.arange(n)])[::-1]
        sizes = sizes[sizes > 0]
        if len(sizes) >= 3 and sizes[1] > sizes[-1]:
            return rtol, int(sizes[1]), full
    raise AssertionError("no edge test of the ladder leaves three components of two sizes")


def _operator(dev, full, min_faces):
    """ops.mesh_components on the list and faces of the call without the stage, and the per-view counts from the host reference"""
    from burn_depth_amd import ops
    n, nf = int(full.count[-1].item()), int(full.face_count[-1].item())
    want = _np(ops.mesh_components(dev, full.faces[:nf], n, min_faces))
    ref = P.mesh_components(full.faces[:nf].cpu().numpy(), n, min_faces, face_counts=full.face_count[:-1].cpu().numpy())
    assert ref.stats[4] >= 1 and ref.stats[3] > ref.stats[4] and ref.stats[1] >= 1
    return want, ref, n, nf


def _same_components(got, want, ref, n, what):
    k = int(want["face_count"][-1])
    assert 0 < k, what
    assert got["face_count"].tolist() == ref.face_count.tolist(), (what, got["face_count"], ref.face_count)
    assert got["component_stats"].tolist() == want["component_stats"].tolist() == ref.stats.tolist(), what
    assert np.array_equal(got["label"][:n], want["label"]) and (got["label"][n:] == -1).all(), what
    assert np.array_equal(got["component_faces"][:n], want["component_faces"]) and (got["component_faces"][n:] == 0).all(), what
    assert np.array_equal(got["faces"][:k], want["faces"][:k]) and np.array_equal(got["face_index"][:k], want["face_index"][:k]), what
    assert (got["faces"][k:] == -11).all() and (got["face_index"][k:] == -11).all(), what  # the rows behind stay untouched


@pytest.mark.parametrize("model", ["da3", "pro"])
def test_model_call_equals_the_operator_eagerly_and_under_graph_replay(dev, model):
    m = _da3(dev, max_batch=3) if model == "da3" else _pro(dev, "small")
    try:
        B, S = (3, 70) if model == "da3" else (1, 512)
        x = _image(B, S).cuda()
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=model == "da3", rgb=rgb, stride=1 if model == "da3" else 4, **OPTS)
        rtol, min_faces, full = _cut_for(m, x, kw)
        want, ref, n, nf = _operator(dev, full, min_faces)
        mesh, comp = dict(max_rtol=rtol), dict(min_faces=min_faces)
        out = m.infer_points(x, mesh=mesh, components=comp, **kw)
        _poison(out)
        got = _np(m.infer_points(x, out=out, mesh=mesh, components=comp, **kw))
        _same_components(got, want, ref, n, (model, "eager"))
        # the in-call stage is face-only: the list and the map are those of the call without it
        f = _np(full)
        assert got["count"].tolist() == f["count"].tolist() and np.array_equal(got["pixel_index"], f["pixel_index"])
        for key in ("xyz", "rgb", "conf"):
            assert (f[key] is None) == (got[key] is None)
            assert f[key] is None or np.array_equal(got[key][:n].view(np.uint8), f[key][:n].view(np.uint8)), key
        # a capacity below the outputs: the true counts
        small = _np(m.infer_points(x, mesh=mesh, components=dict(min_faces=min_faces, face_capacity=5), **kw))
        assert small["face_count"].tolist() == got["face_count"].tolist() and np.array_equal(small["faces"], got["faces"][:5])
        m.enable_graph(True)
        out = m.infer_points(x, mesh=mesh, components=comp, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):
            _poison(out)
            out = m.infer_points(x, out=out, mesh=mesh, components=comp, **kw)
            _same_components(_np(out), want, ref, n, (model, "graph", call))
        assert m.query("allocs") == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


def test_the_rasteriser_sees_the_filtered_faces(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS)
        rtol, min_faces, full = _cut_for(m, x, kw)
        n = int(full.count[-1].item())
        pts = full.xyz[:n].cpu().numpy()
        c = pts.mean(0).astype(np.float64)
        d = 2.0 * float(np.percentile(np.linalg.norm(pts - c, axis=1), 80)) + 1e-3
        E = np.zeros((2, 3, 4), f32)
        E[:, :, :3], E[:, :, 3] = np.eye(3), np.array([0, 0, d]) - c
        E[1, 0, 3] += 0.1 * d
        cams = dict(H=48, W=56, focal_px=torch.tensor([40.0, 55.0]), extrinsics=torch.from_numpy(E))
        call = dict(mesh=dict(max_rtol=rtol), components=dict(min_faces=min_faces), raster=dict(**cams), **kw)
        for graph in (False, True):
            m.enable_graph(graph)
            out = m.infer_points(x, **call)
            for _ in range(2 if graph else 1):
                out = m.infer_points(x, out=out, **call)
            torch.cuda.synchronize()
            assert 0 < int(out.face_count[-1].item()) < int(full.face_count[-1].item())
            tri = ops.render_mesh(dev, out.xyz, out.faces, 48, 56, focal_px=cams["focal_px"], extrinsics=cams["extrinsics"].cuda(), rgb=out.rgb,
                                  face_count=out.face_count[-1:])
            torch.cuda.synchronize()
            for k in ("depth", "face", "rgb", "filled", "skipped"):
                assert torch.equal(getattr(out.raster, k), getattr(tri, k)), (graph, "raster", k)
            assert out.raster.filled[-1].item() > 0
    finally:
        m.enable_graph(False)
        m.destroy()


def test_null_and_zero_min_faces_are_the_call_without_it_and_the_refusals_leave_the_outputs_untouched(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, mesh=dict(max_rtol=0.05), **OPTS)
        m.enable_timing(True)
        names, outs = {}, {}
        for what, extra in (("none", dict()), ("null", dict(components=None)), ("zero", dict(components=dict(min_faces=0))),
                            ("on", dict(components=dict(min_faces=2)))):
            m.read_timing()
            outs[what] = _np(m.infer_points(x, **extra, **kw))
            names[what] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["none"] == names["null"] == names["zero"] and "points_mesh" in names["none"] and "points_components" not in names["none"]
        order = list(names["on"])
        assert order.index("points_mesh") < order.index("points_components")
        n, nf = int(outs["none"]["count"][-1]), int(outs["none"]["face_count"][-1])
        assert n > 0 and nf > 0
        for what in ("null", "zero"):
            for k, v in outs["none"].items():
                rows = n if k in ("xyz", "rgb", "conf") else nf if k == "faces" else None
                assert (v is None) == (outs[what][k] is None), (what, k)
                assert v is None or np.array_equal(v[:rows].view(np.uint8), outs[what][k][:rows].view(np.uint8)), (what, k)
        # refusals: nothing is written
        out = m.infer_points(x, components=dict(min_faces=2), **kw)
        for bad, text in ((dict(components=dict(min_faces=-1)), "min_faces"),
                          (dict(components=dict(min_faces=2), decimate=dict(voxel=0.05)), "decimation")):
            _poison(out)
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, out=out, **bad, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG and text in str(e.value), bad
            torch.cuda.synchronize()
            for k, fill in POISONS.items():
                assert getattr(out, k) is None or (getattr(out, k) == fill).all(), (bad, k)
        with pytest.raises(_lib.MdError) as e:  # without a mesh request
            m.infer_points(x, components=dict(min_faces=2), world=True, **OPTS)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
    finally:
        m.destroy()


def test_entries_through_ctypes_null_parts_refusals_and_host_memory(dev):
    """The narrower entries equal the widest with a null part; compact, comp's pointers with min_faces 0, faces without face_count and
    comp without a mesh are refused by the library itself; the caller's mesh outputs still hold the unfiltered mesh; the
    host-memory call equals the device-memory one."""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S = 2, 70
        rows, fcap = B * S * S, 2 * B * 69 * 69
        x = _image(B, S)
        xd = x.cuda()
        o = _points_opts(world=True, **OPTS)
        DEV, HOST = _lib.MD_MEM_DEVICE, _lib.MD_MEM_HOST
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        shapes = dict(xyz=((rows, 3), f32), conf=((rows,), f32), count=((B + 1,), np.int32), label=((rows,), np.int32),
                      component_faces=((rows,), np.int32), faces=((fcap, 3), np.int32), face_index=((fcap,), np.int32),
                      face_count=((B + 1,), np.int32), component_stats=((5,), np.int32), mesh_faces=((fcap, 3), np.int32),
                      mesh_face_count=((B + 1,), np.int32), pixel_index=((B, S, S), np.int32), point_map=((B, S, S, 3), f32))

        def call(entry, host=False, min_faces=3, with_mesh=True, stray=False, compact=0, no_count=False, no_list=False, voxel=False,
                 outlier=False):
            t = {k: np.full(shape, POISONS.get(k, -3), dt) for k, (shape, dt) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            p = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, p("xyz"), None, p("conf"), p("count"), rows, None)
            msh = _lib.MdPointsMesh(0.05, p("mesh_faces"), p("mesh_face_count"), fcap, p("pixel_index"))
            if no_list:  # no list at all, dense output only; the mesh part then carries its edge test alone
                outs = _lib.MdPointsOutputs(p("point_map"), None, None, None, None, None, 0, None)
                msh = _lib.MdPointsMesh(0.05, None, None, 0, None)
            if voxel or outlier:  # a mesh with outputs is refused with either on its own account: leave it its edge test alone
                msh = _lib.MdPointsMesh(0.05, None, None, 0, None)
            vox = _lib.MdPointsVoxel(0.05, None, None, None) if voxel else None
            outl = _lib.MdPointsOutlier(0.1, 2, None, None, None) if outlier else None
            comp = _lib.MdPointsComponents(min_faces, compact, p("label"), p("component_faces"), None, None, p("faces"), p("face_index"),
                                           None if no_count else p("face_count"), fcap, p("component_stats"))
            if min_faces == 0 and not stray:
                comp = _lib.MdPointsComponents(0, 0, None, None, None, None, None, None, None, 0, None)
            xin = x.numpy() if host else xd
            px = xin.ctypes.data if host else xin.data_ptr()
            kind = HOST if host else DEV
            head = (m._h, C.c_void_p(px), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None, C.byref(vox) if vox else None, None,
                    C.byref(msh) if with_mesh else None, None)
            if entry == "raster":
                rc = lib.md_infer_points_raster(*head, kind, None if host else st)
            elif entry == "decimate":
                rc = lib.md_infer_points_decimate(*head, None, None, kind, None if host else st)
            else:
                rc = lib.md_infer_points_components(*head, C.byref(outl) if outl else None, None, C.byref(comp) if entry == "components" else None, kind,
                                                    None if host else st)
            torch.cuda.synchronize()
            return rc, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        rc, widest = call("components-null")
        assert rc == 0
        n, nf = int(widest["count"][-1]), int(widest["mesh_face_count"][-1])
        assert n > 0 and nf > 0 and (widest["faces"] == -11).all()
        for what, (rc, other) in (("raster", call("raster")), ("decimate", call("decimate")), ("min_faces 0", call("components", min_faces=0))):
            assert rc == 0, what
            for k in widest:
                cut = n if k in ("xyz", "conf") else nf if k == "mesh_faces" else None
                assert np.array_equal(widest[k][:cut].view(np.uint8), other[k][:cut].view(np.uint8)), (what, k)
        for kw, text in ((dict(min_faces=0, stray=True), "without min_faces"), (dict(with_mesh=False), "mesh request"), (dict(compact=1), "compact"),
                         (dict(min_faces=-2), "min_faces"), (dict(no_count=True), "face_count"), (dict(no_list=True), "list's `count`"),
                         (dict(voxel=True), "no longer exist"), (dict(outlier=True), "no longer exist")):
            rc, left = call("components", **kw)
            assert rc == _lib.MD_ERR_INVALID_ARG and text in lib.md_last_error().decode(), (kw, lib.md_last_error())
            for k, v in left.items():
                assert (v == np.asarray(POISONS.get(k, -3), v.dtype)).all(), (kw, k)
        (rc_d, on_device), (rc_h, on_host) = call("components"), call("components", host=True)
        assert rc_d == 0 and rc_h == 0
        ref = P.mesh_components(widest["mesh_faces"][:nf], n, 3, face_counts=widest["mesh_face_count"][:-1])
        kf = int(on_device["face_count"][-1])
        assert on_device["face_count"].tolist() == ref.face_count.tolist() and on_device["component_stats"].tolist() == ref.stats.tolist()
        assert np.array_equal(on_device["faces"][:kf], ref.faces) and np.array_equal(on_device["label"][:n], ref.label)
        # the caller's mesh outputs still hold the unfiltered mesh
        assert np.array_equal(on_device["mesh_face_count"], widest["mesh_face_count"]) and np.array_equal(on_device["mesh_faces"][:nf], widest["mesh_faces"][:nf])
        for k in on_device:
            cut = n if k in ("xyz", "conf") else kf if k in ("faces", "face_index") else nf if k == "mesh_faces" else None
            assert np.array_equal(on_device[k][:cut].view(np.uint8), on_host[k][:cut].view(np.uint8)), k
        assert (on_host["faces"][kf:] == -11).all() and (on_host["face_index"][kf:] == -11).all()
    finally:
        m.destroy()


def test_infer_cli_removes_the_islands_of_one_image_and_of_views(dev, tmp_path):
    """tools/infer.py --ply --mesh --min-component-faces K: one image through md_infer_points_components and then
    ops.mesh_components(compact=True), so the file holds no floater vertex, while --raster-pose / --render-pose write the images of
    the model call (the filtered faces over its uncompacted list); --views through the operator behind the per-view
    meshes, and behind ops.decimate_mesh with --decimate; refused without --mesh and for a negative K."""
    import importlib.util
    from burn_depth_amd import ops
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
    K = 8
    head = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "2", "--edge-rtol", "0.5"]
    mesh = ["--mesh", "--mesh-rtol", "0.1"]
    assert cli.main(head + ["--min-component-faces", str(K)]) == 2
    assert cli.main(head + mesh + ["--min-component-faces", "-1"]) == 2
    m = DepthAnything3.load_file(dev, cfg, ck)
    try:
        prep = P.prepare_depth_anything3_image(rgb, 518).rgb
        x = rgb_to_input_tensor(prep.tobytes(), 518, 518, dev)
        full = m.infer_points(x, rgb=torch.from_numpy(prep[None].copy()).cuda(), dense=False, stride=2, edge_rtol=0.5, world=True,
                              mesh=dict(max_rtol=0.1))
        n, nf = int(full.count[-1].item()), int(full.face_count[-1].item())
        ref = P.mesh_components(full.faces[:nf].cpu().numpy(), n, K, compact=True, xyz=full.xyz[:n].cpu().numpy(), rgb=full.rgb[:n].cpu().numpy())
    finally:
        m.destroy()
    assert ref.stats[1] > 0 and 0 < len(ref.index) < n  # the reference drops islands and floaters here
    # two cameras that look at the cloud from in front of it: the images of the model call are written beside the file
    pts = full.xyz[:n].cpu().numpy()
    c = pts.mean(0).astype(np.float64)
    d = 2.0 * float(np.percentile(np.linalg.norm(pts - c, axis=1), 80)) + 1e-3
    E = np.zeros((2, 3, 4), f32)
    E[:, :, :3], E[:, :, 3] = np.eye(3), np.array([0, 0, d]) - c
    E[1, 0, 3] += 0.1 * d
    Kc = np.array([[40, 0, 28], [0, 40, 24], [0, 0, 1]], f32)
    pose, intr = str(tmp_path / "pose.npy"), str(tmp_path / "K.npy")
    np.save(pose, E)
    np.save(intr, Kc)
    ras, ren = str(tmp_path / "raster.png"), str(tmp_path / "render.png")
    cams = ["--render-size", "48", "56", "--render-intrinsics", intr, "--raster-pose", pose, "--raster-out", ras, "--render-pose", pose,
            "--render-out", ren, "--render-radius", "1"]
    assert cli.main(head + mesh + ["--min-component-faces", str(K)] + cams) == 0
    xyz, col, _, faces = P.read_ply_faces(ply)
    assert np.array_equal(faces, ref.faces) and np.array_equal(xyz.view(np.uint32), ref.xyz.view(np.uint32)) and np.array_equal(col, ref.rgb)
    assert set(np.unique(faces).tolist()) == set(range(len(xyz)))
    # the raster is `ops.render_mesh` on the filtered faces over the model call's uncompacted list, the render `ops.render_points` on that list
    kept = ops.mesh_components(dev, full.faces[:nf], n, K)
    assert 0 < int(kept.face_count[-1].item()) < nf
    view = dict(intrinsics=np.broadcast_to(Kc, (2, 3, 3)).copy(), extrinsics=E)
    tri = ops.render_mesh(dev, full.xyz, kept.faces, 48, 56, rgb=full.rgb, face_count=kept.face_count[-1:], **view)
    dots = ops.render_points(dev, full.xyz, 48, 56, rgb=full.rgb, count=full.count[-1:], radius=1, **view)
    torch.cuda.synchronize()
    assert int(tri.filled[0].item()) > 0 and int(dots.filled[0].item()) > 0
    want_ras, want_ren = str(tmp_path / "want_raster.png"), str(tmp_path / "want_render.png")
    P.save_depth_map(tri.depth[:1].cpu().numpy(), want_ras, None, None)
    P.save_depth_map(dots.depth[:1].cpu().numpy(), want_ren, None, None)
    with open(ras, "rb") as got, open(want_ras, "rb") as want:
        assert got.read() == want.read()
    with open(ren, "rb") as got, open(want_ren, "rb") as want:
        assert got.read() == want.read()
    # --views: the unfiltered file, the filtered one, and the filtered one behind the decimation
    views = ["--model", "depth-anything-3", "--checkpoint", ck, "--views", img, flip, "--ply", ply, "--stride", "2", "--output", str(tmp_path / "d.png")]
    assert cli.main(views + mesh) == 0
    xyz0, col0, _, faces0 = P.read_ply_faces(ply)
    assert cli.main(views + mesh + ["--min-component-faces", str(K)]) == 0
    xyz1, col1, _, faces1 = P.read_ply_faces(ply)
    ref = P.mesh_components(faces0, len(xyz0), K, compact=True, xyz=xyz0, rgb=col0)
    assert ref.stats[1] > 0 and np.array_equal(faces1, ref.faces) and np.array_equal(xyz1.view(np.uint32), ref.xyz.view(np.uint32))
    assert cli.main(views + mesh + ["--decimate", "0.05"]) == 0
    xyz2, col2, _, faces2 = P.read_ply_faces(ply)
    assert cli.main(views + mesh + ["--decimate", "0.05", "--min-component-faces", str(K)]) == 0
    xyz3, _, _, faces3 = P.read_ply_faces(ply)
    ref = P.mesh_components(faces2, len(xyz2), K, compact=True, xyz=xyz2, rgb=col2)
    assert np.array_equal(faces3, ref.faces) and np.array_equal(xyz3.view(np.uint32), ref.xyz.view(np.uint32)) and len(xyz3) <= len(xyz2)
