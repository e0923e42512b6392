"""md_infer_points_smooth: the model -> point cloud -> mesh call with the smoothing behind the mesh stage and the island removal
(DESIGN 12.10). The stage is md_op_smooth_mesh's launches on the call's list and on the faces the rasteriser reads, so every
comparison is bit for bit against `ops.smooth_mesh` on the outputs of the same call without it. All tests need an MI355X
(`-m gpu`)."""
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
from points_util import _da3, _image, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTS = dict(depth_min=1e-3, depth_max=1e6)
POISON = -7.0


def _step(xyz):
    """the CLI's default lattice: the largest finite |coordinate| of the list / 2^21"""
    v = xyz.abs()
    return float(np.float32(float(v[torch.isfinite(v)].max().item()) / 2097152.0))


def _poison(pc):
    for t in (pc.smooth.xyz, pc.smooth.normals):
        if t is not None:
            t.fill_(POISON)
    pc.smooth.stats.fill_(-5)


def _same_smooth(got, want, n, what):
    torch.cuda.synchronize()
    assert torch.equal(got.stats, want.stats) and int(want.stats[4].item()) > 0, (what, got.stats, want.stats)
    assert torch.equal(got.xyz[:n].view(torch.int32), want.xyz[:n].view(torch.int32)), what
    assert torch.equal(got.normals[:n].view(torch.int32), want.normals[:n].view(torch.int32)), what
    assert (got.xyz[n:] == POISON).all() and (got.normals[n:] == POISON).all(), what  # rows behind the list stay untouched


def _scene(dev, B=3):
    x = _image(B, 70).cuda()
    rgb = torch.randint(0, 256, (B, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    return x, dict(world=True, rgb=rgb, normals=True, **OPTS)


@pytest.mark.parametrize("components", [False, True])
def test_model_call_equals_the_operator_eagerly_and_under_graph_replay(dev, components):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=3)
    try:
        x, kw = _scene(dev)
        E = np.zeros((1, 3, 4), f32)
        E[0, :, :3] = np.eye(3)
        kw["render"] = dict(H=32, W=40, focal_px=torch.tensor([30.0]), extrinsics=torch.from_numpy(E))
        extra = dict(mesh=dict(max_rtol=0.2))
        if components:
            extra["components"] = dict(min_faces=2)
        full = m.infer_points(x, **extra, **kw)
        n, nf = int(full.count[-1].item()), int(full.face_count[-1].item())
        assert n > 0 and nf > 0
        sm = dict(step=_step(full.xyz[:n]), iterations=3, lam=0.5, mu=-0.53, pin_boundary=True, normals=True)
        want = ops.smooth_mesh(dev, full.xyz[:n], full.faces[:nf], sm["step"], 3, 0.5, mu=-0.53, pin_boundary=True, normals=True)
        ref = P.smooth_mesh(full.xyz[:n].cpu().numpy(), full.faces[:nf].cpu().numpy(), sm["step"], 3, 0.5, mu=-0.53, normals=True)
        assert want.stats.cpu().numpy().tolist() == ref.stats.tolist() and np.array_equal(want.xyz.cpu().numpy().view(np.uint32), ref.xyz.view(np.uint32))
        out = m.infer_points(x, smooth=sm, **extra, **kw)
        _poison(out)
        out = m.infer_points(x, out=out, smooth=sm, **extra, **kw)
        _same_smooth(out.smooth, want, n, "eager")
        # the list, the per-pixel normals, the faces and the point render are those of the call without the stage
        assert torch.equal(out.count, full.count) and torch.equal(out.face_count, full.face_count) and torch.equal(out.faces[:nf], full.faces[:nf])
        for key in ("xyz", "rgb", "conf", "normals"):
            a, b = getattr(out, key), getattr(full, key)
            assert (a is None) == (b is None) and (a is None or torch.equal(a[:n].view(torch.uint8), b[:n].view(torch.uint8))), key
        for key in ("depth", "index", "rgb", "filled"):
            assert torch.equal(getattr(out.render, key), getattr(full.render, key)), key
        m.enable_graph(True)
        out = m.infer_points(x, smooth=sm, **extra, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):
            _poison(out)
            out = m.infer_points(x, out=out, smooth=sm, **extra, **kw)
            _same_smooth(out.smooth, want, n, ("graph", call))
        assert m.query("allocs") == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


def test_the_rasteriser_draws_the_smoothed_rows(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=3)
    try:
        x, kw = _scene(dev)
        full = m.infer_points(x, mesh=dict(max_rtol=0.2), **kw)
        n = int(full.count[-1].item())
        pts = full.xyz[:n].cpu().numpy()
        c = pts.mean(0).astype(np.float64)
        d = 2.0 * float(np.percentile(np.linalg.norm(pts - c, axis=1), 80)) + 1e-3
        E = np.zeros((2, 3, 4), f32)
        E[:, :, :3], E[:, :, 3] = np.eye(3), np.array([0, 0, d]) - c
        E[1, 0, 3] += 0.1 * d
        cams = dict(H=48, W=56, focal_px=torch.tensor([40.0, 55.0]), extrinsics=torch.from_numpy(E))
        sm = dict(step=_step(full.xyz[:n]), iterations=10, lam=0.5, pin_boundary=False)
        out = m.infer_points(x, mesh=dict(max_rtol=0.2), raster=dict(**cams), smooth=sm, **kw)
        torch.cuda.synchronize()
        assert int(out.smooth.stats[4].item()) > 0
        view = dict(focal_px=cams["focal_px"], extrinsics=cams["extrinsics"].cuda(), rgb=out.rgb, face_count=out.face_count[-1:])
        tri = ops.render_mesh(dev, out.smooth.xyz, out.faces, 48, 56, **view)
        rough = ops.render_mesh(dev, out.xyz, out.faces, 48, 56, **view)
        torch.cuda.synchronize()
        for k in ("depth", "face", "rgb", "filled", "skipped"):
            assert torch.equal(getattr(out.raster, k), getattr(tri, k)), k
        assert out.raster.filled[-1].item() > 0 and not torch.equal(tri.depth, rough.depth)
    finally:
        m.destroy()


def test_null_and_zero_iterations_are_the_call_without_it_and_the_refusals_leave_the_outputs_untouched(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, mesh=dict(max_rtol=0.05), components=dict(min_faces=2), **OPTS)
        on = dict(step=1e-4, iterations=2, lam=0.5, mu=-0.53, normals=True)
        m.enable_timing(True)
        names, outs = {}, {}
        for what, extra in (("none", dict()), ("null", dict(smooth=None)), ("zero", dict(smooth=dict(step=1e-4, iterations=0, lam=0.5))),
                            ("on", dict(smooth=on))):
            m.read_timing()
            outs[what] = m.infer_points(x, **extra, **kw)
            names[what] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        torch.cuda.synchronize()
        assert names["none"] == names["null"] == names["zero"] and "points_components" in names["none"] and "points_smooth" not in names["none"]
        order = list(names["on"])
        assert order.index("points_mesh") < order.index("points_components") < order.index("points_smooth")
        assert [v for v in order if v != "points_smooth"] == list(names["none"])
        n, nf = int(outs["none"].count[-1].item()), int(outs["none"].face_count[-1].item())
        assert n > 0 and nf > 0
        for what in ("null", "zero"):
            assert outs[what].smooth is None
            for k, v in vars(outs["none"]).items():
                if isinstance(v, torch.Tensor):
                    rows = n if k in ("xyz", "rgb", "conf") else nf if k in ("faces", "face_index") else None
                    assert torch.equal(v[:rows].view(torch.uint8), getattr(outs[what], k)[:rows].view(torch.uint8)), (what, k)
        # refusals: nothing is written
        out = outs["on"]
        nan = float("nan")
        bad = [(dict(smooth=dict(on, step=0.0)), "step"), (dict(smooth=dict(on, step=nan)), "step"), (dict(smooth=dict(on, lam=0.0)), "lambda"),
               (dict(smooth=dict(on, lam=1.5)), "lambda"), (dict(smooth=dict(on, mu=0.25)), "mu"), (dict(smooth=dict(on, mu=-1.5)), "mu"),
               (dict(smooth=dict(on, iterations=1025)), "iterations"), (dict(smooth=dict(on, iterations=-1)), "iterations")]
        for extra, text in bad:
            _poison(out)
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, out=out, **extra, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG and text in str(e.value), extra
            torch.cuda.synchronize()
            assert (out.smooth.xyz == POISON).all() and (out.smooth.normals == POISON).all() and (out.smooth.stats == -5).all(), extra
        lone = dict(world=True, **OPTS)
        for extra, text in ((dict(mesh=dict(max_rtol=0.05), decimate=dict(voxel=0.05)), "decimation"), (dict(), "mesh")):
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, smooth=on, **extra, **lone)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG and text in str(e.value), (extra, str(e.value))
    finally:
        m.destroy()


def test_entries_through_ctypes_stray_pointers_missing_list_and_host_memory(dev):
    """A pointer with iterations == 0, the stage without a mesh request, without the list's count, with outlier removal, and
    behind components without their faces are refused by the library itself with nothing written; the narrower entry equals the
    widest with a null part; the host-memory call equals the device-memory one."""
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
        lattice = dict(step=1e-4)  # set from the list of the first call below
        shapes = dict(xyz=((rows, 3), f32), count=((B + 1,), np.int32), faces=((fcap, 3), np.int32), face_count=((B + 1,), np.int32),
                      sxyz=((rows, 3), f32), snrm=((rows, 3), f32), sstats=((5,), np.int32), point_map=((B, S, S, 3), f32))

        def call(entry="smooth", host=False, iterations=2, stray=False, with_mesh=True, no_list=False, outlier=False, comp_no_faces=False):
            t = {k: np.full(shape, -3, dt) for k, (shape, dt) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            p = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, p("xyz"), None, None, p("count"), rows, None)
            msh = _lib.MdPointsMesh(0.05, p("faces"), p("face_count"), fcap, None)
            if no_list:
                outs = _lib.MdPointsOutputs(p("point_map"), None, None, None, None, None, 0, None)
            if no_list or outlier:
                msh = _lib.MdPointsMesh(0.05, None, None, 0, None)
            outl = _lib.MdPointsOutlier(0.1, 2, None, None, None) if outlier else None
            comp = _lib.MdPointsComponents(2, 0, None, None, None, None, None, None, None, 0, None) if comp_no_faces else None
            smo = _lib.MdPointsSmooth(lattice["step"], 0.5, -0.53, iterations, 1, p("sxyz"), p("snrm"), p("sstats"))
            if iterations == 0 and not stray:
                smo = _lib.MdPointsSmooth(0.0, 0.0, 0.0, 0, 0, None, None, None)
            xin = x.numpy() if host else xd
            kind = HOST if host else DEV
            head = (m._h, C.c_void_p(xin.ctypes.data if host else xin.data_ptr()), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs),
                    None, None, None, C.byref(msh) if with_mesh else None, None, C.byref(outl) if outl else None, None,
                    C.byref(comp) if comp else None)
            if entry == "components":
                rc = lib.md_infer_points_components(*head, kind, None if host else st)
            else:
                rc = lib.md_infer_points_smooth(*head, C.byref(smo) if entry == "smooth" else None, kind, None if host else st)
            torch.cuda.synchronize()
            return rc, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        rc, widest = call("smooth-null")
        assert rc == 0
        n, nf = int(widest["count"][-1]), int(widest["face_count"][-1])
        assert n > 0 and nf > 0 and (widest["sxyz"] == -3).all()
        lattice["step"] = _step(torch.from_numpy(widest["xyz"][:n]))
        for what, (rc, other) in (("components", call("components")), ("iterations 0", call(iterations=0))):
            assert rc == 0, what
            for k in widest:
                cut = n if k == "xyz" else nf if k == "faces" else None
                assert np.array_equal(widest[k][:cut].view(np.uint8), other[k][:cut].view(np.uint8)), (what, k)
        for kw, text in ((dict(iterations=0, stray=True), "without iterations"), (dict(with_mesh=False), "mesh request"),
                         (dict(no_list=True), "`count`"), (dict(outlier=True), "no longer exist"), (dict(comp_no_faces=True), "`faces`")):
            rc, left = call(**kw)
            assert rc == _lib.MD_ERR_INVALID_ARG and text in lib.md_last_error().decode(), (kw, lib.md_last_error())
            for k, v in left.items():
                assert (v == np.asarray(-3, v.dtype)).all(), (kw, k)
        (rc_d, on_device), (rc_h, on_host) = call(), call(host=True)
        assert rc_d == 0 and rc_h == 0
        ref = P.smooth_mesh(widest["xyz"][:n], widest["faces"][:nf], lattice["step"], 2, 0.5, mu=-0.53, normals=True)
        assert on_device["sstats"].tolist() == ref.stats.tolist() and ref.stats[4] > 0
        assert np.array_equal(on_device["sxyz"][:n].view(np.uint32), ref.xyz.view(np.uint32))
        assert np.array_equal(on_device["snrm"][:n].view(np.uint32), ref.normals.view(np.uint32))
        for k in on_device:
            cut = n if k in ("xyz", "sxyz", "snrm") else nf if k == "faces" else None
            assert np.array_equal(on_device[k][:cut].view(np.uint8), on_host[k][:cut].view(np.uint8)), k
        assert (on_host["sxyz"][n:] == -3).all() and (on_device["sxyz"][n:] == -3).all()
    finally:
        m.destroy()


def test_infer_cli_smooths_one_image_views_and_the_decimated_mesh(dev, tmp_path):
    """tools/infer.py --ply --mesh --smooth ITER: one image through the stage of the model call, --views and --decimate through
    ops.smooth_mesh on the final vertices and faces; the file holds the operator's positions and, with --normals, its normals."""
    import importlib.util
    from burn_depth_amd import ops
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config
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
    one = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "4", "--edge-rtol", "0.5"]
    views = ["--model", "depth-anything-3", "--checkpoint", ck, "--views", img, flip, "--ply", ply, "--stride", "4", "--output", str(tmp_path / "d.png")]
    mesh = ["--mesh", "--mesh-rtol", "0.1", "--normals"]
    smooth = ["--smooth", "3"]
    assert cli.main(one + smooth) == 2 and cli.main(one + mesh + ["--smooth", "-1"]) == 2 and cli.main(one + mesh + ["--smooth", "1025"]) == 2

    def operator(xyz0, faces0):
        xyz_d = torch.from_numpy(xyz0).cuda()
        step = float(np.float32(float(np.abs(xyz0[np.isfinite(xyz0)]).max()) / 2097152.0))
        got = ops.smooth_mesh(dev, xyz_d, torch.from_numpy(faces0.astype(np.int32)).cuda(), step, 3, 0.5, mu=-0.53, pin_boundary=True, normals=True)
        torch.cuda.synchronize()
        assert int(got.stats[4].item()) > 0
        return got.xyz.cpu().numpy(), got.normals.cpu().numpy()

    for head, extra in ((one, []), (views, []), (one, ["--decimate", "0.05"]), (views, ["--decimate", "0.05"])):
        assert cli.main(head + mesh + extra) == 0
        xyz0, col0, _, faces0 = P.read_ply_faces(ply)
        assert cli.main(head + mesh + extra + smooth) == 0
        xyz1, col1, nrm1, faces1 = P.read_ply_faces(ply)
        want_xyz, want_nrm = operator(xyz0, faces0)
        assert np.array_equal(faces1, faces0) and np.array_equal(col1, col0), extra
        assert np.array_equal(xyz1.view(np.uint32), want_xyz.view(np.uint32)) and not np.array_equal(xyz1, xyz0), extra
        assert np.array_equal(nrm1.view(np.uint32), want_nrm.view(np.uint32)), extra
