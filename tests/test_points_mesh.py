"""The mesh of the list in the combined calls: `ops.unproject(mesh=)` (md_op_unproject_mesh) against the host reference
pipeline.unproject_depth -> pipeline.pixel_index -> pipeline.mesh_grid, and `infer_points(mesh=)` (md_infer_points_mesh) against
`ops.unproject(mesh=)` on the depth and cameras of the call without a mesh. include/mi_depth.h states the contract, DESIGN 12.5
the kernels. The outputs are integers: every comparison is np.array_equal. Runs with `-m gpu` on an MI355X."""
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
from points_util import _bits, _cameras, _da3, _da3_subset, _image, _pro, _t, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
MESH = ("faces", "face_count", "pixel_index")


def _scene(B, H, W, seed=7):
    """A wavy surface with a planted step, a few invalid depths and a confidence map"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    d = np.stack([2.0 + 0.3 * np.sin(0.11 * u + b) + 0.2 * np.cos(0.07 * v) for b in range(B)]).astype(f32)
    d *= (1 + 0.004 * rng.standard_normal(d.shape)).astype(f32)
    d[:, H // 4:H // 2, W // 3:2 * W // 3] *= f32(0.8)
    d[rng.random(d.shape) < 0.03] = 0.0
    d[0, 0, 0], d[-1, -1, -1] = np.nan, np.inf
    conf = rng.uniform(0.5, 2.0, d.shape).astype(f32)
    K, E = _cameras(rng, B, H, W)
    return d, conf, K, E


def _mesh_np(pc):
    torch.cuda.synchronize()
    return {k: (getattr(pc, k).cpu().numpy() if getattr(pc, k) is not None else None) for k in MESH + ("count", "xyz", "point_map")}


def _same_mesh(got, want, what=""):
    """faces below min(face_count[B], capacity), the counts and the map"""
    assert np.array_equal(got["face_count"], want["face_count"]), (what, got["face_count"], want["face_count"])
    n = min(int(want["face_count"][-1]), len(want["faces"]), len(got["faces"]))
    assert np.array_equal(got["faces"][:n], want["faces"][:n]), what
    if want["pixel_index"] is not None and got["pixel_index"] is not None:
        assert np.array_equal(got["pixel_index"], want["pixel_index"]), what
    return n


CASES = [  # use_conf, edge_rtol, stride, normal_min_cos, world, max_rtol
    (1, 0.5, 1, 0.0, 1, 0.05), (1, 0.0, 2, 0.3, 0, 0.05), (0, 0.05, 3, 0.0, 1, 0.0), (1, 0.5, 2, 0.3, 1, 0.02)]


@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (3, 70, 98), (1, 65, 64)])
def test_unproject_mesh_is_identical_to_the_host_reference(dev, B, H, W):
    from burn_depth_amd import ops
    d, conf, K, E = _scene(B, H, W)
    for use_conf, edge, stride, min_cos, world, rtol in CASES:
        kw = dict(pixel_offset=0.5, edge_rtol=edge, stride=stride, world=bool(world), conf_min=1.0 if use_conf else 0.0)
        cf = conf if use_conf else None
        ref = P.unproject_depth(d, K, E if world else None, conf=cf, normal_min_cos=min_cos, **kw)
        pi = P.pixel_index(ref, stride)
        rows = int(ref.count[-1])
        assert 50 < rows < B * H * W and np.array_equal(pi >= 0, (ref.mask != 0) & (P.pixel_index(np.ones_like(ref.mask), stride) >= 0))
        for cap in (None, rows // 2 + 1):  # the vertex limit is the capacity of the list: ample, and in the middle of it
            pc = ops.unproject(dev, _t(d), intrinsics=_t(K), extrinsics=_t(E) if world else None, conf=_t(cf), capacity=cap,
                               normal_min_cos=min_cos, mesh=dict(max_rtol=rtol), **kw)
            got = _mesh_np(pc)
            limit = len(got["xyz"])
            faces, count = P.mesh_grid(d, pi, stride=stride, max_rtol=rtol, vertex_limit=limit)
            what = (use_conf, edge, stride, min_cos, world, rtol, cap)
            n = _same_mesh(got, dict(faces=faces, face_count=count, pixel_index=pi), what)
            assert n == len(faces) > 0 and got["faces"][:n].max() < min(rows, limit), what
            assert np.array_equal(got["count"], ref.count), what
            # pixel <-> row: the list row the map names is the point of that pixel
            sel = (pi >= 0) & (pi < limit)
            assert np.array_equal(_bits(got["xyz"][pi[sel]]), _bits(got["point_map"][sel])), what
        assert count[-1] < P.mesh_grid(d, pi, stride=stride, max_rtol=rtol)[1][-1]  # the limit in mid-list removed faces


def test_each_mesh_output_alone_and_a_short_face_capacity(dev):
    from burn_depth_amd import ops
    from burn_depth_amd.depth_pro import PointCloud
    B, H, W = 2, 37, 53
    d, conf, K, E = _scene(B, H, W)
    kw = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
    full = _mesh_np(ops.unproject(dev, _t(d), intrinsics=_t(K), mesh=dict(max_rtol=0.05), **kw))
    nf, cap = int(full["face_count"][-1]), len(full["xyz"])
    assert nf > 100
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device="cuda")  # noqa: E731
    for names in (("faces", "face_count"), ("face_count",), ("pixel_index",), ("face_count", "pixel_index")):
        out = PointCloud(xyz=torch.empty((cap, 3), device="cuda"), count=i32(B + 1))
        store = i32(nf // 2 * 3 + 32)
        if "faces" in names:
            out.faces = store[:nf // 2 * 3].view(-1, 3)  # a capacity in the middle of the faces
        if "face_count" in names:
            out.face_count = i32(B + 1)
        if "pixel_index" in names:
            out.pixel_index = i32(B, H, W)
        ops.unproject(dev, _t(d), intrinsics=_t(K), dense=False, out=out, mesh=dict(max_rtol=0.05), **kw)
        torch.cuda.synchronize()
        for k in names:
            got = getattr(out, k).cpu().numpy()
            assert np.array_equal(got, full[k][:len(got)]), (names, k)
        assert (store[nf // 2 * 3:] == -7).all(), names
    # capacity 0 of the list: no corner is usable; face_capacity 0: counts only
    pc = ops.unproject(dev, _t(d), intrinsics=_t(K), capacity=0, mesh=True, **kw)
    assert _mesh_np(pc)["face_count"].tolist() == [0, 0, 0]
    pc = ops.unproject(dev, _t(d), intrinsics=_t(K), mesh=dict(max_rtol=0.05, face_capacity=0), **kw)
    assert np.array_equal(_mesh_np(pc)["face_count"], full["face_count"])


def _op_bytes(dev, entry, d, K, mesh):
    """md_op_unproject_normals or md_op_unproject_mesh (mesh: None, or an all-null md_points_mesh) on poisoned outputs -> bytes"""
    from burn_depth_amd.points import _points_opts
    B, H, W = d.shape
    t = dict(point_map=torch.full((B, H, W, 3), 123456.0, device="cuda"), mask=torch.full((B, H, W), 77, dtype=torch.uint8, device="cuda"),
             xyz=torch.full((B * H * W, 3), 123456.0, device="cuda"), count=torch.full((B + 1,), -5, dtype=torch.int32, device="cuda"),
             normal_map=torch.full((B, H, W, 3), 123456.0, device="cuda"), normals=torch.full((B * H * W, 3), 123456.0, device="cuda"))
    p = lambda k: t[k].data_ptr()  # noqa: E731
    outs = _lib.MdPointsOutputs(p("point_map"), p("mask"), p("xyz"), None, None, p("count"), B * H * W, None)
    nrm = _lib.MdPointsNormals(p("normal_map"), p("normals"), 0.3)
    o = _points_opts(pixel_offset=0.5, stride=2, edge_rtol=0.5)
    dd, kk = _t(d), _t(K)
    cam = _lib.MdPointsCameras(kk.data_ptr(), None, None)
    head = (dev.handle, C.c_void_p(dd.data_ptr()), None, None, B, H, W, C.byref(cam), C.byref(o), C.byref(outs), C.byref(nrm))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "normals":
        _lib.check(_lib.load().md_op_unproject_normals(*head, st))
    else:
        _lib.check(_lib.load().md_op_unproject_mesh(*head, C.byref(mesh) if mesh is not None else None, st))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in t.items()}


def test_null_mesh_is_the_normals_operator(dev):
    """(An operator keeps no launch record; the launch names of a NULL mesh are compared on the model call below.)"""
    d, _, K, _ = _scene(2, 37, 53)
    want = _op_bytes(dev, "normals", d, K, None)
    assert _op_bytes(dev, "mesh", d, K, None) == want
    assert _op_bytes(dev, "mesh", d, K, _lib.MdPointsMesh(0.05, None, None, 0, None)) == want


# ---------------------------------------------------------------------------------------------------------------------------------
# md_infer_points_mesh
# ---------------------------------------------------------------------------------------------------------------------------------
def test_da3_mesh_equals_the_operator_on_the_calls_depth(dev):
    from burn_depth_amd import ops
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        _, conf, extr, intr = _da3_subset(m, x)
        forms = (dict(), dict(conf_percentile=30), dict(normals=True, normal_min_cos=0.05), dict(conf_percentile=30, normals=True, normal_min_cos=0.05))
        for i, form in enumerate(forms):
            for mesh in (dict(max_rtol=0.0), dict(max_rtol=0.1, pixel_index=False)):
                kw = dict(world=True, **OPTS)
                plain = m.infer_points(x, **form, **kw)
                op_form = {k: v for k, v in form.items() if k in ("normals", "normal_min_cos")}
                want = _mesh_np(ops.unproject(dev, plain.depth, intrinsics=intr, extrinsics=extr, conf=conf, mesh=mesh, **op_form, **kw))
                got = m.infer_points(x, mesh=mesh, **form, **kw)
                assert (got.pixel_index is None) == (mesh.get("pixel_index") is False)
                n = _same_mesh(_mesh_np(got), want, (i, mesh))
                print(f"da3 form {i} {mesh}: {n} faces of {int(plain.count[-1])} points")
                assert n > 100, (i, mesh, n)
                rows = min(int(plain.count[-1]), len(plain.xyz))  # the cloud is the one of the call without a mesh
                assert torch.equal(got.count, plain.count) and torch.equal(got.xyz[:rows], plain.xyz[:rows]) and torch.equal(got.depth, plain.depth)
                assert int(got.faces[:n].max()) < rows
    finally:
        m.destroy()


def test_depth_pro_mesh_with_rendering(dev):
    from burn_depth_amd import ops
    m = _pro(dev, "tiny")
    try:
        x = _image(2, 512).cuda()
        ref = m.infer(x)
        kw = dict(dense=False, **OPTS)
        mesh = dict(max_rtol=0.05)
        want = _mesh_np(ops.unproject(dev, ref.depth, focal_px=ref.focallength_px, mesh=mesh, **kw))
        got = m.infer_points(x, mesh=mesh, **kw)
        n = _same_mesh(_mesh_np(got), want, "depth pro")
        print(f"depth pro: {n} faces of {int(got.count[-1])} points")
        assert n > 100
        # together with render=: the images are those of the call without a mesh, the mesh that of the call without rendering
        xyz = got.xyz[:int(got.count[-1])].cpu().numpy()
        with np.errstate(all="ignore"):
            reach = np.percentile(np.abs(xyz[:, :2] / xyz[:, 2:]), 90)
        render = dict(H=48, W=64, focal_px=torch.tensor([0.4 * 48 / reach], device="cuda"), radius=1)
        only = m.infer_points(x, render=render, **kw)
        both = m.infer_points(x, render=render, mesh=mesh, **kw)
        _same_mesh(_mesh_np(both), want, "with render")
        torch.cuda.synchronize()
        assert int(only.render.filled[-1]) > 100
        for k in ("depth", "index", "filled"):
            assert torch.equal(getattr(both.render, k), getattr(only.render, k)), k
    finally:
        m.destroy()


FILL = dict(xyz=123456.0, count=-7, depth=123456.0, faces=-7, face_count=-7, pixel_index=-7)
CANARY = 64


def _call(m, entry, x, host, face_cap, mesh=True, thin=0.0, max_rtol=0.2, faces=True, face_count=True, face_capacity=None):
    """md_infer_points_render or md_infer_points_mesh through ctypes, everything in host or in device memory -> (rc, outputs).
    face_cap: the faces the buffer holds, and the struct's face_capacity unless that is given."""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    B, S = x.shape[0], x.shape[2]
    cap = B * 35 * 35
    shapes = dict(xyz=((cap, 3), f32), count=((B + 1,), np.int32), depth=((B, S, S), f32), faces=((face_cap * 3 + CANARY,), np.int32),
                  face_count=((B + 1 + CANARY,), np.int32), pixel_index=((B * S * S + CANARY,), np.int32))
    t = {k: np.full(shape, FILL[k], dt) for k, (shape, dt) in shapes.items()}
    if not host:
        t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
    outs = _lib.MdPointsOutputs(None, None, ptr("xyz"), None, None, ptr("count"), cap, ptr("depth"))
    g = _lib.MdPointsMesh(max_rtol, ptr("faces") if faces else None, ptr("face_count") if face_count else None,
                          face_cap if face_capacity is None else face_capacity, ptr("pixel_index"))
    vox = _lib.MdPointsVoxel(thin, None, None, None)
    o = _points_opts(world=True, **OPTS)
    kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
    xin = x.cpu().numpy() if host else x
    st = None if host else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (m._h, C.c_void_p(xin.ctypes.data if host else xin.data_ptr()), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None,
            C.byref(vox) if thin else None, None)
    if entry == "render":
        rc = lib.md_infer_points_render(*head, kind, st)
    else:
        rc = lib.md_infer_points_mesh(*head, C.byref(g) if mesh else None, kind, st)
    torch.cuda.synchronize()
    return rc, {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}


def test_null_mesh_is_the_render_entry(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        m.enable_timing(True)
        names, outs = {}, {}
        for entry in ("render", "mesh", "with"):
            m.read_timing()
            rc, outs[entry] = _call(m, "render" if entry == "render" else "mesh", x, False, 100, mesh=entry == "with")
            assert rc == _lib.MD_OK
            names[entry] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["render"] == names["mesh"] and "points_unproject" in names["mesh"] and "points_mesh" not in names["mesh"]
        at = names["with"].index("points_unproject")
        assert names["with"][at + 1] == "points_mesh" and [n for n in names["with"] if n != "points_mesh"] == names["render"]
        for k in outs["render"]:
            assert np.array_equal(outs["render"][k].view(np.uint8), outs["mesh"][k].view(np.uint8)), k
        for k in MESH:
            assert (outs["mesh"][k] == FILL[k]).all(), k
    finally:
        m.destroy()


def test_host_in_host_out_equals_device(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        rc, on_device = _call(m, "mesh", x, False, 10000)
        assert rc == _lib.MD_OK
        nf = int(on_device["face_count"][2])
        print(f"host test: {nf} faces")
        assert 100 < nf < 10000 and on_device["face_count"][:2].sum() == nf
        for cap in (10000, nf // 2):
            rc, on_host = _call(m, "mesh", x, True, cap)
            assert rc == _lib.MD_OK
            n = min(nf, cap)
            assert np.array_equal(on_host["face_count"][:3], on_device["face_count"][:3])
            assert np.array_equal(on_host["faces"][:n * 3], on_device["faces"][:n * 3])
            assert np.array_equal(on_host["pixel_index"], on_device["pixel_index"])
            assert (on_host["faces"][n * 3:] == -7).all(), cap  # nothing behind the faces that exist travels
            assert (on_host["face_count"][3:] == -7).all() and (on_host["pixel_index"][2 * 70 * 70:] == -7).all()
            rows = int(on_host["count"][2])
            assert np.array_equal(_bits(on_host["xyz"][:rows]), _bits(on_device["xyz"][:rows])) and (on_host["xyz"][rows:] == f32(FILL["xyz"])).all()
        for k, used in (("faces", nf * 3), ("face_count", 3), ("pixel_index", 2 * 70 * 70)):
            assert (on_device[k][used:] == -7).all(), k
    finally:
        m.destroy()


def test_graph_replay_and_allocations(dev):
    from burn_depth_amd import ops
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        _, conf, extr, intr = _da3_subset(m, x)
        kw = dict(world=True, conf_min=1.0, **OPTS)
        plain = m.infer_points(x, **kw)
        want = {r: _mesh_np(ops.unproject(dev, plain.depth, intrinsics=intr, extrinsics=extr, conf=conf, mesh=dict(max_rtol=r), **kw)) for r in (0.1, 0.0)}
        assert 0 < want[0.1]["face_count"][-1] < want[0.0]["face_count"][-1]
        m.enable_graph(True)
        out = m.infer_points(x, mesh=dict(max_rtol=0.1), **kw)  # call 1 of this key (fresh output pointers): eager
        _same_mesh(_mesh_np(out), want[0.1], "eager")
        allocs = m.query("allocs")
        for call in (1, 2, 3, 4):  # capture, then replays
            out.faces.fill_(-7)
            out.face_count.fill_(-7)
            out.pixel_index.fill_(-7)
            out = m.infer_points(x, out=out, mesh=dict(max_rtol=0.1), **kw)
            _same_mesh(_mesh_np(out), want[0.1], f"graph call {call}")
        for _ in range(3):  # another max_rtol on the same pointers: its own graph and its own result
            out = m.infer_points(x, out=out, mesh=dict(max_rtol=0.0), **kw)
        _same_mesh(_mesh_np(out), want[0.0], "max_rtol 0")
        for _ in range(2):
            m.infer_points(x, out=out, mesh=dict(max_rtol=0.1), **kw)
            m.infer_points(x, out=out, mesh=dict(max_rtol=0.0), **kw)
        _same_mesh(_mesh_np(out), want[0.0], "after the loop")
        assert m.query("allocs") == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


def test_refusals_leave_the_outputs_untouched(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        E, S = _lib.MD_ERR_INVALID_ARG, _lib.MD_ERR_SHAPE
        bad = [(dict(max_rtol=float("nan")), E, "max_rtol"), (dict(max_rtol=float("inf")), E, "max_rtol"), (dict(max_rtol=-0.5), E, "max_rtol"),
               (dict(face_capacity=-1), E, "face_capacity"), (dict(face_count=False), E, "face_count"), (dict(thin=0.05), E, "voxel thinning")]
        for host in (False, True):
            for kw, code, word in bad:
                rc, t = _call(m, "mesh", x, host, 100, **kw)
                assert rc == code and word in _lib.load().md_last_error().decode(), (kw, host)
                for k, v in t.items():
                    assert (v == np.asarray(FILL[k], v.dtype)).all(), (kw, host, k)
        # a mesh without the list's count
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, compact=False, world=True, mesh=True)
        assert e.value.code == E and "`count`" in e.value.message
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, world=True, voxel=0.05, mesh=True)
        assert e.value.code == E and "voxel thinning" in e.value.message
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, world=True, mesh=dict(rtol=0.1))
        assert e.value.code == E
    finally:
        m.destroy()


def test_infer_cli_writes_the_faces_into_the_ply(dev, tmp_path):
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
    img = str(tmp_path / "img.npy")
    np.save(img, rgb)
    ply = str(tmp_path / "mesh.ply")
    head = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "2", "--edge-rtol", "0.5"]
    assert cli.main(head + ["--mesh", "--voxel", "0.1"]) == 2 and cli.main(head[:6] + ["--mesh"]) == 2
    assert cli.main(head + ["--mesh", "--mesh-rtol", "0.1"]) == 0
    xyz, col, _, faces = P.read_ply_faces(ply)
    m = DepthAnything3.load_file(dev, cfg, ck)
    try:
        prep = P.prepare_depth_anything3_image(rgb, 518).rgb
        x = rgb_to_input_tensor(prep.tobytes(), 518, 518, dev)
        pc = m.infer_points(x, rgb=_t(prep[None]), dense=False, stride=2, edge_rtol=0.5, world=True, mesh=dict(max_rtol=0.1))
        want_xyz, want_col, _ = pc.points()
        want = pc.faces[:int(pc.face_count[-1])].cpu().numpy()
    finally:
        m.destroy()
    assert len(faces) > 0 and faces.max() < len(xyz) and np.array_equal(faces, want)
    assert np.array_equal(_bits(xyz), _bits(want_xyz.cpu().numpy())) and np.array_equal(col, want_col.cpu().numpy())
