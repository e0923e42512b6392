"""Model -> cloud with its planes in one call: `infer_points(planes=...)` (md_infer_points_planes) against `ops.fit_planes`
(md_op_fit_planes) applied to the list of `infer_points()` of the same call, eager and under graph replay, and the refusals.
include/mi_depth.h states the contract, DESIGN 12.11 the kernels. Runs with `-m gpu` on an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from burn_depth_amd import _lib  # noqa: E402
from points_util import _da3, _image, _pro, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
NRM = dict(normals=True, normal_min_cos=0.05)
LIST = ("xyz", "conf", "rgb", "normals")
DENSE = ("point_map", "mask", "normal_map", "depth")
FITTED = ("plane", "plane_count", "hypothesis", "dropped")


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(v) for k, v in vars(pc).items() if k not in ("render", "raster", "smooth", "planes")}
    if pc.planes is not None:
        d.update({k: g(getattr(pc.planes, k)) for k in FITTED + ("label",)})
    return d


def _cut(full, k):
    n = int(full["count"][-1])
    return torch.from_numpy(full[k][:n]).cuda() if full[k] is not None else None


def _tol_for(full):
    n = int(full["count"][-1])
    return float(np.float32(0.02 * np.ptp(full["xyz"][:n], axis=0).max()))


def _expect(dev, full, pln):
    """ops.fit_planes on the list of the call without the stage, with the per-view counts from its index"""
    from burn_depth_amd import ops
    want = ops.fit_planes(dev, _cut(full, "xyz"), conf=_cut(full, "conf"), rgb=_cut(full, "rgb"), normals=_cut(full, "normals"), **pln)
    w = _np(want)
    if w["count"] is not None:
        m = int(w["count"][-1])
        bounds = np.concatenate([[0], np.cumsum(full["count"][:-1])])
        w["count"] = np.concatenate([np.diff(np.searchsorted(w["index"][:m], bounds)), [m]]).astype(np.int32)
    return w


def _same(want, got, full, what="", poisoned=True):
    n = int(full["count"][-1])
    for k in FITTED:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (what, k, got[k], want[k])
    assert np.array_equal(got["label"][:n], want["label"][:n]), what
    if poisoned:  # rows at and beyond the device count of the list are not rows: nothing is written there
        assert (got["label"][n:] == -7).all() and len(got["label"]) > n, what
    for k in DENSE:  # the dense outputs are those of the call without the stage
        if full[k] is not None:
            assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), (what, k)
    if want["count"] is None:  # mode 0: the list is the call's own
        assert np.array_equal(got["count"], full["count"]), what
        for k in LIST + ("index",):  # index: an earlier stage's, as in the call without the plane stage
            if full[k] is not None:
                assert np.array_equal(got[k][:n].view(np.uint8), full[k][:n].view(np.uint8)), (what, k)
        return
    m = int(want["count"][-1])
    assert np.array_equal(got["count"], want["count"]), (what, got["count"], want["count"])
    w = min(m, got["xyz"].shape[0])
    for k in LIST + ("index",):
        assert (want[k] is None) == (got[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(got[k][:w].view(np.uint8), want[k][:w].view(np.uint8)), (what, k)
    assert (got["xyz"][m:] == np.float32(POISON)).all(), what  # nothing behind the survivors is written


def _poison(out):
    for t in (out.xyz, out.normals, out.conf, out.planes.plane):
        if t is not None:
            t.fill_(POISON)
    for t in (out.index, out.count, out.planes.plane_count, out.planes.hypothesis, out.planes.label, out.planes.dropped):
        if t is not None:
            t.fill_(-7)


def _poisoned(m, x, **kw):
    out = m.infer_points(x, **kw)
    _poison(out)
    return m.infer_points(x, out=out, **kw)


def test_da3_three_views_planes_equal_fitting_the_list_of_the_call(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 500
        tol = _tol_for(full)
        for mode in ("label", "drop", "keep"):
            pln = dict(planes=3, hypotheses=65, tol=tol, min_inliers=20, seed=5, mode=mode)
            want = _expect(dev, full, pln)
            assert want["plane_count"][3] >= 1
            _same(want, _np(_poisoned(m, x, planes=pln, **kw)), full, mode)
        # the normals predicate reads the list normals; the axis constraint the caller's axis
        pln = dict(planes=2, hypotheses=64, tol=2 * tol, min_inliers=10, seed=6, normal_min_cos=0.3, axis=(0.0, 0.3, 1.0), axis_min_cos=0.2)
        _same(_expect(dev, full, pln), _np(_poisoned(m, x, planes=pln, **kw)), full, "predicates")
        # graph replay on the same pointers: the state is reset inside the graph; nothing is allocated after the first call
        pln = dict(planes=3, hypotheses=65, tol=tol, min_inliers=20, seed=5, mode="drop")
        want = _expect(dev, full, pln)
        m.enable_graph(True)
        out = m.infer_points(x, planes=pln, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            _poison(out)
            out = m.infer_points(x, out=out, planes=pln, **kw)
            _same(want, _np(out), full, f"graph call {call}")
        other = dict(pln, seed=7)  # another seed on the same pointers: its own graph and its own result
        for _ in range(3):
            _poison(out)
            out = m.infer_points(x, out=out, planes=other, **kw)
        _same(_expect(dev, full, other), _np(out), full, "other seed")
        assert m.query("allocs") == allocs
        m.enable_graph(False)
        # behind outlier removal and thinning: the stage reads the list those leave
        chain = dict(outlier=dict(radius=4 * tol, min_neighbours=2), voxel=tol)
        pre = _np(m.infer_points(x, **kw, **chain))
        for mode in ("label", "keep"):
            pln = dict(planes=2, hypotheses=64, tol=tol, min_inliers=10, seed=8, mode=mode)
            got = _np(_poisoned(m, x, planes=pln, **kw, **chain))
            _same(_expect(dev, pre, pln), got, pre, f"chain {mode}")
    finally:
        m.enable_graph(False)
        m.destroy()


def test_depth_pro_planes_capacity_and_the_call_without_the_stage(dev):
    m = _pro(dev, "small")
    try:
        x = _image(2, 512).cuda()
        kw = dict(**OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 1000 and full["conf"] is None
        tol = _tol_for(full)
        pln = dict(planes=8, hypotheses=257, tol=tol, min_inliers=50, seed=1, mode="keep")
        want = _expect(dev, full, pln)
        cnt = int(want["count"][-1])
        assert 0 < cnt < n
        _same(want, _np(_poisoned(m, x, planes=pln, **kw)), full, "depth pro")
        # a capacity below the survivors: the true count, the first rows only
        cap = cnt // 2
        got = _np(m.infer_points(x, planes=pln, capacity=cap, **kw))
        assert np.array_equal(got["count"], want["count"]) and got["xyz"].shape[0] == cap
        for k in ("xyz", "normals", "index"):
            assert np.array_equal(got[k].view(np.uint8), want[k][:cap].view(np.uint8)), k
        assert np.array_equal(got["label"][:n], want["label"][:n])
        # under graph replay
        m.enable_graph(True)
        out = m.infer_points(x, planes=pln, **kw)
        for call in (1, 2):
            _poison(out)
            out = m.infer_points(x, out=out, planes=pln, **kw)
            _same(want, _np(out), full, f"graph call {call}")
        m.enable_graph(False)
        # planes=None and planes=0 are the call without the stage, bit for bit, with the same launches
        m.enable_timing(True)
        m.read_timing()  # empties the launch order
        m.infer_points(x, mesh=True, **kw)
        order = m.read_launch_order()
        for off in (None, dict(planes=0, tol=1.0)):
            m.read_timing()
            got = m.infer_points(x, mesh=True, planes=off, **kw)
            assert got.planes is None and m.read_launch_order() == order and "points_planes" not in order
            got = _np(got)
            for k in LIST + DENSE + ("count",):  # the list below its count: the rows behind it are never written
                rows = n if k in LIST else None
                assert (got[k] is None) == (full[k] is None) and (got[k] is None or np.array_equal(got[k][:rows].view(np.uint8), full[k][:rows].view(np.uint8))), k
        m.read_timing()
        m.infer_points(x, planes=dict(pln, mode="label"), **kw)
        assert m.read_launch_order() == [n for n in order if n != "points_mesh"] + ["points_planes"]
        m.enable_timing(False)
    finally:
        m.enable_graph(False)
        m.destroy()


def test_refusals_come_before_any_launch(dev):
    m = _da3(dev, max_batch=2)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, **OPTS)
        ok = dict(planes=2, hypotheses=16, tol=0.1, min_inliers=5)
        m.enable_timing(True)
        m.infer_points(x, planes=ok, **kw)
        order = m.read_launch_order()
        smooth = dict(step=1e-3, iterations=1, lam=0.5)
        bad = [dict(planes=dict(ok, planes=9)), dict(planes=dict(ok, hypotheses=0)), dict(planes=dict(ok, hypotheses=4097)),
               dict(planes=dict(ok, tol=0.0)), dict(planes=dict(ok, tol=float("inf"))), dict(planes=dict(ok, min_inliers=2)),
               dict(planes=dict(ok, normal_min_cos=1.5)), dict(planes=dict(ok, axis_min_cos=-0.5)), dict(planes=dict(ok, mode=3)),
               dict(planes=dict(ok, normal_min_cos=0.5)),  # no list normals
               dict(planes=dict(ok, axis_min_cos=0.5, axis=(float("nan"), 0, 1))),
               dict(planes=dict(ok, mode="drop"), mesh=True), dict(planes=dict(ok, mode="keep"), mesh=True, components=dict(min_faces=2)),
               dict(planes=dict(ok, mode="keep"), mesh=True, decimate=dict(voxel=0.1)), dict(planes=dict(ok, mode="drop"), mesh=True, smooth=smooth),
               dict(planes=ok, mesh=True, decimate=dict(voxel=0.1))]
        for b in bad:
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, **kw, **b)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, b
        assert m.read_launch_order() == order  # nothing was enqueued by a refused call
        # the library's own refusals of a struct the builder cannot form: pointers with planes == 0, a list output without count
        rq_out = m.infer_points(x, planes=ok, **kw)
        from burn_depth_amd import points
        rq = points._points_request(torch.device("cuda", 0), 2, 70, 70, want_rgb=False, want_conf=True, want_depth=True, out=rq_out, planes=ok,
                                    opts=dict(kw))
        import ctypes as C
        from burn_depth_amd.depth_pro import _stream_ptr

        def call(req):
            return m._lib.md_infer_points_planes(m._h, C.c_void_p(x.data_ptr()), 2, 70, 70, _lib.MD_MEM_DEVICE, None, *req.planes_args(),
                                                 _lib.MD_MEM_DEVICE, _stream_ptr(0))
        assert call(rq) == _lib.MD_OK
        rq.pln.planes = 0
        assert call(rq) == _lib.MD_ERR_INVALID_ARG  # its pointers are still set
        rq.pln.planes = 2
        rq.outs.count = None
        assert call(rq) == _lib.MD_ERR_INVALID_ARG
    finally:
        m.destroy()


def test_host_outputs_match_the_device_call(dev):
    """md_infer_points_planes with everything in host memory against the device-memory call, modes 0 and 2: every output of the
    stage travels through its slot, label with the live count of the list it is parallel to, and nothing behind the rows is written"""
    import ctypes as C
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S, Pn = 2, 70, 3
        cap = B * 35 * 35
        x = _image(B, S)
        xd = x.cuda()
        o = _points_opts(world=True, **OPTS)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f, i32 = np.float32, np.int32
        shapes = dict(xyz=((cap, 3), f, POISON), conf=((cap,), f, POISON), count=((B + 1,), i32, -7), plane=((Pn, 4), f, POISON),
                      plane_count=((Pn + 1,), i32, -7), hypothesis=((Pn,), i32, -7), label=((cap,), i32, -7), index=((cap,), i32, -7),
                      dropped=((1,), i32, -7))

        def call(host, mode, tol):
            t = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, ptr("xyz"), None, ptr("conf"), ptr("count"), cap, None)
            pln = _lib.MdPointsPlanes(Pn, 65, tol, 10, 3, 0.0, (C.c_float * 3)(0, 0, 0), 0.0, mode, ptr("plane"), ptr("plane_count"),
                                      ptr("hypothesis"), ptr("label"), ptr("index") if mode else None, ptr("dropped"))
            kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
            px = x.numpy().ctypes.data if host else xd.data_ptr()
            _lib.check(lib.md_infer_points_planes(m._h, C.c_void_p(px), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None, None,
                                                  None, None, None, None, None, None, None, C.byref(pln), kind, None if host else st))
            torch.cuda.synchronize()
            return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        first = call(False, 0, 1.0)
        n = int(first["count"][-1])
        assert 0 < n < cap
        tol = float(np.float32(0.02 * np.ptp(first["xyz"][:n], axis=0).max()))
        for mode in (0, 2):
            on_device, on_host = call(False, mode, tol), call(True, mode, tol)
            cnt = int(on_device["count"][-1])
            assert on_device["plane_count"][Pn] >= 1 and (0 < cnt < n if mode else cnt == n)
            for k in on_device:
                rows = cnt if k in ("xyz", "conf", "index") else n if k == "label" else None
                assert np.array_equal(on_device[k][:rows].view(np.uint8), on_host[k][:rows].view(np.uint8)), (mode, k)
            for t in (on_device, on_host):
                assert (t["label"][n:] == -7).all() and (t["label"][:n] >= -1).all(), mode  # over the rows of the list in front of the stage
                assert (t["index"][cnt if mode else 0:] == -7).all() and (t["xyz"][cnt:] == np.float32(POISON)).all(), mode
    finally:
        m.destroy()


def test_infer_cli_prints_the_planes_and_writes_the_labels(dev, tmp_path, capsys):
    """tools/infer.py --ply --planes P: one image through the stage of the model call, --views and --mesh through ops.fit_planes on
    the points of the file; label writes the PLY property, drop / keep the cloud without / of the plane points"""
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
    ply = str(tmp_path / "cloud.ply")
    one = ["--model", "depth-anything-3", "--checkpoint", ck, "--image", img, "--ply", ply, "--stride", "4", "--edge-rtol", "0.5"]
    views = ["--model", "depth-anything-3", "--checkpoint", ck, "--views", img, flip, "--ply", ply, "--stride", "4", "--output", str(tmp_path / "d.png")]
    planes = ["--planes", "2", "--plane-hypotheses", "65", "--plane-min-inliers", "10", "--plane-seed", "4"]
    assert cli.main(one + ["--planes", "9"]) == 2 and cli.main(one + ["--mesh"] + planes + ["--plane-mode", "drop"]) == 2
    assert cli.main(one[:-6] + one[-4:] + planes) == 2  # without --ply
    for head, extra in ((one, []), (views, []), (one, ["--mesh"])):
        assert cli.main(head + extra) == 0
        xyz0, col0 = P.read_ply(ply)
        assert P.read_ply_label(ply) is None
        fin = xyz0[np.isfinite(xyz0).all(1)]
        tol = 0.01 * float(torch.from_numpy(np.ptp(fin, axis=0)).max())  # the tool's default: 1 % of the extent, computed on the device list
        want = ops.fit_planes(dev, torch.from_numpy(xyz0).cuda(), planes=2, hypotheses=65, tol=tol, min_inliers=10, seed=4)
        torch.cuda.synchronize()
        found = int(want.planes.plane_count[-1])
        assert found >= 1
        capsys.readouterr()
        assert cli.main(head + extra + planes) == 0
        said = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Plane ")]
        assert len(said) == found and all(f"({int(c)} inliers)" in l for l, c in zip(said, want.planes.plane_count[:found].cpu()))
        xyz1, _ = P.read_ply(ply)
        label = want.planes.label.cpu().numpy()
        assert np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(P.read_ply_label(ply), label)
        if extra:
            continue
        for mode, keep in (("drop", label == -1), ("keep", label >= 0)):
            assert cli.main(head + planes + ["--plane-mode", mode]) == 0
            xyz2, col2 = P.read_ply(ply)
            assert np.array_equal(xyz2.view(np.uint32), xyz0[keep].view(np.uint32)) and np.array_equal(col2, col0[keep]), mode
            assert P.read_ply_label(ply) is None
