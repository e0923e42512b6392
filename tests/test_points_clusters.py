"""Model -> cloud with its clusters in one call: `infer_points(clusters=...)` (md_infer_points_clusters) against
`ops.cluster_points` (md_op_cluster_points) applied to the list of `infer_points()` of the same call, eager and under graph replay,
behind the plane stage, and the refusals. include/mi_depth.h states the contract, DESIGN 12.12 the kernels. Runs with `-m gpu` on
an MI355X."""
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
from points_util import _da3, _image, _pro, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
LIST = ("xyz", "conf", "rgb", "normals")
DENSE = ("point_map", "mask", "normal_map", "depth")
FOUND = ("stats", "dropped")
ROWS = ("label", "cluster_size", "cluster")
TABLE = ("table_label", "table_size", "box")


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(v) for k, v in vars(pc).items() if k not in ("render", "raster", "smooth", "planes", "clusters")}
    if pc.clusters is not None:
        d.update({k: g(getattr(pc.clusters, k)) for k in FOUND + ROWS + TABLE})
    return d


def _cut(full, k):
    n = int(full["count"][-1])
    return torch.from_numpy(full[k][:n]).cuda() if full[k] is not None else None


def _radius_for(full, frac=0.03):
    n = int(full["count"][-1])
    return float(np.float32(frac * np.ptp(full["xyz"][:n], axis=0).max()))


def _expect(dev, full, clu):
    """ops.cluster_points on the list `full` (a dict of numpy rows with `count`), with the per-view counts from its index"""
    from burn_depth_amd import ops
    kw = {k: v for k, v in clu.items() if k != "table"}
    want = ops.cluster_points(dev, _cut(full, "xyz"), conf=_cut(full, "conf"), rgb=_cut(full, "rgb"), normals=_cut(full, "normals"),
                              table=clu.get("table", 256), **kw)
    w = _np(want)
    if w["count"] is not None:
        m = int(w["count"][-1])
        bounds = np.concatenate([[0], np.cumsum(full["count"][:-1])])
        w["count"] = np.concatenate([np.diff(np.searchsorted(w["index"][:m], bounds)), [m]]).astype(np.int32)
    return w


def _same(want, got, full, what=""):
    """got: the model call's outputs, poisoned before the call; full: the list the stage read"""
    n = int(full["count"][-1])
    for k in FOUND:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ROWS:
        assert np.array_equal(got[k][:n], want[k][:n]), (what, k)
        assert (got[k][n:] == -7).all() and len(got[k]) > n, (what, k)  # rows at and beyond the device count are not rows
    t = min(int(want["stats"][1]), got["table_label"].shape[0])
    for k in TABLE:
        assert np.array_equal(got[k][:t].view(np.uint8), want[k][:t].view(np.uint8)), (what, k)
        assert (got[k][t:].view(np.int32) == (-7 if k != "box" else np.float32(POISON).view(np.int32))).all(), (what, k)
    if want["count"] is None:  # mode 0: the list is the one the stage read
        assert np.array_equal(got["count"], full["count"]), what
        for k in LIST:
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
    for t in (out.xyz, out.normals, out.conf, out.clusters.box):
        if t is not None:
            t.fill_(POISON)
    c = out.clusters
    for t in (out.index, out.count, c.label, c.cluster_size, c.cluster, c.table_label, c.table_size, c.stats, c.dropped):
        if t is not None:
            t.fill_(-7)
    if out.planes is not None:
        out.planes.label.fill_(-7)


def _poisoned(m, x, **kw):
    out = m.infer_points(x, **kw)
    _poison(out)
    return m.infer_points(x, out=out, **kw)


def test_da3_three_views_clusters_equal_clustering_the_list_of_the_call(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, normals=True, **OPTS)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 500
        r = _radius_for(full)
        for mode in ("label", "keep"):
            for k in (0, 4):
                clu = dict(radius=r, min_neighbours=k, min_points=5, mode=mode, table=64)
                want = _expect(dev, full, clu)
                assert want["stats"][1] >= 1 and want["stats"][3] < n
                _same(want, _np(_poisoned(m, x, clusters=clu, **kw)), full, (mode, k))
        # graph replay on the same pointers: the state is reset inside the graph; nothing is allocated after the first call
        clu = dict(radius=r, min_neighbours=4, min_points=5, mode="keep", table=64)
        want = _expect(dev, full, clu)
        m.enable_graph(True)
        out = m.infer_points(x, clusters=clu, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            _poison(out)
            out = m.infer_points(x, out=out, clusters=clu, **kw)
            _same(want, _np(out), full, f"graph call {call}")
        other = dict(clu, min_neighbours=2)  # other options on the same pointers: their own graph and their own result
        for _ in range(3):
            _poison(out)
            out = m.infer_points(x, out=out, clusters=other, **kw)
        _same(_expect(dev, full, other), _np(out), full, "other k")
        assert m.query("allocs") == allocs
        m.enable_graph(False)
        # behind the plane stage with mode "drop": the two operators composed
        pln = dict(planes=2, hypotheses=65, tol=r / 2, min_inliers=20, seed=5, mode="drop")
        pre = _np(m.infer_points(x, planes=pln, **kw))
        assert 0 < int(pre["count"][-1]) < n
        for mode in ("label", "keep"):
            clu = dict(radius=r, min_neighbours=3, min_points=4, mode=mode, table=64)
            got = _np(_poisoned(m, x, planes=pln, clusters=clu, **kw))
            _same(_expect(dev, pre, clu), got, pre, f"behind planes {mode}")
    finally:
        m.enable_graph(False)
        m.destroy()


def test_depth_pro_clusters_and_the_call_without_the_stage(dev):
    m = _pro(dev, "small")
    try:
        x = _image(2, 512).cuda()
        kw = dict(normals=True, **OPTS)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 1000 and full["conf"] is None
        clu = dict(radius=_radius_for(full, 0.01), min_neighbours=6, min_points=10, mode="keep", table=32)
        want = _expect(dev, full, clu)
        cnt = int(want["count"][-1])
        assert 0 < cnt < n
        _same(want, _np(_poisoned(m, x, clusters=clu, **kw)), full, "depth pro")
        m.enable_graph(True)
        out = m.infer_points(x, clusters=clu, **kw)
        for call in (1, 2):
            _poison(out)
            out = m.infer_points(x, out=out, clusters=clu, **kw)
            _same(want, _np(out), full, f"graph call {call}")
        m.enable_graph(False)
        # clusters=None and radius 0 are the call without the stage, bit for bit, with the same launches
        m.enable_timing(True)
        m.read_timing()  # empties the launch order
        m.infer_points(x, mesh=True, **kw)
        order = m.read_launch_order()
        for off in (None, dict(radius=0.0)):
            m.read_timing()
            got = m.infer_points(x, mesh=True, clusters=off, **kw)
            assert got.clusters is None and m.read_launch_order() == order and "points_clusters" not in order
            got = _np(got)
            for k in LIST + DENSE + ("count",):
                rows = n if k in LIST else None
                assert (got[k] is None) == (full[k] is None) and (got[k] is None or np.array_equal(got[k][:rows].view(np.uint8), full[k][:rows].view(np.uint8))), k
        m.read_timing()
        m.infer_points(x, planes=dict(planes=1, hypotheses=8, tol=0.1), clusters=dict(clu, mode="label"), **kw)
        assert m.read_launch_order() == [n for n in order if n != "points_mesh"] + ["points_planes", "points_clusters"]
        m.enable_timing(False)
    finally:
        m.enable_graph(False)
        m.destroy()


def test_refusals_narrower_entries_and_host_outputs(dev):
    from burn_depth_amd import points
    from burn_depth_amd.depth_pro import _stream_ptr
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev, max_batch=2)
    try:
        x = _image(2, 70)
        xd = x.cuda()
        kw = dict(world=True, **OPTS)
        ok = dict(radius=0.1, min_neighbours=2, min_points=2)
        m.enable_timing(True)
        m.infer_points(xd, clusters=ok, **kw)
        order = m.read_launch_order()
        pln = dict(planes=1, hypotheses=8, tol=0.1)
        bad = [dict(clusters=dict(ok, radius=-1.0)), dict(clusters=dict(ok, radius=float("inf"))), dict(clusters=dict(ok, min_neighbours=-1)),
               dict(clusters=dict(ok, min_neighbours=(1 << 20) + 1)), dict(clusters=dict(ok, min_points=0)), dict(clusters=dict(ok, max_points=-1)),
               dict(clusters=dict(ok, max_points=1)), dict(clusters=dict(ok, mode=2)), dict(clusters=dict(ok, table=-1)),
               dict(clusters=dict(ok, mode="keep"), mesh=True), dict(clusters=dict(ok, mode="keep"), mesh=True, components=dict(min_faces=2)),
               dict(clusters=dict(ok, mode="keep"), mesh=True, decimate=dict(voxel=0.1)),
               dict(clusters=dict(ok, mode="keep"), mesh=True, smooth=dict(step=1e-3, iterations=1, lam=0.5)),
               dict(clusters=dict(ok, mode="keep"), planes=pln),  # the rows the plane labels are parallel to would not be returned
               dict(clusters=ok, mesh=True, decimate=dict(voxel=0.1))]
        for b in bad:
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(xd, **kw, **b)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, b
        assert m.read_launch_order() == order  # nothing was enqueued by a refused call
        m.enable_timing(False)
        assert m.query("clusters_overflow") == 0  # the probe-loop flag of the last launched call, for device outputs
        # the library's own refusals of a struct the builder cannot form, and the narrower entry against the widest with a null part
        rq_out = m.infer_points(xd, clusters=ok, **kw)
        rq = points._points_request(torch.device("cuda", 0), 2, 70, 70, want_rgb=False, want_conf=True, want_depth=True, out=rq_out, clusters=ok,
                                    opts=dict(kw))

        def call(entry, parts):
            return entry(m._h, C.c_void_p(xd.data_ptr()), 2, 70, 70, _lib.MD_MEM_DEVICE, None, *parts, _lib.MD_MEM_DEVICE, _stream_ptr(0))
        assert call(m._lib.md_infer_points_clusters, rq.clusters_args()) == _lib.MD_OK
        with_stage = _np(rq_out)
        _poison(rq_out)
        assert call(m._lib.md_infer_points_clusters, rq.planes_args() + [None]) == _lib.MD_OK
        widest = _np(rq_out)
        _poison(rq_out)
        assert call(m._lib.md_infer_points_planes, rq.planes_args()) == _lib.MD_OK
        narrower = _np(rq_out)
        n = int(widest["count"][-1])
        assert (widest["label"] == -7).all() and not (with_stage["label"][:n] == -7).any()  # a null part: the stage does not run
        for k in ("xyz", "conf", "count", "point_map", "mask", "depth"):
            rows = n if k in LIST else None
            assert np.array_equal(widest[k][:rows].view(np.uint8), narrower[k][:rows].view(np.uint8)), k
            assert np.array_equal(widest[k][:rows].view(np.uint8), with_stage[k][:rows].view(np.uint8)), k
        rq.clu.radius = 0.0
        assert call(m._lib.md_infer_points_clusters, rq.clusters_args()) == _lib.MD_ERR_INVALID_ARG  # its pointers are still set
        rq.clu.radius = 0.1
        rq.outs.count = None
        assert call(m._lib.md_infer_points_clusters, rq.clusters_args()) == _lib.MD_ERR_INVALID_ARG
        # everything in host memory against the device-memory call, modes 0 and 1
        B, S, T = 2, 70, 16
        cap = B * 35 * 35
        o = _points_opts(world=True, **OPTS)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f, i32 = np.float32, np.int32
        shapes = dict(xyz=((cap, 3), f, POISON), conf=((cap,), f, POISON), count=((B + 1,), i32, -7), label=((cap,), i32, -7),
                      cluster_size=((cap,), i32, -7), cluster=((cap,), i32, -7), table_label=((T,), i32, -7), table_size=((T,), i32, -7),
                      box=((T, 6), f, POISON), stats=((4,), i32, -7), index=((cap,), i32, -7), dropped=((1,), i32, -7))

        def run(host, mode, radius):
            t = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, ptr("xyz"), None, ptr("conf"), ptr("count"), cap, None)
            clu = _lib.MdPointsClusters(radius, 3, 3, 0, mode, ptr("label"), ptr("cluster_size"), ptr("cluster"), ptr("table_label"),
                                        ptr("table_size"), ptr("box"), T, ptr("stats"), ptr("index") if mode else None, ptr("dropped"))
            kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
            px = x.numpy().ctypes.data if host else xd.data_ptr()
            _lib.check(lib.md_infer_points_clusters(m._h, C.c_void_p(px), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None, None,
                                                    None, None, None, None, None, None, None, None, C.byref(clu), kind, None if host else st))
            torch.cuda.synchronize()
            return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        first = run(False, 0, 1.0)
        n = int(first["count"][-1])
        assert 0 < n < cap
        radius = float(np.float32(0.03 * np.ptp(first["xyz"][:n], axis=0).max()))
        for mode in (0, 1):
            on_device, on_host = run(False, mode, radius), run(True, mode, radius)
            cnt, kept = int(on_device["count"][-1]), min(int(on_device["stats"][1]), T)
            assert kept >= 1 and (0 < cnt < n if mode else cnt == n)
            for k in on_device:
                rows = cnt if k in ("xyz", "conf", "index") else n if k in ROWS else kept if k in TABLE else None
                assert np.array_equal(on_device[k][:rows].view(np.uint8), on_host[k][:rows].view(np.uint8)), (mode, k)
            for t in (on_device, on_host):
                assert (t["label"][n:] == -7).all() and (t["label"][:n] >= -1).all(), mode
                assert (t["table_label"][kept:] == -7).all() and (t["box"][kept:] == np.float32(POISON)).all(), mode
                assert (t["index"][cnt if mode else 0:] == -7).all() and (t["xyz"][cnt:] == np.float32(POISON)).all(), mode
    finally:
        m.destroy()


def test_infer_cli_prints_the_clusters_and_writes_the_ids(dev, tmp_path, capsys):
    """tools/infer.py --ply --cluster-radius R: one image through the stage of the model call, --views and --mesh through
    ops.cluster_points on the points of the file, and behind --planes; label writes the PLY property, keep the points of kept clusters"""
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
    assert cli.main(one + ["--cluster-radius", "-1"]) == 2 and cli.main(one + ["--mesh", "--cluster-radius", "1", "--cluster-mode", "keep"]) == 2
    assert cli.main(one + planes + ["--cluster-radius", "1", "--cluster-mode", "keep"]) == 2  # behind --plane-mode label
    assert cli.main(one[:-6] + one[-4:] + ["--cluster-radius", "1"]) == 2  # without --ply

    def clustered(xyz0, radius):
        want = ops.cluster_points(dev, torch.from_numpy(xyz0).cuda(), radius=radius, min_neighbours=3, min_points=5, table=256)
        torch.cuda.synchronize()
        return want.clusters

    def said(kept, sizes):
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Cluster ")]
        assert len(lines) == min(kept, 256) and all(l.startswith(f"Cluster {i}: {int(c)} points") for i, (l, c) in enumerate(zip(lines, sizes))), lines

    for head, extra in ((one, []), (views, []), (one, ["--mesh"])):
        assert cli.main(head + extra) == 0
        xyz0, col0 = P.read_ply(ply)
        fin = xyz0[np.isfinite(xyz0).all(1)]
        radius = float(np.float32(0.03 * np.ptp(fin, axis=0).max()))
        opts = ["--cluster-radius", repr(radius), "--cluster-min-neighbours", "3", "--cluster-min-points", "5"]
        want = clustered(xyz0, radius)
        kept, ids = int(want.stats[1]), want.cluster.cpu().numpy()
        assert kept >= 1 and (ids == -1).any()
        capsys.readouterr()
        assert cli.main(head + extra + opts) == 0
        said(kept, want.table_size.cpu())
        xyz1, _ = P.read_ply(ply)
        assert np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(P.read_ply_label(ply), ids)
        if extra:
            continue
        assert cli.main(head + opts + ["--cluster-mode", "keep"]) == 0
        xyz2, col2 = P.read_ply(ply)
        assert np.array_equal(xyz2.view(np.uint32), xyz0[ids >= 0].view(np.uint32)) and np.array_equal(col2, col0[ids >= 0])
        assert P.read_ply_label(ply) is None
        # behind --planes with --plane-mode drop: the clusters of what is not on a plane
        assert cli.main(head + planes + ["--plane-mode", "drop"]) == 0
        xyz3, _ = P.read_ply(ply)
        assert 0 < len(xyz3) < len(xyz0)
        want = clustered(xyz3, radius)
        capsys.readouterr()
        assert cli.main(head + planes + ["--plane-mode", "drop"] + opts) == 0
        said(int(want.stats[1]), want.table_size.cpu())
        xyz4, _ = P.read_ply(ply)
        assert np.array_equal(xyz4.view(np.uint32), xyz3.view(np.uint32)) and np.array_equal(P.read_ply_label(ply), want.cluster.cpu().numpy())
