"""Model -> cloud without its outliers in one call: `infer_points(outlier=...)` (md_infer_points_outlier) against
`ops.radius_outliers` (md_op_radius_outliers) applied to the unfiltered `infer_points()` of the same call, alone, in front of the
voxel thinning and in front of the point render. include/mi_depth.h states the contract, DESIGN 12.7 the kernels. Runs with
`-m gpu` on an MI355X."""
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
from points_util import _cameras, _da3, _image, _pro, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
NRM = dict(normals=True, normal_min_cos=0.05)
K = 4


def _np(pc):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(pc).items() if k not in ("render", "raster")}


def _radius_for(xyz, share, k=K):
    """a radius that leaves about `share` of the points at k neighbours: bisection on the host reference"""
    span = float(np.ptp(xyz, axis=0).max())
    lo, hi = span * 1e-4, span
    for _ in range(16):
        mid = (lo * hi) ** 0.5
        if P.radius_outliers(xyz, mid, k).count[-1] < share * len(xyz):
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def _cut(full, k):
    n = int(full["count"][-1])
    return torch.from_numpy(full[k][:n]).cuda() if full[k] is not None else None


def _expect(dev, full, radius, k=K):
    """ops.radius_outliers on the unfiltered cloud of the same call, with the per-view counts from its index"""
    from burn_depth_amd import ops
    want = _np(ops.radius_outliers(dev, _cut(full, "xyz"), radius, k, conf=_cut(full, "conf"), rgb=_cut(full, "rgb"), normals=_cut(full, "normals")))
    m = int(want["count"][-1])
    bounds = np.concatenate([[0], np.cumsum(full["count"][:-1])])
    want["count"] = np.concatenate([np.diff(np.searchsorted(want["index"][:m], bounds)), [m]]).astype(np.int32)
    return want, m


def _same_filtered(want, m, got, full, what="", poisoned=True):
    n = int(full["count"][-1])
    assert np.array_equal(got["count"], want["count"]), (what, got["count"], want["count"])
    assert int(got["dropped"][0]) == int(want["dropped"][0]), what
    assert np.array_equal(got["neighbours"][:n], want["neighbours"][:n]), what  # over the rows of the unfiltered list
    for k in ("xyz", "conf", "rgb", "normals", "index"):
        assert (want[k] is None) == (got[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(got[k][:m].view(np.uint8), want[k][:m].view(np.uint8)), (what, k)
    assert got["weight"] is None
    for k in ("point_map", "mask", "normal_map", "depth"):  # the dense outputs are those of the call without the filter
        if full[k] is not None:
            assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), (what, k)
    if poisoned:
        assert (got["xyz"][m:] == np.float32(POISON)).all(), what  # nothing behind the survivors is written
        assert (got["neighbours"][n:] == -7).all(), what


def _poison(out):
    for t in (out.xyz, out.normals, out.conf):
        if t is not None:
            t.fill_(POISON)
    for t in (out.index, out.weight, out.count, out.dropped, out.neighbours):
        if t is not None:
            t.fill_(-7)


def _poisoned(m, x, **kw):
    """infer_points into a cloud whose list tensors are poisoned first"""
    out = m.infer_points(x, **kw)
    _poison(out)
    return m.infer_points(x, out=out, **kw)


def test_da3_three_views_filtered_equals_filtering_the_unfiltered_cloud(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 500 and full["conf"] is not None and full["neighbours"] is None and full["index"] is None
        for share in (0.5, 0.9):
            radius = _radius_for(full["xyz"][:n], share)
            want, cnt = _expect(dev, full, radius)
            assert 0.5 * share * n < cnt < n, (share, cnt, n)
            _same_filtered(want, cnt, _np(_poisoned(m, x, outlier=dict(radius=radius, min_neighbours=K), **kw)), full, share)
        # graph replay on the same pointers: the table is reset inside the graph; nothing is allocated after the first call
        outl = dict(radius=radius, min_neighbours=K)
        m.enable_graph(True)
        out = m.infer_points(x, outlier=outl, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            _poison(out)
            out = m.infer_points(x, out=out, outlier=outl, **kw)
            _same_filtered(want, cnt, _np(out), full, f"graph call {call}")
        # another k on the same pointers: its own graph and its own result
        want2, cnt2 = _expect(dev, full, radius, 2 * K)
        assert cnt2 < cnt
        for _ in range(3):
            out = m.infer_points(x, out=out, outlier=dict(radius=radius, min_neighbours=2 * K), **kw)
        _same_filtered(want2, cnt2, _np(out), full, "2 k", poisoned=False)
        assert m.query("allocs") == allocs
        assert m.query("outlier_overflow") == 0
        m.enable_graph(False)
        # a view filter in front and no normals behind: the outlier removal composes with both
        fkw = dict(world=True, conf_percentile=30, **OPTS)
        full = _np(m.infer_points(x, **fkw))
        radius = _radius_for(full["xyz"][:int(full["count"][-1])], 0.5)
        want, cnt = _expect(dev, full, radius)
        assert cnt > 0 and want["normals"] is None
        _same_filtered(want, cnt, _np(_poisoned(m, x, outlier=dict(radius=radius, min_neighbours=K), **fkw)), full, "filtered")
    finally:
        m.enable_graph(False)
        m.destroy()


def test_depth_pro_filtered_equals_filtering_the_unfiltered_cloud(dev):
    m = _pro(dev, "small")
    try:
        x = _image(2, 512).cuda()
        kw = dict(**OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 1000 and full["conf"] is None
        radius = _radius_for(full["xyz"][:n], 0.5)
        want, cnt = _expect(dev, full, radius)
        assert 0 < cnt < n
        outl = dict(radius=radius, min_neighbours=K)
        _same_filtered(want, cnt, _np(_poisoned(m, x, outlier=outl, **kw)), full, "depth pro")
        # a capacity below the survivors: the true count, the first rows only
        cap = cnt // 2
        got = _np(m.infer_points(x, outlier=outl, capacity=cap, **kw))
        assert np.array_equal(got["count"], want["count"]) and got["xyz"].shape[0] == cap
        for k in ("xyz", "normals", "index"):
            assert np.array_equal(got[k].view(np.uint8), want[k][:cap].view(np.uint8)), k
        assert np.array_equal(got["neighbours"][:n], want["neighbours"][:n])
        # under graph replay
        m.enable_graph(True)
        out = m.infer_points(x, outlier=outl, **kw)
        for call in (1, 2):
            _poison(out)
            out = m.infer_points(x, out=out, outlier=outl, **kw)
            _same_filtered(want, cnt, _np(out), full, f"graph call {call}")
    finally:
        m.enable_graph(False)
        m.destroy()


def test_filter_then_thin_and_filter_then_render_compose_from_the_operators(dev):
    from burn_depth_amd import ops
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        radius = _radius_for(full["xyz"][:n], 0.6)
        outl = dict(radius=radius, min_neighbours=K)
        filt = ops.radius_outliers(dev, _cut(full, "xyz"), radius, K, conf=_cut(full, "conf"), rgb=_cut(full, "rgb"), normals=_cut(full, "normals"))
        f = _np(filt)
        want, cnt = _expect(dev, full, radius)
        assert cnt == int(f["count"][-1])
        assert 0 < cnt < n
        # voxel= too: the thinning of the filtered list
        voxel = float(np.float32(2 * radius))
        thin = _np(ops.voxel_thin(dev, filt.xyz[:cnt], voxel, conf=filt.conf[:cnt], rgb=filt.rgb[:cnt], normals=filt.normals[:cnt]))
        t = int(thin["count"][-1])
        assert 0 < t < cnt
        for graph in (False, True):
            m.enable_graph(graph)
            out = m.infer_points(x, outlier=outl, voxel=voxel, **kw)
            for _ in range(3 if graph else 1):
                _poison(out)
                out = m.infer_points(x, out=out, outlier=outl, voxel=voxel, **kw)
            got = _np(out)
            assert int(got["count"][-1]) == t and got["count"][:-1].sum() == t, graph
            for k in ("xyz", "conf", "rgb", "normals", "index", "weight"):  # index names rows of the filtered list
                assert np.array_equal(got[k][:t].view(np.uint8), thin[k][:t].view(np.uint8)), (graph, k)
            assert int(got["dropped"][0]) == int(thin["dropped"][0])
            assert np.array_equal(got["neighbours"][:n], f["neighbours"][:n]), graph
            assert (got["xyz"][t:] == np.float32(POISON)).all()
        m.enable_graph(False)
        assert m.query("outlier_overflow") == 0 and m.query("voxel_overflow") == 0
        # render= too: the image of the filtered list
        pts = full["xyz"][:n].astype(np.float64)  # two cameras that look at the centroid of the cloud from twice its extent away
        c = pts.mean(0)
        d = 2.0 * float(np.linalg.norm(pts - c, axis=1).max()) + 1e-3
        Kt, Et = _cameras(np.random.default_rng(3), 2, 24, 32)
        for j, a in enumerate((-0.3, 0.2)):
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            Et[j, :, :3], Et[j, :, 3] = R, np.array([0, 0, d]) - R @ c
        cams = dict(intrinsics=torch.from_numpy(Kt).cuda(), extrinsics=torch.from_numpy(Et).cuda())
        img = ops.render_points(dev, filt.xyz, 24, 32, rgb=filt.rgb, count=filt.count[-1:], pixel_offset=0.5, radius=1, **cams)
        bare = ops.render_points(dev, _cut(full, "xyz"), 24, 32, rgb=_cut(full, "rgb"), pixel_offset=0.5, radius=1, **cams)
        for graph in (False, True):
            m.enable_graph(graph)
            for _ in range(3 if graph else 1):
                got = m.infer_points(x, outlier=outl, render=dict(H=24, W=32, pixel_offset=0.5, radius=1, **cams), **kw)
            torch.cuda.synchronize()
            for k in ("depth", "index", "rgb", "filled"):
                assert torch.equal(getattr(got.render, k), getattr(img, k)), (graph, k)
            _same_filtered(want, cnt, _np(got), full, ("render", graph), poisoned=False)
        assert img.filled[-1].item() > 0 and not torch.equal(img.depth, bare.depth)  # the removed rows were visible
    finally:
        m.enable_graph(False)
        m.destroy()


def test_null_outlier_and_zero_radius_are_the_call_without_it_and_a_mesh_is_refused(dev):
    m = _da3(dev)
    try:
        x = _image(2, 70).cuda()
        kw = dict(world=True, **OPTS, **NRM)
        m.enable_timing(True)
        names, outs = {}, {}
        for what, extra in (("none", dict()), ("null", dict(outlier=None)), ("zero", dict(outlier=dict(radius=0.0, min_neighbours=3))),
                            ("on", dict(outlier=dict(radius=0.05, min_neighbours=3)))):
            m.read_timing()
            outs[what] = _np(m.infer_points(x, **extra, **kw))
            names[what] = m.read_launch_order()
            m.read_timing()
        m.enable_timing(False)
        assert names["none"] == names["null"] == names["zero"] and "points_unproject" in names["none"] and "points_outlier" not in names["none"]
        order = list(names["on"])
        assert "points_outlier" in order and order.index("points_unproject") < order.index("points_outlier")
        n = int(outs["none"]["count"][-1])
        assert n > 0
        for what in ("null", "zero"):
            assert outs[what]["neighbours"] is None and outs[what]["index"] is None and outs[what]["dropped"] is None
            for k, v in outs["none"].items():
                rows = n if k in ("xyz", "rgb", "conf", "normals") else None
                assert (v is None) == (outs[what][k] is None), (what, k)
                assert v is None or np.array_equal(v[:rows].view(np.uint8), outs[what][k][:rows].view(np.uint8)), (what, k)
        for bad, code in ((dict(radius=0.1, min_neighbours=3, mesh=True), None), (dict(radius=-1.0, min_neighbours=3), None),
                          (dict(radius=float("nan"), min_neighbours=3), None), (dict(radius=0.1, min_neighbours=0), None),
                          (dict(radius=0.1, min_neighbours=(1 << 20) + 1), None)):
            mesh = bad.pop("mesh", None)
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(x, outlier=bad, mesh=mesh, **kw)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, bad
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, outlier=dict(radius=0.1, min_neighbours=3), mesh=True, **kw)
        assert "a mesh together with outlier removal" in str(e.value)
        none = m.infer_points(x, outlier=dict(radius=0.1, min_neighbours=3), compact=False, **OPTS)  # no list: nothing is filtered
        assert none.neighbours is None and none.xyz is None and none.point_map is not None
    finally:
        m.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# the entries themselves, through ctypes: `infer_points` only reaches the widest one
# ---------------------------------------------------------------------------------------------------------------------------------
FILL = dict(point_map=POISON, mask=77, xyz=POISON, rgb=77, conf=POISON, count=-7, depth=POISON, normal_map=POISON, normals=POISON)
LISTS = ("xyz", "rgb", "conf", "normals")


def _buffers(B, H, W, cap, host=False):
    f, u8, i32 = np.float32, np.uint8, np.int32
    shapes = dict(point_map=((B, H, W, 3), f), mask=((B, H, W), u8), xyz=((cap, 3), f), rgb=((cap, 3), u8), conf=((cap,), f), count=((B + 1,), i32),
                  depth=((B, H, W), f), normal_map=((B, H, W, 3), f), normals=((cap, 3), f))
    t = {k: np.full(shape, FILL[k], dt) for k, (shape, dt) in shapes.items()}
    if not host:
        t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
    outs = _lib.MdPointsOutputs(ptr("point_map"), ptr("mask"), ptr("xyz"), ptr("rgb"), ptr("conf"), ptr("count"), cap, ptr("depth"))
    return t, ptr, outs


def _read(t):
    torch.cuda.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}


def test_narrower_entries_are_the_widest_entry_with_a_null_part_and_host_outputs_match(dev):
    """md_infer_points_raster and md_infer_points_voxel against md_infer_points_outlier with outl NULL and with radius 0: the same
    bytes. Then the widest entry with everything in host memory against the device-memory call."""
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S = 2, 70
        cap = B * 35 * 35
        x = _image(B, S)
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        xd, rd = x.cuda(), rgb.cuda()
        o = _points_opts(world=True, **OPTS)
        DEV, st = _lib.MD_MEM_DEVICE, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (m._h, C.c_void_p(xd.data_ptr()), B, S, S, DEV, C.c_void_p(rd.data_ptr()), None, None)
        zero = _lib.MdPointsOutlier(0.0, 0, None, None, None)

        def call(entry, outl=None):
            t, ptr, outs = _buffers(B, S, S, cap)
            nrm = _lib.MdPointsNormals(ptr("normal_map"), ptr("normals"), NRM["normal_min_cos"])
            mid = (C.byref(o), C.byref(outs), C.byref(nrm), None)
            if entry == "voxel":
                rc = lib.md_infer_points_voxel(*head, *mid, DEV, st)
            elif entry == "raster":
                rc = lib.md_infer_points_raster(*head, *mid, None, None, None, DEV, st)
            else:
                rc = lib.md_infer_points_outlier(*head, *mid, None, None, None, C.byref(outl) if outl else None, DEV, st)
            _lib.check(rc)
            return _read(t)

        widest = call("outlier")
        n = min(int(widest["count"][-1]), cap)
        assert n > 0
        for what, other in (("voxel", call("voxel")), ("raster", call("raster")), ("radius 0", call("outlier", zero))):
            for k in widest:
                rows = n if k in LISTS else None
                assert np.array_equal(widest[k][:rows].view(np.uint8), other[k][:rows].view(np.uint8)), (what, k)

        # host in, host out, the filter on: each output is the device-memory call's, and nothing behind the rows is written
        radius = _radius_for(widest["xyz"][:n], 0.5)

        def filtered(host):
            t, ptr, outs = _buffers(B, S, S, cap, host=host)
            extra = dict(neighbours=np.full(cap, -7, np.int32), index=np.full(cap, -7, np.int32), dropped=np.full(1, -7, np.int32))
            if not host:
                extra = {k: torch.from_numpy(v).cuda() for k, v in extra.items()}
            t.update(extra)
            p2 = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            nrm = _lib.MdPointsNormals(ptr("normal_map"), ptr("normals"), NRM["normal_min_cos"])
            outl = _lib.MdPointsOutlier(radius, K, p2("neighbours"), p2("index"), p2("dropped"))
            xin, cin = (x.numpy(), rgb.numpy()) if host else (xd, rd)
            px, pc = (xin.ctypes.data, cin.ctypes.data) if host else (xin.data_ptr(), cin.data_ptr())
            kind = _lib.MD_MEM_HOST if host else DEV
            _lib.check(lib.md_infer_points_outlier(m._h, C.c_void_p(px), B, S, S, kind, C.c_void_p(pc), None, None, C.byref(o), C.byref(outs),
                                                   C.byref(nrm), None, None, None, None, C.byref(outl), kind, None if host else st))
            return _read(t)

        on_device, on_host = filtered(False), filtered(True)
        cnt = int(on_device["count"][-1])
        assert 0.25 * n < cnt < 0.75 * n and np.array_equal(on_device["count"], on_host["count"])
        for k in on_device:
            rows = cnt if k in LISTS + ("index",) else n if k == "neighbours" else None
            assert np.array_equal(on_device[k][:rows].view(np.uint8), on_host[k][:rows].view(np.uint8)), k
        for k in LISTS:
            assert (on_host[k][cnt:] == np.asarray(FILL[k], on_host[k].dtype)).all(), k
        assert (on_host["index"][cnt:] == -7).all() and (on_host["neighbours"][n:] == -7).all() and (on_host["neighbours"][:n] >= 0).all()
    finally:
        m.destroy()
