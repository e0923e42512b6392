"""Model -> thinned cloud in one call: `infer_points(voxel=...)` (md_infer_points_voxel) against `ops.voxel_thin`
(md_op_voxel_thin) applied to the unthinned `infer_points()` of the same call. include/mi_depth.h states the contract,
DESIGN 12.3 the kernels. Runs with `-m gpu` on an MI355X."""
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
from points_util import _da3, _da3_subset, _image, _pro, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
NRM = dict(normals=True, normal_min_cos=0.05)


def _np(pc):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in vars(pc).items()}


def _voxel_for(xyz, share):
    """a voxel size that leaves about `share` of the points: bisection on the host reference"""
    span = float(np.ptp(xyz, axis=0).max())
    lo, hi = span * 1e-6, span
    for _ in range(30):
        mid = (lo * hi) ** 0.5
        if P.voxel_thin(xyz, mid).count[-1] > share * len(xyz):
            lo = mid
        else:
            hi = mid
    return float(np.float32(hi))


def _expect(dev, full, voxel):
    """ops.voxel_thin on the unthinned cloud of the same call, with the per-view counts from its index"""
    from burn_depth_amd import ops
    n = int(full["count"][-1])
    cut = lambda k: torch.from_numpy(full[k][:n]).cuda() if full[k] is not None else None  # noqa: E731
    want = _np(ops.voxel_thin(dev, cut("xyz"), voxel, conf=cut("conf"), rgb=cut("rgb"), normals=cut("normals")))
    m = int(want["count"][-1])
    bounds = np.concatenate([[0], np.cumsum(full["count"][:-1])])
    want["count"] = np.concatenate([np.diff(np.searchsorted(want["index"][:m], bounds)), [m]]).astype(np.int32)
    return want, m


def _same_thinned(want, m, got, full, what="", poisoned=True):
    assert np.array_equal(got["count"], want["count"]), (what, got["count"], want["count"])
    assert int(got["dropped"][0]) == int(want["dropped"][0]), what
    for k in ("xyz", "conf", "rgb", "normals", "index", "weight"):
        assert (want[k] is None) == (got[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(got[k][:m].view(np.uint8), want[k][:m].view(np.uint8)), (what, k)
    for k in ("point_map", "mask", "normal_map", "depth"):  # the dense outputs are those of the call without thinning
        if full[k] is not None:
            assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), (what, k)
    if poisoned:
        assert (got["xyz"][m:] == np.float32(POISON)).all(), what  # nothing behind the survivors is written


def _poisoned(m, x, **kw):
    """infer_points into a cloud whose list tensors are poisoned first"""
    out = m.infer_points(x, **kw)
    for t in (out.xyz, out.normals, out.conf):
        if t is not None:
            t.fill_(POISON)
    for t in (out.index, out.weight, out.count, out.dropped):
        if t is not None:
            t.fill_(-7)
    return m.infer_points(x, out=out, **kw)


def test_da3_three_views_thinned_equals_thinning_the_unthinned_cloud(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        rgb = torch.randint(0, 256, (3, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, **OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 500 and full["conf"] is not None and full["index"] is None
        for share in (0.5, 0.125):
            voxel = _voxel_for(full["xyz"][:n], share)
            want, cnt = _expect(dev, full, voxel)
            assert 0.25 * share * n < cnt < 2 * share * n and (want["count"][:-1] > 0).all(), (share, cnt, n)
            assert want["weight"][:cnt].sum() + int(want["dropped"][0]) == n
            got = _np(_poisoned(m, x, voxel=voxel, **kw))
            _same_thinned(want, cnt, got, full, share)
        # voxel = 0 is the call without it
        zero = _np(m.infer_points(x, voxel=0.0, **kw))
        assert zero["index"] is None and zero["weight"] is None
        for k, v in full.items():
            rows = n if k in ("xyz", "rgb", "conf", "normals") else None  # the list rows behind the points are not written
            assert (v is None) == (zero[k] is None) and (v is None or np.array_equal(v[:rows].view(np.uint8), zero[k][:rows].view(np.uint8))), k
        # a view filter in front and no normals behind: the thinning composes with both
        fkw = dict(world=True, conf_percentile=30, view_rtol=0.5, min_views=1, **OPTS)
        full = _np(m.infer_points(x, **fkw))
        voxel = _voxel_for(full["xyz"][:int(full["count"][-1])], 0.5)
        want, cnt = _expect(dev, full, voxel)
        assert cnt > 0 and want["normals"] is None
        _same_thinned(want, cnt, _np(_poisoned(m, x, voxel=voxel, **fkw)), full, "filtered")
        with pytest.raises(_lib.MdError) as e:
            m.infer_points(x, voxel=-1.0, **kw)
        assert e.value.code == _lib.MD_ERR_INVALID_ARG
        assert m.query("voxel_overflow") == 0
    finally:
        m.destroy()


def test_depth_pro_thinned_equals_thinning_the_unthinned_cloud(dev):
    m = _pro(dev, "small")
    try:
        x = _image(2, 512).cuda()
        kw = dict(**OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 1000 and full["conf"] is None  # no confidence: the first point of every voxel
        voxel = _voxel_for(full["xyz"][:n], 0.25)
        want, cnt = _expect(dev, full, voxel)
        assert 0 < cnt < n
        _same_thinned(want, cnt, _np(_poisoned(m, x, voxel=voxel, **kw)), full, "depth pro")
        # a capacity below the survivors: the true count, the first rows only
        cap = cnt // 2
        got = _np(m.infer_points(x, voxel=voxel, capacity=cap, **kw))
        assert np.array_equal(got["count"], want["count"]) and got["xyz"].shape[0] == cap
        for k in ("xyz", "normals", "index", "weight"):
            assert np.array_equal(got[k].view(np.uint8), want[k][:cap].view(np.uint8)), k
    finally:
        m.destroy()


def test_thinned_graph_replay_and_allocations(dev):
    m = _da3(dev, max_batch=3)
    try:
        x = _image(3, 70).cuda()
        kw = dict(conf_min=1.0, world=True, **OPTS, **NRM)
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        voxel = _voxel_for(full["xyz"][:n], 0.5)
        want, cnt = _expect(dev, full, voxel)
        assert 0 < cnt < n
        m.enable_graph(True)
        out = m.infer_points(x, voxel=voxel, **kw)  # call 1 of this key (fresh output pointers): eager
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay; the table is reset inside the graph
            for t in (out.xyz, out.normals, out.conf):
                t.fill_(POISON)
            for t in (out.index, out.weight, out.count, out.dropped):
                t.fill_(-7)
            out = m.infer_points(x, out=out, voxel=voxel, **kw)
            _same_thinned(want, cnt, _np(out), full, f"graph call {call}")
        # another voxel size on the same pointers: its own graph and its own result
        voxel2 = 2 * voxel
        want2, cnt2 = _expect(dev, full, voxel2)
        assert cnt2 < cnt
        for _ in range(3):
            out = m.infer_points(x, out=out, voxel=voxel2, **kw)
        got = _np(out)
        assert np.array_equal(got["count"], want2["count"]) and np.array_equal(got["index"][:cnt2], want2["index"][:cnt2])
        before = m.query("allocs")
        for _ in range(3):
            m.infer_points(x, out=out, voxel=voxel, **kw)
            m.infer_points(x, out=out, voxel=voxel2, **kw)
        _same_thinned(want2, cnt2, _np(out), full, "after the loop", poisoned=False)
        assert m.query("allocs") == before == allocs
    finally:
        m.enable_graph(False)
        m.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# the entries themselves, through ctypes: `infer_points` and `ops.unproject` only reach the widest ones
# ---------------------------------------------------------------------------------------------------------------------------------
FILL = dict(point_map=POISON, mask=77, xyz=POISON, rgb=77, conf=POISON, count=-7, depth=POISON, normal_map=POISON, normals=POISON, index=-7,
            weight=-7, dropped=-7)
LISTS = ("xyz", "rgb", "conf", "normals", "index", "weight")


def _buffers(B, H, W, cap, host=False, normals=False, thinning=False, depth=True):
    """Poisoned outputs of one call, numpy (host) or device tensors -> (dict, pointer of a name or None, md_points_outputs)"""
    f, u8, i32 = np.float32, np.uint8, np.int32
    shapes = dict(point_map=((B, H, W, 3), f), mask=((B, H, W), u8), xyz=((cap, 3), f), rgb=((cap, 3), u8), conf=((cap,), f), count=((B + 1,), i32))
    if depth:
        shapes.update(depth=((B, H, W), f))
    if normals:
        shapes.update(normal_map=((B, H, W, 3), f), normals=((cap, 3), f))
    if thinning:
        shapes.update(index=((cap,), i32), weight=((cap,), i32), dropped=((1,), i32))
    t = {k: np.full(shape, FILL[k], dt) for k, (shape, dt) in shapes.items()}
    if not host:
        t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    ptr = lambda k: (t[k].ctypes.data if host else t[k].data_ptr()) if k in t else None  # noqa: E731
    outs = _lib.MdPointsOutputs(ptr("point_map"), ptr("mask"), ptr("xyz"), ptr("rgb"), ptr("conf"), ptr("count"), cap, ptr("depth"))
    return t, ptr, outs


def _read(t):
    torch.cuda.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}


def _same_bytes(a, b, what):
    """every output of b is a's, byte for byte; of the list outputs, the rows that hold points -> their number"""
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    n = min(int(a["count"][-1]), a["xyz"].shape[0])
    assert n > 0, what
    for k in a:
        rows = n if k in LISTS else None
        assert np.array_equal(a[k][:rows].view(np.uint8), b[k][:rows].view(np.uint8)), (what, k)
    return n


def test_narrow_entries_are_the_widest_entry_with_nulls(dev):
    """md_infer_points, _filtered and _normals against md_infer_points_voxel, md_op_unproject against md_op_unproject_normals: the
    same request, with NULL and with all-zero structs for the parts the narrower entry lacks, gives the same bytes."""
    from burn_depth_amd.points import _points_opts, _view_filter_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S = 2, 70
        cap = B * 35 * 35
        x = _image(B, S).cuda()
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        o = _points_opts(world=True, **OPTS)
        fo = _view_filter_opts(o.pixel_offset, 0.0, 0.0, 30)  # the percentile alone: two views of seeded weights confirm no pixel of each other
        DEV, st = _lib.MD_MEM_DEVICE, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (m._h, C.c_void_p(x.data_ptr()), B, S, S, DEV, C.c_void_p(rgb.data_ptr()), None)
        ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
        zero_nrm, zero_vox = _lib.MdPointsNormals(None, None, 0.0), _lib.MdPointsVoxel(0.0, None, None, None)

        def call(entry, filt, normals, zero=False):
            t, ptr, outs = _buffers(B, S, S, cap, normals=normals)
            nrm = _lib.MdPointsNormals(ptr("normal_map"), ptr("normals"), NRM["normal_min_cos"]) if normals else None
            f = fo if filt else None
            if entry == "points":
                rc = lib.md_infer_points(*head, C.byref(o), C.byref(outs), DEV, st)
            elif entry == "filtered":
                rc = lib.md_infer_points_filtered(*head, ref(f), C.byref(o), C.byref(outs), DEV, st)
            elif entry == "normals":
                rc = lib.md_infer_points_normals(*head, ref(f), C.byref(o), C.byref(outs), ref(nrm or (zero_nrm if zero else None)), DEV, st)
            else:
                rc = lib.md_infer_points_voxel(*head, ref(f), C.byref(o), C.byref(outs), ref(nrm or (zero_nrm if zero else None)),
                                               ref(zero_vox if zero else None), DEV, st)
            _lib.check(rc)
            return _read(t)

        counts = {}
        for zero in (False, True):
            for entry, filt, normals in (("points", False, False), ("filtered", True, False), ("normals", False, False),
                                         ("normals", False, True), ("normals", True, True)):
                what = (entry, filt, normals, zero)
                counts[what] = _same_bytes(call("voxel", filt, normals, zero), call(entry, filt, normals, zero), what)
        # the filtered request is another request: the percentile removes points
        assert counts[("filtered", True, False, False)] < counts[("points", False, False, False)] < cap
        # the operators, on the model's own depth and cameras
        depth, conf, extr, intr = _da3_subset(m, x)
        cam = _lib.MdPointsCameras(intr.data_ptr(), extr.data_ptr(), None)

        def op(entry, nrm=None):
            t, _, outs = _buffers(B, S, S, cap, depth=False)
            args = (dev.handle, depth.data_ptr(), conf.data_ptr(), rgb.data_ptr(), B, S, S, C.byref(cam), C.byref(o), C.byref(outs))
            _lib.check(lib.md_op_unproject(*args, st) if entry == "plain" else lib.md_op_unproject_normals(*args, ref(nrm), st))
            return _read(t)

        plain = op("plain")
        assert _same_bytes(op("normals"), plain, "op, null") == _same_bytes(op("normals", zero_nrm), plain, "op, zero") == counts[("points", False, False, False)]
    finally:
        m.destroy()


def test_host_in_host_out_with_filter_normals_and_thinning(dev):
    """md_infer_points_voxel with the image, rgb and every output in host memory, the view filter, the normals and the thinning all
    on: each output is the device-memory call's, byte for byte, and nothing behind the surviving rows is written."""
    from burn_depth_amd.points import _points_opts, _view_filter_opts
    lib = _lib.load()
    m = _da3(dev)
    try:
        B, S = 2, 70
        cap = B * 35 * 35
        x = _image(B, S)
        rgb = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
        fkw = dict(conf_percentile=30)  # the percentile alone: two views of seeded weights confirm no pixel of each other
        full = _np(m.infer_points(x.cuda(), rgb=rgb.cuda(), world=True, **fkw, **OPTS, **NRM))
        n_full = int(full["count"][-1])
        voxel = _voxel_for(full["xyz"][:n_full], 0.5)
        o = _points_opts(world=True, **OPTS)
        fo = _view_filter_opts(o.pixel_offset, 0.0, 0.0, fkw["conf_percentile"])

        def call(host):
            t, ptr, outs = _buffers(B, S, S, cap, host=host, normals=True, thinning=True)
            nrm = _lib.MdPointsNormals(ptr("normal_map"), ptr("normals"), NRM["normal_min_cos"])
            vox = _lib.MdPointsVoxel(voxel, ptr("index"), ptr("weight"), ptr("dropped"))
            xin, cin = (x.numpy(), rgb.numpy()) if host else (x.cuda(), rgb.cuda())
            px, pc = (xin.ctypes.data, cin.ctypes.data) if host else (xin.data_ptr(), cin.data_ptr())
            kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
            _lib.check(lib.md_infer_points_voxel(m._h, C.c_void_p(px), B, S, S, kind, C.c_void_p(pc), None, C.byref(fo), C.byref(o),
                                                 C.byref(outs), C.byref(nrm), C.byref(vox), kind,
                                                 None if host else C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            return _read(t)

        on_device, on_host = call(False), call(True)
        n = _same_bytes(on_device, on_host, "host against device")
        assert 0.25 * n_full < n < 0.75 * n_full  # about half survive
        assert on_host["weight"][:n].sum() + int(on_host["dropped"][0]) == n_full
        for k in LISTS:
            assert (on_host[k][n:] == np.asarray(FILL[k], on_host[k].dtype)).all(), k
    finally:
        m.destroy()
