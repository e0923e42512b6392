"""Model -> cloud matched against a reference cloud in one call: `infer_points(match=...)` (md_infer_points_match) against
`pipeline.match_points` applied to the copied list of `infer_points()` of the same call: the three modes, device and host target,
device and host outputs, between the plane stage and the clustering, graph replay, and the refusals. include/mi_depth.h states the
contract, DESIGN 12.13 the kernels. Runs with `-m gpu` on an MI355X."""
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
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
LIST = ("xyz", "conf", "rgb", "normals")
DENSE = ("point_map", "mask", "normal_map", "depth")
MODES = ("label", "matched", "unmatched")
INF_BITS = 0x7F800000


def _np(pc):
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy() if t is not None else None  # noqa: E731
    d = {k: g(v) for k, v in vars(pc).items() if k not in ("render", "raster", "smooth", "planes", "clusters", "match")}
    if pc.match is not None:
        d.update({k: g(getattr(pc.match, k)) for k in ("nearest", "dist2", "stats", "dropped")})
    if pc.clusters is not None:
        d.update({"cluster": g(pc.clusters.cluster), "cluster_stats": g(pc.clusters.stats)})
    return d


def _rows(full, k):
    n = int(full["count"][-1])
    return full[k][:n] if full[k] is not None else None


def _host(full, target, radius, tol, mode):
    """pipeline.match_points on the copied list `full` (a dict of numpy rows with `count`), with its per-view counts"""
    return P.match_points(_rows(full, "xyz"), target, radius, tol=tol, mode=mode, conf=_rows(full, "conf"), rgb=_rows(full, "rgb"),
                          normals=_rows(full, "normals"), counts=full["count"][:-1])


def _same(want, got, full, what=""):
    """got: the model call's outputs, poisoned before the call; want: HostMatch of the list `full` the stage read"""
    n = int(full["count"][-1])
    assert got["stats"].tolist() == want.stats.tolist() and int(got["dropped"][0]) == want.dropped, (what, got["stats"], want.stats)
    assert np.array_equal(got["nearest"][:n], want.nearest) and np.array_equal(got["dist2"][:n].view(np.uint32), want.dist2.view(np.uint32)), what
    assert (got["nearest"][n:] == -7).all() and len(got["nearest"]) > n and (got["dist2"][n:] == np.float32(POISON)).all(), what  # not rows
    if want.index is None:  # mode 0: the list is the one the stage read
        assert np.array_equal(got["count"], full["count"]), what
        for k in LIST:
            if full[k] is not None:
                assert np.array_equal(got[k][:n].view(np.uint8), full[k][:n].view(np.uint8)), (what, k)
        return
    m = len(want.index)
    assert np.array_equal(got["count"], want.count), (what, got["count"], want.count)
    for k in LIST + ("index",):
        ref = getattr(want, k)
        assert (ref is None) == (got[k] is None), (what, k)
        if ref is not None:
            assert np.array_equal(got[k][:m].view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), (what, k)
    assert (got["xyz"][m:] == np.float32(POISON)).all(), what  # nothing behind the survivors is written


def _poison(out):
    for t in (out.xyz, out.normals, out.conf, out.match.dist2):
        if t is not None:
            t.fill_(POISON)
    for t in (out.index, out.count, out.match.nearest, out.match.stats, out.match.dropped):
        if t is not None:
            t.fill_(-7)
    if out.clusters is not None:
        out.clusters.cluster.fill_(-7)


def _poisoned(m, x, **kw):
    out = m.infer_points(x, **kw)
    _poison(out)
    return m.infer_points(x, out=out, **kw)


def _radius_for(full, frac=0.02):
    n = int(full["count"][-1])
    return float(np.float32(frac * np.ptp(full["xyz"][:n], axis=0).max()))


def test_da3_two_views_match_equals_matching_the_list_of_the_call(dev):
    m = _da3(dev, max_batch=2)
    try:
        x, shifted = _image(2, 70).cuda(), torch.roll(_image(2, 70), (3, 2), (2, 3)).cuda()
        rgb = torch.randint(0, 256, (2, 70, 70, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
        kw = dict(world=True, rgb=rgb, normals=True, **OPTS)
        full = _np(m.infer_points(x, **kw))
        ref = _np(m.infer_points(shifted, **kw))  # the target: the same model's cloud of a shifted image
        n = int(full["count"][-1])
        target = np.ascontiguousarray(ref["xyz"][:int(ref["count"][-1])])
        assert n > 500 and len(target) > 500 and full["count"][0] > 0 and full["count"][1] > 0
        r = _radius_for(full)
        tol = (r / 2, r)
        part = P.match_points(full["xyz"][:n], target, r)
        assert 0 < part.stats[1] < part.stats[0], part.stats  # the reference matches part of the rows but not all
        on_device = torch.from_numpy(target).cuda()
        for mode, name in enumerate(MODES):
            want = _host(full, target, r, tol, mode)
            assert mode == 0 or (want.count[0] > 0 and want.count[1] > 0 and want.count[:2].sum() == want.count[2])  # count[b] per view, B = 2
            for tgt in (on_device, target):  # a device target, a host target
                got = _np(_poisoned(m, x, match=dict(target=tgt, radius=r, tol=tol, mode=name), **kw))
                _same(want, got, full, (name, type(tgt).__name__))
        # graph replay on the same pointers: nothing is allocated after the first call, and a replay reads the target's current contents
        mat = dict(target=on_device, radius=r, tol=tol, mode="unmatched")
        want = _host(full, target, r, tol, 2)
        m.enable_graph(True)
        out = m.infer_points(x, match=mat, **kw)
        allocs = m.query("allocs")
        for call in (1, 2, 3):  # 1: capture, 2 and 3: replay
            _poison(out)
            out = m.infer_points(x, out=out, match=mat, **kw)
            _same(want, _np(out), full, f"graph call {call}")
        moved = target + np.float32(r / 4)
        on_device.copy_(torch.from_numpy(moved))  # in place: the same address, other contents
        changed = _host(full, moved, r, tol, 2)
        assert not np.array_equal(changed.nearest, want.nearest)
        _poison(out)
        out = m.infer_points(x, out=out, match=mat, **kw)
        _same(changed, _np(out), full, "replay after the target changed")
        assert m.query("allocs") == allocs and m.query("match_overflow") == 0
        m.enable_graph(False)
        on_device.copy_(torch.from_numpy(target))
        # drop the floor, drop what the reference holds, cluster the rest: the three host references chained
        pln = dict(planes=1, hypotheses=65, tol=r / 2, min_inliers=20, seed=5, mode="drop")
        clu = dict(radius=r, min_neighbours=2, min_points=3, mode="keep", table=64)
        got = _np(_poisoned(m, x, planes=pln, match=dict(target=on_device, radius=r, tol=tol, mode="unmatched"), clusters=clu, **kw))
        counts = full["count"][:-1]
        a = P.fit_planes(full["xyz"][:n], normals=full["normals"][:n], conf=full["conf"][:n], rgb=full["rgb"][:n], counts=counts,
                         **dict(pln, mode=1))
        assert 0 < len(a.index) < n
        b = P.match_points(a.xyz, target, r, tol=tol, mode=2, conf=a.conf, rgb=a.rgb, normals=a.normals, counts=a.count[:-1])
        assert 0 < len(b.index) < len(a.index)
        c = P.cluster_points(b.xyz, conf=b.conf, rgb=b.rgb, normals=b.normals, counts=b.count[:-1], **dict(clu, mode=1))
        assert 0 < len(c.index) < len(b.index)
        assert np.array_equal(got["count"], c.count), (got["count"], c.count)
        for k in LIST + ("index",):
            assert np.array_equal(got[k][:len(c.index)].view(np.uint8), np.ascontiguousarray(getattr(c, k)).view(np.uint8)), k
        assert np.array_equal(got["nearest"][:len(a.index)], b.nearest) and got["stats"].tolist() == b.stats.tolist()
        assert np.array_equal(got["cluster"][:len(b.index)], c.cluster) and got["cluster_stats"].tolist() == c.stats.tolist()
    finally:
        m.enable_graph(False)
        m.destroy()


def test_depth_pro_match_and_the_call_without_the_stage(dev):
    m = _pro(dev, "tiny")
    try:
        x = _image(2, 512).cuda()
        kw = dict(normals=True, **dict(OPTS, stride=8))
        full = _np(m.infer_points(x, **kw))
        n = int(full["count"][-1])
        assert n > 500 and full["conf"] is None
        ref = _np(m.infer_points(torch.roll(x, (5, 3), (2, 3)), **kw))
        target = np.ascontiguousarray(ref["xyz"][:int(ref["count"][-1])])
        r = _radius_for(full, 0.01)
        want = _host(full, target, r, (r,), 1)
        assert 0 < want.stats[1] < want.stats[0], want.stats
        mat = dict(target=torch.from_numpy(target).cuda(), radius=r, tol=(r,), mode="matched")
        _same(want, _np(_poisoned(m, x, match=mat, **kw)), full, "depth pro")
        # match=None and radius 0 are the cluster entry's call, bit for bit, with the same launches
        clu = dict(radius=r, min_neighbours=2, min_points=3, table=16)
        m.enable_timing(True)
        m.read_timing()  # empties the launch order
        base = m.infer_points(x, clusters=clu, **kw)
        order = m.read_launch_order()
        base = _np(base)
        for off in (None, dict(radius=0.0)):
            m.read_timing()
            got = m.infer_points(x, clusters=clu, match=off, **kw)
            assert got.match is None and m.read_launch_order() == order and "points_match" not in order
            got = _np(got)
            for k in LIST + DENSE + ("count", "cluster", "cluster_stats"):
                rows = n if k in LIST + ("cluster",) else None
                assert (got[k] is None) == (base[k] is None) and (got[k] is None or np.array_equal(got[k][:rows].view(np.uint8), base[k][:rows].view(np.uint8))), k
        m.read_timing()
        m.infer_points(x, planes=dict(planes=1, hypotheses=8, tol=0.1), clusters=clu, match=dict(mat, mode="label"), **kw)
        assert m.read_launch_order()[-3:] == ["points_planes", "points_match", "points_clusters"]
        m.enable_timing(False)
    finally:
        m.destroy()


def test_refusals_and_host_outputs(dev):
    from burn_depth_amd.points import _points_opts
    lib = _lib.load()
    m = _da3(dev, max_batch=2)
    try:
        x = _image(2, 70)
        xd = x.cuda()
        kw = dict(world=True, **OPTS)
        first = _np(m.infer_points(xd, **kw))
        n = int(first["count"][-1])
        ref = _np(m.infer_points(torch.roll(xd, (3, 2), (2, 3)), **kw))
        target = np.ascontiguousarray(ref["xyz"][:int(ref["count"][-1])])
        tgt = torch.from_numpy(target).cuda()
        r = _radius_for(first)
        ok = dict(target=tgt, radius=r)
        m.enable_timing(True)
        m.infer_points(xd, match=ok, **kw)
        order = m.read_launch_order()
        pln = dict(planes=1, hypotheses=8, tol=0.1)
        clu = dict(radius=r, mode="keep")
        bad = [dict(match=dict(ok, radius=-1.0)), dict(match=dict(ok, radius=float("inf"))), dict(match=dict(ok, radius=1e30)),
               dict(match=dict(ok, tol=(-1.0,))), dict(match=dict(ok, tol=(2 * r,))), dict(match=dict(ok, tol=(float("nan"),))),
               dict(match=dict(ok, mode=3)), dict(match=dict(ok, mode=-1)),
               dict(match=dict(ok, mode="matched"), mesh=True), dict(match=dict(ok, mode="unmatched"), mesh=True, components=dict(min_faces=2)),
               dict(match=dict(ok, mode="matched"), mesh=True, decimate=dict(voxel=0.1)),
               dict(match=dict(ok, mode="matched"), mesh=True, smooth=dict(step=1e-3, iterations=1, lam=0.5)),
               dict(match=dict(ok, mode="matched"), planes=pln),  # the rows the plane labels are parallel to would not be returned
               dict(match=ok, clusters=clu),  # cluster mode 1 behind match mode 0: not the rows `nearest` is parallel to
               dict(match=ok, mesh=True, decimate=dict(voxel=0.1))]
        for b in bad:
            with pytest.raises(_lib.MdError) as e:
                m.infer_points(xd, **kw, **b)
            assert e.value.code == _lib.MD_ERR_INVALID_ARG, b
        assert m.read_launch_order() == order  # nothing was enqueued by a refused call
        m.enable_timing(False)
        assert m.query("match_overflow") == 0
        # the library's own refusals of a struct the builder cannot form; everything in host memory against the device-memory call
        B, S = 2, 70
        cap = B * 35 * 35
        o = _points_opts(world=True, **OPTS)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f, i32 = np.float32, np.int32
        shapes = dict(xyz=((cap, 3), f, POISON), conf=((cap,), f, POISON), count=((B + 1,), i32, -7), nearest=((cap,), i32, -7),
                      dist2=((cap,), f, POISON), stats=((8,), i32, -7), index=((cap,), i32, -7), dropped=((1,), i32, -7))

        def run(host, mode, radius=r, expect=_lib.MD_OK, parts=None, **over):
            t = {k: np.full(shape, fill, dt) for k, (shape, dt, fill) in shapes.items()}
            if not host:
                t = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            ptr = lambda k: t[k].ctypes.data if host else t[k].data_ptr()  # noqa: E731
            outs = _lib.MdPointsOutputs(None, None, ptr("xyz"), None, ptr("conf"), ptr("count"), cap, None)
            fields = dict(radius=radius, target=target.ctypes.data if host else tgt.data_ptr(), target_rows=len(target),
                          target_kind=_lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE, mode=mode, tol=(C.c_float * 4)(r / 2, r),
                          nearest=ptr("nearest"), dist2=ptr("dist2"), stats=ptr("stats"), index=ptr("index") if mode else None, dropped=ptr("dropped"))
            fields.update(over)
            if "count" in over:
                outs.count = fields.pop("count")
            mat = _lib.MdPointsMatch(**fields)
            kind = _lib.MD_MEM_HOST if host else _lib.MD_MEM_DEVICE
            px = x.numpy().ctypes.data if host else xd.data_ptr()
            part = lambda k: C.byref(parts[k]) if parts and k in parts else None  # noqa: E731
            rc = lib.md_infer_points_match(m._h, C.c_void_p(px), B, S, S, kind, None, None, None, C.byref(o), C.byref(outs), None, part("vox"), None,
                                           None, None, part("outl"), None, None, None, part("pln"), part("clu"), C.byref(mat), kind,
                                           None if host else st)
            assert rc == expect, (rc, lib.md_last_error().decode())
            torch.cuda.synchronize()
            return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in t.items()}

        run(False, 0, radius=0.0, expect=_lib.MD_ERR_INVALID_ARG)  # its pointers are still set
        run(False, 0, expect=_lib.MD_ERR_INVALID_ARG, count=None)  # the stage without the list's count
        run(False, 0, expect=_lib.MD_ERR_INVALID_ARG, index=tgt.data_ptr())  # index without mode 1 / 2
        run(False, 0, expect=_lib.MD_ERR_INVALID_ARG, target_rows=-1)
        run(False, 0, expect=_lib.MD_ERR_INVALID_ARG, target=None)
        run(False, 0, expect=_lib.MD_ERR_INVALID_ARG, target_kind=7)
        run(False, 0, expect=_lib.MD_ERR_SHAPE, target_rows=1 << 30)
        # modes 1 / 2 with an earlier stage's index, and cluster mode 1 with the match stage's: the rows they are parallel to are not
        # returned. `infer_points` never forms such a call (it leaves those pointers out), so the structs are formed here. Each
        # call is in order once the pointer is gone, so it is this refusal that answers; nothing is enqueued by a refused call
        rows = torch.empty(cap, dtype=torch.int32, device="cuda")
        earlier = lambda index: dict(  # noqa: E731
            vox=_lib.MdPointsVoxel(voxel=r, index=index), outl=_lib.MdPointsOutlier(radius=r, min_neighbours=1, index=index),
            pln=_lib.MdPointsPlanes(planes=1, hypotheses=8, tol=r, min_inliers=3, mode=1, index=index))
        keep = _lib.MdPointsClusters(radius=r, min_points=1, mode=1)
        for mode in (1, 2):
            for k, part in earlier(None).items():
                run(False, mode, parts={k: part})
            run(False, mode, parts=dict(clu=keep), index=None)
        m.enable_timing(True)
        m.read_timing()  # empties the launch order
        run(False, 1)
        order = m.read_launch_order()
        assert "points_match" in order
        for mode in (1, 2):
            for k, part in earlier(rows.data_ptr()).items():
                run(False, mode, expect=_lib.MD_ERR_INVALID_ARG, parts={k: part})
                assert "index" in lib.md_last_error().decode() and "matching" in lib.md_last_error().decode(), (mode, k)
            run(False, mode, expect=_lib.MD_ERR_INVALID_ARG, parts=dict(clu=keep))  # mat->index is set
            assert "index" in lib.md_last_error().decode() and "clustering" in lib.md_last_error().decode(), mode
        assert m.read_launch_order() == order
        m.enable_timing(False)
        for mode in (0, 1, 2):
            want = P.match_points(first["xyz"][:n], target, r, tol=(r / 2, r), mode=mode, conf=first["conf"][:n], counts=first["count"][:-1])
            on_device, on_host = run(False, mode), run(True, mode)
            cnt = int(on_device["count"][-1])
            assert (0 < cnt < n and cnt == len(want.index)) if mode else cnt == n
            for t in (on_device, on_host):
                assert np.array_equal(t["nearest"][:n], want.nearest) and np.array_equal(t["dist2"][:n].view(np.uint32), want.dist2.view(np.uint32)), mode
                assert t["stats"].tolist() == want.stats.tolist() and (t["nearest"][n:] == -7).all(), mode
                assert (t["index"][cnt if mode else 0:] == -7).all() and (t["xyz"][cnt:] == np.float32(POISON)).all(), mode
                if mode:
                    assert np.array_equal(t["index"][:cnt], want.index) and np.array_equal(t["count"], want.count), mode
                    assert np.array_equal(t["xyz"][:cnt].view(np.uint32), want.xyz.view(np.uint32)), mode
                    assert np.array_equal(t["conf"][:cnt].view(np.uint32), want.conf.view(np.uint32)), mode
    finally:
        m.destroy()


def test_infer_cli_prints_the_match_and_writes_the_label(dev, tmp_path, capsys):
    """tools/infer.py --ply --match-ply REF.ply --match-radius R: one image through the stage of the model call, --views through
    ops.match_points on the points of the file; label writes `nearest >= 0`, unmatched the points without a counterpart"""
    import importlib.util
    from burn_depth_amd import ops
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
    assert cli.main(one + ["--match-ply", ref_ply]) == 2  # without a radius
    assert cli.main(one + ["--mesh", "--match-ply", ref_ply, "--match-radius", "1", "--match-mode", "matched"]) == 2
    assert cli.main(one + ["--match-ply", ref_ply, "--match-radius", "1", "--cluster-radius", "1", "--cluster-mode", "keep"]) == 2
    for head in (one, views):
        assert cli.main(head) == 0
        xyz0, col0 = P.read_ply(ply)
        fin = xyz0[np.isfinite(xyz0).all(1)]
        radius = float(np.float32(0.01 * np.ptp(fin, axis=0).max()))
        ref = (xyz0[::2] + np.float32(radius / 3)).astype(np.float32)  # every second point, moved by less than the radius
        P.write_ply(ref_ply, ref, col0[::2])
        want = ops.match_points(dev, torch.from_numpy(xyz0).cuda(), torch.from_numpy(P.read_ply(ref_ply)[0]).cuda(), radius, tol=(radius / 2, radius)).match
        torch.cuda.synchronize()
        stats, hit = want.stats.cpu().tolist(), (want.nearest >= 0).cpu().numpy()
        assert 0 < stats[1] < stats[0]
        opts = ["--match-ply", ref_ply, "--match-radius", repr(radius), "--match-tol", repr(radius / 2), repr(radius)]
        capsys.readouterr()
        assert cli.main(head + opts) == 0
        said = capsys.readouterr().out.splitlines()
        assert any(l.startswith(f"Match: {stats[0]} points in range, {stats[1]} with a counterpart") for l in said), said
        assert [l.split("(")[1] for l in said if l.startswith("Precision at ")] == [f"{stats[4 + t]} of {len(xyz0)} points)" for t in range(2)], said
        xyz1, _ = P.read_ply(ply)
        assert np.array_equal(xyz1.view(np.uint32), xyz0.view(np.uint32)) and np.array_equal(P.read_ply_label(ply), hit.astype(np.int32))
        assert cli.main(head + opts + ["--match-mode", "unmatched"]) == 0
        xyz2, col2 = P.read_ply(ply)
        keep = (want.nearest == -1).cpu().numpy()
        assert np.array_equal(xyz2.view(np.uint32), xyz0[keep].view(np.uint32)) and np.array_equal(col2, col0[keep])
        assert P.read_ply_label(ply) is None
