"""Model -> thinned cloud in one call: `infer_points(voxel=...)` (md_infer_points_voxel) against `ops.voxel_thin`
(md_op_voxel_thin) applied to the unthinned `infer_points()` of the same call. include/mi_depth.h states the contract,
DESIGN 12.3 the kernels. Runs with `-m gpu` on an MI355X."""
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

pytestmark = pytest.mark.gpu
POISON = 123456.0
OPTS = dict(pixel_offset=0.5, stride=2, edge_rtol=0.5)
NRM = dict(normals=True, normal_min_cos=0.05)


@pytest.fixture(scope="module")
def dev():
    from burn_depth_amd.depth_pro import Device
    return Device(0)


def _da3(dev, precision="BF16", max_batch=3):
    """the reduced dual-head preset (70 x 70)"""
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthAnything3Config, Precision
    from burn_depth_amd.depth_anything3 import DepthAnything3
    cfg = DepthAnything3Config.tiny_dual_test()
    cfg.max_batch, cfg.precision = max_batch, getattr(Precision, precision)
    return DepthAnything3.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _pro(dev, precision="BF16", max_batch=2):
    """Depth Pro at the small preset (128-pixel windows, a 512 x 512 input)"""
    from burn_depth_amd import weights as Wt
    from burn_depth_amd.config import DepthProConfig, Precision
    from burn_depth_amd.depth_pro import DepthPro
    cfg = DepthProConfig.small_test()
    cfg.max_batch, cfg.precision = max_batch, getattr(Precision, precision)
    return DepthPro.new(dev, cfg, seed=0, init_scheme=Wt.INIT_PARITY)


def _image(B, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 3, S, S, generator=g) - 0.45) / 0.225


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
    m = _da3(dev)
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
    m = _pro(dev)
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
    m = _da3(dev)
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
