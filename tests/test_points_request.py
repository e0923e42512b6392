"""The point path's request builder (`burn_depth_amd.points._points_request`) on CPU tensors against expectations recorded once
from the commit before the builders moved out of `depth_pro.py` (test_points_request.json, keyed "<case>/s<stride>", then "fresh"
and, only where it differs from "fresh", "again"). The builders only allocate tensors and read `data_ptr()`, so no GPU and no
library call is needed. Per case and stride, once with fresh tensors and once with `out=` the first result ("again"): every
non-pointer struct field by value; every pointer field by the
name of the tensor of the result it aliases (null, or "stale" for the address of a tensor the result no longer holds); shape and
dtype of every tensor of the result; which structs are None; for a refusal the MdError code and message."""
import ctypes as C
import dataclasses
import json
import os

import pytest
import torch

B, H, W = 2, 5, 7  # 5 and 7 are odd, so stride 2 rounds the lattice up (3 x 4)
K = [[[100.0, 0, 3.5], [0, 100.0, 2.5], [0, 0, 1]]] * B
E = [[[1.0, 0, 0, 0.1], [0, 1.0, 0, 0.2], [0, 0, 1.0, 0.3]]] * B
TARGET = dict(H=4, W=6, focal_px=[50.0, 60.0, 70.0])
MESH = {"mesh": True}
SMOOTH = dict(step=0.01, iterations=2, lam=0.5, mu=-0.53)
INFER = dict(want_rgb=True, want_conf=True, want_depth=True, focal_px=100.0, voxel=0.0)  # what `infer_points` hands over by default

# name -> the keywords on top of INFER ("opts" is merged with the stride); "out_of": build `out` from that case first
CASES = {
    "plain": {},
    "no_rgb_conf": dict(want_rgb=False, want_conf=False),
    "world": dict(intrinsics=K, extrinsics=E, focal_px=None, opts=dict(world=True, pixel_offset=0.5, depth_min=0.1, depth_max=50.0, conf_min=0.5,
                                                                      edge_rtol=0.05)),
    "list_only": dict(dense=False),
    "dense_only": dict(compact=False),
    "capacity": dict(capacity=11),
    "filter": dict(conf_percentile=40, view_rtol=0.01, min_views=1),
    "normals": dict(normals=True),
    "normals_dense_only": dict(normals=True, compact=False),
    "min_cos": dict(normal_min_cos=0.2),
    "voxel": dict(voxel=0.05),
    "render": dict(render=dict(TARGET, radius=1, z_near=0.1)),
    "render_intrinsics": dict(render=dict(H=4, W=6, intrinsics=K, extrinsics=E)),
    "mesh_true": MESH,
    "mesh_face_capacity": dict(mesh=dict(face_capacity=9, max_rtol=0.1)),
    "mesh_no_pixel_index": dict(mesh=dict(pixel_index=False)),
    "raster": dict(MESH, raster=dict(TARGET, cull=1, max_extent=64)),
    "outlier": dict(outlier=dict(radius=0.1, min_neighbours=3)),
    "voxel_outlier": dict(voxel=0.05, outlier=dict(radius=0.1)),
    "decimate": dict(MESH, decimate=dict(voxel=0.1)),
    "decimate_face_capacity": dict(mesh=dict(max_rtol=0.2, pixel_index=False), decimate=dict(voxel=0.1, face_capacity=7)),
    "decimate_voxel": dict(MESH, voxel=0.05, decimate=dict(voxel=0.1)),
    "decimate_outlier": dict(MESH, outlier=dict(radius=0.1), decimate=dict(voxel=0.1)),
    "decimate_dense_only": dict(MESH, compact=False, decimate=dict(voxel=0.1)),
    "components": dict(MESH, components=dict(min_faces=4)),
    "components_face_capacity": dict(mesh=dict(max_rtol=0.2), components=dict(min_faces=4, face_capacity=7)),
    "components_decimate": dict(MESH, components=dict(min_faces=4), decimate=dict(voxel=0.1)),
    "smooth": dict(MESH, smooth=SMOOTH),
    "smooth_normals": dict(MESH, smooth=dict(SMOOTH, normals=True, pin_boundary=False)),
    "smooth_components": dict(MESH, components=dict(min_faces=4), smooth=SMOOTH),
    "everything": dict(MESH, normals=True, conf_percentile=10, render=TARGET, raster=TARGET, components=dict(min_faces=2), smooth=SMOOTH),
    "off_decimate": dict(mesh=dict(face_capacity=9), decimate=dict(voxel=0)),
    "off_components": dict(MESH, components=dict(min_faces=0)),
    "off_smooth": dict(MESH, smooth=dict(SMOOTH, iterations=0)),
    "off_smooth_no_mesh": dict(smooth=dict(iterations=0)),
    "off_outlier": dict(outlier=dict(radius=0, min_neighbours=2)),
    "off_all_no_mesh": dict(decimate=dict(voxel=0), components=dict(min_faces=0), smooth=dict(iterations=0), outlier={}),
    "unproject": dict(want_depth=False, voxel=None, focal_px=None, intrinsics=K),
    "unproject_mesh_normals": dict(want_depth=False, voxel=None, normals=True, normal_min_cos=0.1, mesh=dict(max_rtol=0.05)),
    # an `out` that carries a part's tensors asks for that part
    "out_voxel_plain_call": dict(out_of="voxel"),
    "out_outlier_plain_call": dict(out_of="outlier"),
    "out_mesh_normals_plain_call": dict(out_of="unproject_mesh_normals"),
    "out_decimate_no_thinning_part": dict(out_of="decimate", voxel=None, **MESH, decimate=dict(voxel=0.1)),
    # refusals
    "refuse_out_without_normals": dict(out_of="plain", normals=True),
    "refuse_out_without_mesh": dict(out_of="plain", **MESH),
    "refuse_mesh_keyword": dict(mesh=dict(bogus=1, other=2)),
    "refuse_outlier_keyword": dict(outlier=dict(radius=0.1, bogus=1)),
    "refuse_decimate_keyword": dict(mesh=dict(face_capacity=9), decimate=dict(voxel=0.1, bogus=1)),
    "refuse_components_keyword": dict(mesh=dict(face_capacity=9), components=dict(min_faces=4, bogus=1)),
    "refuse_smooth_keyword": dict(MESH, smooth=dict(SMOOTH, bogus=1)),
    "refuse_smooth_without_step": dict(MESH, smooth=dict(iterations=2, lam=0.5)),
    "refuse_components_without_mesh": dict(components=dict(min_faces=4), decimate=dict(voxel=0.1), smooth=SMOOTH),
    "refuse_decimate_without_mesh": dict(decimate=dict(voxel=0.1), smooth=SMOOTH),
    "refuse_smooth_without_mesh": dict(smooth=SMOOTH),
    "refuse_smooth_without_list": dict(MESH, compact=False, smooth=SMOOTH),
    "refuse_render_without_cameras": dict(render=dict(H=4, W=6)),
    "refuse_raster_without_cameras": dict(MESH, raster=dict(H=4, W=6)),
    "refuse_camera_shape": dict(focal_px=None, intrinsics=[1.0, 2.0, 3.0, 4.0, 5.0]),
    "refuse_outlier_before_components": dict(outlier=dict(bogus=1), components=dict(min_faces=4)),
}
STRUCTS = ("cam", "fo", "opts", "outs", "nrm", "vox", "rnd", "msh", "rst", "outl", "dec", "comp", "smo")  # the widest entry's order


def keywords(case: str, stride: int) -> dict:
    kw = {**INFER, **{k: v for k, v in CASES[case].items() if k != "out_of"}}
    kw["opts"] = dict(kw.get("opts", {}), stride=stride)
    return kw


def tensors_of(cloud) -> dict:
    """name -> tensor for every tensor of the result, the nested results as `render.depth`."""
    named = {}
    for f in dataclasses.fields(cloud):
        v = getattr(cloud, f.name)
        if isinstance(v, torch.Tensor):
            named[f.name] = v
        elif v is not None:
            named.update({f"{f.name}.{g.name}": getattr(v, g.name) for g in dataclasses.fields(v) if getattr(v, g.name) is not None})
    return named


def describe_struct(s, names: dict):
    if s is None:
        return None
    d = {}
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            d[name] = describe_struct(v, names)
        elif ctype is C.c_void_p:
            d[name] = None if not v else names.get(v, "stale")
        else:
            d[name] = v
    return d


def describe(cloud, structs: dict, keep: list) -> dict:
    """The JSON form of one built request. structs: name -> ctypes struct or None, for STRUCTS."""
    named = tensors_of(cloud)
    names = {t.data_ptr(): n for n, t in named.items()}
    assert len(names) == len(named) and 0 not in names, "two tensors of the result share an address"
    names.update({t.data_ptr(): f"keep[{i}]" for i, t in enumerate(keep)})
    return {"tensors": {n: [list(t.shape), str(t.dtype)] for n, t in named.items()},
            "keep": [[list(t.shape), t.flatten().tolist()] for t in keep],
            "structs": {n: describe_struct(structs[n], names) for n in STRUCTS}}


def run_case(build, case: str, stride: int) -> dict:
    """`build(**keywords) -> (cloud, structs, keep)` on one case -> {"fresh": ..., "again": ...}, or {"fresh": {"error": ...}}."""
    from burn_depth_amd import _lib
    out_of = CASES[case].get("out_of")
    out = build(**keywords(out_of, stride))[0] if out_of else None
    try:
        cloud, structs, keep = build(**keywords(case, stride), out=out)
    except _lib.MdError as e:
        return {"fresh": {"error": [e.code, e.message]}}
    got = {"fresh": describe(cloud, structs, keep)}
    again, structs, keep = build(**keywords(case, stride), out=cloud)
    assert again is cloud
    got["again"] = describe(again, structs, keep)
    return got


@pytest.fixture
def keep_alive(monkeypatch):
    """Every tensor `torch.empty` makes stays alive for the test, so an address is never handed out twice and a pointer to a
    tensor the result no longer holds reads "stale", not the name of whatever the allocator put there next."""
    made, empty = [], torch.empty

    def keeping(*a, **k):
        made.append(empty(*a, **k))
        return made[-1]

    monkeypatch.setattr(torch, "empty", keeping)
    return made


def _build(**kw):
    from burn_depth_amd.points import _points_request
    rq = _points_request(torch.device("cpu"), B, H, W, **kw)
    return rq.cloud, {n: getattr(rq, n) for n in STRUCTS}, rq.keep


with open(os.path.splitext(__file__)[0] + ".json") as _f:
    EXPECTED = json.load(_f)


def test_the_recording_covers_the_matrix():
    assert sorted(EXPECTED) == sorted(f"{c}/s{s}" for c in CASES for s in (1, 2))


@pytest.mark.parametrize("stride", (1, 2))
@pytest.mark.parametrize("case", sorted(CASES))
def test_request_matches_the_recording(case, stride, keep_alive):
    got = json.loads(json.dumps(run_case(_build, case, stride)))  # tuples and lists compare alike
    want = EXPECTED[f"{case}/s{stride}"]
    assert ("error" in got["fresh"]) == ("error" in want["fresh"]), got["fresh"].get("error")
    for which in got:
        expect = want.get(which, want["fresh"])  # "again" is recorded only where it differs
        assert sorted(got[which]) == sorted(expect)
        for part in expect:
            assert got[which][part] == expect[part], (which, part)


def test_args_are_the_widest_entry_s_structs_in_order(keep_alive):
    from burn_depth_amd import _lib
    from burn_depth_amd.points import _points_request
    rq = _points_request(torch.device("cpu"), B, H, W, **keywords("everything", 2))
    args, types = rq.args(), _lib.SYMBOLS["md_infer_points_smooth"][1][7:-2]
    assert len(args) == len(types) == len(STRUCTS)
    for a, t, n in zip(args, types, STRUCTS):
        s = getattr(rq, n)
        assert (a is None) == (s is None) and (s is None or (isinstance(s, t._type_) and C.addressof(a._obj) == C.addressof(s))), n
    assert [n for n in STRUCTS if getattr(rq, n) is None] == ["vox", "outl", "dec"]


def test_depth_pro_re_exports_the_results_and_points_stands_alone():
    import ast
    from burn_depth_amd import depth_pro, points
    assert all(getattr(depth_pro, n) is getattr(points, n) for n in ("PointCloud", "RenderedPoints", "RasterisedMesh", "SmoothedMesh"))
    with open(points.__file__) as f:
        tree = ast.parse(f.read())
    local = [a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level for a in n.names]
    assert local == ["_lib"]  # no import cycle: nothing of the package but the ctypes binding
