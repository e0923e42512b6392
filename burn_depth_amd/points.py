"""The point path's binding: its result dataclasses and the builders of every `md_points_*` struct (include/mi_depth.h).

`_points_request` turns the keyword set of `infer_points` / `ops.unproject` into one `PointsRequest`; it alone decides which
stage owns which tensor of the `PointCloud`. The builders only allocate tensors and read `data_ptr()`, so they run on any
torch device. `depth_pro` re-exports the four dataclasses; `ops` builds its list operators on the same pieces.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib


@dataclass
class RenderedPoints:
    """What `md_op_render_points` / `md_infer_points_render` return (include/mi_depth.h). Device tensors: depth f32 [T,H,W] (0 at
    holes), index int32 [T,H,W] (the winner's row, -1 at holes), rgb u8 [T,H,W,3] (with an rgb row), filled int32 [T+1]."""
    depth: Optional[torch.Tensor] = None
    index: Optional[torch.Tensor] = None
    rgb: Optional[torch.Tensor] = None
    filled: Optional[torch.Tensor] = None


@dataclass
class RasterisedMesh:
    """What `md_op_render_mesh` / `md_infer_points_raster` return (include/mi_depth.h). Device tensors: depth f32 [T,H,W] (0 at
    holes), face int32 [T,H,W] (the winning face, -1 at holes), rgb u8 [T,H,W,3] (with an rgb row; affine in screen space), filled
    int32 [T+1], skipped int32 [T+1] (faces dropped for a box beyond max_extent)."""
    depth: Optional[torch.Tensor] = None
    face: Optional[torch.Tensor] = None
    rgb: Optional[torch.Tensor] = None
    filled: Optional[torch.Tensor] = None
    skipped: Optional[torch.Tensor] = None


@dataclass
class SmoothedMesh:
    """What `md_op_smooth_mesh` / `md_infer_points_smooth` return (include/mi_depth.h). Device tensors: xyz f32 [capacity,3] the
    smoothed rows (the input bits of a row that did not move), normals f32 [capacity,3] the area-weighted vertex normals of the
    smoothed faces (None when not asked for), stats int32 [5] the invalid and degenerate faces, the rows not in range, the open
    rows and the moved rows."""
    xyz: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None
    stats: Optional[torch.Tensor] = None


@dataclass
class FittedPlanes:
    """What `md_op_fit_planes` / `md_infer_points_planes` return (include/mi_depth.h). Device tensors: plane f32 [P,4] (n.x n.y n.z d
    of every plane found, the normal facing the origin, zero rows behind them), plane_count int32 [P+1] (the inliers of every
    plane, then the planes found), hypothesis int32 [P] (the winning hypothesis, -1 behind the planes found), label int32 [rows
    of the input list] (the plane of every row, -1 none, -2 a coordinate that is not finite), dropped int32 [1]."""
    plane: Optional[torch.Tensor] = None
    plane_count: Optional[torch.Tensor] = None
    hypothesis: Optional[torch.Tensor] = None
    label: Optional[torch.Tensor] = None
    dropped: Optional[torch.Tensor] = None


@dataclass
class PointClusters:
    """What `md_op_cluster_points` / `md_infer_points_clusters` return (include/mi_depth.h). Device tensors: label, cluster_size and
    cluster int32 [rows of the input list] (the smallest core row of the row's cluster, -1 noise, -2 dropped; the rows of that
    cluster; the dense id of a kept cluster, else -1 / -2), table_label / table_size int32 [table] and box f32 [table,6] (min xyz,
    max xyz) of the kept clusters in ascending label, of which the first min(stats[1], table) are written, stats int32 [4]
    (clusters found, clusters kept, noise rows, rows in kept clusters), dropped int32 [1]."""
    label: Optional[torch.Tensor] = None
    cluster_size: Optional[torch.Tensor] = None
    cluster: Optional[torch.Tensor] = None
    table_label: Optional[torch.Tensor] = None
    table_size: Optional[torch.Tensor] = None
    box: Optional[torch.Tensor] = None
    stats: Optional[torch.Tensor] = None
    dropped: Optional[torch.Tensor] = None


@dataclass
class PointMatch:
    """What `md_op_match_points` / `md_infer_points_match` return (include/mi_depth.h). Device tensors: nearest int32 and dist2 f32
    [rows of the input list] (the nearest target row within the radius, -1 none, -2 dropped; its squared distance, +inf for -1 and
    -2 rows), stats int32 [8] (in-range rows, matched rows, target rows in the grid, 0, rows within tol[0..4)), dropped int32 [1].
    `index` is the source row of every row the call kept (modes "matched" / "unmatched"): the same tensor as the cloud's `index`."""
    nearest: Optional[torch.Tensor] = None
    dist2: Optional[torch.Tensor] = None
    stats: Optional[torch.Tensor] = None
    dropped: Optional[torch.Tensor] = None
    index: Optional[torch.Tensor] = None


@dataclass
class PointRegistration:
    """What `md_op_register_points` returns (include/mi_depth.h). Device tensors: transform f64 [12] (R row-major, then t: a row p
    moves to R p + t), pairs int32 and sum_d2 f64 [iterations + 1] (the pair count and the sum of squared distances of every
    pass; entry `iterations` is the evaluation pass under the final transform, skipped iterations are 0), stats int32 [8] (solves
    done, status 0 ran all / 1 converged / 2 too few pairs, in-range rows and pairs of the evaluation pass, target rows in the
    grid), dropped int32 [1], nearest int32 and dist2 f32 [N] (`PointMatch`'s, for the moved rows), xyz f32 [N,3] the moved rows
    and normals f32 [N,3] the rotated normals (None when not asked for). With target_normals= (the point-to-plane form,
    `md_points_register_plane`): pairs and sum_d2 cover the usable pairs only, status 3 is a degenerate system, and sum_r2 f64
    [iterations + 1] holds the sum of squared point-to-plane residuals of every pass (None in the point-to-point form)."""
    transform: Optional[torch.Tensor] = None
    pairs: Optional[torch.Tensor] = None
    sum_d2: Optional[torch.Tensor] = None
    stats: Optional[torch.Tensor] = None
    dropped: Optional[torch.Tensor] = None
    nearest: Optional[torch.Tensor] = None
    dist2: Optional[torch.Tensor] = None
    xyz: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None
    sum_r2: Optional[torch.Tensor] = None

    def matrix(self) -> torch.Tensor:
        """The transform as a 4x4 f64 matrix on the host (synchronises)."""
        a = self.transform.cpu()
        m = torch.eye(4, dtype=torch.float64)
        m[:3, :3] = a[:9].reshape(3, 3)
        m[:3, 3] = a[9:]
        return m


@dataclass
class PointCloud:
    """What `md_op_unproject` / `md_infer_points` return (include/mi_depth.h). Device tensors: the dense point map [B,H,W,3] and
    mask u8 [B,H,W]; the compacted list xyz [capacity,3] (rgb u8 [capacity,3], conf [capacity]) in (view, row, column) order, of
    which the first min(count[B], capacity) rows are points; count int32 [B+1] (per view, then the total); the depth [B,H,W].
    With normals (`md_op_unproject_normals` / `md_infer_points_normals`): normal_map [B,H,W,3] and normals [capacity,3], rows
    parallel to xyz. With voxel thinning (`md_op_voxel_thin` / `md_infer_points_voxel`): the list holds one row per occupied
    voxel, index int32 [capacity] is the source row of every output row in the unthinned list, weight int32 [capacity] the
    points of its voxel, dropped int32 [1] the rows outside the grid. With `infer_points(render=...)`
    (`md_infer_points_render`): render = the `RenderedPoints` of the list. With `mesh=` (`md_op_unproject_mesh` /
    `md_infer_points_mesh`): faces int32 [face_capacity,3] name rows of xyz, in (view, row, column, triangle) order, of which
    the first min(face_count[B], face_capacity) are faces; face_count int32 [B+1]; pixel_index int32 [B,H,W] is the row of
    every pixel in the list, -1 where it is not in it. With `raster=` (`md_infer_points_raster`): raster = the `RasterisedMesh` of
    those faces. With `outlier=` (`md_op_radius_outliers` / `md_infer_points_outlier`): the list holds the rows with at least
    min_neighbours other rows within radius; neighbours int32 [rows of the unfiltered list] is min(neighbours, min_neighbours) of
    every unfiltered row (-1 outside the grid); without voxel thinning index is the source row of every output row in the
    unfiltered list and dropped the rows outside the grid. With `ops.decimate_mesh` (`md_op_decimate_mesh`): the list is voxel
    thinning's, remap int32 [input rows] the output row of every input row's voxel (-1 outside the grid), faces / face_count the
    kept faces over the output rows, face_index int32 [face_capacity] their source faces, faces_dropped int32 [3] the invalid,
    degenerate and duplicate faces. With `components=` (`md_op_mesh_components` / `md_infer_points_components`): label int32 [rows
    of the list] the smallest row of every row's component (-1 behind the list's total), component_faces int32 [rows] its valid
    faces, faces / face_count the faces of the components that are large enough, face_index their source faces, component_stats
    int32 [5] the invalid, dropped and clipped faces and the components with a face and kept; with the operator's compact also
    index and remap. With `smooth=` (`md_infer_points_smooth`): smooth = the `SmoothedMesh` of the list over the faces the
    rasteriser reads; the list itself is unchanged. With `planes=` (`md_op_fit_planes` / `md_infer_points_planes`): planes = the
    `FittedPlanes` of the list; with its mode "drop" / "keep" the list holds the rows without / of a plane and index is the
    source row of every output row in the list in front of the stage. With `clusters=` (`md_op_cluster_points` /
    `md_infer_points_clusters`): clusters = the `PointClusters` of the list the plane stage ends with; with its mode "keep" the
    list holds the rows of kept clusters and index is their source row likewise. With `match=` (`md_op_match_points` /
    `md_infer_points_match`): match = the `PointMatch` of the list the plane stage ends with against the reference cloud; with
    its mode "matched" / "unmatched" the list holds those rows and index is their source row likewise. None when not asked for."""
    point_map: Optional[torch.Tensor] = None
    mask: Optional[torch.Tensor] = None
    xyz: Optional[torch.Tensor] = None
    rgb: Optional[torch.Tensor] = None
    conf: Optional[torch.Tensor] = None
    count: Optional[torch.Tensor] = None
    depth: Optional[torch.Tensor] = None
    normal_map: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None
    index: Optional[torch.Tensor] = None
    weight: Optional[torch.Tensor] = None
    dropped: Optional[torch.Tensor] = None
    render: Optional["RenderedPoints"] = None
    faces: Optional[torch.Tensor] = None
    face_count: Optional[torch.Tensor] = None
    pixel_index: Optional[torch.Tensor] = None
    raster: Optional["RasterisedMesh"] = None
    neighbours: Optional[torch.Tensor] = None
    remap: Optional[torch.Tensor] = None
    face_index: Optional[torch.Tensor] = None
    faces_dropped: Optional[torch.Tensor] = None
    label: Optional[torch.Tensor] = None
    component_faces: Optional[torch.Tensor] = None
    component_stats: Optional[torch.Tensor] = None
    smooth: Optional["SmoothedMesh"] = None
    planes: Optional["FittedPlanes"] = None
    clusters: Optional["PointClusters"] = None
    match: Optional["PointMatch"] = None
    registration: Optional["PointRegistration"] = None  # `register=` (`md_infer_points_register`): with apply the list itself holds the moved rows

    def points(self):
        """(xyz, rgb, conf) cut to the points that exist (reads `count`: synchronises)."""
        n = min(int(self.count[-1].item()), int(self.xyz.shape[0]))
        cut = lambda t: t[:n] if t is not None else None  # noqa: E731
        return cut(self.xyz), cut(self.rgb), cut(self.conf)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return t.data_ptr() if t is not None else None


def _f32(dev, *shape) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _i32(dev, *shape) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.int32, device=dev)


def _u8(dev, *shape) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.uint8, device=dev)


def _lattice(B: int, H: int, W: int, stride: int):
    """(rows per view, rows, default face capacity) of the strided lattice of B views of H x W pixels: what the unthinned list
    can hold, and two faces per quad."""
    s = max(int(stride), 1)  # a bad stride is the library's to refuse
    h, w = (H + s - 1) // s, (W + s - 1) // s
    return h * w, B * h * w, 2 * B * (h - 1) * (w - 1)


def _mesh_keywords(mesh, allowed: set, stage: str = "", stage_kw=(), stage_allowed=frozenset()) -> dict:
    """The keywords of mesh= (True stands for none) checked against `allowed` and, for a stage beside the mesh, its own dict
    against `stage_allowed` in the same refusal."""
    kw = dict(mesh) if isinstance(mesh, dict) else {}
    unknown = (set(kw) - allowed) | (set(stage_kw) - stage_allowed)
    if unknown:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"unknown mesh{' / ' + stage if stage else ''} keywords {sorted(unknown)}")
    return kw


def _points_opts(pixel_offset=0.0, depth_min=0.0, depth_max=0.0, conf_min=0.0, edge_rtol=0.0, stride=1, world=False) -> "_lib.MdPointsOpts":
    return _lib.MdPointsOpts(float(pixel_offset), float(depth_min), float(depth_max), float(conf_min), float(edge_rtol), int(stride),
                             int(bool(world)))


def _view_filter_opts(pixel_offset=0.0, depth_min=0.0, depth_max=0.0, conf_percentile=0, view_rtol=0.0, min_views=0) -> "_lib.MdViewFilterOpts":
    return _lib.MdViewFilterOpts(float(pixel_offset), float(depth_min), float(depth_max), int(conf_percentile), float(view_rtol), int(min_views))


def _points_outputs(dev, B: int, H: int, W: int, dense: bool, compact: bool, capacity: Optional[int], stride: int, want_rgb: bool,
                    want_conf: bool, want_depth: bool, out: Optional[PointCloud]):
    """A PointCloud of fresh device tensors (or `out`, to write into again) and its md_points_outputs."""
    if out is None:
        out = PointCloud()
        if dense:
            out.point_map, out.mask = _f32(dev, B, H, W, 3), _u8(dev, B, H, W)
        if compact:
            cap = int(capacity) if capacity is not None else _lattice(B, H, W, stride)[1]
            out.xyz, out.count = _f32(dev, cap, 3), _i32(dev, B + 1)
            out.rgb = _u8(dev, cap, 3) if want_rgb else None
            out.conf = _f32(dev, cap) if want_conf else None
        if want_depth:
            out.depth = _f32(dev, B, H, W)
    c = _lib.MdPointsOutputs(_ptr(out.point_map), _ptr(out.mask), _ptr(out.xyz), _ptr(out.rgb), _ptr(out.conf), _ptr(out.count),
                             int(out.xyz.shape[0]) if out.xyz is not None else 0, _ptr(out.depth))
    return out, c


def _points_cameras(dev, B: int, intrinsics=None, extrinsics=None, focal_px=None):
    """md_points_cameras of device fp32 tensors ([B,3,3] / [B,1,3,3], [B,3,4] / [B,1,3,4], [B] or a float). Returns (struct, keep-alive)."""
    keep = []

    def put(t, n):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t, dtype=np.float32))
        if t.numel() == 1 and n == B:
            t = t.reshape(1).expand(B)
        t = t.to(device=dev, dtype=torch.float32).contiguous()
        if t.numel() != n:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"camera tensor of {t.numel()} values, expected {n}")
        keep.append(t)
        return t.data_ptr()

    return _lib.MdPointsCameras(put(intrinsics, B * 9), put(extrinsics, B * 12), put(focal_px, B)), keep


def _points_normals(dev, B: int, H: int, W: int, normals: bool, min_cos: float, out: PointCloud, fresh: bool):
    """md_points_normals for `out`: with `fresh` (the PointCloud was made for this call) the normal tensors are created beside the
    dense map and the list it has; otherwise the ones it carries are written again, and asking for normals with an `out` that
    carries none is refused."""
    if normals and not fresh and out.normal_map is None and out.normals is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "normals=True with an `out` that carries neither `normal_map` nor `normals`")
    if fresh and normals:
        if out.point_map is not None:
            out.normal_map = _f32(dev, B, H, W, 3)
        if out.xyz is not None:
            out.normals = _f32(dev, int(out.xyz.shape[0]), 3)
    return _lib.MdPointsNormals(_ptr(out.normal_map), _ptr(out.normals), float(min_cos))


def _points_voxel(dev, voxel: float, out: PointCloud, fresh: bool):
    """md_points_voxel for `out`: with `fresh` index, weight and dropped are created beside the list it has; otherwise the ones it
    carries are written again."""
    if fresh and voxel and out.xyz is not None:
        cap = int(out.xyz.shape[0])
        out.index, out.weight, out.dropped = _i32(dev, cap), _i32(dev, cap), _i32(dev, 1)
    return _lib.MdPointsVoxel(float(voxel), _ptr(out.index), _ptr(out.weight), _ptr(out.dropped))


def _points_outlier(dev, rows: int, outlier: dict, thin: bool, out: PointCloud, fresh: bool):
    """md_points_outlier for `out`. outlier: a dict with radius and min_neighbours. rows: the rows the unfiltered list can have.
    With `fresh` neighbours (and, without thinning, index and dropped, which are the thinning's otherwise) are created beside the
    list it has; otherwise the ones it carries are written again. radius == 0 is the call without the filter and takes no tensor."""
    unknown = set(outlier) - {"radius", "min_neighbours"}
    if unknown:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"unknown outlier keywords {sorted(unknown)}")
    radius, k = float(outlier.get("radius", 0.0)), int(outlier.get("min_neighbours", 1))
    if not radius:
        return _lib.MdPointsOutlier(radius, k, None, None, None)
    if fresh and out.xyz is not None:
        out.neighbours = _i32(dev, rows)
        if not thin:
            out.index, out.dropped = _i32(dev, int(out.xyz.shape[0])), _i32(dev, 1)
    return _lib.MdPointsOutlier(radius, k, _ptr(out.neighbours), None if thin else _ptr(out.index), None if thin else _ptr(out.dropped))


def _points_mesh(dev, B: int, H: int, W: int, stride: int, mesh, out: PointCloud, fresh: bool):
    """md_points_mesh for `out`. mesh: True, or a dict with any of max_rtol (0 = no discontinuity cut), face_capacity (default:
    two faces per quad of the strided lattice) and pixel_index (default True: also return the map). With `fresh` the tensors
    are created; otherwise the ones `out` carries are written again."""
    kw = _mesh_keywords(mesh, {"max_rtol", "face_capacity", "pixel_index"})
    if mesh and not fresh and out.faces is None and out.face_count is None and out.pixel_index is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "mesh= with an `out` that carries neither `faces`, `face_count` nor `pixel_index`")
    cap = int(out.faces.shape[0]) if out.faces is not None else 0
    if fresh:
        cap = kw.get("face_capacity")
        cap = _lattice(B, H, W, stride)[2] if cap is None else int(cap)  # a negative capacity is the library's to refuse
        out.faces, out.face_count = _i32(dev, max(cap, 0), 3), _i32(dev, B + 1)
        if kw.get("pixel_index", True):
            out.pixel_index = _i32(dev, B, H, W)
    return _lib.MdPointsMesh(float(kw.get("max_rtol", 0.0)), _ptr(out.faces) or None, _ptr(out.face_count), cap, _ptr(out.pixel_index))


def _stage_faces(dev, B: int, H: int, W: int, fcap: int, kw: dict, stage: dict, out: PointCloud, alloc: bool):
    """The faces of a stage behind the mesh (decimation, island removal): faces, face_index and face_count of `out` are that
    stage's, so the mesh part carries only its edge test and the map. With `alloc` they are created, face_capacity of `stage`
    defaulting to `fcap`. -> (md_points_mesh, the stage's face capacity)."""
    if alloc:
        cap = stage.get("face_capacity")
        cap = max(fcap if cap is None else int(cap), 0)
        out.faces, out.face_index, out.face_count = _i32(dev, cap, 3), _i32(dev, cap), _i32(dev, B + 1)
        if kw.get("pixel_index", True):
            out.pixel_index = _i32(dev, B, H, W)
    frows = [int(t.shape[0]) for t in (out.faces, out.face_index) if t is not None]
    return _lib.MdPointsMesh(float(kw.get("max_rtol", 0.0)), None, None, 0, _ptr(out.pixel_index)), min(frows) if frows else 0


def _points_decimate(dev, B: int, H: int, W: int, stride: int, mesh, decimate: dict, out: PointCloud, fresh: bool):
    """(md_points_mesh, md_points_decimate) for `out` with the decimation on. mesh: True, or a dict with max_rtol / pixel_index;
    decimate: dict(voxel=, face_capacity=). With `fresh` the tensors are created beside the list `out` has; otherwise the ones
    it carries are written again."""
    kw = _mesh_keywords(mesh, {"max_rtol", "pixel_index"}, "decimate", decimate, {"voxel", "face_capacity"})
    alloc = fresh and out.xyz is not None
    _, rows, fcap = _lattice(B, H, W, stride)
    if alloc:
        cap = int(out.xyz.shape[0])
        out.index, out.weight, out.dropped, out.remap, out.faces_dropped = _i32(dev, cap), _i32(dev, cap), _i32(dev, 1), _i32(dev, rows), _i32(dev, 3)
    msh, fcap = _stage_faces(dev, B, H, W, fcap, kw, decimate, out, alloc)
    dec = _lib.MdPointsDecimate(float(decimate["voxel"]), _ptr(out.index), _ptr(out.weight), _ptr(out.dropped), _ptr(out.remap),
                                _ptr(out.faces) or None, _ptr(out.face_index) or None, _ptr(out.face_count), fcap, _ptr(out.faces_dropped))
    return msh, dec


def _points_components(dev, B: int, H: int, W: int, stride: int, mesh, components: dict, out: PointCloud, fresh: bool):
    """(md_points_mesh, md_points_components) for `out` with the island removal on. mesh: True, or a dict with max_rtol /
    pixel_index; components: dict(min_faces=, face_capacity=). With `fresh` the tensors are created; otherwise the ones `out`
    carries are written again."""
    kw = _mesh_keywords(mesh, {"max_rtol", "pixel_index"}, "components", components, {"min_faces", "face_capacity"})
    _, rows, fcap = _lattice(B, H, W, stride)
    if fresh:
        out.label, out.component_faces, out.component_stats = _i32(dev, rows), _i32(dev, rows), _i32(dev, 5)
    msh, fcap = _stage_faces(dev, B, H, W, fcap, kw, components, out, fresh)
    comp = _lib.MdPointsComponents(int(components["min_faces"]), 0, _ptr(out.label), _ptr(out.component_faces), None, None,
                                   _ptr(out.faces) or None, _ptr(out.face_index) or None, _ptr(out.face_count), fcap,
                                   _ptr(out.component_stats))
    return msh, comp


def _points_smooth(dev, smooth: dict, out: PointCloud, fresh: bool):
    """md_points_smooth for `out` with the smoothing on. smooth: dict(step=, iterations=, lam=, mu=, pin_boundary=, normals=). With
    `fresh` the tensors of `out.smooth` are created, rows parallel to the list; otherwise the ones `out` carries are written again."""
    unknown = set(smooth) - {"step", "iterations", "lam", "mu", "pin_boundary", "normals"}
    if unknown or "step" not in smooth or "lam" not in smooth:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"smooth= takes step, iterations, lam, mu, pin_boundary, normals; unknown {sorted(unknown)}")
    if out.xyz is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "smooth= needs the compacted list")
    if fresh or out.smooth is None:
        cap = int(out.xyz.shape[0])
        out.smooth = SmoothedMesh(xyz=_f32(dev, cap, 3), normals=_f32(dev, cap, 3) if smooth.get("normals") else None, stats=_i32(dev, 5))
    s = out.smooth
    return _lib.MdPointsSmooth(float(smooth["step"]), float(smooth["lam"]), float(smooth.get("mu", 0.0)), int(smooth["iterations"]),
                               1 if smooth.get("pin_boundary", True) else 0, _ptr(s.xyz), _ptr(s.normals), _ptr(s.stats))


PLANE_MODES = {"label": 0, "drop": 1, "keep": 2}
_PLANE_KEYWORDS = {"planes", "hypotheses", "tol", "min_inliers", "seed", "normal_min_cos", "axis", "axis_min_cos", "mode"}


def _planes_struct(planes: dict, fitted: "FittedPlanes", index: Optional[torch.Tensor]) -> "_lib.MdPointsPlanes":
    """md_points_planes of the keywords planes= (P), hypotheses=, tol=, min_inliers=, seed=, normal_min_cos=, axis=, axis_min_cos=,
    mode= ("label" / "drop" / "keep" or 0 / 1 / 2) writing into `fitted` and `index`. The ranges are the library's to refuse."""
    unknown = set(planes) - _PLANE_KEYWORDS
    if unknown or "tol" not in planes:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"planes= takes {sorted(_PLANE_KEYWORDS)} and needs tol; unknown {sorted(unknown)}")
    mode = planes.get("mode", 0)
    if isinstance(mode, str):
        if mode not in PLANE_MODES:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"plane mode {mode!r}: one of {sorted(PLANE_MODES)}")
        mode = PLANE_MODES[mode]
    axis = [float(v) for v in planes.get("axis", (0.0, 0.0, 0.0))]
    if len(axis) != 3:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "the plane axis has three components")
    return _lib.MdPointsPlanes(int(planes.get("planes", 1)), int(planes.get("hypotheses", 256)), float(planes["tol"]),
                               int(planes.get("min_inliers", 3)), int(planes.get("seed", 0)) & 0xFFFFFFFF,
                               float(planes.get("normal_min_cos", 0.0)), (C.c_float * 3)(*axis), float(planes.get("axis_min_cos", 0.0)),
                               int(mode), _ptr(fitted.plane), _ptr(fitted.plane_count), _ptr(fitted.hypothesis), _ptr(fitted.label),
                               _ptr(index) if mode else None, _ptr(fitted.dropped))


def _plane_mode(planes: Optional[dict]) -> int:
    """0 label, 1 drop, 2 keep; 0 also for a request that is off or whose mode the builder will refuse."""
    mode = (planes or {}).get("mode", 0) if planes and planes.get("planes", 1) else 0
    return PLANE_MODES.get(mode, 0) if isinstance(mode, str) else int(mode)


def _points_planes(dev, rows: int, planes: dict, out: PointCloud, fresh: bool):
    """md_points_planes for `out` with the stage on. rows: the rows the list in front of the stage can have. With `fresh` the
    tensors of `out.planes` are created, label over the rows of the list the stage reads (the list of the call, or with mode
    "drop" / "keep" the one in front of it) and, with those modes, index beside the list; otherwise the ones `out` carries are
    written again."""
    if out.xyz is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "planes= needs the compacted list")
    cut = _plane_mode(planes) != 0
    if fresh or out.planes is None:
        P, cap = max(int(planes.get("planes", 1)), 0), int(out.xyz.shape[0])
        out.planes = FittedPlanes(plane=_f32(dev, P, 4), plane_count=_i32(dev, P + 1), hypothesis=_i32(dev, P),
                                  label=_i32(dev, rows if cut else cap), dropped=_i32(dev, 1))
        if cut:
            out.index = _i32(dev, cap)
    return _planes_struct(planes, out.planes, out.index)


CLUSTER_MODES = {"label": 0, "keep": 1}
_CLUSTER_KEYWORDS = {"radius", "min_neighbours", "min_points", "max_points", "mode", "table"}
CLUSTER_TABLE_DEFAULT = 256


def _cluster_mode_of(mode) -> int:
    """0 label, 1 keep, by name or number; 0 also for a name the builder will refuse."""
    return CLUSTER_MODES.get(mode, 0) if isinstance(mode, str) else int(mode)


def _cluster_mode(clusters: Optional[dict]) -> int:
    """The mode of a clusters= request; 0 for one that is off."""
    return _cluster_mode_of(clusters.get("mode", 0)) if clusters and clusters.get("radius") else 0


def _new_clusters(dev, rows: int, table: int) -> "PointClusters":
    """Fresh tensors for a list of `rows` rows and a table of `table` rows."""
    table = max(int(table), 0)
    return PointClusters(label=_i32(dev, rows), cluster_size=_i32(dev, rows), cluster=_i32(dev, rows), table_label=_i32(dev, table),
                         table_size=_i32(dev, table), box=_f32(dev, table, 6), stats=_i32(dev, 4), dropped=_i32(dev, 1))


def _clusters_struct(clusters: dict, found: "PointClusters", index: Optional[torch.Tensor]) -> "_lib.MdPointsClusters":
    """md_points_clusters of the keywords radius=, min_neighbours= (k), min_points=, max_points=, mode= ("label" / "keep" or 0 / 1),
    table= (rows of the cluster table) writing into `found` and `index`. The ranges are the library's to refuse."""
    unknown = set(clusters) - _CLUSTER_KEYWORDS
    if unknown or "radius" not in clusters:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"clusters= takes {sorted(_CLUSTER_KEYWORDS)} and needs radius; unknown {sorted(unknown)}")
    mode = clusters.get("mode", 0)
    if isinstance(mode, str):
        if mode not in CLUSTER_MODES:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"cluster mode {mode!r}: one of {sorted(CLUSTER_MODES)}")
        mode = CLUSTER_MODES[mode]
    held, table = (int(found.table_label.shape[0]) if found.table_label is not None else None), clusters.get("table")
    if table is None:
        table = CLUSTER_TABLE_DEFAULT if held is None else held
    elif table >= 0 and held is not None:  # a negative one is the library's to refuse
        table = min(int(table), held)
    return _lib.MdPointsClusters(float(clusters["radius"]), int(clusters.get("min_neighbours", 0)), int(clusters.get("min_points", 1)),
                                 int(clusters.get("max_points", 0)), int(mode), _ptr(found.label), _ptr(found.cluster_size), _ptr(found.cluster),
                                 _ptr(found.table_label), _ptr(found.table_size), _ptr(found.box), int(table), _ptr(found.stats),
                                 _ptr(index) if mode else None, _ptr(found.dropped))


def _points_clusters(dev, rows: int, clusters: dict, out: PointCloud, fresh: bool):
    """md_points_clusters for `out` with the stage on. rows: the rows the list in front of the stage can have. With `fresh` the
    tensors of `out.clusters` are created, the row outputs over the rows of the list the stage reads (the list of the call, or
    with mode "keep" the one in front of it) and, with that mode, index beside the list; otherwise the ones `out` carries are
    written again."""
    if out.xyz is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "clusters= needs the compacted list")
    cut = _cluster_mode(clusters) != 0
    if fresh or out.clusters is None:
        cap = int(out.xyz.shape[0])
        table = clusters.get("table")
        out.clusters = _new_clusters(dev, rows if cut else cap, CLUSTER_TABLE_DEFAULT if table is None else table)
        if cut:
            out.index = _i32(dev, cap)
    return _clusters_struct(clusters, out.clusters, out.index)


MATCH_MODES = {"label": 0, "matched": 1, "unmatched": 2}
_MATCH_KEYWORDS = {"target", "radius", "tol", "mode"}


def _match_mode_of(mode) -> int:
    """0 label, 1 matched, 2 unmatched, by name or number; 0 also for a name the builder will refuse."""
    return MATCH_MODES.get(mode, 0) if isinstance(mode, str) else int(mode)


def _match_mode(match: Optional[dict]) -> int:
    """The mode of a match= request; 0 for one that is off."""
    return _match_mode_of(match.get("mode", 0)) if match and match.get("radius") else 0


def _new_match(dev, rows: int) -> "PointMatch":
    """Fresh tensors for a list of `rows` rows."""
    return PointMatch(nearest=_i32(dev, rows), dist2=_f32(dev, rows), stats=_i32(dev, 8), dropped=_i32(dev, 1))


def _match_target(dev, target):
    """The target of a match= request -> (pointer, rows, memory kind, keep-alive): a tensor on `dev` is read where it lies, by
    address; a numpy array or a CPU tensor is a host target, which the model call copies."""
    if isinstance(target, torch.Tensor) and target.is_cuda:
        t = target
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != torch.device(dev):
            t = t.to(device=dev, dtype=torch.float32).contiguous()
        t = t.reshape(-1, 3)
        return _ptr(t), int(t.shape[0]), _lib.MD_MEM_DEVICE, t
    host = np.ascontiguousarray(target.numpy() if isinstance(target, torch.Tensor) else target, dtype=np.float32).reshape(-1, 3)
    return (C.c_void_p(host.ctypes.data) if len(host) else None), len(host), _lib.MD_MEM_HOST, host


def _match_struct(match: dict, target, target_rows: int, target_kind: int, found: "PointMatch", index: Optional[torch.Tensor]) -> "_lib.MdPointsMatch":
    """md_points_match of the keywords target=, radius=, tol= (up to four tolerances), mode= ("label" / "matched" / "unmatched" or
    0 / 1 / 2) writing into `found` and `index`. The ranges are the library's to refuse."""
    unknown = set(match) - _MATCH_KEYWORDS
    if unknown or "radius" not in match:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"match= takes {sorted(_MATCH_KEYWORDS)} and needs radius; unknown {sorted(unknown)}")
    mode = match.get("mode", 0)
    if isinstance(mode, str):
        if mode not in MATCH_MODES:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"match mode {mode!r}: one of {sorted(MATCH_MODES)}")
        mode = MATCH_MODES[mode]
    tol = [float(v) for v in (match.get("tol") or ())]
    if len(tol) > 4:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "match= takes at most four tolerances")
    return _lib.MdPointsMatch(float(match["radius"]), target, int(target_rows), int(target_kind), int(mode), (C.c_float * 4)(*tol),
                              _ptr(found.nearest), _ptr(found.dist2), _ptr(found.stats), _ptr(index) if mode else None, _ptr(found.dropped))


def _points_match(dev, rows: int, match: dict, out: PointCloud, fresh: bool, keep: list):
    """md_points_match for `out` with the stage on. rows: the rows the list in front of the stage can have. With `fresh` the
    tensors of `out.match` are created, the row outputs over the rows of the list the stage reads (the list of the call, or with
    mode "matched" / "unmatched" the one in front of it) and, with those modes, index beside the list; otherwise the ones `out`
    carries are written again. The target's keep-alive joins `keep`."""
    if out.xyz is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "match= needs the compacted list")
    if match.get("target") is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "match= needs target")
    cut = _match_mode(match) != 0
    if fresh or out.match is None:
        cap = int(out.xyz.shape[0])
        out.match = _new_match(dev, rows if cut else cap)
        if cut:
            out.index = _i32(dev, cap)
    ptr, T, kind, alive = _match_target(dev, match["target"])
    keep.append(alive)
    out.match.index = out.index if cut else None
    return _match_struct(match, ptr, T, kind, out.match, out.index)


_REGISTER_KEYWORDS = {"target", "radius", "iterations", "init", "min_pairs", "rot_eps", "trans_eps", "apply", "target_normals"}


def _register_init(init):
    """init= of a registration -> a ctypes array of twelve doubles (R row-major, then t), or None: twelve values, or a 3x4 / 4x4 matrix."""
    if init is None:
        return None
    m = torch.as_tensor(init, dtype=torch.float64).cpu()
    if m.numel() == 16:
        m = m.reshape(4, 4)[:3]
    if m.dim() == 2:
        m = torch.cat([m[:, :3].reshape(9), m[:, 3]])
    if m.numel() != 12:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "init holds twelve values, or is a 3x4 / 4x4 matrix")
    return (C.c_double * 12)(*[float(v) for v in m.reshape(12)])


def _register_min_pairs(reg: dict) -> int:
    """min_pairs= of a registration; not given: the smallest its form takes, 3, or 6 with target_normals=."""
    given = reg.get("min_pairs")
    return given if given is not None else (6 if reg.get("target_normals") is not None else 3)


def _register_struct(reg: dict, target, target_rows: int, target_kind: int, found: "PointRegistration", keep: list) -> "_lib.MdPointsRegister":
    """md_points_register of the keywords radius=, iterations=, init=, min_pairs=, rot_eps=, trans_eps=, apply= writing into `found`.
    The ranges are the library's to refuse. The init array joins `keep`."""
    start = _register_init(reg.get("init"))
    keep.append(start)
    return _lib.MdPointsRegister(float(reg["radius"]), target, int(target_rows), int(target_kind), int(reg.get("iterations", 10)),
                                 int(_register_min_pairs(reg)), int(bool(reg.get("apply", False))), float(reg.get("rot_eps", 0.0)),
                                 float(reg.get("trans_eps", 0.0)), C.cast(start, C.c_void_p) if start is not None else None,
                                 _ptr(found.transform), _ptr(found.pairs), _ptr(found.sum_d2), _ptr(found.stats), _ptr(found.dropped),
                                 _ptr(found.nearest), _ptr(found.dist2))


def _register_plane_struct(dev, normals, target_rows: int, target_kind: int, found: "PointRegistration", keep: list) -> "_lib.MdPointsRegisterPlane":
    """md_points_register_plane of target_normals= [T,3], which is of the target's memory kind (a device tensor beside a device
    target, a numpy array or a CPU tensor beside a host target), writing sum_r2 into `found` (created here when it has none). The
    normals' keep-alive joins `keep`."""
    ptr, T, kind, alive = _match_target(dev, normals)
    if T != int(target_rows) or kind != int(target_kind):
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "target_normals is [target rows, 3] and lies where target lies (device or host)")
    keep.append(alive)
    if found.sum_r2 is None:  # zeros: a target without rows has no normals to point at, and the library then writes none
        found.sum_r2 = torch.zeros(int(found.pairs.shape[0]), dtype=torch.float64, device=dev)
    return _lib.MdPointsRegisterPlane(ptr, _ptr(found.sum_r2))


def _new_registration(dev, rows: int, iterations: int) -> "PointRegistration":
    """Fresh tensors for a list of `rows` rows and `iterations` rounds."""
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device=dev)  # noqa: E731
    history = max(int(iterations), 0) + 1
    return PointRegistration(transform=f64(12), pairs=_i32(dev, history), sum_d2=f64(history), stats=_i32(dev, 8), dropped=_i32(dev, 1),
                             nearest=_i32(dev, rows), dist2=_f32(dev, rows))


def _points_register(dev, rows: int, reg: dict, own_list: bool, out: PointCloud, fresh: bool, keep: list):
    """md_points_register for `out` with the stage on. rows: the rows the list in front of the stage can have; own_list: the
    matching or the clustering cuts, so the stage reads that list and nearest / dist2 lie over its rows, otherwise over the
    list of the call. The target's keep-alive joins `keep`."""
    unknown = set(reg) - _REGISTER_KEYWORDS
    if unknown or "radius" not in reg:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"register= takes {sorted(_REGISTER_KEYWORDS)} and needs radius; unknown {sorted(unknown)}")
    if out.xyz is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "register= needs the compacted list")
    if reg.get("target") is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "register= needs target")
    if fresh or out.registration is None:
        out.registration = _new_registration(dev, rows if own_list else int(out.xyz.shape[0]), reg.get("iterations", 10))
    ptr, T, kind, alive = _match_target(dev, reg["target"])
    keep.append(alive)
    return _register_struct(reg, ptr, T, kind, out.registration, keep)


def _points_register_plane(dev, reg: dict, part: "_lib.MdPointsRegister", out: PointCloud, keep: list):
    """md_points_register_plane for `out` behind `_points_register`'s `part`, or None without target_normals=."""
    if reg.get("target_normals") is None:
        return None
    return _register_plane_struct(dev, reg["target_normals"], part.target_rows, part.target_kind, out.registration, keep)


def _target_cameras(dev, intrinsics, extrinsics, focal_px):
    """The target cameras of a rendering or a rasterisation -> (T, md_points_cameras, keep-alive). T is the number of cameras given."""
    src = intrinsics if intrinsics is not None else focal_px
    if src is None:
        raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "neither intrinsics nor a focal length for the target cameras")
    n = src.numel() if isinstance(src, torch.Tensor) else int(np.asarray(src).size)
    T = max(n // 9 if intrinsics is not None else n, 1)
    return (T, *_points_cameras(dev, T, intrinsics, extrinsics, focal_px))


def _render_request(dev, H: int, W: int, intrinsics=None, extrinsics=None, focal_px=None, *, pixel_offset=0.0, z_near=0.0, z_far=0.0,
                    radius=0, want_rgb=False, out: Optional[RenderedPoints] = None):
    """The target cameras, options and outputs of a rendering -> (T, cameras, md_render_opts, RenderedPoints, md_render_outputs,
    keep-alive). Fresh output tensors are allocated unless `out` is given."""
    T, cam, keep = _target_cameras(dev, intrinsics, extrinsics, focal_px)
    if out is None:
        out = RenderedPoints(_f32(dev, T, H, W), _i32(dev, T, H, W), _u8(dev, T, H, W, 3) if want_rgb else None, _i32(dev, T + 1))
    o = _lib.MdRenderOpts(float(pixel_offset), float(z_near), float(z_far), int(radius))
    return T, cam, o, out, _lib.MdRenderOutputs(_ptr(out.depth), _ptr(out.index), _ptr(out.rgb), _ptr(out.filled)), keep


def _raster_request(dev, H: int, W: int, intrinsics=None, extrinsics=None, focal_px=None, *, pixel_offset=0.0, z_near=0.0, z_far=0.0,
                    cull=0, max_extent=0, want_rgb=False, out: Optional[RasterisedMesh] = None):
    """`_render_request` for a mesh rasterisation -> (T, cameras, md_raster_opts, RasterisedMesh, md_raster_outputs, keep-alive)."""
    T, cam, keep = _target_cameras(dev, intrinsics, extrinsics, focal_px)
    if out is None:
        out = RasterisedMesh(_f32(dev, T, H, W), _i32(dev, T, H, W), _u8(dev, T, H, W, 3) if want_rgb else None, _i32(dev, T + 1),
                             _i32(dev, T + 1))
    o = _lib.MdRasterOpts(float(pixel_offset), float(z_near), float(z_far), int(cull), int(max_extent))
    return T, cam, o, out, _lib.MdRasterOutputs(_ptr(out.depth), _ptr(out.face), _ptr(out.rgb), _ptr(out.filled), _ptr(out.skipped)), keep


class PointsRequest(NamedTuple):
    """One point-path call: the `PointCloud` it fills, every struct of the widest entry (`md_infer_points_smooth`) in the order
    that entry takes them, None for a part not asked for, and the tensors the camera structs point into."""
    # the field order is load-bearing: `args()` hands cam .. smo to the library in this order, which is the entry's argument order
    cloud: PointCloud
    cam: "_lib.MdPointsCameras"
    fo: Optional["_lib.MdViewFilterOpts"]
    opts: "_lib.MdPointsOpts"
    outs: "_lib.MdPointsOutputs"
    nrm: Optional["_lib.MdPointsNormals"]
    vox: Optional["_lib.MdPointsVoxel"]
    rnd: Optional["_lib.MdPointsRender"]
    msh: Optional["_lib.MdPointsMesh"]
    rst: Optional["_lib.MdPointsRaster"]
    outl: Optional["_lib.MdPointsOutlier"]
    dec: Optional["_lib.MdPointsDecimate"]
    comp: Optional["_lib.MdPointsComponents"]
    smo: Optional["_lib.MdPointsSmooth"]
    keep: list
    pln: Optional["_lib.MdPointsPlanes"] = None  # behind `keep`: `md_infer_points_planes` takes it behind `args()`
    clu: Optional["_lib.MdPointsClusters"] = None  # `md_infer_points_clusters` takes it behind `planes_args()`
    mat: Optional["_lib.MdPointsMatch"] = None  # `md_infer_points_match` takes it behind `clusters_args()`
    reg: Optional["_lib.MdPointsRegister"] = None  # `md_infer_points_register` takes it behind `match_args()`
    rpl: Optional["_lib.MdPointsRegisterPlane"] = None  # `md_infer_points_register_plane` takes it behind `register_args()`

    def args(self) -> list:
        """The struct arguments of `md_infer_points_smooth`, by reference, NULL for the parts not asked for."""
        return [C.byref(s) if s is not None else None for s in self[1:14]]

    def clusters_args(self) -> list:
        """The struct arguments of `md_infer_points_clusters`: those of `planes_args()`, then the cluster part."""
        return self.planes_args() + [C.byref(self.clu) if self.clu is not None else None]

    def match_args(self) -> list:
        """The struct arguments of `md_infer_points_match`: those of `clusters_args()`, then the match part."""
        return self.clusters_args() + [C.byref(self.mat) if self.mat is not None else None]

    def register_args(self) -> list:
        """The struct arguments of `md_infer_points_register`: those of `match_args()`, then the register part."""
        return self.match_args() + [C.byref(self.reg) if self.reg is not None else None]

    def register_plane_args(self) -> list:
        """The struct arguments of `md_infer_points_register_plane`: those of `register_args()`, then the plane part."""
        return self.register_args() + [C.byref(self.rpl) if self.rpl is not None else None]

    def planes_args(self) -> list:
        """The struct arguments of `md_infer_points_planes`: those of `args()`, then the plane part."""
        return self.args() + [C.byref(self.pln) if self.pln is not None else None]


def _points_request(dev, B: int, H: int, W: int, *, want_rgb: bool, want_conf: bool, want_depth: bool, intrinsics=None, extrinsics=None,
                    focal_px=None, dense: bool = True, compact: bool = True, capacity: Optional[int] = None,
                    out: Optional[PointCloud] = None, conf_percentile: int = 0, view_rtol: float = 0.0, min_views: int = 0,
                    normals: bool = False, normal_min_cos: float = 0.0, voxel: Optional[float] = None, render: Optional[dict] = None,
                    mesh=None, raster: Optional[dict] = None, outlier: Optional[dict] = None, decimate: Optional[dict] = None,
                    components: Optional[dict] = None, smooth: Optional[dict] = None, planes: Optional[dict] = None,
                    clusters: Optional[dict] = None, match: Optional[dict] = None, register: Optional[dict] = None,
                    opts: Optional[dict] = None) -> PointsRequest:
    """The keyword set of `infer_points` / `ops.unproject` (their docstrings say what each means) as a `PointsRequest`. opts: the
    fields of `md_points_opts`; want_rgb / want_conf / want_depth: the call can fill those outputs. A part is None when it was
    not asked for, by keyword or by an `out` that carries its tensors; fresh tensors are allocated unless `out` is given.
    voxel=None: the entry has no thinning part. render / raster: the keywords of `_render_request` / `_raster_request`; the
    images go to fresh tensors, or to the `render` / `raster` that `out` carries."""
    fresh = out is None
    # a stage given with its switch at zero is "given but off": the library gets a struct that is all zero (the outlier removal:
    # its options and no tensor) where a stage not given is NULL
    deci = bool(decimate) and bool(decimate.get("voxel"))
    isl = bool(components) and bool(components.get("min_faces"))
    o = _points_opts(**(opts or {}))
    res, outs = _points_outputs(dev, B, H, W, dense, compact, capacity, o.stride, want_rgb, want_conf, want_depth, out)
    cam, keep = _points_cameras(dev, B, intrinsics, extrinsics, focal_px)
    fo = nrm = vox = rnd = msh = rst = outl = dec = comp = smo = pln = clu = mat = reg = rpl = None
    keep_rows = _cluster_mode(clusters) != 0  # the clustering writes the list: index is its own
    match_rows = _match_mode(match) != 0  # the matching writes the list, in front of the clustering
    cut = _plane_mode(planes) != 0 or match_rows or keep_rows  # a later stage writes the list: an earlier stage's index is not returned
    if conf_percentile or view_rtol or min_views:
        fo = _view_filter_opts(o.pixel_offset, o.depth_min, o.depth_max, conf_percentile, view_rtol, min_views)
    if normals or normal_min_cos or res.normal_map is not None or res.normals is not None:
        nrm = _points_normals(dev, B, H, W, normals, normal_min_cos, res, fresh)
    # index, weight and dropped have one owner: the thinning with voxel > 0; else the decimation when it is on; else the outlier
    # removal when it is on (index and dropped); else an `out` that carries one of them asks for the thinning part at voxel 0
    filt = bool(outlier) and bool(outlier.get("radius"))
    if voxel is not None and (voxel or (not deci and not filt and (res.index is not None or res.weight is not None or res.dropped is not None))):
        vox = _points_voxel(dev, voxel, res, fresh)
        if cut:
            vox.index = vox.weight = None
            res.weight = None
    if render is not None:
        T, tcam, ro, res.render, routs, tkeep = _render_request(dev, **render, want_rgb=res.rgb is not None, out=res.render)
        rnd = _lib.MdPointsRender(T, int(render["H"]), int(render["W"]), tcam, ro, routs)
        keep = keep + tkeep
    # faces, face_count and pixel_index are the mesh's, also when only an `out` that carries them asks for it, unless the
    # decimation or the island removal is on: then the faces are that stage's and it forms the mesh part, max_rtol and pixel_index only
    if not (deci or isl) and (mesh or res.faces is not None or res.face_count is not None or res.pixel_index is not None):
        msh = _points_mesh(dev, B, H, W, o.stride, mesh, res, fresh)
    if raster is not None:
        T, tcam, so, res.raster, souts, tkeep = _raster_request(dev, **raster, want_rgb=res.rgb is not None, out=res.raster)
        rst = _lib.MdPointsRaster(T, int(raster["H"]), int(raster["W"]), tcam, so, souts)
        keep = keep + tkeep
    if outlier is not None:
        outl = _points_outlier(dev, _lattice(B, H, W, o.stride)[1], outlier, bool(voxel) or cut, res, fresh)
    if isl:
        if not mesh:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "components= needs mesh=")
        msh, comp = _points_components(dev, B, H, W, o.stride, mesh, components, res, fresh)
    elif components is not None:
        comp = _lib.MdPointsComponents()
    if deci:  # behind the island removal: with both on (the library refuses it) the mesh part and the faces of `out` are the decimation's
        if not mesh:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "decimate= needs mesh=")
        msh, dec = _points_decimate(dev, B, H, W, o.stride, mesh, decimate, res, fresh)
    elif decimate is not None:
        dec = _lib.MdPointsDecimate()
    if smooth and smooth.get("iterations"):
        if not mesh:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "smooth= needs mesh=")
        smo = _points_smooth(dev, smooth, res, fresh)
    elif smooth is not None:
        smo = _lib.MdPointsSmooth()
    if planes and planes.get("planes", 1):
        pln = _points_planes(dev, _lattice(B, H, W, o.stride)[1], planes, res, fresh)
        if keep_rows or match_rows:
            pln.index = None
    elif planes is not None:
        pln = _lib.MdPointsPlanes()
    if match and match.get("radius"):  # in front of the clustering, whose index replaces this one
        keep = list(keep)
        mat = _points_match(dev, _lattice(B, H, W, o.stride)[1], match, res, fresh, keep)
        if keep_rows:
            mat.index = None
            res.match.index = None
    elif match is not None:
        mat = _lib.MdPointsMatch()
    if register and register.get("radius"):  # directly in front of the matching, on the list it reads
        keep = list(keep)
        reg = _points_register(dev, _lattice(B, H, W, o.stride)[1], register, match_rows or keep_rows, res, fresh, keep)
        rpl = _points_register_plane(dev, register, reg, res, keep)
    elif register is not None:
        reg = _lib.MdPointsRegister()
    if clusters and clusters.get("radius"):
        clu = _points_clusters(dev, _lattice(B, H, W, o.stride)[1], clusters, res, fresh)
    elif clusters is not None:
        clu = _lib.MdPointsClusters()
    return PointsRequest(res, cam, fo, o, outs, nrm, vox, rnd, msh, rst, outl, dec, comp, smo, keep, pln, clu, mat, reg, rpl)
