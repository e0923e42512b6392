"""Counterpart of the reference's `example/inference.rs`: image -> depth PNG.

  python tools/infer.py --model depth-pro        --checkpoint depth_pro.safetensors --image photo.npy [--output depth.png]
  python tools/infer.py --model depth-anything-3 --checkpoint da3_small.safetensors  --image photo.npy
  python tools/infer.py --model depth-pro        --checkpoint depth_pro.safetensors --image photo.npy --focal-px 1200

`--focal-px F` (Depth Pro only): the camera's known focal length in pixels of the image; the FOV network does not run.
`--on-device`: the whole flow (prepare, inference, restore, min-max normalisation, 8-bit pixels) runs in one device call,
`md_process_frame`; the PNG is the same as the default path's up to the resize's rounding (bit-identical when the image
needs no resize).

`--ply OUT.ply`: also writes the depth as a coloured point cloud (binary little-endian PLY), back-projected on the device in the
same call as the inference (`md_infer_points`): Depth Pro with its predicted (or `--focal-px`) focal length in camera space,
Depth-Anything-v3 `small` with its predicted intrinsics / extrinsics in world space. `--normals` adds the surface
normals (`nx ny nz`, `md_infer_points_normals`) and `--normal-min-cos` drops surfaces seen at a grazing angle. `--conf-min`, `--edge-rtol`, `--stride`
filter the cloud (`md_points_opts`); `--conf-percentile Q` first drops the lowest Q % of the confidences on the device
(`md_infer_points_filtered`; Depth-Anything-v3 `small`, whose confidence has no scale a caller could know in advance).

`--views A.npy B.npy ...` (Depth-Anything-v3 `small`): the images are the views of ONE scene, the first one its reference view; they run
through `infer_views` (cross-view attention, `md_da3_infer_views`), so depths and cameras are mutually consistent. One depth PNG per
view is written beside `--output` (`depth_v0.png`, ...). With `--ply` the device outputs go to `ops.filter_views` (`--view-rtol`,
`--min-views`, `--conf-percentile`) and `ops.unproject` with the model's own extrinsics and intrinsics: one world-space cloud.

`--voxel X` (with `--ply`): the cloud is thinned on the device to one point per occupied voxel of side X, the most confident one
(`md_infer_points_voxel`; with `--views`, `ops.voxel_thin` over the cloud of all views, which share the grid).

`--outlier-radius R [--outlier-min K]` (with `--ply`): the points with fewer than K (default 8) other points within R leave the cloud
on the device before the thinning and the render see it (`md_infer_points_outlier`; with `--views`, `ops.radius_outliers` in front of
`ops.voxel_thin`, over the cloud of all views). Not together with `--mesh`.

`--render-pose E.npy --render-out view.png` (with `--ply`): the cloud is also z-buffered on the device into a virtual camera with the
world-to-camera pose E ([3,4], or [T,3,4] of which every pose is rendered and the first written) and its depth image written as a
normalised PNG, holes black (`md_infer_points_render`; with `--views`, `ops.render_points` on the cloud of all views).
`--render-size H W` (default: the view's size), `--render-radius R` (the (2R+1)^2 pixel footprint of a point),
`--render-intrinsics K.npy` ([3,3]; default: the first view's, scaled to the render size: with `--views` the model's, for one Depth
Pro image `--focal-px`).

`--mesh [--mesh-rtol X]` (with `--ply`): the file also carries the triangle mesh of the depth grid over its points (`element face`),
cut where neighbouring depths differ by more than X of the nearer one (default 0.05; 0 = no cut), computed on the device
(`md_infer_points_mesh`; with `--views`, `ops.unproject(mesh=)`: one mesh per view, not merged). Not together with `--voxel`.

`--decimate V` (with `--ply --mesh`): the mesh is decimated on the device by vertex clustering at voxel side V: one vertex per
occupied voxel (the most confident one), the faces re-indexed, collapsed faces and later copies of a face dropped; the file then
holds the decimated list and faces (`md_infer_points_decimate`; with `--views`, `ops.decimate_mesh` behind the per-view meshes, which
welds the sheets of overlapping views). Not together with `--voxel` or `--outlier-radius`.

`--min-component-faces K` (with `--ply --mesh`): the islands of the mesh leave on the device: the faces of the connected components
with fewer than K faces are dropped (`md_infer_points_components`, so `--raster-pose` sees the filtered faces), and before the file
is written `ops.mesh_components(compact=True)` drops the vertices that only they named, so the file holds no floater; the images of
`--raster-pose` / `--render-pose` stay those of the model call, over its uncompacted list. With `--views`
the operator runs behind the per-view meshes, and behind `ops.decimate_mesh` when `--decimate` is given.

`--planes P [--plane-tol T] [--plane-hypotheses H] [--plane-min-inliers K] [--plane-seed S] [--plane-mode label|drop|keep]
[--plane-up X Y Z --plane-up-cos C]` (with `--ply`): RANSAC extraction of up to P planes from the cloud on the device; the plane equations
n.x n.y n.z d and their inlier counts are printed. `label` writes the plane of every point as the int property `label` of the file (-1 none),
`drop` / `keep` write the cloud without / of the plane points (not with `--mesh`). `--plane-up` keeps only planes whose normal lies within
the cosine C of that axis (the floor with the up axis). One image without `--mesh`: the stage runs inside the model call
(`md_infer_points_planes`); with `--views` or `--mesh`, `ops.fit_planes` runs on the final points. T defaults to 1 % of the cloud's extent.
`--cluster-radius R [--cluster-min-neighbours K] [--cluster-min-points A] [--cluster-max-points B] [--cluster-mode label|keep]` (with
`--ply`): DBSCAN (K = 0: Euclidean cluster extraction) of the cloud on the device, behind `--planes` when both are given, so `--planes P
--plane-mode drop --cluster-radius R` clusters what is not on a plane; the table of kept clusters (size, label, box) is printed. `label`
writes the dense cluster id of every point as the int property `label` of the file (-1 none; it replaces the plane labels), `keep` writes
the points of kept clusters (not with `--mesh`, nor behind `--plane-mode label`). One image without `--mesh` runs inside the model call
(`md_infer_points_clusters`); with `--views` or `--mesh`, `ops.cluster_points` runs on the final points.
`--register-ply REF.ply --register-radius R [--register-iterations K] [--register-apply]` (with `--ply`): rigid point-to-point ICP of
the cloud onto the points of REF.ply, in front of the match step; prints the 4x4 transform, the solves, the pairs and the RMS distance of
the first and the last pass. `--register-apply` writes the aligned cloud, and `--match-ply` / `--cluster-radius` then see it (not with
`--mesh`). One image: the stage of the model call (`md_infer_points_register`); with `--views` or `--mesh`, `ops.register_points` on the
final points. `--register-metric plane` measures every pair along the normal of its reference point (point-to-plane ICP; REF.ply must hold
nx ny nz, as `--normals` writes them) and also prints the status and the RMS point-to-plane residual of the first and the last pass.
`--match-ply REF.ply --match-radius R [--match-tol T ...] [--match-mode label|matched|unmatched]` (with `--ply`): the nearest point of the
reference cloud REF.ply within R for every point of the cloud, on the device, behind `--planes` and in front of `--cluster-radius`, so
`--planes P --plane-mode drop --match-ply REF.ply --match-radius R --match-mode unmatched --cluster-radius C` drops the floor and what the
reference scan already holds and clusters the rest; the counters and, per tolerance T (up to four, each at most R), the precision (points
within T of the reference / all points) are printed. `label` writes "has a counterpart" (1 / 0) as the int property `label` of the file
(`--cluster-radius` replaces it), `matched` / `unmatched` write the points with / without a counterpart (not with `--mesh`, nor behind
`--plane-mode label`, nor `label` in front of `--cluster-mode keep`). One image without `--mesh` runs inside the model call
(`md_infer_points_match`); with `--views` or `--mesh`, `ops.match_points` runs on the final points.
`--smooth ITER [--smooth-step S] [--smooth-lambda L] [--smooth-mu M] [--smooth-free-boundary]` (with `--ply --mesh`): Taubin smoothing
of the mesh on the device, ITER lambda | mu step pairs (`--smooth-mu 0`: ITER Laplacian steps) on an integer lattice of side S, the open
boundary pinned unless freed. The file holds the smoothed positions and, with `--normals`, the vertex normals of the smoothed faces. One
image: the stage runs inside the model call (`md_infer_points_smooth`, so `--raster-pose` draws the smoothed mesh); with `--views`, or
behind `--decimate` / `--min-component-faces`, `ops.smooth_mesh` runs on the final vertices and faces. S defaults to the largest finite
|coordinate| of the list / 2^21, computed on the host (one image: from a first call without the stage).

`--raster-pose E.npy --raster-out view.png` (with `--ply --mesh`): the mesh is also rasterised on the device into a virtual camera with
the world-to-camera pose E ([3,4], or [T,3,4] of which every pose is drawn and the first written), a render without holes, and its
depth image written as a normalised PNG (`md_infer_points_raster`; with `--views`, `ops.render_mesh` on the meshes of all views).
`--render-size` and `--render-intrinsics` apply to it as to `--render-pose`.

`--image`: uint8 RGB [H,W,3] as .npy (JPEG decoding is out of scope). Depth-Anything-v3 inputs are resized on the
shortest side (Catmull-Rom) and centre-cropped to the model resolution (src/model/mod.rs:162-210); the depth map is
restored to the original size, min-max normalised and written as an 8-bit PNG (example/inference.rs:103-199)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def render_request(a, h, w, K=None, focal=None):
    """--render-*: the keywords of a rendering into the pose file's cameras, or a message. K [3,3] / focal: the first view's at h x w."""
    E = np.asarray(np.load(a.render_pose), np.float32)
    if E.shape[-2:] != (3, 4) or E.ndim not in (2, 3):
        return None, f"--render-pose must be [3,4] or [T,3,4], got {E.shape}"
    E = E.reshape(-1, 3, 4)
    H, W = a.render_size or (h, w)
    if a.render_intrinsics:
        K = np.asarray(np.load(a.render_intrinsics), np.float32).reshape(3, 3)
    elif K is not None:
        K = np.asarray(K, np.float32).reshape(3, 3) * np.array([[W / w], [H / h], [1.0]], np.float32)
    elif focal is not None:
        K = np.array([[focal * W / w, 0, W / 2], [0, focal * H / h, H / 2], [0, 0, 1]], np.float32)
    else:
        return None, "--render-pose needs --render-intrinsics (or, for one Depth Pro image, --focal-px)"
    return dict(H=int(H), W=int(W), intrinsics=np.broadcast_to(K, (len(E), 3, 3)).copy(), extrinsics=E, radius=a.render_radius), None


def write_render(a, P, r, path=None) -> None:
    import torch
    torch.cuda.synchronize()
    P.save_depth_map(r.depth[:1].cpu().numpy(), path or a.render_out, None, None)
    print(f"Rendered {int(r.filled[0])} pixels of the first pose to {path or a.render_out}")


def raster_request(a, h, w, K=None, focal=None):
    """--raster-pose: `render_request` on its pose file, without the point footprint"""
    req, why = render_request(argparse.Namespace(**dict(vars(a), render_pose=a.raster_pose)), h, w, K=K, focal=focal)
    if req:
        del req["radius"]
    return req, why


def smooth_step(a, xyz) -> float:
    """--smooth-step, or the default lattice side: the largest finite |coordinate| of the list over 2^21"""
    if a.smooth_step > 0:
        return a.smooth_step
    import torch
    v = xyz.abs()
    v = v[torch.isfinite(v)]
    top = float(v.max().item()) if v.numel() else 0.0
    return float(np.float32(top / 2097152.0)) if top > 0 else 1.0


def planes_request(a, xyz) -> dict:
    """the planes= keywords of --planes; without --plane-tol the tolerance is 1 % of the largest finite extent of the list"""
    tol = a.plane_tol
    if not tol > 0:
        fin = xyz[xyz.isfinite().all(1)]
        tol = 0.01 * float((fin.max(0).values - fin.min(0).values).max()) if len(fin) else 1.0
    up = dict(axis=tuple(a.plane_up), axis_min_cos=a.plane_up_cos) if a.plane_up else {}
    return dict(planes=a.planes, hypotheses=a.plane_hypotheses, tol=tol, min_inliers=a.plane_min_inliers, seed=a.plane_seed, mode=a.plane_mode, **up)


CLUSTER_TABLE = 256  # rows of the printed table


def clusters_request(a) -> dict:
    """the clusters= keywords of --cluster-radius"""
    return dict(radius=a.cluster_radius, min_neighbours=a.cluster_min_neighbours, min_points=a.cluster_min_points,
                max_points=a.cluster_max_points, mode=a.cluster_mode, table=CLUSTER_TABLE)


def print_clusters(found) -> None:
    stats = found.stats.cpu().tolist()
    rows = min(stats[1], int(found.table_label.shape[0]))
    for i, (l, n, b) in enumerate(zip(found.table_label[:rows].cpu().tolist(), found.table_size[:rows].cpu().tolist(), found.box[:rows].cpu().tolist())):
        print(f"Cluster {i}: {n} points, label {l}, box {b[0]:.6g} {b[1]:.6g} {b[2]:.6g} .. {b[3]:.6g} {b[4]:.6g} {b[5]:.6g}")
    print(f"Clusters: {stats[0]} found, {stats[1]} kept, {stats[2]} noise points, {stats[3]} points in kept clusters")


def match_request(a, dev) -> dict:
    """the match= keywords of --match-ply: the reference cloud goes to the device once"""
    import torch
    from burn_depth_amd import pipeline as P
    ref = np.ascontiguousarray(P.read_ply(a.match_ply)[0], dtype=np.float32)
    return dict(target=torch.from_numpy(ref).to(dev), radius=a.match_radius, tol=tuple(a.match_tol), mode=a.match_mode)


def register_request(a, dev) -> dict:
    """the register= keywords of --register-ply: the reference cloud goes to the device once"""
    import torch
    from burn_depth_amd import pipeline as P
    if a.register_metric == "plane":  # the normals of the file, which main() has seen to be there
        ref, _, nrm = P.read_ply_normals(a.register_ply)
        return dict(target=torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(dev), radius=a.register_radius,
                    iterations=a.register_iterations, target_normals=torch.from_numpy(np.ascontiguousarray(nrm, dtype=np.float32)).to(dev))
    ref = np.ascontiguousarray(P.read_ply(a.register_ply)[0], dtype=np.float32)
    return dict(target=torch.from_numpy(ref).to(dev), radius=a.register_radius, iterations=a.register_iterations)


def print_registration(found) -> None:
    """the 4x4 of the transform, then the pairs and the RMS distance of the first and of the evaluation pass"""
    stats, pairs, sums = found.stats.cpu().tolist(), found.pairs.cpu().tolist(), found.sum_d2.cpu().tolist()
    print("Registration:")
    for row in found.matrix().tolist():
        print("  " + " ".join(f"{v:+.9e}" for v in row))
    rms = lambda k: (sums[k] / pairs[k]) ** 0.5 if pairs[k] else float("nan")  # noqa: E731
    state = {0: "ran every round", 1: "converged", 2: "too few pairs", 3: "degenerate system"}[stats[1]]
    print(f"Registration: {stats[0]} solves ({state}), {pairs[0]} -> {pairs[-1]} pairs, RMS distance {rms(0):.6g} -> {rms(-1):.6g}, "
          f"{stats[4]} reference points in the grid")
    if found.sum_r2 is not None:  # --register-metric plane: the pairs above are the usable ones
        r2 = found.sum_r2.cpu().tolist()
        res = lambda k: (r2[k] / pairs[k]) ** 0.5 if pairs[k] else float("nan")  # noqa: E731
        print(f"Registration (plane): status {stats[1]}, RMS point-to-plane residual {res(0):.6g} -> {res(-1):.6g}")


def print_match(found, a, rows: int) -> None:
    stats = found.stats.cpu().tolist()
    print(f"Match: {stats[0]} points in range, {stats[1]} with a counterpart within {a.match_radius:.6g}, {stats[2]} reference points in the grid")
    for t, tol in enumerate(a.match_tol):
        print(f"Precision at {tol:.6g}: {stats[4 + t] / rows if rows else 0.0:.6f} ({stats[4 + t]} of {rows} points)")


def print_planes(fitted) -> None:
    found = int(fitted.plane_count[-1])
    for i, (w, c) in enumerate(zip(fitted.plane[:found].cpu().tolist(), fitted.plane_count[:found].cpu().tolist())):
        print(f"Plane {i}: {w[0]:+.6f} x {w[1]:+.6f} y {w[2]:+.6f} z {w[3]:+.6f} = 0  ({c} inliers)")
    if not found:
        print("No plane found")


def smooth_request(a, step: float) -> dict:
    return dict(step=step, iterations=a.smooth, lam=a.smooth_lambda, mu=a.smooth_mu, pin_boundary=not a.smooth_free_boundary, normals=a.normals)


def run_views(a) -> int:
    """--views: one scene through `infer_views`; depth PNGs per view, and with --ply one filtered world-space cloud."""
    import torch
    from burn_depth_amd import _lib, ops
    from burn_depth_amd import pipeline as P
    from burn_depth_amd.config import Precision
    from burn_depth_amd.depth_pro import Device
    from burn_depth_amd.inference import rgb_to_input_tensor
    if a.model != "depth-anything-3":
        print("--views applies to Depth-Anything-v3 `small`", file=sys.stderr)
        return 2
    imgs = [np.load(v) for v in a.views]
    for v, im in zip(a.views, imgs):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            print(f"{v}: expected uint8 [H,W,3], got {im.dtype} {im.shape}", file=sys.stderr)
            return 2
    dev = Device(0)
    try:
        model = P.AnyDepthModel.load(P.DepthModelKind(a.model), dev, a.checkpoint, Precision.BF16 if a.precision == "bf16" else Precision.F32, max_batch=len(imgs))
    except RuntimeError as e:
        print(str(e), file=sys.stderr)
        return 1
    preps = [model.prepare_input_image(im) for im in imgs]
    if len({(p.width, p.height) for p in preps}) != 1:
        print("--views: the prepared views must share one size", file=sys.stderr)
        return 2
    x = torch.stack([rgb_to_input_tensor(p.rgb.tobytes(), p.width, p.height, dev)[0] for p in preps])[None]  # [1, V, 3, H, W]
    try:
        out = model.infer_views(x)
    except _lib.MdError as e:
        print(str(e), file=sys.stderr)
        return 1
    base = a.output or os.path.join(os.path.dirname(os.path.abspath(a.views[0])), "depth.png")
    stem, ext = os.path.splitext(base)
    for i, (im, p) in enumerate(zip(imgs, preps)):
        oh, ow = im.shape[:2]
        restore = (ow, oh) if (p.width != ow or p.height != oh or p.crop is not None) else None
        P.save_depth_map(out.depth[i:i + 1].cpu().numpy(), f"{stem}_v{i}{ext}", p.crop, restore)
    print(f"Model `{a.model}` wrote {len(imgs)} normalized depth maps to {stem}_v*{ext}")
    if a.ply:
        K, E = out.intrinsics[:, 0], out.extrinsics[:, 0]
        depth = out.depth
        if a.view_rtol > 0 or a.conf_percentile > 0:
            depth, _, _, _ = ops.filter_views(dev, out.depth, out.depth_confidence, intrinsics=K, extrinsics=E, conf_percentile=a.conf_percentile,
                                              view_rtol=a.view_rtol, min_views=a.min_views)
        rgb = torch.from_numpy(np.stack([p.rgb for p in preps])).to(depth.device)
        pc = ops.unproject(dev, depth, intrinsics=K, extrinsics=E, conf=out.depth_confidence, rgb=rgb, dense=False, conf_min=a.conf_min,
                           edge_rtol=a.edge_rtol, stride=a.stride, world=True, normals=a.normals, normal_min_cos=a.normal_min_cos,
                           mesh=dict(max_rtol=a.mesh_rtol, pixel_index=False) if a.mesh else None)
        faces = pc.faces[:int(pc.face_count[-1])].cpu().numpy() if a.mesh else None
        xyz, col, conf = pc.points()
        nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.outlier_radius > 0:  # the points without enough neighbours over all views leave first
            try:
                pc = ops.radius_outliers(dev, xyz, a.outlier_radius, a.outlier_min, conf=conf, rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            xyz, col, conf = pc.points()
            nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.decimate > 0:  # vertex clustering over the meshes of all views: the sheets are welded where they share a voxel
            try:
                pc = ops.decimate_mesh(dev, xyz, pc.faces[:len(faces)], a.decimate, conf=conf, rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            faces = pc.faces[:int(pc.face_count[-1])].cpu().numpy()
            xyz, col, _ = pc.points()
            nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.min_component_faces > 0:  # the islands of the (decimated) mesh leave, and the vertices only they named with them
            try:
                pc = ops.mesh_components(dev, pc.faces[:len(faces)], int(xyz.shape[0]), a.min_component_faces, xyz=xyz, rgb=col, normals=nrm,
                                         compact=True)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            faces = pc.faces[:int(pc.face_count[-1])].cpu().numpy()
            xyz, col, _ = pc.points()
            nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.smooth > 0:  # the final vertices move; the faces, the colours and the row order stay
            try:
                sm = ops.smooth_mesh(dev, xyz, pc.faces[:len(faces)], **smooth_request(a, smooth_step(a, xyz)))
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            xyz, nrm = sm.xyz, sm.normals
        if a.voxel > 0:  # one point per occupied voxel over all views: the most confident one
            try:
                pc = ops.voxel_thin(dev, xyz, a.voxel, conf=conf, rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            xyz, col, _ = pc.points()
            nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        label = None
        if a.planes > 0:  # on the points of the file
            try:
                pc = ops.fit_planes(dev, xyz, **planes_request(a, xyz), rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            print_planes(pc.planes)
            if a.plane_mode == "label":
                label = pc.planes.label.cpu().numpy()
                pc.xyz, pc.rgb, pc.count = xyz, col, torch.tensor([xyz.shape[0]], dtype=torch.int32, device=xyz.device)  # what --render-pose draws
            else:
                xyz, col, _ = pc.points()
                nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.register_ply:  # on the points the plane step left, in front of the match step
            try:
                req = register_request(a, xyz.device)
                found = ops.register_points(dev, xyz, req.pop("target"), **req, normals=nrm, apply=a.register_apply)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            print_registration(found)
            if a.register_apply:  # the file, the later steps and --render-pose see the aligned cloud
                xyz, nrm = found.xyz, found.normals if a.normals else None
                pc.xyz, pc.rgb, pc.count = xyz, col, torch.tensor([xyz.shape[0]], dtype=torch.int32, device=xyz.device)
        if a.match_ply:  # on the points the register step left
            try:
                req = match_request(a, xyz.device)
                pc = ops.match_points(dev, xyz, req.pop("target"), **req, rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            print_match(pc.match, a, int(xyz.shape[0]))
            if a.match_mode == "label":
                label = (pc.match.nearest >= 0).to(torch.int32).cpu().numpy()
                pc.xyz, pc.rgb, pc.count = xyz, col, torch.tensor([xyz.shape[0]], dtype=torch.int32, device=xyz.device)  # what --render-pose draws
            else:
                xyz, col, _ = pc.points()
                nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        if a.cluster_radius > 0:  # on the points the match step left
            try:
                pc = ops.cluster_points(dev, xyz, **clusters_request(a), rgb=col, normals=nrm)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
            print_clusters(pc.clusters)
            if a.cluster_mode == "label":
                label = pc.clusters.cluster.cpu().numpy()
                pc.xyz, pc.rgb, pc.count = xyz, col, torch.tensor([xyz.shape[0]], dtype=torch.int32, device=xyz.device)  # what --render-pose draws
            else:
                xyz, col, _ = pc.points()
                nrm = pc.normals[:xyz.shape[0]] if a.normals else None
        P.write_ply(a.ply, xyz.cpu().numpy(), col.cpu().numpy(), nrm.cpu().numpy() if a.normals else None, faces=faces, label=label)
        print(f"Model `{a.model}` wrote {xyz.shape[0]} points{f' and {len(faces)} faces' if a.mesh else ''} of {len(imgs)} views to {a.ply}")
        if a.render_pose:
            req, why = render_request(a, preps[0].height, preps[0].width, K=K[0].cpu().numpy())
            if why:
                print(why, file=sys.stderr)
                return 2
            try:
                write_render(a, P, ops.render_points(dev, pc.xyz, req.pop("H"), req.pop("W"), rgb=pc.rgb, count=pc.count[-1:], **req))
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
        if a.raster_pose:
            req, why = raster_request(a, preps[0].height, preps[0].width, K=K[0].cpu().numpy())
            if why:
                print(why, file=sys.stderr)
                return 2
            if a.voxel > 0:
                print("--raster-pose with --views takes no --voxel (the faces name rows of the unthinned list)", file=sys.stderr)
                return 2
            try:
                r = ops.render_mesh(dev, pc.xyz, pc.faces, req.pop("H"), req.pop("W"), rgb=pc.rgb, face_count=pc.face_count[-1:], **req)
                write_render(a, P, r, a.raster_out)
            except _lib.MdError as e:
                print(str(e), file=sys.stderr)
                return 1
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["depth-pro", "depth-anything-3"], default="depth-pro")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--image", default="")
    ap.add_argument("--views", nargs="+", default=[], help="the views of one scene, reference view first (Depth-Anything-v3 small; instead of --image)")
    ap.add_argument("--view-rtol", type=float, default=0.0, help="--views --ply: drop a pixel that other views contradict by more than this ratio (0 = off)")
    ap.add_argument("--min-views", type=int, default=0, help="--views --ply: keep pixels that at least this many other views support")
    ap.add_argument("--output", default="")
    ap.add_argument("--precision", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--focal-px", type=float, default=None, help="known focal length in pixels of the image (Depth Pro only)")
    ap.add_argument("--on-device", action="store_true", help="prepare, infer and build the PNG's pixels in one device call (md_process_frame)")
    ap.add_argument("--ply", default="", help="write the point cloud of the prepared image to this .ply (md_infer_points)")
    ap.add_argument("--conf-min", type=float, default=0.0, help="--ply: keep pixels whose confidence is at least this (Depth-Anything-v3 small)")
    ap.add_argument("--conf-percentile", type=int, default=0, help="--ply: drop the lowest this-many percent (0..99) of the confidences (Depth-Anything-v3 small)")
    ap.add_argument("--edge-rtol", type=float, default=0.0, help="--ply: drop pixels whose depth differs from a neighbour's by more than this ratio (0 = off)")
    ap.add_argument("--stride", type=int, default=1, help="--ply: keep every stride-th row and column")
    ap.add_argument("--normals", action="store_true", help="--ply: also write the surface normals (nx ny nz; md_infer_points_normals)")
    ap.add_argument("--normal-min-cos", type=float, default=0.0,
                    help="--ply: drop pixels whose surface is seen at a cosine below this (grazing angles; 0 = off, at most 1)")
    ap.add_argument("--voxel", type=float, default=0.0,
                    help="--ply: keep one point per occupied voxel of this side, the most confident one (md_infer_points_voxel; 0 = off)")
    ap.add_argument("--outlier-radius", type=float, default=0.0,
                    help="--ply: drop the points with fewer than --outlier-min others within this radius (md_infer_points_outlier; 0 = off)")
    ap.add_argument("--outlier-min", type=int, default=8, help="--outlier-radius: the neighbours a point needs to stay")
    ap.add_argument("--render-pose", default="", help="--ply: also render the cloud into the world-to-camera pose(s) of this .npy ([3,4] or [T,3,4])")
    ap.add_argument("--render-size", type=int, nargs=2, metavar=("H", "W"), default=None, help="--render-pose: image size (default: the view's)")
    ap.add_argument("--render-radius", type=int, default=0, help="--render-pose: a point covers the (2R+1)^2 pixels around its pixel")
    ap.add_argument("--render-intrinsics", default="", help="--render-pose: [3,3] .npy (default: the first view's, scaled to the render size)")
    ap.add_argument("--render-out", default="", help="--render-pose: the rendered depth of the first pose as a normalised PNG")
    ap.add_argument("--mesh", action="store_true", help="--ply: also write the triangle mesh of the depth grid over the points (md_infer_points_mesh)")
    ap.add_argument("--mesh-rtol", type=float, default=0.05,
                    help="--mesh: cut an edge whose depths differ by more than this fraction of the nearer one (0 = no cut)")
    ap.add_argument("--decimate", type=float, default=0.0,
                    help="--ply --mesh: vertex-clustering decimation at this voxel side: one vertex per voxel, collapsed and doubled faces dropped "
                         "(md_infer_points_decimate; 0 = off)")
    ap.add_argument("--min-component-faces", type=int, default=0,
                    help="--ply --mesh: drop the connected components of the mesh with fewer faces than this, and the vertices only they "
                         "named (md_infer_points_components, ops.mesh_components; 0 = off)")
    ap.add_argument("--smooth", type=int, default=0,
                    help="--ply --mesh: Taubin smoothing of the mesh, this many lambda | mu step pairs (md_infer_points_smooth, ops.smooth_mesh; 0 = off)")
    ap.add_argument("--smooth-step", type=float, default=0.0, help="--smooth: the lattice side (0 = the largest finite |coordinate| of the list / 2^21)")
    ap.add_argument("--smooth-lambda", type=float, default=0.5, help="--smooth: the factor of the shrinking steps, in (0, 1]")
    ap.add_argument("--smooth-mu", type=float, default=-0.53, help="--smooth: the factor of the inflating steps, in [-1, 0]; 0 = Laplacian smoothing")
    ap.add_argument("--smooth-free-boundary", action="store_true", help="--smooth: let the open boundary of the mesh move too")
    ap.add_argument("--planes", type=int, default=0, help="--ply: extract up to this many planes (1..8) from the cloud (md_infer_points_planes, ops.fit_planes; 0 = off)")
    ap.add_argument("--plane-tol", type=float, default=0.0, help="--planes: the inlier distance (0 = 1 %% of the cloud's extent)")
    ap.add_argument("--plane-hypotheses", type=int, default=1024, help="--planes: three-point hypotheses per plane, 1..4096")
    ap.add_argument("--plane-min-inliers", type=int, default=100, help="--planes: the inliers a plane needs, at least 3")
    ap.add_argument("--plane-seed", type=int, default=0, help="--planes: the seed of the samples")
    ap.add_argument("--plane-mode", choices=["label", "drop", "keep"], default="label",
                    help="--planes: write the plane of every point as the PLY property `label`, or the cloud without / of the plane points")
    ap.add_argument("--cluster-radius", type=float, default=0.0, help="--ply: DBSCAN of the cloud with this neighbour radius (md_infer_points_clusters, ops.cluster_points; 0 = off)")
    ap.add_argument("--cluster-min-neighbours", type=int, default=0, help="--cluster-radius: the neighbours a core point needs, 0..2^20 (0 = Euclidean cluster extraction)")
    ap.add_argument("--cluster-min-points", type=int, default=1, help="--cluster-radius: the points a kept cluster has at least")
    ap.add_argument("--cluster-max-points", type=int, default=0, help="--cluster-radius: the points a kept cluster has at most (0 = no limit)")
    ap.add_argument("--cluster-mode", choices=["label", "keep"], default="label",
                    help="--cluster-radius: write the dense cluster id of every point as the PLY property `label`, or the points of kept clusters")
    ap.add_argument("--match-ply", default="", help="--ply: match the cloud against the points of this reference .ply (md_infer_points_match, ops.match_points)")
    ap.add_argument("--match-radius", type=float, default=0.0, help="--match-ply: the search radius, > 0")
    ap.add_argument("--match-tol", type=float, nargs="+", default=[], metavar="T", help="--match-ply: up to four tolerances in (0, radius] whose precision is printed")
    ap.add_argument("--match-mode", choices=["label", "matched", "unmatched"], default="label",
                    help="--match-ply: write `has a counterpart` as the PLY property `label`, or the points with / without a counterpart")
    ap.add_argument("--register-ply", default="", help="--ply: rigid ICP of the cloud onto the points of this reference .ply, in front of --match-ply "
                    "(md_infer_points_register, ops.register_points); prints the 4x4 transform")
    ap.add_argument("--register-radius", type=float, default=0.0, help="--register-ply: the pairing radius, > 0")
    ap.add_argument("--register-iterations", type=int, default=10, help="--register-ply: the rounds, 1..64")
    ap.add_argument("--register-metric", choices=["point", "plane"], default="point", help="--register-ply: plane measures a pair along the normal of its "
                    "reference point (nx ny nz of REF.ply, which must hold them; md_infer_points_register_plane)")
    ap.add_argument("--register-apply", action="store_true", help="--register-ply: write the aligned cloud; the match and cluster steps see it (not with --mesh)")
    ap.add_argument("--plane-up", type=float, nargs=3, metavar=("X", "Y", "Z"), help="--planes: only planes whose normal lies within --plane-up-cos of this axis")
    ap.add_argument("--plane-up-cos", type=float, default=0.9, help="--plane-up: the smallest |cosine| between a plane's normal and the axis")
    ap.add_argument("--raster-pose", default="", help="--ply --mesh: also rasterise the mesh into the world-to-camera pose(s) of this .npy ([3,4] or [T,3,4])")
    ap.add_argument("--raster-out", default="", help="--raster-pose: the rasterised depth of the first pose as a normalised PNG")
    a = ap.parse_args(argv)
    if bool(a.raster_pose) != bool(a.raster_out) or (a.raster_pose and not (a.ply and a.mesh)):
        print("--raster-pose and --raster-out go together, and with --ply --mesh", file=sys.stderr)
        return 2
    if a.mesh and (not a.ply or a.voxel > 0):
        print("--mesh goes with --ply, and not with --voxel (a thinned list has no grid)", file=sys.stderr)
        return 2
    if a.decimate != 0 and (not (a.ply and a.mesh) or a.voxel > 0 or a.outlier_radius != 0):
        print("--decimate goes with --ply --mesh, and not with --voxel or --outlier-radius (the decimation is the thinning)", file=sys.stderr)
        return 2
    if a.min_component_faces != 0 and (a.min_component_faces < 0 or not (a.ply and a.mesh)):
        print("--min-component-faces is a positive face count and goes with --ply --mesh", file=sys.stderr)
        return 2
    if a.smooth != 0 and (not 1 <= a.smooth <= 1024 or not (a.ply and a.mesh)):
        print("--smooth is a step count in 1..1024 and goes with --ply --mesh", file=sys.stderr)
        return 2
    if a.cluster_radius != 0 and (not a.cluster_radius > 0 or not a.ply or (a.cluster_mode == "keep" and (a.mesh or (a.planes and a.plane_mode == "label")))):
        print("--cluster-radius is > 0 and goes with --ply; --cluster-mode keep not with --mesh (the faces name the rows) nor behind --plane-mode label",
              file=sys.stderr)
        return 2
    if a.match_ply and (not a.match_radius > 0 or not a.ply or len(a.match_tol) > 4 or
                        (a.match_mode != "label" and (a.mesh or (a.planes and a.plane_mode == "label"))) or
                        (a.match_mode == "label" and a.cluster_radius > 0 and a.cluster_mode == "keep")):
        print("--match-ply goes with --ply and --match-radius > 0 and takes at most four --match-tol; --match-mode matched / unmatched not with --mesh "
              "(the faces name the rows) nor behind --plane-mode label; --match-mode label not in front of --cluster-mode keep", file=sys.stderr)
        return 2
    if a.register_ply and (not a.register_radius > 0 or not a.ply or not 1 <= a.register_iterations <= 64 or (a.register_apply and a.mesh)):
        print("--register-ply goes with --ply, --register-radius > 0 and --register-iterations in 1..64; --register-apply not with --mesh "
              "(the faces and the smoothed rows belong to the cloud before it moved)", file=sys.stderr)
        return 2
    if a.register_apply and not a.register_ply:
        print("--register-apply goes with --register-ply", file=sys.stderr)
        return 2
    if a.register_metric == "plane":
        from burn_depth_amd import pipeline as P
        if not a.register_ply or (os.path.exists(a.register_ply) and P.read_ply_normals(a.register_ply)[2] is None):
            print("--register-metric plane goes with --register-ply REF.ply, and REF.ply holds the normals nx ny nz", file=sys.stderr)
            return 2
    if a.planes != 0 and (not 1 <= a.planes <= 8 or not a.ply or (a.mesh and a.plane_mode != "label")):
        print("--planes is a plane count in 1..8 and goes with --ply; --plane-mode drop / keep not with --mesh (the faces name the rows)", file=sys.stderr)
        return 2
    if a.outlier_radius != 0 and (not a.ply or a.mesh):
        print("--outlier-radius goes with --ply, and not with --mesh (the faces name rows of the unfiltered list)", file=sys.stderr)
        return 2
    if bool(a.render_pose) != bool(a.render_out) or (a.render_pose and not a.ply):
        print("--render-pose and --render-out go together, and with --ply", file=sys.stderr)
        return 2
    if a.focal_px is not None and a.model != "depth-pro":
        print(f"--focal-px applies to Depth Pro only, not to `{a.model}`", file=sys.stderr)
        return 2
    if a.focal_px is not None and not (np.isfinite(a.focal_px) and a.focal_px > 0):
        print(f"--focal-px must be a finite focal length > 0, got {a.focal_px}", file=sys.stderr)
        return 2
    from burn_depth_amd import pipeline as P
    from burn_depth_amd.config import Precision
    from burn_depth_amd.depth_pro import Device
    if not os.path.exists(a.checkpoint):   # example/inference.rs:52-62
        print(f"Checkpoint `{a.checkpoint}` not found. Run tools/import_weights.py first.", file=sys.stderr)
        return 1
    if bool(a.image) == bool(a.views):
        print("give either --image or --views", file=sys.stderr)
        return 2
    if a.views:
        return run_views(a)
    rgb = np.load(a.image)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        print(f"--image must be uint8 [H,W,3], got {rgb.dtype} {rgb.shape}", file=sys.stderr)
        return 2
    kind = P.DepthModelKind(a.model)
    try:
        model = P.AnyDepthModel.load(kind, Device(0), a.checkpoint, Precision.BF16 if a.precision == "bf16" else Precision.F32)
    except RuntimeError as e:
        print(str(e), file=sys.stderr)
        return 1
    if a.on_device and a.focal_px is not None:
        print("--on-device takes no --focal-px (the frame call predicts the focal length)", file=sys.stderr)
        return 2
    if a.ply:
        import torch
        from burn_depth_amd import _lib, ops
        from burn_depth_amd.inference import rgb_to_input_tensor
        prep = model.prepare_input_image(rgb)
        x = rgb_to_input_tensor(prep.rgb.tobytes(), prep.width, prep.height, model.model.device)
        render = None
        if a.render_pose:
            render, why = render_request(a, prep.height, prep.width, focal=a.focal_px)
            if why:
                print(why, file=sys.stderr)
                return 2
        raster = None
        if a.raster_pose:
            raster, why = raster_request(a, prep.height, prep.width, focal=a.focal_px)
            if why:
                print(why, file=sys.stderr)
                return 2
        in_call = bool(a.smooth) and not a.decimate and not a.min_component_faces  # the stage of the model call; else the operator below
        try:
            call = dict(**({"f_px": a.focal_px} if a.focal_px is not None else {}), rgb=torch.from_numpy(prep.rgb[None]),
                        dense=False, conf_min=a.conf_min, conf_percentile=a.conf_percentile, edge_rtol=a.edge_rtol, stride=a.stride,
                        world=bool(getattr(model.model.config, "dual_head", False)), normals=a.normals, normal_min_cos=a.normal_min_cos)
            smooth = None
            if in_call:  # without --smooth-step a first call gives the list, whose extent sets the lattice
                smooth = smooth_request(a, a.smooth_step if a.smooth_step > 0 else smooth_step(a, model.infer_points(x, **call).points()[0]))
            pc = model.infer_points(x, **call, voxel=a.voxel, render=render,
                                    mesh=dict(max_rtol=a.mesh_rtol, pixel_index=False) if a.mesh else None, raster=raster,
                                    outlier=dict(radius=a.outlier_radius, min_neighbours=a.outlier_min) if a.outlier_radius else None,
                                    decimate=dict(voxel=a.decimate) if a.decimate else None,
                                    components=dict(min_faces=a.min_component_faces) if a.min_component_faces and not a.decimate else None,
                                    smooth=smooth)
            planes_in_call = bool(a.planes) and not a.mesh
            clusters_in_call = a.cluster_radius > 0 and not a.mesh
            match_in_call = bool(a.match_ply) and not a.mesh
            register_in_call = bool(a.register_ply) and not a.mesh
            if planes_in_call or clusters_in_call or match_in_call or register_in_call:  # a first call gives the list, whose extent sets the default tolerance; the stages then run inside the call
                pc = model.infer_points(x, **call, voxel=a.voxel, render=render, planes=planes_request(a, pc.points()[0]) if planes_in_call else None,
                                        clusters=clusters_request(a) if clusters_in_call else None,
                                        match=match_request(a, x.device) if match_in_call else None,
                                        register=dict(register_request(a, x.device), apply=a.register_apply) if register_in_call else None,
                                        outlier=dict(radius=a.outlier_radius, min_neighbours=a.outlier_min) if a.outlier_radius else None)
            xyz, col, _ = pc.points()
            nrm = pc.normals[:xyz.shape[0]] if a.normals else None
            if in_call:
                xyz = pc.smooth.xyz[:xyz.shape[0]]
                nrm = pc.smooth.normals[:xyz.shape[0]] if a.normals else None
            flt = pc  # what the file holds; `pc` stays the model call's result, whose images are written below
            if a.min_component_faces:  # the file holds no floater vertex: the list is compacted to the rows the kept faces name
                flt = ops.mesh_components(Device(0), pc.faces[:int(pc.face_count[-1])], int(xyz.shape[0]), a.min_component_faces, xyz=xyz,
                                          rgb=col, normals=nrm, compact=True)
                xyz, col, _ = flt.points()
                nrm = flt.normals[:xyz.shape[0]] if a.normals else None
            if a.smooth and not in_call:  # behind the decimation / the compaction: the operator on the vertices and faces of the file
                sm = ops.smooth_mesh(Device(0), xyz, flt.faces[:int(flt.face_count[-1])], **smooth_request(a, smooth_step(a, xyz)))
                xyz, nrm = sm.xyz, sm.normals
            label = None
            if a.planes:  # beside a mesh: the operator labels the vertices of the file
                fitted = pc.planes if planes_in_call else ops.fit_planes(Device(0), xyz, **planes_request(a, xyz)).planes
                print_planes(fitted)
                if a.plane_mode == "label":
                    label = fitted.label[:xyz.shape[0]].cpu().numpy()
            if a.register_ply:  # beside a mesh: the operator estimates on the vertices of the file, which stay
                if register_in_call:
                    print_registration(pc.registration)
                else:
                    req = register_request(a, xyz.device)
                    print_registration(ops.register_points(Device(0), xyz, req.pop("target"), **req))
            if a.match_ply:  # beside a mesh: the operator labels the vertices of the file
                if match_in_call:
                    near = pc.match
                else:
                    req = match_request(a, xyz.device)
                    near = ops.match_points(Device(0), xyz, req.pop("target"), **req).match
                rows = int(near.stats[0] + near.dropped[0]) if match_in_call else int(xyz.shape[0])  # the rows the stage read
                print_match(near, a, rows)
                if a.match_mode == "label":
                    label = (near.nearest[:xyz.shape[0]] >= 0).to(torch.int32).cpu().numpy()
            if a.cluster_radius > 0:  # beside a mesh: the operator labels the vertices of the file
                found = pc.clusters if clusters_in_call else ops.cluster_points(Device(0), xyz, **clusters_request(a)).clusters
                print_clusters(found)
                if a.cluster_mode == "label":
                    label = found.cluster[:xyz.shape[0]].cpu().numpy()
        except _lib.MdError as e:
            print(str(e), file=sys.stderr)
            return 1
        faces = flt.faces[:int(flt.face_count[-1])].cpu().numpy() if a.mesh else None
        P.write_ply(a.ply, xyz.cpu().numpy(), col.cpu().numpy(), nrm.cpu().numpy() if a.normals else None, faces=faces, label=label)
        print(f"Model `{kind.value}` wrote {xyz.shape[0]} points{f' and {len(faces)} faces' if a.mesh else ''} to {a.ply}")
        if render is not None:
            write_render(a, P, pc.render)
        if raster is not None:
            write_render(a, P, pc.raster, a.raster_out)
        if not a.output:
            return 0
    oh, ow = rgb.shape[:2]
    path = a.output or os.path.join(os.path.dirname(os.path.abspath(a.image)), "depth.png")
    if a.on_device:
        fr = model.model.process_frame(rgb, target=0, restore=True, normalize=True, fmt="u8", prepared=False)
        P.write_gray_png(path, fr.display[0].cpu().numpy())
        f, fy = fr.focallength_px, fr.fovy_rad
        print(f"Focal length (px): {f.cpu().tolist() if f is not None else 'not provided by this model'}")
        print(f"Vertical FOV (rad): {fy.cpu().tolist() if fy is not None else 'not provided by this model'}")
        print(f"Model `{kind.value}` wrote normalized depth map to {path}")
        return 0
    prep = model.prepare_input_image(rgb)
    out = model.infer_from_rgb(prep, a.focal_px)
    restore = (ow, oh) if (prep.width != ow or prep.height != oh or prep.crop is not None) else None
    P.save_depth_map(out.depth.cpu().numpy(), path, prep.crop, restore)
    f = getattr(out, "focallength_px", None)
    print(f"Focal length (px): {f.cpu().tolist() if f is not None else 'not provided by this model'}")
    fy = getattr(out, "fovy_rad", None)
    print(f"Vertical FOV (rad): {fy.cpu().tolist() if fy is not None else 'not provided by this model'}")
    print(f"Model `{kind.value}` wrote normalized depth map to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
