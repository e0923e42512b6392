"""Host-side pre/post-processing either side of the hot path, mirroring the reference's CLI flow
`example/inference.rs`: AnyDepthModel::load -> prepare_input_image -> infer_from_rgb -> save_depth_map.

* `AnyDepthModel` / `DepthModelKind`           -- src/model/mod.rs:17-142
* `prepare_depth_anything3_image`             -- src/model/mod.rs:162-210 (shortest-side resize + centre crop). The
  resize itself is `image::imageops::resize(.., FilterType::CatmullRom)` from the un-vendored `image` crate: its
  separable resampler is restated here from the crate's published algorithm (**parity unpinned**: no value-level
  test of the reference touches it).
* `crop_depth_field`, `resize_depth_field`, `sample_depth_bilinear`, the min-max normalisation of `save_depth_map`
                                              -- example/inference.rs:103-273 (restated exactly, fp32)
* `prepare_input_frame`, `depth_to_display`   -- the viewer's frame path (crates/bevy_burn_depth/src/lib.rs:16-132): the host
  references of the device frame call `md_process_frame` (`DepthPro.process_frame`)
* `unproject_depth`, `write_ply` / `read_ply`  -- the point path (no counterpart in the reference): the host reference the
  device kernels of `md_op_unproject` / `md_infer_points` are bit-identical to, and a binary little-endian PLY writer / reader
* `filter_views`                              -- the host reference of `md_op_filter_views` / `md_infer_points_filtered`: the exact
  confidence percentile and the cross-view support test in front of the point path
* `pixel_index`, `mesh_grid`                  -- the host reference of `md_op_mesh_grid` / `md_infer_points_mesh`: the map pixel -> list
  row and the triangle mesh of the depth grid over the list's rows, bit-identical to the device's
* `render_points`                             -- the host reference of `md_op_render_points` / `md_infer_points_render`: the cloud
  z-buffered into target cameras on 64-bit keys
* `render_mesh`                               -- the host reference of `md_op_render_mesh` / `md_infer_points_raster`: the faces of the
  mesh rasterised into target cameras, integer coverage at 1/256 pixel and 64-bit keys
* `decimate_mesh`                             -- the host reference of `md_op_decimate_mesh`: voxel thinning's vertices, the faces
  re-indexed to them, collapsed faces and later copies of an oriented triangle dropped
* `mesh_components`                           -- the host reference of `md_op_mesh_components` / `md_infer_points_components`: the
  connected components of the faces (the smallest row of each as its label) and the faces of those with enough faces
* `smooth_mesh`                               -- the host reference of `md_op_smooth_mesh` / `md_infer_points_smooth`: Taubin /
  Laplacian smoothing on an integer lattice with int64 sums, and the area-weighted vertex normals of the smoothed faces
* `radius_outliers`                           -- the host reference of `md_op_radius_outliers` / `md_infer_points_outlier`: the rows
  with enough neighbours in the 27 cells around their own, bit-identical to the device's
* `write_gray_png`                            -- the reference uses `image::GrayImage::save`; a stdlib-zlib PNG writer
  stands in (8-bit grayscale, filter 0), `read_gray_png` reads it back for the tests.
JPEG decoding stays out of scope: images come in as uint8 arrays."""
from __future__ import annotations

import enum
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

f32 = np.float32


class DepthModelKind(enum.Enum):
    DEPTH_PRO = "depth-pro"            # src/model/mod.rs:31-36 (`as_str`)
    DEPTH_ANYTHING3 = "depth-anything-3"


@dataclass
class ImageCropRegion:
    x: int
    y: int
    width: int
    height: int


@dataclass
class PreparedModelImage:
    width: int
    height: int
    rgb: np.ndarray                    # uint8 [H, W, 3]
    crop: Optional[ImageCropRegion] = None


# ------------------------------------------------------------------------------------------------------------
# image crate resampling (imageops::sample: vertical_sample then horizontal_sample through an f32 image)
# ------------------------------------------------------------------------------------------------------------
def _catmull_rom(x: np.ndarray) -> np.ndarray:
    """`bc_cubic_spline(x, 0, 0.5)`, support 2."""
    a = np.abs(x).astype(f32)
    b, c = f32(0.0), f32(0.5)
    k = np.where(a < 1, (12 - 9 * b - 6 * c) * a ** 3 + (-18 + 12 * b + 6 * c) * a ** 2 + (6 - 2 * b),
                 np.where(a < 2, (-b - 6 * c) * a ** 3 + (6 * b + 30 * c) * a ** 2 + (-12 * b - 48 * c) * a + (8 * b + 24 * c), 0.0))
    return (k / 6).astype(f32)


def _sample_axis(img: np.ndarray, new_len: int, axis: int) -> np.ndarray:
    """One pass of the separable resampler along `axis` of an f32 [H, W, C] image."""
    n = img.shape[axis]
    ratio = f32(n) / f32(new_len)
    sratio = max(ratio, f32(1.0))
    support = f32(2.0) * sratio
    out_shape = list(img.shape)
    out_shape[axis] = new_len
    out = np.empty(out_shape, f32)
    src = np.moveaxis(img, axis, 0)
    dst = np.moveaxis(out, axis, 0)
    for o in range(new_len):
        centre = (f32(o) + f32(0.5)) * ratio
        left = int(min(max(np.floor(centre - support), 0), n - 1))
        right = int(min(max(np.ceil(centre + support), left + 1), n))
        c = centre - f32(0.5)
        w = _catmull_rom((np.arange(left, right, dtype=f32) - c) / sratio)
        w = (w / w.sum(dtype=f32)).astype(f32)
        dst[o] = np.tensordot(w, src[left:right], axes=(0, 0))
    return out


def resize_catmull_rom(rgb: np.ndarray, new_width: int, new_height: int) -> np.ndarray:
    """`imageops::resize(image, w, h, FilterType::CatmullRom)` on an 8-bit RGB image."""
    if rgb.dtype != np.uint8 or rgb.ndim != 3:
        raise ValueError("expected uint8 [H,W,C]")
    if rgb.shape[1] == new_width and rgb.shape[0] == new_height:
        return rgb.copy()
    tmp = _sample_axis(rgb.astype(f32), new_height, 0)   # vertical pass keeps f32
    out = _sample_axis(tmp, new_width, 1)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)  # clamp + round-to-nearest on the way back to u8


def prepare_depth_anything3_image(rgb: np.ndarray, target: int) -> PreparedModelImage:
    """src/model/mod.rs:162-210."""
    if target == 0:
        raise ValueError("depth_anything3 requires a non-zero target resolution")
    oh, ow = rgb.shape[:2]
    if ow == target and oh == target:
        return PreparedModelImage(target, target, rgb.copy(), None)
    shortest = f32(max(min(ow, oh), 1))
    scale = f32(target) / shortest
    sw = max(int(np.round(f32(ow) * scale)), target)   # f32::round = half away from zero; sizes are never at .5 here
    sh = max(int(np.round(f32(oh) * scale)), target)
    resized = resize_catmull_rom(rgb, sw, sh)
    cx, cy = max(sw - target, 0) // 2, max(sh - target, 0) // 2
    return PreparedModelImage(target, target, np.ascontiguousarray(resized[cy:cy + target, cx:cx + target]), None)


# ------------------------------------------------------------------------------------------------------------
# save_depth_map (example/inference.rs:103-273)
# ------------------------------------------------------------------------------------------------------------
def crop_depth_field(values: np.ndarray, region: ImageCropRegion) -> np.ndarray:
    h, w = values.shape
    if region.x + region.width > w or region.y + region.height > h:
        raise ValueError(f"Crop region {region} exceeds depth tensor bounds {w}x{h}")
    return values[region.y:region.y + region.height, region.x:region.x + region.width].copy()


def resize_depth_field(values: np.ndarray, dst_width: int, dst_height: int) -> np.ndarray:
    """`resize_depth_field` + `sample_depth_bilinear`: half-pixel centres, x0 = clamp(floor(x)), and the fraction
    taken against the CLAMPED x0 (so the border extrapolates, unlike Depth Pro's own resize)."""
    sh, sw = values.shape
    if sw == dst_width and sh == dst_height:
        return values.astype(f32, copy=True)
    v = values.astype(f32)
    sx = f32(sw) / f32(dst_width) if dst_width > 1 else f32(0)
    sy = f32(sh) / f32(dst_height) if dst_height > 1 else f32(0)
    xs = ((np.arange(dst_width, dtype=f32) + f32(0.5)) * sx - f32(0.5)) if dst_width > 1 else np.zeros(dst_width, f32)
    ys = ((np.arange(dst_height, dtype=f32) + f32(0.5)) * sy - f32(0.5)) if dst_height > 1 else np.zeros(dst_height, f32)

    def idx(c, n):
        c0 = np.clip(np.floor(c), 0, n - 1).astype(np.int64)
        c1 = np.clip(c0 + 1, 0, n - 1)
        return c0, c1, (c - c0.astype(f32)).astype(f32)

    x0, x1, fx = idx(xs, sw)
    y0, y1, fy = idx(ys, sh)
    one = f32(1)
    top = v[y0][:, x0] * (one - fx) + v[y0][:, x1] * fx
    bot = v[y1][:, x0] * (one - fx) + v[y1][:, x1] * fx
    return (top * (one - fy)[:, None] + bot * fy[:, None]).astype(f32)


def depth_to_u8(depth: np.ndarray, crop: Optional[ImageCropRegion] = None,
                target_dims: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The pixel values `save_depth_map` writes: optional crop, optional bilinear restore to (width, height),
    min-max normalisation over the finite values (all non-finite -> range [0,1], non-finite pixels -> 0)."""
    if depth.ndim == 3:
        if depth.shape[0] != 1:
            raise ValueError(f"Example expects batch size of 1, got {depth.shape[0]}.")
        depth = depth[0]
    v = depth.astype(f32)
    if crop is not None:
        v = crop_depth_field(v, crop)
    if target_dims is not None and (target_dims[0] != v.shape[1] or target_dims[1] != v.shape[0]):
        v = resize_depth_field(v, target_dims[0], target_dims[1])
    fin = np.isfinite(v)
    lo, hi = (f32(v[fin].min()), f32(v[fin].max())) if fin.any() else (f32(0), f32(1))
    rng = max(f32(hi - lo), np.finfo(f32).eps)
    norm = np.where(fin, np.clip((v - lo) / rng, 0, 1), 0).astype(f32)
    return np.clip(np.floor(norm * f32(255) + f32(0.5)), 0, 255).astype(np.uint8)  # f32::round on non-negative values


def prepare_input_frame(rgb: np.ndarray, patch_size: int, preferred_resolution: Optional[int]) -> PreparedModelImage:
    """`prepare_input_frame` (crates/bevy_burn_depth/src/lib.rs:76-132): with a preferred resolution, the shortest-side
    Catmull-Rom resize + centre crop of `prepare_depth_anything3_image` (target raised to the patch size); without one, a
    centre crop to patch-aligned sizes (`align_down`: multiples of 4 * patch from 4 * patch on, of patch below that, the size
    itself below one patch)."""
    patch_size = max(int(patch_size), 1)
    if preferred_resolution is not None:
        return prepare_depth_anything3_image(rgb, max(int(preferred_resolution), patch_size, 1))
    h, w = rgb.shape[:2]
    alignment = patch_size * 4

    def align_down(v: int) -> int:
        if v < patch_size:
            return v
        return v - v % (alignment if v >= alignment else patch_size)

    cw, ch = max(align_down(w), 1), max(align_down(h), 1)
    if cw == w and ch == h:
        return PreparedModelImage(w, h, rgb.copy(), None)
    ox, oy = (w - cw) // 2, (h - ch) // 2
    return PreparedModelImage(cw, ch, np.ascontiguousarray(rgb[oy:oy + ch, ox:ox + cw]), None)


def depth_to_display(depth: np.ndarray, crop: Optional[ImageCropRegion] = None, target_dims: Optional[Tuple[int, int]] = None,
                     normalize: bool = True, fmt: str = "u8") -> np.ndarray:
    """The display step of the frame path, per frame of [H,W] or [B,H,W]: `depth_to_u8`'s pixels for fmt "u8" (needs
    normalize); for fmt "rgba" the viewer's texture (lib.rs:40-73) -- grey = the same min-max normalised value (or the raw
    depth without normalize) three times, alpha 1 -- as f32 [..., 4]."""
    if fmt not in ("u8", "rgba"):
        raise ValueError(f"unknown display format `{fmt}`")
    if fmt == "u8" and not normalize:
        raise ValueError("the u8 display needs normalize")
    frames = depth[None] if depth.ndim == 2 else depth
    out = []
    for d in frames:
        if fmt == "u8":
            out.append(depth_to_u8(d, crop, target_dims))
            continue
        v = d.astype(f32)
        if crop is not None:
            v = crop_depth_field(v, crop)
        if target_dims is not None and (target_dims[0] != v.shape[1] or target_dims[1] != v.shape[0]):
            v = resize_depth_field(v, target_dims[0], target_dims[1])
        if normalize:
            fin = np.isfinite(v)
            lo, hi = (f32(v[fin].min()), f32(v[fin].max())) if fin.any() else (f32(0), f32(1))
            rng = max(f32(hi - lo), np.finfo(f32).eps)
            v = np.where(fin, np.clip((v - lo) / rng, 0, 1), 0).astype(f32)
        out.append(np.stack([v, v, v, np.ones_like(v)], axis=-1).astype(f32))
    res = np.stack(out)
    return res[0] if depth.ndim == 2 else res


def write_gray_png(path: str, pixels: np.ndarray) -> None:
    if pixels.dtype != np.uint8 or pixels.ndim != 2:
        raise ValueError("expected uint8 [H,W]")
    h, w = pixels.shape

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = b"".join(b"\x00" + pixels[y].tobytes() for y in range(h))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_gray_png(path: str) -> np.ndarray:
    """Reader for the files `write_gray_png` produces (8-bit grayscale, filter type 0 rows)."""
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w = 8, b"", 0
    h = 0
    while pos < len(b):
        (n,), tag = struct.unpack(">I", b[pos:pos + 4]), b[pos + 4:pos + 8]
        data = b[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h = struct.unpack(">II", data[:8])
        elif tag == b"IDAT":
            idat += data
        pos += 12 + n
    raw = zlib.decompress(idat)
    rows = np.frombuffer(raw, np.uint8).reshape(h, w + 1)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].copy()


# ------------------------------------------------------------------------------------------------------------
# point path: the host reference of md_op_unproject / md_infer_points (include/mi_depth.h states the op order)
# ------------------------------------------------------------------------------------------------------------
@dataclass
class HostPoints:
    point_map: np.ndarray            # [B,H,W,3], (0,0,0) at invalid pixels
    mask: np.ndarray                 # uint8 [B,H,W]
    xyz: np.ndarray                  # [N,3], order (b, v, u) ascending
    rgb: Optional[np.ndarray]        # uint8 [N,3]
    conf: Optional[np.ndarray]       # [N]
    count: np.ndarray                # int32 [B+1]: per view, then the total
    normal_map: Optional[np.ndarray] = None  # [B,H,W,3] (normals=True): the unit normal, (0,0,0) where invalid or not defined
    normals: Optional[np.ndarray] = None     # [N,3], rows parallel to xyz


def unproject_depth(depth, intrinsics=None, extrinsics=None, focal_px=None, conf=None, rgb=None, *, pixel_offset=0.0,
                    depth_min=0.0, depth_max=0.0, conf_min=0.0, edge_rtol=0.0, stride=1, world=False,
                    normals=False, normal_min_cos=0.0, dtype=np.float32) -> HostPoints:
    """depth [B,H,W] and pinhole cameras -> point map, validity mask and the ordered list of valid points. Every step is one
    rounded operation of `dtype`, in the order of the device kernels (kernels/points.hip): with dtype f32 the results are
    theirs bit for bit; dtype=np.float64 is the same formulas for the geometric tests. intrinsics [B,3,3] or focal_px [B]
    (K = f, f, W/2, H/2); extrinsics [B,3,4] world-to-camera (camera.rs:248-254), applied inverted when `world`.

    normals / normal_min_cos (md_op_unproject_normals; include/mi_depth.h states the contract): the surface normal of every pixel
    from its four neighbours, and with normal_min_cos > 0 the grazing-angle test in the validity. The defaults compute what the
    call computed before they existed."""
    T = np.dtype(dtype).type
    d = np.asarray(depth, dtype=dtype)
    if d.ndim != 3:
        raise ValueError(f"expected depth [B,H,W], got {d.shape}")
    B, H, W = d.shape
    if stride < 1:
        raise ValueError("stride must be at least 1")
    if intrinsics is not None:
        K = np.asarray(intrinsics, dtype=dtype).reshape(B, 3, 3)
        fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    elif focal_px is not None:
        f = np.asarray(focal_px, dtype=dtype).reshape(B)
        fx, fy = f, f
        cx, cy = np.full(B, T(W) / T(2), dtype), np.full(B, T(H) / T(2), dtype)
    else:
        raise ValueError("neither intrinsics nor a focal length")
    if world and extrinsics is None:
        raise ValueError("world needs extrinsics")
    if not np.isfinite(normal_min_cos) or not 0 <= normal_min_cos <= 1:
        raise ValueError("normal_min_cos must lie in [0, 1]")
    want_normals = bool(normals) or normal_min_cos > 0
    f32i = np.finfo(np.float32)
    dmin = T(depth_min) if depth_min > 0 else T(f32i.tiny)
    dmax = T(depth_max) if depth_max > 0 else T(f32i.max)
    with np.errstate(all="ignore"):
        valid = np.isfinite(d) & (d >= dmin) & (d <= dmax)
        cf = None
        if conf is not None:
            cf = np.asarray(conf, dtype=dtype).reshape(B, H, W)
            valid &= cf >= T(conf_min)
        if edge_rtol > 0:
            rt = T(edge_rtol)

            def ok(dc, dn):  # a neighbour that is not finite or <= 0 is ignored
                return ~(np.isfinite(dn) & (dn > 0)) | (np.abs(dc - dn) <= rt * np.minimum(dc, dn))

            valid[:, 1:, :] &= ok(d[:, 1:, :], d[:, :-1, :])
            valid[:, :-1, :] &= ok(d[:, :-1, :], d[:, 1:, :])
            valid[:, :, 1:] &= ok(d[:, :, 1:], d[:, :, :-1])
            valid[:, :, :-1] &= ok(d[:, :, :-1], d[:, :, 1:])
        off = T(pixel_offset)
        u = np.arange(W, dtype=dtype)[None, None, :]
        v = np.arange(H, dtype=dtype)[None, :, None]
        b3 = lambda a: a.astype(dtype)[:, None, None]  # noqa: E731
        rx = ((u + off) - b3(cx)) / b3(fx)
        ry = ((v + off) - b3(cy)) / b3(fy)
        x, y, z = rx * d, ry * d, d
        nm = None
        if want_normals:
            nrm, defined, cosv = _pixel_normals(d, cf, (x, y, np.broadcast_to(z, d.shape)), dmin, dmax, T(conf_min), T(edge_rtol), T(f32i.tiny))
            if normal_min_cos > 0:
                valid &= defined & (cosv >= T(normal_min_cos))
        if world:
            E = np.asarray(extrinsics, dtype=dtype).reshape(B, 3, 4)
            R = lambda i, j: E[:, i, j][:, None, None]  # noqa: E731
            if want_normals:  # n_w = R^T n in the operation order of the point below, not renormalised
                nrm = [(R(0, j) * nrm[0] + R(1, j) * nrm[1]) + R(2, j) * nrm[2] for j in range(3)]
            qx, qy, qz = x - R(0, 3), y - R(1, 3), z - R(2, 3)
            x = (R(0, 0) * qx + R(1, 0) * qy) + R(2, 0) * qz
            y = (R(0, 1) * qx + R(1, 1) * qy) + R(2, 1) * qz
            z = (R(0, 2) * qx + R(1, 2) * qy) + R(2, 2) * qz
        pm = np.stack([np.broadcast_to(c, d.shape) for c in (x, y, z)], axis=-1).astype(dtype)
        if want_normals:
            nm = np.where((valid & defined)[..., None], np.stack(nrm, axis=-1), T(0)).astype(dtype)
    pm = np.where(valid[..., None], pm, T(0)).astype(dtype)
    sel = valid.copy()
    if stride > 1:
        keep = np.zeros((H, W), bool)
        keep[::stride, ::stride] = True
        sel &= keep[None]
    count = np.concatenate([sel.reshape(B, -1).sum(1), [sel.sum()]]).astype(np.int32)
    return HostPoints(pm, valid.astype(np.uint8), pm[sel], None if rgb is None else np.asarray(rgb, np.uint8).reshape(B, H, W, 3)[sel],
                      None if cf is None else cf[sel], count, nm if normals else None, nm[sel] if normals else None)


def _pixel_normals(d, cf, P, dmin, dmax, conf_min, rt, tiny):
    """The normal of md_op_unproject_normals (include/mi_depth.h) for every pixel of d [B,H,W] at once: P = the camera-space
    points (x, y, z), cf = the confidence map or None. -> ((nx, ny, nz) in camera space, defined, cosv). One rounded operation of
    d's dtype per step, in the order of pixel_normal (kernels/points.hip). With x right, y down, z forward every cross of the
    pair order below points at the camera: for positive depths the sign of P_c . (e_a x e_b) is the sign of det(r_c, r_a, r_b)
    of the three pixel rays, whatever the depths, so cosv > 0 in exact arithmetic and nothing is flipped."""
    B, H, W = d.shape

    def at(a, dv, du, fill):  # a at (v + dv, u + du), `fill` outside the image
        pad = np.pad(a, ((0, 0), (1, 1), (1, 1)), constant_values=fill)
        return pad[:, 1 + dv:1 + dv + H, 1 + du:1 + du + W]

    inside = np.ones((B, H, W), bool)
    e, use = {}, {}
    for name, (dv, du) in (("E", (0, 1)), ("S", (1, 0)), ("W", (0, -1)), ("N", (-1, 0))):
        dn = at(d, dv, du, 0)
        ok = at(inside, dv, du, False) & np.isfinite(dn) & (dn >= dmin) & (dn <= dmax)
        if cf is not None:
            ok &= at(cf, dv, du, 0) >= conf_min
        if rt > 0:
            ok &= np.abs(d - dn) <= rt * np.minimum(d, dn)
        use[name] = ok
        e[name] = [at(c, dv, du, 0) - c for c in P]
    m = [np.zeros_like(d) for _ in range(3)]
    have = np.zeros((B, H, W), bool)
    for a, b in (("S", "E"), ("E", "N"), ("N", "W"), ("W", "S")):
        (ax, ay, az), (bx, by, bz) = e[a], e[b]
        c = ((ay * bz) - (az * by), (az * bx) - (ax * bz), (ax * by) - (ay * bx))
        both = use[a] & use[b]
        m = [np.where(both, np.where(have, mi + ci, ci), mi) for mi, ci in zip(m, c)]  # summed from the first usable pair on
        have |= both
    len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
    defined = have & np.isfinite(len2) & (len2 >= tiny)
    s = np.sqrt(len2)
    n = [np.where(defined, mi / s, d.dtype.type(0)) for mi in m]
    px, py, pz = P
    cosv = -((n[0] * px + n[1] * py) + n[2] * pz) / np.sqrt((px * px + py * py) + pz * pz)
    return n, defined, cosv


def filter_views(depth, conf=None, intrinsics=None, extrinsics=None, focal_px=None, *, pixel_offset=0.0, depth_min=0.0,
                 depth_max=0.0, conf_percentile=0, view_rtol=0.0, min_views=0, dtype=np.float32):
    """The host reference of md_op_filter_views (include/mi_depth.h states the contract): depth [B,H,W], optional conf [B,H,W]
    and the cameras of `unproject_depth` -> (depth_out [B,H,W]: d where kept, else 0; support uint8 [B,H,W]; tau, a `dtype`
    scalar; kept int32 [B+1]: per view, then the total). Every step is one rounded operation of `dtype`, in the order of the
    device kernels (kernels/view_filter.hip): with f32 the results are theirs bit for bit; dtype=np.float64 is the same
    formulas for the geometric tests."""
    T = np.dtype(dtype).type
    d = np.asarray(depth, dtype=dtype)
    if d.ndim != 3:
        raise ValueError(f"expected depth [B,H,W], got {d.shape}")
    B, H, W = d.shape
    q = int(conf_percentile)
    if not 0 <= q <= 99:
        raise ValueError("conf_percentile outside 0..99")
    if q > 0 and conf is None:
        raise ValueError("conf_percentile needs a confidence map")
    if not np.isfinite(view_rtol) or view_rtol < 0:
        raise ValueError("view_rtol must be finite and >= 0")
    views = view_rtol > 0
    if (not views and min_views != 0) or (views and not 1 <= min_views <= B - 1):
        raise ValueError("min_views: 0 without view_rtol, 1..B-1 with it")
    if views and not 2 <= B <= 64:
        raise ValueError("view_rtol takes 2..64 views")
    f32i = np.finfo(np.float32)
    dmin = T(depth_min) if depth_min > 0 else T(f32i.tiny)
    dmax = T(depth_max) if depth_max > 0 else T(f32i.max)
    with np.errstate(all="ignore"):
        cand = np.isfinite(d) & (d >= dmin) & (d <= dmax)
        cf = None
        if conf is not None:
            cf = np.asarray(conf, dtype=dtype).reshape(B, H, W)
            cand &= np.isfinite(cf) & (cf >= T(0))
        # ---- percentile: tau = the k-th smallest candidate confidence, k = (N - 1) q // 100 ----
        tau = T(0)
        if q > 0:
            c = cf[cand]
            c = np.where(c == 0, T(0), c)  # -0 counts as +0
            if c.size:
                tau = np.sort(c)[((c.size - 1) * q) // 100]
        surv = cand & (cf >= tau) if cf is not None else cand
        # ---- cross-view support ----
        support = np.zeros((B, H, W), np.uint8)
        if views:
            if extrinsics is None:
                raise ValueError("view_rtol needs extrinsics")
            if intrinsics is not None:
                K = np.asarray(intrinsics, dtype=dtype).reshape(B, 3, 3)
                fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
            elif focal_px is not None:
                fx = fy = np.asarray(focal_px, dtype=dtype).reshape(B)
                cx, cy = np.full(B, T(W) / T(2), dtype), np.full(B, T(H) / T(2), dtype)
            else:
                raise ValueError("neither intrinsics nor a focal length")
            E = np.asarray(extrinsics, dtype=dtype).reshape(B, 3, 4)
            off, rt, half = T(pixel_offset), T(view_rtol), T(0.5)
            u = np.arange(W, dtype=dtype)[None, :]
            v = np.arange(H, dtype=dtype)[:, None]
            for i in range(B):
                # X_w exactly as unproject_depth(world=True) computes it
                rx = ((u + off) - cx[i]) / fx[i]
                ry = ((v + off) - cy[i]) / fy[i]
                qx, qy, qz = rx * d[i] - E[i, 0, 3], ry * d[i] - E[i, 1, 3], d[i] - E[i, 2, 3]
                X = [(E[i, 0, a] * qx + E[i, 1, a] * qy) + E[i, 2, a] * qz for a in range(3)]
                sup = np.zeros((H, W), np.int32)
                for j in range(B):
                    if j == i:
                        continue
                    px, py, pz = [((E[j, a, 0] * X[0] + E[j, a, 1] * X[1]) + E[j, a, 2] * X[2]) + E[j, a, 3] for a in range(3)]
                    uf = ((fx[j] * (px / pz)) + cx[j]) - off
                    vf = ((fy[j] * (py / pz)) + cy[j]) - off
                    uu, vv = np.floor(uf + half), np.floor(vf + half)
                    seen = (pz > 0) & (uu >= 0) & (uu < T(W)) & (vv >= 0) & (vv < T(H))
                    ui, vi = np.where(seen, uu, 0).astype(np.int64), np.where(seen, vv, 0).astype(np.int64)
                    dj = d[j][vi, ui]
                    ok = seen & surv[j][vi, ui] & (np.abs(pz - dj) <= rt * np.minimum(pz, dj))
                    sup += ok
                support[i] = np.where(surv[i], sup, 0).astype(np.uint8)
        kept_mask = surv & (support >= min_views)
    depth_out = np.where(kept_mask, d, T(0)).astype(dtype)
    kept = np.concatenate([kept_mask.reshape(B, -1).sum(1), [kept_mask.sum()]]).astype(np.int32)
    return depth_out, support, T(tau), kept


@dataclass
class HostVoxels:
    xyz: np.ndarray                  # f32 [M,3]: one input row per occupied voxel, in ascending input index
    conf: Optional[np.ndarray]       # f32 [M]
    rgb: Optional[np.ndarray]        # uint8 [M,3]
    normals: Optional[np.ndarray]    # f32 [M,3]
    index: np.ndarray                # int32 [M]: the source row
    weight: np.ndarray               # int32 [M]: in-range points of the row's voxel
    count: np.ndarray                # int32 [B+1]: survivors per view, then their total
    dropped: int                     # rows that are not finite or outside the grid


def voxel_thin(xyz, voxel, conf=None, rgb=None, normals=None, counts=None) -> HostVoxels:
    """The host reference of md_op_voxel_thin / md_infer_points_voxel (include/mi_depth.h states the contract): of the points of
    every voxel of side `voxel` the one with the largest confidence survives, among equals the first; the survivors keep the input
    order and every row is copied unchanged. f32, one rounded operation per step: the device kernels (kernels/voxel.hip) give the
    same bits. counts: the rows of every view of the input, [B] (default: one view) -> `count` per view."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = len(p)
    vs = np.float32(voxel)
    if not np.isfinite(vs) or not vs > 0:
        raise ValueError("voxel must be finite and > 0")
    if N >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    cf = None if conf is None else np.ascontiguousarray(conf, dtype=np.float32).reshape(N)
    half = np.float32(1 << 20)
    with np.errstate(all="ignore"):
        c = np.floor(p / vs)
        ok = np.isfinite(p).all(1) & (c >= -half).all(1) & (c < half).all(1)
    idx = np.nonzero(ok)[0].astype(np.uint64)
    cell = (c[ok].astype(np.int64) + (1 << 20)).astype(np.uint64)
    key = (cell[:, 0] << np.uint64(42)) | (cell[:, 1] << np.uint64(21)) | cell[:, 2]
    w = np.zeros(len(idx), np.uint64)
    if cf is not None:
        ci = cf[ok]
        with np.errstate(all="ignore"):
            use = np.isfinite(ci) & (ci >= 0)
        wb = ci.view(np.uint32).astype(np.uint64)
        wb[wb == 0x80000000] = 0  # -0 counts as +0
        w = np.where(use, wb, np.uint64(0))
    rank = (w << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)  # the device's atomicMax word
    order = np.lexsort((rank, key))
    ks = key[order]
    last = np.ones(len(ks), bool)
    last[:-1] = ks[1:] != ks[:-1]  # the largest rank of every key
    first = np.ones(len(ks), bool)
    first[1:] = last[:-1]
    size = np.diff(np.append(np.nonzero(first)[0], len(ks)))
    win = (np.uint64(0xFFFFFFFF) - (rank[order][last] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    asc = np.argsort(win, kind="stable")
    index, weight = win[asc].astype(np.int32), size[asc].astype(np.int32)
    if counts is None:
        bounds = np.array([0, N], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]), N)
    per_view = np.diff(np.searchsorted(index, bounds, side="left"))
    count = np.concatenate([per_view, [len(index)]]).astype(np.int32)
    take = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)[index]  # noqa: E731
    return HostVoxels(p[index], None if cf is None else cf[index], take(rgb, np.uint8, (N, 3)), take(normals, np.float32, (N, 3)), index,
                      weight, count, int(N - ok.sum()))


@dataclass
class HostDecimated:
    vertices: HostVoxels             # exactly voxel_thin's outputs on the same rows
    remap: np.ndarray                # int32 [N]: the output row of the survivor of every input row's voxel (the true rank), -1 outside the grid
    faces: np.ndarray                # int32 [K,3]: the kept faces over the output rows, in ascending source face, winding unchanged
    face_index: np.ndarray           # int32 [K]: the source face
    face_count: np.ndarray           # int32 [B+1]: kept faces per view of their source face, then their total
    faces_dropped: np.ndarray        # int32 [3]: invalid, degenerate, duplicate faces


def decimate_mesh(xyz, faces, voxel, conf=None, rgb=None, normals=None, counts=None, face_counts=None, capacity=None) -> HostDecimated:
    """The host reference of md_op_decimate_mesh (include/mi_depth.h states the contract): vertex clustering. The vertices are
    voxel_thin's; face (p, q, r) maps to (remap[p], remap[q], remap[r]) and is, in this order, invalid (a corner outside 0..N-1, a
    remap of -1 or one >= capacity), degenerate (two mapped corners equal), a duplicate (an earlier live face has the same triple
    after both are rotated so that the smallest index comes first; the reversed triple is another face) or kept, as its mapped
    triple in the input's rotation. capacity: the rows the vertex outputs hold (default N); the returned lists are not cut to it.
    counts / face_counts: the rows / faces of every view of the input, [B] (default: one view). Selection only: the device
    kernels (kernels/decimate.hip) give the same bits."""
    v = voxel_thin(xyz, voxel, conf, rgb, normals, counts)
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = len(p)
    fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    F = len(fc)
    if F >= 1 << 30:
        raise ValueError("fewer than 2^30 faces")
    cap = N if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("capacity is negative")
    vs, half = np.float32(voxel), np.float32(1 << 20)
    with np.errstate(all="ignore"):
        c = np.floor(p / vs)
        ok = np.isfinite(p).all(1) & (c >= -half).all(1) & (c < half).all(1)
    cell = (c[ok].astype(np.int64) + (1 << 20)).astype(np.uint64)
    key = (cell[:, 0] << np.uint64(42)) | (cell[:, 1] << np.uint64(21)) | cell[:, 2]
    full = np.zeros(N, np.uint64)
    full[ok] = key
    skey = full[v.index]  # one key per output row; every in-range row's key is among them
    by_key = np.argsort(skey)
    remap = np.full(N, -1, np.int32)
    remap[ok] = by_key[np.searchsorted(skey[by_key], key)].astype(np.int32)
    inside = ((fc >= 0) & (fc < N)).all(1)
    padded = np.append(remap, np.int32(-1))  # a corner outside the list reads the -1 behind it
    m = padded[np.where(inside[:, None], fc, N)]
    invalid = ~inside | (m < 0).any(1) | (m >= cap).any(1)
    degenerate = ~invalid & ((m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2]))
    live = np.nonzero(~invalid & ~degenerate)[0]
    lm = m[live]
    k = np.argmin(lm, axis=1)  # distinct corners: the smallest is unique
    at = np.arange(len(lm))
    rot = np.stack([lm[at, k], lm[at, (k + 1) % 3], lm[at, (k + 2) % 3]], axis=1)
    if len(rot):
        _, first = np.unique(rot, axis=0, return_index=True)  # the first occurrence = the smallest source face
        kept = live[np.sort(first)]
    else:
        kept = live
    if face_counts is None:
        bounds = np.array([0, F], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(face_counts, np.int64).reshape(-1))]), F)
    per_view = np.diff(np.searchsorted(kept, bounds, side="left"))
    face_count = np.concatenate([per_view, [len(kept)]]).astype(np.int32)
    dropped = np.array([invalid.sum(), degenerate.sum(), len(live) - len(kept)], np.int32)
    return HostDecimated(v, remap, m[kept], kept.astype(np.int32), face_count, dropped)


@dataclass
class HostComponents:
    label: np.ndarray                # int32 [N]: the smallest row of every row's component
    component_faces: np.ndarray      # int32 [N]: the valid faces of every row's component, 0 for a row no valid face names
    faces: np.ndarray                # int32 [K,3]: the kept faces in ascending source face, winding unchanged (through remap with compact)
    face_index: np.ndarray           # int32 [K]: the source face
    face_count: np.ndarray           # int32 [B+1]: kept faces per view of their source face, then their total
    stats: np.ndarray                # int32 [5]: invalid, dropped, clipped faces, components with a face, components kept
    index: Optional[np.ndarray] = None   # compact: int32 [M] the surviving rows in ascending order
    remap: Optional[np.ndarray] = None   # compact: int32 [N] the output row of a surviving row, -1 otherwise
    xyz: Optional[np.ndarray] = None     # compact: the carried rows of the survivors
    conf: Optional[np.ndarray] = None
    rgb: Optional[np.ndarray] = None
    normals: Optional[np.ndarray] = None


def mesh_components(faces, n_rows, min_faces=1, face_counts=None, compact=False, capacity=None, xyz=None, conf=None, rgb=None,
                    normals=None, face_capacity=None) -> HostComponents:
    """The host reference of md_op_mesh_components (include/mi_depth.h states the contract): connected components of the faces
    int32 [F,3] over `n_rows` rows and island removal. A face is invalid when a corner is < 0 or >= n_rows: it joins nothing and
    is never kept. Two rows are connected when a valid face names both (sharing one vertex joins; a degenerate face joins what
    it names); label[i] = the smallest row of row i's component; component_faces[i] = its valid faces. A valid face is kept iff
    its component has at least min_faces >= 1 faces; the kept faces come in ascending f. face_counts: the faces of every view of
    the input, [B] (default: one view). compact: the rows that a face of a kept component names survive in ascending order
    (index, remap, the carried rows), the faces are written through remap, and a face of a kept component with a mapped corner
    >= capacity (default n_rows) is clipped: dropped and counted. face_capacity: the rows faces / face_index hold (default: all);
    face_count stays the true total. The vertex lists are not cut to `capacity`. Integers only:
    the device kernels (kernels/components.hip) give the same bits."""
    N, min_faces = int(n_rows), int(min_faces)
    fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    F = len(fc)
    if N < 0 or N >= 1 << 30 or F >= 1 << 30:
        raise ValueError("fewer than 2^30 rows and faces")
    if min_faces < 1:
        raise ValueError("min_faces >= 1")
    valid = ((fc >= 0) & (fc < N)).all(1)
    vf = fc[valid].astype(np.int64)
    # label propagation that keeps lab[i] <= i and lab[i] inside i's component: hook the corners and their labels under the
    # face's smallest label, jump until lab[lab] == lab; at the fixed point a label is constant on a component, a member of it
    # and <= every member
    lab = np.arange(N, dtype=np.int64)
    while len(vf):
        la = lab[vf]
        m = np.repeat(la.min(1), 3)
        new = lab.copy()
        np.minimum.at(new, la.ravel(), m)
        np.minimum.at(new, vf.ravel(), m)
        while True:
            jump = new[new]
            if np.array_equal(jump, new):
                break
            new = jump
        if np.array_equal(new, lab):
            break
        lab = new
    size = np.bincount(lab[vf[:, 0]], minlength=N) if len(vf) else np.zeros(N, np.int64)
    component_faces = size[lab] if N else np.zeros(0, np.int64)
    roots = (lab == np.arange(N)) & (size > 0)
    big = np.zeros(F, bool)
    big[valid] = size[lab[vf[:, 0]]] >= min_faces
    stats = np.zeros(5, np.int32)
    stats[0], stats[1] = F - valid.sum(), (valid & ~big).sum()
    stats[3], stats[4] = roots.sum(), (roots & (size >= min_faces)).sum()
    res = HostComponents(lab.astype(np.int32), component_faces.astype(np.int32), None, None, None, stats)
    keep = big
    if compact:
        cap = N if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError("capacity is negative")
        survive = component_faces >= min_faces
        res.index = np.nonzero(survive)[0].astype(np.int32)
        res.remap = np.full(N, -1, np.int32)
        res.remap[res.index] = np.arange(len(res.index), dtype=np.int32)
        mapped = res.remap[np.where(big[:, None], fc, 0)] if N else np.zeros((F, 3), np.int32)
        clipped = big & (mapped >= cap).any(1)
        stats[2] = clipped.sum()
        keep = big & ~clipped
        res.faces = np.ascontiguousarray(mapped[keep], dtype=np.int32)
        carry = lambda a, dt, w: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape((N, w) if w else (N,))[res.index]  # noqa: E731
        res.xyz, res.conf, res.rgb, res.normals = carry(xyz, np.float32, 3), carry(conf, np.float32, 0), carry(rgb, np.uint8, 3), carry(normals, np.float32, 3)
    else:
        res.faces = fc[keep]
    kept = np.nonzero(keep)[0]
    if face_counts is None:
        bounds = np.array([0, F], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(face_counts, np.int64).reshape(-1))]), F)
    per_view = np.diff(np.searchsorted(kept, bounds, side="left"))
    res.face_index = kept.astype(np.int32)
    res.face_count = np.concatenate([per_view, [len(kept)]]).astype(np.int32)
    if face_capacity is not None:
        if int(face_capacity) < 0:
            raise ValueError("face_capacity is negative")
        res.faces, res.face_index = res.faces[:int(face_capacity)], res.face_index[:int(face_capacity)]
    return res


@dataclass
class HostSmoothed:
    xyz: np.ndarray                      # f32 [min(N, capacity),3]: the smoothed rows; the input bits of a row that did not move
    normals: Optional[np.ndarray]        # f32 [min(N, capacity),3]: the area-weighted normals of the smoothed faces; None when not asked for
    stats: np.ndarray                    # int32 [5]: invalid faces, degenerate faces, rows not in range, open rows, moved rows


def _smooth_mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64's finaliser on a uint64 array, modulo 2^64 (kernels/smooth_math.h: smooth_mix64)."""
    x = x.astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def smooth_mesh(xyz, faces, step, iterations, lam, mu=0.0, pin_boundary=True, normals=False, capacity=None) -> HostSmoothed:
    """The host reference of md_op_smooth_mesh / md_infer_points_smooth (include/mi_depth.h states the contract): Taubin (lam | mu)
    or, with mu == 0, Laplacian smoothing of the rows xyz f32 [N,3] over the faces int32 [F,3] with the face-weighted umbrella
    operator, on an integer lattice of side `step`: k = rint(p / step) in f32; a face with a corner outside 0..N-1 or on a row
    that is not in range (non-finite, or |k| > 2^22) is invalid, a valid face with two equal corners degenerate, the others are
    live; deg[v] += 2 and open[v] += mix(next) - mix(prev) per corner of a live face; a row is pinned with deg == 0, out of range,
    or pin_boundary and open != 0; every step adds k[next] + k[prev] to S[v] in int64 and moves an unpinned row by
    rint(factor * (S / deg - k)) in f64, clamped to +-2^62. A row that ends where it began returns its input bits, any other
    k * step in f64 rounded to f32. normals: the int64 cross products of the final lattice positions summed per corner and
    normalised in f64. capacity: the rows the outputs hold (default N); every row takes part all the same. Integer sums only, in
    any order: the device kernels (kernels/smooth.hip) give the same bits."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    fc = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    N, F, iterations = len(p), len(fc), int(iterations)
    step, lam, mu = np.float32(step), np.float32(lam), np.float32(mu)
    if N >= 1 << 30 or F >= 1 << 30:
        raise ValueError("fewer than 2^30 rows and faces")
    if not (np.isfinite(step) and step > 0):
        raise ValueError("step is finite and > 0")
    if not (0 < lam <= 1) or not (-1 <= mu <= 0):
        raise ValueError("0 < lam <= 1 and -1 <= mu <= 0")
    if not 1 <= iterations <= 1024:
        raise ValueError("1 <= iterations <= 1024")
    cap = N if capacity is None else int(capacity)
    if cap < 0:
        raise ValueError("capacity is negative")
    with np.errstate(all="ignore"):
        kf = np.rint(p / step)  # f32
        in_range = np.isfinite(p).all(1) & (np.abs(kf) <= np.float32(4194304.0)).all(1)
        k0 = np.where(in_range[:, None], kf, np.float32(0)).astype(np.int64)
    inside = ((fc >= 0) & (fc < N)).all(1)
    valid = inside.copy()
    valid[inside] = in_range[fc[inside]].all(1)
    degenerate = valid & ((fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2]))
    lf = fc[valid & ~degenerate].astype(np.int64)
    v, nxt, prv = lf.ravel(), lf[:, [1, 2, 0]].ravel(), lf[:, [2, 0, 1]].ravel()
    deg = np.zeros(N, np.int64)
    np.add.at(deg, v, 2)
    opened = np.zeros(N, np.uint64)
    np.add.at(opened, v, _smooth_mix64(nxt) - _smooth_mix64(prv))
    free = ~((deg == 0) | ~in_range | (bool(pin_boundary) & (opened != 0)))
    degf = deg[free].astype(np.float64)[:, None]
    k = k0.copy()
    for t in range(2 * iterations if mu != 0 else iterations):
        factor = np.float64(mu if (mu != 0 and t & 1) else lam)
        S = np.zeros((N, 3), np.int64)
        np.add.at(S, v, k[nxt] + k[prv])
        d = S[free].astype(np.float64) / degf - k[free].astype(np.float64)
        r = np.clip(np.rint(factor * d), -2.0 ** 62, 2.0 ** 62)
        k[free] = k[free] + r.astype(np.int64)
    moved = (k != k0).any(1)
    out = p.copy()
    out[moved] = (k[moved].astype(np.float64) * np.float64(step)).astype(np.float32)
    nrm = None
    if normals:
        ka, kb, kc = k[lf[:, 0]], k[lf[:, 1]], k[lf[:, 2]]
        u, w = kb - ka, kc - ka
        cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        acc = np.zeros((N, 3), np.int64)
        for j in range(3):
            np.add.at(acc, lf[:, j], cross)
        nz = (deg > 0) & (acc != 0).any(1)
        x = acc[nz].astype(np.float64)
        length = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        nrm = np.zeros((N, 3), np.float32)
        nrm[nz] = (x / length[:, None]).astype(np.float32)
        nrm = nrm[:cap]
    stats = np.array([F - valid.sum(), degenerate.sum(), (~in_range).sum(), ((deg > 0) & (opened != 0)).sum(), moved.sum()], np.int32)
    return HostSmoothed(out[:cap], nrm, stats)


@dataclass
class HostOutliers:
    xyz: np.ndarray                  # f32 [M,3]: the surviving input rows, in ascending input index
    conf: Optional[np.ndarray]       # f32 [M]
    rgb: Optional[np.ndarray]        # uint8 [M,3]
    normals: Optional[np.ndarray]    # f32 [M,3]
    index: np.ndarray                # int32 [M]: the source row
    neighbours: np.ndarray           # int32 [N] over the input rows: min(neighbours, min_neighbours), -1 outside the grid
    count: np.ndarray                # int32 [B+1]: survivors per view, then their total
    dropped: int                     # rows that are not finite or outside the grid


def radius_outliers(xyz, radius, min_neighbours, conf=None, rgb=None, normals=None, counts=None) -> HostOutliers:
    """The host reference of md_op_radius_outliers / md_infer_points_outlier (include/mi_depth.h states the contract): a row survives
    when at least min_neighbours other rows lie in the 27 cells of side `radius` around its own AND within `radius` of it,
    d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius in f32, one rounded operation per step; the count saturates at min_neighbours. The
    survivors keep the input order and every row is copied unchanged: the device kernels (kernels/outlier.hip) give the same bits.
    A lexsort by cell key, then the 27 shifted lookups. counts: the rows of every view of the input, [B] (default: one view)."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = len(p)
    rs = np.float32(radius)
    k = int(min_neighbours)
    if not np.isfinite(rs) or not rs > 0:
        raise ValueError("radius must be finite and > 0")
    if k != min_neighbours or k < 1 or k > 1 << 20:
        raise ValueError("min_neighbours must be an integer in 1 .. 2^20")
    if N >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    half = np.float32(1 << 20)
    with np.errstate(all="ignore"):
        c = np.floor(p / rs)
        ok = np.isfinite(p).all(1) & (c >= -half).all(1) & (c < half).all(1)
    rows = np.nonzero(ok)[0]
    cell = c[ok].astype(np.int64) + (1 << 20)  # biased: 0 .. 2^21 - 1 on every axis
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    order = np.argsort(key, kind="stable")
    ks, ps = key[order], p[ok][order]  # the in-range points, cell by cell
    r2 = rs * rs
    found = np.zeros(len(ks), np.int64)
    for d in np.ndindex(3, 3, 3):
        q = cell[order] + (np.array(d, np.int64) - 1)
        inside = ((q >= 0) & (q < (1 << 21))).all(1)  # a key with a coordinate outside the grid is skipped
        qk = (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]
        lo = np.searchsorted(ks, qk, side="left")
        hi = np.where(inside, np.searchsorted(ks, qk, side="right"), lo)
        at = lo.copy()
        while True:  # step t of every bucket walk at once; rows that are saturated or through their bucket have left
            live = np.nonzero((at < hi) & (found < k))[0]
            if not len(live):
                break
            j = at[live]
            with np.errstate(all="ignore"):
                dx, dy, dz = (ps[j, a] - ps[live, a] for a in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                hit = (d2 <= r2) & (j != live)  # the row's own entry, by position: duplicates count
            found[live] += hit
            at[live] += 1
    neighbours = np.full(N, -1, np.int32)
    neighbours[rows[order]] = np.minimum(found, k).astype(np.int32)
    index = np.nonzero(neighbours == k)[0].astype(np.int32)
    if counts is None:
        bounds = np.array([0, N], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]), N)
    per_view = np.diff(np.searchsorted(index, bounds, side="left"))
    count = np.concatenate([per_view, [len(index)]]).astype(np.int32)
    take = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)[index]  # noqa: E731
    return HostOutliers(p[index], take(conf, np.float32, (N,)), take(rgb, np.uint8, (N, 3)), take(normals, np.float32, (N, 3)), index,
                        neighbours, count, int(N - ok.sum()))


@dataclass
class HostPlanes:
    plane: np.ndarray                # f32 [P,4]: n.x n.y n.z d of every plane found, zero rows behind them
    plane_count: np.ndarray          # int32 [P+1]: the inliers of every plane, then the planes found
    hypothesis: np.ndarray           # int32 [P]: the winning hypothesis, -1 behind the planes found
    label: np.ndarray                # int32 [N] over the input rows: the plane, -1 none, -2 a coordinate that is not finite
    dropped: int                     # rows with a coordinate that is not finite
    xyz: Optional[np.ndarray]        # mode 1 / 2: f32 [M,3] the rows without / of a plane, in ascending input row; None with mode 0
    conf: Optional[np.ndarray]       # f32 [M]
    rgb: Optional[np.ndarray]        # uint8 [M,3]
    normals: Optional[np.ndarray]    # f32 [M,3]
    index: Optional[np.ndarray]      # int32 [M]: the source row
    count: Optional[np.ndarray]      # int32 [B+1]: survivors per view, then their total


def _plane_of_rows(p0, p1, p2, axis, axis_min_cos):
    """The plane through three rows (f32 [3] each) -> f32 [4] n.x n.y n.z d, or None for an invalid triple (kernels/planes_math.h:
    plane_of_rows, line by line; every operation is one f32 operation)."""
    T = np.float32
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        nx = e1[1] * e2[2] - e1[2] * e2[1]
        ny = e1[2] * e2[0] - e1[0] * e2[2]
        nz = e1[0] * e2[1] - e1[1] * e2[0]
        len2 = (nx * nx + ny * ny) + nz * nz
        if not (np.isfinite(len2) and len2 > T(1e-30)):
            return None
        s = np.sqrt(len2)
        nx, ny, nz = nx / s, ny / s, nz / s
        d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2])
        flip = d < 0
        if d == 0:  # either zero: the first non-zero component of n decides
            first = nx if nx != 0 else (ny if ny != 0 else nz)
            flip = first < 0
        if flip:
            nx, ny, nz, d = -nx, -ny, -nz, -d
        if axis_min_cos > 0 and not np.abs((nx * axis[0] + ny * axis[1]) + nz * axis[2]) >= axis_min_cos:
            return None
    return np.array([nx, ny, nz, d], np.float32)


def fit_planes(xyz, planes=1, hypotheses=256, tol=0.0, min_inliers=3, seed=0, normals=None, normal_min_cos=0.0, axis=(0.0, 0.0, 0.0),
               axis_min_cos=0.0, mode=0, conf=None, rgb=None, counts=None) -> HostPlanes:
    """The host reference of md_op_fit_planes / md_infer_points_planes (include/mi_depth.h states the contract): `planes` rounds of
    RANSAC over the live rows of xyz f32 [N,3]. A round draws `hypotheses` triples from the live index with splitmix64's finaliser
    (`_smooth_mix64`), builds every triple's plane in f32, one rounded operation per step, counts the live rows within `tol` of it
    (and, with normal_min_cos > 0, with a normal within that cosine of the plane's), and the largest count, ties to the smallest
    hypothesis, takes its inliers out of the live set when it reaches min_inliers; a round that fails ends the call. Vectorised
    over the rows, one hypothesis at a time: the device kernels (kernels/planes.hip) give the same bits. mode 0 / "label": the
    labels only; 1 / "drop", 2 / "keep": also the rows without / of a plane, every given row copied unchanged. counts: the rows of
    every view of the input, [B] (default: one view)."""
    T = np.float32
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = len(p)
    P, Hh, k = int(planes), int(hypotheses), int(min_inliers)
    mode = {"label": 0, "drop": 1, "keep": 2}.get(mode, mode)
    tol, ncos, acos = T(tol), T(normal_min_cos), T(axis_min_cos)
    a = np.asarray(axis, np.float32).reshape(3)
    if not 1 <= P <= 8 or not 1 <= Hh <= 4096 or k < 3 or mode not in (0, 1, 2):
        raise ValueError("planes in 1..8, hypotheses in 1..4096, min_inliers >= 3, mode 0, 1 or 2")
    if not np.isfinite(tol) or not tol > 0 or not 0 <= ncos <= 1 or not 0 <= acos <= 1:
        raise ValueError("tol finite and > 0, normal_min_cos and axis_min_cos in [0, 1]")
    if ncos > 0 and normals is None:
        raise ValueError("normal_min_cos > 0 needs normals")
    if acos > 0 and not np.isfinite(a).all():
        raise ValueError("axis_min_cos > 0 needs a finite axis")
    if N >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    m = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(N, 3)
    ok = np.isfinite(p).all(1)
    label = np.where(ok, -1, -2).astype(np.int32)
    plane, plane_count, hypothesis = np.zeros((P, 4), np.float32), np.zeros(P + 1, np.int32), np.full(P, -1, np.int32)
    for r in range(P):
        live = np.nonzero(label == -1)[0]
        M = len(live)
        if M < 3:
            break
        word = (np.uint64(int(seed) & 0xFFFFFFFF) << np.uint64(32)) | (np.uint64(r) << np.uint64(28))
        h3 = (np.arange(Hh, dtype=np.uint64)[:, None] << np.uint64(2)) | np.arange(3, dtype=np.uint64)[None, :]
        pick = live[(_smooth_mix64(word | h3) % np.uint64(M)).astype(np.int64)]  # [Hh,3] rows
        q = p[live]
        qm = m[live] if ncos > 0 else None
        best, best_h, best_w, best_in = 0, -1, None, None
        for h in range(Hh):
            i0, i1, i2 = (int(v) for v in pick[h])
            if i0 == i1 or i0 == i2 or i1 == i2:
                continue
            w = _plane_of_rows(p[i0], p[i1], p[i2], a, acos)
            if w is None:
                continue
            with np.errstate(all="ignore"):
                inl = np.abs(((w[0] * q[:, 0] + w[1] * q[:, 1]) + w[2] * q[:, 2]) + w[3]) <= tol
                if ncos > 0:
                    inl &= np.abs((w[0] * qm[:, 0] + w[1] * qm[:, 1]) + w[2] * qm[:, 2]) >= ncos
            c = int(inl.sum())
            if c > best:  # ties: the smallest h stays
                best, best_h, best_w, best_in = c, h, w, inl
        if best < k:
            break
        plane[r], plane_count[r], hypothesis[r] = best_w, best, best_h
        plane_count[P] = r + 1
        label[live[best_in]] = r
    dropped = int(N - ok.sum())
    if mode == 0:
        return HostPlanes(plane, plane_count, hypothesis, label, dropped, None, None, None, None, None, None)
    index = np.nonzero(label == -1 if mode == 1 else label >= 0)[0].astype(np.int32)
    if counts is None:
        bounds = np.array([0, N], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]), N)
    per_view = np.diff(np.searchsorted(index, bounds, side="left"))
    count = np.concatenate([per_view, [len(index)]]).astype(np.int32)
    take = lambda v, dt, shape: None if v is None else np.ascontiguousarray(v, dtype=dt).reshape(shape)[index]  # noqa: E731
    return HostPlanes(plane, plane_count, hypothesis, label, dropped, p[index], take(conf, np.float32, (N,)), take(rgb, np.uint8, (N, 3)),
                      take(normals, np.float32, (N, 3)), index, count)


@dataclass
class HostRender:
    depth: np.ndarray                # f32 [T,H,W]: the winner's p.z, 0 at holes
    index: np.ndarray                # int32 [T,H,W]: the winner's row, -1 at holes
    rgb: Optional[np.ndarray]        # uint8 [T,H,W,3]: the winner's colour, 0 at holes
    filled: np.ndarray               # int32 [T+1]: filled pixels per target, then their total


@dataclass
class HostClusters:
    label: np.ndarray                # int32 [N] over the input rows: the smallest core row of the row's cluster, -1 noise, -2 dropped
    cluster_size: np.ndarray         # int32 [N]: core + border rows of the row's cluster, 0 for noise and dropped rows
    cluster: np.ndarray              # int32 [N]: the dense id of a kept cluster, -1 every other in-range row, -2 dropped
    table_label: np.ndarray          # int32 [min(C, table)]: the label of every kept cluster, ascending
    table_size: np.ndarray           # int32 [min(C, table)]
    box: np.ndarray                  # f32 [min(C, table),6]: min xyz, max xyz over the cluster's rows (-0 below +0)
    stats: np.ndarray                # int32 [4]: clusters found, clusters kept, noise rows, rows in kept clusters
    dropped: int                     # rows that are not finite or outside the grid
    xyz: Optional[np.ndarray]        # mode 1: f32 [M,3] the rows of kept clusters, in ascending input row; None with mode 0
    conf: Optional[np.ndarray]       # f32 [M]
    rgb: Optional[np.ndarray]        # uint8 [M,3]
    normals: Optional[np.ndarray]    # f32 [M,3]
    index: Optional[np.ndarray]      # int32 [M]: the source row
    count: Optional[np.ndarray]      # int32 [B+1]: survivors per view, then their total


def _neighbour_pairs(ks, cells, ps, r2):
    """The neighbour pairs of the in-range points sorted by cell key (ks keys, cells biased cells, ps positions), as a stream of
    (i, j) index arrays into that order, every ordered pair once: the 27 shifted lookups of `radius_outliers`, each bucket walked
    to its end."""
    for d in np.ndindex(3, 3, 3):
        q = cells + (np.array(d, np.int64) - 1)
        inside = ((q >= 0) & (q < (1 << 21))).all(1)  # a key with a coordinate outside the grid is skipped
        qk = (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2]
        lo = np.searchsorted(ks, qk, side="left")
        hi = np.where(inside, np.searchsorted(ks, qk, side="right"), lo)
        live = np.nonzero(lo < hi)[0]
        at = lo[live]
        while len(live):  # step t of every bucket walk at once
            with np.errstate(all="ignore"):
                dx, dy, dz = (ps[at, a] - ps[live, a] for a in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
                hit = (d2 <= r2) & (at != live)  # the row's own entry, by position: duplicates are neighbours
            yield live[hit], at[hit]
            at = at + 1
            go = at < hi[live]
            live, at = live[go], at[go]


def _ordered_keys(v: np.ndarray) -> np.ndarray:
    """The usual ordered key of an f32: the unsigned order of the keys is the numeric order of the floats, -0 below +0."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000))


def cluster_points(xyz, radius, min_neighbours=0, min_points=1, max_points=0, mode=0, table=None, conf=None, rgb=None, normals=None,
                   counts=None) -> HostClusters:
    """The host reference of md_op_cluster_points / md_infer_points_clusters (include/mi_depth.h states the contract): DBSCAN on
    the neighbour relation of `radius_outliers` (the 27 cells of side `radius` around a row's own AND d2 <= radius*radius in f32).
    A core row has at least min_neighbours neighbours; a cluster is a connected component of the core rows and is named by its
    smallest core row; a non-core row with a core neighbour takes the smallest label among them; the rest is noise (-1); rows
    that are not finite or outside the grid are dropped (-2). Kept clusters (min_points <= size, and size <= max_points unless
    that is 0) get dense ids in ascending label. mode 1 also returns the rows of kept clusters in input order. table: rows of
    the cluster table (default: all). The device kernels (kernels/clusters.hip) give the same bits. A sort by cell key for the
    pairs, labels by min-propagation with pointer jumping. counts: the rows of every view of the input, [B] (default: one view)."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    N = len(p)
    rs = np.float32(radius)
    k = int(min_neighbours)
    if not np.isfinite(rs) or not rs > 0:
        raise ValueError("radius must be finite and > 0")
    if k != min_neighbours or k < 0 or k > 1 << 20:
        raise ValueError("min_neighbours must be an integer in 0 .. 2^20")
    if int(min_points) != min_points or min_points < 1:
        raise ValueError("min_points must be an integer >= 1")
    if int(max_points) != max_points or max_points < 0 or 0 < max_points < min_points:
        raise ValueError("max_points must be 0 or an integer >= min_points")
    if mode not in (0, 1):
        raise ValueError("mode is 0 or 1")
    if table is not None and table < 0:
        raise ValueError("a negative table capacity")
    if N >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    half = np.float32(1 << 20)
    with np.errstate(all="ignore"):
        c = np.floor(p / rs)
        ok = np.isfinite(p).all(1) & (c >= -half).all(1) & (c < half).all(1)
    cell = c[ok].astype(np.int64) + (1 << 20)  # biased: 0 .. 2^21 - 1 on every axis
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    order = np.argsort(key, kind="stable")
    row = np.nonzero(ok)[0][order]  # the input row of every sorted point
    ks, cells, ps = key[order], cell[order], p[ok][order]
    r2 = rs * rs
    M = len(ks)
    core = np.ones(M, bool)
    if k > 0:
        found = np.zeros(M, np.int64)
        for i, _ in _neighbour_pairs(ks, cells, ps, r2):
            found += np.bincount(i, minlength=M)
        core = found >= k
    ei, ej = [], []  # the edges of the core graph, each once, in input rows
    for i, j in _neighbour_pairs(ks, cells, ps, r2):
        e = core[i] & core[j] & (row[j] < row[i])
        ei.append(row[i[e]])
        ej.append(row[j[e]])
    ei, ej = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (ei, ej))
    lab = np.arange(N, dtype=np.int64)  # over the input rows; only core rows are read
    while True:
        before = lab.copy()
        np.minimum.at(lab, ei, lab[ej])
        np.minimum.at(lab, ej, lab[ei])
        while True:  # pointer jumping: every row to the label of its label
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
        if (lab == before).all():
            break
    label = np.full(N, -2, np.int64)
    label[row] = np.where(core, lab[row], -1)
    if k > 0:
        best = np.full(M, N, np.int64)
        for i, j in _neighbour_pairs(ks, cells, ps, r2):
            e = ~core[i] & core[j]
            np.minimum.at(best, i[e], lab[row[j[e]]])
        border = ~core & (best < N)
        label[row[border]] = best[border]
    size_at = np.bincount(label[label >= 0], minlength=N) if N else np.zeros(0, np.int64)
    cluster_size = np.where(label >= 0, size_at[np.maximum(label, 0)], 0)
    kept_row = (cluster_size >= min_points) & ((max_points == 0) | (cluster_size <= max_points))
    roots = np.nonzero(label == np.arange(N))[0]
    kept_roots = roots[kept_row[roots]]  # ascending label
    dense = np.full(N, -1, np.int64)
    dense[kept_roots] = np.arange(len(kept_roots))
    cluster = np.where(label >= 0, np.where(kept_row, dense[np.maximum(label, 0)], -1), np.where(label == -2, -2, -1))
    stats = np.array([len(roots), len(kept_roots), (label == -1).sum(), kept_row.sum()], np.int32)
    T = len(kept_roots) if table is None else min(int(table), len(kept_roots))
    lo = np.full((T, 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((T, 3), np.uint32)
    boxed = np.nonzero((cluster >= 0) & (cluster < T))[0]
    keys = _ordered_keys(p[boxed])
    for a in range(3):
        np.minimum.at(lo[:, a], cluster[boxed], keys[:, a])
        np.maximum.at(hi[:, a], cluster[boxed], keys[:, a])
    bk = np.concatenate([lo, hi], 1)
    box = np.where(bk & np.uint32(0x80000000), bk ^ np.uint32(0x80000000), ~bk).astype(np.uint32).view(np.float32)
    out = HostClusters(label.astype(np.int32), cluster_size.astype(np.int32), cluster.astype(np.int32), kept_roots[:T].astype(np.int32),
                       size_at[kept_roots[:T]].astype(np.int32), box, stats, int(N - ok.sum()), None, None, None, None, None, None)
    if mode == 0:
        return out
    index = np.nonzero(cluster >= 0)[0].astype(np.int32)
    if counts is None:
        bounds = np.array([0, N], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]), N)
    per_view = np.diff(np.searchsorted(index, bounds, side="left"))
    take = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)[index]  # noqa: E731
    out.xyz, out.conf, out.rgb, out.normals = p[index], take(conf, np.float32, (N,)), take(rgb, np.uint8, (N, 3)), take(normals, np.float32, (N, 3))
    out.index, out.count = index, np.concatenate([per_view, [len(index)]]).astype(np.int32)
    return out


@dataclass
class HostMatch:
    nearest: np.ndarray              # int32 [N] over the input rows: the nearest target row within the radius, -1 none, -2 dropped
    dist2: np.ndarray                # f32 [N]: its squared distance; the bit pattern 0x7F800000 for -1 and -2 rows
    stats: np.ndarray                # int32 [8]: in-range rows, matched rows, target rows in the grid, 0, rows within tol[0..4)
    dropped: int                     # source rows that are not finite or outside the grid
    xyz: Optional[np.ndarray]        # mode 1 / 2: f32 [M,3] the matched / unmatched rows, in ascending input row; None with mode 0
    conf: Optional[np.ndarray]       # f32 [M]
    rgb: Optional[np.ndarray]        # uint8 [M,3]
    normals: Optional[np.ndarray]    # f32 [M,3]
    index: Optional[np.ndarray]      # int32 [M]: the source row
    count: Optional[np.ndarray]      # int32 [B+1]: survivors per view, then their total


def _grid_cells(p, rs):
    """The outlier removal's cells of the rows p f32 [N,3] at side rs -> (in range [N] bool, biased cells of the in-range rows
    int64 [M,3], their keys int64 [M])."""
    half = np.float32(1 << 20)
    with np.errstate(all="ignore"):
        c = np.floor(p / rs)
        ok = np.isfinite(p).all(1) & (c >= -half).all(1) & (c < half).all(1)
    cell = c[ok].astype(np.int64) + (1 << 20)  # biased: 0 .. 2^21 - 1 on every axis
    return ok, cell, (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]


def _match_grid(q, rs):
    """The matching's grid of the target q f32 [T,3] at cell side rs -> (in range [T] bool, sorted cell keys, the rows in that
    order, their target rows uint64). The target is sorted by cell key."""
    t_ok, _, t_key = _grid_cells(q, rs)
    order = np.argsort(t_key, kind="stable")
    trow = np.nonzero(t_ok)[0][order].astype(np.uint64)  # the target row of every sorted entry
    return t_ok, t_key[order], q[t_ok][order], trow


def _match_nearest(p, grid, rs, r2):
    """The matching's walk of the rows p f32 [N,3] through `grid` -> (in range [N] bool, the in-range rows, their smallest key
    (bits(d2) << 32) | target row over the candidates within r2, all ones without one). Every row makes 27 lookups and walks
    the buckets, all rows at once."""
    _, ks, ts, trow = grid
    ok, cells, _ = _grid_cells(p, rs)
    src = np.nonzero(ok)[0]
    ps = p[src]
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(len(src), none, np.uint64)
    for d in np.ndindex(3, 3, 3):
        c = cells + (np.array(d, np.int64) - 1)
        inside = ((c >= 0) & (c < (1 << 21))).all(1)  # a key with a coordinate outside the grid is skipped
        qk = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
        lo = np.searchsorted(ks, qk, side="left")
        hi = np.where(inside, np.searchsorted(ks, qk, side="right"), lo)
        live = np.nonzero(lo < hi)[0]
        at = lo[live]
        while len(live):  # step t of every bucket walk at once
            with np.errstate(all="ignore"):
                dx, dy, dz = (ts[at, a] - ps[live, a] for a in range(3))
                d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float32)
            hit = d2 <= r2
            key = (d2[hit].view(np.uint32).astype(np.uint64) << np.uint64(32)) | trow[at[hit]]
            best[live[hit]] = np.minimum(best[live[hit]], key)  # a row appears once per step
            at = at + 1
            go = at < hi[live]
            live, at = live[go], at[go]
    return ok, src, best


def match_points(xyz, target, radius, tol=(), mode=0, conf=None, rgb=None, normals=None, counts=None) -> HostMatch:
    """The host reference of md_op_match_points / md_infer_points_match (include/mi_depth.h states the contract): for every row of
    xyz [N,3] the nearest row of target [T,3] among its candidates: the target rows whose cell (side `radius`, the cells of
    `radius_outliers`) differs from the row's by at most 1 on every axis AND whose d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius
    in f32. The nearest has the smallest key (bits(d2) << 32) | target row; -1 without a candidate, -2 for a row that is not
    finite or outside the grid. tol: up to four tolerances in (0, radius] (0: unused); stats[4 + t] counts the matched rows with
    d2 <= tol[t]*tol[t]. mode 1 / 2 also returns the matched / unmatched in-range rows in input order. The device kernels
    (kernels/match.hip) give the same bits. The target is sorted by cell key; every source row makes 27 lookups and walks the
    buckets, all rows at once. counts: the rows of every view of the input, [B] (default: one view)."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    N, T = len(p), len(q)
    rs = np.float32(radius)
    with np.errstate(all="ignore"):
        r2 = rs * rs
    if not np.isfinite(rs) or not rs > 0 or not np.isfinite(r2):
        raise ValueError("radius and its square must be finite and > 0")
    tols = np.zeros(4, np.float32)
    if len(tol) > 4:
        raise ValueError("at most four tolerances")
    tols[:len(tol)] = np.asarray(tol, np.float32)
    if not (tols >= 0).all() or not (tols <= rs).all():
        raise ValueError("a tolerance is 0 or lies in (0, radius]")
    if mode not in (0, 1, 2):
        raise ValueError("mode is 0, 1 or 2")
    if N >= 1 << 30 or T >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    grid = _match_grid(q, rs)
    t_ok = grid[0]
    ok, src, best = _match_nearest(p, grid, rs, r2)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    found = best != none
    nearest = np.full(N, -2, np.int32)
    nearest[src] = np.where(found, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    bits = np.full(N, 0x7F800000, np.uint32)
    bits[src] = np.where(found, (best >> np.uint64(32)).astype(np.uint32), np.uint32(0x7F800000))
    dist2 = bits.view(np.float32)
    stats = np.zeros(8, np.int32)
    stats[0], stats[1], stats[2] = len(src), int(found.sum()), int(t_ok.sum())
    matched = nearest >= 0
    for t in range(4):
        if tols[t] > 0:
            stats[4 + t] = int((matched & (dist2 <= tols[t] * tols[t])).sum())
    out = HostMatch(nearest, dist2, stats, int(N - ok.sum()), None, None, None, None, None, None)
    if mode == 0:
        return out
    index = np.nonzero(matched if mode == 1 else nearest == -1)[0].astype(np.int32)
    if counts is None:
        bounds = np.array([0, N], np.int64)
    else:
        bounds = np.minimum(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64).reshape(-1))]), N)
    per_view = np.diff(np.searchsorted(index, bounds, side="left"))
    take = lambda a, dt, shape: None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(shape)[index]  # noqa: E731
    out.xyz, out.conf, out.rgb, out.normals = p[index], take(conf, np.float32, (N,)), take(rgb, np.uint8, (N, 3)), take(normals, np.float32, (N, 3))
    out.index, out.count = index, np.concatenate([per_view, [len(index)]]).astype(np.int32)
    return out


@dataclass
class HostRegistration:
    transform: np.ndarray            # f64 [12]: R row-major, then t
    pairs: np.ndarray                # int32 [K+1]: the pair count of every pass, entry K the evaluation pass; 0 for skipped iterations
    sum_d2: np.ndarray               # f64 [K+1]: the sum of squared distances likewise
    stats: np.ndarray                # int32 [8]: solves done, status, in-range rows and pairs of the evaluation pass, target rows in the grid
    dropped: int                     # rows whose moved row is not finite or outside the grid in the evaluation pass
    nearest: np.ndarray              # int32 [N]: match_points' nearest of the moved rows of the evaluation pass
    dist2: np.ndarray                # f32 [N]
    xyz: np.ndarray                  # f32 [N,3]: the moved rows of the evaluation pass
    normals: Optional[np.ndarray]    # f32 [N,3]: the rotated normals
    sum_r2: Optional[np.ndarray] = None  # f64 [K+1]: the sum of squared point-to-plane residuals; with target_normals only


REG_SWEEPS = 8     # kRegSweeps of kernels/register_math.h
_REG_TILE = 4096   # tile_compact.h: item = tile * 4096 + step * 256 + thread


def _reg_workgroup(v):
    """The value of a 256-thread workgroup, v f64 [.., 256, L] -> [.., L]: the halving tree over the 64 lanes of every wave,
    then (W0 + W1) + (W2 + W3)."""
    w = v.reshape(v.shape[:-2] + (4, 64, v.shape[-1]))
    h = 32
    while h >= 1:
        w = w[..., :h, :] + w[..., h:2 * h, :]
        h //= 2
    w = w[..., 0, :]
    return (w[..., 0, :] + w[..., 1, :]) + (w[..., 2, :] + w[..., 3, :])


def _reg_sums(leaves):
    """The L sums of a pass in the contract's fixed shape (L = 16, or 29 in the point-to-plane form). leaves f64 [tiles * 4096, L]
    in item order, +0.0 where an item has no pair."""
    tiles, L = len(leaves) // _REG_TILE, leaves.shape[1]
    v = leaves.reshape(tiles, 16, 256, L)
    acc = np.zeros((tiles, 256, L), np.float64)
    for s in range(16):  # a thread's left fold over its steps
        acc = acc + v[:, s]
    tile = _reg_workgroup(acc)
    rounds = (tiles + 255) // 256
    part = np.zeros((max(rounds, 1) * 256, L), np.float64)
    part[:tiles] = tile
    part = part.reshape(-1, 256, L)
    acc = np.zeros((256, L), np.float64)
    for r in range(len(part)):  # thread u folds the tiles u, u + 256, ..
        acc = acc + part[r]
    return _reg_workgroup(acc)


def _reg_rotate(a, v, p, q):
    """reg_jacobi_rotate of kernels/register_math.h, line for line, on lists of np.float64."""
    f = np.float64
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (f(2.0) * apq)
    sign = f(1.0) if theta >= 0.0 else f(-1.0)
    t = sign / (np.abs(theta) + np.sqrt(theta * theta + f(1.0)))
    c = f(1.0) / np.sqrt(t * t + f(1.0))
    s = t * c
    for k in range(4):
        akp, akq = a[k][p], a[k][q]
        a[k][p] = c * akp - s * akq
        a[k][q] = s * akp + c * akq
    for k in range(4):
        apk, aqk = a[p][k], a[q][k]
        a[p][k] = c * apk - s * aqk
        a[q][k] = s * apk + c * aqk
    for k in range(4):
        vkp, vkq = v[k][p], v[k][q]
        v[k][p] = c * vkp - s * vkq
        v[k][q] = s * vkp + c * vkq


def _reg_quat_matrix(w, x, y, z):
    """reg_quat_matrix of kernels/register_math.h, line for line: the unit quaternion -> R row-major, a list of nine np.float64."""
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    xy, xz, yz, wx, wy, wz = x * y, x * z, y * z, w * x, w * y, w * z
    two = np.float64(2.0)
    return [((ww + xx) - yy) - zz, two * (xy - wz), two * (xz + wy),
            two * (xy + wz), ((ww - xx) + yy) - zz, two * (yz - wx),
            two * (xz - wy), two * (yz + wx), ((ww - xx) - yy) + zz]


REG_PLANE_LEAVES = 29  # kRegPlaneLeaves of kernels/register_math.h


def register_solve_plane(n, S, A_old):
    """reg_solve_plane of kernels/register_math.h, line for line: the usable pair count n, the 29 sums S and the transform the
    pass ran under -> the composed transform f64 [12], or None when the system is degenerate (a Cholesky pivot that is not > 0,
    or a component of the solution that is not finite)."""
    f = np.float64
    S = [f(v) for v in S]
    A_old = [f(v) for v in A_old]
    with np.errstate(all="ignore"):
        M = [[f(0.0)] * 6 for _ in range(6)]
        L = [[f(0.0)] * 6 for _ in range(6)]
        at = 0
        for i in range(6):
            for j in range(i, 6):
                M[i][j] = M[j][i] = S[at]
                at += 1
        for j in range(6):
            s = M[j][j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            if not s > 0.0:
                return None
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, 6):
                v = M[i][j]
                for k in range(j):
                    v = v - L[i][k] * L[j][k]
                L[i][j] = v / L[j][j]
        x, y = [f(0.0)] * 6, [f(0.0)] * 6
        for i in range(6):
            v = S[21 + i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v / L[i][i]
        for i in range(5, -1, -1):
            v = y[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * x[k]
            x[i] = v / L[i][i]
        if not all(np.isfinite(v) for v in x):
            return None
        qx, qy, qz = f(0.5) * x[0], f(0.5) * x[1], f(0.5) * x[2]
        ln = np.sqrt(((f(1.0) + qx * qx) + qy * qy) + qz * qz)
        qw = f(1.0) / ln
        qx, qy, qz = qx / ln, qy / ln, qz / ln
        dR = _reg_quat_matrix(qw, qx, qy, qz)
        A = [f(0.0)] * 12
        for a in range(3):
            for b in range(3):
                A[3 * a + b] = (dR[3 * a] * A_old[b] + dR[3 * a + 1] * A_old[3 + b]) + dR[3 * a + 2] * A_old[6 + b]
            A[9 + a] = ((dR[3 * a] * A_old[9] + dR[3 * a + 1] * A_old[10]) + dR[3 * a + 2] * A_old[11]) + x[3 + a]
    return np.array(A, np.float64)


def register_solve(n, S, sweeps=REG_SWEEPS):
    """reg_solve of kernels/register_math.h, line for line: the pair count n and the sixteen sums S -> the transform f64 [12]."""
    f = np.float64
    S = [f(x) for x in S]
    with np.errstate(all="ignore"):
        dn = f(n)
        pbar = [S[a] / dn for a in range(3)]
        qbar = [S[3 + b] / dn for b in range(3)]
        H = [[S[6 + 3 * a + b] - S[a] * qbar[b] for b in range(3)] for a in range(3)]
        m = [[f(0.0)] * 4 for _ in range(4)]
        m[0][0] = (H[0][0] + H[1][1]) + H[2][2]
        m[1][1] = (H[0][0] - H[1][1]) - H[2][2]
        m[2][2] = (H[1][1] - H[0][0]) - H[2][2]
        m[3][3] = (H[2][2] - H[0][0]) - H[1][1]
        m[0][1] = m[1][0] = H[1][2] - H[2][1]
        m[0][2] = m[2][0] = H[2][0] - H[0][2]
        m[0][3] = m[3][0] = H[0][1] - H[1][0]
        m[1][2] = m[2][1] = H[0][1] + H[1][0]
        m[1][3] = m[3][1] = H[2][0] + H[0][2]
        m[2][3] = m[3][2] = H[1][2] + H[2][1]
        v = [[f(1.0) if i == j else f(0.0) for j in range(4)] for i in range(4)]
        for _ in range(sweeps):
            for p in range(3):
                for q in range(p + 1, 4):
                    _reg_rotate(m, v, p, q)
        top = 0
        for k in range(1, 4):
            if m[k][k] > m[top][top]:
                top = k
        w, x, y, z = v[0][top], v[1][top], v[2][top], v[3][top]
        ln = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / ln, x / ln, y / ln, z / ln
        if w < 0.0:
            w, x, y, z = -w, -x, -y, -z
        A = _reg_quat_matrix(w, x, y, z)
        A += [qbar[a] - ((A[3 * a] * pbar[0] + A[3 * a + 1] * pbar[1]) + A[3 * a + 2] * pbar[2]) for a in range(3)]
    return np.array(A, np.float64)


def _reg_turn(A, v, shift):
    """(float)(((R_a0 x + R_a1 y) + R_a2 z) [+ t_a]) of the rows v f32 [N,3], a NaN written as 0x7FC00000."""
    x, y, z = (v[:, a].astype(np.float64) for a in range(3))
    out = np.empty((len(v), 3), np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            r = (A[3 * a] * x + A[3 * a + 1] * y) + A[3 * a + 2] * z
            out[:, a] = ((r + A[9 + a]) if shift else r).astype(np.float32)
    bits = out.view(np.uint32)
    bits[np.isnan(out)] = 0x7FC00000
    return out


def register_points(xyz, target, radius, iterations=10, init=None, min_pairs=None, rot_eps=0.0, trans_eps=0.0, normals=None,
                    target_normals=None) -> HostRegistration:
    """The host reference of md_op_register_points (include/mi_depth.h states the contract, kernels/register_math.h its arithmetic):
    rigid point-to-point ICP of xyz [N,3] onto target [T,3]. Every pass moves the rows under the running transform in f64 with one
    cast to f32, pairs them through `match_points`' grid and walk, and sums the sixteen leaves of every pair in the fixed tree of
    the tile layout; `register_solve` restates the Jacobi solve. init: twelve f64, R row-major then t (None: the identity). The
    device kernels (kernels/register.hip) give the same bits. min_pairs: None is the smallest the form takes, 3, or 6 with
    target_normals. target_normals [T,3]: the point-to-plane form of md_op_register_points_plane: the 29 leaves of every usable
    pair (a target normal that is finite and not all zero) from the MOVED row, `register_solve_plane`, status 3 for a degenerate
    system, `sum_r2`; pairs, sum_d2 and stats[3] then cover the usable pairs only."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    N, T, K = len(p), len(q), int(iterations)
    plane = target_normals is not None
    if min_pairs is None:
        min_pairs = 6 if plane else 3
    if plane:
        tn = np.ascontiguousarray(target_normals, dtype=np.float32).reshape(-1, 3)
        if len(tn) != T:
            raise ValueError("target_normals is [T,3]")
        if min_pairs < 6:
            raise ValueError("min_pairs is at least 6 in the point-to-plane form")
        tn_ok = np.isfinite(tn).all(1) & (tn != 0).any(1)
        tn64 = tn.astype(np.float64)
    rs = np.float32(radius)
    with np.errstate(all="ignore"):
        r2 = rs * rs
    if not np.isfinite(rs) or not rs > 0 or not np.isfinite(r2):
        raise ValueError("radius and its square must be finite and > 0")
    if not 1 <= K <= 64:
        raise ValueError("iterations outside 1..64")
    if min_pairs < 3:
        raise ValueError("min_pairs is at least 3")
    if not (np.isfinite(rot_eps) and rot_eps >= 0 and np.isfinite(trans_eps) and trans_eps >= 0):
        raise ValueError("rot_eps and trans_eps are finite and >= 0")
    A = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64) if init is None else np.asarray(init, np.float64).reshape(12).copy()
    if not np.isfinite(A).all():
        raise ValueError("init is not finite")
    if N >= 1 << 30 or T >= 1 << 30:
        raise ValueError("fewer than 2^30 rows")
    grid = _match_grid(q, rs)
    items = (N + _REG_TILE - 1) // _REG_TILE * _REG_TILE
    p64, q64 = p.astype(np.float64), q.astype(np.float64)

    def one_pass(A):
        moved = _reg_turn(A, p, True)
        ok, src, best = _match_nearest(moved, grid, rs, r2)
        found = best != np.uint64(0xFFFFFFFFFFFFFFFF)
        rows, j = src[found], (best[found] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2 = (best[found] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        if plane:  # reg_add_plane_leaves, one rounded operation per step
            use = tn_ok[j]
            rows, j, d2 = rows[use], j[use], d2[use]
            leaves = np.zeros((items, REG_PLANE_LEAVES), np.float64)
            with np.errstate(all="ignore"):
                m, n = moved[rows].astype(np.float64), tn64[j]
                J = np.empty((len(rows), 6), np.float64)
                J[:, 0] = m[:, 1] * n[:, 2] - m[:, 2] * n[:, 1]
                J[:, 1] = m[:, 2] * n[:, 0] - m[:, 0] * n[:, 2]
                J[:, 2] = m[:, 0] * n[:, 1] - m[:, 1] * n[:, 0]
                J[:, 3:] = n
                d = q64[j] - m
                r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
                at = 0
                for a in range(6):
                    for b in range(a, 6):
                        leaves[rows, at] = J[:, a] * J[:, b]
                        at += 1
                leaves[rows, 21:27] = J * r[:, None]
                leaves[rows, 27] = r * r
            leaves[rows, 28] = d2.astype(np.float64)
            return moved, ok, src, best, found, len(rows), _reg_sums(leaves)
        leaves = np.zeros((items, 16), np.float64)
        leaves[rows, 0:3], leaves[rows, 3:6] = p64[rows], q64[j]
        leaves[rows, 6:15] = (p64[rows][:, :, None] * q64[j][:, None, :]).reshape(-1, 9)
        leaves[rows, 15] = d2.astype(np.float64)
        return moved, ok, src, best, found, len(rows), _reg_sums(leaves)

    pairs, sum_d2, stats = np.zeros(K + 1, np.int32), np.zeros(K + 1, np.float64), np.zeros(8, np.int32)
    sum_r2 = np.zeros(K + 1, np.float64) if plane else None
    for k in range(K):
        if stats[1] != 0:
            break
        n, S = one_pass(A)[5:]
        pairs[k], sum_d2[k] = n, S[28 if plane else 15]
        if plane:
            sum_r2[k] = S[27]
        if n < min_pairs:
            stats[1] = 2
            break
        A_new = register_solve_plane(n, S, A) if plane else register_solve(n, S)
        if A_new is None:
            stats[1] = 3
            break
        stats[0] += 1
        if (rot_eps > 0 or trans_eps > 0) and np.abs(A_new[:9] - A[:9]).max() <= rot_eps and np.abs(A_new[9:] - A[9:]).max() <= trans_eps:
            stats[1] = 1
        A = A_new
    moved, ok, src, best, found, n, S = one_pass(A)
    pairs[K], sum_d2[K] = n, S[28 if plane else 15]
    if plane:
        sum_r2[K] = S[27]
    stats[2], stats[3], stats[4] = len(src), n, int(grid[0].sum())
    nearest = np.full(N, -2, np.int32)
    nearest[src] = np.where(found, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    bits = np.full(N, 0x7F800000, np.uint32)
    bits[src] = np.where(found, (best >> np.uint64(32)).astype(np.uint32), np.uint32(0x7F800000))
    turned = None if normals is None else _reg_turn(A, np.ascontiguousarray(normals, dtype=np.float32).reshape(N, 3), False)
    return HostRegistration(A, pairs, sum_d2, stats, int(N - ok.sum()), nearest, bits.view(np.float32), moved, turned, sum_r2)


def render_points(xyz, H, W, intrinsics=None, extrinsics=None, focal_px=None, rgb=None, count=None, *, pixel_offset=0.0, z_near=0.0,
                  z_far=0.0, radius=0) -> HostRender:
    """The host reference of md_op_render_points / md_infer_points_render (include/mi_depth.h states the contract): the list xyz
    [N,3] (its first min(max(count, 0), N) rows) projected into T target cameras (intrinsics [T,3,3] or focal_px [T]; extrinsics
    [T,3,4] world-to-camera, None = the points are in the camera's frame) and z-buffered over the (2 radius + 1)^2 footprint:
    a pixel keeps the smallest key (bits(p.z) << 32) | row. f32, one rounded operation per step: the device kernels
    (kernels/render.hip) give the same bits."""
    T32 = np.float32
    p = np.ascontiguousarray(xyz, dtype=T32).reshape(-1, 3)
    N = len(p)
    H, W, radius = int(H), int(W), int(radius)
    if intrinsics is not None:
        K = np.asarray(intrinsics, dtype=T32).reshape(-1, 3, 3)
        fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    elif focal_px is not None:
        fx = fy = np.asarray(focal_px, dtype=T32).reshape(-1)
        cx, cy = np.full(len(fx), T32(W) / T32(2), T32), np.full(len(fx), T32(H) / T32(2), T32)
    else:
        raise ValueError("neither intrinsics nor a focal length")
    T = len(fx)
    E = None if extrinsics is None else np.asarray(extrinsics, dtype=T32).reshape(T, 3, 4)
    if T <= 0 or H <= 0 or W <= 0 or T * H * W >= 1 << 31 or H >= 1 << 24 or W >= 1 << 24 or N >= 1 << 31:
        raise ValueError("invalid shape")
    if not 0 <= radius <= 16:
        raise ValueError("radius outside 0..16")
    if not all(np.isfinite(v) for v in (pixel_offset, z_near, z_far)) or z_near < 0 or z_far < 0 or (z_near > 0 and 0 < z_far < z_near):
        raise ValueError("pixel_offset and the bounds must be finite, the bounds >= 0 and z_far >= z_near")
    f32i = np.finfo(np.float32)
    zn = T32(z_near) if z_near > 0 else T32(f32i.tiny)
    zf = T32(z_far) if z_far > 0 else T32(f32i.max)
    n = N if count is None else min(max(int(count), 0), N)
    x, y, z = p[:n, 0], p[:n, 1], p[:n, 2]
    row = np.arange(n, dtype=np.uint64)
    off, half = T32(pixel_offset), T32(0.5)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full((T, H * W), empty, np.uint64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(p[:n]).all(1)
        for j in range(T):
            if E is None:
                px, py, pz = x, y, z
            else:
                px, py, pz = [((E[j, a, 0] * x + E[j, a, 1] * y) + E[j, a, 2] * z) + E[j, a, 3] for a in range(3)]
            uf = ((fx[j] * (px / pz)) + cx[j]) - off
            vf = ((fy[j] * (py / pz)) + cy[j]) - off
            uu, vv = np.floor(uf + half), np.floor(vf + half)
            seen = fin & np.isfinite(pz) & (pz >= zn) & (pz <= zf) & (uu >= 0) & (uu < T32(W)) & (vv >= 0) & (vv < T32(H))
            ui, vi = uu[seen].astype(np.int64), vv[seen].astype(np.int64)
            key = (np.ascontiguousarray(pz[seen], dtype=T32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | row[seen]
            for dv in range(-radius, radius + 1):
                for du in range(-radius, radius + 1):
                    vy, ux = vi + dv, ui + du
                    ok = (vy >= 0) & (vy < H) & (ux >= 0) & (ux < W)
                    np.minimum.at(keys[j], vy[ok] * W + ux[ok], key[ok])
    keys = keys.reshape(T, H, W)
    hit = keys != empty
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(T32), T32(0)).astype(T32)
    index = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    color = None
    if rgb is not None:
        c = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(N, 3)
        color = np.zeros((T, H, W, 3), np.uint8)
        color[hit] = c[index[hit]]
    filled = np.concatenate([hit.reshape(T, -1).sum(1), [hit.sum()]]).astype(np.int32)
    return HostRender(depth, index, color, filled)


def pixel_index(mask, stride: int = 1) -> np.ndarray:
    """The host reference of `pixel_index` (md_points_mesh, include/mi_depth.h): mask [B,H,W] (the validity mask of the point path,
    or a `HostPoints`) -> int32 [B,H,W], the row of every pixel in the compacted list (valid pixels of the strided lattice in
    (view, row, column) order), -1 where the pixel is not in it."""
    m = np.asarray(mask.mask if isinstance(mask, HostPoints) else mask)
    if m.ndim != 3:
        raise ValueError(f"expected a mask [B,H,W], got {m.shape}")
    if stride < 1:
        raise ValueError("stride must be at least 1")
    sel = np.zeros(m.shape, bool)
    sel[:, ::stride, ::stride] = m[:, ::stride, ::stride] != 0
    flat = sel.reshape(-1)
    return np.where(flat, np.cumsum(flat, dtype=np.int64) - 1, -1).astype(np.int32).reshape(m.shape)


def mesh_grid(depth, pixel_index, stride: int = 1, max_rtol: float = 0.0, vertex_limit: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The host reference of md_op_mesh_grid / md_op_unproject_mesh / md_infer_points_mesh (include/mi_depth.h states the
    contract): depth [B,H,W] and the map pixel -> list row int32 [B,H,W] -> (faces int32 [F,3], face_count int32 [B+1]). The
    quads of the strided lattice, each split along the diagonal with the smaller depth difference (or the one its usable corners
    allow) into two triangles of camera-facing winding; a triangle is emitted when its corners have an index in [0, vertex_limit)
    (0 = no limit) and, with max_rtol > 0, |dx - dy| <= max_rtol * min(dx, dy) holds on its three edges. The comparisons are f32,
    one rounded operation per step, so the faces are the device's bit for bit; the order is (view, row, column, triangle)."""
    d = np.asarray(depth, dtype=np.float32)
    pi = np.asarray(pixel_index)
    if d.ndim != 3 or pi.shape != d.shape:
        raise ValueError(f"expected depth and pixel_index [B,H,W], got {d.shape} and {pi.shape}")
    if not np.issubdtype(pi.dtype, np.integer):
        raise ValueError("pixel_index must be an integer map")
    if stride < 1:
        raise ValueError("stride must be at least 1")
    if not np.isfinite(max_rtol) or max_rtol < 0:
        raise ValueError("max_rtol must be finite and >= 0")
    if vertex_limit < 0:
        raise ValueError("vertex_limit must be >= 0")
    B = d.shape[0]
    dn, pn = d[:, ::stride, ::stride], pi[:, ::stride, ::stride].astype(np.int64)
    corner = lambda a: (a[:, :-1, :-1], a[:, :-1, 1:], a[:, 1:, :-1], a[:, 1:, 1:])  # noqa: E731  a, b, c, d
    ia, ib, ic, id_ = corner(pn)
    da, db, dc, dd = corner(dn)
    use = lambda i: (i >= 0) & ((i < vertex_limit) if vertex_limit else True)  # noqa: E731
    ua, ub, uc, ud = use(ia), use(ib), use(ic), use(id_)
    rt = np.float32(max_rtol)
    with np.errstate(all="ignore"):
        def edge(dx, dy):
            if max_rtol == 0:
                return np.ones(dx.shape, bool)
            return np.abs(dx - dy) <= rt * np.fmin(dx, dy)

        ad = np.where(ua & ub & uc & ud, np.abs(da - dd) <= np.abs(db - dc), ua & ud)
        # a-d: (a, c, d), (a, d, b); b-c: (a, c, b), (b, c, d)
        first = np.where(ad, ua & uc & ud & edge(da, dc) & edge(dc, dd) & edge(dd, da), ua & uc & ub & edge(da, dc) & edge(dc, db) & edge(db, da))
        second = np.where(ad, ua & ud & ub & edge(da, dd) & edge(dd, db) & edge(db, da), ub & uc & ud & edge(db, dc) & edge(dc, dd) & edge(dd, db))
    tri = np.stack([np.stack([ia, ic, np.where(ad, id_, ib)], -1),
                    np.stack([np.where(ad, ia, ib), np.where(ad, id_, ic), np.where(ad, ib, id_)], -1)], -2)  # [B,Hq,Wq,2,3]
    emit = np.stack([first, second], -1)
    count = np.concatenate([emit.reshape(B, -1).sum(1), [emit.sum()]]).astype(np.int32)
    return tri[emit].astype(np.int32).reshape(-1, 3), count


@dataclass
class HostRaster:
    depth: np.ndarray                # f32 [T,H,W]: the winner's interpolated z, 0 at holes
    face: np.ndarray                 # int32 [T,H,W]: the winning face, -1 at holes
    rgb: Optional[np.ndarray]        # uint8 [T,H,W,3]: the winner's colour, affine in screen space, 0 at holes
    filled: np.ndarray               # int32 [T+1]: filled pixels per target, then their total
    skipped: np.ndarray              # int32 [T+1]: faces dropped for a box beyond max_extent per target, then their total


def render_mesh(xyz, faces, H, W, intrinsics=None, extrinsics=None, focal_px=None, rgb=None, face_count=None, *, pixel_offset=0.0,
                z_near=0.0, z_far=0.0, cull=0, max_extent=0) -> HostRaster:
    """The host reference of md_op_render_mesh / md_infer_points_raster (include/mi_depth.h states the contract, step by step): the
    faces int [F,3] (the first min(max(face_count, 0), F)) over the rows of xyz [N,3] rasterised into T target cameras (intrinsics
    [T,3,3] or focal_px [T]; extrinsics [T,3,4] world-to-camera, None = the points are in the camera's frame). The vertices are
    projected as `render_points` projects, snapped to 1/256 pixel, covered pixels found in int64, their depth from one f64 division
    and rounded f32 operations; a pixel keeps the smallest key (bits(z) << 32) | face. The colour is affine in screen space. The
    device kernels (kernels/raster.hip) give the same bits."""
    T32, I64 = np.float32, np.int64
    p = np.ascontiguousarray(xyz, dtype=T32).reshape(-1, 3)
    fc = np.asarray(faces).reshape(-1, 3).astype(I64)
    N, F = len(p), len(fc)
    H, W, max_extent = int(H), int(W), int(max_extent)
    if intrinsics is not None:
        K = np.asarray(intrinsics, dtype=T32).reshape(-1, 3, 3)
        fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    elif focal_px is not None:
        fx = fy = np.asarray(focal_px, dtype=T32).reshape(-1)
        cx, cy = np.full(len(fx), T32(W) / T32(2), T32), np.full(len(fx), T32(H) / T32(2), T32)
    else:
        raise ValueError("neither intrinsics nor a focal length")
    T = len(fx)
    E = None if extrinsics is None else np.asarray(extrinsics, dtype=T32).reshape(T, 3, 4)
    if T <= 0 or H <= 0 or W <= 0 or T * H * W >= 1 << 31 or H >= 1 << 24 or W >= 1 << 24 or N >= 1 << 31 or F >= 1 << 31:
        raise ValueError("invalid shape")
    if cull not in (0, 1):
        raise ValueError("cull is 0 or 1")
    if not 0 <= max_extent <= 1024:
        raise ValueError("max_extent outside 0..1024")
    if not all(np.isfinite(v) for v in (pixel_offset, z_near, z_far)) or z_near < 0 or z_far < 0 or (z_near > 0 and 0 < z_far < z_near):
        raise ValueError("pixel_offset and the bounds must be finite, the bounds >= 0 and z_far >= z_near")
    extent = max_extent or 64
    f32i = np.finfo(np.float32)
    zn = T32(z_near) if z_near > 0 else T32(f32i.tiny)
    zf = T32(z_far) if z_far > 0 else T32(f32i.max)
    n = F if face_count is None else min(max(int(face_count), 0), F)
    fc = fc[:n]
    off, half, sub, one, guard = T32(pixel_offset), T32(0.5), T32(256), T32(1), T32(16777216)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full((T, H * W), empty, np.uint64)
    skipped = np.zeros(T + 1, np.int64)
    col = None if rgb is None else np.ascontiguousarray(rgb, dtype=np.uint8).reshape(N, 3)
    setups = []

    def weights(X, Y, sign, px, py):  # step 6: int64 [m] each
        e = lambda a, b: (X[:, b] - X[:, a]) * (py - Y[:, a]) - (Y[:, b] - Y[:, a]) * (px - X[:, a])  # noqa: E731
        return sign * e(1, 2), sign * e(2, 0), sign * e(0, 1)

    with np.errstate(all="ignore"):
        inside = ((fc >= 0) & (fc < N)).all(1)                                  # step 1
        rows = np.where(inside[:, None], fc, 0)
        v = p[rows] if N else np.zeros((n, 3, 3), T32)                          # [n, vertex, xyz]
        ok0 = inside & np.isfinite(v).all((1, 2))
        x, y, z = v[..., 0], v[..., 1], v[..., 2]
        for j in range(T):
            if E is None:                                                       # step 2
                px, py, pz = x, y, z
            else:
                px, py, pz = [((E[j, a, 0] * x + E[j, a, 1] * y) + E[j, a, 2] * z) + E[j, a, 3] for a in range(3)]
            ok = ok0 & (np.isfinite(pz) & (pz >= zn) & (pz <= zf)).all(1)
            uf = ((fx[j] * (px / pz)) + cx[j]) - off
            vf = ((fy[j] * (py / pz)) + cy[j]) - off
            sx, sy = np.floor(uf * sub + half), np.floor(vf * sub + half)        # step 3
            ok &= ((np.abs(sx) < guard) & (np.abs(sy) < guard)).all(1)
            X, Y = np.where(ok[:, None], sx, 0).astype(I64), np.where(ok[:, None], sy, 0).astype(I64)
            iz = one / np.where(ok[:, None], pz, one).astype(T32)
            A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])  # step 4
            ok &= A != 0
            if cull:
                ok &= A < 0
            sign = np.where(A < 0, -1, 1).astype(I64)
            A = A * sign
            u0, u1 = np.maximum(0, (X.min(1) + 255) >> 8), np.minimum(W - 1, X.max(1) >> 8)  # step 5
            v0, v1 = np.maximum(0, (Y.min(1) + 255) >> 8), np.minimum(H - 1, Y.max(1) >> 8)
            bw, bh = u1 - u0 + 1, v1 - v0 + 1
            ok &= (bw > 0) & (bh > 0)
            big = ok & ((bw > extent) | (bh > extent))
            skipped[j] = big.sum()
            ok &= ~big
            setups.append((X, Y, sign, A, iz))
            d = np.nonzero(ok)[0]
            if not len(d):
                continue
            for dv in range(int(bh[d].max())):
                for du in range(int(bw[d].max())):
                    s = d[(dv < bh[d]) & (du < bw[d])]
                    if not len(s):
                        continue
                    pu, pv = u0[s] + du, v0[s] + dv
                    w0, w1, w2 = weights(X[s], Y[s], sign[s], 256 * pu, 256 * pv)
                    cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
                    a = A[s].astype(np.float64)
                    b0, b1, b2 = [(w.astype(np.float64) / a).astype(T32) for w in (w0, w1, w2)]   # step 7
                    zi = (b0 * iz[s, 0] + b1 * iz[s, 1]) + b2 * iz[s, 2]
                    zz = (one / zi).astype(T32)
                    cov &= np.isfinite(zz) & (zz >= zn) & (zz <= zf)
                    key = (np.ascontiguousarray(zz[cov]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | s[cov].astype(np.uint64)
                    np.minimum.at(keys[j], pv[cov] * W + pu[cov], key)                           # step 8
        skipped[T] = skipped[:T].sum()
        keys = keys.reshape(T, H, W)
        hit = keys != empty
        depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(T32), T32(0)).astype(T32)
        face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        color = None
        if col is not None:
            color = np.zeros((T, H, W, 3), np.uint8)
            for j in range(T):
                pv, pu = np.nonzero(hit[j])
                if not len(pv):
                    continue
                s = face[j][pv, pu].astype(I64)
                X, Y, sign, A, _ = setups[j]
                w = weights(X[s], Y[s], sign[s], 256 * pu.astype(I64), 256 * pv.astype(I64))
                a = A[s].astype(np.float64)
                b0, b1, b2 = [(k.astype(np.float64) / a).astype(T32)[:, None] for k in w]
                c0, c1, c2 = [col[fc[s, k]].astype(T32) for k in range(3)]
                color[j][pv, pu] = np.minimum(np.floor(((b0 * c0 + b1 * c1) + b2 * c2) + half), T32(255)).astype(np.uint8)
    filled = np.concatenate([hit.reshape(T, -1).sum(1), [hit.sum()]]).astype(np.int32)
    return HostRaster(depth, face, color, filled, skipped.astype(np.int32))


def write_ply(path: str, xyz: np.ndarray, rgb: Optional[np.ndarray] = None, normals: Optional[np.ndarray] = None,
              faces: Optional[np.ndarray] = None, label: Optional[np.ndarray] = None) -> None:
    """Binary little-endian PLY: `x y z` float, optional `nx ny nz` float, optional `red green blue` uchar, optional `label` int
    (the plane of every point, `fit_planes`; label=None: the file without it); with `faces` int [F,3] an `element face` of
    `uchar int` vertex_indices lists behind the vertices (faces=None: the file without it)."""
    xyz = np.ascontiguousarray(xyz, dtype="<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        normals = np.ascontiguousarray(normals, dtype="<f4").reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError(f"{len(normals)} normals for {len(xyz)} points")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb is not None:
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
        if len(rgb) != len(xyz):
            raise ValueError(f"{len(rgb)} colours for {len(xyz)} points")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if label is not None:
        label = np.ascontiguousarray(label, dtype="<i4").reshape(-1)
        if len(label) != len(xyz):
            raise ValueError(f"{len(label)} labels for {len(xyz)} points")
        fields += [("label", "<i4")]
    rec = np.empty(len(xyz), dtype=np.dtype(fields))
    for i, n in enumerate("xyz"):
        rec[n] = xyz[:, i]
        if normals is not None:
            rec["n" + n] = normals[:, i]
    if rgb is not None:
        for i, n in enumerate(("red", "green", "blue")):
            rec[n] = rgb[:, i]
    if label is not None:
        rec["label"] = label
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}"]
    names = {"<f4": "float", "u1": "uchar", "<i4": "int"}
    head += [f"property {names[t]} {n}" for n, t in fields]
    tail = b""
    if faces is not None:
        faces = np.asarray(faces).reshape(-1, 3)
        if len(faces) and (faces.min() < 0 or faces.max() >= len(xyz)):
            raise ValueError(f"a face names a vertex outside 0..{len(xyz) - 1}")
        frec = np.empty(len(faces), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        frec["n"], frec["v"] = 3, faces
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        tail = frec.tobytes()
    head += ["end_header"]
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii") + rec.tobytes() + tail)


def read_ply(path: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """Reader for the files `write_ply` produces -> (xyz f32 [N,3], rgb uint8 [N,3] or None)."""
    xyz, rgb, _ = read_ply_normals(path)
    return xyz, rgb


def _ply_vertex_fields(lines):
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    return [(l.split()[2], kinds[l.split()[1]]) for l in lines if l.startswith("property") and l.split()[1] != "list"]


def read_ply_label(path: str) -> Optional[np.ndarray]:
    """The `label` column of a file `write_ply(label=)` produced -> int32 [N], or None when the file has none."""
    b = open(path, "rb").read()
    end = b.index(b"end_header\n") + len(b"end_header\n")
    lines = b[:end].decode("ascii").split("\n")
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    rec = np.frombuffer(b, dtype=np.dtype(_ply_vertex_fields(lines)), count=n, offset=end)
    return rec["label"].astype(np.int32) if "label" in rec.dtype.names else None


def read_ply_normals(path: str) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
    """`read_ply` with the normals -> (xyz f32 [N,3], rgb uint8 [N,3] or None, normals f32 [N,3] or None)."""
    b = open(path, "rb").read()
    end = b.index(b"end_header\n") + len(b"end_header\n")
    lines = b[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    rec = np.frombuffer(b, dtype=np.dtype(_ply_vertex_fields(lines)), count=n, offset=end)
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1).astype(np.float32)
    rgb = np.stack([rec["red"], rec["green"], rec["blue"]], axis=-1) if "red" in rec.dtype.names else None
    nrm = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=-1).astype(np.float32) if "nx" in rec.dtype.names else None
    return xyz, rgb, nrm


def read_ply_faces(path: str) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
    """`read_ply_normals` with the faces -> (xyz, rgb or None, normals or None, faces int32 [F,3] or None when the file has no
    face element)."""
    xyz, rgb, nrm = read_ply_normals(path)
    b = open(path, "rb").read()
    end = b.index(b"end_header\n") + len(b"end_header\n")
    lines = b[:end].decode("ascii").split("\n")
    face = [l for l in lines if l.startswith("element face")]
    if not face:
        return xyz, rgb, nrm, None
    assert "property list uchar int vertex_indices" in lines
    size = {"float": 4, "uchar": 1, "int": 4}
    vertex_bytes = sum(size[l.split()[1]] for l in lines if l.startswith("property") and l.split()[1] != "list") * len(xyz)
    frec = np.frombuffer(b, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=int(face[0].split()[2]), offset=end + vertex_bytes)
    assert (frec["n"] == 3).all()
    return xyz, rgb, nrm, frec["v"].astype(np.int32)


def save_depth_map(depth: np.ndarray, path: str, crop: Optional[ImageCropRegion] = None,
                   target_dims: Optional[Tuple[int, int]] = None) -> np.ndarray:
    px = depth_to_u8(depth, crop, target_dims)
    write_gray_png(path, px)
    return px


# ------------------------------------------------------------------------------------------------------------
# AnyDepthModel (src/model/mod.rs:40-142)
# ------------------------------------------------------------------------------------------------------------
class AnyDepthModel:
    def __init__(self, kind: DepthModelKind, model):
        self.kind, self.model = kind, model

    @staticmethod
    def load(kind: DepthModelKind, device, checkpoint: str, precision=None, max_batch=None) -> "AnyDepthModel":
        """`AnyDepthModel::load`: Depth Pro loads directly; Depth-Anything-v3 tries metric_large then small, small
        first when the file name contains "small" (mod.rs:62-100). Errors carry the reference's message prefix."""
        from . import _lib
        from .config import DepthAnything3Config, DepthProConfig
        from .depth_anything3 import DepthAnything3
        from .depth_pro import DepthPro
        if kind == DepthModelKind.DEPTH_PRO:
            cfg = DepthProConfig()
            if precision is not None:
                cfg.precision = precision
            try:
                return AnyDepthModel(kind, DepthPro.load_with_config(device, cfg, checkpoint))
            except _lib.MdError as e:
                raise RuntimeError(f"Failed to load DepthPro checkpoint: {e}") from e
        configs = [DepthAnything3Config.metric_large(), DepthAnything3Config.small()]
        if "small" in os.path.basename(checkpoint).lower():
            configs.reverse()
        last = None
        for cfg in configs:
            if precision is not None:
                cfg.precision = precision
            if max_batch is not None:  # images per call (`infer_views`: scenes x views)
                cfg.max_batch = int(max_batch)
            try:
                return AnyDepthModel(kind, DepthAnything3.load_file(device, cfg, checkpoint))
            except _lib.MdError as e:
                last = e
        raise RuntimeError(f"Failed to load Depth Anything 3 checkpoint `{checkpoint}`: {last}")

    def process_frame(self, rgb, normalize_relative_depth: bool = True, fmt: str = "rgba"):
        """`process_frame` (crates/bevy_burn_depth/src/lib.rs:16-74) on the device: prepare at the model's resolution, infer,
        min-max normalise (normalize_relative_depth) and build the display at the model's resolution -- RGBA f32 for the
        viewer's texture, or "u8" grey. rgb: uint8 [H,W,3] / [B,H,W,3] (numpy or torch). Returns a `FrameResult`."""
        return self.model.process_frame(rgb, target=0, restore=False, normalize=normalize_relative_depth, fmt=fmt)

    def infer_points(self, x, **kw):
        """`md_infer_points`: the model, then its depth (and cameras) as a point cloud, in one device call -> `PointCloud`.
        Keywords as `DepthPro.infer_points` / `DepthAnything3.infer_points`, conf_percentile= / view_rtol= / min_views= (the view
        filter, `md_infer_points_filtered`), normals= / normal_min_cos= (`md_infer_points_normals`), voxel= (`md_infer_points_voxel`)
        render= (`md_infer_points_render`), mesh= (`md_infer_points_mesh`), raster= (`md_infer_points_raster`), outlier=
        (`md_infer_points_outlier`), decimate= (`md_infer_points_decimate`), components= (`md_infer_points_components`) and
        smooth= (`md_infer_points_smooth`), planes= (`md_infer_points_planes`), clusters= (`md_infer_points_clusters`) and match=
        (`md_infer_points_match`) included."""
        return self.model.infer_points(x, **kw)

    def infer_views(self, x):
        """`md_da3_infer_views`: x [B, V, 3, H, W], B scenes of V views -> `DepthAnything3Inference` with every field [B*V, ...].
        Depth-Anything-v3 `small` only: Depth Pro has no cross-view attention."""
        if self.kind == DepthModelKind.DEPTH_PRO:
            raise ValueError("multi-view inference applies to Depth-Anything-v3, not to Depth Pro")
        return self.model.infer_views(x)

    def preferred_input_resolution(self) -> Optional[int]:
        return None if self.kind == DepthModelKind.DEPTH_PRO else self.model.img_size()

    def prepare_input_image(self, rgb: np.ndarray) -> PreparedModelImage:
        if self.kind == DepthModelKind.DEPTH_PRO:
            return PreparedModelImage(rgb.shape[1], rgb.shape[0], rgb.copy(), None)
        return prepare_depth_anything3_image(rgb, self.model.img_size())

    def infer_from_rgb(self, prepared: PreparedModelImage, f_px: Optional[float] = None):
        """f_px: the caller's focal length in pixels of the prepared image (Depth Pro only: the FOV network does not run)."""
        if f_px is None:
            return self.model.infer_from_rgb(prepared.rgb.tobytes(), prepared.width, prepared.height)
        if self.kind != DepthModelKind.DEPTH_PRO:
            raise ValueError(f"a known focal length applies to Depth Pro only, not to `{self.kind.value}`")
        return self.model.infer_from_rgb(prepared.rgb.tobytes(), prepared.width, prepared.height, f_px)
