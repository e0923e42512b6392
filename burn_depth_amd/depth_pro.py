"""Host-side mirror of the reference's Depth Pro interface over the C ABI.

Same names, argument meaning and error behaviour as the reference (file:line under the
reference repository):

* ``DepthPro.new(device, config)``            -- depth_pro/mod.rs:145-191
* ``DepthPro.load(device, path)``             -- depth_pro/mod.rs:193-198
* ``DepthPro.load_with_config``               -- depth_pro/mod.rs:200-208
* ``DepthPro.infer(x) -> DepthProInference``  -- depth_pro/mod.rs:312-364
* ``DepthPro.infer(x, f_px)``                 -- the same with the caller's focal length (ml-depth-pro's ``infer(x, f_px)``):
                                                 no FOV network, md_depth_pro_infer_with_focal
* ``img_size`` / ``interpolation_method``     -- depth_pro/mod.rs:296,308
* ``decoder_from_features`` / ``head_debug``  -- depth_pro/mod.rs:262-267, 289-307
* debug taps                                  -- encoder.rs:106-123, mod.rs:135-142,285-287

PyTorch is used only as plumbing: device buffers (``torch.empty(..., device="cuda")``), the
current HIP stream, and ``torch.distributed``.  All arithmetic happens in libmi_depth.so.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, points
from .config import DepthProConfig, InterpolationMethod, Precision
from .points import FittedPlanes, PointCloud, PointClusters, PointMatch, PointRegistration, RasterisedMesh, RenderedPoints, SmoothedMesh  # noqa: F401 -- the point path's results, re-exported


class Device:
    """`<B as Backend>::Device::default()` (README.md:21): one engine device = one GPU."""

    def __init__(self, ordinal: int = 0):
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.md_device_open(int(ordinal), C.byref(h)))
        self.handle = h
        self.ordinal = int(ordinal)
        torch.cuda.set_device(self.ordinal)

    @staticmethod
    def default() -> "Device":
        return Device(int(os.environ.get("LOCAL_RANK", "0")))

    def synchronize(self) -> None:
        _lib.check(_lib.load().md_device_synchronize(self.handle))

    def close(self) -> None:
        if self.handle:
            _lib.load().md_device_close(self.handle)
            self.handle = None


@dataclass
class DepthProInference:
    """depth_pro/mod.rs:128-133."""
    depth: torch.Tensor           # [B, H, W]
    focallength_px: torch.Tensor  # [B]
    fovx_deg: torch.Tensor        # [B]
    fovy_rad: torch.Tensor        # [B]


@dataclass
class FrameResult:
    """What `md_process_frame` returns (include/mi_depth.h): the display map (u8 [B,oh,ow] or RGBA f32 [B,oh,ow,4]), the
    model-resolution depth [B,th,tw], the normalisation range [B,2], the prepared frame [B,th,tw,3] and, for Depth Pro,
    focal length and vertical field of view [B]. Device tensors."""
    display: Optional[torch.Tensor]
    depth: torch.Tensor
    depth_range: torch.Tensor
    prepared: Optional[torch.Tensor] = None
    focallength_px: Optional[torch.Tensor] = None
    fovy_rad: Optional[torch.Tensor] = None


@dataclass
class HeadDebug:
    """depth_pro/mod.rs:135-142."""
    conv0: torch.Tensor      # [B, F/2, s, s]
    deconv: torch.Tensor     # [B, F/2, 2s, 2s]
    conv1: torch.Tensor      # [B, 32, 2s, 2s]
    relu: torch.Tensor       # [B, 32, 2s, 2s]
    pre_out: torch.Tensor    # [B, 1, 2s, 2s]
    canonical: torch.Tensor  # [B, 1, 2s, 2s]


def _c_cfg(cfg: DepthProConfig) -> Tuple[_lib.MdDepthProCfg, list]:
    keep = [cfg.patch_encoder_preset.encode(), cfg.image_encoder_preset.encode(),
            cfg.fov_encoder_preset.encode() if cfg.fov_encoder_preset else None]
    c = _lib.MdDepthProCfg(keep[0], keep[1], keep[2], int(cfg.decoder_features), int(bool(cfg.use_fov_head)),
                           int(cfg.interpolation), int(cfg.precision), int(cfg.max_batch), float(cfg.ln_eps))
    return c, keep


def _stream_ptr(device_ordinal: int) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device_ordinal).cuda_stream)


def _focal_arg(f_px, B: int, on_device: bool, device_ordinal: int):
    """The caller's focal lengths as the fp32 [B] buffer md_depth_pro_infer_with_focal reads, in the memory kind of the image:
    a float is broadcast to B, a sequence or a [B] tensor gives one value per image. A CUDA fp32 contiguous [B] tensor on this GPU
    is passed as it is (a replayed graph reads whatever it then holds). Returns (pointer, keep-alive)."""
    if isinstance(f_px, torch.Tensor):
        t = f_px.detach().reshape(-1)
        if t.numel() == 1 and B != 1:
            t = t.expand(B)
    elif isinstance(f_px, (int, float, np.floating, np.integer)):
        t = torch.full((B,), float(f_px), dtype=torch.float32)
    else:
        t = torch.tensor([float(v) for v in f_px], dtype=torch.float32)
    if t.numel() != B:
        raise _lib.MdError(_lib.MD_ERR_SHAPE, f"f_px holds {t.numel()} focal lengths for a batch of {B}")
    if on_device:
        t = t.to(device=torch.device("cuda", device_ordinal), dtype=torch.float32).contiguous()
    else:
        t = t.to(device="cpu", dtype=torch.float32).contiguous()
    return C.c_void_p(t.data_ptr()), t


class DepthPro:
    def __init__(self, device: Device, handle: C.c_void_p, config: DepthProConfig):
        self.device = device
        self._h = handle
        self.config = config
        self._lib = _lib.load()
        self._parent: Optional["DepthPro"] = None  # the root model of a fork (keeps it alive)
        self._forks = weakref.WeakSet()            # live forks of a root

    # ---- construction ---------------------------------------------------------------------
    @staticmethod
    def new(device: Device, config: Optional[DepthProConfig] = None, seed: int = 0, init_scheme: int = 0) -> "DepthPro":
        config = config or DepthProConfig()
        c, keep = _c_cfg(config)
        h = C.c_void_p()
        _lib.check(_lib.load().md_depth_pro_create(device.handle, C.byref(c), C.c_uint64(seed), int(init_scheme), C.byref(h)))
        return DepthPro(device, h, config)

    @staticmethod
    def load(device: Device, checkpoint_path: str) -> "DepthPro":
        return DepthPro.load_with_config(device, DepthProConfig(), checkpoint_path)

    @staticmethod
    def load_with_config(device: Device, config: DepthProConfig, checkpoint_path: str) -> "DepthPro":
        c, keep = _c_cfg(config)
        h = C.c_void_p()
        _lib.check(_lib.load().md_depth_pro_load_with_config(device.handle, C.byref(c), os.fspath(checkpoint_path).encode(),
                                                             C.byref(h)))
        return DepthPro(device, h, config)

    def fork(self) -> "DepthPro":
        """`model.clone()` / sharing `&DepthPro` across threads (depth_pro/mod.rs:119-126,312): a second inference
        context (own workspace, own default stream) on the SAME device weights (md_model_fork). Destroy forks before
        the model they were forked from."""
        h = C.c_void_p()
        _lib.check(self._lib.md_model_fork(self._h, C.byref(h)))
        f = type(self)(self.device, h, self.config)
        # the fork aliases this model's weight arenas: keep the root alive until every fork is gone, and let the root
        # find its live forks when it is destroyed first
        f._parent = self._parent if self._parent is not None else self
        f._parent._forks.add(f)
        return f

    def destroy(self) -> None:
        """md_model_destroy. A root with live forks refuses (MD_ERR_INVALID_ARG): they alias its weights and go first."""
        if not self._h:
            return
        _lib.check(self._lib.md_model_destroy(self._h))
        self._h = None
        if self._parent is not None:
            self._parent._forks.discard(self)
            self._parent = None

    def __del__(self):
        try:
            for f in list(self._forks):  # only reachable at interpreter shutdown: a live fork holds a reference to its root
                f.destroy()
            self.destroy()
        except Exception as e:  # noqa: BLE001 -- at interpreter shutdown module globals (even `_lib.MdError`) may already be None
            if _lib is not None and getattr(_lib, "MdError", None) is not None and isinstance(e, _lib.MdError):
                import warnings  # never silent: a failed destroy leaks the weight / workspace arenas
                warnings.warn(f"DepthPro.__del__: {e}", ResourceWarning)

    # ---- introspection --------------------------------------------------------------------
    def query(self, key: str) -> int:
        v = C.c_int64()
        _lib.check(self._lib.md_model_query(self._h, key.encode(), C.byref(v)))
        return int(v.value)

    def set_option(self, key: str, value: int) -> None:
        """md_model_set_option: "batch_invariant" = 1 makes a Depth-Anything-v3 model's 16-bit results independent of the batch an image
        sits in (no launch-size-dependent kernel form), as the reference's `infer` is a pure batch map."""
        _lib.check(self._lib.md_model_set_option(self._h, key.encode(), C.c_int64(int(value))))

    def img_size(self) -> int:
        return self.query("img_size")

    def interpolation_method(self) -> int:
        return self.query("interpolation")

    def param_names(self) -> List[Tuple[str, int]]:
        out = []
        for i in range(self._lib.md_model_param_count(self._h)):
            name, n = C.c_char_p(), C.c_size_t()
            _lib.check(self._lib.md_model_param_info(self._h, i, C.byref(name), C.byref(n)))
            out.append((name.value.decode(), int(n.value)))
        return out

    # ---- records (Module::into_record / load_record, src/lib.rs:163-177) -------------------
    def get_tensor(self, name: str, count: int) -> np.ndarray:
        buf = np.empty(count, dtype=np.float32)
        _lib.check(self._lib.md_model_get_tensor(self._h, name.encode(), buf.ctypes.data_as(C.c_void_p), count))
        return buf

    def set_tensor(self, name: str, values: np.ndarray) -> None:
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        _lib.check(self._lib.md_model_set_tensor(self._h, name.encode(), v.ctypes.data_as(C.c_void_p), v.size))

    def commit_weights(self) -> None:
        _lib.check(self._lib.md_model_commit_weights(self._h))

    def round_weights_to_f16(self) -> "DepthPro":
        """Round every parameter to the nearest IEEE half, in place, and commit: what `DepthPro::load` of the reference's
        f16 record (`HalfPrecisionSettings`, depth_pro/mod.rs:193-208) of these weights holds. In `Precision.F16X2` the
        weights are then exact MFMA operands (`query("weight_terms") == 2`)."""
        _lib.check(self._lib.md_model_round_weights_f16(self._h))
        return self

    def into_record(self) -> Dict[str, np.ndarray]:
        return {n: self.get_tensor(n, c) for n, c in self.param_names()}

    def load_record(self, record: Dict[str, np.ndarray]) -> "DepthPro":
        for n, _ in self.param_names():
            self.set_tensor(n, record[n])
        self.commit_weights()
        return self

    def weight_arena(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(self._lib.md_model_weight_arena(self._h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    # ---- inference ------------------------------------------------------------------------
    def infer(self, x: torch.Tensor, f_px=None) -> DepthProInference:
        """x: [B,3,H,W] fp32, ImageNet-normalised (any H, W), on the GPU or the host.
        f_px: the caller's focal length in pixels of the W-wide input -- a float (every image), a sequence or a [B] tensor --
        or None to predict it with the FOV network. With f_px the FOV network does not run and focallength_px is f_px."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,3,H,W], got {tuple(x.shape)}")
        x = x.contiguous().to(torch.float32)
        B, _, H, W = x.shape
        dev = torch.device("cuda", self.device.ordinal)
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        focal = torch.empty((B,), dtype=torch.float32, device=dev)
        fovx = torch.empty((B,), dtype=torch.float32, device=dev)
        fovy = torch.empty((B,), dtype=torch.float32, device=dev)
        in_kind = _lib.MD_MEM_DEVICE if x.is_cuda else _lib.MD_MEM_HOST
        self._infer_call(x, B, H, W, in_kind, f_px, depth, focal, fovx, fovy)
        return DepthProInference(depth, focal, fovx, fovy)

    def infer_into(self, x: torch.Tensor, depth: torch.Tensor, focal: torch.Tensor, fovx: torch.Tensor,
                   fovy: torch.Tensor, f_px=None) -> None:
        """Allocation-free variant used by the benchmark loop (all tensors on this GPU; f_px as in `infer`, a CUDA [B] fp32
        tensor keeps it allocation-free)."""
        B, _, H, W = x.shape
        self._infer_call(x, B, H, W, _lib.MD_MEM_DEVICE, f_px, depth, focal, fovx, fovy)

    def _infer_call(self, x, B, H, W, in_kind, f_px, depth, focal, fovx, fovy) -> None:
        outs = (C.c_void_p(depth.data_ptr()), C.c_void_p(focal.data_ptr()), C.c_void_p(fovx.data_ptr()), C.c_void_p(fovy.data_ptr()))
        if f_px is None:
            _lib.check(self._lib.md_depth_pro_infer(self._h, C.c_void_p(x.data_ptr()), B, H, W, in_kind, *outs,
                                                    _lib.MD_MEM_DEVICE, _stream_ptr(self.device.ordinal)))
            return
        fp, keep = _focal_arg(f_px, B, in_kind == _lib.MD_MEM_DEVICE, self.device.ordinal)
        _lib.check(self._lib.md_depth_pro_infer_with_focal(self._h, C.c_void_p(x.data_ptr()), B, H, W, in_kind, fp, *outs,
                                                           _lib.MD_MEM_DEVICE, _stream_ptr(self.device.ordinal)))
        del keep

    def infer_windows(self, x: torch.Tensor, parts: int, timings: bool = False):
        """`infer` with the ViT stage run as `parts` consecutive windows of its 37 B sequences on this GPU -- the launches the
        ranks of the tile-parallel mode (`NativeComm.infer_tiles`) issue, without the exchange. Bit-identical to `infer`.
        With `timings`, also returns (window_ms list, tail_ms): GPU milliseconds of each window and of everything behind the
        ViT stage."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,3,H,W], got {tuple(x.shape)}")
        x = x.contiguous().to(torch.float32)
        B, _, H, W = x.shape
        dev = torch.device("cuda", self.device.ordinal)
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        focal, fovx, fovy = (torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(3))
        wms = (C.c_float * max(int(parts), 1))()
        tms = C.c_float()
        in_kind = _lib.MD_MEM_DEVICE if x.is_cuda else _lib.MD_MEM_HOST
        _lib.check(self._lib.md_depth_pro_infer_windows(self._h, C.c_void_p(x.data_ptr()), B, H, W, in_kind,
                                                        C.c_void_p(depth.data_ptr()), C.c_void_p(focal.data_ptr()),
                                                        C.c_void_p(fovx.data_ptr()), C.c_void_p(fovy.data_ptr()), _lib.MD_MEM_DEVICE,
                                                        int(parts), wms if timings else None, C.byref(tms) if timings else None,
                                                        _stream_ptr(self.device.ordinal)))
        out = DepthProInference(depth, focal, fovx, fovy)
        return (out, [float(v) for v in wms], float(tms.value)) if timings else out

    # ---- the decoder / the head alone on caller tensors (depth_pro/mod.rs:262-307) --------------
    def decoder_level_shapes(self) -> List[Tuple[int, int]]:
        """(channels, size) of the encoder feature each decoder level takes, finest first (encoder.rs:416-434)."""
        return [(self.query(f"decoder_level{l}_channels"), self.query(f"decoder_level{l}_size"))
                for l in range(self.query("decoder_levels"))]

    def _view(self, t: torch.Tensor) -> Tuple[torch.Tensor, "_lib.MdNchwView"]:
        if t.dim() != 4:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,C,H,W], got {tuple(t.shape)}")
        t = t.contiguous().to(torch.float32)
        return t, _lib.MdNchwView(C.c_void_p(t.data_ptr()), int(t.shape[1]), int(t.shape[2]), int(t.shape[3]))

    def decoder_from_features(self, features: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, List[torch.Tensor]]:
        """`DepthPro::decoder_from_features(&self, features)` (depth_pro/mod.rs:262-267): the decoder alone on the caller's
        encoder features (finest first; all on this GPU or all on the host) -> (features, lowres_features, fusion_outputs),
        fusion_outputs[0] the finest. A wrong level count raises MdError(MD_ERR_LEVELS) where the reference panics
        (decoder.rs:200-205), a wrong shape MdError(MD_ERR_SHAPE)."""
        if len(features) == 0:
            raise _lib.MdError(_lib.MD_ERR_LEVELS, "Got encoder output levels = 0")
        B = int(features[0].shape[0])
        if any(int(f.shape[0]) != B or f.is_cuda != features[0].is_cuda for f in features):
            raise _lib.MdError(_lib.MD_ERR_SHAPE, "features differ in batch size or memory kind")
        keep, views = zip(*[self._view(f) for f in features])
        arr = (_lib.MdNchwView * len(views))(*views)
        dev = torch.device("cuda", self.device.ordinal)
        F = self.query("decoder_features")
        shapes = self.decoder_level_shapes()
        s0, s_last = shapes[0][1], shapes[-1][1]
        out_feat = torch.empty((B, F, s0, s0), dtype=torch.float32, device=dev)
        out_low = torch.empty((B, F, s_last, s_last), dtype=torch.float32, device=dev)
        fus = [torch.empty((B, F, s0 if l == 0 else 2 * shapes[l][1], s0 if l == 0 else 2 * shapes[l][1]), dtype=torch.float32, device=dev)
               for l in range(len(shapes))]
        fptr = (C.c_void_p * len(fus))(*[C.c_void_p(t.data_ptr()) for t in fus])
        in_kind = _lib.MD_MEM_DEVICE if features[0].is_cuda else _lib.MD_MEM_HOST
        _lib.check(self._lib.md_depth_pro_decoder_from_features(self._h, arr, len(views), B, in_kind, C.c_void_p(out_feat.data_ptr()),
                                                                C.c_void_p(out_low.data_ptr()), fptr, _lib.MD_MEM_DEVICE,
                                                                _stream_ptr(self.device.ordinal)))
        del keep
        return out_feat, out_low, fus

    def head_debug(self, feature: torch.Tensor) -> HeadDebug:
        """`DepthPro::head_debug(&self, feature)` (depth_pro/mod.rs:289-307): the depth head layer by layer on the caller's
        decoder feature [B, F, s, s]."""
        t, view = self._view(feature)
        B, _, s, _ = t.shape
        dev = torch.device("cuda", self.device.ordinal)
        F2 = self.query("decoder_features") // 2
        mk = lambda c, hw: torch.empty((B, c, hw, hw), dtype=torch.float32, device=dev)  # noqa: E731
        hd = HeadDebug(mk(F2, s), mk(F2, 2 * s), mk(32, 2 * s), mk(32, 2 * s), mk(1, 2 * s), mk(1, 2 * s))
        out = _lib.MdHeadDebug(*[C.c_void_p(x.data_ptr()) for x in (hd.conv0, hd.deconv, hd.conv1, hd.relu, hd.pre_out, hd.canonical)])
        in_kind = _lib.MD_MEM_DEVICE if t.is_cuda else _lib.MD_MEM_HOST
        _lib.check(self._lib.md_depth_pro_head_debug(self._h, C.byref(view), int(B), in_kind, C.byref(out), _lib.MD_MEM_DEVICE,
                                                     _stream_ptr(self.device.ordinal)))
        return hd

    @staticmethod
    def infer_tiles_loopback(contexts: List["DepthPro"], x: torch.Tensor, root: int = 0) -> DepthProInference:
        """The tile-parallel single-image call (`NativeComm.infer_tiles`) with a loopback transport: `contexts` (a model and its forks)
        stand for the ranks, each runs its window of the ViT stage in its own workspace, the root copies the other windows' tokens and
        hook rows where RCCL would deliver them (md_depth_pro_infer_tiles_loopback). Bit-identical to `infer`; a one-GPU test entry."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,3,H,W], got {tuple(x.shape)}")
        x = x.contiguous().to(torch.float32)
        B, _, H, W = x.shape
        me = contexts[root]
        dev = torch.device("cuda", me.device.ordinal)
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        focal, fovx, fovy = (torch.empty((B,), dtype=torch.float32, device=dev) for _ in range(3))
        arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
        in_kind = _lib.MD_MEM_DEVICE if x.is_cuda else _lib.MD_MEM_HOST
        _lib.check(me._lib.md_depth_pro_infer_tiles_loopback(arr, len(contexts), int(root), C.c_void_p(x.data_ptr()), B, H, W, in_kind,
                                                             C.c_void_p(depth.data_ptr()), C.c_void_p(focal.data_ptr()), C.c_void_p(fovx.data_ptr()),
                                                             C.c_void_p(fovy.data_ptr()), _lib.MD_MEM_DEVICE, _stream_ptr(me.device.ordinal)))
        return DepthProInference(depth, focal, fovx, fovy)

    def infer_from_rgb(self, rgb: bytes, width: int, height: int, f_px=None) -> DepthProInference:
        """`infer_from_rgb` (src/inference.rs:128-137); raises MdError(MD_ERR_SHAPE) on a bad length. f_px: the caller's focal
        length in pixels of the image (a float), or None to predict it."""
        dev = torch.device("cuda", self.device.ordinal)
        depth = torch.empty((1, height, width), dtype=torch.float32, device=dev) if width > 0 and height > 0 else None
        focal = torch.empty((1,), dtype=torch.float32, device=dev)
        fovy = torch.empty((1,), dtype=torch.float32, device=dev)
        buf = (C.c_uint8 * len(rgb)).from_buffer_copy(rgb) if len(rgb) else (C.c_uint8 * 1)()
        outs = (C.c_void_p(depth.data_ptr() if depth is not None else 0), C.c_void_p(focal.data_ptr()), C.c_void_p(fovy.data_ptr()),
                _lib.MD_MEM_DEVICE, _stream_ptr(self.device.ordinal))
        if f_px is None:
            _lib.check(self._lib.md_infer_from_rgb(self._h, C.cast(buf, C.c_void_p), len(rgb), int(width), int(height),
                                                   _lib.MD_MEM_HOST, *outs))
        else:
            if isinstance(f_px, torch.Tensor) or not isinstance(f_px, (int, float, np.floating, np.integer)):
                vals = [float(v) for v in (f_px.reshape(-1).tolist() if isinstance(f_px, torch.Tensor) else f_px)]
                if len(vals) != 1:
                    raise _lib.MdError(_lib.MD_ERR_SHAPE, f"f_px holds {len(vals)} focal lengths for one image")
                f_px = vals[0]
            _lib.check(self._lib.md_infer_from_rgb_with_focal(self._h, C.cast(buf, C.c_void_p), len(rgb), int(width), int(height),
                                                              _lib.MD_MEM_HOST, C.c_float(float(f_px)), *outs))
        return DepthProInference(depth, focal, torch.empty(0), fovy)

    # ---- frame path --------------------------------------------------------------------------
    MODEL_KIND = "depth-pro"
    _FRAME_FORMATS = {"u8": _lib.MD_FRAME_U8_GRAY, "rgba": _lib.MD_FRAME_RGBA_F32}

    def _frame_opts(self, target: int, restore: bool, normalize: bool, fmt: str) -> "_lib.MdFrameOpts":
        if fmt not in self._FRAME_FORMATS:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"unknown display format `{fmt}` (u8 | rgba)")
        return _lib.MdFrameOpts(int(target), int(bool(restore)), int(bool(normalize)), self._FRAME_FORMATS[fmt])

    def frame_geometry(self, width: int, height: int, target: int = 0, restore: bool = True, normalize: bool = True,
                       fmt: str = "u8") -> Tuple[int, int, int, int]:
        """(th, tw, oh, ow) of `process_frame` on width x height frames: model input / depth size, display size."""
        o = self._frame_opts(target, restore, normalize, fmt)
        v = [C.c_int() for _ in range(4)]
        _lib.check(self._lib.md_frame_geometry(self._h, int(width), int(height), C.byref(o), *(C.byref(x) for x in v)))
        return tuple(x.value for x in v)

    def process_frame(self, rgb, target: int = 0, restore: bool = True, normalize: bool = True, fmt: str = "u8",
                      prepared: bool = True, out: Optional[FrameResult] = None) -> FrameResult:
        """`md_process_frame`: uint8 RGB frames [H,W,3] / [B,H,W,3] (numpy: host memory; torch: its device) -> prepared input,
        inference and display in one device call. target / restore / normalize / fmt: `md_frame_opts`. `out`: a FrameResult
        of an earlier call to write into again (fixed output pointers: what a captured graph replays)."""
        if isinstance(rgb, np.ndarray):
            if rgb.dtype != np.uint8:
                raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"expected uint8 frames, got {rgb.dtype}")
            rgb = np.ascontiguousarray(rgb)
            keep, ptr, in_kind = rgb, rgb.ctypes.data, _lib.MD_MEM_HOST
        elif isinstance(rgb, torch.Tensor):
            if rgb.dtype != torch.uint8:
                raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, f"expected uint8 frames, got {rgb.dtype}")
            rgb = rgb.contiguous()
            keep, ptr, in_kind = rgb, rgb.data_ptr(), (_lib.MD_MEM_DEVICE if rgb.is_cuda else _lib.MD_MEM_HOST)
        else:
            raise _lib.MdError(_lib.MD_ERR_INVALID_ARG, "rgb must be a numpy array or a torch tensor")
        if keep.ndim == 3:
            keep = keep[None] if isinstance(keep, np.ndarray) else keep.unsqueeze(0)
        if keep.ndim != 4 or keep.shape[3] != 3:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,H,W,3] frames, got {tuple(keep.shape)}")
        B, H, W = (int(x) for x in keep.shape[:3])
        th, tw, oh, ow = self.frame_geometry(W, H, target, restore, normalize, fmt)
        if out is None:
            dev = torch.device("cuda", self.device.ordinal)
            f = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
            pro = self.MODEL_KIND == "depth-pro"
            out = FrameResult(display=f(B, oh, ow, dt=torch.uint8) if fmt == "u8" else f(B, oh, ow, 4), depth=f(B, th, tw),
                              depth_range=f(B, 2), prepared=f(B, th, tw, 3, dt=torch.uint8) if prepared else None,
                              focallength_px=f(B) if pro else None, fovy_rad=f(B) if pro else None)
        ptr_of = lambda t: t.data_ptr() if t is not None else None
        o = self._frame_opts(target, restore, normalize, fmt)
        outs = _lib.MdFrameOutputs(ptr_of(out.display), ptr_of(out.depth), ptr_of(out.depth_range), ptr_of(out.prepared),
                                   ptr_of(out.focallength_px), ptr_of(out.fovy_rad))
        _lib.check(self._lib.md_process_frame(self._h, C.c_void_p(ptr), B, W, H, in_kind, C.byref(o), C.byref(outs), _lib.MD_MEM_DEVICE,
                                              _stream_ptr(self.device.ordinal)))
        return out

    # ---- point path --------------------------------------------------------------------------
    def infer_points(self, x: torch.Tensor, f_px=None, intrinsics=None, extrinsics=None, rgb: Optional[torch.Tensor] = None,
                     dense: bool = True, compact: bool = True, capacity: Optional[int] = None, out: Optional[PointCloud] = None,
                     conf_percentile: int = 0, view_rtol: float = 0.0, min_views: int = 0, normals: bool = False,
                     normal_min_cos: float = 0.0, voxel: float = 0.0, render: Optional[dict] = None, mesh=None,
                     raster: Optional[dict] = None, outlier: Optional[dict] = None, decimate: Optional[dict] = None,
                     components: Optional[dict] = None, smooth: Optional[dict] = None, planes: Optional[dict] = None, clusters: Optional[dict] = None,
                     match: Optional[dict] = None, register: Optional[dict] = None, **opts) -> PointCloud:
        """The model -> point cloud call: x [B,3,H,W] fp32 on this GPU -> the model's depth unprojected with its own cameras, or the
        caller's (Depth Pro: f_px = the known-focal call; intrinsics [B,3,3]; extrinsics [B,3,4] world-to-camera for world=True).
        rgb: u8 [B,H,W,3] device tensor to gather colours from. opts: pixel_offset, depth_min, depth_max, conf_min, edge_rtol, stride,
        world (`md_points_opts`). `out`: a PointCloud of an earlier call to write into again (what a captured graph replays).
        Every form runs through the widest entry, `md_infer_points_smooth`, with NULL for the parts not asked for, which is
        `md_infer_points` / `_filtered` / `_normals` / `_voxel` / `_render` / `_mesh` / `_raster` / `_outlier` / `_decimate` /
        `_components` on the same arguments:
        conf_percentile / view_rtol / min_views (`md_view_filter_opts`): when one of them is set the view filter drops the lowest
        conf_percentile % of the confidences of the call and the pixels fewer than min_views other views confirm within view_rtol
        before the unprojection; `depth` is then the filtered depth.
        normals / normal_min_cos (`md_points_normals`): also returns the surface normals (`normal_map`, `normals`) and, with
        normal_min_cos > 0, drops the pixels seen at a grazing angle; it composes with the view filter.
        voxel > 0 (`md_points_voxel`): thins the list to one point per occupied voxel of that side (the most confident one, ties to
        the first) and returns `index`, `weight` and `dropped` beside it; the B views share one grid. It composes with the view
        filter and the normals.
        render (`md_points_render`): a dict with H, W, the target cameras (intrinsics [T,3,3] or focal_px [T]; extrinsics [T,3,4]
        world-to-camera or None) and optionally pixel_offset, z_near, z_far, radius: the list the call ends with is z-buffered into
        those cameras in the same call; the images come back as `render` (`RenderedPoints`). Needs compact=True.
        mesh (`md_points_mesh`): True, or a dict with any of max_rtol, face_capacity, pixel_index: the triangle mesh of the depth
        grid over the rows of the list, cut where neighbouring depths differ by more than max_rtol of the nearer one; comes back
        as `faces`, `face_count` and `pixel_index`. Needs compact=True; not with voxel > 0.
        raster (`md_points_raster`): a dict as render's with cull and max_extent in place of radius: the faces of `mesh=` are
        rasterised into those cameras in the same call, a render without holes; the images come back as `raster`
        (`RasterisedMesh`). Needs mesh= with faces.
        outlier (`md_points_outlier`): dict(radius=, min_neighbours=): the rows with fewer than min_neighbours other rows within
        radius leave the list before the thinning and the render see it; returns `neighbours` over the rows of the unfiltered list
        and, without voxel > 0, `index` and `dropped`. The B views share one grid. Needs compact=True; not with mesh=.
        decimate (`md_points_decimate`): dict(voxel=, face_capacity=) beside mesh=: vertex clustering behind the mesh. The list is
        then voxel thinning's at that side (`index`, `weight`, `dropped`), `faces` / `face_count` are the decimated ones over its
        rows, `face_index` their source faces in the undecimated mesh, `faces_dropped` the invalid, degenerate and duplicate faces,
        and `remap` carries `pixel_index` (rows of the undecimated list) over to the list returned. render= and raster= see the
        decimated list and faces. voxel 0 or None: the call without it. Not with voxel > 0 or outlier=.
        components (`md_points_components`): dict(min_faces=, face_capacity=) beside mesh=: island removal behind the mesh. The list
        is unchanged; `faces` / `face_count` are the faces of the components with at least min_faces faces, `face_index` their
        source faces in the unfiltered mesh, `label` / `component_faces` the component of every row of the list and
        `component_stats` the counters. raster= sees the filtered faces. min_faces 0 or None: the call without it. Not with
        decimate=, voxel > 0 or outlier=.
        smooth (`md_points_smooth`): dict(step=, iterations=, lam=, mu=0.0, pin_boundary=True, normals=False) beside mesh=: Taubin
        (lam | mu) or Laplacian smoothing of the list over the faces the rasteriser reads (those of components= when given), on
        the integer lattice of side step. The list, `normals` and render= are unchanged; the smoothed rows, the vertex normals of
        the smoothed faces and the counters come back as `smooth` (`SmoothedMesh`), and raster= draws the smoothed rows.
        iterations 0 or None: the call without it. Not with decimate=, voxel > 0 or outlier= (`ops.smooth_mesh` serves those).
        planes (`md_points_planes`, the one form that runs through `md_infer_points_planes`): dict(planes=1, hypotheses=256, tol=,
        min_inliers=3, seed=0, normal_min_cos=0, axis=(x, y, z), axis_min_cos=0, mode="label"): RANSAC plane extraction from the
        list behind every other list stage; the equations, the inlier counts and the label of every row come back as `planes`
        (`FittedPlanes`). mode "drop" / "keep": the list the call returns (and render= sees) holds the rows without / of a plane
        and `index` names their rows in the list in front of the stage; not with mesh=. normal_min_cos > 0 needs normals=True.
        planes 0 or None: the call without it.
        clusters (`md_points_clusters`, the one form that runs through `md_infer_points_clusters`): dict(radius=, min_neighbours=0,
        min_points=1, max_points=0, mode="label", table=256): DBSCAN (min_neighbours 0: Euclidean cluster extraction) of the list
        the plane stage ends with, so planes=dict(mode="drop") followed by clusters= labels what is not on a plane; the labels,
        sizes, dense ids, the table of kept clusters with their boxes and the counters come back as `clusters` (`PointClusters`).
        mode "keep": the list the call returns (and render= sees) holds the rows of kept clusters and `index` names their rows in
        the list in front of the stage; not with mesh=, and behind planes= only with its mode "drop" / "keep". radius 0 or None:
        the call without it.
        match (`md_points_match`, the one form that runs through `md_infer_points_match`): dict(target=, radius=, tol=(), mode="label"):
        the nearest row of the reference cloud `target` ([T,3]; a tensor on the GPU is read where it lies, a numpy array or CPU
        tensor is copied with every call) within `radius` for every row of the list the plane stage ends with, in front of
        clusters=, so planes=dict(mode="drop"), match=dict(mode="unmatched"), clusters= drops the floor and what the reference
        scan already holds and clusters the rest in one call; nearest, dist2, the counters (also the rows within each of up to four
        tolerances) come back as `match` (`PointMatch`). mode "matched" / "unmatched": the list the call returns holds the rows
        with / without a counterpart and `index` names their rows in the list in front of the stage; not with mesh=, and behind
        planes= only with its mode "drop" / "keep"; clusters=dict(mode="keep") only behind these two modes. radius 0 or None: the
        call without it.
        register (`md_points_register`, the one form that runs through `md_infer_points_register`): dict(target=, radius=,
        iterations=10, init=None, min_pairs=3, rot_eps=0, trans_eps=0, apply=False): rigid point-to-point ICP of the list match=
        reads onto the reference cloud `target` (as match='s), directly in front of match=; the transform, the histories, the
        counters, nearest and dist2 come back as `registration` (`PointRegistration`). apply=True: the moved rows (and normals)
        replace that list in place, so match= and clusters= see the aligned cloud; not with mesh=. radius 0 or None: the call
        without it. target_normals= [T,3] where `target` lies: the point-to-plane form through `md_infer_points_register_plane`
        (min_pairs at least 6, status 3 a degenerate system, `registration.sum_r2`); without it the call is the one above."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise _lib.MdError(_lib.MD_ERR_SHAPE, f"expected [B,3,H,W], got {tuple(x.shape)}")
        dev = torch.device("cuda", self.device.ordinal)
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        B, _, H, W = (int(v) for v in x.shape)
        if rgb is not None:
            rgb = rgb.to(device=dev, dtype=torch.uint8).contiguous()
        rq = points._points_request(
            dev, B, H, W, want_rgb=rgb is not None, want_conf=bool(getattr(self.config, "dual_head", False)), want_depth=True,
            intrinsics=intrinsics, extrinsics=extrinsics, focal_px=f_px, dense=dense, compact=compact, capacity=capacity, out=out,
            conf_percentile=conf_percentile, view_rtol=view_rtol, min_views=min_views, normals=normals, normal_min_cos=normal_min_cos,
            voxel=voxel, render=render, mesh=mesh, raster=raster, outlier=outlier, decimate=decimate, components=components,
            smooth=smooth, planes=planes, clusters=clusters, match=match, register=register, opts=opts)
        if rq.rpl is not None:
            entry, parts = self._lib.md_infer_points_register_plane, rq.register_plane_args()
        elif rq.reg is not None:
            entry, parts = self._lib.md_infer_points_register, rq.register_args()
        elif rq.mat is not None:
            entry, parts = self._lib.md_infer_points_match, rq.match_args()
        elif rq.clu is not None:
            entry, parts = self._lib.md_infer_points_clusters, rq.clusters_args()
        else:
            entry, parts = (self._lib.md_infer_points_planes, rq.planes_args()) if rq.pln is not None else (self._lib.md_infer_points_smooth, rq.args())
        _lib.check(entry(self._h, C.c_void_p(x.data_ptr()), B, H, W, _lib.MD_MEM_DEVICE,
                         C.c_void_p(rgb.data_ptr()) if rgb is not None else None, *parts, _lib.MD_MEM_DEVICE, _stream_ptr(self.device.ordinal)))
        return rq.cloud

    # ---- debug taps / timing --------------------------------------------------------------
    def enable_taps(self, enable: bool = True) -> None:
        _lib.check(self._lib.md_model_enable_taps(self._h, int(enable)))

    def read_tap(self, name: str) -> np.ndarray:
        dims = (C.c_int64 * 4)()
        _lib.check(self._lib.md_model_read_tap(self._h, name.encode(), None, 0, C.byref(dims)))
        shape = [int(d) for d in dims]
        n = int(np.prod([max(d, 1) for d in shape]))
        out = np.empty(n, dtype=np.float32)
        _lib.check(self._lib.md_model_read_tap(self._h, name.encode(), out.ctypes.data_as(C.c_void_p), n, C.byref(dims)))
        return out.reshape([max(d, 1) for d in shape])

    def enable_timing(self, enable: bool = True) -> None:
        _lib.check(self._lib.md_model_enable_timing(self._h, int(enable)))

    def set_timing_filter(self, family: Optional[str] = None) -> None:
        """Time only the launches of one kernel family (None = all): md_model_set_timing_filter."""
        _lib.check(self._lib.md_model_set_timing_filter(self._h, family.encode() if family else None))

    def enable_graph(self, enable: bool = True) -> None:
        """Replay the launch schedule from a hipGraph for repeated calls with the same buffers (md_model_enable_graph)."""
        _lib.check(self._lib.md_model_enable_graph(self._h, int(enable)))

    def read_launch_order(self) -> List[str]:
        n = C.c_int()
        _lib.check(self._lib.md_model_read_launch_order(self._h, None, 0, C.byref(n)))
        names = (C.c_char_p * max(n.value, 1))()
        _lib.check(self._lib.md_model_read_launch_order(self._h, names, n.value, C.byref(n)))
        return [names[i].decode() for i in range(n.value)]

    def read_timing(self) -> Dict[str, Tuple[float, int]]:
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        calls = (C.c_int * cap)()
        n = C.c_int()
        _lib.check(self._lib.md_model_read_timing(self._h, names, ms, calls, cap, C.byref(n)))
        return {names[i].decode(): (float(ms[i]), int(calls[i])) for i in range(min(n.value, cap))}
