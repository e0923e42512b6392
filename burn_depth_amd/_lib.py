"""ctypes binding of libmi_depth.so (include/mi_depth.h).

The HIP library is the product: if it is missing the import fails loudly -- there is no
CPU/PyTorch fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi_depth.so")

MD_OK = 0
MD_ERR_INVALID_ARG, MD_ERR_SHAPE, MD_ERR_IO, MD_ERR_FORMAT, MD_ERR_HIP = -1, -2, -3, -4, -5
MD_ERR_UNSUPPORTED, MD_ERR_NO_FOV, MD_ERR_OOM, MD_ERR_LEVELS = -6, -7, -8, -9
MD_MEM_HOST, MD_MEM_DEVICE = 0, 1
MD_COMM_ID_BYTES = 128
MD_FRAME_U8_GRAY, MD_FRAME_RGBA_F32 = 0, 1
VIT_GEMM_RESID, VIT_GEMM_QKV, VIT_GEMM_FC1, VIT_GEMM_PATCH_EMBED = 0, 1, 2, 3
DECODER_GEMM_CONV3, DECODER_GEMM_CONV3_S2, DECODER_GEMM_PIXSHUF, DECODER_GEMM_HEAD, DECODER_GEMM_HEAD_UP2 = 0, 1, 2, 3, 4
INDEXED_GEMM_ROWS, INDEXED_GEMM_ROWS_RES, INDEXED_GEMM_PIXSHUF = 0, 1, 2
COMPOSE_DECONV_CONV, COMPOSE_DECONV_PAIR, COMPOSE_C1C3, COMPOSE_HEAD = 0, 1, 2, 3
TILE_256x256, TILE_128x128, TILE_256x32, TILE_128x64, TILE_64x64, TILE_AUTO = 0, 1, 2, 3, 4, 99


class MdError(RuntimeError):
    """Maps the reference's `Result::Err(String)` / `RecorderError` / panics."""

    def __init__(self, code: int, message: str):
        super().__init__(f"mi_depth error {code}: {message}")
        self.code = code
        self.message = message


class MdDa3Outputs(C.Structure):
    """md_da3_outputs (include/mi_depth.h)."""
    _fields_ = [("depth", C.c_void_p), ("depth_confidence", C.c_void_p), ("aux", C.c_void_p), ("aux_confidence", C.c_void_p),
                ("pose_encoding", C.c_void_p), ("extrinsics", C.c_void_p), ("intrinsics", C.c_void_p)]


class MdFrameOpts(C.Structure):
    """md_frame_opts (include/mi_depth.h)."""
    _fields_ = [("target", C.c_int), ("restore", C.c_int), ("normalize", C.c_int), ("format", C.c_int)]


class MdFrameOutputs(C.Structure):
    """md_frame_outputs (include/mi_depth.h)."""
    _fields_ = [("display", C.c_void_p), ("depth", C.c_void_p), ("depth_range", C.c_void_p), ("prepared", C.c_void_p),
                ("focallength_px", C.c_void_p), ("fovy_rad", C.c_void_p)]


class MdPointsOpts(C.Structure):
    """md_points_opts (include/mi_depth.h)."""
    _fields_ = [("pixel_offset", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float), ("conf_min", C.c_float),
                ("edge_rtol", C.c_float), ("stride", C.c_int), ("world", C.c_int)]


class MdPointsCameras(C.Structure):
    """md_points_cameras (include/mi_depth.h)."""
    _fields_ = [("intrinsics", C.c_void_p), ("extrinsics", C.c_void_p), ("focal_px", C.c_void_p)]


class MdPointsOutputs(C.Structure):
    """md_points_outputs (include/mi_depth.h)."""
    _fields_ = [("point_map", C.c_void_p), ("mask", C.c_void_p), ("xyz", C.c_void_p), ("rgb", C.c_void_p), ("conf", C.c_void_p),
                ("count", C.c_void_p), ("capacity", C.c_int64), ("depth", C.c_void_p)]


class MdPointsNormals(C.Structure):
    """md_points_normals (include/mi_depth.h)."""
    _fields_ = [("normal_map", C.c_void_p), ("normals", C.c_void_p), ("min_cos", C.c_float)]


class MdPointsVoxel(C.Structure):
    """md_points_voxel (include/mi_depth.h)."""
    _fields_ = [("voxel", C.c_float), ("index", C.c_void_p), ("weight", C.c_void_p), ("dropped", C.c_void_p)]


class MdPointsOutlier(C.Structure):
    """md_points_outlier (include/mi_depth.h)."""
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_int), ("neighbours", C.c_void_p), ("index", C.c_void_p), ("dropped", C.c_void_p)]


class MdPointsDecimate(C.Structure):
    """md_points_decimate (include/mi_depth.h)."""
    _fields_ = [("voxel", C.c_float), ("index", C.c_void_p), ("weight", C.c_void_p), ("dropped", C.c_void_p), ("remap", C.c_void_p),
                ("faces", C.c_void_p), ("face_index", C.c_void_p), ("face_count", C.c_void_p), ("face_capacity", C.c_int64),
                ("faces_dropped", C.c_void_p)]


class MdPointsComponents(C.Structure):
    """md_points_components (include/mi_depth.h)."""
    _fields_ = [("min_faces", C.c_int32), ("compact", C.c_int32), ("label", C.c_void_p), ("component_faces", C.c_void_p), ("index", C.c_void_p),
                ("remap", C.c_void_p), ("faces", C.c_void_p), ("face_index", C.c_void_p), ("face_count", C.c_void_p),
                ("face_capacity", C.c_int64), ("stats", C.c_void_p)]


class MdPointsSmooth(C.Structure):
    """md_points_smooth (include/mi_depth.h)."""
    _fields_ = [("step", C.c_float), ("lam", C.c_float), ("mu", C.c_float), ("iterations", C.c_int32), ("pin_boundary", C.c_int32),
                ("xyz", C.c_void_p), ("normals", C.c_void_p), ("stats", C.c_void_p)]


class MdPointsPlanes(C.Structure):
    """md_points_planes (include/mi_depth.h)."""
    _fields_ = [("planes", C.c_int32), ("hypotheses", C.c_int32), ("tol", C.c_float), ("min_inliers", C.c_int32), ("seed", C.c_uint32),
                ("normal_min_cos", C.c_float), ("axis", C.c_float * 3), ("axis_min_cos", C.c_float), ("mode", C.c_int32),
                ("plane", C.c_void_p), ("plane_count", C.c_void_p), ("hypothesis", C.c_void_p), ("label", C.c_void_p), ("index", C.c_void_p),
                ("dropped", C.c_void_p)]


class MdPointsClusters(C.Structure):
    """md_points_clusters (include/mi_depth.h)."""
    _fields_ = [("radius", C.c_float), ("min_neighbours", C.c_int32), ("min_points", C.c_int32), ("max_points", C.c_int32), ("mode", C.c_int32),
                ("label", C.c_void_p), ("cluster_size", C.c_void_p), ("cluster", C.c_void_p), ("table_label", C.c_void_p),
                ("table_size", C.c_void_p), ("box", C.c_void_p), ("table_capacity", C.c_int64), ("stats", C.c_void_p), ("index", C.c_void_p),
                ("dropped", C.c_void_p)]


class MdPointsMatch(C.Structure):
    """md_points_match (include/mi_depth.h)."""
    _fields_ = [("radius", C.c_float), ("target", C.c_void_p), ("target_rows", C.c_int64), ("target_kind", C.c_int32), ("mode", C.c_int32),
                ("tol", C.c_float * 4), ("nearest", C.c_void_p), ("dist2", C.c_void_p), ("stats", C.c_void_p), ("index", C.c_void_p),
                ("dropped", C.c_void_p)]


class MdPointsRegister(C.Structure):
    """md_points_register (include/mi_depth.h)."""
    _fields_ = [("radius", C.c_float), ("target", C.c_void_p), ("target_rows", C.c_int64), ("target_kind", C.c_int32),
                ("iterations", C.c_int32), ("min_pairs", C.c_int32), ("apply", C.c_int32), ("rot_eps", C.c_double), ("trans_eps", C.c_double),
                ("init", C.c_void_p), ("transform", C.c_void_p), ("pairs", C.c_void_p), ("sum_d2", C.c_void_p), ("stats", C.c_void_p),
                ("dropped", C.c_void_p), ("nearest", C.c_void_p), ("dist2", C.c_void_p)]


class MdPointsRegisterPlane(C.Structure):
    """md_points_register_plane (include/mi_depth.h)."""
    _fields_ = [("target_normals", C.c_void_p), ("sum_r2", C.c_void_p)]


class MdRenderOpts(C.Structure):
    """md_render_opts (include/mi_depth.h)."""
    _fields_ = [("pixel_offset", C.c_float), ("z_near", C.c_float), ("z_far", C.c_float), ("radius", C.c_int)]


class MdRenderOutputs(C.Structure):
    """md_render_outputs (include/mi_depth.h)."""
    _fields_ = [("depth", C.c_void_p), ("index", C.c_void_p), ("rgb", C.c_void_p), ("filled", C.c_void_p)]


class MdPointsRender(C.Structure):
    """md_points_render (include/mi_depth.h)."""
    _fields_ = [("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cam", MdPointsCameras), ("opts", MdRenderOpts), ("out", MdRenderOutputs)]


class MdPointsMesh(C.Structure):
    """md_points_mesh (include/mi_depth.h)."""
    _fields_ = [("max_rtol", C.c_float), ("faces", C.c_void_p), ("face_count", C.c_void_p), ("face_capacity", C.c_int64),
                ("pixel_index", C.c_void_p)]


class MdRasterOpts(C.Structure):
    """md_raster_opts (include/mi_depth.h)."""
    _fields_ = [("pixel_offset", C.c_float), ("z_near", C.c_float), ("z_far", C.c_float), ("cull", C.c_int), ("max_extent", C.c_int)]


class MdRasterOutputs(C.Structure):
    """md_raster_outputs (include/mi_depth.h)."""
    _fields_ = [("depth", C.c_void_p), ("face", C.c_void_p), ("rgb", C.c_void_p), ("filled", C.c_void_p), ("skipped", C.c_void_p)]


class MdPointsRaster(C.Structure):
    """md_points_raster (include/mi_depth.h)."""
    _fields_ = [("T", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cam", MdPointsCameras), ("opts", MdRasterOpts), ("out", MdRasterOutputs)]


class MdViewFilterOpts(C.Structure):
    """md_view_filter_opts (include/mi_depth.h)."""
    _fields_ = [("pixel_offset", C.c_float), ("depth_min", C.c_float), ("depth_max", C.c_float), ("conf_percentile", C.c_int),
                ("view_rtol", C.c_float), ("min_views", C.c_int)]


class MdViewFilterOutputs(C.Structure):
    """md_view_filter_outputs (include/mi_depth.h)."""
    _fields_ = [("depth", C.c_void_p), ("support", C.c_void_p), ("conf_threshold", C.c_void_p), ("kept", C.c_void_p)]


class MdDa3Cfg(C.Structure):
    _fields_ = [("variant", C.c_char_p), ("image_size", C.c_int), ("precision", C.c_int), ("max_batch", C.c_int),
                ("ln_eps", C.c_float), ("image_width", C.c_int)]


class MdVitGemmGroup(C.Structure):
    """md_vit_gemm_group (include/mi_depth.h)."""
    _fields_ = [("row0", C.c_int), ("rows", C.c_int), ("arow0", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p), ("scale", C.c_void_p),
                ("gamma_next", C.c_void_p), ("c", C.c_void_p), ("pos", C.c_void_p)]


class MdVitGemm(C.Structure):
    """md_vit_gemm (include/mi_depth.h)."""
    _fields_ = [("kind", C.c_int), ("precision", C.c_int), ("tile", C.c_int), ("N", C.c_int), ("K", C.c_int), ("a_rows", C.c_int),
                ("a", C.c_void_p), ("ngroups", C.c_int), ("g", MdVitGemmGroup * 4), ("out_rows", C.c_int), ("x", C.c_void_p),
                ("x_out", C.c_void_p), ("ln_out", C.c_void_p), ("ln_stats_out", C.c_void_p), ("ln_stats", C.c_void_p), ("ln_raw", C.c_int),
                ("ln_eps", C.c_float), ("ln_inv_n", C.c_float), ("S", C.c_int), ("D", C.c_int), ("P", C.c_int), ("qk", C.c_void_p),
                ("vT", C.c_void_p), ("out", C.c_void_p)]


class MdAttentionOp(C.Structure):
    """md_attention_op (include/mi_depth.h)."""
    _fields_ = [("T", C.c_int), ("V", C.c_int), ("N", C.c_int), ("heads", C.c_int), ("precision", C.c_int), ("seq_stride", C.c_int),
                ("kpad", C.c_int), ("out_fp8_inv", C.c_float), ("small", C.c_int), ("poison_pad", C.c_int), ("qkv", C.c_void_p),
                ("out", C.c_void_p)]


ATTN_FORMS = {-1: "none", 0: "plain", 1: "key-split", 2: "assembly", 3: "views", 4: "fp8-out", 5: "fp32-path"}  # md_attention_form


class MdDecoderGemmHeadCh(C.Structure):
    """md_decoder_gemm_head_ch (include/mi_depth.h)."""
    _fields_ = [("w", C.c_void_p), ("b", C.c_float), ("act", C.c_int), ("out", C.c_void_p), ("bstride", C.c_int64)]


class MdDecoderGemm(C.Structure):
    """md_decoder_gemm (include/mi_depth.h)."""
    _fields_ = [("kind", C.c_int), ("precision", C.c_int), ("tile", C.c_int), ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int),
                ("Cin_p", C.c_int), ("Cout", C.c_int), ("ngroups", C.c_int), ("in_shared", C.c_int), ("res1_shared", C.c_int),
                ("w", C.c_void_p * 2), ("bias", C.c_void_p * 2), ("in_", C.c_void_p), ("act", C.c_int), ("res1", C.c_void_p), ("res2", C.c_void_p),
                ("res_mod", C.c_int), ("out", C.c_void_p), ("out2", C.c_void_p), ("ldo", C.c_int), ("out_f32", C.c_int), ("ps_f", C.c_int),
                ("ps_coff", C.c_int), ("head_nch", C.c_int), ("ch", MdDecoderGemmHeadCh * 8), ("head_w", C.c_void_p), ("head_b", C.c_float),
                ("head_act", C.c_int), ("Cmid", C.c_int), ("w2", C.c_void_p), ("bias2", C.c_void_p)]


class MdIndexedGemm(C.Structure):
    """md_indexed_gemm (include/mi_depth.h)."""
    _fields_ = [("kind", C.c_int), ("precision", C.c_int), ("tile", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("rows_a", C.c_int),
                ("a", C.c_void_p), ("index", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("res1", C.c_void_p), ("res_mod", C.c_int),
                ("out", C.c_void_p), ("out_rows", C.c_int64), ("ldo", C.c_int), ("out_f32", C.c_int), ("B", C.c_int),
                ("ph", C.c_int), ("pw", C.c_int), ("ps_f", C.c_int), ("ps_coff", C.c_int)]


class MdCameraEncode(C.Structure):
    """md_camera_encode (include/mi_depth.h)."""
    _fields_ = [("B", C.c_int), ("V", C.c_int), ("D", C.c_int), ("heads", C.c_int), ("depth", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("eps_tok", C.c_float), ("eps_blk", C.c_float), ("w", C.c_void_p * 8), ("blk", (C.c_void_p * 14) * 8), ("extr", C.c_void_p),
                ("intr", C.c_void_p), ("out", C.c_void_p), ("pose_out", C.c_void_p)]


class MdCameraDecode(C.Structure):
    """md_camera_decode (include/mi_depth.h)."""
    _fields_ = [("B", C.c_int), ("din", C.c_int), ("H", C.c_int), ("W", C.c_int), ("cam", C.c_void_p), ("w", C.c_void_p * 10),
                ("pose", C.c_void_p), ("extr", C.c_void_p), ("intr", C.c_void_p)]


class MdNchwView(C.Structure):
    """md_nchw_view (include/mi_depth.h): one NCHW fp32 tensor with its shape."""
    _fields_ = [("data", C.c_void_p), ("channels", C.c_int), ("height", C.c_int), ("width", C.c_int)]


class MdHeadDebug(C.Structure):
    """md_head_debug (include/mi_depth.h) = `HeadDebug`, depth_pro/mod.rs:135-142."""
    _fields_ = [("conv0", C.c_void_p), ("deconv", C.c_void_p), ("conv1", C.c_void_p), ("relu", C.c_void_p),
                ("pre_out", C.c_void_p), ("canonical", C.c_void_p)]


class MdDepthProCfg(C.Structure):
    _fields_ = [
        ("patch_encoder_preset", C.c_char_p),
        ("image_encoder_preset", C.c_char_p),
        ("fov_encoder_preset", C.c_char_p),
        ("decoder_features", C.c_int),
        ("use_fov_head", C.c_int),
        ("interpolation", C.c_int),
        ("precision", C.c_int),
        ("max_batch", C.c_int),
        ("ln_eps", C.c_float),
    ]


# every symbol include/mi_depth.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
_I = C.c_int
SYMBOLS = {
    "md_last_error": (C.c_char_p, []),
    "md_version": (C.c_char_p, []),
    "md_device_open": (_I, [_I, C.POINTER(_P)]),
    "md_device_close": (_I, [_P]),
    "md_device_synchronize": (_I, [_P]),
    "md_depth_pro_cfg_default": (None, [C.POINTER(MdDepthProCfg)]),
    "md_depth_pro_create": (_I, [_P, C.POINTER(MdDepthProCfg), C.c_uint64, _I, C.POINTER(_P)]),
    "md_depth_pro_load": (_I, [_P, C.c_char_p, C.POINTER(_P)]),
    "md_depth_pro_load_with_config": (_I, [_P, C.POINTER(MdDepthProCfg), C.c_char_p, C.POINTER(_P)]),
    "md_checkpoint_info": (_I, [C.c_char_p, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(_I), C.POINTER(C.c_int64 * 8), C.POINTER(_I)]),
    "md_checkpoint_read_tensor": (_I, [C.c_char_p, C.c_char_p, _P, C.c_size_t]),
    "md_model_set_tensor": (_I, [_P, C.c_char_p, _P, C.c_size_t]),
    "md_model_get_tensor": (_I, [_P, C.c_char_p, _P, C.c_size_t]),
    "md_model_param_count": (_I, [_P]),
    "md_model_param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]),
    "md_model_commit_weights": (_I, [_P]),
    "md_model_round_weights_f16": (_I, [_P]),
    "md_model_weight_arena": (_I, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "md_model_destroy": (_I, [_P]),
    "md_model_fork": (_I, [_P, C.POINTER(_P)]),
    "md_depth_pro_infer": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "md_depth_pro_infer_with_focal": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "md_depth_pro_decoder_from_features": (_I, [_P, C.POINTER(MdNchwView), _I, _I, _I, _P, _P, C.POINTER(C.c_void_p), _I, _P]),
    "md_depth_pro_head_debug": (_I, [_P, C.POINTER(MdNchwView), _I, _I, C.POINTER(MdHeadDebug), _I, _P]),
    "md_depth_pro_infer_windows": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "md_infer_from_rgb": (_I, [_P, _P, C.c_size_t, _I, _I, _I, _P, _P, _P, _I, _P]),
    "md_infer_from_rgb_with_focal": (_I, [_P, _P, C.c_size_t, _I, _I, _I, C.c_float, _P, _P, _P, _I, _P]),
    "md_frame_geometry": (_I, [_P, _I, _I, C.POINTER(MdFrameOpts), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "md_process_frame": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(MdFrameOpts), C.POINTER(MdFrameOutputs), _I, _P]),
    "md_points_opts_default": (None, [C.POINTER(MdPointsOpts)]),
    "md_op_unproject": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdPointsOpts), C.POINTER(MdPointsOutputs), _P]),
    "md_view_filter_opts_default": (None, [C.POINTER(MdViewFilterOpts)]),
    "md_op_filter_views": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdViewFilterOpts),
                                C.POINTER(MdViewFilterOutputs), _P]),
    "md_op_unproject_normals": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdPointsOpts),
                                     C.POINTER(MdPointsOutputs), C.POINTER(MdPointsNormals), _P]),
    "md_op_voxel_thin": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(MdPointsVoxel), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_render_opts_default": (None, [C.POINTER(MdRenderOpts)]),
    "md_op_render_points": (_I, [_P, _P, _P, C.c_int64, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdRenderOpts),
                                 C.POINTER(MdRenderOutputs), _P]),
    "md_op_mesh_grid": (_I, [_P, _P, _P, _I, _I, _I, _I, C.c_int64, C.POINTER(MdPointsMesh), _P]),
    "md_op_unproject_mesh": (_I, [_P, _P, _P, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdPointsOpts),
                                  C.POINTER(MdPointsOutputs), C.POINTER(MdPointsNormals), C.POINTER(MdPointsMesh), _P]),
    "md_raster_opts_default": (None, [C.POINTER(MdRasterOpts)]),
    "md_op_render_mesh": (_I, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P, _I, _I, _I, C.POINTER(MdPointsCameras), C.POINTER(MdRasterOpts),
                               C.POINTER(MdRasterOutputs), _P]),
    "md_op_radius_outliers": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(MdPointsOutlier), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_decimate_mesh": (_I, [_P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, C.POINTER(MdPointsDecimate), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_mesh_components": (_I, [_P, _P, _P, _P, _P, C.c_int64, _P, C.c_int64, C.POINTER(MdPointsComponents), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_smooth_mesh": (_I, [_P, _P, C.c_int64, _P, C.c_int64, C.POINTER(MdPointsSmooth), C.c_int64, _P]),
    "md_op_fit_planes": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(MdPointsPlanes), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_cluster_points": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(MdPointsClusters), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_match_points": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.POINTER(MdPointsMatch), C.POINTER(MdPointsOutputs), _P, _P]),
    "md_op_register_points": (_I, [_P, _P, _P, C.c_int64, C.POINTER(MdPointsRegister), _P, _P, _P]),
    "md_op_register_points_plane": (_I, [_P, _P, _P, C.c_int64, C.POINTER(MdPointsRegister), C.POINTER(MdPointsRegisterPlane), _P, _P, _P]),
    "md_raster_inline_pixels": (_I, []),
    "md_debug_raster_queue": (_I, [_I]),
    "md_da3_cfg_default": (None, [C.POINTER(MdDa3Cfg)]),
    "md_da3_create": (_I, [_P, C.POINTER(MdDa3Cfg), C.c_uint64, _I, C.POINTER(_P)]),
    "md_da3_load": (_I, [_P, C.POINTER(MdDa3Cfg), C.c_char_p, C.POINTER(_P)]),
    "md_da3_infer": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "md_da3_infer_ex": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "md_da3_infer_views": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "md_model_enable_graph": (_I, [_P, _I]),
    "md_da3_infer_with_camera": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _P]),
    "md_gemm_ksplit_launches": (_I, []),
    "md_debug_gemm_direct_store": (_I, [_I]),
    "md_debug_gemm_persistent": (_I, [_I]),
    "md_debug_gemm_stagger": (_I, [_I, _I]),
    "md_debug_gemm_stagger_ticks": (_I, [_I]),
    "md_da3_infer_raw": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P]),
    "md_da3_infer_from_tokens": (_I, [_P, C.POINTER(C.c_void_p), _I, _I, _I, _I, _I, _P, _I, _P]),
    "md_da3_param_inventory": (_I, [C.POINTER(MdDa3Cfg), _I, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), _F, _F]),
    "md_model_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_int64)]),
    "md_model_set_option": (_I, [_P, C.c_char_p, C.c_int64]),
    "md_model_enable_taps": (_I, [_P, _I]),
    "md_model_read_tap": (_I, [_P, C.c_char_p, _P, C.c_size_t, C.POINTER(C.c_int64 * 4)]),
    "md_model_enable_timing": (_I, [_P, _I]),
    "md_model_set_timing_filter": (_I, [_P, C.c_char_p]),
    "md_model_read_timing": (_I, [_P, C.POINTER(C.c_char_p), _F, C.POINTER(_I), _I, C.POINTER(_I)]),
    "md_model_read_launch_order": (_I, [_P, C.POINTER(C.c_char_p), _I, C.POINTER(_I)]),
    "md_op_rgb_to_input": (_I, [_P, _P, C.c_size_t, _I, _I, _P, _P]),
    "md_catmull_rom_taps": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), _F]),
    "md_op_resize_catmull_rom": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "md_op_depth_display": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "md_op_resize_bilinear": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "md_op_resize_bilinear_ex": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "md_op_pyramid_patchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, C.POINTER(_I), C.POINTER(_I), _P]),
    "md_op_resize_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P]),
    "md_op_resize_nhwc_ex": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _I, _P]),
    "md_op_resize_output_size": (_I, [_I, _I, C.c_float, C.c_float, C.POINTER(_I), C.POINTER(_I)]),
    "md_op_split": (_I, [_P, _P, _I, _I, _I, _I, C.c_float, _P, C.POINTER(_I), _P]),
    "md_op_merge": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, C.POINTER(_I), C.POINTER(_I), _P]),
    "md_op_layernorm": (_I, [_P, _P, _P, _P, _I, _I, C.c_float, _P, _P]),
    "md_op_linear": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_linear_tile": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_attention": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "md_op_attention_views": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_attention_ex": (_I, [_P, C.POINTER(MdAttentionOp), _P]),
    "md_debug_attention_last_form": (_I, [C.POINTER(_I * 4)]),
    "md_op_conv3x3": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_deconv2x2": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_conv2d_direct": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_qkv_norm_rope": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _P, _P, _P]),
    "md_op_qk_norm_rope": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _I, _P, _P]),
    "md_op_hook_cat_ln": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, C.c_float, _P, _P, C.c_float, _I, _P, _P, _P]),
    "md_op_patchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
    "md_op_set_token0": (_I, [_P, _P, _I, _I, _I, _P, _I, _P]),
    "md_op_border_bias_fix": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P]),
    "md_op_compose_weights": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "md_op_layernorm_ex": (_I, [_P, _P, _I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_P), C.POINTER(_P), C.c_float, _I, _I,
                                C.c_float, _P, _I, _P, _P]),
    "md_op_store_rows": (_I, [_P, _P, C.c_int64, _I, _I, _P, _P]),
    "md_op_load_rows": (_I, [_P, _P, C.c_int64, _I, _I, _P, _P]),
    "md_op_f32_to_fp8": (_I, [_P, _P, C.c_int64, C.c_float, _P, _P]),
    "md_op_pack_fp8_rows": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "md_op_nchw_to_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_nhwc_to_nchw": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_ln_fold_vectors": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "md_op_ln_finish": (_I, [_P, _P, C.c_int64, C.c_float, C.c_float, _P, _P]),
    "md_op_vit_gemm": (_I, [_P, C.POINTER(MdVitGemm), _P]),
    "md_debug_gemm_last_form": (_I, [C.POINTER(_I * 8)]),
    "md_debug_gemm_last_launch": (_I, [C.POINTER(_I * 4)]),
    "md_op_decoder_gemm": (_I, [_P, C.POINTER(MdDecoderGemm), _P]),
    "md_op_indexed_gemm": (_I, [_P, C.POINTER(MdIndexedGemm), _P]),
    "md_op_merge_index_table": (_I, [_I, _I, _I, _I, _I, _I, _P, C.c_int64]),
    "md_op_token_index_table": (_I, [_I, _I, _I, _I, _P, C.c_int64]),
    "md_op_camera_encode": (_I, [_P, C.POINTER(MdCameraEncode), _P]),
    "md_op_camera_decode": (_I, [_P, C.POINTER(MdCameraDecode), _P]),
    "md_op_pose_to_camera": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "md_op_conv2d_direct_ex": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "md_op_fov_to_focal": (_I, [C.c_float, _I, _I, _F, _F]),
    "md_op_focal_to_fov": (_I, [C.c_float, _I, _I, _F, _F]),
    "md_bench_gemm": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _F]),
    "md_gemm_pick_tile": (_I, [_I, _I, _I, _I]),
    "md_bench_attention": (_I, [_P, _I, _I, _I, _I, _F]),
    "md_bench_attention_ex": (_I, [_P, _I, _I, _I, _I, C.c_float, _I, _F]),
    "md_debug_attention_asm": (_I, [_I]),
    "md_debug_attention_asm_launches": (C.c_long, []),
    "md_debug_attention_redo_units": (C.c_long, [_P, _I]),
    "md_bench_attention_qkv": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, C.POINTER(C.c_long)]),
    "md_comm_unique_id": (_I, [_P]),
    "md_comm_init_rank": (_I, [_P, _P, _I, _I, C.POINTER(_P)]),
    "md_comm_rank": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "md_comm_count": (_I, [_P, C.POINTER(_I)]),
    "md_comm_destroy": (_I, [_P]),
    "md_comm_broadcast_weights": (_I, [_P, _P, _I]),
    "md_comm_scatter_images": (_I, [_P, _P, _P, C.c_size_t, _I, _P]),
    "md_comm_gather_depth": (_I, [_P, _P, _P, C.c_size_t, _I, _P]),
    "md_depth_pro_infer_tiles_loopback": (_I, [C.POINTER(_P), _I, _I, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _P]),
    "md_comm_depth_pro_infer_tiles": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "md_param_inventory": (_I, [C.POINTER(MdDepthProCfg), _I, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), _F, _F]),
    "md_uniform_stream": (_I, [C.c_char_p, C.c_uint64, C.c_size_t, C.c_float, C.c_float, _P]),
    "md_split_geometry": (_I, [_I, _I, C.c_float, C.POINTER(_I), C.POINTER(_I)]),
    "md_feature_padding": (_I, [_I, _I, _I]),
}


def _infer_points(*parts):
    """An md_infer_points* entry: (model, image, B, H, W, in_kind, rgb, cameras, its parts, out_kind, stream)."""
    return _I, [_P, _P, _I, _I, _I, _I, _P, C.POINTER(MdPointsCameras), *(C.POINTER(p) for p in parts), _I, _P]


# every entry behind `_filtered` takes the widest entry's parts up to its own; md_infer_points has no view filter
_POINTS_HEAD = [MdViewFilterOpts, MdPointsOpts, MdPointsOutputs]
_POINTS_PARTS = [("normals", MdPointsNormals), ("voxel", MdPointsVoxel), ("render", MdPointsRender), ("mesh", MdPointsMesh),
                 ("raster", MdPointsRaster), ("outlier", MdPointsOutlier), ("decimate", MdPointsDecimate), ("components", MdPointsComponents),
                 ("smooth", MdPointsSmooth), ("planes", MdPointsPlanes), ("clusters", MdPointsClusters),
                 ("match", MdPointsMatch), ("register", MdPointsRegister), ("register_plane", MdPointsRegisterPlane)]
SYMBOLS["md_infer_points"] = _infer_points(*_POINTS_HEAD[1:])
SYMBOLS["md_infer_points_filtered"] = _infer_points(*_POINTS_HEAD)
SYMBOLS.update({f"md_infer_points_{name}": _infer_points(*_POINTS_HEAD, *(p for _, p in _POINTS_PARTS[:i + 1]))
                for i, (name, _) in enumerate(_POINTS_PARTS)})

_lib = None


def load() -> C.CDLL:
    """Load libmi_depth.so (built by `__graft_entry__.build()` / `make -C burn_depth_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
            "burn_depth_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted from the header
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != MD_OK:
        msg = load().md_last_error()
        raise MdError(code, msg.decode("utf-8", "replace") if msg else "")
