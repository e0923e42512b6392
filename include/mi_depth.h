/*
 * mi_depth.h -- C ABI of libmi_depth.so, the MI355X-native (gfx950) drop-in for the hot path
 * of mosure/burn_depth: DepthPro::load / DepthPro::infer (and the helpers either side of it).
 *
 * Every entry point cites the reference interface it replaces (path:line under the reference
 * repository).  Plain pointers and sizes only; no torch / HIP types in the signatures (a
 * hipStream_t is passed as void*).  All functions return 0 (MD_OK) or a negative md_status and
 * record a message retrievable with md_last_error() -- the reference's panics
 * (expect!/assert!/panic!) become checked preconditions with distinct codes, never aborts.
 *
 * Threading: one in-flight infer per md_model_t (the workspace arena is per model), matching
 * the reference's `infer(&self)` + per-caller Mutex usage (crates/bevy_burn_depth/src/lib.rs:18,29).
 */
#ifndef MI_DEPTH_H
#define MI_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct md_device_s* md_device_t;
typedef struct md_model_s* md_model_t;

typedef enum md_status {
  MD_OK = 0,
  MD_ERR_INVALID_ARG = -1, /* null pointer, unknown preset/key (vit.rs:49-50 panic)            */
  MD_ERR_SHAPE = -2,       /* bad B/H/W, RGB length mismatch (inference.rs:90-95 Err)           */
  MD_ERR_IO = -3,          /* file cannot be read (RecorderError, mod.rs:193-208)               */
  MD_ERR_FORMAT = -4,      /* container malformed / tensor missing or wrong shape               */
  MD_ERR_HIP = -5,         /* HIP runtime failure                                               */
  MD_ERR_UNSUPPORTED = -6, /* configuration outside what the kernels support                    */
  MD_ERR_NO_FOV = -7,      /* "FOV head required for focal length" (mod.rs:329 expect)          */
  MD_ERR_OOM = -8,         /* workspace arena exhausted                                         */
  MD_ERR_LEVELS = -9       /* decoder level-count mismatch (decoder.rs:200-205 panic)           */
} md_status;

typedef enum md_mem_kind { MD_MEM_HOST = 0, MD_MEM_DEVICE = 1 } md_mem_kind;
/* Arithmetic type of the MFMA operands; accumulation, LayerNorm, softmax and the final
 * focal/clamp/reciprocal are fp32 in both modes. */
/* MD_PREC_FP8 (Depth-Anything-v3 only, BASELINE config 5): bf16 everywhere except the four ViT linear layers
 * (qkv, proj, fc1, fc2), which run on OCP e4m3 MFMA operands -- weights quantised per output channel at commit,
 * activations with static per-tensor scales -- with fp32 accumulation. */
/* MD_PREC_F16: IEEE half MFMA operands (v_mfma_f32_*_f16, the bf16 rate) -- the reference stores its weights as f16
 * (`HalfPrecisionSettings`, depth_pro/mod.rs:206), so checkpoint weights are exact operands and activations carry 3
 * more mantissa bits than bf16; stores saturate at +-65504. The accurate fast mode. */
/* MD_PREC_F16X2 (Depth Pro): the accurate FAST mode. Every activation that feeds an MFMA is kept as two IEEE-half planes,
 * value = hi + lo (hi = f16(x), lo = f16(x - hi): 22 significant bits); the reference's checkpoints are f16
 * (`HalfPrecisionSettings`, depth_pro/mod.rs:206), so a weight is an exact f16 operand and every product is two
 * v_mfma_f32_*_f16 with fp32 accumulation (W.x_hi + W.x_lo). Weights that are NOT f16-exact (fp32 checkpoints, the layer
 * products composed at commit) are kept as hi + lo too and cost a third MFMA (W_lo.x_hi); md_model_query("weight_terms")
 * says which form the committed weights took. q.k^T runs on three terms, softmax and every sum stay fp32. */
typedef enum md_precision { MD_PREC_BF16 = 0, MD_PREC_F32 = 1, MD_PREC_FP8 = 2, MD_PREC_F16 = 3, MD_PREC_F16X2 = 4 } md_precision;
/* depth_pro/interpolate.rs:11-22 */
/* Stand-alone operator checks only (md_op_linear*, md_op_conv3x3, md_op_deconv2x2): OR into `precision` to route the
 * result through the engine's storage type (bf16 in the BF16 / FP8 modes) before it is widened to the fp32 output --
 * the store epilogues the engine itself uses -- instead of the fp32 store. Ignored for MD_PREC_F32. */
#define MD_OP_STORAGE_OUT 0x100
/* OR into `precision` of md_op_attention / md_op_attention_views (16-bit modes): the staging tensors' padding -- the rows between N and
 * the sequence stride, the slack rows behind the last sequence, the V^T columns between N and the padded key count -- holds a large
 * finite value instead of zero before the kernel runs. The result must not change by a bit: the kernel masks what it over-reads. */
#define MD_OP_POISON_PAD 0x200
typedef enum md_interp { MD_INTERP_CUSTOM = 0, MD_INTERP_BURN = 1 } md_interp;
/* synthetic initialisation (no trained weights exist in the reference tree) */
typedef enum md_init_scheme { MD_INIT_REFERENCE = 0, MD_INIT_PARITY = 1 } md_init_scheme;

/* DepthProConfig, depth_pro/mod.rs:35-66 (same fields, same defaults via md_depth_pro_cfg_default). */
typedef struct md_depth_pro_cfg {
  const char* patch_encoder_preset; /* "dinov2l16_384" | "dinov2l16_128" | "tiny16_128" */
  const char* image_encoder_preset;
  const char* fov_encoder_preset;   /* NULL = FOV head without its own ViT (fov.rs:118-155) */
  int decoder_features;             /* 256 */
  int use_fov_head;                 /* 1 */
  int interpolation;                /* md_interp, default CUSTOM */
  int precision;                    /* md_precision, engine-side addition */
  int max_batch;                    /* images per infer call the workspace is sized for */
  float ln_eps;                     /* burn_dino's LayerNorm eps is not visible; default 1e-6 */
} md_depth_pro_cfg;

/* Last error message of the calling thread ("" if none). Maps RecorderError / String errors. */
const char* md_last_error(void);
/* Library version string. */
const char* md_version(void);

/* `<B as Backend>::Device::default()` (README.md:21, src/lib.rs:15-22): one device = one GPU. */
int md_device_open(int hip_ordinal, md_device_t* out);
int md_device_close(md_device_t dev);
int md_device_synchronize(md_device_t dev); /* `B::sync(&device)` (bench/inference.rs:46) */

/* `DepthProConfig::default()` (depth_pro/mod.rs:54-66). */
void md_depth_pro_cfg_default(md_depth_pro_cfg* cfg);

/* `DepthPro::new(&device, cfg)` (depth_pro/mod.rs:145-191): seeded synthetic initialisation. */
int md_depth_pro_create(md_device_t dev, const md_depth_pro_cfg* cfg, uint64_t seed, int init_scheme,
                        md_model_t* out);
/* `DepthPro::load(&device, path)` (depth_pro/mod.rs:193-198): default config. `path` is either
 *  - the reference's own checkpoint: a Burn `NamedMpkFileRecorder<HalfPrecisionSettings>` record (`.mpk`, mod.rs:206) --
 *    MessagePack, tensors keyed by Burn field path, `nn::Linear` weights [d_input, d_output] (transposed on load); the reader
 *    follows Burn 0.19's published record layout and is UNVALIDATED ON A REAL BURN RECORD (none exists in the reference tree);
 *  - or the engine's safetensors container keyed by the same field paths (tools/import_weights.py).
 * The format is recognised from the first bytes of the file, not from its name. */
int md_depth_pro_load(md_device_t dev, const char* path, md_model_t* out);
/* `DepthPro::load_with_config` (depth_pro/mod.rs:200-208). */
int md_depth_pro_load_with_config(md_device_t dev, const md_depth_pro_cfg* cfg, const char* path,
                                  md_model_t* out);
/* Host-only view of a checkpoint file (either format above; no device needed): the number of tensors it holds, and for
 * 0 <= index < that number the tensor's name (Burn field path), dtype ("F16" | "F32" | "BF16"), rank and shape as stored in
 * the file (a Burn record's Linear weights read [d_input, d_output] here). `name` / `dtype` point into thread-local storage
 * that lives until the next call on this thread. Returns the tensor count, or a negative MD_ERR_* code. */
int md_checkpoint_info(const char* path, int index, const char** name, const char** dtype, int* rank, int64_t shape[8],
                       int* is_burn_record);
/* The values of one tensor of a checkpoint file widened to fp32, in the file's own element order (`count` must match). */
int md_checkpoint_read_tensor(const char* path, const char* name, float* out_host, size_t count);
/* `Module::load_record` / `into_record` (src/lib.rs:163-177): read or replace one named
 * parameter with host fp32 data. `count` = number of elements and must match. */
int md_model_set_tensor(md_model_t m, const char* name, const float* host_data, size_t count);
int md_model_get_tensor(md_model_t m, const char* name, float* host_data, size_t count);
/* Number of parameters / name+element count of the i-th one (fixed inventory order). */
int md_model_param_count(md_model_t m);
int md_model_param_info(md_model_t m, int index, const char** name, size_t* count);
/* Must be called after md_model_set_tensor calls and before the next infer: re-packs the
 * MFMA operand copies (bf16, [N][K] / tap-major layouts) from the fp32 master weights. */
int md_model_commit_weights(md_model_t m);
/* `DepthPro::load` reads an f16 record (`NamedMpkFileRecorder<HalfPrecisionSettings>`, depth_pro/mod.rs:193-208): every
 * parameter of a loaded reference model is an IEEE half widened to f32. Rounds the fp32 master copy of every parameter the
 * same way, in place, and commits -- turns a seeded (md_depth_pro_create) or fp32-loaded model into what the reference's
 * f16 checkpoint of the same weights would give. In MD_PREC_F16X2 the committed weights are then exact MFMA operands
 * (two terms per product instead of three: md_model_query "weight_terms"). */
int md_model_round_weights_f16(md_model_t m);
/* The packed device-resident weight arena (for an RCCL broadcast from rank 0). */
int md_model_weight_arena(md_model_t m, void** device_ptr, size_t* bytes);
int md_model_destroy(md_model_t m);
/* `Clone` of a loaded model / sharing `&DepthPro` between threads (`DepthPro` is `Module + Clone + Debug`,
 * depth_pro/mod.rs:119-126; `infer(&self)`, mod.rs:312; the viewer shares one model behind an Arc,
 * crates/bevy_burn_depth/src/lib.rs:18,29): a second inference context on the SAME weights. The fork aliases the root
 * model's parameter and packed-operand arenas (no copy of the 5.6 GB) and owns a workspace arena, index tables, taps,
 * timing, graphs and a default stream of its own, so one infer per context may be in flight concurrently (the
 * threading rule at the top of this file then holds per context). set_tensor / commit / weight_arena are rejected on
 * a fork; the root must be destroyed after its forks (MD_ERR_INVALID_ARG otherwise). Depth Pro models only:
 * Depth-Anything-v3 models keep per-shape tables beside their workspace, like the reference's `CachedDepthAnything3`
 * (depth_anything3/mod.rs:44,67-70, not Sync) -> MD_ERR_UNSUPPORTED. */
int md_model_fork(md_model_t m, md_model_t* out);

/* `DepthPro::infer(&self, x)` (depth_pro/mod.rs:312-364). Input NCHW fp32, ImageNet-normalised,
 * any H x W (resized to img_size^2 and back like the reference). Outputs (DepthProInference,
 * mod.rs:128-133): depth[B*H*W], focallength_px[B], fovx_deg[B], fovy_rad[B]; any output pointer
 * may be NULL to skip it. in_kind/out_kind say whether the pointers are host or device memory.
 * `stream` is a hipStream_t (NULL = the model's own stream); the call is asynchronous for
 * device outputs and synchronises for host outputs. Host pointers may be pageable memory: they travel through pinned bounce
 * buffers owned by the model (grow-only, like the device staging for H x W != img_size: no allocation per call). */
int md_depth_pro_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth,
                       float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind, void* stream);

/* `md_depth_pro_infer` with the caller's focal length (Apple ml-depth-pro's `infer(x, f_px)`; burn_depth's README passes
 * `None`): f_px[B] fp32, one focal length per image in pixels of the input as passed (width W before any resize), in memory of
 * kind `in_kind` like the image. f_px == NULL is exactly md_depth_pro_infer (same launches, same bits, MD_ERR_NO_FOV without a
 * FOV head). With f_px the FOV encoder and head do not run -- a model built with use_fov_head = 0 infers depth this way -- and
 *   focallength_px = f_px (bit for bit), fovx_deg = 2 atan(W / (2 f_px)) in degrees, fovy_rad from that fovx through the
 *   reference's fovy_from_fovx_rad (mod.rs:370-414), depth = mod.rs:330-363 with ratio = W / f_px
 * (an f_px equal to the predicted focal length gives md_depth_pro_infer's depth bit for bit). Host values that are not finite
 * or not > 0 -> MD_ERR_INVALID_ARG before anything is launched; device values are not inspected (the call stays
 * asynchronous) and are read at run time, also by a replayed graph. One batch is either all known or all predicted. */
int md_depth_pro_infer_with_focal(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const float* f_px,
                                  float* depth, float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind,
                                  void* stream);

/* One NCHW fp32 tensor handed across the boundary with its shape: `data` is [B, channels, height, width] (B is the call's). */
typedef struct md_nchw_view {
  const float* data;
  int channels, height, width;
} md_nchw_view;

/* `DepthPro::decoder_from_features(&self, features: &[Tensor<B,4>]) -> (Tensor<B,4>, Tensor<B,4>, Vec<Tensor<B,4>>)`
 * (depth_pro/mod.rs:262-267 = `MultiresConvDecoder::forward_with_debug`, layers/decoder.rs:195-222): the decoder alone on
 * CALLER-SUPPLIED encoder features -- the entry the reference's harness uses to replay the decoder on PyTorch's encoder
 * features (example/correctness.rs:538-560). `features[l]`, l = 0 .. levels-1, finest first: the default configuration takes
 * [B,256,768,768], [B,256,384,384], [B,512,192,192], [B,1024,96,96], [B,1024,48,48] (md_model_query "decoder_levels",
 * "decoder_level{l}_channels", "decoder_level{l}_size"). Outputs, NCHW fp32, any pointer may be NULL to skip it:
 *   out_features [B, F, s0, s0]  the fused feature map (what the depth head takes),
 *   out_lowres   [B, F, s4, s4]  `convs[last](features[last])`, the FOV network's input,
 *   out_fusions[l]               the output of fusion block l (index 0 = finest, as the reference returns them after its
 *                                `reverse()`): [B, F, 2 s_l, 2 s_l] for l >= 1, [B, F, s0, s0] for l = 0 (== out_features).
 * A wrong number of levels -> MD_ERR_LEVELS (the reference panics, decoder.rs:200-205); a level whose shape is not the
 * model's -> MD_ERR_SHAPE (Burn panics on the mismatched convolution / addition). Runs in the model's precision mode on the kernels `md_depth_pro_infer` runs; it is a debug entry (taps
 * machinery: eager, allocates its fp32 staging per call), not a hot path. */
int md_depth_pro_decoder_from_features(md_model_t m, const md_nchw_view* features, int levels, int B, int in_kind,
                                       float* out_features, float* out_lowres, float* const* out_fusions, int out_kind,
                                       void* stream);

/* `HeadDebug` (depth_pro/mod.rs:135-142): the six tensors `DepthPro::head_debug(&self, feature)` returns (mod.rs:289-307).
 * NCHW fp32; NULL fields are skipped. With s = the decoder feature's size (768 by default) and F = decoder_features:
 * conv0 [B,F/2,s,s], deconv [B,F/2,2s,2s], conv1 and relu [B,32,2s,2s], pre_out and canonical [B,1,2s,2s]. */
typedef struct md_head_debug {
  float* conv0;
  float* deconv;
  float* conv1;
  float* relu;
  float* pre_out;
  float* canonical;
} md_head_debug;

/* `DepthPro::head_debug(&self, feature: Tensor<B,4>) -> HeadDebug` (depth_pro/mod.rs:289-307): the depth head layer by layer
 * on a CALLER-SUPPLIED decoder feature [B, F, s, s] (example/correctness.rs:382-390 feeds it the decoder's output). Every
 * layer runs UN-FUSED here (conv0 3x3, deconv k2s2, conv1 3x3, relu, conv_out 1x1, relu), each tensor materialised in the
 * model's precision mode; `md_depth_pro_infer` runs the same arithmetic with conv_out . relu behind conv1's accumulators and
 * the deconv composed into conv1, so in MD_PREC_F32 the two agree to fp32 rounding and in the 16-bit
 * modes to the rounding of the materialised intermediates. A shape that is not the model's -> MD_ERR_SHAPE. Debug entry. */
int md_depth_pro_head_debug(md_model_t m, const md_nchw_view* feature, int B, int in_kind, const md_head_debug* out,
                            int out_kind, void* stream);

/* The same call with the ViT stage run as `parts` consecutive windows of its 37 B sequences (35 B patch tiles + B image +
 * B fov, layers/encoder.rs:329-348, 409; fov.rs:203) on THIS device: the launches the `parts` ranks of
 * md_comm_depth_pro_infer_tiles issue, one rank after the other, without the exchange. Results are bit-identical to
 * md_depth_pro_infer (the tiles never interact before `merge`). Single-GPU test and projection tool of the tile-parallel
 * mode: window_ms[parts] / tail_ms (either may be NULL) receive the GPU milliseconds of each window and of everything
 * behind the ViT stage, so max(window_ms) + tail_ms is the device time of one frame on `parts` GPUs before the exchange.
 * 1 <= parts <= 64; synchronises the stream when timings are requested. */
int md_depth_pro_infer_windows(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth,
                               float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind, int parts,
                               float* window_ms, float* tail_ms, void* stream);

/* `infer_from_rgb` + `rgb_to_input_tensor` (src/inference.rs:79-137): packed RGB bytes,
 * row-major, `rgb_len` must equal w*h*3 (else MD_ERR_SHAPE, as the reference's Err). B = 1. */
int md_infer_from_rgb(md_model_t m, const uint8_t* rgb, size_t rgb_len, int w, int h, int in_kind,
                      float* depth, float* focallength_px, float* fovy_rad, int out_kind, void* stream);

/* md_infer_from_rgb with the caller's focal length f_px (a host scalar, pixels of the w-wide image): the outputs of
 * md_depth_pro_infer_with_focal. A value that is not finite or not > 0 -> MD_ERR_INVALID_ARG. */
int md_infer_from_rgb_with_focal(md_model_t m, const uint8_t* rgb, size_t rgb_len, int w, int h, int in_kind,
                                 float f_px, float* depth, float* focallength_px, float* fovy_rad, int out_kind,
                                 void* stream);

/* ---- frame path: u8 RGB camera frames in, a displayable depth map out (the viewer's `process_frame`,
 * crates/bevy_burn_depth/src/lib.rs:16-132, and the CLI's prepare / save_depth_map, example/inference.rs:79-273) ---------
 * Everything runs on the device in one call: preparation (Catmull-Rom resize + centre crop, or a patch-aligned crop, and
 * the input normalisation), the model, and the display step (crop back to the frame's aspect, bilinear restore to the
 * frame's size, per-frame min-max over the finite values, grey u8 or RGBA f32). */
#define MD_FRAME_U8_GRAY 0  /* u8 [B,oh,ow]: floor(n * 255 + 0.5), the CLI's PNG pixels; needs normalize = 1 */
#define MD_FRAME_RGBA_F32 1 /* f32 [B,oh,ow,4]: (n, n, n, 1), the viewer's texture */
typedef struct md_frame_opts {
  int target;    /* Depth-Anything-v3: > 0 shortest-side Catmull-Rom resize to target (raised to the patch size) + centre
                    crop (prepare_depth_anything3_image); 0 = the model's img_size; -1 = patch-aligned centre crop, no resize
                    (prepare_input_frame without a preferred resolution). Depth Pro: must be 0 (the model resizes). */
  int restore;   /* 1: the display map is brought back to the frame's w x h (example/inference.rs:82-93) */
  int normalize; /* 1: per-frame min-max over the finite values (depth_to_u8); 0: raw depth (RGBA only) */
  int format;    /* MD_FRAME_U8_GRAY | MD_FRAME_RGBA_F32 */
} md_frame_opts;

typedef struct md_frame_outputs {
  void* display;          /* u8 [B,oh,ow] or f32 [B,oh,ow,4]; NULL = skip */
  float* depth;           /* model-resolution depth [B,th,tw]; NULL = skip */
  float* depth_range;     /* [B,2] lo, hi of the normalisation (0, 1 for a frame without a finite value); NULL = skip */
  uint8_t* prepared;      /* [B,th,tw,3] the resized / cropped frame the model saw; NULL = skip */
  float* focallength_px;  /* Depth Pro only, [B]; NULL = skip */
  float* fovy_rad;        /* Depth Pro only, [B]; NULL = skip */
} md_frame_outputs;

/* Sizes of a frame call: th x tw = the model input (and `depth`), oh x ow = the display map. */
int md_frame_geometry(md_model_t m, int w, int h, const md_frame_opts* o, int* th, int* tw, int* oh, int* ow);
/* B >= 1 frames of one size w x h, packed u8 RGB [B,h,w,3] in memory kind in_kind; every output in out_kind. With
 * md_model_enable_graph(m, 1), a device frame with device outputs replays one captured graph per (stream, B, w, h, opts,
 * output pointers). No host synchronisation inside the call except for host frames (pinned staging) and host outputs.
 * Errors: rgb / o / out NULL -> MD_ERR_INVALID_ARG; w, h <= 0 or B outside 1..max_batch -> MD_ERR_SHAPE; a target the
 * Depth-Anything-v3 model rejects -> MD_ERR_SHAPE; Depth Pro with target != 0, an unknown format or U8 without normalize
 * -> MD_ERR_INVALID_ARG. */
int md_process_frame(md_model_t m, const uint8_t* rgb, int B, int w, int h, int in_kind, const md_frame_opts* o,
                     const md_frame_outputs* out, int out_kind, void* stream);

/* ---- point path: depth and pinhole cameras to a point cloud on the device ----------------------------------------
 * Pixel (row v, column u) of view b with depth d, in f32, one rounded operation per step and no fused multiply-add
 * (pipeline.unproject_depth restates it in numpy bit for bit):
 *   rx = ((u + off) - cx) / fx,  ry = ((v + off) - cy) / fy,  p_c = (rx d, ry d, d)     fx = K[0][0], fy = K[1][1],
 *                                                                                       cx = K[0][2], cy = K[1][2]; skew ignored
 *   world = 1, E = [R | t] world-to-camera (camera.rs:248-254): q = p_c - t, p_w = R^T q, each coordinate
 *   (R0j qx + R1j qy) + R2j qz.
 * A pixel is valid when d is finite and depth_min <= d <= depth_max; a confidence map, when there is one, holds
 * conf >= conf_min; and, with edge_rtol > 0, |d - dn| <= edge_rtol * min(d, dn) for each of the 4 neighbours inside the
 * image whose depth dn is finite and > 0. */
typedef struct md_points_opts {
  float pixel_offset;         /* 0.0 = integer grid (goes with cx = W/2, cy = H/2) | 0.5 = pixel centres; any finite value */
  float depth_min, depth_max; /* 0 = the default of that bound: the smallest positive normal f32 / FLT_MAX (d <= 0 is never valid) */
  float conf_min;             /* used only when there is a confidence map */
  float edge_rtol;            /* 0 = off */
  int stride;                 /* >= 1: only pixels with u % stride == 0 and v % stride == 0 enter the compacted list */
  int world;                  /* 1: apply the inverse of `extrinsics` */
} md_points_opts;
typedef struct md_points_cameras {
  const float* intrinsics; /* [B,3,3] */
  const float* extrinsics; /* [B,3,4] world-to-camera; required when world = 1 (md_infer_points: unless the model predicts them) */
  const float* focal_px;   /* [B]; alternative to intrinsics: K = (f, f, W/2, H/2) */
} md_points_cameras;
typedef struct md_points_outputs {
  float* point_map;  /* dense f32 [B,H,W,3], (0,0,0) at invalid pixels; NULL = skip */
  uint8_t* mask;     /* dense u8 [B,H,W], 1 = valid; NULL = skip */
  float* xyz;        /* compacted f32 [capacity,3], order (b, v, u) ascending; needs count */
  uint8_t* rgb;      /* u8 [capacity,3] gathered from the rgb input; needs count */
  float* conf;       /* f32 [capacity] gathered from the confidence map; needs count */
  int32_t* count;    /* [B+1]: count[b] = points of view b, count[B] = their total (also when it exceeds capacity: then
                        only the first `capacity` points are written) */
  int64_t capacity;  /* points the compacted outputs hold */
  float* depth;      /* md_infer_points only: the depth that was unprojected, [B,H,W]; NULL = skip */
} md_points_outputs;

/* pixel_offset 0, depth bounds 0 (defaults), conf_min 0, edge_rtol 0, stride 1, world 0 */
void md_points_opts_default(md_points_opts* o);
/* The stand-alone operator on caller tensors: every pointer (cameras included) is a device pointer. conf_dev / rgb_dev may
 * be NULL. Errors, before any launch: o / out / cam NULL, stride < 1, capacity < 0, xyz / rgb / conf without count, an rgb
 * output without rgb_dev, a conf output without conf_dev, pixel_offset / edge_rtol / conf_min / a depth bound not finite or
 * negative (or depth_max < depth_min), world = 1 without extrinsics, neither intrinsics nor focal_px -> MD_ERR_INVALID_ARG;
 * B, H, W <= 0 or B*H*W >= 2^31 -> MD_ERR_SHAPE. */
int md_op_unproject(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                    const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, void* stream);
/* Model -> points in one call: the model's infer body, then the operator's kernels on its results, on the caller's stream.
 * nchw, rgb ([B,H,W,3] u8 or NULL) and the pointers of cam are of in_kind, every output of out_kind. cam NULL (or a NULL
 * field) = the model's own:
 *   Depth Pro: depth + the predicted focal length; cam->focal_px = the known-focal call (the FOV network does not run);
 *     no confidence; world = 1 needs cam->extrinsics.
 *   Depth-Anything-v3 dual head (`small`): depth, depth_confidence and the camera decoder's intrinsics / extrinsics.
 *   Depth-Anything-v3 mono head (`metric_large`): cam->intrinsics or cam->focal_px is required (MD_ERR_UNSUPPORTED
 *     without), no confidence (conf_min is ignored).
 * With md_model_enable_graph(m, 1), device inputs and outputs replay one captured graph per (stream, shape, options,
 * pointers). No host synchronisation inside the call except for host inputs / outputs. Errors as md_op_unproject's, plus
 * nchw NULL / an unknown memory kind -> MD_ERR_INVALID_ARG and B > max_batch -> MD_ERR_SHAPE. */
int md_infer_points(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                    const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, int out_kind,
                    void* stream);

/* ---- view filter: a confidence percentile and a cross-view consistency test in front of the point path ---------------
 * depth [B,H,W], an optional confidence map [B,H,W] and the cameras of the point path -> the same depth with rejected
 * pixels set to 0, which md_op_unproject never keeps (d <= 0). f32, one rounded operation per step, no fused multiply-add
 * (pipeline.filter_views restates it in numpy bit for bit):
 *   candidate: d finite and depth_min <= d <= depth_max (0 = the defaults of md_points_opts); with a confidence map also
 *     conf finite and >= 0.
 *   percentile q = conf_percentile in 0..99, 0 = off (tau = 0): N = the candidates over all B views of the call,
 *     k = ((int64)(N - 1) * q) / 100, tau = the k-th smallest candidate confidence counting from 0 (N = 0: tau = 0; -0
 *     counts as +0). The selection is exact. A survivor is a candidate with conf >= tau; without a confidence map every
 *     candidate survives and q must be 0.
 *   cross-view support, view_rtol > 0: for a survivor (i, v, u) with depth d, X_w = the point md_op_unproject writes for it
 *     with world = 1. For every other view j, ascending: p = R_j X_w + t_j, each coordinate ((Rk0 x + Rk1 y) + Rk2 z) + tk;
 *     the view sees the point when p.z > 0 and, with uf = ((fx_j (p.x / p.z)) + cx_j) - off, uu = floorf(uf + 0.5f) (vf, vv
 *     likewise), 0 <= uu < W and 0 <= vv < H compared in float; it supports the pixel when pixel (vv, uu) of view j is a
 *     survivor with depth d_j and |p.z - d_j| <= view_rtol * min(p.z, d_j). support = the number of supporting views; the
 *     pixel is kept when support >= min_views. view_rtol = 0: no test, support = 0, every survivor is kept. */
typedef struct md_view_filter_opts {
  float pixel_offset;         /* as md_points_opts */
  float depth_min, depth_max; /* as md_points_opts: 0 = the default of that bound */
  int conf_percentile;        /* q in 0..99: the lowest q % of the candidate confidences are dropped; 0 = off */
  float view_rtol;            /* > 0: the cross-view test (needs extrinsics, 2 <= B <= 64); 0 = off */
  int min_views;              /* 1 .. B-1 with view_rtol > 0; 0 with view_rtol = 0 */
} md_view_filter_opts;
typedef struct md_view_filter_outputs {
  float* depth;          /* f32 [B,H,W]: d where kept, else 0; must not be the input. NULL = skip */
  uint8_t* support;      /* u8 [B,H,W]: supporting views of a survivor, 0 elsewhere. NULL = skip */
  float* conf_threshold; /* f32 [1]: tau. NULL = skip */
  int32_t* kept;         /* int32 [B+1]: kept pixels per view, then their total. NULL = skip */
} md_view_filter_outputs;

/* everything 0: a pass-through of the candidates */
void md_view_filter_opts_default(md_view_filter_opts* o);
/* The stand-alone operator on caller tensors: every pointer (cameras included) is a device pointer; conf_dev may be NULL.
 * cam is needed only with view_rtol > 0 (intrinsics or focal_px, and extrinsics). Everything is enqueued on `stream`; the
 * call returns after the stream has drained, because its scratch is freed on return. Errors, before any launch: o / out
 * NULL, every output NULL, out->depth == depth_dev, conf_percentile outside 0..99 or > 0 without conf_dev, view_rtol not
 * finite or negative, min_views != 0 with view_rtol = 0, min_views < 1 or > B - 1 with view_rtol > 0, view_rtol > 0 without
 * extrinsics or without intrinsics / focal_px, pixel_offset or a depth bound not finite (a bound negative, or
 * depth_max < depth_min) -> MD_ERR_INVALID_ARG; B, H, W <= 0, B*H*W >= 2^31, B >= 65536, or with view_rtol > 0: B < 2,
 * B > 64, H or W >= 2^24 -> MD_ERR_SHAPE (the shape is checked before min_views against B). */
int md_op_filter_views(md_device_t dev, const float* depth_dev, const float* conf_dev, int B, int H, int W,
                       const md_points_cameras* cam, const md_view_filter_opts* o, const md_view_filter_outputs* out, void* stream);
/* md_infer_points with the filter between the model and the unprojection: the filter reads the model's depth and
 * confidence (dual head) and the cameras the unprojection uses (the model's own or the caller's); the filtered depth is
 * what is unprojected and what out->depth receives. `o` applies afterwards, unchanged (conf_min on top of tau).
 * fo->pixel_offset / depth_min / depth_max must equal o's. Graph replay, memory kinds and errors as md_infer_points',
 * plus md_op_filter_views' (conf_percentile > 0 on a model without a confidence map, view_rtol > 0 where neither the
 * model nor the caller has extrinsics -> MD_ERR_INVALID_ARG). After the first call of a shape nothing is allocated. */
int md_infer_points_filtered(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                             const md_points_cameras* cam, const md_view_filter_opts* fo, const md_points_opts* o,
                             const md_points_outputs* out, int out_kind, void* stream);

/* ---- point path: surface normals and a grazing-angle filter ------------------------------------------------------------
 * The normal of pixel c = (v, u) of view b with depth d_c, from its one ring of four neighbours. f32, one rounded operation
 * per step and no fused multiply-add (pipeline.unproject_depth(normals=True) restates it in numpy bit for bit):
 *   P(v, u) = the camera-space point p_c of the point path above (world = 0).
 *   A neighbour n out of E = (v, u+1), S = (v+1, u), W = (v, u-1), N = (v-1, u) is usable when it lies inside the image, its
 *     depth d_n is finite and depth_min <= d_n <= depth_max (the bounds resolved as md_points_opts resolves them), a
 *     confidence map, when there is one, holds conf_n >= conf_min, and, with edge_rtol > 0,
 *     |d_c - d_n| <= edge_rtol * min(d_c, d_n). Only this ring is read: the neighbour's own edge test does not enter.
 *   e_n = P_n - P_c per component. For the pairs (a, b) = (S,E), (E,N), (N,W), (W,S), in this order, whose two neighbours
 *     are usable: a x b = ((ay bz) - (az by), (az bx) - (ax bz), (ax by) - (ay bx)); m = their sum from left to right,
 *     starting from the first usable pair. With x right, y down, z forward every such cross points at the camera.
 *   len2 = (mx mx + my my) + mz mz. The normal is defined when a pair was usable and len2 is finite and >= FLT_MIN:
 *     n = (mx / s, my / s, mz / s), s = sqrtf(len2); otherwise n = (0, 0, 0).
 *   world = 1: n_w = R^T n, each coordinate (R0j nx + R1j ny) + R2j nz, not renormalised.
 *   cosv = -((nx px + ny py) + nz pz) / sqrtf((px px + py py) + pz pz), n and p = P_c in camera space. With min_cos > 0 a
 *     pixel is valid only when every condition of the point path holds, its normal is defined and cosv >= min_cos; this
 *     validity feeds the mask, the point map, the list and count as the other conditions do.
 *   stride thins the list only: the neighbours are always the adjacent pixels. f32 denormals are outside the contract. */
typedef struct md_points_normals {
  float* normal_map; /* dense f32 [B,H,W,3]: the normal at valid pixels with a defined normal, (0,0,0) elsewhere; NULL = skip */
  float* normals;    /* compacted f32 [capacity,3], rows parallel to xyz; needs count */
  float min_cos;     /* 0 = off, else in (0, 1] */
} md_points_normals;

/* md_op_unproject with normals. nrm NULL or all zero: md_op_unproject on the same arguments, the same launches and bits.
 * Errors as md_op_unproject's, plus, before any launch: min_cos not finite, negative or above 1, normals without count
 * -> MD_ERR_INVALID_ARG. */
int md_op_unproject_normals(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H,
                            int W, const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out,
                            const md_points_normals* nrm, void* stream);
/* md_infer_points (fo NULL) / md_infer_points_filtered (fo given) with normals; nrm's pointers are of out_kind. nrm NULL or
 * all zero: those calls on the same arguments. The graph key contains nrm's three fields. Errors as theirs, plus
 * md_op_unproject_normals'. After the first call of a shape nothing is allocated. */
int md_infer_points_normals(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                            const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                            const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm, int out_kind,
                            void* stream);

/* ---- point path: voxel thinning of a point list ------------------------------------------------------------------------
 * A list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3] -> one input row per
 * occupied voxel of side `voxel` > 0. Selection, not averaging: the output is a subset of the input rows, and nothing in
 * it depends on the order in which threads arrive. f32, one rounded operation per step, no fused multiply-add
 * (pipeline.voxel_thin restates it in numpy bit for bit):
 *   cell: c_a = floorf(p_a / voxel) for a = x, y, z. Point i is in range when its three coordinates are finite and
 *     -2^20 <= c_a < 2^20 on every axis (compared in float). key = ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) |
 *     (c_z + 2^20), an unsigned 64-bit integer; the all-ones word never occurs and marks an empty table slot. Points out of
 *     range are dropped and counted (`dropped`).
 *   rank: w = conf_i when there is a confidence row and conf_i is finite and >= 0 (-0 counts as +0), otherwise w = 0. The
 *     survivor of a voxel is its in-range point with the largest w; among equals the smallest input index wins. On the
 *     device this is one atomicMax of the word (bits(w) << 32) | (0xFFFFFFFF - i): the bit pattern of a non-negative finite
 *     f32 is monotone in its value.
 *   weight = the number of in-range points of the survivor's voxel (an integer atomicAdd).
 *   output: the survivors in ascending input index, so the (view, row, column) order of the point path is kept; every given
 *     row is copied unchanged; index = the source row, weight as above. count[b] = the survivors of view b, count[B] = their
 *     total M, also when M exceeds `capacity`: then only the first `capacity` rows are written and the memory behind them
 *     stays untouched. All views of a call are one scene: they share the voxel grid.
 *   f32 denormals are outside the contract.
 * The table is open addressing with linear probing over a power of two >= 2 N slots of 20 bytes in device memory, reset on
 * the stream inside every call; the hash is a fixed 64-bit mixer and cannot influence the result. */
typedef struct md_points_voxel {
  float voxel;      /* voxel side; 0 = no thinning (md_infer_points_voxel), finite and >= 0 */
  int32_t* index;   /* int32 [capacity]: the source row of every output row; needs count. NULL = skip */
  int32_t* weight;  /* int32 [capacity]: in-range points in the output row's voxel; needs count. NULL = skip */
  int32_t* dropped; /* int32 [1]: rows not finite or out of range. NULL = skip */
} md_points_voxel;

/* The stand-alone operator on caller device lists: the N rows are one view. Of `out` the fields xyz, rgb, conf, count
 * (int32 [2]: M twice, the point path's [B+1] with B = 1) and capacity are used, the others must be NULL; normals_out
 * [capacity,3] takes the normals rows. Everything is enqueued on `stream`; the call returns after the stream has drained,
 * because its table is freed on return. Errors, before any launch: dev / vox / out NULL, xyz_dev NULL with N > 0, voxel not
 * finite or <= 0, N < 0, capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index, weight) without count, an
 * rgb / conf / normals output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG;
 * N >= 2^30 -> MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP after the launches. */
int md_op_voxel_thin(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                     int64_t N, const md_points_voxel* vox, const md_points_outputs* out, float* normals_out, void* stream);
/* md_infer_points_normals with the thinning behind the scatter: the unthinned list (at most B ceil(H/stride) ceil(W/stride)
 * rows) goes to a grow-only buffer of the model, as does the table; the thinned list goes to out->xyz / rgb / conf and
 * nrm->normals, and out->count receives the thinned counts. The confidence row is the model's confidence map where it has
 * one (dual head), whether or not out->conf is set. The dense outputs are those of the call without thinning. vox's
 * pointers are of out_kind. vox NULL or voxel == 0 (index, weight and dropped then NULL): md_infer_points_normals on the
 * same arguments, the same launches and bits; a call without out->count thins nothing. The graph key contains vox's four
 * fields. Errors as md_infer_points_normals', plus, before any launch: voxel not finite or negative, index / weight without
 * count, index / weight / dropped with voxel == 0 -> MD_ERR_INVALID_ARG; B ceil(H/stride) ceil(W/stride) >= 2^30 ->
 * MD_ERR_SHAPE. With host outputs a probe loop that ran out of table -> MD_ERR_HIP; with device outputs the call does not
 * wait for the device and md_model_query(m, "voxel_overflow") reads the flag of the last call (it waits for the
 * device). After the first call of a shape nothing is allocated. */
int md_infer_points_voxel(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                          const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                          const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                          const md_points_voxel* vox, int out_kind, void* stream);

/* ---- point path: render a point list into target cameras -------------------------------------------------------------------
 * The inverse direction: a list xyz f32 [N,3] with an optional parallel row rgb u8 [N,3] -> for each of T target cameras
 * (md_points_cameras with T in place of B: intrinsics [T,3,3] or focal_px [T], K = (f, f, W/2, H/2); extrinsics [T,3,4]
 * world-to-camera, NULL = the points are already in the camera's frame) a z-buffered H x W image. Selection, not blending: a
 * pixel shows one input row, and nothing depends on the order in which threads arrive. f32, one rounded operation per step,
 * no fused multiply-add (pipeline.render_points restates it in numpy bit for bit):
 *   rows: n = min(max(*count, 0), N) with a device count word (int32), n = N without: the list md_op_unproject or
 *     md_op_voxel_thin wrote is rendered without a host read. Point i < n is skipped when a coordinate is not finite.
 *   projection into target j, the view filter's: p = R_j X + t_j, each coordinate ((Rk0 x + Rk1 y) + Rk2 z) + tk (extrinsics
 *     NULL: p = X). The target sees the point when p.z is finite and z_near <= p.z <= z_far (0 = the default of that bound,
 *     resolved as md_points_opts resolves depth_min / depth_max, so p.z > 0) and, with uf = ((fx (p.x / p.z)) + cx) - off,
 *     uu = floorf(uf + 0.5f) (vf, vv likewise), 0 <= uu < W and 0 <= vv < H compared in float before any conversion: a NaN
 *     or an infinity from the division is never in the image.
 *   footprint: the (2 radius + 1)^2 pixel square around (vv, uu), clipped to the image. For each of its pixels the candidate
 *     key is ((uint64)bits(p.z) << 32) | (uint32)i, and the pixel keeps the minimum key: the nearest p.z (for p.z > 0 the bit
 *     order is the value order), among equal p.z the smallest row. An empty pixel's key is all ones, which no candidate equals.
 *   outputs: depth = the winner's p.z, 0 at holes; index = the winner's row, -1 at holes; rgb = the winner's rgb row, 0 at
 *     holes; filled[j] = the pixels of target j that are no holes, filled[T] = their total (integer adds).
 * The keys take 8 bytes per pixel of device memory; they are cleared on the stream inside every call. */
typedef struct md_render_opts {
  float pixel_offset;  /* as md_points_opts */
  float z_near, z_far; /* bounds of p.z; 0 = the default of that bound (smallest positive normal f32 / FLT_MAX) */
  int radius;          /* 0..16: the footprint is the (2 radius + 1)^2 pixel square around the hit pixel */
} md_render_opts;
typedef struct md_render_outputs {
  float* depth;    /* f32 [T,H,W]; NULL = skip */
  int32_t* index;  /* int32 [T,H,W]; NULL = skip */
  uint8_t* rgb;    /* u8 [T,H,W,3]; needs the rgb row. NULL = skip */
  int32_t* filled; /* int32 [T+1]; NULL = skip */
} md_render_outputs;
typedef struct md_points_render { /* the rendering part of md_infer_points_render */
  int T, H, W;                    /* target cameras and their image size */
  md_points_cameras cam;          /* [T, ..] pointers of in_kind */
  md_render_opts opts;
  md_render_outputs out;          /* pointers of out_kind; rgb needs the list output out->rgb */
} md_points_render;

/* everything 0: integer grid, default bounds, one pixel per point */
void md_render_opts_default(md_render_opts* o);
/* The stand-alone operator on caller device tensors (cameras included); rgb_dev and count_dev may be NULL. Everything is
 * enqueued on `stream`; the call returns after the stream has drained, because its key buffer is freed on return. N = 0 is
 * legal: every pixel is a hole. Errors, before any launch: dev / opts / out / cam NULL, every output NULL, an rgb output
 * without rgb_dev, xyz_dev NULL with N > 0, neither intrinsics nor focal_px, radius < 0 or > 16, pixel_offset or a bound not
 * finite, a bound negative, z_far < z_near (both given) -> MD_ERR_INVALID_ARG; N < 0, N >= 2^31, T, H, W <= 0,
 * T*H*W >= 2^31, H or W >= 2^24 -> MD_ERR_SHAPE. */
int md_op_render_points(md_device_t dev, const float* xyz_dev, const uint8_t* rgb_dev, int64_t N, const int32_t* count_dev, int T,
                        int H, int W, const md_points_cameras* cam, const md_render_opts* opts, const md_render_outputs* out,
                        void* stream);
/* md_infer_points_voxel with the rendering behind it: the list the call ends with (thinned or not; its first
 * min(count[B], capacity) rows, read from the device count) is rendered into rnd's targets in the same call and graph. The
 * keys and, for host cameras, their device copies live in grow-only buffers of the model. rnd NULL: md_infer_points_voxel on
 * the same arguments, the same launches and bits. The graph key contains rnd's fields. Errors as md_infer_points_voxel's and
 * md_op_render_points', plus: rnd without the list outputs out->xyz and out->count, rnd->out.rgb without out->rgb ->
 * MD_ERR_INVALID_ARG. After the first call of a shape nothing is allocated. */
int md_infer_points_render(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                           const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                           const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, int out_kind, void* stream);

/* ---- point path: triangle mesh of the depth grid ---------------------------------------------------------------------------
 * A surface over the list: neighbouring lattice pixels are joined into triangles, which are cut at depth discontinuities. The
 * vertices are the rows of the compacted list, a face is three of them. Selection with integer outputs: a face is emitted or
 * not from f32 comparisons, one rounded operation per step, no fused multiply-add, no atomics (pipeline.pixel_index and
 * pipeline.mesh_grid restate it in numpy bit for bit):
 *   lattice: with stride = md_points_opts.stride, node (i, j) is pixel (v, u) = (i stride, j stride), 0 <= i < Hs =
 *     ceil(H / stride), 0 <= j < Ws = ceil(W / stride). Quad (b, i, j) exists for i < Hs - 1, j < Ws - 1; its corners are
 *     a = (i, j), b = (i, j+1), c = (i+1, j), d = (i+1, j+1).
 *   pixel_index int32 [B,H,W]: the row of a pixel in the compacted list as xyz orders it: its true rank, global over the
 *     views, also beyond `capacity`; -1 where the pixel did not enter the list.
 *   usable corner: its index is >= 0 and below the vertex limit: `capacity` of the list in the combined calls, vertex_limit in
 *     md_op_mesh_grid (0 = no limit).
 *   edge (x, y) between usable corners with depths dx, dy: max_rtol == 0: it passes; otherwise it passes when
 *     fabsf(dx - dy) <= max_rtol * fminf(dx, dy) (subtract, abs, min, multiply, compare).
 *   diagonal: all four corners usable: a-d when fabsf(da - dd) <= fabsf(db - dc), otherwise b-c; a or d unusable: b-c;
 *     otherwise a-d.
 *   triangles, in this order inside a quad: diagonal a-d: (a, c, d), (a, d, b); diagonal b-c: (a, c, b), (b, c, d). A triangle
 *     is emitted when its three corners are usable and its three edges pass. All four windings face the camera: with x right,
 *     y down, z forward, (p1 - p0) x (p2 - p0) has negative z in the image plane, the orientation of md_points_normals.
 *   faces int32 [face_capacity,3]: list rows, ordered by (b, i, j, triangle). face_count int32 [B+1]: the true totals per view
 *     and overall, also when they exceed face_capacity: then only the first face_capacity faces are written and the memory
 *     behind them stays untouched, as count / capacity behave. */
typedef struct md_points_mesh {
  float max_rtol;          /* 0 = no discontinuity cut; finite and >= 0 */
  int32_t* faces;          /* int32 [face_capacity,3]; needs face_count. NULL = skip */
  int32_t* face_count;     /* int32 [B+1]; NULL = skip */
  int64_t face_capacity;   /* faces that `faces` holds */
  int32_t* pixel_index;    /* int32 [B,H,W]; NULL = skip */
} md_points_mesh;

/* The face kernels alone on caller device tensors: depth_dev f32 [B,H,W], pixel_index_dev int32 [B,H,W] (any map: it need
 * not come from a list). mesh->pixel_index is ignored. Everything is enqueued on `stream`; the call returns after the stream
 * has drained, because its scratch is freed on return. A lattice without quads (Hs or Ws = 1): face_count all zero, faces
 * untouched. Errors, before any launch: dev / mesh / depth_dev / pixel_index_dev NULL, stride < 1, vertex_limit < 0, max_rtol
 * not finite or negative, face_capacity < 0, faces without face_count -> MD_ERR_INVALID_ARG; B, H, W <= 0 or
 * B*H*W >= 2^30 (two faces per quad must fit int32) -> MD_ERR_SHAPE. */
int md_op_mesh_grid(md_device_t dev, const float* depth_dev, const int32_t* pixel_index_dev, int B, int H, int W, int stride,
                    int64_t vertex_limit, const md_points_mesh* mesh, void* stream);
/* md_op_unproject_normals with the mesh of its list: one launch writes pixel_index (into a scratch of the call when the
 * caller takes none and asks for faces), three write the faces. The depths of the edge test are depth_dev's. mesh NULL (or
 * its three outputs NULL): md_op_unproject_normals on the same arguments, the same launches and bits. The call returns after
 * the stream has drained. Errors as md_op_unproject_normals' and md_op_mesh_grid's, plus: a mesh output without out->count
 * -> MD_ERR_INVALID_ARG; B*H*W >= 2^30 with a mesh output -> MD_ERR_SHAPE. */
int md_op_unproject_mesh(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                         const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out,
                         const md_points_normals* nrm, const md_points_mesh* mesh, void* stream);
/* md_infer_points_render with the mesh of the list: the mesh stage runs directly behind the unprojection, on the depth that
 * was unprojected (out->depth). mesh's pointers are of out_kind; with host outputs only the first
 * min(face_count[B], face_capacity) rows of faces travel. The face scratch and a pixel_index the caller does not take live in
 * a grow-only buffer of the model. mesh NULL (or its three outputs NULL): md_infer_points_render on the same arguments, the
 * same launches and bits. The graph key contains mesh's fields. Errors as md_infer_points_render's and md_op_unproject_mesh's,
 * plus: a mesh output together with voxel thinning (the rows the faces name no longer exist) -> MD_ERR_INVALID_ARG. After the
 * first call of a shape nothing is allocated. */
int md_infer_points_mesh(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                         const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                         const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                         const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, int out_kind,
                         void* stream);

/* ---- point path: rasterise the mesh into target cameras ---------------------------------------------------------------------
 * A render without holes: the faces md_op_mesh_grid / md_infer_points_mesh wrote over the list are drawn into T target cameras
 * (md_points_cameras with T in place of B, as md_op_render_points takes them; extrinsics NULL = the points are already in the
 * camera's frame). Inputs: xyz f32 [N,3], faces int32 [F,3] (rows of xyz), optionally rgb u8 [N,3] and a device face-count
 * word: the live faces are n = min(max(*count, 0), F), which is face_count[B] of the mesh stage read without a host round
 * trip. Selection, not blending: a pixel shows one face, chosen by the minimum of a 64-bit key, so nothing depends on the order
 * in which threads arrive. Per face f < n and target j (pipeline.render_mesh restates every step bit for bit):
 *   1 indices: the face is skipped when a vertex row lies outside 0..N-1 (tested on the device: a bad index never becomes a
 *     read) or a vertex coordinate is not finite.
 *   2 projection, md_op_render_points' step for step, for each vertex: p = ((Rk0 x + Rk1 y) + Rk2 z) + tk (extrinsics NULL:
 *     p = X); the vertex is visible when p.z is finite and z_near <= p.z <= z_far (0 = the default of that bound, resolved as
 *     md_render_opts does); uf = ((fx (p.x / p.z)) + cx) - off, vf likewise. All three vertices must be visible: there is no
 *     near-plane clipping, a triangle that crosses a bound is dropped.
 *   3 snap to 1/256 pixel: sx = floorf(uf * 256.f + 0.5f), sy likewise; the face is skipped unless fabsf(sx) < 16777216.f and
 *     fabsf(sy) < 16777216.f for all three vertices, compared in float before any conversion (a NaN or an infinity fails);
 *     then X = (int64)sx, Y = (int64)sy. From here coverage is integer arithmetic.
 *   4 area: A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) in int64. A == 0: skipped. cull = 1: a face with A > 0 is skipped (with x
 *     right and y down the faces md_op_mesh_grid emits have A < 0 in their own camera). For A < 0 the three weights of step 6
 *     and A are negated.
 *   5 bounding box in ints, clipped to the image: u0 = max(0, (min X + 255) >> 8), u1 = min(W-1, max X >> 8) (arithmetic
 *     shifts), v0, v1 likewise. An empty box: skipped. A box wider or taller than max_extent pixels: skipped and counted in
 *     skipped[j] and skipped[T]. The cap is part of the contract: it bounds the work one face can cause, and it drops the
 *     rubber sheets a stretched depth edge makes.
 *   6 coverage of pixel (u, v) of the box, P = (256 u, 256 v): w0 = edge(V1,V2,P), w1 = edge(V2,V0,P), w2 = edge(V0,V1,P) with
 *     edge(a,b,P) = (bx-ax)(Py-ay) - (by-ay)(Px-ax); covered when all three are >= 0. The test is inclusive on every edge: two
 *     faces that share an edge compute the same integers with opposite signs, so no pixel falls between them; a pixel on the
 *     edge belongs to both and the key decides.
 *   7 depth: b_i = (float)((double)w_i / (double)A) (the ints are below 2^51, so exact in f64: one f64 division, one rounding
 *     to f32); iz = (b0 * (1.f/z0) + b1 * (1.f/z1)) + b2 * (1.f/z2) with z_i = p.z of vertex i; z = 1.f / iz. The candidate
 *     is dropped unless z is finite and z_near <= z <= z_far, which makes the bit order of z its value order.
 *   8 key: ((uint64)bits(z) << 32) | (uint32)f; the pixel keeps the minimum: the nearest face, among equal z the smallest
 *     face. All ones marks an empty pixel.
 * Outputs: depth = the winner's z, 0 at holes; face = the winner, -1 at holes; rgb channel = fminf(floorf(((b0 c0 + b1 c1)
 * + b2 c2) + 0.5f), 255.f) with the b's of the winning face recomputed at that pixel and c_i the channel of vertex i as f32,
 * 0 at holes: the colour is affine in screen space, not perspective-correct; filled[j] = the pixels of target j that are no
 * holes, filled[T] their total; skipped[j] = the faces step 5 dropped for their extent, skipped[T] their total.
 * Device memory: 8 bytes per pixel of keys and a fixed queue of (face, target) pairs for the faces with larger boxes; a full
 * queue changes the schedule, never the image. */
typedef struct md_raster_opts {
  float pixel_offset;  /* as md_points_opts */
  float z_near, z_far; /* bounds of p.z and of the interpolated z; 0 = the default of that bound, as md_render_opts */
  int cull;            /* 0: both sides are drawn; 1: only the winding md_op_mesh_grid emits (A < 0) */
  int max_extent;      /* 0 = 64; 1..1024: a face whose clipped box is wider or taller is skipped and counted */
} md_raster_opts;
typedef struct md_raster_outputs {
  float* depth;     /* f32 [T,H,W]; NULL = skip */
  int32_t* face;    /* int32 [T,H,W]; NULL = skip */
  uint8_t* rgb;     /* u8 [T,H,W,3]; needs the rgb row. NULL = skip */
  int32_t* filled;  /* int32 [T+1]; NULL = skip */
  int32_t* skipped; /* int32 [T+1]; NULL = skip */
} md_raster_outputs;
typedef struct md_points_raster { /* the rasterising part of md_infer_points_raster */
  int T, H, W;                    /* target cameras and their image size */
  md_points_cameras cam;          /* [T, ..] pointers of in_kind */
  md_raster_opts opts;
  md_raster_outputs out;          /* pointers of out_kind; rgb needs the list output out->rgb */
} md_points_raster;

/* everything 0: integer grid, default bounds, both sides, max_extent 64 */
void md_raster_opts_default(md_raster_opts* o);
/* The stand-alone operator on caller device tensors (cameras included); rgb_dev and face_count_dev may be NULL. Everything is
 * enqueued on `stream`; the call returns after the stream has drained, because its scratch is freed on return. F = 0 is
 * legal: every pixel is a hole. Errors, before any launch (the outputs stay untouched): dev / opts / out / cam NULL, every
 * output NULL, an rgb output without rgb_dev, xyz_dev NULL with N > 0, faces_dev NULL with F > 0, neither intrinsics nor
 * focal_px, cull not 0 or 1, max_extent < 0 or > 1024, pixel_offset or a bound not finite, a bound negative, z_far < z_near
 * (both given) -> MD_ERR_INVALID_ARG; N or F < 0 or >= 2^31, T, H, W <= 0, T*H*W >= 2^31, H or W >= 2^24 -> MD_ERR_SHAPE. */
int md_op_render_mesh(md_device_t dev, const float* xyz_dev, const uint8_t* rgb_dev, int64_t N, const int32_t* faces_dev, int64_t F,
                      const int32_t* face_count_dev, int T, int H, int W, const md_points_cameras* cam, const md_raster_opts* opts,
                      const md_raster_outputs* out, void* stream);
/* md_infer_points_mesh with the rasterising behind the rendering: the faces of the mesh stage (their first
 * min(face_count[B], face_capacity), read from the device count) over the list's xyz / rgb are drawn into rst's targets in the
 * same call and graph. The keys, the queue and, for host cameras, their device copies live in grow-only buffers of the model.
 * rst NULL: md_infer_points_mesh on the same arguments, the same launches and bits. The graph key contains rst's fields.
 * Errors as md_infer_points_mesh's and md_op_render_mesh's, plus: rst without the list outputs out->xyz and out->count or
 * without mesh->faces and mesh->face_count, rst->out.rgb without out->rgb -> MD_ERR_INVALID_ARG (voxel thinning already
 * excludes the mesh). After the first call of a shape nothing is allocated. */
int md_infer_points_raster(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                           const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                           const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                           const md_points_raster* rst, int out_kind, void* stream);
/* The largest clipped box, in pixels, that the setup kernel draws in the face's own thread; a larger one goes through the
 * queue (a compile-time constant of kernels/raster.hip). The image does not depend on it. */
int md_raster_inline_pixels(void);

/* ---- point path: radius outlier removal of a point list -------------------------------------------------------------------
 * A list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3] -> the rows that have at
 * least k = min_neighbours other rows within `radius` > 0 (1 <= k <= 2^20). Selection: a row survives or it does not, and the
 * decision is an integer count of a deterministic f32 predicate, so nothing depends on the order in which threads arrive.
 * f32, one rounded operation per step, no fused multiply-add (pipeline.radius_outliers restates it in numpy bit for bit):
 *   cell: c_a = floorf(p_a / radius). In range, key and the empty mark are voxel thinning's with `radius` as the side: the
 *     coordinates finite, -2^20 <= c_a < 2^20 on every axis (compared in float), key = ((c_x + 2^20) << 42) |
 *     ((c_y + 2^20) << 21) | (c_z + 2^20), all ones = an empty slot. Rows out of range are dropped and counted (`dropped`).
 *   neighbour: in-range row j != i is a neighbour of in-range row i when |c_a(j) - c_a(i)| <= 1 on all three axes AND
 *     d2 <= r2, with dx = p_j.x - p_i.x (dy, dz likewise), d2 = (dx*dx + dy*dy) + dz*dz and r2 = radius*radius. The test is
 *     inclusive; rows with equal coordinates are neighbours of each other; a row is never its own neighbour. The predicate
 *     is symmetric (f32 subtraction is antisymmetric).
 *   The cell condition is part of the definition, not an optimisation. In exact arithmetic d <= radius implies it; in f32 the
 *     quotient p_a / radius and the difference p_j.a - p_i.a are rounded, and a pair within rounding of the radius along one
 *     axis can pass d2 <= r2 and yet sit two cells apart: p_i.x = -1e-30 lies in cell -1, p_j.x = radius in cell 1, and dx
 *     rounds to the radius. Such a pair is NOT a neighbour pair here. This is the only deviation from the pure radius test:
 *     it needs |p_j.a - p_i.a| within an ulp of `radius` on one axis, so the other two differences are about 0. Making the
 *     27-cell search the definition keeps the device and the host identical.
 *   neighbours[i] = min(n_i, k) with n_i the number of neighbours of row i: the count saturates at k (a search may stop at
 *     the k-th hit). Rows out of range get -1. int32 over the INPUT rows [N].
 *   survivors: neighbours[i] == k. Output: the survivors in ascending input index, so the (view, row, column) order is kept;
 *     every given row is copied unchanged; index = the source row. count[b] = the survivors of view b, count[B] = their total
 *     M, also when M exceeds `capacity`: then only the first `capacity` rows are written and the memory behind them stays
 *     untouched. All views of a call share the grid.
 *   f32 denormals are outside the contract.
 * The grid is voxel thinning's table (linear probing over the power of two >= max(2 N, 1024) slots) extended to cell buckets:
 * per slot a count and a start, and the in-range positions stored bucket by bucket in 12 N bytes. The order of the buckets and
 * of the rows inside one varies from run to run; it is layout and reaches no output. Reset on the stream inside every call. */
typedef struct md_points_outlier {
  float radius;        /* 0 = no outlier removal (md_infer_points_outlier), finite and >= 0 */
  int min_neighbours;  /* k, 1 .. 2^20 */
  int32_t* neighbours; /* int32 [N] over the rows of the unfiltered list: min(n_i, k), -1 out of range. NULL = skip */
  int32_t* index;      /* int32 [capacity]: the source row of every output row; needs count. NULL = skip */
  int32_t* dropped;    /* int32 [1]: rows not finite or out of range. NULL = skip */
} md_points_outlier;

/* The stand-alone operator on caller device lists, modelled on md_op_voxel_thin: the N rows are one view. Of `out` the fields
 * xyz, rgb, conf, count (int32 [2]: M twice) and capacity are used, the others must be NULL; normals_out [capacity,3] takes
 * the normals rows. Everything is enqueued on `stream`; the call returns after the stream has drained, because its scratch is
 * freed on return. Errors, before any launch: dev / outl / out NULL, xyz_dev NULL with N > 0, radius not finite or <= 0,
 * min_neighbours < 1 or > 2^20, N < 0, capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index) without count,
 * an rgb / conf / normals output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG;
 * N >= 2^30 -> MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP after the launches. */
int md_op_radius_outliers(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev,
                          const float* normals_dev, int64_t N, const md_points_outlier* outl, const md_points_outputs* out,
                          float* normals_out, void* stream);
/* md_infer_points_raster with the outlier removal between the unprojection and the thinning: the unfiltered list goes to a
 * grow-only buffer of the model, as do the table, the buckets and the ballot words; thinning and the point render see the
 * filtered list (with thinning the filter writes a second grow-only list and the thinning writes the caller's). out->count
 * receives the counts of the list the call ends with. outl->neighbours is int32 over the rows of the unfiltered list (at most
 * B ceil(H/stride) ceil(W/stride); the first unfiltered-total rows are written); outl->index names rows of the unfiltered
 * list and is written only without thinning (with it, vox->index names rows of the filtered list). outl's pointers are of
 * out_kind. outl NULL or radius == 0 (its pointers then NULL): md_infer_points_raster on the same arguments, the same
 * launches and bits; a call without out->count filters nothing. The graph key contains outl's fields. Errors as
 * md_infer_points_raster's, plus, before any launch: radius not finite or negative, min_neighbours < 1 or > 2^20 with
 * radius > 0, neighbours / index without count, any of outl's pointers with radius == 0, outlier removal together with a
 * mesh (the rows its faces name no longer exist) -> MD_ERR_INVALID_ARG; a list of >= 2^30 rows -> MD_ERR_SHAPE. With host
 * outputs a probe loop that ran out of table -> MD_ERR_HIP; with device outputs md_model_query(m, "outlier_overflow") reads
 * the flag of the last call (it waits for the device). After the first call of a shape nothing is allocated. */
int md_infer_points_outlier(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                            const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                            const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                            const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                            const md_points_raster* rst, const md_points_outlier* outl, int out_kind, void* stream);

/* ---- point path: vertex-clustering decimation of a mesh ---------------------------------------------------------------------
 * A vertex list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3], and faces int32
 * [F,3] over its rows -> one vertex per occupied voxel of side `voxel` > 0 and the faces re-indexed to those vertices.
 * Selection only: a vertex is an input row, a face is an input face with new indices; nothing is averaged, no float is summed
 * and nothing depends on the order in which threads arrive (pipeline.decimate_mesh restates it in numpy bit for bit).
 *   vertices: exactly voxel thinning's. Cell, range test, key and rank w are md_points_voxel's; the survivor of a voxel is its
 *     in-range row with the largest w, among equals the smallest index; the survivors come in ascending input index; index,
 *     weight, count [B+1], dropped and capacity behave as there, so every vertex output is bitwise md_op_voxel_thin's on the
 *     same rows. A vertex that no face names stays in the list.
 *   remap int32 [N]: remap[i] = the output row of the survivor of row i's voxel, -1 for a row out of range. It is the true
 *     rank, also when it is >= capacity (that row was not written).
 *   faces: face f with the corners (p, q, r) maps to (remap[p], remap[q], remap[r]) and falls into exactly one class, tested
 *     in this order:
 *       1 invalid     a corner is < 0 or >= N, or its remap is -1, or its remap is >= capacity: no kept face names a row that
 *                     was not written;
 *       2 degenerate  two of the mapped corners are equal;
 *       3 duplicate   some face g < f that is neither invalid nor degenerate has the same ORIENTED triangle: its mapped triple
 *                     equals f's after each is rotated so that its smallest index comes first. The three cyclic rotations
 *                     of a triple are one face. The reversed triple is a DIFFERENT face and is kept: it is the other side of
 *                     a fold, and the winding of a face carries meaning for the rasteriser's culling and for normals;
 *       4 kept        otherwise.
 *     The kept faces come in ascending f, each written as its mapped triple in the rotation the input had, so the winding is
 *     unchanged. face_index = the source face. face_count[b] = the kept faces whose source face belongs to view b (the views
 *     of the faces are the prefix of the INPUT face counts; the stand-alone operator has one view), face_count[B] = their
 *     total, also beyond face_capacity: then only the first face_capacity rows are written and the memory behind them stays
 *     untouched. faces_dropped [3] = the sizes of classes 1, 2, 3.
 *   limits: N < 2^30 and F < 2^30.
 * The duplicate test is a hash set over oriented triangles in device memory: the power of two >= max(2 F, 1024) int32 slots
 * that hold a face id (-1 = empty), linear probing, a fixed 64-bit mixer over the rotated triple. The identity of a slot is the
 * triple of whichever id it holds, all ids that ever sit in one slot have the same triple, and the slot ends as the smallest of
 * them (atomicMin), so the hash and the order of arrival decide where a triangle lives and never which face is kept. Table and
 * counters are reset on the stream inside every call. */
typedef struct md_points_decimate {
  float voxel;            /* voxel side, finite and > 0; 0 = no decimation (md_infer_points_decimate) */
  int32_t* index;         /* int32 [capacity]: the source row of every vertex; needs count. NULL = skip */
  int32_t* weight;        /* int32 [capacity]: in-range rows of the vertex's voxel; needs count. NULL = skip */
  int32_t* dropped;       /* int32 [1]: rows not finite or out of range. NULL = skip */
  int32_t* remap;         /* int32 [N]: the output row of every input row's voxel, -1 out of range. NULL = skip */
  int32_t* faces;         /* int32 [face_capacity,3]: the kept faces over the output rows; needs face_count. NULL = skip */
  int32_t* face_index;    /* int32 [face_capacity]: the source face of every kept face; needs face_count. NULL = skip */
  int32_t* face_count;    /* int32 [B+1]: kept faces per view, then their total. NULL = skip */
  int64_t face_capacity;  /* rows of faces / face_index, >= 0 */
  int32_t* faces_dropped; /* int32 [3]: invalid, degenerate, duplicate faces. NULL = skip */
} md_points_decimate;

/* The stand-alone operator on caller device lists, modelled on md_op_voxel_thin: the N rows and the F faces are one view. Of
 * `out` the fields xyz, rgb, conf, count (int32 [2]: M twice) and capacity are used, the others must be NULL; normals_out
 * [capacity,3] takes the normals rows; dec->face_count is int32 [2]. Everything is enqueued on `stream`; the call returns after
 * the stream has drained, because its scratch is freed on return. Errors, before any launch: dev / dec / out NULL, xyz_dev
 * NULL with N > 0, faces_dev NULL with F > 0, voxel not finite or <= 0, N < 0, F < 0, capacity < 0, face_capacity < 0, a
 * compacted output (xyz, rgb, conf, normals_out, index, weight) without count, faces / face_index without face_count, an
 * rgb / conf / normals output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG; N >= 2^30 or
 * F >= 2^30 -> MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP after the launches;
 * the outputs and the class counts of such a call are unspecified. */
int md_op_decimate_mesh(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                        int64_t N, const int32_t* faces_dev, int64_t F, const md_points_decimate* dec, const md_points_outputs* out,
                        float* normals_out, void* stream);
/* md_infer_points_outlier with the decimation behind the mesh stage and in front of the point render and the rasteriser. With it
 * on, the scatter fills a grow-only list of the model (at most R = B ceil(H/stride) ceil(W/stride) rows), the mesh stage writes
 * all faces of that list (every row of it is usable as a corner) with their true count to a grow-only home of the model, and the
 * decimation writes the caller's list (out->xyz / rgb / conf, nrm->normals, out->count) and dec's face outputs; the confidence
 * row is the model's confidence map where it has one, whether or not out->conf is set. dec->remap is int32 [R]: rows behind the
 * undecimated total hold -1. dec->face_count is int32 [B+1], by the view of the source face. mesh must be given (its max_rtol
 * sets the edge test; its outputs may all be NULL): mesh->faces and mesh->face_count, if taken, still receive the undecimated
 * mesh of the undecimated list, mesh->pixel_index names rows of that list and dec->remap carries them over. The point render and
 * the rasteriser see the decimated list and the decimated faces; rasterising then needs dec->faces and dec->face_count. dec's
 * pointers are of out_kind. dec NULL or voxel == 0 (its pointers then NULL): md_infer_points_outlier on the same arguments, the
 * same launches and bits. The graph key contains dec's fields. Errors as md_infer_points_outlier's, plus, before any launch:
 * voxel not finite or negative, face_capacity < 0, faces / face_index without face_count, index / weight without count, any of
 * dec's pointers with voxel == 0, decimation without a mesh request or without count, together with voxel thinning (two grids:
 * the decimation is the thinning) or with outlier removal -> MD_ERR_INVALID_ARG; 2 R >= 2^30 -> MD_ERR_SHAPE. With host
 * outputs a probe loop that ran out of table -> MD_ERR_HIP; with device outputs md_model_query(m, "decimate_overflow") reads
 * the flags of the last call that was launched or captured (it waits for the device); as with "voxel_overflow" and
 * "outlier_overflow", a replay of a graph captured for another shape does not move that record, so query after a call of the
 * shape that was enqueued last outside a replay. After the first call of a shape nothing is allocated. */
int md_infer_points_decimate(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                             const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                             const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                             const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec, int out_kind,
                             void* stream);

/* ---- point path: connected components of a mesh, island removal ------------------------------------------------------------
 * N vertex rows and faces int32 [F,3] over them -> the component of every row and the faces of the components that are large
 * enough. Integers only: nothing here computes a float, nothing is averaged and nothing depends on the order in which threads
 * arrive (pipeline.mesh_components restates it in numpy bit for bit).
 *   validity: a face is INVALID when a corner is < 0 or >= N. Invalid faces join nothing, are never kept, and are counted. A
 *     degenerate face (two corners equal) is valid: it joins what it names.
 *   components: two rows are connected when a valid face names both (vertex connectivity: sharing one vertex joins, a shared
 *     edge is not required). label int32 [N]: label[i] = the smallest row index of row i's component; a row that no valid face
 *     names is a component of its own, label[i] = i. component_faces int32 [N]: the number of valid faces in row i's component,
 *     0 for a row that no valid face names.
 *   selection: a valid face is kept iff its component has at least min_faces >= 1 faces. The kept faces come in ascending f
 *     with unchanged corners and unchanged winding; face_index = the source face. face_count[b] = the kept faces whose source
 *     face belongs to view b (the views of the faces are the prefix of the INPUT face counts; the stand-alone operator has one
 *     view), face_count[B] = their true total, also beyond face_capacity: then only the first face_capacity rows are written
 *     and the memory behind them stays untouched.
 *   stats int32 [5]: invalid faces; faces of dropped components; clipped faces (compact, below; 0 without it); components that
 *     have at least one face; components kept.
 *   compact != 0 (stand-alone operator only): the vertex list is compacted too. A row survives iff a face of a KEPT COMPONENT
 *     names it; the survivors come in ascending input index into out->xyz / rgb / conf, normals_out, index (the source row) and
 *     out->count (int32 [2]: M twice); capacity and the memory behind the rows behave as in md_op_voxel_thin. remap int32 [N] =
 *     the true output rank of a surviving row, also when it is >= capacity, and -1 otherwise. The faces are written through
 *     remap, and a face of a kept component with a mapped corner >= capacity is CLIPPED: dropped and counted, so no written face
 *     names an unwritten row. Vertex survival does not depend on clipping. With compact == 0 the vertex outputs, index and remap
 *     must be NULL, and the faces keep the input's indices.
 *   limits: N < 2^30 and F < 2^30.
 * The labelling is a lock-free union-find in device memory (kernels/components_math.h): parent[v] <= v at all times, a root is
 * only ever hooked under a smaller row by compare-and-swap, so the root of a finished component is its smallest row whatever
 * the order of arrival. The forest and the counters are set on the stream inside every call. */
typedef struct md_points_components {
  int32_t min_faces;        /* faces a component needs to be kept, >= 1; 0 = the stage is off (md_infer_points_components) */
  int32_t compact;          /* != 0: compact the vertex list too (md_op_mesh_components only) */
  int32_t* label;           /* int32 [N]: the smallest row of every row's component. NULL = skip */
  int32_t* component_faces; /* int32 [N]: the valid faces of every row's component. NULL = skip */
  int32_t* index;           /* int32 [capacity]: the source row of every surviving row (compact); needs count. NULL = skip */
  int32_t* remap;           /* int32 [N]: the output row of every surviving row, -1 otherwise (compact). NULL = skip */
  int32_t* faces;           /* int32 [face_capacity,3]: the kept faces; needs face_count. NULL = skip */
  int32_t* face_index;      /* int32 [face_capacity]: the source face of every kept face; needs face_count. NULL = skip */
  int32_t* face_count;      /* int32 [B+1]: kept faces per view, then their total. NULL = skip */
  int64_t face_capacity;    /* rows of faces / face_index, >= 0 */
  int32_t* stats;           /* int32 [5]: invalid, dropped, clipped faces, components with a face, components kept. NULL = skip */
} md_points_components;

/* The stand-alone operator on caller device lists, modelled on md_op_decimate_mesh: the N rows and the F faces are one view.
 * The vertex rows are optional: xyz_dev may be NULL with compact == 0 (N still bounds the corners). Of `out` the fields xyz,
 * rgb, conf, count (int32 [2]) and capacity are used, and only with compact; the others must be NULL; out itself may be NULL
 * with compact == 0. comp->face_count is int32 [2]. Everything is enqueued on `stream`; the call returns after the stream has
 * drained, because its scratch is freed on return. Errors, before any launch: dev / comp NULL, min_faces < 1, N < 0, F < 0,
 * faces_dev NULL with F > 0, face_capacity < 0, faces / face_index without face_count; with compact == 0: a vertex output,
 * index, remap or count set; with compact != 0: out NULL, capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index)
 * without count, an xyz / rgb / conf / normals output without that input row; a dense output or out->depth set
 * -> MD_ERR_INVALID_ARG; N >= 2^30 or F >= 2^30 -> MD_ERR_SHAPE. */
int md_op_mesh_components(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                          int64_t N, const int32_t* faces_dev, int64_t F, const md_points_components* comp, const md_points_outputs* out,
                          float* normals_out, void* stream);
/* md_infer_points_decimate with the island removal behind the mesh stage and in front of the point render and the rasteriser
 * (launch-order name "points_components"). With it on, the mesh stage writes all faces of the call's list with their true
 * per-view counts to a grow-only home of the model; mesh->faces and mesh->face_count, if taken, still receive the unfiltered
 * mesh; the stage writes comp's outputs, and the rasteriser reads those: rasterising then needs comp->faces and
 * comp->face_count. label and component_faces are int32 [R] over the call's list, R = B ceil(H/stride) ceil(W/stride); rows
 * behind its total hold -1 and 0. The in-call stage is face-only: the list and the point render are unchanged. comp's pointers
 * are of out_kind. comp NULL or min_faces == 0 (its pointers then NULL): md_infer_points_decimate on the same arguments, the
 * same launches, bits and launch-order names. The graph key contains comp's fields. Errors as md_infer_points_decimate's, plus,
 * before any launch: min_faces < 0, compact != 0, face_capacity < 0, faces / face_index without face_count, any of comp's
 * pointers with min_faces == 0, the stage without a mesh request or without the list's count, or together with dec on, voxel thinning or
 * outlier removal (the rows the faces name no longer exist) -> MD_ERR_INVALID_ARG; 2 R >= 2^30 -> MD_ERR_SHAPE. After the first call of a shape nothing is allocated. */
int md_infer_points_components(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                               const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                               const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                               const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                               const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                               const md_points_components* comp, int out_kind, void* stream);
/* PROCESS-WIDE (returns the previous setting): the capacity of the (face, target) queue of later md_op_render_mesh /
 * md_infer_points_raster calls, 0 = the default (2^20 pairs). A push that finds the queue full draws the face in place: same
 * bits at every capacity; for the test of that branch. MD_ERR_INVALID_ARG (< 0) for a negative capacity. */
int md_debug_raster_queue(int capacity);

/* ---- point path: Taubin smoothing of a mesh and its vertex normals -----------------------------------------------------------
 * N vertex rows xyz [N,3] and faces int32 [F,3] over them -> the smoothed rows and the area-weighted normals of the smoothed
 * faces. This stage averages, and still nothing depends on the order in which threads arrive: the rows are rounded to an integer
 * lattice once and every sum is an integer sum modulo 2^64 (pipeline.smooth_mesh restates it in numpy bit for bit).
 *   lattice: step is an f32, finite and > 0. Per axis k = rintf(p / step): one f32 division, round half to even. A row is IN
 *     RANGE when its coordinates are finite and |k| <= 2^22 on every axis, compared in float.
 *   faces: a face is INVALID when a corner is < 0 or >= N or names a row that is not in range. A valid face is DEGENERATE when
 *     two of its corners are equal. Both kinds contribute nothing and are counted. The other faces are LIVE.
 *   topology, once, from the faces alone: for a live face (a,b,c) and each corner v with successor n and predecessor p in the
 *     winding, deg[v] += 2 and open[v] += mix(n) - mix(p) in uint64 modulo 2^64, mix = splitmix64's finaliser (x ^= x >> 30;
 *     x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31). Around a closed, consistently oriented fan
 *     every neighbour is once a successor and once a predecessor and open == 0; an open fan leaves mix(last) - mix(first). The
 *     contract is this formula, not "boundary": a collision is part of it and is bit-identical too.
 *   pinned rows: deg == 0, or the row is not in range, or pin_boundary != 0 and open != 0.
 *   steps: Jacobi updates, every row reads the positions of the step before. mu != 0: 2 * iterations steps with the factor
 *     lambda on the even and mu on the odd ones (Taubin); mu == 0: iterations steps with lambda (Laplacian). In a step a live
 *     face adds k[n] + k[p] per axis to S[v] (int64) for each of its corners, and a row that is not pinned then does per axis
 *     d = (double)S / (double)deg - (double)k;  r = rint((double)factor * d), clamped to [-2^62, 2^62];  k += (int64)r
 *     in f64 with one rounded operation each, rint half to even, no fused multiply-add. Integer arithmetic wraps modulo 2^64.
 *   positions: a row whose final lattice position equals its first one on all axes returns its INPUT BITS (every pinned row
 *     does); any other row returns (float)((double)k * (double)step) per axis.
 *   normals: every live face adds the int64 cross product (k_b - k_a) x (k_c - k_a) of the final lattice positions to Nrm of
 *     its three corners. A row with deg == 0 or Nrm == 0 gets (0,0,0); any other, per axis, (float)((double)Nrm_a / l) with
 *     l = sqrt((x*x + y*y) + z*z) in f64. The sign follows the winding.
 *   stats int32 [5]: invalid faces; degenerate faces; rows not in range; rows with deg > 0 and open != 0 (pinned or not); rows
 *     that moved.
 *   limits: 0 < lambda <= 1, -1 <= mu <= 0, 1 <= iterations <= 1024, N < 2^30 and F < 2^30.
 * Integer global atomics and vector stores only; the lattice, the accumulators and the counters are set on the stream inside
 * every call. */
typedef struct md_points_smooth {
  float step;           /* the lattice side, finite and > 0 */
  float lambda;         /* the factor of the even steps, in (0, 1] */
  float mu;             /* the factor of the odd steps, in [-1, 0]; 0 = Laplacian smoothing, no odd steps */
  int32_t iterations;   /* 1..1024; 0 = the stage is off (md_infer_points_smooth) */
  int32_t pin_boundary; /* != 0: rows with open != 0 do not move */
  float* xyz;           /* float [capacity,3]: the smoothed rows. NULL = skip */
  float* normals;       /* float [capacity,3]: the vertex normals of the smoothed mesh. NULL = skip */
  int32_t* stats;       /* int32 [5]: invalid and degenerate faces, rows not in range, open rows, moved rows. NULL = skip */
} md_points_smooth;

/* The stand-alone operator on caller device lists, modelled on md_op_mesh_components: all N rows take part, rows >= capacity are
 * not written and the memory behind them stays untouched. Everything is enqueued on `stream`; the call returns after the stream
 * has drained, because its scratch is freed on return. Errors, before any launch: dev / smooth NULL, step not finite or <= 0,
 * lambda, mu or iterations outside their limits (NaN included), N < 0, F < 0, capacity < 0, xyz_dev NULL with N > 0, faces_dev
 * NULL with F > 0 -> MD_ERR_INVALID_ARG; N >= 2^30 or F >= 2^30 -> MD_ERR_SHAPE. */
int md_op_smooth_mesh(md_device_t dev, const float* xyz_dev, int64_t N, const int32_t* faces_dev, int64_t F, const md_points_smooth* smooth,
                      int64_t capacity, void* stream);
/* md_infer_points_components with the smoothing behind the mesh stage and the island removal and in front of the rasteriser
 * (launch-order name "points_smooth"). The stage works on the call's list, N = min(count, capacity) read on the device, and on
 * the faces the rasteriser would read: comp's kept faces when that stage is on (smoothing then needs comp->faces and
 * comp->face_count), the mesh stage's otherwise (written, complete, to a grow-only home of the model; mesh->faces, if taken, are
 * a copy). It writes smooth->xyz, normals [out->capacity,3] (rows >= N are not written) and stats, of out_kind. The caller's
 * list, nrm's per-pixel normals and the point render are unchanged; the rasteriser reads the smoothed positions when the stage
 * is on. smooth NULL or iterations == 0 (its pointers then NULL): md_infer_points_components on the same arguments, the same
 * launches, bits and launch-order names. The graph key contains smooth's fields. Errors as md_infer_points_components', plus,
 * before any launch: a limit of the contract broken, a pointer set with iterations == 0, the stage without a mesh request or
 * without the list's count, or together with dec on, voxel thinning or outlier removal (md_op_smooth_mesh serves those routes)
 * -> MD_ERR_INVALID_ARG; 2 R >= 2^30 -> MD_ERR_SHAPE. After the first call of a shape nothing is allocated. */
int md_infer_points_smooth(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                           const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                           const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                           const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                           const md_points_components* comp, const md_points_smooth* smooth, int out_kind, void* stream);

/* ---- point path: RANSAC plane extraction from a point list ---------------------------------------------------------------------
 * A list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3] -> up to P = `planes` planes
 * (1..8), the label of every row, and with mode 1 / 2 the list without / of the plane rows. The decision is an integer inlier
 * count of a deterministic f32 predicate and the winner an arg-max with a fixed tie rule, so nothing depends on the order in
 * which threads arrive. f32, one rounded operation per step, no fused multiply-add, in exactly the order written (sqrtf and /
 * are the correctly rounded ones); pipeline.fit_planes restates it in numpy bit for bit. Denormals are outside the contract.
 *   live rows: a row with a coordinate that is not finite is dropped: label -2, counted in `dropped`. Before round 0 every other
 *     row is live (label -1). Rows at and beyond the device count of the list are not rows.
 *   round p = 0 .. P-1:
 *   1 live index: the live rows in ascending row order are live[0 .. M_p). M_p < 3: the round fails.
 *   2 sampling: hypothesis h = 0 .. Hh-1 (Hh = `hypotheses`, 1..4096) draws corner j = 0, 1, 2 as row live[mix64(x) mod M_p],
 *     x = (u64)seed << 32 | (u64)p << 28 | (u64)h << 2 | j, the modulo unsigned 64-bit, mix64 splitmix64's finaliser
 *     (x ^= x >> 30, x *= 0xbf58476d1ce4e5b9, x ^= x >> 27, x *= 0x94d049bb133111eb, x ^= x >> 31). Two equal rows among the
 *     three make the hypothesis invalid.
 *   3 plane: e1 = p1 - p0, e2 = p2 - p0; n.x = e1.y*e2.z - e1.z*e2.y, n.y = e1.z*e2.x - e1.x*e2.z, n.z = e1.x*e2.y - e1.y*e2.x
 *     (two products, one subtraction each); len2 = (n.x*n.x + n.y*n.y) + n.z*n.z; invalid unless len2 is finite and > 1e-30f;
 *     s = sqrtf(len2), n = n / s (three divisions); d = -((n.x*p0.x + n.y*p0.y) + n.z*p0.z). Orientation: d < 0 negates n and d;
 *     d == 0 (either zero) negates both when the first non-zero component of n is negative: the normal faces the origin, the
 *     camera of a single view. With axis_min_cos > 0 the hypothesis is invalid unless
 *     fabsf((n.x*a.x + n.y*a.y) + n.z*a.z) >= axis_min_cos; the axis is used as given, not normalised.
 *   4 inliers: live row q is an inlier of a valid hypothesis when fabsf(((n.x*q.x + n.y*q.y) + n.z*q.z) + d) <= tol (inclusive)
 *     and, with normal_min_cos > 0, fabsf((n.x*m.x + n.y*m.y) + n.z*m.z) >= normal_min_cos for its normal m (an all-zero normal
 *     fails). count[h] = the inliers, 0 for an invalid hypothesis. The winner is the largest count, among equal counts the
 *     smallest h. The round succeeds when that count >= min_inliers (>= 3).
 *   5 outcome: success: plane[p] = (n, d) of the winner, hypothesis[p] = h, plane_count[p] = count; its inliers get label p and
 *     leave the live set. Failure: this and every later round write nothing: plane[p..] = 0, hypothesis = -1, plane_count = 0.
 *     All P rounds are enqueued regardless (a round behind a failed one finds a device flag set), so the launch sequence is
 *     static. plane_count[P] = the planes found.
 *   mode 0: labels only. mode 1 keeps the rows with label -1, mode 2 the rows with label >= 0: the survivors in ascending input
 *     row, every given row copied unchanged, index = the source row; count[b] = the survivors of view b, count[B] = their total
 *     M, also when M exceeds `capacity`: then only the first `capacity` rows are written and the memory behind them stays
 *     untouched. All views of a call share the planes.
 *   The plane is the winning hypothesis's: there is no least-squares refit (it would need float sums in a fixed order). */
typedef struct md_points_planes {
  int32_t planes;       /* P, 1..8; 0 = the stage is off (md_infer_points_planes) */
  int32_t hypotheses;   /* Hh per plane, 1..4096 */
  float tol;            /* finite and > 0 */
  int32_t min_inliers;  /* >= 3 */
  uint32_t seed;
  float normal_min_cos; /* in [0, 1]; 0 = normals not used, > 0 needs normals */
  float axis[3];        /* finite when axis_min_cos > 0 */
  float axis_min_cos;   /* in [0, 1]; 0 = no axis constraint */
  int32_t mode;         /* 0 = label only, 1 = drop the plane rows, 2 = keep only the plane rows */
  float* plane;         /* float [P,4]: n.x n.y n.z d. NULL = skip */
  int32_t* plane_count; /* int32 [P+1]: the inliers of every plane, then the planes found. NULL = skip */
  int32_t* hypothesis;  /* int32 [P]: the winning h, -1 for a round that did not succeed. NULL = skip */
  int32_t* label;       /* int32 [N] over the INPUT rows: the plane, -1 none, -2 dropped. NULL = skip */
  int32_t* index;       /* int32 [capacity], mode 1 / 2: the source row of every output row; needs count. NULL = skip */
  int32_t* dropped;     /* int32 [1]: rows with a coordinate that is not finite. NULL = skip */
} md_points_planes;

/* The stand-alone operator on caller device lists, modelled on md_op_radius_outliers: the N rows are one view. Of `out` the
 * fields xyz, rgb, conf, count (int32 [2]: M twice) and capacity are used, with mode 1 / 2 only; the others must be NULL;
 * normals_out [capacity,3] takes the normals rows. Everything is enqueued on `stream`; the call returns after the stream has
 * drained, because its scratch is freed on return. Errors, before any launch: dev / pln / out NULL, xyz_dev NULL with N > 0, an
 * option outside its range (planes 0 included), normal_min_cos > 0 without normals_dev, axis_min_cos > 0 with an axis that is not
 * finite, N < 0, capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index) without count or with mode 0, an rgb /
 * conf / normals output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG; N >= 2^30 -> MD_ERR_SHAPE. */
int md_op_fit_planes(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                     int64_t N, const md_points_planes* pln, const md_points_outputs* out, float* normals_out, void* stream);
/* md_infer_points_smooth with the plane extraction behind every other list and mesh stage and in front of the point render and the
 * rasteriser (launch-order name "points_planes"). It reads the list the mesh stages read, behind view filter, outlier removal
 * and thinning; the normals predicate reads nrm's list normals (normal_min_cos > 0 needs nrm->normals). mode 0: the caller's
 * list is unchanged and pln->label is int32 over its rows, [out->capacity], of which the first min(count[B], capacity) are
 * written. mode 1 / 2: the stage writes the caller's list and out->count (the stage before it then fills a grow-only list of the
 * model), pln->label is int32 over the rows of that input list (at most B ceil(H/stride) ceil(W/stride)) and pln->index names
 * its rows; the point render sees the list the call ends with. pln's pointers are of out_kind. The scratch comes from grow-only
 * buffers of the model: after the first call of a shape nothing is allocated. pln NULL or planes == 0 (its pointers then NULL):
 * md_infer_points_smooth on the same arguments, the same launches and bits. The graph key contains pln's fields. Errors as
 * md_infer_points_smooth's, plus, before any launch: an option outside its range, normal_min_cos > 0 without the list normals,
 * axis_min_cos > 0 with an axis that is not finite, the stage without the list's count, index without mode 1 / 2, any of pln's
 * pointers with planes == 0, mode 1 / 2 together with a mesh, decimation, components or smoothing (the rows the faces name would
 * vanish) or with voxel thinning's or the outlier removal's index (the rows they are parallel to are not returned), mode 0
 * together with decimation -> MD_ERR_INVALID_ARG; a list of >= 2^30 rows -> MD_ERR_SHAPE. */
int md_infer_points_planes(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                           const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                           const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                           const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                           const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                           int out_kind, void* stream);

/* ---- point path: DBSCAN / Euclidean clustering of a point list ---------------------------------------------------------------
 * A list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3] -> the cluster of every row,
 * a table of the clusters and, with mode 1, the rows of the kept clusters. Every output is integers on a deterministic f32
 * predicate (or a selection among the input coordinates), so nothing depends on the order in which threads arrive;
 * pipeline.cluster_points restates it in numpy bit for bit. f32, one rounded operation per step, no fused multiply-add.
 * Denormals are outside the contract.
 *   cells and neighbours: the outlier removal's (md_points_outlier above), word for word: cell c_a = floorf(p_a / radius), the
 *     same range test and 63-bit key; rows out of range or not finite get label -2 and are counted in `dropped`; in-range rows
 *     i != j are neighbours when their cells differ by at most 1 on every axis AND (dx*dx + dy*dy) + dz*dz <= radius*radius,
 *     inclusive. The cell condition is part of the definition. Rows with equal coordinates are neighbours of each other.
 *   core rows: k = min_neighbours, 0 <= k <= 2^20. An in-range row is a core row when it has at least k neighbours (the count
 *     saturates at k). k = 0: every in-range row is a core row and the stage is plain Euclidean cluster extraction.
 *   clusters: the connected components of the graph whose vertices are the core rows and whose edges are the neighbour pairs of
 *     core rows. The label of a cluster is its smallest core row.
 *   border rows: an in-range row that is not core but has a core neighbour takes the smallest label among its core neighbours'
 *     clusters: a fixed rule, where textbook DBSCAN depends on the order of the visit. A border row never joins two clusters.
 *   noise: an in-range row that is neither gets label -1.
 *   sizes: the size of a cluster is its core rows plus its border rows. A cluster is kept when min_points <= size and
 *     (max_points == 0 or size <= max_points), min_points >= 1. Kept clusters get the dense ids 0 .. C-1 in ascending label.
 *   label / cluster_size / cluster, int32 over the INPUT rows [N]: the label before the size filter; the size of the row's cluster
 *     (0 for noise and dropped rows); the dense id of a kept cluster, -1 for every other in-range row, -2 for a dropped row.
 *   the table, `table_capacity` rows: table_label, table_size, and box f32 [6] = min x y z, max x y z over the cluster's rows,
 *     under the total order of the usual ordered key of an f32 (bits ^ 0x80000000 for a clear sign bit, ~bits for a set one:
 *     -0 lies below +0); each value is the bit pattern of an input coordinate. Ids at or beyond table_capacity are not written
 *     and the memory behind the clusters that exist stays untouched.
 *   stats int32 [4]: clusters found, clusters kept, noise rows, rows in kept clusters: true counts whatever the capacities.
 *   mode 0: labels only. mode 1 keeps the rows of kept clusters: the survivors in ascending input row, every given row copied
 *     unchanged, index = the source row; count[b] = the survivors of view b, count[B] = their total M, also when M exceeds
 *     `capacity`: then only the first `capacity` rows are written and the memory behind them stays untouched. All views of a
 *     call share the grid and the clusters. N < 2^30.
 * The grid is the outlier removal's with 16-byte bucket entries (xyz and the source row); the labelling is the lock-free
 * union-find of the mesh components (parent[v] <= v: the root of a finished tree is its smallest row). */
typedef struct md_points_clusters {
  float radius;           /* 0 = the stage is off (md_infer_points_clusters), finite and >= 0 */
  int32_t min_neighbours; /* k, 0 .. 2^20 */
  int32_t min_points;     /* >= 1 */
  int32_t max_points;     /* 0 = no upper limit, else >= min_points */
  int32_t mode;           /* 0 = label only, 1 = keep the rows of kept clusters */
  int32_t* label;         /* int32 [N] over the INPUT rows. NULL = skip */
  int32_t* cluster_size;  /* int32 [N]. NULL = skip */
  int32_t* cluster;       /* int32 [N]. NULL = skip */
  int32_t* table_label;   /* int32 [table_capacity]. NULL = skip */
  int32_t* table_size;    /* int32 [table_capacity]. NULL = skip */
  float* box;             /* float [table_capacity,6]. NULL = skip */
  int64_t table_capacity; /* >= 0 */
  int32_t* stats;         /* int32 [4]. NULL = skip */
  int32_t* index;         /* int32 [capacity], mode 1: the source row of every output row; needs count. NULL = skip */
  int32_t* dropped;       /* int32 [1]. NULL = skip */
} md_points_clusters;

/* The stand-alone operator on caller device lists, modelled on md_op_fit_planes: the N rows are one view. Of `out` the fields
 * xyz, rgb, conf, count (int32 [2]: M twice) and capacity are used, with mode 1 only; the others must be NULL; normals_out
 * [capacity,3] takes the normals rows. Everything is enqueued on `stream`; the call returns after the stream has drained,
 * because its scratch is freed on return. Errors, before any launch: dev / clu / out NULL, xyz_dev NULL with N > 0, radius not
 * finite or <= 0, min_neighbours < 0 or > 2^20, min_points < 1, max_points < 0 or 0 < max_points < min_points, mode outside 0
 * and 1, N < 0, capacity or table_capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index) without count or with
 * mode 0, an rgb / conf / normals output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG;
 * N >= 2^30 -> MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP after the launches. */
int md_op_cluster_points(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                         int64_t N, const md_points_clusters* clu, const md_points_outputs* out, float* normals_out, void* stream);
/* md_infer_points_planes with the clustering behind the plane extraction and in front of the point render and the rasteriser
 * (launch-order name "points_clusters"). It reads the list the plane stage ends with, so planes with mode 1 followed by
 * clustering is one call. mode 0: the caller's list is unchanged and label / cluster_size / cluster are int32 over its rows,
 * [out->capacity], of which the first min(count[B], capacity) are written. mode 1: the stage writes the caller's list and
 * out->count (the stage before it then fills a grow-only list of the model), the three row outputs are int32 over the rows of
 * that input list (at most B ceil(H/stride) ceil(W/stride)) and clu->index names its rows; the point render sees the list the
 * call ends with. clu's pointers are of out_kind. The scratch comes from grow-only buffers of the model: after the first call
 * of a shape nothing is allocated. clu NULL or radius == 0 (its pointers then NULL): md_infer_points_planes on the same
 * arguments, the same launches and bits. The graph key contains clu's fields. Errors as md_infer_points_planes's, plus, before
 * any launch: an option outside its range (radius negative or not finite), the stage without the list's count, index without
 * mode 1, any of clu's pointers with radius == 0, mode 1 together with a mesh, decimation, components or smoothing (the rows
 * the faces name would vanish) or with an earlier stage's index (voxel thinning's, the outlier removal's, the plane stage's:
 * the rows they are parallel to are not returned) or behind a plane stage with mode 0 (its label would be parallel to rows that
 * are not returned), mode 0 without the list output out->xyz or together with decimation -> MD_ERR_INVALID_ARG; a list of
 * >= 2^30 rows -> MD_ERR_SHAPE. With host outputs a probe loop that ran out of table -> MD_ERR_HIP; with device outputs
 * md_model_query(m, "clusters_overflow") reads the flag of the last call that was launched or captured (it waits for the
 * device), as "outlier_overflow" does. */
int md_infer_points_clusters(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                             const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                             const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                             const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                             const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                             const md_points_clusters* clu, int out_kind, void* stream);

/* ---- point path: the nearest row of a reference cloud for every row of a point list -------------------------------------------
 * A source list xyz f32 [N,3] with optional parallel rows conf f32 [N], rgb u8 [N,3] and normals f32 [N,3], and a target list
 * f32 [T,3] -> for every source row the nearest target row within `radius`, counters for precision / recall, and, with mode 1 /
 * 2, the source rows with / without a counterpart. Every output is a selection on a deterministic f32 value, so nothing depends
 * on the order in which threads arrive; pipeline.match_points restates it in numpy bit for bit. N and T < 2^30. f32, one
 * rounded operation per step, no fused multiply-add. Denormals are outside the contract.
 *   cells: the outlier removal's (md_points_outlier above), word for word, on both lists: cell c_a = floorf(p_a / radius), the
 *     same range test and 63-bit key. Target rows that are not finite or out of range are not in the grid. Source rows that are
 *     not finite or out of range are dropped: nearest = -2, counted in `dropped`.
 *   candidates: target row j is a candidate of in-range source row i when their cells differ by at most 1 on every axis AND
 *     d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius, inclusive, with dx = t_x - s_x and so on. The cell condition is part of the
 *     definition.
 *   nearest: the candidate with the smallest 64-bit key (bits(d2) << 32) | j. d2 >= +0 and is never NaN here, so the bit order
 *     is the numeric order; ties go to the smallest target row; duplicate target rows are legal. No candidate: nearest = -1.
 *   nearest int32 [N] / dist2 f32 [N] over the INPUT rows: the target row (-1 none, -2 dropped) and its d2, the bit pattern
 *     0x7F800000 for -1 and -2 rows.
 *   tol[4]: each entry 0 (unused) or in (0, radius]. A matched row is within tol[t] when d2 <= tol[t]*tol[t].
 *   stats int32 [8], true counts whatever the capacities: [0] in-range source rows, [1] matched rows, [2] target rows in the
 *     grid, [3] 0, [4..8) rows within tol[0..4), 0 for an unused entry. Precision at tol[t] is stats[4+t] / N; recall is the same
 *     figure of the swapped call.
 *   mode 0: labels only. mode 1 keeps the matched rows, mode 2 the in-range rows without a match; dropped rows leave in both.
 *     Compaction is the cluster stage's mode 1: the survivors in ascending input row, every given row copied unchanged, index =
 *     the source row; count[b] = the survivors of view b, count[B] = their total M, also when M exceeds `capacity`: then only the
 *     first `capacity` rows are written and the memory behind them stays untouched. All views of a call share the target.
 * The grid is the clustering's, 16-byte bucket entries (xyz and the target row), built from the target and sized by T. */
typedef struct md_points_match {
  float radius;          /* 0 = the stage is off (md_infer_points_match) */
  const float* target;   /* f32 [target_rows,3] */
  int64_t target_rows;
  int32_t target_kind;   /* MD_MEM_HOST | MD_MEM_DEVICE; the operator takes device only */
  int32_t mode;          /* 0 label, 1 keep matched, 2 keep unmatched */
  float tol[4];
  int32_t* nearest;      /* int32 [N] over the INPUT rows. NULL = skip */
  float* dist2;          /* f32 [N]. NULL = skip */
  int32_t* stats;        /* int32 [8]. NULL = skip */
  int32_t* index;        /* int32 [capacity], modes 1 / 2; needs count. NULL = skip */
  int32_t* dropped;      /* int32 [1]. NULL = skip */
} md_points_match;

/* The stand-alone operator on caller device lists, modelled on md_op_cluster_points: the N rows are one view. Of `out` the fields
 * xyz, rgb, conf, count (int32 [2]: M twice) and capacity are used, with mode 1 / 2 only; the others must be NULL; normals_out
 * [capacity,3] takes the normals rows. Everything is enqueued on `stream`; the call returns after the stream has drained,
 * because its scratch is freed on return. T == 0 is legal: every in-range row gets -1. Errors, before any launch: dev / mat /
 * out NULL, xyz_dev NULL with N > 0, radius not finite or <= 0 or radius*radius not finite, a tol entry negative, not finite or
 * above radius, mode outside 0..2, target_rows < 0, target NULL with target_rows > 0, target_kind not MD_MEM_DEVICE, N < 0,
 * capacity < 0, a compacted output (xyz, rgb, conf, normals_out, index) without count or with mode 0, an rgb / conf / normals
 * output without that input row, a dense output or out->depth set -> MD_ERR_INVALID_ARG; N or target_rows >= 2^30 ->
 * MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP after the launches. */
int md_op_match_points(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                       int64_t N, const md_points_match* mat, const md_points_outputs* out, float* normals_out, void* stream);
/* md_infer_points_clusters with the matching behind the plane extraction and in front of the clustering (launch-order name
 * "points_match"), so "drop the floor, drop what the reference scan already holds, cluster the rest" is one call. mode 0: the
 * caller's list is unchanged and nearest / dist2 are over its rows, [out->capacity], of which the first min(count[B], capacity)
 * are written; it needs out->xyz and the list's count. mode 1 / 2: the stage is a link of the list chain scatter -> outlier
 * removal -> thinning -> planes (mode 1 / 2) -> match (mode 1 / 2) -> clusters (mode 1): the last link writes the caller's list
 * and out->count, every other one a grow-only list of the model; nearest / dist2 are over the rows of the stage's input list
 * (at most B ceil(H/stride) ceil(W/stride)) and mat->index names its rows. mat's pointers are of out_kind; the target is of
 * target_kind, and a host target is copied into a grow-only buffer of the model with every call. A device target is read by
 * address: a graph replay sees its current contents. The scratch comes from grow-only buffers of the model: after the first
 * call of a shape nothing is allocated. mat NULL or radius == 0 (its pointers then NULL): md_infer_points_clusters on the same
 * arguments, the same launches and bits. The graph key contains every field of mat. Errors as md_infer_points_clusters's,
 * plus, before any launch: the operator's refusals of radius (0 allowed), tol, mode and the target (target_kind may be
 * MD_MEM_HOST), the stage without the list's count, index without mode 1 / 2, any of mat's pointers with radius == 0, mode 1 / 2
 * together with a mesh, decimation, components or smoothing (the rows the faces name would vanish) or with an earlier stage's
 * index (voxel thinning's, the outlier removal's, the plane stage's) or behind a plane stage with mode 0, mode 0 without the
 * list output out->xyz or together with decimation, clustering with mode 1 behind matching with mode 0 (its rows would not be
 * the rows `nearest` is parallel to) or together with mat->index -> MD_ERR_INVALID_ARG; a list or a target of >= 2^30 rows ->
 * MD_ERR_SHAPE. With host outputs a probe loop that ran out of table -> MD_ERR_HIP; with device outputs
 * md_model_query(m, "match_overflow") reads the flag of the last call that was launched or captured, as "clusters_overflow"
 * does. */
int md_infer_points_match(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                          const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                          const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                          const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                          const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                          const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                          const md_points_clusters* clu, const md_points_match* mat, int out_kind, void* stream);

/* ---- point path: rigid ICP registration of a point list onto a reference cloud ---------------------------------------------------
 * A source list xyz f32 [N,3] (optional normals f32 [N,3]) and a target list f32 [T,3] -> the rigid transform (rotation and
 * translation, no scale) that moves the source onto the target by point-to-point ICP, with per-iteration pair counts and
 * squared-distance sums and, optionally, the moved rows. The arithmetic is held once in kernels/register_math.h, which compiles
 * for the device and the host; pipeline.register_points restates it in numpy bit for bit. Denormals are outside the contract.
 *   transform A: twelve f64, R row-major in A[0..9), then t in A[9..12). A_0 = init, or the identity.
 *   one pass under A, for every source row i below the live count:
 *     moved row m_a = (float)(((R_a0*x + R_a1*y) + R_a2*z) + t_a): the f32 inputs widened to f64, every operation rounded once,
 *       one final cast to f32 (round to nearest even).
 *     nearest target row j of m: md_points_match's definition word for word with cell side `radius`: the 27 cells, the gate
 *       (dx*dx + dy*dy) + dz*dz <= radius*radius in f32, the smallest key (bits(d2) << 32) | j. A moved row that is not finite
 *       or out of the grid's range is dropped and has no pair.
 *     a paired row contributes sixteen f64 leaves built from the ORIGINAL source row p and the target row q, widened exactly:
 *       p_a (leaves 0..2), q_a (3..5), p_a * q_b (6 + 3a + b), (double)d2 (15). So the solve gives the full transform and
 *       nothing is composed. Every other item contributes +0.0. The pair count is an integer.
 *   the sums have a fixed shape over the tile layout item = tile*4096 + step*256 + thread: a thread's value is the left fold,
 *     from +0.0, of its leaves over step = 0..15; a wave's value the halving tree over its lanes (v[l] += v[l+h] for l < h, h =
 *     32, 16, .., 1); a tile's value (W0 + W1) + (W2 + W3). The call's value: thread u of one 256-thread workgroup left-folds,
 *     from +0.0, the tile values u, u+256, u+512, .. in ascending order; the 256 thread values go through the same wave tree and
 *     four-wave combine. All leaves are finite, so nothing depends on the order of arrival.
 *   the solve (register_math.h, reg_solve; one thread, f64, only + - * /, sqrt and comparisons): centroids pbar = S_p / n,
 *     qbar = S_q / n; H_ab = S_pq_ab - S_p_a * qbar_b; Horn's symmetric 4x4 matrix of H; a fixed number of cyclic Jacobi sweeps
 *     (kRegSweeps; theta = (a_qq - a_pp) / (2 a_pq), t = sign / (|theta| + sqrt(theta*theta + 1)), c = 1 / sqrt(t*t + 1), s = t*c;
 *     a pivot that is exactly 0 is skipped); the eigenvector of the largest eigenvalue (ties: smallest index), normalised, w >= 0;
 *     R from the quaternion; t = qbar - R pbar. The operation order is the header's.
 *   iteration k = 0..K-1: a pass under A_k, the sums, then: n < min_pairs -> status 2, A stays, every later iteration changes
 *     nothing; otherwise A_{k+1} = the solve's result, and with the stop test on (rot_eps > 0 or trans_eps > 0) and
 *     max |R'_ab - R_ab| <= rot_eps and max |t'_a - t_a| <= trans_eps -> status 1, likewise. All K iterations are always
 *     enqueued. Then one evaluation pass under the final A, without a solve: entry K of the histories and the row outputs.
 *   pairs int32 [K+1] / sum_d2 f64 [K+1]: the pair count and the sum of d2 of the pass at entry k; 0 for skipped iterations.
 *   stats int32 [8]: [0] solves done, [1] status (0 ran all K, 1 converged, 2 too few pairs), [2] in-range rows and [3] pairs of
 *     the evaluation pass, [4] target rows in the grid, [5..8) 0. dropped int32 [1]: rows whose moved row is not finite or out of
 *     range in the evaluation pass.
 *   nearest int32 [N] / dist2 f32 [N]: md_points_match's mode 0 outputs for the moved rows of the evaluation pass.
 *   moved rows (the operator's xyz_out) f32 [N,3], written for every row, and rotated normals (float)((R_a0*nx + R_a1*ny) +
 *     R_a2*nz); a NaN component is written as the bit pattern 0x7FC00000. */
typedef struct md_points_register {
  float radius;          /* pairing radius and cell side; 0 = the stage is off (md_infer_points_register) */
  const float* target;   /* f32 [target_rows,3] */
  int64_t target_rows;
  int32_t target_kind;   /* MD_MEM_HOST | MD_MEM_DEVICE; the operator takes device only */
  int32_t iterations;    /* K, 1..64 */
  int32_t min_pairs;     /* >= 3 */
  int32_t apply;         /* md_infer_points_register: 1 = the moved rows (and normals) replace the list's in place; 0 = estimate
                          * only. The operator reads only its range: its moved rows go to xyz_out / normals_out */
  double rot_eps;        /* both 0 = no stop test */
  double trans_eps;
  const double* init;    /* HOST memory, f64 [12]; NULL = identity */
  double* transform;     /* f64 [12]. NULL = skip */
  int32_t* pairs;        /* int32 [iterations + 1]. NULL = skip */
  double* sum_d2;        /* f64 [iterations + 1]. NULL = skip */
  int32_t* stats;        /* int32 [8]. NULL = skip */
  int32_t* dropped;      /* int32 [1]. NULL = skip */
  int32_t* nearest;      /* int32 [N]. NULL = skip */
  float* dist2;          /* f32 [N]. NULL = skip */
} md_points_register;

/* The stand-alone operator on caller device lists: the N rows are one view; every pointer but reg->init is a device pointer.
 * xyz_out f32 [N,3] (NULL = skip) takes the moved rows and may be xyz_dev itself: a thread reads only its own row;
 * normals_out f32 [N,3] (NULL = skip) the rotated normals. Launches: reset, insert, alloc, fill (the matching's grid, built
 * once from the target), K times (step, solve), the evaluation step and its reduce. Everything is enqueued on `stream`; the
 * call returns after the stream has drained, because its scratch is freed on return. T == 0 and N == 0 are legal: status 2.
 * Errors, before any launch: dev / reg NULL, xyz_dev NULL with N > 0, radius not finite or <= 0 or radius*radius not finite,
 * target_rows < 0, target NULL with target_rows > 0, target_kind not MD_MEM_DEVICE, iterations outside 1..64, min_pairs < 3,
 * an eps negative or not finite, a value of init not finite, N < 0, normals_out without normals_dev -> MD_ERR_INVALID_ARG;
 * N or target_rows >= 2^30 -> MD_ERR_SHAPE. A probe loop that ran out of table (impossible at load <= 0.5) -> MD_ERR_HIP
 * after the launches. */
int md_op_register_points(md_device_t dev, const float* xyz_dev, const float* normals_dev, int64_t N, const md_points_register* reg,
                          float* xyz_out, float* normals_out, void* stream);
/* md_infer_points_match with the registration directly in front of the matching (launch-order name "points_register"), on the
 * list the matching reads: the call's list below its capacity (nearest / dist2 then [out->capacity], of which the first
 * min(count[B], capacity) are written), or, when the matching (mode 1 / 2) or the clustering (mode 1) cuts, the model's own list
 * in front of them (nearest / dist2 then over its rows, at most B ceil(H/stride) ceil(W/stride)). apply = 0 only estimates.
 * apply = 1 replaces that list's rows, and its normals when the call carries them, by the moved ones in place, so the matching
 * and the clustering see the aligned cloud: "align to the reference, drop what the reference already holds, cluster the rest" is
 * one call. reg's output pointers are of out_kind; init is host memory and its values are read during the call; the target is
 * of target_kind: a host target is copied into a grow-only buffer of the model with every call (such a call is not captured
 * into a graph), a device target is read by address, so a graph replay sees its current contents. The scratch is a grow-only
 * buffer of the model. reg NULL or radius == 0 (its output pointers then NULL): md_infer_points_match on the same arguments, the
 * same launches and bits. The graph key contains every field of reg and the values of init. Errors as md_infer_points_match's,
 * plus, before any launch: the operator's refusals of radius (0 allowed), the target (target_kind may be MD_MEM_HOST),
 * iterations, min_pairs, the eps and init, apply outside 0 and 1, an output pointer with radius == 0, the stage without the
 * list's count or without the list output out->xyz, together with decimation, apply = 1 together with a mesh, components or
 * smoothing (their faces and rows belong to the cloud before it moved) -> MD_ERR_INVALID_ARG; a list or a target of >= 2^30
 * rows -> MD_ERR_SHAPE. The dense maps (point_map, normal_map) are written before the stage and keep the model's frame. With host outputs a probe loop that ran out of table -> MD_ERR_HIP; with device
 * outputs md_model_query(m, "register_overflow") reads the flag as "match_overflow" does. */
int md_infer_points_register(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                             const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                             const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                             const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                             const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                             const md_points_clusters* clu, const md_points_match* mat, const md_points_register* reg,
                             int out_kind, void* stream);

/* ---- point path: point-to-plane ICP against the reference cloud's normals ----------------------------------------------------
 * md_points_register_plane rides beside the unchanged md_points_register and switches its ICP to the point-to-plane metric
 * (Chen & Medioni): the distance of a pair is measured along the target row's normal, so a surface may slide along itself.
 * Transform, histories, stats, dropped, nearest, dist2, the moved rows, init, the stop test and the evaluation pass mean what
 * md_points_register says; the arithmetic is held once in kernels/register_math.h (reg_add_plane_leaves, reg_solve_plane) and
 * pipeline.register_points(target_normals=) restates it in numpy bit for bit. The differences:
 *   pairing: unchanged. The row is moved in f64 and cast once to m; the nearest target row j within radius is md_points_match's;
 *     nearest / dist2 report that pair whatever its normal.
 *   usable pair: the three components of n = target_normals[j] are finite and not all zero (the point path writes (0,0,0) where
 *     a pixel has no normal). Only usable pairs enter the sums; pairs[k], stats[3] and sum_d2[k] count or sum usable pairs only.
 *   leaves per usable pair: 29 f64, from m, q = target[j] and n widened exactly, one rounded operation per step, contraction off:
 *     c = m x n (c0 = m1*n2 - m2*n1, ..: exact products, the subtraction rounds once); d_a = (double)q_a - (double)m_a;
 *     r = ((d0*n0 + d1*n1) + d2*n2); J = (c0, c1, c2, n0, n1, n2); leaves 0..20 the upper triangle of J J^T in row-major order
 *     (J_i * J_j, i <= j), 21..26 J_i * r, 27 r * r, 28 (double)d2 of the pair. The sum tree is md_points_register's over 29
 *     leaves; all leaves are finite, so nothing depends on the order of arrival.
 *   the solve (reg_solve_plane; one thread, f64, only + - * /, sqrt and comparisons): the symmetric 6x6 M and b from the sums;
 *     Cholesky in the order j = 0..5: s = M_jj - sum_{k<j} L_jk^2 as a left fold in ascending k, !(s > 0) -> degenerate,
 *     L_jj = sqrt(s), L_ij = (M_ij - sum_k L_ik L_jk) / L_jj for i > j; forward then backward substitution for
 *     x = (w0, w1, w2, t0, t1, t2); a component of x that is not finite -> degenerate. The increment's rotation dR is that of the
 *     quaternion (1, w0/2, w1/2, w2/2), normalised by len = sqrt(((1 + x*x) + y*y) + z*z) and four divisions, through the
 *     quaternion-to-matrix lines of reg_solve. R'_ab = (dR_a0*R_0b + dR_a1*R_1b) + dR_a2*R_2b;
 *     t'_a = ((dR_a0*t_0 + dR_a1*t_1) + dR_a2*t_2) + tau_a.
 *   iteration: n < min_pairs -> status 2 as before (n counts usable pairs; min_pairs >= 6). A degenerate system -> status 3: A
 *     stays and every later iteration changes nothing (a target with one normal direction only, all rows paired with one target
 *     row). The test is the exact !(s > 0): a deficiency that rounding hides is not detected, and nothing is damped. Otherwise
 *     A_{k+1} is the composed transform, then the stop test.
 *   sum_r2 f64 [K+1]: leaf 27 of the pass at entry k; 0 for skipped iterations. */
typedef struct md_points_register_plane {
  const float* target_normals; /* f32 [target_rows,3], of the memory kind of reg->target. NULL = the part is off: the call IS the
                                * point-to-point entry on the same arguments, bit for bit, and sum_r2 is not written */
  double* sum_r2;              /* f64 [iterations + 1]. NULL = skip */
} md_points_register_plane;

/* md_op_register_points in the point-to-plane form; plane NULL or plane->target_normals NULL: md_op_register_points on the same
 * arguments, the same launches and bits. Launches: as the operator's, on the plane forms of the step and reduce kernels. Errors,
 * before any launch: the operator's, plus target_normals with reg->target NULL and min_pairs < 6 -> MD_ERR_INVALID_ARG. */
int md_op_register_points_plane(md_device_t dev, const float* xyz_dev, const float* normals_dev, int64_t N, const md_points_register* reg,
                                const md_points_register_plane* plane, float* xyz_out, float* normals_out, void* stream);
/* md_infer_points_register with `plane` behind `reg`: the widest entry. plane NULL or target_normals NULL: md_infer_points_register
 * on the same arguments. The normals are of reg->target_kind: a host target's normals are copied into a grow-only buffer beside
 * the target's with every call (such a call is not captured into a graph), device normals are read by address, so a graph replay
 * sees their current contents. sum_r2 is of out_kind. The graph key contains both fields. Errors as md_infer_points_register's,
 * plus, before any launch: target_normals while the registration is off (reg NULL, radius == 0) or its target NULL, and
 * min_pairs < 6 -> MD_ERR_INVALID_ARG. */
int md_infer_points_register_plane(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                                   const md_points_cameras* cam, const md_view_filter_opts* fo /* NULL = no view filter */,
                                   const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                                   const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                                   const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                                   const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                                   const md_points_clusters* clu, const md_points_match* mat, const md_points_register* reg,
                                   const md_points_register_plane* plane, int out_kind, void* stream);

/* ---- Depth-Anything-v3---------------------------------------------------------------------------------
 * "metric_large" = `DepthAnything3Config::metric_large()` (depth_anything3/mod.rs:153-156): ViT-L/14, 518x518,
 * hooks [4,11,17,23], mono head `DepthAnything3HeadConfig::metric_large` (dpt.rs:41-58).
 * "small" = `DepthAnything3Config::small()` (mod.rs:158-171): ViT-S/14 with QK-norm / 2-D RoPE / camera token /
 * concatenated hooks from block 4 (mod.rs:190-196), hooks [5,7,9,11], dual head (dpt.rs:60-79) and the camera
 * decoder (camera.rs:113-199). "tiny" / "tiny_dual" are test-only reductions of the two (70x70).
 * The model handle is an md_model_t: set/get_tensor, commit, query, timing and destroy work on it unchanged. */
typedef struct md_da3_cfg {
  const char* variant; /* "metric_large" | "small" | "tiny" | "tiny_dual" */
  int image_size;      /* square input side, a multiple of 14; 0 = the variant's native size (518 / 70). Other
                        * sizes interpolate the position embedding bicubically (DINOv2 interpolate_pos_encoding,
                        * offset 0.1) once, when the weights are committed. */
  int precision;       /* md_precision */
  int max_batch;
  float ln_eps;        /* backbone LayerNorm eps (burn_dino's is not visible; default 1e-6) */
  int image_width;     /* 0 = square (image_size x image_size); else the input is image_size rows x image_width columns,
                        * both multiples of 14 -- `DepthAnything3::infer` only asserts divisibility (mod.rs:509-520) */
} md_da3_cfg;
void md_da3_cfg_default(md_da3_cfg* cfg);
/* `DepthAnything3::new(&device, cfg)` (depth_anything3/mod.rs:253-286): seeded synthetic weights. */
int md_da3_create(md_device_t dev, const md_da3_cfg* cfg, uint64_t seed, int init_scheme, md_model_t* out);
/* `DepthAnything3::new(cfg).load_file(path, ..)` (example/correctness.rs:977-982): a Burn `.mpk` record or the engine's
 * safetensors container, as md_depth_pro_load. */
int md_da3_load(md_device_t dev, const md_da3_cfg* cfg, const char* path, md_model_t* out);
/* `DepthAnything3::infer(&self, x)` (depth_anything3/mod.rs:288-291): NCHW fp32 in, depth [B*H*W] out.
 * H and W may be ANY multiples of the patch size (mod.rs:509-520 asserts only that; else MD_ERR_SHAPE). The model keeps
 * per-size tables like the reference's `PosEmbedCache` (dpt.rs:784-833, keyed by shape) and burn_dino's interpolated
 * position embedding: the first call at a new size builds them (host work) and, if the size needs more workspace than any
 * size before it, grows the arena; later calls at that size find everything cached (md_model_query "da3_shape_builds" /
 * "allocs" stop moving). image_size x image_width of the config is just the size the model is prepared for at creation.
 * Up to 16 sizes stay cached (least recently used first out).
 * Numerics across batch sizes: in the 16-bit operand modes (bf16 / f16 / f16x2) a launch that leaves most CUs idle behind a long
 * contraction splits it over wave groups, and a small attention launch splits its keys over two groups (DESIGN.md sections 5.1, 9),
 * so image i of a batch and the same image alone agree to rounding, not to the bit; the fp32 mode and every Depth Pro call are bit-identical across batch sizes. */
int md_da3_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, int out_kind,
                 void* stream);
/* `DepthAnything3Inference` (depth_anything3/mod.rs:231-239) for the dual-head `small` variant. Every pointer
 * except `depth` may be NULL (that output is then not computed). Shapes, fp32, batch-major:
 *   depth, depth_confidence [B,H,W]; aux [B,6,8*H/14,8*W/14] (ray values); aux_confidence [B,8*H/14,8*W/14];
 *   pose_encoding [B,1,9] = (t3 | quat xyzw | fov_h fov_w); extrinsics [B,1,3,4] (world-to-camera);
 *   intrinsics [B,1,3,3] (camera.rs:281-358). The mono variant accepts `depth` only (else MD_ERR_UNSUPPORTED). */
typedef struct md_da3_outputs {
  float* depth;
  float* depth_confidence;
  float* aux;
  float* aux_confidence;
  float* pose_encoding;
  float* extrinsics;
  float* intrinsics;
} md_da3_outputs;
int md_da3_infer_ex(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const md_da3_outputs* out,
                    int out_kind, void* stream);
/* Multi-view inference of the dual-head `small` variant (restated from the public Depth-Anything-3 definition,
 * the reference tree only ever passes one view: parity unpinned). nchw is [B*V, 3, H, W]: B scenes of V views each, scene-major; view 0
 * of a scene is its reference view (no reordering). Patch embedding, the blocks before `ext_block_start` and the local blocks run per
 * view exactly as in md_da3_infer_ex on B*V images. Entering block `ext_block_start`, token 0 of view 0 becomes camera_token[:, 0] and
 * token 0 of views 1 .. V-1 camera_token[:, 1]. In a global block (odd index >= ext_block_start) every query attends over the V * NT
 * tokens of all views of its scene in view order, one softmax over all of them; q/k-norm, RoPE positions, LayerNorm, the linear layers
 * and the hooks stay per token. The head and the camera decoder run per view: every output is [B*V, ...] in (scene, view) order with
 * the per-image shapes of md_da3_outputs. Arithmetic: the mode's operand rounding, fp32 softmax and accumulation, as md_da3_infer_ex.
 * V = 1 is md_da3_infer_ex on the same batch (same launches, same bits). B*V > max_batch -> MD_ERR_SHAPE. With V > 1: the mono-head
 * variant (`metric_large`, no global blocks), the fp32 parity mode (its attention materialises one view's scores) and a call that also
 * carries caller cameras (the camera encoder yields one token per image, not per view) -> MD_ERR_UNSUPPORTED. */
int md_da3_infer_views(md_model_t m, const float* nchw, int B, int V, int H, int W, int in_kind, const md_da3_outputs* out,
                       int out_kind, void* stream);
/* `DepthAnything3::infer_with_camera` (depth_anything3/mod.rs:301-309 -> 522-531): known cameras condition the backbone.
 * extrinsics [B, views, 3, 4] (world-to-camera) and intrinsics [B, views, 3, 3], fp32, in the same memory kind as `nchw`;
 * 1 <= views <= 16. The camera encoder (camera.rs:50-110: pose encoding of each view -> PoseBranch -> token_norm -> a trunk
 * of transformer blocks over the view tokens -> trunk_norm -> mean over views) yields one token per image, which takes the
 * place of the learned camera token in the backbone. A variant without a camera encoder (`metric_large`) ignores the
 * camera inputs, as the reference's match does (mod.rs:522-527), and the call equals md_da3_infer_ex. */
int md_da3_infer_with_camera(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const float* extrinsics,
                             const float* intrinsics, int views, const md_da3_outputs* out, int out_kind, void* stream);
/* `DepthAnything3::infer_raw` (depth_anything3/mod.rs:364-380): logits [B, C, H, W] fp32. Dual head (`small`): C = 2, the main
 * branch's `depth_logits` before the activations (depth = exp(ch 0), confidence = exp(ch 1) + 1; dpt.rs:271,337-354,443-469).
 * Mono head (`metric_large`): C = 1, `forward_raw`'s result (its exp activation applied, dpt.rs:700). */
int md_da3_infer_raw(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* logits, int out_kind, void* stream);
/* `DepthAnything3::infer_from_tokens(patches, height, width)` (depth_anything3/mod.rs:389-469; the head-only comparison of
 * example/da3_small_correctness.rs:278-322): the DPT head alone on caller-supplied hook tokens. tokens[0..3]: the four hooks'
 * `DinoIntermediate::patches`, each [B, tokens_per_image, din] fp32 in the memory kind `in_kind`; din = embed_dim (mono head) or
 * 2 * embed_dim (dual head: cat(local, final-normed)); tokens_per_image = (H/14)*(W/14) patch rows, or one more with a leading row
 * that is skipped (`patch_token_start`, mod.rs:419-424); anything else is MD_ERR_SHAPE. The head applies its own token LayerNorm.
 * No camera prediction (mod.rs:468 passes None): pose_encoding / extrinsics / intrinsics must be NULL (MD_ERR_UNSUPPORTED).
 * The trace the reference returns beside the inference (aux_stage_necks, aux_head_input) is read through the taps. */
int md_da3_infer_from_tokens(md_model_t m, const float* const* tokens, int tokens_per_image, int B, int H, int W, int in_kind,
                             const md_da3_outputs* out, int out_kind, void* stream);
int md_da3_param_inventory(const md_da3_cfg* cfg, int init_scheme, int index, const char** name, size_t* count,
                           float* lo, float* hi);

/* hipGraph replay: with it enabled, an infer call whose (stream, B, H, W, input pointer, output pointers) were seen
 * before is replayed from an instantiated graph of the launch schedule (first call eager, second call captured).
 * Only all-device-memory calls at the configured image size are eligible; timing / tap modes run eagerly. */
int md_model_enable_graph(md_model_t m, int enable);

/* `img_size()` (mod.rs:296), `interpolation_method()` (mod.rs:308) and friends.
 * keys: "img_size", "patch_window", "interpolation", "precision", "max_batch", "num_params",
 *       "workspace_bytes", "weight_bytes", "tiles_per_image", "seq_stride", "is_fork", "forks",
 *       "weight_terms" (MFMA terms per product with a plain weight: 1; MD_PREC_F16X2: 2 = f16-exact weights, 3 otherwise),
 *       "allocs" (device / pinned-host allocations the infer calls of this model have made so far: staging buffers for
 *       host pointers and non-native input sizes grow on demand and are then reused, so the count stops moving once the
 *       largest shapes have been seen), "da3_shape_builds" (Depth-Anything-v3: input sizes whose tables were built),
 *       "decoder_levels", "decoder_features", "decoder_level{0..4}_channels", "decoder_level{0..4}_size" (Depth Pro: the
 *       shapes md_depth_pro_decoder_from_features / md_depth_pro_head_debug take). */
int md_model_query(md_model_t m, const char* key, int64_t* out);

/* Model options. "batch_invariant" (0 | 1, default 0): the reference's `infer` is a pure batch map (the batch is only ever concatenated,
 * layers/encoder.rs:216-225; depth_anything3/mod.rs:495-564) -- an image gives the same tensor alone and inside a batch. Depth Pro models
 * always do (bit for bit, tested). Depth-Anything-v3 models in the 16-bit modes pick two kernel forms by LAUNCH SIZE (the k-split
 * GEMM of small long-K launches and the two-key-group attention of few-workgroup launches, DESIGN.md sections 5.1 / 5.2): deterministic,
 * but another summation order -- the last bits of an image's result can then differ between B = 1 and B = 8. With the option set
 * neither form is used (config 2: ~8 % slower at B = 1) and the batch map is exact. Also a md_model_query key.
 * "ln_fold" (0 | 1 | 2 | 3, default 1; Depth Pro): the LayerNorms between the GEMMs of a ViT block (burn_dino block order, called from
 * /root/reference/src/model/depth_pro/layers/encoder.rs:346-348) run inside those GEMMs instead of as launches (DESIGN.md section
 * 5.1.1): LN(x) W^T + b = rstd (round(gamma x) W^T - mu c) + d. Same values in exact arithmetic; the operand rounding falls on
 * gamma x instead of LN(x). 1 = automatic: on for the 16-bit modes when the ViT is 1024 wide and its sequences have >= 256 tokens
 * (the default configuration); 0 = off (stand-alone LayerNorm launches); 2 = on whenever the model can (MD_ERR_UNSUPPORTED when it
 * cannot: fp32 / fp8 modes, other widths); 3 = a bench diagnostic (the unfolded schedule through the fold-form kernels on neutral
 * statistics). A MODEL-level choice: batch sizes, sequence windows and forks compute the same bits. Set it before md_model_fork (a fork
 * copies its root's setting when it is made) and to the same value on every rank of md_comm_depth_pro_infer_tiles (latency mode at >= 4
 * ranks: 0 is faster there, the windows are too small for the 256 x 256 tiles the fold keeps to). Query keys: "ln_fold", "ln_fold_active". */
int md_model_set_option(md_model_t m, const char* key, int64_t value);

/* Debug taps (EncoderDebug encoder.rs:106-123, HeadDebug mod.rs:135-142, fusion outputs
 * mod.rs:285-287). After an infer, copy the named intermediate (converted to NCHW fp32, the
 * reference's layout) to host memory. `dims` receives up to 4 dims. Names follow
 * example/correctness.rs:98-122: encoder_feature_{0..4}, encoder_merge_latent{0,1},
 * encoder_merge_x{0,1,2}, decoder_fusion_{0..4}, decoder_feature, decoder_lowres_feature,
 * head_conv0, head_deconv, canonical_inverse_depth, fov_deg, split_x{0,1,2}.
 * Pass host_data = NULL to query dims only. Taps must be enabled before the infer.
 * Depth-Anything-v3 models (`DepthTrace` / `infer_with_trace`, depth_anything3/mod.rs:241-246,329-362, and the head's
 * stages, dpt.rs:587-731): backbone_tokens_{0..3} [B, P, D | 2D] (the hook patch tokens the head receives),
 * stage_{0..3} (prepare_stage outputs), layer{1..4}_rn, refinenet{4..1} (+ "_aux" for the dual head's second pyramid),
 * output_conv1, head_input (resized + UV table), aux_neck, aux_head_input; camera_token [B, D] (the camera encoder's
 * result, after md_da3_infer_with_camera). */
int md_model_enable_taps(md_model_t m, int enable);
int md_model_read_tap(md_model_t m, const char* name, float* host_data, size_t capacity, int64_t dims[4]);

/* ---- stand-alone operators on device pointers (the reference's public helpers; used by the
 * parity tests to check each kernel against the oracle) ------------------------------------ */
/* `rgb_to_input_tensor` (src/inference.rs:79-121) on device: u8 HWC -> fp32 NCHW. */
int md_op_rgb_to_input(md_device_t dev, const uint8_t* rgb_dev, size_t rgb_len, int w, int h, float* out_dev,
                       void* stream);
/* `resize_bilinear_align_corners_false(x, [oh,ow], method)` (interpolate.rs:123-134), fp32 NCHW. */
int md_op_resize_bilinear(md_device_t dev, const float* in_dev, int B, int C, int H, int W, float* out_dev,
                          int OH, int OW, int method, void* stream);
/* The same with the post step of the last resize of `DepthPro::infer`: post = 1 writes the final depth
 * 1 / clamp(blend, 1e-4, 1e4) (at equal input and output size: of the input itself); post = 0 is md_op_resize_bilinear. */
int md_op_resize_bilinear_ex(md_device_t dev, const float* in_dev, int B, int C, int H, int W, float* out_dev,
                             int OH, int OW, int method, int post, void* stream);
/* The front of `DepthProEncoder::forward` as the engine runs it (encoder.rs:326-344): pyramid x1 = resize(x, 0.5),
 * x2 = resize(x, 0.25); split(x0, 0.25) | split(x1, 0.5) | x2 concatenated on dim 0 ([35B,3,win,win]); and the ViT's
 * patch extraction, written as the A matrix of the patch-embed GEMM: out[(tile * P + py * g + px)][c * ps^2 + ky * ps + kx]
 * in `precision`'s storage type. x [B,3,S,S] fp32 with S = 4 * window. rows_out / cols_out receive the matrix shape (pass
 * x_dev = out_dev = NULL to query it). force_generic != 0 selects the grid-stride kernel that serves
 * InterpolationMethod::Burn also for Custom (the one-read LDS-staged kernel is the default for Custom, patch 16). A level-0
 * tile stride (floor(0.75 * window)) that is no multiple of 4 is MD_ERR_UNSUPPORTED: level 0 is copied in 16-byte reads. */
int md_op_pyramid_patchify(md_device_t dev, const float* x_dev, int B, int S, int window, int patch, int method, int precision,
                           int force_generic, void* out_dev, int* rows_out, int* cols_out, void* stream);
/* `resize_bilinear(tensor, [oh, ow], _)` of the Depth-Anything-v3 head (depth_anything3/interpolate.rs:7-47) on the
 * engine's NHWC feature-map layout: in [B,H,W,C] -> out [B,OH,OW,C], elements of `precision`'s storage type (bf16 / f16
 * / f32), C a multiple of 8. method MD_INTERP_BURN = align_corners=True (what that head uses), MD_INTERP_CUSTOM = False. */
int md_op_resize_nhwc(md_device_t dev, const void* in_dev, int B, int H, int W, int C, void* out_dev, int OH, int OW,
                      int method, int precision, void* stream);
/* The same launch in the forms the engines give it: pixels of ld_in / ld_out >= C logical channels (multiples of 8; columns
 * C .. ld_out of `out` are not written), an optional fp32 addend table [OH, OW, C] shared by all batch items (NULL: none), and
 * MD_PREC_F16X2 besides bf16 / f16 / f32. Both buffers hold the STORED bytes of `precision`'s storage type; a split-half pixel
 * is [hi: ld | lo: ld]. Ordered on the stream like md_op_resize_nhwc (no synchronisation). ld < C or an unknown method /
 * precision -> MD_ERR_INVALID_ARG; C % 8 != 0 or ld % 8 != 0 -> MD_ERR_UNSUPPORTED. */
int md_op_resize_nhwc_ex(md_device_t dev, const void* in_dev, int B, int H, int W, int C, int ld_in, void* out_dev, int OH, int OW,
                         int ld_out, int method, const float* addend_dev, int precision, void* stream);
/* The frame path's Catmull-Rom taps (pipeline._catmull_rom / _sample_axis, host only): the window [left, left + count) of
 * output `index` of an in_len -> out_len pass and its normalised weights (capacity: count, at most 4 * in_len / out_len + 6;
 * weights may be NULL to query the window). */
int md_catmull_rom_taps(int in_len, int out_len, int index, int* left, int* count, float* weights);
/* The frame path's preparation alone: u8 [B,h,w,3] (device) -> shortest-side Catmull-Rom resize to sw x sh, centre crop at
 * (cx, cy) of size tw x th -> out_u8 [B,th,tw,3] and / or the normalised fp32 NCHW input out_nchw [B,3,th,tw] (either may be
 * NULL). sw = w and sh = h: a pure crop. */
int md_op_resize_catmull_rom(md_device_t dev, const uint8_t* rgb_dev, int B, int h, int w, int sw, int sh, int cx, int cy,
                             int tw, int th, uint8_t* out_u8, float* out_nchw, void* stream);
/* The frame path's display step alone: depth [B,h,w] (device) -> crop (crop_w = 0: the whole map) -> bilinear restore to
 * ow x oh (pipeline.resize_depth_field; the crop's size: no restore) -> MD_FRAME_U8_GRAY / MD_FRAME_RGBA_F32 `out`,
 * range [B,2] (either may be NULL). */
int md_op_depth_display(md_device_t dev, const float* depth_dev, int B, int h, int w, int crop_x, int crop_y, int crop_w,
                        int crop_h, int ow, int oh, int normalize, int format, void* out, float* range, void* stream);
/* `resize_bilinear_scale` (interpolate.rs:136-145): writes the output dims to oh/ow. */
int md_op_resize_output_size(int H, int W, float scale_h, float scale_w, int* oh, int* ow);
/* `DepthProEncoder::split` (encoder.rs:190-232): fp32 NCHW [B,C,S,S] -> [steps^2*B,C,win,win]. */
int md_op_split(md_device_t dev, const float* in_dev, int B, int C, int S, int window, float overlap,
                float* out_dev, int* steps_out, void* stream);
/* `DepthProEncoder::merge` (encoder.rs:234-282): fp32 NCHW tiles -> stitched map. */
int md_op_merge(md_device_t dev, const float* in_dev, int tiles, int C, int h, int w, int batch, int padding,
                float* out_dev, int* out_h, int* out_w, void* stream);
/* LayerNorm over the last dim (burn nn::LayerNorm as used by burn_dino): x[rows,D] fp32 -> fp32. */
int md_op_layernorm(md_device_t dev, const float* x_dev, const float* gamma_dev, const float* beta_dev, int rows,
                    int D, float eps, float* out_dev, void* stream);
/* Linear: out[M,N] = act(x[M,K] @ w[N,K]^T + bias), fp32 in/out; operands rounded per
 * `precision`. act: 0 none, 1 relu, 2 gelu(erf). (burn nn::Linear) */
int md_op_linear(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int M, int N,
                 int K, int act, int precision, float* out_dev, void* stream);
/* Same with an explicit GEMM tile configuration (0 = 256x256, 1 = 128x128, 2 = 256x32, 99 = auto);
 * lets the parity tests and the bench exercise every tile shape. */
int md_op_linear_tile(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int M, int N,
                      int K, int act, int precision, int tile, float* out_dev, void* stream);
/* Multi-head attention core on a fused qkv tensor [T, N, 3*heads*64] (timm layout), fp32 in/out:
 * softmax(q k^T / 8) v -> [T, N, heads*64]. (burn_dino attention, quiet_softmax=false) */
int md_op_attention(md_device_t dev, const float* qkv_dev, int T, int N, int heads, int precision, float* out_dev,
                    void* stream);
/* Cross-view attention (Depth-Anything-v3 global blocks over V views of a scene): the T sequences of
 * qkv [T, N, 3*heads*64] come in groups of V consecutive ones (T % V == 0, else MD_ERR_SHAPE); a query of sequence g*V + i attends
 * over the V*N keys of sequences g*V .. g*V + V-1 taken in that order -- ONE softmax over all of them:
 *   out[g*V+i, n, h*64+d] = sum_{j<V, k<N} softmax_{(j,k)}(q[g*V+i, n, h] . k[g*V+j, k, h] / 8) * v[g*V+j, k, h, d].
 * Same staging, operand rounding and fp32 softmax / accumulation as md_op_attention; bf16, f16 and f16x2 (the fp32 mode returns
 * MD_ERR_UNSUPPORTED for V > 1). V = 1 is md_op_attention: the same launch, the same bits. */
int md_op_attention_views(md_device_t dev, const float* qkv_dev, int T, int V, int N, int heads, int precision, float* out_dev,
                          void* stream);
/* The same entry with every launch parameter in a descriptor (test-only): md_op_attention and md_op_attention_views are this call with
 * seq_stride = kpad = 0, out_fp8_inv = 0, small = -1. */
typedef struct md_attention_op {
  int T, V, N, heads;  /* T sequences in groups of V views (1: single-view), N tokens, head_dim 64 */
  int precision;       /* MD_PREC_*, optionally | MD_OP_POISON_PAD */
  int seq_stride;      /* rows per sequence of the staged q | k and output rows; 0 = N rounded up to 4. < N: MD_ERR_SHAPE */
  int kpad;            /* columns per row of the staged V^T; 0 = N rounded up to 64. Not a multiple of 64 covering N: MD_ERR_INVALID_ARG */
  float out_fp8_inv;   /* > 0: the e4m3-output form (bf16, V = 1; else MD_ERR_UNSUPPORTED): out = uint8 [T, N, heads*64], the OCP e4m3 bytes of
                        * clamp(value * out_fp8_inv, +-448) */
  int small;           /* -1: the launcher's own rule for the small-launch (key-split) form; 0: that form off for this call */
  int poison_pad;      /* != 0: as MD_OP_POISON_PAD -- rows N .. seq_stride, the slack rows and the V^T columns N .. kpad hold 0x7000 */
  const float* qkv;    /* [T, N, 3*heads*64] fp32 (timm layout) */
  void* out;           /* fp32 [T, N, heads*64], or the e4m3 bytes (see out_fp8_inv) */
} md_attention_op;
int md_op_attention_ex(md_device_t dev, const md_attention_op* desc, void* stream);
/* Host-only: the form the calling thread's last attention launch took -- out[4] = form, workgroups of the main launch, query waves and
 * key groups per workgroup. md_op_attention_ex resets it to MD_ATTN_FORM_NONE before it launches. */
typedef enum md_attention_form {
  MD_ATTN_FORM_NONE = -1, MD_ATTN_FORM_PLAIN = 0, MD_ATTN_FORM_KEY_SPLIT = 1, MD_ATTN_FORM_ASSEMBLY = 2, MD_ATTN_FORM_VIEWS = 3,
  MD_ATTN_FORM_FP8_OUT = 4, MD_ATTN_FORM_F32_PATH = 5
} md_attention_form;
int md_debug_attention_last_form(int out[4]);
/* Conv2d 3x3 stride 1 pad 1 (burn nn::Conv2d): fp32 NCHW in/out, w [Cout,Cin,3,3]. */
int md_op_conv3x3(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B, int Cin,
                  int H, int W, int Cout, int pre_relu, int precision, float* out_dev, void* stream);
/* ConvTranspose2d k=2 s=2 (burn nn::ConvTranspose2d): fp32 NCHW, w [Cin,Cout,2,2]. */
int md_op_deconv2x2(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B, int Cin,
                    int H, int W, int Cout, int precision, float* out_dev, void* stream);
/* Generic small Conv2d (any k/stride/pad), fp32 exact; the FOV head path (fov.rs:16-49). */
int md_op_conv2d_direct(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B,
                        int Cin, int H, int W, int Cout, int k, int stride, int pad, int relu, float* out_dev,
                        void* stream);
/* ---- the Depth-Anything-v3 token kernels alone (test-only). fp32 device tensors in and out; rows pass through `precision`'s
 * storage type (MD_PREC_BF16 / F32 / F16 / F16X2) exactly as the engine holds them. RoPE tables: the model's own function, for
 * the grid ph x pw with ph = (n_tokens - 1) / pw. ---- */
/* The QKV projection with the per-head q/k LayerNorm(64) + 2-D RoPE: x [T*S, K], w [3D, K], bias [3D], gammas / betas [64];
 * token t = row % S sits at (0, 0) for t == 0 or t >= n_tokens, else at patch (1 + (t-1) / pw, 1 + (t-1) % pw), or at (1, 1)
 * when global_pos. form 0: the plain QKV GEMM followed by the stand-alone q/k-norm + RoPE kernel (rows t >= n_tokens keep
 * the GEMM's plain q | k); form 1: the GEMM's fused epilogue. tile: 3 = 128x64, 4 = 64x64, 99 = auto; a tile the fused
 * epilogue cannot take is MD_ERR_UNSUPPORTED. qk_out [T*S, 2D] = q' | k' (q' carries the softmax scale of the mode),
 * vt_out [T, D/64, 64, kpad] = V^T as the epilogue lays it out, kpad = S rounded up to 64. */
int md_op_qkv_norm_rope(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, const float* q_gamma,
                        const float* q_beta, const float* k_gamma, const float* k_beta, int T, int S, int n_tokens, int K, int D,
                        int pw, int global_pos, float rope_frequency, float eps, int precision, int tile, int form,
                        float* qk_out, float* vt_out, void* stream);
/* The stand-alone q/k-norm + RoPE kernel on caller rows qk_in [T*S, 2D] = q | k -> qk_out (rows t >= n_tokens untouched). */
int md_op_qk_norm_rope(md_device_t dev, const float* qk_in, const float* q_gamma, const float* q_beta, const float* k_gamma,
                       const float* k_beta, int T, int S, int n_tokens, int D, int pw, int global_pos, float rope_frequency,
                       float eps, int precision, float* qk_out, void* stream);
/* hook = LayerNorm_head(cat(x_local, LayerNorm_final(x))): x_local, x [T*S, D] -> out [T*S, 2D], updated in place (rows
 * t >= n_tokens keep the caller's values); cam_out [T, 2D] = the raw token-0 concat, may be NULL. */
int md_op_hook_cat_ln(md_device_t dev, const float* x_local, const float* x, int T, int S, int n_tokens, int D,
                      const float* norm_g, const float* norm_b, float eps_final, const float* head_g, const float* head_b,
                      float eps_head, int precision, float* out, float* cam_out, void* stream);
/* Generic patch extraction: x [B,3,H,W] -> out [B * (H/ps) * (W/ps), Kp] (Kp >= 3 ps^2, tail zero). cls_x != NULL: the same
 * launch writes cls + pos0 to row 0 and zeroes rows n_tokens .. S-1 of every sequence of cls_x [B*S, D] (in place). */
int md_op_patchify(md_device_t dev, const float* x_dev, int B, int H, int W, int ps, int Kp, int precision, float* out,
                   float* cls_x, int S, int n_tokens, int D, const float* cls, const float* pos0, void* stream);
/* x[b*S, :] = src[b * src_stride, 0:D] for every sequence of x [nseq*S, D] (in place). */
int md_op_set_token0(md_device_t dev, float* x, int nseq, int S, int D, const float* src, int src_stride, void* stream);
/* Adds bias9[class] - bias9[4] to the border pixels of the NHWC map [B,H,W,ld] (columns 0 .. C-1; in place), bias9 [9, C]. */
int md_op_border_bias_fix(md_device_t dev, float* map, int B, int H, int W, int C, int ld, const float* bias9, int precision,
                          void* stream);
/* ---- the layer compositions of the commit alone (test-only): two layers with nothing between them are packed as ONE layer on the
 * product of their fp32 weights; this entry runs the commit's own composition launches on fp32 device tensors of the CALLER and
 * returns the fp32 product before it is rounded and packed. cin -> cmid -> cout are the channels of the first and second layer.
 *   DECONV_CONV  w_first [cin, cmid, 2, 2] (ConvTranspose2d k2 s2, no bias), w_second [cout, cmid] (Conv2d 1x1)
 *                -> out [cin, cout, 2, 2], one k2 s2 deconvolution. The 1x1's bias is NOT composed: the deconvolution in front of it
 *                has no bias, so W2 (deconv(x)) + b2 = deconv'(x) + b2 on every output pixel, and the engine hands b2 [cout] unchanged
 *                to the pixel-shuffle launch as its bias (one value per output channel, the same for the four parities).
 *   DECONV_PAIR  w_first [cin, cmid, 2, 2], w_second [cmid, cout, 2, 2] (both ConvTranspose2d k2 s2, no bias)
 *                -> out [cin, cout, 4, 4], one k4 s4 deconvolution, tap (2 dy1 + dy2, 2 dx1 + dx2).
 *   C1C3         w_first [cmid, cin] (Conv2d 1x1, bias_first [cmid]), w_second [cout, cmid, 3, 3] (Conv2d 3x3 pad 1, bias_second [cout])
 *                -> out [cout, cin, 3, 3]; bias9_out [9, cout].
 *   HEAD         w_first [cin, cmid, 2, 2] (ConvTranspose2d k2 s2, bias_first [cmid]), w_second [cout, cmid, 3, 3] (Conv2d 3x3 pad 1,
 *                bias_second [cout]) -> out [4 cout, cin, 3, 3] on the deconvolution's input grid, column group 2 py + px = the output
 *                pixel's parity; bias9_out [9, cout].
 * bias9_out[3 ry + rx] = bias_second + the first layer's bias through the taps of the 3x3 that lie inside the map at an output pixel of
 * row class ry (0 first row, 1 interior, 2 last row) and column class rx. bias_first, bias_second and bias9_out come all three or not at
 * all (the weight alone). Refused before any launch, MD_ERR_INVALID_ARG unless noted: a null weight or `out`; an unknown kind; a channel
 * count <= 0 (MD_ERR_SHAPE); any bias pointer with DECONV_CONV or DECONV_PAIR; one or two of the three bias pointers. ---- */
typedef enum md_compose_kind { MD_COMPOSE_DECONV_CONV = 0, MD_COMPOSE_DECONV_PAIR = 1, MD_COMPOSE_C1C3 = 2, MD_COMPOSE_HEAD = 3 } md_compose_kind;
int md_op_compose_weights(md_device_t dev, int kind, int cin, int cmid, int cout, const float* w_first, const float* w_second,
                          const float* bias_first, const float* bias_second, float* out, float* bias9_out, void* stream);
/* ---- the kernels that write MFMA operands, alone (test-only). Every output buffer is the caller's device memory and receives the
 * STORED bytes of `precision`'s storage type -- bf16, f16, fp32, split-half rows [hi: width | lo: width] of f16, e4m3 bytes --, no
 * widened copy, so a test can compare roundings bit for bit. Each call synchronises its stream before it returns. ---- */
/* The engine's LayerNorm launch: x [rows, D] fp32, sequences of S rows, `ngroups` (1..4) consecutive sequence ranges
 * [seq0[i], seq0[i] + nseq[i]) with their own gamma[i] / beta[i] (host arrays of device pointers; gamma[i] NULL = non-affine).
 * out: rows of `precision` (MD_PREC_FP8: e4m3 bytes of value * fp8_inv_scale, saturating), or fp32 when out_f32. tok0 != NULL: row 0 of
 * every sequence is first replaced by tok0[seq * tok0_stride .. + D] and written back into x. D % 4 != 0 or D > 1024 -> MD_ERR_UNSUPPORTED. */
int md_op_layernorm_ex(md_device_t dev, float* x, int rows, int D, int S, int ngroups, const int* seq0, const int* nseq,
                       const float* const* gamma, const float* const* beta, float eps, int precision, int out_f32, float fp8_inv_scale,
                       const float* tok0, int tok0_stride, void* out, void* stream);
/* fp32 [count] -> storage rows (width = logical row width; MD_PREC_F16X2 needs it and count % width == 0), and back. */
int md_op_store_rows(md_device_t dev, const float* in, int64_t count, int width, int precision, void* out, void* stream);
int md_op_load_rows(md_device_t dev, const void* in, int64_t count, int width, int precision, float* out, void* stream);
/* out[i] = e4m3(clamp(in[i] * inv_scale, +-448)); count % 4 == 0. */
int md_op_f32_to_fp8(md_device_t dev, const float* in, int64_t count, float inv_scale, void* out, void* stream);
/* w [N, K] fp32 -> e4m3 [N, Kp] (columns K .. Kp zero; Kp % 4 == 0) and scale [N] = amax_n / 448 (1 for an all-zero row). */
int md_op_pack_fp8_rows(md_device_t dev, const float* w, int N, int K, int Kp, void* out, float* scale, void* stream);
/* fp32 NCHW -> storage NHWC with `ld` logical elements per pixel (0 = C; split-half pixels are [hi: ld | lo: ld]); columns C .. ld of
 * `out` are not written. relu: max(v, 0) first. */
int md_op_nchw_to_nhwc(md_device_t dev, const float* in, int B, int C, int H, int W, int precision, int relu, int ld, void* out,
                       void* stream);
/* storage NHWC with `ld` elements per pixel, channels coff .. coff + C -> fp32 NCHW [B, C, H, W]. */
int md_op_nhwc_to_nchw(md_device_t dev, const void* in, int B, int C, int H, int W, int ld, int coff, int precision, float* out,
                       void* stream);
/* The vectors of a LayerNorm folded into the linear layer behind it: c[n] = sum_k gamma[k] Wr[n][k], d[n] = bias[n] + sum_k beta[k] Wr[n][k],
 * Wr = w [N, K] as `precision`'s operand holds it; bias may be NULL. */
int md_op_ln_fold_vectors(md_device_t dev, const float* w, const float* gamma, const float* beta, const float* bias, int N, int K,
                          int precision, float* c, float* d, void* stream);
/* parts [rows][4][2] = (mean, centred sum of squares) of four 256-column tiles -> ab [rows][2] = (rstd, -mu * rstd). */
int md_op_ln_finish(md_device_t dev, const float* parts, int64_t rows, float inv_n, float eps, float* ab, void* stream);
/* ---- the GEMM forms of the ViT token stream alone (test-only): the residual + LayerScale update of proj / fc2 (with the LayerNorm
 * fold's producer part), the QKV projection and fc1's GELU store (with the fold's consumer part), the patch embedding. Every tensor is
 * an fp32 device tensor; operands are staged into `precision`'s storage type as md_op_linear_tile stages them (split-half: two or three
 * terms by the weights; e4m3: activations on the scale 8/448, weights per row), storage-typed results are widened back. The entry
 * pre-fills NOTHING: every output buffer is the caller's, a storage-typed one is first narrowed from the caller's values (which must
 * be exact in the type) and widened back behind the launch, so bytes the launch leaves alone come back as they went in. ---- */
typedef enum md_vit_gemm_kind { MD_VIT_GEMM_RESID = 0, MD_VIT_GEMM_QKV = 1, MD_VIT_GEMM_FC1 = 2, MD_VIT_GEMM_PATCH_EMBED = 3 } md_vit_gemm_kind;
typedef struct md_vit_gemm_group {
  int row0, rows, arow0;   /* first output row, rows, first A row (groups may alias A rows) */
  const float* w;          /* [N, K] */
  const float* bias;       /* [N]; fold consumer: d */
  const float* scale;      /* RESID: LayerScale [N] */
  const float* gamma_next; /* RESID, optional (all groups or none): the fold's producer part */
  const float* c;          /* QKV / FC1, optional (all groups or none): the fold's consumer part */
  const float* pos;        /* PATCH_EMBED: [1 + P, N] */
} md_vit_gemm_group;
typedef struct md_vit_gemm {
  int kind, precision, tile;
  int N, K;                /* QKV: N = 3 D */
  int a_rows;              /* rows of a */
  const float* a;          /* [a_rows, K] */
  int ngroups;             /* 1 .. 4 */
  md_vit_gemm_group g[4];
  int out_rows;            /* rows of every output below */
  float* x;                /* RESID: [out_rows, N] in/out (read only when x_out is set); PATCH_EMBED: [nseq * S, N] in/out */
  float* x_out;            /* RESID, optional: the out-of-place form's output */
  float* ln_out;           /* RESID producer: [out_rows, N] = gamma_next . x_new in the storage type */
  float* ln_stats_out;     /* RESID producer: [out_rows, N / 256, 2] (mean, centred sum of squares) per 256-column tile */
  const float* ln_stats;   /* consumer: ln_raw 1: [out_rows, 4, 2] partials; 0: [out_rows, 2] (rstd, -mu rstd) */
  int ln_raw;
  float ln_eps, ln_inv_n;
  int S, D;                /* QKV: rows per sequence (out_rows = T * S), embedding; PATCH_EMBED: S = rows per sequence of x */
  int P;                   /* PATCH_EMBED: patches per sequence */
  float* qk;               /* QKV: [out_rows, 2 D] = q * attn_qscale | k */
  float* vT;               /* QKV: [T, D / 64, 64, kpad], kpad = S rounded up to 64 */
  float* out;              /* FC1: [out_rows, N] = gelu(..) in the storage type */
} md_vit_gemm;
int md_op_vit_gemm(md_device_t dev, const md_vit_gemm* desc, void* stream);
/* Host-only: what the calling thread's last launch of the 256 x 256 GEMM family ran -- out[8] = family (0 one tile per workgroup,
 * 1 the fc1 / QKV / lean-convolution tile loop, 2 the read-modify-write tile loop; -1: md_op_vit_gemm launched another tile), epilogue kind
 * (the one-tile kernel's EK; for a loop the kind it replaces), fold, qkv, conv, diag, tiles, workgroups. */
int md_debug_gemm_last_form(int out[8]);
/* Host-only: what the calling thread's last GEMM launch through md_op_vit_gemm / md_op_decoder_gemm resolved, whichever kernel of the
 * family took it -- out[4] = tile (0 = 256x256, 1 = 128x128, 2 = 256x32, 3 = 128x64, 4 = 64x64; -1: no launch), the launcher-set fast
 * form of the pixel shuffle (16-byte stores of whole 8-column groups), the contraction length K of the launch (split-half operands:
 * the padded channels -- times 9 for a 3x3 convolution -- times the two or three terms of the weight), 0. */
int md_debug_gemm_last_launch(int out[4]);
/* ---- the GEMM forms of the convolutional decoders and heads alone (test-only): one launch of the GEMM family with the parameters the
 * engines' call sites give it, on buffers the CALLER owns. Activations, residual inputs and T-typed outputs are raw device tensors of
 * `precision`'s storage type in the engine's layout: NHWC pixels of `ld` logical channels, split-half pixels [hi: ld | lo: ld]
 * (md_op_nchw_to_nhwc / md_op_store_rows write them, md_op_load_rows / md_op_nhwc_to_nchw read them); fp32 outputs are float tensors.
 * Weights and biases are fp32 masters, packed per call as the engine packs them at commit (split-half: two terms when every weight
 * of the launch is an exact half, else three; the composed head weight always three). The entry allocates no output and pre-fills
 * nothing; it launches and synchronises. MD_PREC_BF16 / F16 / F16X2 / F32; anything else is MD_ERR_INVALID_ARG. ---- */
typedef enum md_decoder_gemm_kind {
  MD_DECODER_GEMM_CONV3 = 0,    /* 3x3 s1 p1, EPI_STORE: out = act(conv + bias + res1 + res2), out2 = relu(out); 1 or 2 weight groups */
  MD_DECODER_GEMM_CONV3_S2 = 1, /* 3x3 s2 p1, EPI_STORE: T-typed NHWC output, or (out_f32) fp32 rows of Cout with a ReLU */
  MD_DECODER_GEMM_PIXSHUF = 2,  /* ConvTranspose2d k = s = f (2 or 4) into channels [ps_coff, ps_coff + Cout) of NHWC pixels of ldo */
  MD_DECODER_GEMM_HEAD = 3,     /* 3x3 s1 p1 to 32 channels -> relu -> 1x1 to head_nch channels (0: one, `head_w`) -> act, fp32 planes */
  MD_DECODER_GEMM_HEAD_UP2 = 4  /* deconv k2s2 -> conv 3x3 to 32 -> relu -> 1x1 -> relu composed into one launch, fp32 [B, 2H, 2W] */
} md_decoder_gemm_kind;
typedef struct md_decoder_gemm_head_ch {
  const float* w; /* [32] */
  float b;
  int act;        /* 0 relu, 1 exp, 2 linear, 3 exp + 1 */
  float* out;     /* pixel (img, y, x) at out[img * bstride + y * W + x] */
  int64_t bstride;
} md_decoder_gemm_head_ch;
typedef struct md_decoder_gemm {
  int kind, precision, tile; /* tile: 99 = the launcher's choice, else 0 .. 4 as md_debug_gemm_last_launch names them */
  int B, H, W;               /* input pixel grid of ONE weight group */
  int Cin, Cin_p;            /* weight input channels; logical channels per input pixel (the contraction runs over all Cin_p, weights zero-padded) */
  int Cout;                  /* HEAD / HEAD_UP2: 32 */
  int ngroups;               /* CONV3: 1 or 2 -- group g = weights g on images [g B, (g + 1) B) of out / out2 / res2 */
  int in_shared, res1_shared;/* CONV3, two groups: both read images [0, B) of in / of res1 (else group g reads its own images) */
  const float* w[2];         /* CONV3*, HEAD: [Cout, Cin, 3, 3]; PIXSHUF: [Cin, Cout, f, f]; HEAD_UP2: the deconvolution [Cin, Cmid, 2, 2] */
  const float* bias[2];      /* [Cout]; may be NULL for CONV3; HEAD_UP2: the deconvolution's [Cmid] */
  const void* in;            /* [images, H, W, Cin_p] T */
  int act;                   /* CONV3: 0 none, 1 relu */
  const void* res1;          /* CONV3, optional: [.., OH, OW, ldo] T */
  const void* res2;
  int res_mod;               /* CONV3, one group, > 0: res1 row = m % res_mod (a table the images share) */
  void* out;                 /* T: [images, OH, OW, ldo]; out_f32: float [M, Cout]; HEAD: one-channel plane float [M]; HEAD_UP2: float [B, 2H, 2W] */
  void* out2;                /* CONV3 / PIXSHUF, optional: relu(out), same layout */
  int ldo;                   /* logical channels per output pixel */
  int out_f32;               /* CONV3_S2: the fp32 form (ldo = Cout) */
  int ps_f, ps_coff;         /* PIXSHUF */
  int head_nch;              /* HEAD: 0 = the one-channel form (head_w, head_b, head_act, out), else 1 .. 8 channels `ch` in one launch */
  md_decoder_gemm_head_ch ch[8];
  const float* head_w;       /* HEAD one-channel form, HEAD_UP2: [32] */
  float head_b;
  int head_act;              /* HEAD one-channel form */
  int Cmid;                  /* HEAD_UP2: channels between the deconvolution and the 3x3 convolution */
  const float* w2;           /* HEAD_UP2: the 3x3 convolution [32, Cmid, 3, 3] */
  const float* bias2;        /* HEAD_UP2: [32] */
} md_decoder_gemm;
int md_op_decoder_gemm(md_device_t dev, const md_decoder_gemm* desc, void* stream);
/* ---- the gathered-row GEMM forms alone (test-only): logical row m of A reads physical row index[m], as the Depth Pro encoder tail
 * (enc_proj, the low-resolution deconvolution, fov_proj) and the Depth-Anything-v3 stage projection launch it, with the engines' own
 * launch-parameter builders. Every tensor is the CALLER's fp32 device tensor: `a`, `w`, `res1` are narrowed to `precision`'s storage
 * per call (weights packed as at commit; split-half: two terms when every weight is an exact half, else three); a T-typed `out` is
 * narrowed before and widened behind the launch, so what the launch leaves alone returns bit for bit when it is exact in the type.
 * `index` is copied to the host and every entry must lie in [0, rows_a): MD_ERR_INVALID_ARG otherwise, before any launch.
 * index == NULL: the same parameters as a dense launch over a [M, K]. MD_PREC_BF16 / F16 / F16X2 / F32. ---- */
typedef enum md_indexed_gemm_kind {
  MD_INDEXED_GEMM_ROWS = 0,     /* out[m, :N] = a[index[m]] . w^T + bias; bias may be NULL; T-typed rows of ldo, or (out_f32) fp32 */
  MD_INDEXED_GEMM_ROWS_RES = 1, /* ROWS + res1[m % res_mod], a T-typed table [res_mod, ldo]; T-typed output */
  MD_INDEXED_GEMM_PIXSHUF = 2   /* ConvTranspose2d k = s = ps_f of the gathered [B, ph, pw] map into channels [ps_coff, ps_coff + N) */
} md_indexed_gemm_kind;
typedef struct md_indexed_gemm {
  int kind, precision, tile; /* tile: 99 = the launcher's choice, else 0 .. 4 as md_debug_gemm_last_launch names them */
  int M, N, K;               /* logical rows; output channels (PIXSHUF: of one pixel); contraction = row width of a */
  int rows_a;                /* rows of a */
  const float* a;            /* [rows_a, K]; index == NULL: [M, K] */
  const int32_t* index;      /* [M] device, or NULL */
  const float* w;            /* ROWS*: [N, K]; PIXSHUF: [K, N, ps_f, ps_f] */
  const float* bias;         /* [N]; ROWS: may be NULL */
  const float* res1;         /* ROWS_RES: [res_mod, ldo] */
  int res_mod;
  float* out;                /* [out_rows, ldo]; PIXSHUF: pixels [B, ps_f ph, ps_f pw] of ldo */
  int64_t out_rows;          /* rows of out the caller owns, >= the launch's */
  int ldo, out_f32;          /* logical channels per output row; ROWS: the fp32 store */
  int B, ph, pw;             /* PIXSHUF: M = B ph pw */
  int ps_f, ps_coff;         /* PIXSHUF: 2 | 4; first channel of the slice */
} md_indexed_gemm;
int md_op_indexed_gemm(md_device_t dev, const md_indexed_gemm* desc, void* stream);
/* Host-only, no device: the gather tables of the Depth Pro encoder tail. md_op_merge_index_table: the merged map of a g x g token grid
 * split into steps x steps tiles with `pad` halo tokens (the reference's merge as a gather) -- entry ((b Y) X) of the [B, E, E] map, E =
 * steps (g - 2 pad) + 2 pad (steps == 1: g), is the token row (seq0 + (j steps + i) B + b) SS + 1 + ty g + tx of sequences of SS rows.
 * md_op_token_index_table: entry b P + p = (seq0 + b) SS + 1 + p, the patch rows of B whole sequences. Both return the number of
 * entries (negative: an error code); out == NULL returns the count only, else capacity must hold it. */
int md_op_merge_index_table(int B, int g, int steps, int pad, int SS, int seq0, int32_t* out, int64_t capacity);
int md_op_token_index_table(int B, int P, int SS, int seq0, int32_t* out, int64_t capacity);
/* ---- the Depth-Anything-v3 camera path alone (test-only): the camera encoder, the camera decoder and the pose -> matrices tail as the
 * engine launches them, on fp32 device tensors the CALLER owns. The entries allocate only the launchers' scratch, pre-fill nothing,
 * launch and synchronise. What a launcher refuses (views outside 1..16, width % 8, width % heads, depth outside 0..8; decoder width % 4,
 * batch < 1) returns with the launcher's code before any device work. ---- */
typedef struct md_camera_encode {
  int B, V, D, heads, depth; /* images, views per image (1..16), token width, attention heads, trunk blocks (0..8) */
  int H, W;                  /* image size the intrinsics refer to */
  float eps_tok, eps_blk;    /* LayerNorm eps of token_norm / trunk_norm, and of the blocks' norm1 / norm2 */
  const float* w[8];         /* pose_branch fc1 [D/2, 9], its bias, fc2 [D, D/2], its bias, token_norm gamma, beta, trunk_norm gamma, beta */
  const float* blk[8][14];   /* block i: norm1 gamma, beta, norm2 gamma, beta, qkv [3D, D], bias, proj [D, D], bias, ls1, fc1 [4D, D], bias,
                              * fc2 [D, 4D], bias, ls2 */
  const float* extr;         /* [B, V, 3, 4] world-to-camera */
  const float* intr;         /* [B, V, 3, 3] */
  float* out;                /* [B, D] */
  float* pose_out;           /* optional [B, V, 9]: the pose encoding the kernel fed to pose_branch (t3 | quat xyzw | fov_h fov_w) */
} md_camera_encode;
int md_op_camera_encode(md_device_t dev, const md_camera_encode* desc, void* stream);
typedef struct md_camera_decode {
  int B, din, H, W;
  const float* cam;   /* [B, din] */
  const float* w[10]; /* backbone_1 [din, din], bias, backbone_2 [din, din], bias, fc_t [3, din], bias, fc_qvec [4, din], bias, fc_fov [2, din], bias */
  float* pose;        /* [B, 9] */
  float* extr;        /* optional [B, 12] world-to-camera */
  float* intr;        /* optional [B, 9] */
} md_camera_decode;
int md_op_camera_decode(md_device_t dev, const md_camera_decode* desc, void* stream);
/* pose [B, 9] -> extr [B, 12] world-to-camera, intr [B, 9]; either output may be NULL. The same device function as the decoder's tail. */
int md_op_pose_to_camera(md_device_t dev, const float* pose, int B, int H, int W, float* extr, float* intr, void* stream);
/* md_op_conv2d_direct as the FOV head runs it: the input held in `in_precision`'s storage type, add = optional fp32 NHWC tensor added
 * to the input, out = fp32 NHWC [B, OH, OW, out_ld] (out_ld 0 = Cout; columns Cout .. out_ld are not written). */
int md_op_conv2d_direct_ex(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, const float* add_dev, int B,
                           int Cin, int H, int W, int Cout, int k, int stride, int pad, int relu, int in_precision, int out_ld,
                           float* out_dev, void* stream);
/* `fovy_from_fovx_rad` (mod.rs:370-414) + focal length (mod.rs:330-336) on host scalars. */
int md_op_fov_to_focal(float fovx_deg, int H, int W, float* focal_px, float* fovy_rad);
/* The reverse, on host scalars: a focal length f_px (pixels of the W-wide image) -> fovx_deg = 2 atan(W / (2 f_px)) in
 * degrees and fovy_rad through `fovy_from_fovx_rad` (what md_depth_pro_infer_with_focal returns). f_px not finite or
 * not > 0 -> MD_ERR_INVALID_ARG. */
int md_op_focal_to_fov(float f_px, int H, int W, float* fovx_deg, float* fovy_rad);

/* Kernel micro-benchmark: times `iters` launches of the GEMM kernel (random bf16/f32 operands resident
 * in HBM, plain store epilogue, out element = operand type) with HIP events on the launch stream and
 * returns the average milliseconds per launch. mode: 0 dense GEMM [M,K]x[N,K]^T; 1 conv3x3 over an
 * NHWC [1,H,W,K] image with M = H*W (pass H in `aux0`, W in `aux1`), N = Cout.
 * Timing-only ablation flags ride in `tile >> 8` (results are then meaningless): 1 no in-loop global loads, 2 every
 * k-tile re-reads k-tile 0, 4 bias + GELU epilogue (fc1), 8 pixel-shuffle epilogue of a k2s2 deconvolution (mode 0:
 * `aux0` x `aux1` = input pixel grid, N = 4*Cout), 16 fp32 read-modify-write epilogue (proj / fc2), 32 per-workgroup
 * phase stamps of one launch printed to stderr (s_memrealtime at seven points + shader clock around the main loop),
 * 64 no global stores, 128 no staging writes. tools/kernel_bench.py names the combinations. */
int md_bench_gemm(md_device_t dev, int mode, int M, int N, int K, int aux0, int aux1, int precision, int tile, int iters,
                  float* avg_ms);
/* Host-only diagnostic (no GPU work): the tile the engine's launch cost model picks for a dense [M,K] x [N,K]^T GEMM in
 * `precision` -- 0 = 256x256, 1 = 128x128, 2 = 256x32 (N <= 32), 3 = 128x64, 4 = 64x64. */
int md_gemm_pick_tile(int M, int N, int K, int precision);
/* Host-only diagnostic: launches of the 64 x 64 GEMM kernel that split their contraction over wave groups inside the workgroup
 * (gemm_kernel's KSPLIT) since the library was loaded (modulo 2^31) -- lets a test check that the form it
 * means to exercise actually ran. */
int md_gemm_ksplit_launches(void);
/* PROCESS-WIDE A/B switch (default 1; returns the previous value): may the lean 2-byte store epilogues of the 256 x 256 GEMM kernel
 * (fc1, the q | k tiles of qkv, convolutions without residual inputs) store straight from the accumulator layout -- the W tile's
 * LDS image in a permuted row order, one 16-byte store per lane and (m-block, column half) -- instead of staging the tile through
 * LDS? Same values, same bits; for benches and the bit-identity test. Graphs captured before a change keep
 * their form. */
int md_debug_gemm_direct_store(int on);
/* PROCESS-WIDE A/B switch (a mask, default 15; returns the previous value): which launches of the 256 x 256 GEMM kernel with >= 1024 tiles (the QKV projection: 768)
 * may run as a persistent tile loop -- one workgroup per CU, the next tile's first k-tile requested before the current tile's epilogue
 * (DESIGN.md section 5.1.2): 1 = the fc1 form (dense A, bias (+ LayerNorm fold) + GELU, direct stores: gemm256p_kernel), 2 = the fused
 * QKV projection (one-plane types), 4 = the read-modify-write GEMMs proj / fc2 (gemm256r_kernel), 8 = the implicit 3 x 3 GEMMs of the decoder's residual units (bias; with or without residual
 * inputs / a relu'd second output). Same arithmetic, same bits. */
int md_debug_gemm_persistent(int mask);
/* Timing switch of the tile loops: half of every XCD's workgroups start `ticks` (10 ns each) after the other half, so that one half's
 * epilogues (proj / fc2: the fp32 residual stream's read + write, HBM-bound) meet the other half's main loops instead of each other.
 * which: 0 the read-modify-write loop at <= 16 k-tiles per tile (proj; default 2000), 1 the same at more (fc2; 0), 2 the fc1 loop (0),
 * 3 the QKV loop (0). Same bits. MD_ERR_INVALID_ARG for another `which` or negative ticks. */
int md_debug_gemm_stagger(int which, int ticks);
/* The value in force for `which` (so that a test restores what it found); MD_ERR_INVALID_ARG (< 0) for another `which`. */
int md_debug_gemm_stagger_ticks(int which);
/* Same for the fused bf16 attention kernel: T sequences of n_tokens, `heads` heads of 64. */
int md_bench_attention(md_device_t dev, int T, int n_tokens, int heads, int iters, float* avg_ms);
/* The same with the operand type (MD_PREC_BF16 | MD_PREC_F16) and the range of the random q / k values, uniform in
 * +-qk_scale (q is taken as already carrying the softmax scale): 0.7 gives logits of a few units (the bf16 kernel's fast
 * body), 4.0 and above logits beyond its +-32 check (the running-maximum body). */
int md_bench_attention_ex(md_device_t dev, int T, int n_tokens, int heads, int precision, float qk_scale, int iters,
                          float* avg_ms);
/* The same on CALLER-supplied operands: qkv_dev = [T, n_tokens, 3 * heads * 64] fp32 on the device, rows q | k | v as the fused QKV
 * projection of /root/reference/src/model/depth_pro/layers/vit.rs:45-68 (burn_dino's attention) produces them; q is scaled by
 * 1/sqrt(64) inside. *redo_units_per_launch (may be NULL) = the (sequence, head) units per launch whose row sums left the assembly
 * kernel's fast range and were recomputed by the running-maximum body (-1: the assembly kernel is not in use). For stress operands
 * with outlier logits (plain softmax, vit.rs:60: outliers are legal inputs). */
int md_bench_attention_qkv(md_device_t dev, const float* qkv_dev, int T, int n_tokens, int heads, int precision, int iters,
                           float* avg_ms, long* redo_units_per_launch);
/* PROCESS-WIDE (round 5: per host thread): may bf16 attention launches of exactly 577 tokens (Depth Pro: 576 patches + the class
 * token) take the assembly-owned gfx950 kernel (kernels/attn577_gfx950.s)? Default 1; returns the previous value. 0 runs the HIP
 * kernel that every other shape runs -- an A/B switch for benches and parity tests, not a numerics option: both forms compute the
 * same sums (the assembly kernel adds the rounded probabilities on the matrix pipe). Graphs captured before a change keep their form. */
int md_debug_attention_asm(int on);
/* Launches of the assembly-owned attention kernel since the library was loaded: what a bench line may say about the form it timed. */
long md_debug_attention_asm_launches(void);
/* (sequence, head) units the assembly kernel flagged for the running-maximum body on `dev` since the last reset (reset != 0 clears
 * the counter). Synchronises the device. -1: the code object is not loaded there. 0 over a whole run = the fast body served every unit. */
long md_debug_attention_redo_units(md_device_t dev, int reset);

/* ---- multi-GPU: RCCL over xGMI behind the C ABI ------------------------------------------------------------------
 * BASELINE north_star: "independent images shard naturally across the 8 GPUs of one node with RCCL broadcast of weights and
 * gather of depth maps over xGMI", reached by the (Rust) host through this FFI layer. One process (or thread) per GPU;
 * DepthPro::infer itself never communicates -- B is a pure batch dimension (encoder.rs:216-225,249-255). The reference has
 * no collectives: these calls sit next to `DepthPro::load` / `infer` in a multi-GPU host, see INTEGRATION.md
 * section 4. All buffers are device pointers of the communicator's device; transfers are asynchronous on `stream` (NULL =
 * the device's stream, the one md_depth_pro_infer uses for stream == NULL), so they order with the inference around them. */
typedef struct md_comm_s* md_comm_t;
#define MD_COMM_ID_BYTES 128
/* A fresh rendezvous id (ncclUniqueId). The root creates it; the host hands the 128 bytes to every rank out of band
 * (environment, file, its own RPC) -- the one thing the library cannot do for a multi-process launch. */
int md_comm_unique_id(uint8_t id[MD_COMM_ID_BYTES]);
/* Collective over all ranks: joins the communicator of `world_size` ranks as `rank` on this device. */
int md_comm_init_rank(md_device_t dev, const uint8_t id[MD_COMM_ID_BYTES], int world_size, int rank, md_comm_t* out);
int md_comm_rank(md_comm_t c, int* rank, int* world_size);
/* The number of ranks RCCL itself reports for the communicator (`ncclCommCount`). */
int md_comm_count(md_comm_t c, int* ranks_seen);
int md_comm_destroy(md_comm_t c);
/* Collective: `DepthPro::load` happens on `root` only; its fp32 parameter arena is broadcast into every rank's model (same
 * config) in 1-GiB buckets and every rank commits (packs its own MFMA operand copies). Synchronises the device's stream. */
int md_comm_broadcast_weights(md_comm_t c, md_model_t m, int root);
/* Collective: the root holds `world_size` shards of `elems_per_rank` floats back to back (rank-major; e.g. [world*B,3,H,W]);
 * every rank -- the root too -- ends up with its shard in `shard_dev`. One group of ncclSend / ncclRecv (xGMI is point to
 * point: the root's links carry the shards in parallel). `all_dev` is ignored on the other ranks. */
int md_comm_scatter_images(md_comm_t c, const float* all_dev, float* shard_dev, size_t elems_per_rank, int root, void* stream);
/* Collective: the inverse for the results (depth [B,H,W] per rank -> [world*B,H,W] on the root). */
int md_comm_gather_depth(md_comm_t c, const float* shard_dev, float* all_dev, size_t elems_per_rank, int root, void* stream);

/* Tile-parallel `DepthPro::infer` for ONE call (second mode: the only way more GPUs shorten the latency of a
 * single image). Every rank of `comm` calls it with its replica of the same committed weights (md_comm_broadcast_weights):
 *   1. the root's input [B,3,H,W] (host or device pointer; NULL on the other ranks) is broadcast to every rank's staging buffer;
 *   2. rank r runs pyramid + patchify (0.02 ms) and the three ViT encoders on sequences [37B*r/n, 37B*(r+1)/n) of the 37 B
 *      (the sliding-window tiles of layers/encoder.rs:329-348 and the image / fov sequences never interact before `merge`);
 *   3. the final tokens of every window and the two hook outputs of its high-resolution tiles (encoder.rs:375-390) go to the
 *      root as ONE group of ncclSend / ncclRecv (B = 1, bf16: 100 MB in total, 1/n of it per link);
 *   4. the root runs merge, encoder tail, decoder, head and FOV network and fills the outputs; the other ranks return after
 *      their send (their output pointers are ignored and may be NULL).
 * The result on the root is bit-identical to md_depth_pro_infer on one GPU. Eager only (no graph replay). */
int md_comm_depth_pro_infer_tiles(md_comm_t comm, md_model_t model, const float* nchw, int B, int H, int W, int in_kind,
                                  float* depth, float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind,
                                  int root, void* stream);
/* The tile-parallel call with a LOOPBACK transport: the `parts` ranks are `parts` inference contexts on ONE device (a model and its
 * md_model_fork contexts, or separately created models with the same weights), each runs ITS window of the ViT stage in its own
 * workspace, and where md_comm_depth_pro_infer_tiles would ncclSend / ncclRecv a part's final tokens and hook rows, the root copies
 * them out of that part's workspace (sender and receiver sizes are compared: MD_ERR_INVALID_ARG on a mismatch). Everything of the
 * N > 1 code path except RCCL itself runs -- window clipping per rank, the segment table, the root-only tail -- on one GPU; the
 * result is bit-identical to md_depth_pro_infer. Test entry (single-GPU boxes cannot form a two-rank communicator). */
int md_depth_pro_infer_tiles_loopback(const md_model_t* models, int parts, int root, const float* nchw, int B, int H, int W,
                                      int in_kind, float* depth, float* focallength_px, float* fovx_deg, float* fovy_rad,
                                      int out_kind, void* stream);

/* ---- host-only utilities (no GPU needed) ---------------------------------------------------- */
/* The parameter inventory of `DepthPro::new` for a config: returns the number of parameters; for
 * 0 <= index < count also the name (static storage, valid until the next call from this thread),
 * element count and the uniform range [lo, hi) the seeded initialiser draws from. */
int md_param_inventory(const md_depth_pro_cfg* cfg, int init_scheme, int index, const char** name, size_t* count,
                       float* lo, float* hi);
/* The seeded generator itself: `count` values of stream (name, seed) in [lo, hi). */
int md_uniform_stream(const char* name, uint64_t seed, size_t count, float lo, float hi, float* out_host);
/* Split geometry (encoder.rs:196-206) and feature padding (encoder.rs:28-38). */
int md_split_geometry(int image_size, int window, float overlap, int* stride, int* steps);
int md_feature_padding(int window, int stride, int feature_size);

/* Per-kernel-family timing (HIP events recorded on the stream each kernel is launched on; enable
 * first). Entries accumulate over infer calls until read; reading sums them by family name into
 * names/ms/calls (capacity `cap`, count in *n) and clears them. */
int md_model_enable_timing(md_model_t m, int enable);
/* Restrict the events to ONE kernel family (e.g. "fc1_gemm"); NULL or "" = every family. Two event records per launch
 * cost about 0.7 % of a Depth Pro step when every one of its ~226 launches is timed; a throughput measurement times the
 * family it reports against its roofline inside the timed region and the rest in a separate pass. */
int md_model_set_timing_filter(md_model_t m, const char* family);
int md_model_read_timing(md_model_t m, const char** names, float* ms, int* calls, int cap, int* n);
/* Family name of every kernel launch recorded since timing was enabled / last read, in launch order
 * (one entry per kernel launch; does not clear). Lets a rocprofv3 trace be mapped to families. */
int md_model_read_launch_order(md_model_t m, const char** names, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif /* MI_DEPTH_H */
