// extern "C" surface of libmi_depth.so (include/mi_depth.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <optional>
#include <vector>

#include "md_engine.h"
#include "md_engine_util.h"

using namespace md;

namespace {
// scoped device allocation of the stand-alone operators, with 4 KiB of slack. Zeroed, or `raw`: launcher scratch whose kernels write
// every word they read is allocated, not cleared, so that a call the launcher refuses has started no device work
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes, bool raw = false) {
    if (hipMalloc(&p, bytes + 4096) != hipSuccess) {
      set_error("hipMalloc(%zu) failed", bytes);
      return MD_ERR_OOM;
    }
    return raw || hipMemset(p, 0, bytes + 4096) == hipSuccess ? MD_OK : MD_ERR_HIP;
  }
};
hipStream_t pick_stream(md_device_t dev, void* stream) { return stream ? (hipStream_t)stream : dev->stream; }
int ke_of(int prec) { return prec == MD_PREC_F32 ? 32 : (prec == MD_PREC_FP8 ? 128 : 64); }
// MD_PREC_F16X2: MFMA terms of a product with these weights -- 2 when every value is an exact IEEE half, else 3
int split_terms_of(const float* w_dev, long n, hipStream_t st, int* terms) {
  unsigned bad = 0;
  MD_TRY(count_inexact_f16(w_dev, n, st, &bad));
  *terms = bad == 0 ? 2 : 3;
  return MD_OK;
}
size_t esz_of(int prec) { return prec == MD_PREC_F32 ? 4 : (prec == MD_PREC_FP8 ? 1 : 2); }
size_t storage_bytes(int precision) { return esz_of(precision) * (precision == MD_PREC_F16X2 ? 2 : 1); }  // split-half: two planes per element
bool token_op_prec(int precision) {
  return precision == MD_PREC_BF16 || precision == MD_PREC_F32 || precision == MD_PREC_F16 || precision == MD_PREC_F16X2;
}

// A storage-typed output of a stand-alone launch: narrowed from the caller's fp32 values before the launch, widened back behind it, so
// the bytes the launch leaves alone return as they came. `narrow` = false: the launch writes every element it returns, and what it
// leaves alone reads back as the zeroed buffer's
struct StorageOut {
  DevBuf buf;
  float* user = nullptr;
  long count = 0;
  int width = 0, prec = MD_PREC_BF16;
  int open(float* u, long n, int w, int precision, hipStream_t st, bool narrow = true) {
    user = u; count = n; width = w; prec = precision;
    MD_TRY(buf.alloc((size_t)n * storage_bytes(prec)));
    return narrow ? launch_f32_to_rows(u, n, buf.p, prec, st, w) : MD_OK;
  }
  int close(hipStream_t st) { return user ? launch_rows_to_f32(buf.p, count, user, prec, st, width) : MD_OK; }  // (never opened: nothing)
};

// The staging of one stand-alone launch, opened once per entry behind its argument checks: the device, the stream, the precision and
// the operand geometry the launch-parameter builders of md_engine_util.h read (OperandGeom: all they read of a model), here built
// for a precision alone. Weight buffers are the entry's own allocations: three terms where it allocates before the count is known.
struct OpStage {
  hipStream_t st = nullptr;
  int prec = MD_PREC_F32;
  bool split = false;
  OperandGeom geom;
  DevBuf zp;
  int open(md_device_t dev, void* stream, int precision = MD_PREC_F32) {
    MD_HIP(hipSetDevice(dev->ordinal));
    st = pick_stream(dev, stream);
    prec = precision;
    split = precision == MD_PREC_F16X2;
    geom = OperandGeom{ke_of(prec), split ? 2 : 1, split ? 2 : 1, nullptr};
    return MD_OK;
  }
  size_t es() const { return storage_bytes(prec); }
  int zero_page() {  // geom.zero_page, allocated at the first call
    if (!zp.p) MD_TRY(zp.alloc(4096));
    geom.zero_page = zp.p;
    return MD_OK;
  }
  // geom.wterms over the weight groups of the launch, one call per group of n values: the split-half term count of plain weights as
  // model_commit decides it. One K for the launch: three terms as soon as one group's weights are not exact halves
  int terms_of(const float* w_dev, long n) {
    if (!split) return MD_OK;
    int t = 2;
    MD_TRY(split_terms_of(w_dev, n, st, &t));
    geom.wterms = std::max(geom.wterms, t);
    return MD_OK;
  }
  // the A operand of a dense GEMM in the precision's storage: split-half rows [hi | lo]; e4m3 on the static scale 8 / 448 (the
  // engine's LayerNorm-output scale), which *ascale then holds
  int dense_a(const float* src, long rows, int K, DevBuf& buf, float* ascale) {
    const long n = rows * K;
    if (prec == MD_PREC_FP8 && n % 4 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "e4m3 A operand: rows * K = %ld must be a multiple of 4", n);
    MD_TRY(buf.alloc((size_t)n * es()));
    if (prec != MD_PREC_FP8) return launch_f32_to_rows(src, n, buf.p, prec, st, split ? K : 0);
    *ascale = 8.0f / 448.0f;
    return launch_f32_to_fp8(src, n, 1.0f / *ascale, buf.p, st);
  }
  // W [N][K] of a dense GEMM into `buf`: split-half rows [W | W] or [Wh | Wh | Wl] by the launch's terms, e4m3 rows with their
  // per-row scales in `scale_buf`, or plain rows
  int dense_w(const float* src, int N, int K, DevBuf& buf, DevBuf& scale_buf) {
    if (split) {
      PackEntry e;
      e.kind = PACK_NK; e.d0 = N; e.d1 = K; e.k = 1; e.kp = K;
      return conv_w(src, e, buf);
    }
    if (prec != MD_PREC_FP8) return launch_f32_to_rows(src, (long)N * K, buf.p, prec, st);
    MD_TRY(scale_buf.alloc((size_t)N * 4));
    return launch_pack_fp8_rows(src, N, K, K, buf.p, (float*)scale_buf.p, st);
  }
  // the NHWC A operand of a convolution from the caller's NCHW values
  int nhwc_a(const float* src_nchw, int B, int C, int H, int W, int relu, DevBuf& buf) {
    MD_TRY(buf.alloc((size_t)B * H * W * C * es()));
    return launch_nchw_to_nhwc(src_nchw, B, C, H, W, buf.p, prec, relu, st);
  }
  // `e` packed into `buf`; terms == 0: in the launch's plain-weight form (split_terms)
  int conv_w(const float* src, PackEntry e, DevBuf& buf, int terms = 0) {
    e.terms = split_terms(geom, terms);
    e.dst = buf.p;
    return pack_weight(src, e, prec, st);
  }
  // the NHWC result `buf` of C channels back to the caller's NCHW: fp32 values, or (t_out) the precision's storage
  int nchw_out(const DevBuf& buf, int B, int C, int H, int W, bool t_out, float* out_nchw) {
    return launch_nhwc_to_nchw(buf.p, B, C, H, W, C, 0, out_nchw, t_out ? prec : MD_PREC_F32, st);
  }
  int finish() {  // the buffers of the call are freed on return
    MD_HIP(hipStreamSynchronize(st));
    return MD_OK;
  }
};
}  // namespace

extern "C" {

const char* md_last_error(void) { return get_error(); }
const char* md_version(void) { return "mi_depth 0.1 (gfx950)"; }

int md_device_open(int hip_ordinal, md_device_t* out) {
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "out is null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) MD_FAIL(MD_ERR_HIP, "no HIP device available");
  if (hip_ordinal < 0 || hip_ordinal >= n) MD_FAIL(MD_ERR_INVALID_ARG, "device ordinal %d out of range [0,%d)", hip_ordinal, n);
  MD_HIP(hipSetDevice(hip_ordinal));
  md_device_s* d = new md_device_s();
  d->ordinal = hip_ordinal;
  // a BLOCKING stream: implicitly ordered with the legacy default stream, so a caller that hands over
  // buffers produced on the null stream (and passes stream = NULL) needs no extra synchronisation
  if (hipStreamCreateWithFlags(&d->stream, hipStreamDefault) != hipSuccess) {
    delete d;
    MD_FAIL(MD_ERR_HIP, "hipStreamCreate failed");
  }
  *out = d;
  return MD_OK;
}

int md_device_close(md_device_t dev) {
  if (!dev) return MD_OK;
  (void)hipSetDevice(dev->ordinal);
  if (dev->stream) (void)hipStreamDestroy(dev->stream);
  delete dev;
  return MD_OK;
}

int md_device_synchronize(md_device_t dev) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  MD_HIP(hipSetDevice(dev->ordinal));
  MD_HIP(hipDeviceSynchronize());
  return MD_OK;
}

void md_depth_pro_cfg_default(md_depth_pro_cfg* cfg) {
  if (!cfg) return;
  cfg->patch_encoder_preset = "dinov2l16_384";
  cfg->image_encoder_preset = "dinov2l16_384";
  cfg->fov_encoder_preset = "dinov2l16_384";
  cfg->decoder_features = 256;
  cfg->use_fov_head = 1;
  cfg->interpolation = MD_INTERP_CUSTOM;
  cfg->precision = MD_PREC_BF16;
  cfg->max_batch = 1;
  cfg->ln_eps = 1e-6f;
}

int md_depth_pro_create(md_device_t dev, const md_depth_pro_cfg* cfg, uint64_t seed, int init_scheme, md_model_t* out) {
  if (!dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "device/out is null");
  ModelCfg mc;
  MD_TRY(parse_cfg(cfg, &mc));
  md_model_t m = nullptr;
  MD_TRY(model_create(dev, mc, &m));
  int s = model_init_seeded(m, seed, init_scheme);
  if (s != MD_OK) {
    model_destroy(m);
    return s;
  }
  *out = m;
  return MD_OK;
}

int md_depth_pro_load_with_config(md_device_t dev, const md_depth_pro_cfg* cfg, const char* path, md_model_t* out) {
  if (!dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "device/out is null");
  ModelCfg mc;
  MD_TRY(parse_cfg(cfg, &mc));
  // fail on I/O problems before touching the GPU (RecorderError path, mod.rs:193-208)
  {
    Container probe;
    MD_TRY(read_container(path, &probe));
  }
  md_model_t m = nullptr;
  MD_TRY(model_create(dev, mc, &m));
  int s = model_load_container(m, path);
  if (s != MD_OK) {
    model_destroy(m);
    return s;
  }
  *out = m;
  return MD_OK;
}

int md_depth_pro_load(md_device_t dev, const char* path, md_model_t* out) {
  md_depth_pro_cfg c;
  md_depth_pro_cfg_default(&c);
  return md_depth_pro_load_with_config(dev, &c, path, out);
}

int md_checkpoint_info(const char* path, int index, const char** name, const char** dtype, int* rank, int64_t shape[8],
                       int* is_burn_record) {
  static thread_local Container c;
  static thread_local std::string loaded;
  static thread_local std::vector<std::string> names;
  if (!path) MD_FAIL(MD_ERR_INVALID_ARG, "checkpoint path is null");
  if (loaded != path || index < 0) {  // (re)read on a new path and on every count query
    c = Container();
    loaded.clear();
    MD_TRY(read_container(path, &c));
    loaded = path;
    names.clear();
    for (auto& kv : c.tensors) names.push_back(kv.first);
    c.bytes.clear();  // only the directory is kept
    c.bytes.shrink_to_fit();
  }
  if (is_burn_record) *is_burn_record = c.burn_record ? 1 : 0;
  if (index >= 0 && index < (int)names.size()) {
    const ContainerTensor& t = c.tensors[names[index]];
    if (t.shape.size() > 8) MD_FAIL(MD_ERR_FORMAT, "tensor `%s` has rank %zu", names[index].c_str(), t.shape.size());
    if (name) *name = names[index].c_str();
    if (dtype) *dtype = t.dtype.c_str();
    if (rank) *rank = (int)t.shape.size();
    if (shape)
      for (size_t i = 0; i < t.shape.size(); ++i) shape[i] = t.shape[i];
  }
  return (int)names.size();
}

int md_checkpoint_read_tensor(const char* path, const char* name, float* out_host, size_t count) {
  if (!path || !name || !out_host) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  Container c;
  MD_TRY(read_container(path, &c));
  auto it = c.tensors.find(name);
  if (it == c.tensors.end()) MD_FAIL(MD_ERR_INVALID_ARG, "checkpoint `%s` has no tensor `%s`", path, name);
  size_t n = 1;
  for (auto d : it->second.shape) n *= (size_t)d;
  if (n != count) MD_FAIL(MD_ERR_SHAPE, "tensor `%s` has %zu elements, got %zu", name, n, count);
  return container_tensor_to_f32(c, it->second, out_host, count);
}

int md_model_param_count(md_model_t m) { return m ? (int)m->params.size() : 0; }

int md_model_param_info(md_model_t m, int index, const char** name, size_t* count) {
  if (!m || index < 0 || index >= (int)m->params.size()) MD_FAIL(MD_ERR_INVALID_ARG, "parameter index %d out of range", index);
  if (name) *name = m->params[index].name.c_str();
  if (count) *count = m->params[index].count();
  return MD_OK;
}

int md_model_set_tensor(md_model_t m, const char* name, const float* host_data, size_t count) {
  if (!m || !name || !host_data) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (m->parent) MD_FAIL(MD_ERR_INVALID_ARG, "a fork shares its root's weights: set tensors on the root model");
  auto it = m->pindex.find(name);
  if (it == m->pindex.end()) MD_FAIL(MD_ERR_INVALID_ARG, "unknown parameter `%s`", name);
  if (m->params[it->second].count() != count)
    MD_FAIL(MD_ERR_SHAPE, "parameter `%s` has %zu elements, got %zu", name, m->params[it->second].count(), count);
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipMemcpy(m->w32[it->second], host_data, count * 4, hipMemcpyHostToDevice));
  m->committed = false;
  return MD_OK;
}

int md_model_get_tensor(md_model_t m, const char* name, float* host_data, size_t count) {
  if (!m || !name || !host_data) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  auto it = m->pindex.find(name);
  if (it == m->pindex.end()) MD_FAIL(MD_ERR_INVALID_ARG, "unknown parameter `%s`", name);
  if (m->params[it->second].count() != count)
    MD_FAIL(MD_ERR_SHAPE, "parameter `%s` has %zu elements, got %zu", name, m->params[it->second].count(), count);
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipMemcpy(host_data, m->w32[it->second], count * 4, hipMemcpyDeviceToHost));
  return MD_OK;
}

int md_model_commit_weights(md_model_t m) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  return model_commit(m);
}

int md_model_round_weights_f16(md_model_t m) { return model_round_weights_f16(m); }

int md_model_weight_arena(md_model_t m, void** device_ptr, size_t* bytes) {
  if (!m || !device_ptr || !bytes) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (m->parent) MD_FAIL(MD_ERR_INVALID_ARG, "a fork shares its root's weights: take the arena of the root model");
  *device_ptr = m->w32_base;
  *bytes = m->w32_bytes;
  m->committed = false;  // the caller is about to overwrite it (broadcast); commit afterwards
  return MD_OK;
}

int md_model_destroy(md_model_t m) { return model_destroy(m); }

int md_model_fork(md_model_t m, md_model_t* out) { return model_fork(m, out); }

int md_depth_pro_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth,
                       float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind, void* stream) {
  if (!nchw) MD_FAIL(MD_ERR_INVALID_ARG, "input pointer is null");
  if (m && m->kind != 0) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth Pro model");
  return model_infer(m, nchw, B, H, W, in_kind, depth, focallength_px, fovx_deg, fovy_rad, out_kind, (hipStream_t)stream,
                     nullptr, 0);
}

int md_depth_pro_infer_with_focal(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const float* f_px, float* depth,
                                  float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind, void* stream) {
  if (!nchw) MD_FAIL(MD_ERR_INVALID_ARG, "input pointer is null");
  if (m && m->kind != 0) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth Pro model");
  return model_infer(m, nchw, B, H, W, in_kind, depth, focallength_px, fovx_deg, fovy_rad, out_kind, (hipStream_t)stream,
                     nullptr, 0, f_px, in_kind);
}

int md_depth_pro_decoder_from_features(md_model_t m, const md_nchw_view* features, int levels, int B, int in_kind,
                                       float* out_features, float* out_lowres, float* const* out_fusions, int out_kind,
                                       void* stream) {
  return model_decoder_from_features(m, features, levels, B, in_kind, out_features, out_lowres, out_fusions, out_kind, (hipStream_t)stream);
}

int md_depth_pro_head_debug(md_model_t m, const md_nchw_view* feature, int B, int in_kind, const md_head_debug* out, int out_kind,
                            void* stream) {
  return model_head_debug(m, feature, B, in_kind, out, out_kind, (hipStream_t)stream);
}

int md_depth_pro_infer_windows(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth,
                               float* focallength_px, float* fovx_deg, float* fovy_rad, int out_kind, int parts,
                               float* window_ms, float* tail_ms, void* stream) {
  if (!nchw) MD_FAIL(MD_ERR_INVALID_ARG, "input pointer is null");
  if (m && m->kind != 0) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth Pro model");
  if (parts < 1 || parts > 64) MD_FAIL(MD_ERR_INVALID_ARG, "parts = %d (1 .. 64)", parts);
  ShardPlan sp;
  sp.parts = parts;
  sp.part = -1;
  sp.window_ms = window_ms;
  sp.tail_ms = tail_ms;
  return model_infer_sharded(m, nchw, B, H, W, in_kind, depth, focallength_px, fovx_deg, fovy_rad, out_kind, (hipStream_t)stream, sp);
}

int md_infer_from_rgb(md_model_t m, const uint8_t* rgb, size_t rgb_len, int w, int h, int in_kind, float* depth,
                      float* focallength_px, float* fovy_rad, int out_kind, void* stream) {
  if (!rgb) MD_FAIL(MD_ERR_INVALID_ARG, "rgb pointer is null");
  if (w <= 0 || h <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid image size %dx%d", w, h);
  // inference.rs:85-95: length check comes first and is an Err, not a panic
  const size_t expected = (size_t)w * (size_t)h * 3;
  if (rgb_len != expected) MD_FAIL(MD_ERR_SHAPE, "expected %zu RGB bytes for %dx%d, got %zu", expected, w, h, rgb_len);
  if (m && m->kind != 0) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth Pro model");
  return model_infer(m, nullptr, 1, h, w, in_kind, depth, focallength_px, nullptr, fovy_rad, out_kind, (hipStream_t)stream,
                     rgb, rgb_len);
}

int md_infer_from_rgb_with_focal(md_model_t m, const uint8_t* rgb, size_t rgb_len, int w, int h, int in_kind, float f_px,
                                 float* depth, float* focallength_px, float* fovy_rad, int out_kind, void* stream) {
  if (!rgb) MD_FAIL(MD_ERR_INVALID_ARG, "rgb pointer is null");
  if (w <= 0 || h <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid image size %dx%d", w, h);
  const size_t expected = (size_t)w * (size_t)h * 3;
  if (rgb_len != expected) MD_FAIL(MD_ERR_SHAPE, "expected %zu RGB bytes for %dx%d, got %zu", expected, w, h, rgb_len);
  if (m && m->kind != 0) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth Pro model");
  return model_infer(m, nullptr, 1, h, w, in_kind, depth, focallength_px, nullptr, fovy_rad, out_kind, (hipStream_t)stream,
                     rgb, rgb_len, &f_px, MD_MEM_HOST);
}

int md_model_enable_graph(md_model_t m, int enable) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  m->graph_enabled = enable != 0;
  return MD_OK;
}

int md_model_query(md_model_t m, const char* key, int64_t* out) {
  if (!m || !key || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const std::string k = key;
  if (k == "img_size") *out = m->S;
  else if (k == "patch_window") *out = m->win;
  else if (k == "interpolation") *out = m->cfg.interpolation;
  else if (k == "precision") *out = m->prec;
  else if (k == "max_batch") *out = m->cfg.max_batch;
  else if (k == "num_params") {
    int64_t n = 0;
    for (auto& p : m->params) n += (int64_t)p.count();
    *out = n;
  } else if (k == "workspace_bytes") *out = (int64_t)m->ws.cap;
  else if (k == "weight_bytes") *out = m->parent ? 0 : (int64_t)(m->w32_bytes + m->wpk_bytes);  // a fork owns none
  else if (k == "tiles_per_image") *out = m->steps0 * m->steps0 + m->steps1 * m->steps1 + 1;
  else if (k == "seq_stride") *out = m->SS;
  else if (k == "is_fork") *out = m->parent ? 1 : 0;
  else if (k == "forks") *out = m->forks.load();
  else if (k == "weight_terms") *out = model_root(m)->wterms;
  else if (k == "allocs") *out = m->alloc_count;
  else if (k == "voxel_overflow") return points_voxel_overflow(m, out);
  else if (k == "outlier_overflow") return points_outlier_overflow(m, out);
  else if (k == "clusters_overflow") return points_clusters_overflow(m, out);
  else if (k == "match_overflow") return points_match_overflow(m, out);
  else if (k == "register_overflow") return points_register_overflow(m, out);
  else if (k == "decimate_overflow") return points_decimate_overflow(m, out);
  else if (k == "da3_shape_builds") *out = da3_shape_builds(m);
  else if (k == "batch_invariant") *out = m->batch_invariant ? 1 : 0;
  else if (k == "ln_fold") *out = m->ln_fold_opt;
  else if (k == "ln_fold_active") *out = m->ln_fold_on() ? 1 : 0;
  else if (model_decoder_query(m, k, out)) {}
  else MD_FAIL(MD_ERR_INVALID_ARG, "unknown query key `%s`", key);
  return MD_OK;
}

int md_model_set_option(md_model_t m, const char* key, int64_t value) {
  if (!m || !key) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const std::string k = key;
  if (k == "batch_invariant") {
    if (value != 0 && value != 1) MD_FAIL(MD_ERR_INVALID_ARG, "batch_invariant takes 0 or 1");
    if (m->batch_invariant != (value != 0)) {
      m->batch_invariant = value != 0;
      MD_HIP(hipSetDevice(m->dev->ordinal));
      MD_HIP(hipDeviceSynchronize());
      m->graphs.clear();  // captured graphs hold the kernel forms of the old setting
    }
    return MD_OK;
  }
  if (k == "ln_fold") {
    if (value < 0 || value > 4) MD_FAIL(MD_ERR_INVALID_ARG, "ln_fold takes 0 (off), 1 (automatic), 2 (on whenever the model can), 3 / 4 (bench diagnostics: unfolded schedule through the fold-form consumer kernels on neutral statistics / the fold with the ln_finish launch)");
    if (value >= 2 && !m->ln_fold_can) MD_FAIL(MD_ERR_UNSUPPORTED, "ln_fold: this model cannot fold its LayerNorms (16-bit Depth Pro models of width %% 256 == 0 can)");
    if (m->ln_fold_opt != (int)value) {
      m->ln_fold_opt = (int)value;
      MD_HIP(hipSetDevice(m->dev->ordinal));
      MD_HIP(hipDeviceSynchronize());
      m->graphs.clear();  // captured graphs hold the launches of the old setting
    }
    return MD_OK;
  }
  MD_FAIL(MD_ERR_INVALID_ARG, "unknown option `%s`", key);
}

int md_model_enable_taps(md_model_t m, int enable) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  m->taps_enabled = enable != 0;
  return MD_OK;
}

int md_model_read_tap(md_model_t m, const char* name, float* host_data, size_t capacity, int64_t dims[4]) {
  if (!m || !name) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  auto it = m->taps.find(name);
  if (it == m->taps.end() || !it->second.dev) MD_FAIL(MD_ERR_INVALID_ARG, "tap `%s` was not captured", name);
  if (dims) memcpy(dims, it->second.dims, sizeof(int64_t) * 4);
  if (!host_data) return MD_OK;
  if (capacity < it->second.count) MD_FAIL(MD_ERR_SHAPE, "tap `%s` needs %zu floats, capacity %zu", name, it->second.count, capacity);
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipDeviceSynchronize());
  MD_HIP(hipMemcpy(host_data, it->second.dev, it->second.count * 4, hipMemcpyDeviceToHost));
  return MD_OK;
}

int md_model_enable_timing(md_model_t m, int enable) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  m->timing_enabled = enable != 0;
  return MD_OK;
}

int md_model_set_timing_filter(md_model_t m, const char* family) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  m->timing_filter = family ? family : "";
  return MD_OK;
}

int md_model_read_timing(md_model_t m, const char** names, float* ms, int* calls, int cap, int* n) {
  if (!m || !n) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipDeviceSynchronize());
  m->timing_names_out.clear();
  std::vector<float> tot;
  std::vector<int> cnt;
  for (auto& t : m->timing) {
    float e = 0.f;
    if (hipEventElapsedTime(&e, t.a, t.b) != hipSuccess) continue;
    size_t i = 0;
    for (; i < m->timing_names_out.size(); ++i)
      if (m->timing_names_out[i] == t.name) break;
    if (i == m->timing_names_out.size()) {
      m->timing_names_out.push_back(t.name);
      tot.push_back(0.f);
      cnt.push_back(0);
    }
    tot[i] += e;
    cnt[i] += 1;
  }
  for (auto& t : m->timing) {  // entries accumulate across infers until they are read
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  m->timing.clear();
  *n = (int)m->timing_names_out.size();
  for (int i = 0; i < *n && i < cap; ++i) {
    if (names) names[i] = m->timing_names_out[i].c_str();
    if (ms) ms[i] = tot[i];
    if (calls) calls[i] = cnt[i];
  }
  return MD_OK;
}

int md_model_read_launch_order(md_model_t m, const char** names, int cap, int* n) {
  if (!m || !n) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  *n = (int)m->timing.size();
  for (int i = 0; i < *n && i < cap; ++i)
    if (names) names[i] = m->timing[i].name.c_str();
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------
// stand-alone operators
// ------------------------------------------------------------------------------------------------
int md_op_rgb_to_input(md_device_t dev, const uint8_t* rgb_dev, size_t rgb_len, int w, int h, float* out_dev, void* stream) {
  if (!dev || !rgb_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (w <= 0 || h <= 0 || rgb_len != (size_t)w * h * 3)
    MD_FAIL(MD_ERR_SHAPE, "expected %zu RGB bytes for %dx%d, got %zu", (size_t)w * h * 3, w, h, rgb_len);
  MD_HIP(hipSetDevice(dev->ordinal));
  return launch_rgb_to_input(rgb_dev, w, h, out_dev, pick_stream(dev, stream));
}

int md_frame_geometry(md_model_t m, int w, int h, const md_frame_opts* o, int* th, int* tw, int* oh, int* ow) {
  return frame_geometry(m, w, h, o, th, tw, oh, ow);
}

int md_process_frame(md_model_t m, const uint8_t* rgb, int B, int w, int h, int in_kind, const md_frame_opts* o,
                     const md_frame_outputs* out, int out_kind, void* stream) {
  return process_frame(m, rgb, B, w, h, in_kind, o, out, out_kind, (hipStream_t)stream);
}

void md_points_opts_default(md_points_opts* o) {
  if (!o) return;
  o->pixel_offset = 0.f;
  o->depth_min = o->depth_max = 0.f;
  o->conf_min = 0.f;
  o->edge_rtol = 0.f;
  o->stride = 1;
  o->world = 0;
}

int md_op_unproject(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                    const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, void* stream) {
  return op_unproject(dev, DepthMaps{depth_dev, conf_dev, rgb_dev, B, H, W}, cam, o, out, nullptr, (hipStream_t)stream);
}

int md_infer_points(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                    const md_points_opts* o, const md_points_outputs* out, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, nullptr, nullptr, nullptr, false}, (hipStream_t)stream);
}

void md_view_filter_opts_default(md_view_filter_opts* o) {
  if (!o) return;
  o->pixel_offset = 0.f;
  o->depth_min = o->depth_max = 0.f;
  o->conf_percentile = 0;
  o->view_rtol = 0.f;
  o->min_views = 0;
}

int md_op_filter_views(md_device_t dev, const float* depth_dev, const float* conf_dev, int B, int H, int W, const md_points_cameras* cam,
                       const md_view_filter_opts* o, const md_view_filter_outputs* out, void* stream) {
  return op_filter_views(dev, DepthMaps{depth_dev, conf_dev, nullptr, B, H, W}, cam, o, out, (hipStream_t)stream);
}

int md_infer_points_filtered(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                             const md_points_cameras* cam, const md_view_filter_opts* fo, const md_points_opts* o,
                             const md_points_outputs* out, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nullptr, nullptr, true}, (hipStream_t)stream);
}

int md_op_unproject_normals(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                            const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                            void* stream) {
  return op_unproject(dev, DepthMaps{depth_dev, conf_dev, rgb_dev, B, H, W}, cam, o, out, nrm, (hipStream_t)stream);
}

int md_infer_points_normals(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                            const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                            int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, nullptr, false}, (hipStream_t)stream);
}

int md_op_voxel_thin(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                     int64_t N, const md_points_voxel* vox, const md_points_outputs* out, float* normals_out, void* stream) {
  return op_voxel_thin(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, vox, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_voxel(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                          const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                          const md_points_voxel* vox, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false}, (hipStream_t)stream);
}

void md_render_opts_default(md_render_opts* o) {
  if (!o) return;
  o->pixel_offset = 0.f;
  o->z_near = o->z_far = 0.f;
  o->radius = 0;
}

int md_op_render_points(md_device_t dev, const float* xyz_dev, const uint8_t* rgb_dev, int64_t N, const int32_t* count_dev, int T, int H,
                        int W, const md_points_cameras* cam, const md_render_opts* opts, const md_render_outputs* out, void* stream) {
  return op_render_points(dev, PointList{xyz_dev, nullptr, rgb_dev, nullptr, N}, count_dev, T, H, W, cam, opts, out, (hipStream_t)stream);
}

int md_infer_points_render(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                           const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd}, (hipStream_t)stream);
}

int md_op_mesh_grid(md_device_t dev, const float* depth_dev, const int32_t* pixel_index_dev, int B, int H, int W, int stride,
                    int64_t vertex_limit, const md_points_mesh* mesh, void* stream) {
  return op_mesh_grid(dev, DepthMaps{depth_dev, nullptr, nullptr, B, H, W}, pixel_index_dev, stride, vertex_limit, mesh, (hipStream_t)stream);
}

int md_op_unproject_mesh(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                         const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                         const md_points_mesh* mesh, void* stream) {
  return op_unproject(dev, DepthMaps{depth_dev, conf_dev, rgb_dev, B, H, W}, cam, o, out, nrm, (hipStream_t)stream, mesh);
}

int md_infer_points_mesh(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                         const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                         const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh}, (hipStream_t)stream);
}

void md_raster_opts_default(md_raster_opts* o) {
  if (!o) return;
  o->pixel_offset = 0.f;
  o->z_near = o->z_far = 0.f;
  o->cull = 0;
  o->max_extent = 0;
}

int md_op_render_mesh(md_device_t dev, const float* xyz_dev, const uint8_t* rgb_dev, int64_t N, const int32_t* faces_dev, int64_t F,
                      const int32_t* face_count_dev, int T, int H, int W, const md_points_cameras* cam, const md_raster_opts* opts,
                      const md_raster_outputs* out, void* stream) {
  return op_render_mesh(dev, PointList{xyz_dev, nullptr, rgb_dev, nullptr, N}, faces_dev, F, face_count_dev, T, H, W, cam, opts, out,
                        (hipStream_t)stream);
}

int md_infer_points_raster(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                           const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                           int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst}, (hipStream_t)stream);
}

int md_op_radius_outliers(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                          int64_t N, const md_points_outlier* outl, const md_points_outputs* out, float* normals_out, void* stream) {
  return op_radius_outliers(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, outl, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_outlier(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                            const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                            const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                            const md_points_outlier* outl, int out_kind, void* stream) {
  return infer_points(m, PointsCall{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst, outl},
                      (hipStream_t)stream);
}

int md_infer_points_decimate(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                             const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                             const md_points_outlier* outl, const md_points_decimate* dec, int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_decimate_mesh(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                        int64_t N, const int32_t* faces_dev, int64_t F, const md_points_decimate* dec, const md_points_outputs* out,
                        float* normals_out, void* stream) {
  return op_decimate_mesh(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, faces_dev, F, dec, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_components(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                               const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                               const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                               const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp, int out_kind,
                               void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_mesh_components(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev,
                          int64_t N, const int32_t* faces_dev, int64_t F, const md_points_components* comp, const md_points_outputs* out,
                          float* normals_out, void* stream) {
  return op_mesh_components(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, faces_dev, F, comp, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_smooth(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                           const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                           const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp,
                           const md_points_smooth* smooth, int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_smooth_mesh(md_device_t dev, const float* xyz_dev, int64_t N, const int32_t* faces_dev, int64_t F, const md_points_smooth* smooth,
                      int64_t capacity, void* stream) {
  return op_smooth_mesh(dev, xyz_dev, N, faces_dev, F, smooth, capacity, (hipStream_t)stream);
}

int md_infer_points_planes(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                           const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                           const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                           const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp,
                           const md_points_smooth* smooth, const md_points_planes* pln, int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth; c.pln = pln;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_fit_planes(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev, int64_t N,
                     const md_points_planes* pln, const md_points_outputs* out, float* normals_out, void* stream) {
  return op_fit_planes(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, pln, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_clusters(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                             const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                             const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp,
                             const md_points_smooth* smooth, const md_points_planes* pln, const md_points_clusters* clu, int out_kind,
                             void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth; c.pln = pln; c.clu = clu;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_cluster_points(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev, int64_t N,
                         const md_points_clusters* clu, const md_points_outputs* out, float* normals_out, void* stream) {
  return op_cluster_points(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, clu, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_match(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                          const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                          const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                          const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp,
                          const md_points_smooth* smooth, const md_points_planes* pln, const md_points_clusters* clu, const md_points_match* mat,
                          int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth; c.pln = pln; c.clu = clu; c.mat = mat;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_match_points(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev, int64_t N,
                       const md_points_match* mat, const md_points_outputs* out, float* normals_out, void* stream) {
  return op_match_points(dev, PointList{xyz_dev, conf_dev, rgb_dev, normals_dev, N}, mat, out, normals_out, (hipStream_t)stream);
}

int md_infer_points_register(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                             const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm,
                             const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh, const md_points_raster* rst,
                             const md_points_outlier* outl, const md_points_decimate* dec, const md_points_components* comp,
                             const md_points_smooth* smooth, const md_points_planes* pln, const md_points_clusters* clu, const md_points_match* mat,
                             const md_points_register* reg, int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth; c.pln = pln; c.clu = clu; c.mat = mat; c.reg = reg;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_register_points(md_device_t dev, const float* xyz_dev, const float* normals_dev, int64_t N, const md_points_register* reg,
                           float* xyz_out, float* normals_out, void* stream) {
  return op_register_points(dev, xyz_dev, normals_dev, N, reg, xyz_out, normals_out, (hipStream_t)stream);
}

int md_infer_points_register_plane(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb,
                                   const md_points_cameras* cam, const md_view_filter_opts* fo, const md_points_opts* o, const md_points_outputs* out,
                                   const md_points_normals* nrm, const md_points_voxel* vox, const md_points_render* rnd, const md_points_mesh* mesh,
                                   const md_points_raster* rst, const md_points_outlier* outl, const md_points_decimate* dec,
                                   const md_points_components* comp, const md_points_smooth* smooth, const md_points_planes* pln,
                                   const md_points_clusters* clu, const md_points_match* mat, const md_points_register* reg,
                                   const md_points_register_plane* plane, int out_kind, void* stream) {
  PointsCall c{nchw, B, H, W, in_kind, rgb, cam, o, out, out_kind, fo, nrm, vox, false, rnd, mesh, rst};
  c.outl = outl; c.dec = dec; c.comp = comp; c.smooth = smooth; c.pln = pln; c.clu = clu; c.mat = mat; c.reg = reg; c.rpl = plane;
  return infer_points(m, c, (hipStream_t)stream);
}

int md_op_register_points_plane(md_device_t dev, const float* xyz_dev, const float* normals_dev, int64_t N, const md_points_register* reg,
                                const md_points_register_plane* plane, float* xyz_out, float* normals_out, void* stream) {
  return op_register_points(dev, xyz_dev, normals_dev, N, reg, xyz_out, normals_out, (hipStream_t)stream, plane);
}

int md_raster_inline_pixels(void) { return md::raster_inline_pixels(); }
int md_debug_raster_queue(int capacity) { return capacity < 0 ? MD_ERR_INVALID_ARG : md::raster_queue_capacity(capacity); }

int md_catmull_rom_taps(int in_len, int out_len, int index, int* left, int* count, float* weights) {
  if (!left || !count) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (in_len <= 0 || out_len <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid pass %d -> %d", in_len, out_len);
  if (index < 0 || index >= out_len) MD_FAIL(MD_ERR_INVALID_ARG, "index %d outside [0, %d)", index, out_len);
  catmull_rom_window(in_len, out_len, index, left, count, weights);
  return MD_OK;
}

int md_op_resize_catmull_rom(md_device_t dev, const uint8_t* rgb_dev, int B, int h, int w, int sw, int sh, int cx, int cy, int tw, int th,
                             uint8_t* out_u8, float* out_nchw, void* stream) {
  if (!rgb_dev || (!out_u8 && !out_nchw)) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || h <= 0 || w <= 0 || sw <= 0 || sh <= 0 || tw <= 0 || th <= 0 || cx < 0 || cy < 0 || cx + tw > sw || cy + th > sh)
    MD_FAIL(MD_ERR_SHAPE, "invalid resize %dx%d -> %dx%d, crop %dx%d at (%d, %d)", w, h, sw, sh, tw, th, cx, cy);
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  OpStage s;
  MD_TRY(s.open(dev, stream));
  // tables of the two passes (identity when the size stays), uploaded for this call only
  const bool crop_only = sw == w && sh == h;
  std::vector<int> left[2], count[2];
  std::vector<int2> win[2];
  std::vector<float> wt[2];
  int maxc[2] = {1, 1};
  const int in_len[2] = {h, w}, out_len[2] = {sh, sw};
  DevBuf tab[2], wbuf[2], tmp;
  for (int a = 0; a < 2; ++a) {
    const int n = out_len[a];
    maxc[a] = crop_only ? 1 : catmull_rom_max_taps(in_len[a], n);
    left[a].assign(n, 0);
    count[a].assign(n, 1);
    wt[a].assign((size_t)n * maxc[a], 0.f);
    win[a].resize(n);
    for (int o = 0; o < n; ++o) {
      if (crop_only) {
        left[a][o] = o;
        wt[a][(size_t)o * maxc[a]] = 1.f;
      } else {
        catmull_rom_window(in_len[a], n, o, &left[a][o], &count[a][o], &wt[a][(size_t)o * maxc[a]]);
      }
      win[a][o] = make_int2(left[a][o], count[a][o]);
    }
    MD_TRY(tab[a].alloc((size_t)n * sizeof(int2)));
    MD_TRY(wbuf[a].alloc(wt[a].size() * 4));
    MD_HIP(hipMemcpy(tab[a].p, win[a].data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice));
    MD_HIP(hipMemcpy(wbuf[a].p, wt[a].data(), wt[a].size() * 4, hipMemcpyHostToDevice));
  }
  int xb0 = 0, nq = 0;
  catmull_rom_span(left[1].data(), count[1].data(), cx, tw, &xb0, &nq);
  MD_TRY(tmp.alloc((size_t)B * th * nq * 16));
  MD_TRY(launch_resize_catmull_rom(rgb_dev, B, h, w, CrAxis{(const int2*)tab[0].p, (const float*)wbuf[0].p, maxc[0]}, cy, th,
                                   CrAxis{(const int2*)tab[1].p, (const float*)wbuf[1].p, maxc[1]}, cx, tw, xb0, nq, (float*)tmp.p, out_u8,
                                   out_nchw, s.st));
  return s.finish();
}

int md_op_depth_display(md_device_t dev, const float* depth_dev, int B, int h, int w, int crop_x, int crop_y, int crop_w, int crop_h, int ow,
                        int oh, int normalize, int format, void* out, float* range, void* stream) {
  if (!depth_dev || (!out && !range)) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (format != MD_FRAME_U8_GRAY && format != MD_FRAME_RGBA_F32) MD_FAIL(MD_ERR_INVALID_ARG, "unknown display format %d", format);
  if (format == MD_FRAME_U8_GRAY && !normalize) MD_FAIL(MD_ERR_INVALID_ARG, "the u8 grey display needs normalize = 1");
  if (crop_w == 0) {
    crop_x = crop_y = 0;
    crop_w = w;
    crop_h = h;
  }
  if (B <= 0 || h <= 0 || w <= 0 || ow <= 0 || oh <= 0 || crop_x < 0 || crop_y < 0 || crop_w <= 0 || crop_h <= 0 || crop_x + crop_w > w ||
      crop_y + crop_h > h)
    MD_FAIL(MD_ERR_SHAPE, "invalid display of [%d,%d,%d]: crop %dx%d at (%d, %d) -> %dx%d", B, h, w, crop_w, crop_h, crop_x, crop_y, ow, oh);
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  OpStage s;
  MD_TRY(s.open(dev, stream));
  const DisplayGeom g = display_geom(B, h, w, crop_x, crop_y, crop_w, crop_h, ow, oh);
  DevBuf parts;
  MD_TRY(parts.alloc((size_t)B * display_parts(g) * sizeof(float2)));
  MD_TRY(launch_depth_display(depth_dev, g, normalize, format, out, range, (float2*)parts.p, s.st));
  return s.finish();
}

int md_op_resize_bilinear(md_device_t dev, const float* in_dev, int B, int C, int H, int W, float* out_dev, int OH, int OW,
                          int method, void* stream) {
  return md_op_resize_bilinear_ex(dev, in_dev, B, C, H, W, out_dev, OH, OW, method, 0, stream);
}

int md_op_resize_bilinear_ex(md_device_t dev, const float* in_dev, int B, int C, int H, int W, float* out_dev, int OH, int OW,
                             int method, int post, void* stream) {
  if (!dev || !in_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid input shape");
  if (method != MD_INTERP_CUSTOM && method != MD_INTERP_BURN) MD_FAIL(MD_ERR_INVALID_ARG, "unknown interpolation method %d", method);
  if (post != 0 && post != 1) MD_FAIL(MD_ERR_INVALID_ARG, "post: 0 (none) or 1 (the final depth 1 / clamp), got %d", post);
  MD_HIP(hipSetDevice(dev->ordinal));
  return launch_resize_bilinear(in_dev, B * C, H, W, out_dev, OH, OW, method, post, pick_stream(dev, stream));
}

int md_op_pyramid_patchify(md_device_t dev, const float* x_dev, int B, int S, int window, int patch, int method, int precision,
                           int force_generic, void* out_dev, int* rows_out, int* cols_out, void* stream) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || S <= 0 || window <= 0 || patch <= 0 || S != 4 * window || window % patch != 0) MD_FAIL(MD_ERR_SHAPE, "pyramid: S must be 4 * window and window a multiple of the patch size");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  PyramidGeom g;
  g.B = B; g.S = S; g.win = window; g.ps = patch; g.method = method;
  split_geometry(S, window, 0.25f, &g.stride0, &g.steps0);      // encoder.rs:329
  split_geometry(S / 2, window, 0.5f, &g.stride1, &g.steps1);   // encoder.rs:330
  const int grid = window / patch;
  if (rows_out) *rows_out = (g.steps0 * g.steps0 + g.steps1 * g.steps1 + 1) * B * grid * grid;
  if (cols_out) *cols_out = 3 * patch * patch;
  if (!x_dev || !out_dev) return MD_OK;  // geometry query
  MD_HIP(hipSetDevice(dev->ordinal));
  return launch_pyramid_patchify(x_dev, g, out_dev, precision, pick_stream(dev, stream), force_generic != 0);
}

int md_op_resize_nhwc(md_device_t dev, const void* in_dev, int B, int H, int W, int C, void* out_dev, int OH, int OW, int method,
                      int precision, void* stream) {
  if (!dev || !in_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (precision != MD_PREC_BF16 && precision != MD_PREC_F32 && precision != MD_PREC_F16) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  return md_op_resize_nhwc_ex(dev, in_dev, B, H, W, C, C, out_dev, OH, OW, C, method, nullptr, precision, stream);
}

// The forms the engines launch: padded pixel strides, the fp32 addend table [OH][OW][C], split-half pixels [hi: ld | lo: ld]. The
// caller's buffers hold the stored bytes. No staging buffer lives in the call, so it stays ordered on the stream like
// md_op_resize_nhwc (which the benchmark times) and does not synchronise.
int md_op_resize_nhwc_ex(md_device_t dev, const void* in_dev, int B, int H, int W, int C, int ld_in, void* out_dev, int OH, int OW,
                         int ld_out, int method, const float* addend_dev, int precision, void* stream) {
  if (!dev || !in_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  if (method != MD_INTERP_CUSTOM && method != MD_INTERP_BURN) MD_FAIL(MD_ERR_INVALID_ARG, "unknown interpolation method %d", method);
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (C % 8 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "resize_nhwc: C=%d must be a multiple of 8", C);
  if (ld_in < C || ld_out < C) MD_FAIL(MD_ERR_INVALID_ARG, "resize_nhwc: %d channels in pixels of %d / %d", C, ld_in, ld_out);
  // the kernel moves 8 elements (16 bytes of a 2-byte type) per access at channel offsets that are multiples of 8
  if (ld_in % 8 != 0 || ld_out % 8 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "resize_nhwc: pixel strides %d / %d must be multiples of 8", ld_in, ld_out);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  return launch_resize_nhwc(in_dev, B, H, W, C, ld_in, out_dev, OH, OW, ld_out, method, addend_dev, precision, s.st);
}

int md_op_resize_output_size(int H, int W, float scale_h, float scale_w, int* oh, int* ow) {
  if (!oh || !ow) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  // interpolate.rs:24-27
  const long a = (long)std::floor((float)H * scale_h), b = (long)std::floor((float)W * scale_w);
  *oh = (int)(a > 1 ? a : 1);
  *ow = (int)(b > 1 ? b : 1);
  return MD_OK;
}

int md_op_split(md_device_t dev, const float* in_dev, int B, int C, int S, int window, float overlap, float* out_dev,
                int* steps_out, void* stream) {
  if (!dev || !in_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || C <= 0 || S <= 0 || window <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  int stride, steps;
  split_geometry(S, window, overlap, &stride, &steps);
  if (steps_out) *steps_out = steps;
  if (!out_dev) return MD_OK;  // geometry query
  if ((steps - 1) * stride + window > S) MD_FAIL(MD_ERR_SHAPE, "window %d with stride %d does not tile %d", window, stride, S);
  MD_HIP(hipSetDevice(dev->ordinal));
  return launch_split(in_dev, B, C, S, window, stride, steps, out_dev, pick_stream(dev, stream));
}

int md_op_merge(md_device_t dev, const float* in_dev, int tiles, int C, int h, int w, int batch, int padding, float* out_dev,
                int* out_h, int* out_w, void* stream) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (tiles <= 0 || batch <= 0 || C <= 0 || h <= 0 || w <= 0 || padding < 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  const int steps = (int)std::lround(std::sqrt((double)(tiles / batch)));  // encoder.rs:240
  if (steps <= 0 || steps * steps * batch != tiles) MD_FAIL(MD_ERR_SHAPE, "%d tiles is not steps^2 * batch(%d)", tiles, batch);
  if (steps > 1 && (h - 2 * padding <= 0 || w - 2 * padding <= 0)) MD_FAIL(MD_ERR_SHAPE, "padding %d too large for %dx%d tiles", padding, h, w);
  const int OH = merged_extent(h, steps, padding), OW = merged_extent(w, steps, padding);
  if (out_h) *out_h = OH;
  if (out_w) *out_w = OW;
  if (!out_dev || !in_dev) return MD_OK;
  MD_HIP(hipSetDevice(dev->ordinal));
  return launch_merge(in_dev, batch, C, h, w, steps, padding, out_dev, OH, OW, pick_stream(dev, stream));
}

int md_op_layernorm(md_device_t dev, const float* x_dev, const float* gamma_dev, const float* beta_dev, int rows, int D,
                    float eps, float* out_dev, void* stream) {
  if (!dev || !x_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (rows <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid rows");
  MD_HIP(hipSetDevice(dev->ordinal));
  SeqGroups g;
  memset(&g, 0, sizeof(g));
  g.ngroups = 1;
  g.nseq[0] = rows;
  g.a[0] = gamma_dev;
  g.b[0] = beta_dev;
  return launch_layernorm(x_dev, out_dev, rows, D, eps, 1, g, MD_PREC_F32, 1, pick_stream(dev, stream));
}

int md_op_linear(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int M, int N, int K, int act,
                 int precision, float* out_dev, void* stream) {
  return md_op_linear_tile(dev, x_dev, w_dev, bias_dev, M, N, K, act, precision, TILE_AUTO, out_dev, stream);
}

int md_op_linear_tile(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int M, int N, int K,
                      int act, int precision, int tile, float* out_dev, void* stream) {
  if (!dev || !x_dev || !w_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (M <= 0 || N <= 0 || K <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  const KsplitScope ksplit(1);  // the stand-alone operator exercises the k-split form of the 64 x 64 kernel (what the DA3 engine runs)
  const bool storage_out = (precision & MD_OP_STORAGE_OUT) && (precision & 0xff) != MD_PREC_F32;
  precision &= 0xff;
  if (!token_op_prec(precision) && precision != MD_PREC_FP8) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (K % ke_of(precision) != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "K=%d must be a multiple of %d", K, ke_of(precision));
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  DevBuf xa, wa, ws;
  StorageOut ob;
  GemmParams p;
  MD_TRY(wa.alloc((size_t)N * K * esz_of(precision) * (s.split ? 3 : 1)));
  MD_TRY(s.terms_of(w_dev, (long)N * K));
  MD_TRY(s.dense_a(x_dev, M, K, xa, &p.ascale));
  MD_TRY(s.dense_w(w_dev, N, K, wa, ws));
  p.N = N; p.ngroups = 1; p.g_rows[0] = M; p.W[0] = wa.p; p.wscale[0] = (const float*)ws.p; p.A = xa.p;
  split_dense_a(s.geom, p, K, K, 0);
  p.epi = EPI_STORE; p.act = act; p.out_f32 = storage_out ? 0 : 1; p.bias[0] = bias_dev; p.out = out_dev;
  if (storage_out) {  // (fp8 operands store bf16) every element is the launch's: nothing to narrow
    MD_TRY(ob.open(out_dev, (long)M * N, N, precision == MD_PREC_FP8 ? MD_PREC_BF16 : precision, s.st, false));
    p.out = ob.buf.p;
  }
  split_out(s.geom, p, N, storage_out);
  MD_TRY(launch_gemm(p, A_DENSE, precision, tile, s.st));
  MD_TRY(ob.close(s.st));
  return s.finish();
}

// md_op_attention (V = 1), md_op_attention_views and md_op_attention_ex: one staging, one launcher
static int op_attention(md_device_t dev, const md_attention_op& d, void* stream) {
  const float* qkv_dev = d.qkv;
  const int T = d.T, V = d.V, N = d.N, heads = d.heads;
  if (!dev || !qkv_dev || !d.out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (T <= 0 || N <= 0 || heads <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  if (V < 1 || T % V != 0) MD_FAIL(MD_ERR_SHAPE, "%d sequences in groups of %d views", T, V);
  // MD_OP_POISON_PAD / poison_pad: whatever the staging does not write (rows N .. S of every sequence, the slack rows, columns N .. kpad
  // of V^T) holds a large finite value (0x7000: 8192 as a half, 1.6e29 as bf16) instead of zero
  const bool poison = (d.precision & MD_OP_POISON_PAD) != 0 || d.poison_pad != 0;
  const int precision = d.precision & ~MD_OP_POISON_PAD;
  if (poison && precision == MD_PREC_F32) MD_FAIL(MD_ERR_UNSUPPORTED, "MD_OP_POISON_PAD fills 16-bit staging tensors");
  if (V > 1 && precision == MD_PREC_F32) MD_FAIL(MD_ERR_UNSUPPORTED, "cross-view attention runs in the bf16, f16 and f16x2 modes");
  const bool fp8_out = d.out_fp8_inv > 0.f;
  if (!(d.out_fp8_inv >= 0.f)) MD_FAIL(MD_ERR_INVALID_ARG, "out_fp8_inv must be >= 0");
  if (fp8_out && precision != MD_PREC_BF16) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: e4m3 output rows are built for bf16 operands");
  if (fp8_out && V > 1) MD_FAIL(MD_ERR_UNSUPPORTED, "cross-view attention writes plain output rows");
  if (d.small != -1 && d.small != 0) MD_FAIL(MD_ERR_INVALID_ARG, "small: -1 (the launcher's rule) or 0 (off)");
  // the strides, validated as the launchers validate them (the buffers below are sized from them before any launcher sees them)
  const int D = heads * 64, SS = d.seq_stride ? d.seq_stride : (N + 3) / 4 * 4, kpad = d.kpad ? d.kpad : (N + 63) / 64 * 64;
  if (SS < N) MD_FAIL(MD_ERR_SHAPE, "attention: %d tokens in sequences of %d rows", N, SS);
  if (kpad % 64 != 0 || kpad < (N + 63) / 64 * 64) MD_FAIL(MD_ERR_INVALID_ARG, "attention: kpad=%d must be a multiple of 64 covering %d keys", kpad, N);
  // the fp32 path's score GEMM writes S columns into rows of kpad floats
  if (precision == MD_PREC_F32 && (SS % 4 != 0 || SS > kpad)) MD_FAIL(MD_ERR_INVALID_ARG, "attention (fp32): seq_stride=%d must be a multiple of 4 within kpad=%d", SS, kpad);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  hipStream_t st = s.st;
  const size_t es = s.es();
  DevBuf qk, vT, ao, sc;
  MD_TRY(qk.alloc(((size_t)T * SS + 64) * 2 * D * es));
  MD_TRY(vT.alloc((size_t)T * heads * 64 * kpad * es));
  MD_TRY(ao.alloc(((size_t)T * SS + 64) * D * es));
  if (poison) {
    MD_HIP(hipMemsetD16Async((hipDeviceptr_t)qk.p, 0x7000, ((size_t)T * SS + 64) * 2 * D * es / 2, st));
    MD_HIP(hipMemsetD16Async((hipDeviceptr_t)vT.p, 0x7000, (size_t)T * heads * 64 * kpad * es / 2, st));
  }
  MD_TRY(launch_qkv_split(qkv_dev, T, N, heads, SS, kpad, qk.p, vT.p, attn_qscale(precision), precision, st));
  attention_note_form(ATTN_FORM_NONE, 0, 0, 0);
  if (precision != MD_PREC_F32) {
    DevBuf redo;  // zeroed flags: 577-token bf16 launches take the assembly kernel, like the model's
    MD_TRY(redo.alloc((size_t)attention_redo_ints(T * heads) * 4));
    if (precision == MD_PREC_BF16) MD_TRY(attention_asm_prepare());
    const long v_plane = (long)T * heads * 64 * kpad;
    std::optional<AttnSmallScope> small_off;  // small = -1: the thread's own setting stays
    if (d.small == 0) small_off.emplace(0);
    if (fp8_out) MD_TRY(launch_attention(qk.p, vT.p, ao.p, T, SS, N, heads, D, kpad, precision, st, d.out_fp8_inv, v_plane, (int*)redo.p));
    else MD_TRY(launch_attention_views(qk.p, vT.p, ao.p, T, V, SS, N, heads, D, kpad, precision, st, v_plane, (int*)redo.p));
    MD_HIP(hipStreamSynchronize(st));  // `redo` is released at the end of this scope
  } else {
    MD_TRY(sc.alloc((size_t)T * heads * SS * kpad * 4));
    MD_TRY(attention_f32(nullptr, st, qk.p, vT.p, ao.p, (float*)sc.p, T, SS, N, heads, kpad));
  }
  if (fp8_out)  // e4m3 rows of D bytes: the N valid rows of every sequence, as they are
    MD_HIP(hipMemcpy2DAsync(d.out, (size_t)N * D, ao.p, (size_t)SS * D, (size_t)N * D, (size_t)T, hipMemcpyDeviceToDevice, st));
  else
    MD_TRY(launch_unpad_rows(ao.p, T, N, SS, D, (float*)d.out, precision, st));
  return s.finish();
}

static md_attention_op attention_op_of(const float* qkv_dev, int T, int V, int N, int heads, int precision, float* out_dev) {
  md_attention_op d;
  memset(&d, 0, sizeof(d));
  d.T = T; d.V = V; d.N = N; d.heads = heads; d.precision = precision; d.small = -1;
  d.qkv = qkv_dev; d.out = out_dev;
  return d;
}

int md_op_attention(md_device_t dev, const float* qkv_dev, int T, int N, int heads, int precision, float* out_dev, void* stream) {
  return op_attention(dev, attention_op_of(qkv_dev, T, 1, N, heads, precision, out_dev), stream);
}

int md_op_attention_views(md_device_t dev, const float* qkv_dev, int T, int V, int N, int heads, int precision, float* out_dev, void* stream) {
  return op_attention(dev, attention_op_of(qkv_dev, T, V, N, heads, precision, out_dev), stream);
}

int md_op_attention_ex(md_device_t dev, const md_attention_op* desc, void* stream) {
  if (!desc) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  return op_attention(dev, *desc, stream);
}

int md_debug_attention_last_form(int out[4]) {
  if (!out) return MD_ERR_INVALID_ARG;
  const AttnForm f = attention_last_form();
  out[0] = f.form; out[1] = f.grid; out[2] = f.qw; out[3] = f.ks;
  return MD_OK;
}

int md_op_conv3x3(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B, int Cin, int H, int W,
                  int Cout, int pre_relu, int precision, float* out_dev, void* stream) {
  if (!dev || !x_dev || !w_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  const bool storage_out = (precision & MD_OP_STORAGE_OUT) && (precision & 0xff) != MD_PREC_F32;
  precision &= 0xff;
  if (Cin % ke_of(precision) != 0 || Cout % 4 != 0)
    MD_FAIL(MD_ERR_UNSUPPORTED, "conv3x3: Cin=%d must be a multiple of %d and Cout=%d of 4", Cin, ke_of(precision), Cout);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  DevBuf xa, wa, oa;
  MD_TRY(wa.alloc((size_t)Cout * 9 * Cin * esz_of(precision) * (s.split ? 3 : 1)));
  MD_TRY(oa.alloc((size_t)B * H * W * Cout * 4));
  MD_TRY(s.zero_page());
  MD_TRY(s.nhwc_a(x_dev, B, Cin, H, W, pre_relu, xa));
  MD_TRY(s.terms_of(w_dev, (long)Cout * Cin * 9));
  PackEntry e;
  e.kind = PACK_CONV3; e.d0 = Cout; e.d1 = Cin; e.k = 3; e.kp = Cin;
  MD_TRY(s.conv_w(w_dev, e, wa));
  const ConvW cw{wa.p, bias_dev};
  GemmParams p = conv3_params(s.geom, B, xa.p, H, W, Cin, &cw, Cout, oa.p, Cout, ACT_NONE, nullptr, nullptr, nullptr);
  if (!storage_out) { p.out_f32 = 1; p.ldo = Cout; p.o_plane = 0; }  // an fp32 destination: one plane of Cout floats per pixel
  MD_TRY(launch_gemm(p, A_CONV3, precision, TILE_AUTO, s.st));
  MD_TRY(s.nchw_out(oa, B, Cout, H, W, storage_out, out_dev));
  return s.finish();
}

int md_op_deconv2x2(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B, int Cin, int H,
                    int W, int Cout, int precision, float* out_dev, void* stream) {
  if (!dev || !x_dev || !w_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  const bool storage_out = (precision & MD_OP_STORAGE_OUT) && (precision & 0xff) != MD_PREC_F32;
  precision &= 0xff;
  if (Cin % ke_of(precision) != 0 || Cout % 4 != 0)
    MD_FAIL(MD_ERR_UNSUPPORTED, "deconv: Cin=%d must be a multiple of %d and Cout=%d of 4", Cin, ke_of(precision), Cout);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  DevBuf xa, wa, oa;
  MD_TRY(wa.alloc((size_t)4 * Cout * Cin * esz_of(precision) * (s.split ? 3 : 1)));
  MD_TRY(oa.alloc((size_t)B * 4 * H * W * Cout * 4));
  MD_TRY(s.nhwc_a(x_dev, B, Cin, H, W, 0, xa));
  MD_TRY(s.terms_of(w_dev, (long)Cin * Cout * 4));
  PackEntry e;
  e.kind = PACK_DECONV; e.d0 = Cin; e.d1 = Cout; e.k = 2; e.kp = Cin;
  MD_TRY(s.conv_w(w_dev, e, wa));
  GemmParams p = deconv2_params(s.geom, B, xa.p, Cin, nullptr, H, W, wa.p, Cin, Cout, bias_dev, oa.p, Cout, 0);
  if (!storage_out) { p.out_f32 = 1; p.ldo = Cout; p.o_plane = 0; }  // an fp32 destination: one plane of Cout floats per pixel
  MD_TRY(launch_gemm(p, A_DENSE, precision, TILE_AUTO, s.st));
  MD_TRY(s.nchw_out(oa, B, Cout, 2 * H, 2 * W, storage_out, out_dev));
  return s.finish();
}

int md_op_conv2d_direct(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, int B, int Cin, int H,
                        int W, int Cout, int k, int stride, int pad, int relu, float* out_dev, void* stream) {
  if (!dev || !x_dev || !w_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || k <= 0 || stride <= 0 || pad < 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  const int OH = (H + 2 * pad - k) / stride + 1, OW = (W + 2 * pad - k) / stride + 1;
  if (H + 2 * pad < k || W + 2 * pad < k) MD_FAIL(MD_ERR_SHAPE, "input %dx%d smaller than kernel %d", H, W, k);
  OpStage s;
  MD_TRY(s.open(dev, stream, MD_PREC_F32));
  DevBuf xa, wa, oa;
  MD_TRY(wa.alloc((size_t)Cout * k * k * Cin * 4));
  MD_TRY(oa.alloc((size_t)B * OH * OW * Cout * 4));
  MD_TRY(s.nhwc_a(x_dev, B, Cin, H, W, 0, xa));
  PackEntry e;
  e.kind = PACK_DIRECT; e.d0 = Cout; e.d1 = Cin; e.k = k; e.kp = Cin; e.f32 = 1;
  MD_TRY(s.conv_w(w_dev, e, wa));
  MD_TRY(launch_conv_direct(xa.p, MD_PREC_F32, nullptr, B, H, W, Cin, (const float*)wa.p, bias_dev, Cout, k, stride, pad, relu,
                            (float*)oa.p, s.st));
  MD_TRY(s.nchw_out(oa, B, Cout, OH, OW, false, out_dev));
  return s.finish();
}

// ---- the Depth-Anything-v3 token kernels alone ----
namespace {
struct RopeDev {  // the model's tables of one grid, uploaded for one call
  DevBuf cos, sin;
  int build(int n_tokens, int pw, float base) {
    std::vector<float> rc, rs;
    da3_rope_tables((n_tokens - 1) / pw, pw, base, &rc, &rs);
    MD_TRY(cos.alloc(rc.size() * 4));
    MD_TRY(sin.alloc(rs.size() * 4));
    MD_HIP(hipMemcpy(cos.p, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    MD_HIP(hipMemcpy(sin.p, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
    return MD_OK;
  }
};
int check_token_grid(const char* op, int T, int S, int n_tokens, int D, int pw) {
  if (T <= 0 || n_tokens <= 0 || S < n_tokens || D <= 0 || D % 64 != 0) MD_FAIL(MD_ERR_SHAPE, "%s: T=%d S=%d n_tokens=%d D=%d", op, T, S, n_tokens, D);
  if (pw <= 0 || (n_tokens - 1) % pw != 0) MD_FAIL(MD_ERR_SHAPE, "%s: %d patches do not fill rows of %d", op, n_tokens - 1, pw);
  return MD_OK;
}
}  // namespace

int md_op_qkv_norm_rope(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, const float* q_gamma,
                        const float* q_beta, const float* k_gamma, const float* k_beta, int T, int S, int n_tokens, int K, int D, int pw,
                        int global_pos, float rope_frequency, float eps, int precision, int tile, int form, float* qk_out, float* vt_out,
                        void* stream) {
  if (!dev || !x_dev || !w_dev || !bias_dev || !q_gamma || !q_beta || !k_gamma || !k_beta || !qk_out || !vt_out)
    MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (form != 0 && form != 1) MD_FAIL(MD_ERR_INVALID_ARG, "form = %d (0: GEMM + kernel, 1: fused epilogue)", form);
  MD_TRY(check_token_grid("qkv_norm_rope", T, S, n_tokens, D, pw));
  if (K <= 0 || K % ke_of(precision) != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "K=%d must be a multiple of %d", K, ke_of(precision));
  // no k-split: the fused epilogue never runs it (pick_ksplit), so the plain GEMM of form 0 keeps the same summation order and the
  // V tiles of the two forms can be compared bit for bit
  const KsplitScope ksplit(0);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  hipStream_t st = s.st;
  const int heads = D / 64, kpad = (S + 63) / 64 * 64, N = 3 * D;
  const long rows = (long)T * S;
  const size_t es = s.es(), vt_elems = (size_t)T * heads * 64 * kpad;
  if (vt_elems >= ((size_t)1 << 31) || rows * 2 * D >= (1L << 31)) MD_FAIL(MD_ERR_UNSUPPORTED, "qkv_norm_rope: tensors of this size are not a test");
  DevBuf xa, wa, ws, qk, vT;  // (ws: the e4m3 scales of OpStage::dense_w, never filled here)
  RopeDev rope;
  GemmParams p;
  MD_TRY(wa.alloc((size_t)N * K * esz_of(precision) * (s.split ? 3 : 1)));
  MD_TRY(qk.alloc(((size_t)rows + 64) * 2 * D * es));
  MD_TRY(vT.alloc(vt_elems * es));
  MD_TRY(rope.build(n_tokens, pw, rope_frequency));
  MD_TRY(s.terms_of(w_dev, (long)N * K));
  MD_TRY(s.dense_a(x_dev, rows, K, xa, &p.ascale));
  MD_TRY(s.dense_w(w_dev, N, K, wa, ws));
  p.N = N; p.ngroups = 1; p.g_rows[0] = (int)rows; p.W[0] = wa.p; p.A = xa.p;
  split_dense_a(s.geom, p, K, K, 0);
  p.bias[0] = bias_dev;
  p.v_plane = s.split ? (long)vt_elems : 0;
  p.epi = EPI_QKV; p.out = qk.p; p.vT = vT.p; p.seq_stride = S; p.embed = D; p.heads = heads; p.kpad = kpad; p.qscale = attn_qscale(precision);
  if (form == 1) {
    p.qkn_g[0] = q_gamma; p.qkn_b[0] = q_beta; p.qkn_g[1] = k_gamma; p.qkn_b[1] = k_beta;
    p.qkn_eps = eps; p.rope_cos = (const float*)rope.cos.p; p.rope_sin = (const float*)rope.sin.p;
    p.rope_pw = pw; p.rope_global = global_pos ? 1 : 0; p.rope_ntok = n_tokens;
  } else if (tile != TILE_AUTO && tile != TILE_64x64 && tile != TILE_128x64) {
    MD_FAIL(MD_ERR_UNSUPPORTED, "qkv_norm_rope: tile %d (the 64-column tiles or auto)", tile);
  }
  MD_TRY(launch_gemm(p, A_DENSE, precision, tile, st));
  if (form == 0)
    MD_TRY(launch_qk_norm_rope(qk.p, rows, S, n_tokens, D, heads, pw, q_gamma, q_beta, k_gamma, k_beta, eps, (const float*)rope.cos.p,
                               (const float*)rope.sin.p, global_pos ? 1 : 0, attn_qscale(precision), precision, st));
  // q | k rows: split-half [q_hi | q_lo | k_hi | k_lo] reads as 2 * rows rows of [hi: D | lo: D]
  MD_TRY(launch_rows_to_f32(qk.p, rows * 2 * D, qk_out, precision, st, D));
  MD_TRY(launch_rows_to_f32(vT.p, (long)vt_elems, vt_out, precision, st, (int)vt_elems));
  return s.finish();
}

int md_op_qk_norm_rope(md_device_t dev, const float* qk_in, const float* q_gamma, const float* q_beta, const float* k_gamma,
                       const float* k_beta, int T, int S, int n_tokens, int D, int pw, int global_pos, float rope_frequency, float eps,
                       int precision, float* qk_out, void* stream) {
  if (!dev || !qk_in || !q_gamma || !q_beta || !k_gamma || !k_beta || !qk_out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  MD_TRY(check_token_grid("qk_norm_rope", T, S, n_tokens, D, pw));
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  const long rows = (long)T * S;
  DevBuf qk;
  RopeDev rope;
  MD_TRY(qk.alloc((size_t)rows * 2 * D * s.es()));
  MD_TRY(rope.build(n_tokens, pw, rope_frequency));
  MD_TRY(launch_f32_to_rows(qk_in, rows * 2 * D, qk.p, precision, s.st, D));
  MD_TRY(launch_qk_norm_rope(qk.p, rows, S, n_tokens, D, D / 64, pw, q_gamma, q_beta, k_gamma, k_beta, eps, (const float*)rope.cos.p,
                             (const float*)rope.sin.p, global_pos ? 1 : 0, attn_qscale(precision), precision, s.st));
  MD_TRY(launch_rows_to_f32(qk.p, rows * 2 * D, qk_out, precision, s.st, D));
  return s.finish();
}

int md_op_hook_cat_ln(md_device_t dev, const float* x_local, const float* x, int T, int S, int n_tokens, int D, const float* norm_g,
                      const float* norm_b, float eps_final, const float* head_g, const float* head_b, float eps_head, int precision,
                      float* out, float* cam_out, void* stream) {
  if (!dev || !x_local || !x || !norm_g || !norm_b || !head_g || !head_b || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (T <= 0 || n_tokens <= 0 || S < n_tokens || D <= 0) MD_FAIL(MD_ERR_SHAPE, "hook_cat_ln: T=%d S=%d n_tokens=%d D=%d", T, S, n_tokens, D);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  const long rows = (long)T * S;
  StorageOut ob;
  MD_TRY(ob.open(out, rows * 2 * D, 2 * D, precision, s.st));
  MD_TRY(launch_hook_cat_ln(x_local, x, rows, S, n_tokens, D, norm_g, norm_b, eps_final, head_g, head_b, eps_head, ob.buf.p, cam_out, precision, s.st));
  MD_TRY(ob.close(s.st));
  return s.finish();
}

int md_op_patchify(md_device_t dev, const float* x_dev, int B, int H, int W, int ps, int Kp, int precision, float* out, float* cls_x,
                   int S, int n_tokens, int D, const float* cls, const float* pos0, void* stream) {
  if (!dev || !x_dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (B <= 0 || H <= 0 || W <= 0 || ps <= 0 || H % ps || W % ps || Kp < 3 * ps * ps) MD_FAIL(MD_ERR_SHAPE, "patchify: %dx%d / patch %d / K %d", H, W, ps, Kp);
  if (cls_x && n_tokens != 1 + (H / ps) * (W / ps)) MD_FAIL(MD_ERR_SHAPE, "patchify: n_tokens = %d for a %dx%d grid", n_tokens, H / ps, W / ps);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  StorageOut ob;  // every element is the launch's: nothing to narrow
  MD_TRY(ob.open(out, (long)B * (H / ps) * (W / ps) * Kp, Kp, precision, s.st, false));
  MD_TRY(launch_patchify(x_dev, B, H, W, ps, Kp, ob.buf.p, precision, s.st, cls_x, S, n_tokens, D, cls, pos0));
  MD_TRY(ob.close(s.st));
  return s.finish();
}

int md_op_set_token0(md_device_t dev, float* x, int nseq, int S, int D, const float* src, int src_stride, void* stream) {
  if (!dev || !x || !src) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (nseq <= 0 || S <= 0 || D <= 0 || src_stride < 0) MD_FAIL(MD_ERR_SHAPE, "set_token0: nseq=%d S=%d D=%d stride=%d", nseq, S, D, src_stride);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_set_token0(x, nseq, S, D, src, s.st, src_stride));
  return s.finish();
}

int md_op_border_bias_fix(md_device_t dev, float* map, int B, int H, int W, int C, int ld, const float* bias9, int precision, void* stream) {
  if (!dev || !map || !bias9) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (B <= 0 || H < 2 || W < 2 || C <= 0 || ld < C) MD_FAIL(MD_ERR_SHAPE, "border_bias_fix: [%d,%d,%d] C=%d ld=%d", B, H, W, C, ld);
  OpStage s;
  MD_TRY(s.open(dev, stream, precision));
  StorageOut mb;
  MD_TRY(mb.open(map, (long)B * H * W * ld, ld, precision, s.st));
  MD_TRY(launch_border_bias_fix(mb.buf.p, B, H, W, C, ld, bias9, precision, s.st));
  MD_TRY(mb.close(s.st));
  return s.finish();
}

// ---- the layer compositions of model_commit alone: the fp32 product a pack is made from, before pack_weight rounds it ----
int md_op_compose_weights(md_device_t dev, int kind, int cin, int cmid, int cout, const float* w_first, const float* w_second,
                          const float* bias_first, const float* bias_second, float* out, float* bias9_out, void* stream) {
  if (!dev || !w_first || !w_second || !out) MD_FAIL(MD_ERR_INVALID_ARG, "compose_weights: null argument");
  if (kind < MD_COMPOSE_DECONV_CONV || kind > MD_COMPOSE_HEAD) MD_FAIL(MD_ERR_INVALID_ARG, "compose_weights: kind %d", kind);
  if (cin <= 0 || cmid <= 0 || cout <= 0) MD_FAIL(MD_ERR_SHAPE, "compose_weights: channels %d -> %d -> %d", cin, cmid, cout);
  const bool any_bias = bias_first || bias_second || bias9_out;
  if (any_bias && (kind == MD_COMPOSE_DECONV_CONV || kind == MD_COMPOSE_DECONV_PAIR))
    MD_FAIL(MD_ERR_INVALID_ARG, "compose_weights: kind %d has no bias classes (the first layer is bias-free, the 1x1's bias rides on the launch)", kind);
  if (any_bias && !(bias_first && bias_second && bias9_out))
    MD_FAIL(MD_ERR_INVALID_ARG, "compose_weights: the bias classes need both layers' biases and bias9_out");
  const int taps = kind == MD_COMPOSE_DECONV_CONV ? 4 : (kind == MD_COMPOSE_DECONV_PAIR ? 16 : (kind == MD_COMPOSE_C1C3 ? 9 : 36));
  if ((long)cin * cout * taps >= (1L << 31) || (long)cin * cmid * 4 >= (1L << 31) || (long)cmid * cout * 9 >= (1L << 31))
    MD_FAIL(MD_ERR_UNSUPPORTED, "compose_weights: tensors of this size are not a test");
  OpStage s;
  MD_TRY(s.open(dev, stream));
  switch (kind) {
    case MD_COMPOSE_DECONV_CONV: MD_TRY(compose_deconv_conv(w_first, w_second, cin, cmid, cout, out, s.st)); break;
    case MD_COMPOSE_DECONV_PAIR: MD_TRY(compose_deconv_pair(w_first, w_second, cin, cmid, cout, out, s.st)); break;
    case MD_COMPOSE_C1C3: MD_TRY(compose_c1c3(w_first, w_second, cin, cmid, cout, out, s.st)); break;
    default: MD_TRY(compose_head(w_first, w_second, cin, cmid, cout, out, s.st)); break;
  }
  // PACK_C1C3_B / PACK_HEAD_B: the second layer's 3x3 weight, the first layer's bias, the second layer's bias
  if (bias9_out) MD_TRY(compose_head_bias(w_second, bias_first, bias_second, cmid, cout, bias9_out, s.st));
  return s.finish();
}

// ---- the kernels that write MFMA operands, alone: the caller's buffers hold the stored bytes (no widened copy) ----
int md_op_layernorm_ex(md_device_t dev, float* x, int rows, int D, int S, int ngroups, const int* seq0, const int* nseq,
                       const float* const* gamma, const float* const* beta, float eps, int precision, int out_f32, float fp8_inv_scale,
                       const float* tok0, int tok0_stride, void* out, void* stream) {
  if (!dev || !x || !out || !seq0 || !nseq || !gamma || !beta) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision) && precision != MD_PREC_FP8) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (rows <= 0 || D <= 0 || S <= 0 || tok0_stride < 0) MD_FAIL(MD_ERR_SHAPE, "layernorm_ex: rows=%d D=%d S=%d stride=%d", rows, D, S, tok0_stride);
  if (ngroups < 1 || ngroups > 4) MD_FAIL(MD_ERR_INVALID_ARG, "layernorm_ex: %d groups (1..4)", ngroups);
  SeqGroups g;
  memset(&g, 0, sizeof(g));
  g.ngroups = ngroups;
  int next = 0;
  for (int i = 0; i < ngroups; ++i) {  // consecutive sequence ranges from 0, as the engine builds them
    if (seq0[i] != next || nseq[i] <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "layernorm_ex: group %d = [%d, +%d) does not follow sequence %d", i, seq0[i], nseq[i], next);
    if (gamma[i] && !beta[i]) MD_FAIL(MD_ERR_INVALID_ARG, "layernorm_ex: group %d has gamma but no beta", i);
    g.seq0[i] = seq0[i]; g.nseq[i] = nseq[i]; g.a[i] = gamma[i]; g.b[i] = beta[i];
    next += nseq[i];
  }
  if ((long)next * S < rows) MD_FAIL(MD_ERR_SHAPE, "layernorm_ex: %d sequences of %d rows do not cover %d rows", next, S, rows);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_layernorm(x, out, rows, D, eps, S, g, precision, out_f32, s.st, fp8_inv_scale, tok0, tok0_stride, tok0 ? x : nullptr));
  return s.finish();
}

int md_op_store_rows(md_device_t dev, const float* in, int64_t count, int width, int precision, void* out, void* stream) {
  if (!dev || !in || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (count <= 0 || width < 0) MD_FAIL(MD_ERR_SHAPE, "store_rows: count=%lld width=%d", (long long)count, width);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_f32_to_rows(in, (long)count, out, precision, s.st, width));
  return s.finish();
}

int md_op_load_rows(md_device_t dev, const void* in, int64_t count, int width, int precision, float* out, void* stream) {
  if (!dev || !in || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (count <= 0 || width < 0) MD_FAIL(MD_ERR_SHAPE, "load_rows: count=%lld width=%d", (long long)count, width);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_rows_to_f32(in, (long)count, out, precision, s.st, width));
  return s.finish();
}

int md_op_f32_to_fp8(md_device_t dev, const float* in, int64_t count, float inv_scale, void* out, void* stream) {
  if (!dev || !in || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (count <= 0) MD_FAIL(MD_ERR_SHAPE, "f32_to_fp8: count=%lld", (long long)count);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_f32_to_fp8(in, (long)count, inv_scale, out, s.st));
  return s.finish();
}

int md_op_pack_fp8_rows(md_device_t dev, const float* w, int N, int K, int Kp, void* out, float* scale, void* stream) {
  if (!dev || !w || !out || !scale) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (N <= 0 || K <= 0) MD_FAIL(MD_ERR_SHAPE, "pack_fp8_rows: N=%d K=%d", N, K);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_pack_fp8_rows(w, N, K, Kp, out, scale, s.st));
  return s.finish();
}

int md_op_nchw_to_nhwc(md_device_t dev, const float* in, int B, int C, int H, int W, int precision, int relu, int ld, void* out,
                       void* stream) {
  if (!dev || !in || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || ld < 0) MD_FAIL(MD_ERR_SHAPE, "nchw_to_nhwc: [%d,%d,%d,%d] ld=%d", B, C, H, W, ld);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_nchw_to_nhwc(in, B, C, H, W, out, precision, relu ? 1 : 0, s.st, ld));
  return s.finish();
}

int md_op_nhwc_to_nchw(md_device_t dev, const void* in, int B, int C, int H, int W, int ld, int coff, int precision, float* out,
                       void* stream) {
  if (!dev || !in || !out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "nhwc_to_nchw: [%d,%d,%d,%d]", B, C, H, W);
  if (coff < 0 || ld < coff + C) MD_FAIL(MD_ERR_INVALID_ARG, "nhwc_to_nchw: channels [%d, %d) outside a pixel of %d", coff, coff + C, ld);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_nhwc_to_nchw(in, B, C, H, W, ld, coff, out, precision, s.st));
  return s.finish();
}

int md_op_ln_fold_vectors(md_device_t dev, const float* w, const float* gamma, const float* beta, const float* bias, int N, int K,
                          int precision, float* c, float* d, void* stream) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", precision);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_ln_fold_vectors(w, gamma, beta, bias, N, K, precision, c, d, s.st));
  return s.finish();
}

int md_op_ln_finish(md_device_t dev, const float* parts, int64_t rows, float inv_n, float eps, float* ab, void* stream) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_ln_finish(parts, ab, (long)rows, inv_n, eps, s.st));
  return s.finish();
}

// ---- the GEMM forms of the ViT token stream alone ----
int md_op_vit_gemm(md_device_t dev, const md_vit_gemm* d, void* stream) {
  if (!dev || !d || !d->a) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const int prec = d->precision, kind = d->kind, N = d->N, K = d->K, G = d->ngroups;
  if (!token_op_prec(prec) && !(prec == MD_PREC_FP8 && kind == MD_VIT_GEMM_RESID)) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: kind %d has no precision %d", kind, prec);
  if (kind < MD_VIT_GEMM_RESID || kind > MD_VIT_GEMM_PATCH_EMBED) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: kind %d", kind);
  if (G < 1 || G > kMaxGroups) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: %d groups (1..%d)", G, kMaxGroups);
  if (N <= 0 || N % 4 != 0 || K <= 0 || K % ke_of(prec) != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "vit_gemm: N=%d (x4), K=%d (x%d)", N, K, ke_of(prec));
  if (d->a_rows <= 0 || d->out_rows <= 0) MD_FAIL(MD_ERR_SHAPE, "vit_gemm: a_rows=%d out_rows=%d", d->a_rows, d->out_rows);
  const bool patch = kind == MD_VIT_GEMM_PATCH_EMBED, resid = kind == MD_VIT_GEMM_RESID, qkv = kind == MD_VIT_GEMM_QKV;
  const bool producer = resid && d->g[0].gamma_next, consumer = (qkv || kind == MD_VIT_GEMM_FC1) && d->g[0].c;
  // the row space the groups' output rows live in: patch rows for the patch embedding (x row = seq * S + 1 + p), else rows of the outputs
  long row_space = d->out_rows;
  if (patch) {
    if (d->P <= 0 || d->S < 1 + d->P || d->out_rows % d->S != 0 || !d->x) MD_FAIL(MD_ERR_SHAPE, "vit_gemm: patch embed P=%d S=%d rows=%d", d->P, d->S, d->out_rows);
    row_space = (long)(d->out_rows / d->S) * d->P;
  }
  // fold consumer and V^T store: four-row groups all inside or all outside a weight group, as the token buffers (rows padded to x4) give them
  const int row_mult = (consumer || qkv) ? 4 : 1;
  for (int g = 0; g < G; ++g) {
    const md_vit_gemm_group& q = d->g[g];
    if (!q.w || !q.bias) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: group %d has no weight / bias", g);
    if (q.rows <= 0 || q.row0 < 0 || (long)q.row0 + q.rows > row_space || q.arow0 < 0 || (long)q.arow0 + q.rows > d->a_rows)
      MD_FAIL(MD_ERR_SHAPE, "vit_gemm: group %d = rows [%d, +%d) from A row %d outside %ld output / %d A rows", g, q.row0, q.rows, q.arow0, row_space, d->a_rows);
    if (q.rows % row_mult != 0 || q.row0 % row_mult != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "vit_gemm: group %d: rows [%d, +%d) must be multiples of %d here", g, q.row0, q.rows, row_mult);
    if (resid && !q.scale) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: group %d has no LayerScale", g);
    if (patch && !q.pos) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: group %d has no position table", g);
    if ((resid && !q.gamma_next != !producer) || (!resid && !patch && !q.c != !consumer)) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: the LayerNorm fold is for every group or for none");
  }
  if (producer || consumer) {  // (gemm256_form refuses the rest; the smaller tiles would silently ignore the fold's fields)
    if (d->tile != TILE_256x256 || N % 256 != 0 || prec == MD_PREC_F32 || prec == MD_PREC_FP8) MD_FAIL(MD_ERR_UNSUPPORTED, "vit_gemm: the LayerNorm fold runs on the 256 x 256 kernel, 16-bit operands, N %% 256 == 0");
    if (producer && (!d->ln_out || !d->ln_stats_out)) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: fold producer outputs missing");
    if (consumer && (!d->ln_stats || (d->ln_raw && K != 1024))) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: fold consumer statistics missing (raw partials: four per row, K = 1024)");
  }
  const int D = d->D, S = d->S, heads = D / 64, kpad = (S + 63) / 64 * 64;
  size_t vt_elems = 0;
  if (resid && !d->x) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: x missing");
  if (kind == MD_VIT_GEMM_FC1 && !d->out) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: out missing");
  if (qkv) {
    if (!d->qk || !d->vT) MD_FAIL(MD_ERR_INVALID_ARG, "vit_gemm: qk / vT missing");
    if (D <= 0 || D % 64 != 0 || N != 3 * D || S <= 0 || S % 4 != 0 || d->out_rows % S != 0) MD_FAIL(MD_ERR_SHAPE, "vit_gemm: qkv N=%d D=%d S=%d rows=%d", N, D, S, d->out_rows);
    vt_elems = (size_t)(d->out_rows / S) * heads * 64 * kpad;
    if (vt_elems >= ((size_t)1 << 31) || (long)d->out_rows * 2 * D >= (1L << 31)) MD_FAIL(MD_ERR_UNSUPPORTED, "vit_gemm: tensors of this size are not a test");
  }
  const KsplitScope ksplit(1);  // as md_op_linear_tile: the k-split form of the 64 x 64 kernel is what the DA3 engine runs
  OpStage s;
  MD_TRY(s.open(dev, stream, prec));
  hipStream_t st = s.st;
  const bool split = s.split;
  const int xm = s.geom.xm;

  // ---- operands ----
  DevBuf xa, wa[kMaxGroups], ws[kMaxGroups];
  GemmParams p;
  for (int g = 0; g < G; ++g) MD_TRY(s.terms_of(d->g[g].w, (long)N * K));
  MD_TRY(s.dense_a(d->a, d->a_rows, K, xa, &p.ascale));
  for (int g = 0; g < G; ++g) {
    const md_vit_gemm_group& q = d->g[g];
    MD_TRY(wa[g].alloc((size_t)N * K * esz_of(prec) * split_terms(s.geom, 0)));
    MD_TRY(s.dense_w(q.w, N, K, wa[g], ws[g]));
    p.g_row0[g] = q.row0; p.g_rows[g] = q.rows; p.g_arow0[g] = q.arow0;
    p.W[g] = wa[g].p; p.wscale[g] = (const float*)ws[g].p; p.bias[g] = q.bias; p.scale[g] = q.scale; p.pos[g] = q.pos;
    if (producer) p.ln_gamma[g] = q.gamma_next;
    if (consumer) p.ln_c[g] = q.c;
  }
  p.N = N; p.ngroups = G; p.A = xa.p;
  split_dense_a(s.geom, p, K, K, 0);
  if (consumer) {
    p.ln_stats = d->ln_stats; p.ln_raw = d->ln_raw ? 1 : 0; p.ln_parts = K / 256; p.ln_inv_n = d->ln_inv_n; p.ln_eps = d->ln_eps;
  }

  // ---- the epilogue and its outputs ----
  StorageOut o1, o2;
  const long rows = d->out_rows;
  if (resid) {
    p.epi = EPI_RESID_LS;
    split_out(s.geom, p, N, false);
    p.out = d->x_out ? d->x_out : d->x;
    p.resid_src = d->x_out ? d->x : nullptr;
    if (producer) {
      MD_TRY(o1.open(d->ln_out, rows * N, N, prec, st));
      p.ln_out = o1.buf.p; p.ln_ldo = (long)N * xm; p.ln_plane = split ? N : 0;
      p.ln_stats_out = d->ln_stats_out; p.ln_parts = N / 256;
    }
  } else if (qkv) {
    MD_TRY(o1.open(d->qk, rows * 2 * D, D, prec, st));  // (no slack rows: every row is the caller's and returns to it) split-half rows [q_hi | q_lo | k_hi | k_lo] = 2 * rows rows of [hi: D | lo: D]
    MD_TRY(o2.open(d->vT, (long)vt_elems, (int)vt_elems, prec, st));     // split-half: the lo plane behind the whole hi plane
    p.epi = EPI_QKV; p.out = o1.buf.p; p.vT = o2.buf.p; p.v_plane = split ? (long)vt_elems : 0;
    p.seq_stride = S; p.embed = D; p.heads = heads; p.kpad = kpad; p.qscale = attn_qscale(prec);
  } else if (kind == MD_VIT_GEMM_FC1) {
    p.epi = EPI_STORE; p.act = ACT_GELU;
    if (prec == MD_PREC_F32) {
      p.out_f32 = 1; p.out = d->out;
    } else {
      MD_TRY(o1.open(d->out, rows * N, N, prec, st));
      p.out = o1.buf.p;
    }
    split_out(s.geom, p, N, !p.out_f32);
  } else {
    p.epi = EPI_PATCH_EMBED; p.out = d->x; p.seq_stride = S; p.seq_patches = d->P; p.embed = N;
    split_out(s.geom, p, N, false);
  }
  gemm_forget_form();
  MD_TRY(launch_gemm(p, A_DENSE, prec, d->tile, st));
  MD_TRY(o1.close(st));
  MD_TRY(o2.close(st));
  return s.finish();
}

// ---- the GEMM forms of the convolutional decoders and heads alone ----
int md_op_decoder_gemm(md_device_t dev, const md_decoder_gemm* d, void* stream) {
  if (!dev || !d || !d->in || !d->out || !d->w[0]) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const int prec = d->precision, kind = d->kind;
  if (!token_op_prec(prec)) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: the decoders run in bf16, f16, f16x2 and f32, not in precision %d", prec);
  if (kind < MD_DECODER_GEMM_CONV3 || kind > MD_DECODER_GEMM_HEAD_UP2) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: kind %d", kind);
  const bool conv = kind == MD_DECODER_GEMM_CONV3, s2 = kind == MD_DECODER_GEMM_CONV3_S2, ps = kind == MD_DECODER_GEMM_PIXSHUF;
  const bool head = kind == MD_DECODER_GEMM_HEAD, up2 = kind == MD_DECODER_GEMM_HEAD_UP2;
  const int B = d->B, H = d->H, W = d->W, Cin = d->Cin, Cin_p = d->Cin_p, Cout = d->Cout, G = conv ? d->ngroups : 1;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) MD_FAIL(MD_ERR_SHAPE, "decoder_gemm: [%d,%d,%d] %d -> %d channels", B, H, W, Cin, Cout);
  if (Cin_p < Cin || Cin_p % ke_of(prec) != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "decoder_gemm: Cin_p=%d must hold Cin=%d in whole k-tiles of %d", Cin_p, Cin, ke_of(prec));
  if (Cout % 4 != 0 || ((head || up2) && Cout != 32)) MD_FAIL(MD_ERR_UNSUPPORTED, "decoder_gemm: Cout=%d (x4; the head tails: 32)", Cout);
  if (G < 1 || G > 2 || (G == 2 && !d->w[1])) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: %d weight groups (1 or 2, each with a weight)", G);
  if (!conv && (d->res1 || d->res2 || d->res_mod)) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: residual inputs belong to CONV3");
  if (!conv && !ps && d->out2) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: a second output belongs to CONV3 and PIXSHUF");
  if (conv && d->res_mod && (G != 1 || !d->res1 || d->res_mod < 0)) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: res_mod wraps res1 of a one-group launch");
  if (conv && d->act != ACT_NONE && d->act != ACT_RELU) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: act %d", d->act);
  if ((conv || s2 || ps) && !(s2 && d->out_f32) && d->ldo < (ps ? d->ps_coff : 0) + Cout) MD_FAIL(MD_ERR_SHAPE, "decoder_gemm: %d channels at %d do not fit a pixel of %d", Cout, ps ? d->ps_coff : 0, d->ldo);
  if (d->out_f32 && !s2) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: the fp32 store is CONV3_S2's");
  if (ps && ((d->ps_f != 2 && d->ps_f != 4) || d->ps_coff < 0 || !d->bias[0])) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: pixel shuffle f=%d coff=%d (+ bias)", d->ps_f, d->ps_coff);
  if ((head || up2 || s2) && !d->bias[0]) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: bias missing");
  if (head && (d->head_nch < 0 || d->head_nch > 8)) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: %d head channels (0 .. 8)", d->head_nch);
  if (up2 && (d->Cmid <= 0 || !d->w2 || !d->bias2 || !d->head_w)) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: HEAD_UP2 needs Cmid, w2, bias2, head_w");
  if ((long)G * B * H * W * (ps ? d->ps_f * d->ps_f : 1) >= (1L << 31)) MD_FAIL(MD_ERR_UNSUPPORTED, "decoder_gemm: tensors of this size are not a test");
  const KsplitScope ksplit(1);  // (the Depth-Anything-v3 engine, whose head these forms are, runs with the k-split form allowed)
  OpStage s;
  MD_TRY(s.open(dev, stream, prec));
  hipStream_t st = s.st;
  const OperandGeom& geom = s.geom;  // (the term count: two when every plain weight of the launch is an exact half)
  DevBuf wa[2], composed, bias9;
  MD_TRY(s.zero_page());
  const int taps = ps ? d->ps_f * d->ps_f : 9;
  for (int g = 0; g < G && !up2; ++g) MD_TRY(s.terms_of(d->w[g], (long)Cout * Cin * taps));
  const int terms = up2 ? 3 : 0;  // (the composed head weight is a sum of products, never f16-exact: model_commit packs it in three terms)
  ConvW cw[2];
  for (int g = 0; g < G; ++g) {
    PackEntry e;
    e.kp = Cin_p;
    if (ps) { e.kind = PACK_DECONV; e.d0 = Cin; e.d1 = Cout; e.k = d->ps_f; }
    else { e.kind = PACK_CONV3; e.d0 = up2 ? 4 * Cout : Cout; e.d1 = Cin; e.k = 3; }
    MD_TRY(wa[g].alloc(pack_elems(e, split_terms(geom, terms)) * esz_of(prec)));
    const float* src = d->w[g];
    if (up2) {  // add_pack_fused(PACK_HEAD_W) as model_commit runs it: the product in fp32, then packed as a 3x3 convolution of 4 x 32 columns; PACK_HEAD_B: nine bias classes
      MD_TRY(composed.alloc((size_t)4 * Cout * Cin * 9 * 4));
      MD_TRY(bias9.alloc((size_t)9 * Cout * 4));
      MD_TRY(compose_head(d->w[0], d->w2, Cin, d->Cmid, Cout, (float*)composed.p, st));
      MD_TRY(compose_head_bias(d->w2, d->bias[0], d->bias2, d->Cmid, Cout, (float*)bias9.p, st));
      src = (const float*)composed.p;
    }
    MD_TRY(s.conv_w(src, e, wa[g], terms));
    cw[g] = ConvW{wa[g].p, up2 ? (const float*)bias9.p : d->bias[g]};
  }

  GemmParams p;
  int amode = A_CONV3;
  if (conv) {
    // md_engine_util.h conv3(): residual_unit's second convolution (res1 = x, res2 = the skip, out2 = the relu'd copy, two groups with
    // the shared input / residual), its first (ACT_RELU), the layerN_rn maps (md_da3.hip da3_prepare_stages: out2 only)
    p = conv3_params(geom, B, d->in, H, W, Cin_p, cw, Cout, d->out, d->ldo, d->act, d->res1, d->res2, d->out2, terms, G, d->in_shared != 0,
                     d->res1_shared != 0);
    if (d->res_mod) p.res_mod = d->res_mod;  // md_da3.hip da3_prepare_stages, the stage projection: `p.res_mod = P`, a table per image
  } else if (s2) {
    const int OH = (H + 2 - 3) / 2 + 1, OW = (W + 2 - 3) / 2 + 1;
    p.N = Cout; p.ngroups = 1; p.g_rows[0] = B * OH * OW;
    p.W[0] = cw[0].w; p.bias[0] = cw[0].b;
    p.A = d->in; p.cH = H; p.cW = W; p.cOH = OH; p.cOW = OW; p.cstride = 2; p.zero_page = geom.zero_page;
    split_conv_a(geom, p, Cin_p, 0);
    if (d->out_f32) {  // md_engine.hip run_fov, the downsampling convolution of the FOV head: ReLU, fp32 rows of Cout
      p.epi = EPI_STORE; p.act = ACT_RELU; p.out_f32 = 1; p.out = d->out; p.ldo = Cout;
    } else {           // md_da3.hip da3_prepare_stages, stage 3's resize
      p.epi = EPI_STORE; p.out = d->out;
      split_out(geom, p, d->ldo, true);
    }
  } else if (ps) {
    // md_engine_util.h deconv2(): the decoder's upsampling (f = 2, into a channel slice, with the relu'd copy) and the stage resizes of
    // md_da3.hip da3_prepare_stages (f = 4 | 2)
    p = deconv2_params(geom, B, d->in, Cin_p, nullptr, H, W, cw[0].w, Cin_p, Cout, cw[0].b, d->out, d->ldo, d->ps_coff, d->out2, d->ps_f, terms);
    amode = A_DENSE;
  } else if (head) {
    // md_da3.hip tail(): `nch` channels in one launch; head_nch == 0: the one-channel form of the same epilogue (GemmParams::head_w)
    p.N = 32; p.ngroups = 1; p.g_rows[0] = B * H * W; p.W[0] = cw[0].w;
    p.A = d->in; p.cH = H; p.cW = W; p.zero_page = geom.zero_page;
    split_conv_a(geom, p, Cin_p, 0);
    p.epi = EPI_HEAD; p.bias[0] = cw[0].b; p.head_nch = d->head_nch; p.head_plane = H * W;
    for (int i = 0; i < d->head_nch; ++i) {
      const md_decoder_gemm_head_ch& c = d->ch[i];
      if (!c.w || !c.out || c.bstride < (int64_t)H * W) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: head channel %d", i);
      p.head_wc[i] = c.w; p.head_bs[i] = c.b; p.head_acts[i] = c.act; p.head_out[i] = c.out; p.head_bstride[i] = (long)c.bstride;
    }
    if (d->head_nch == 0) {
      if (!d->head_w) MD_FAIL(MD_ERR_INVALID_ARG, "decoder_gemm: head_w missing");
      p.head_w = d->head_w; p.head_b = d->head_b; p.head_act = d->head_act; p.out = d->out;
    }
  } else {
    // md_engine.hip run_decoder_head, "head_tail_fused": deconv k2s2 -> conv1 3x3 -> relu -> conv_out 1x1 -> relu on conv0's output
    p.N = 4 * 32; p.ngroups = 1; p.g_rows[0] = B * H * W; p.W[0] = cw[0].w;
    p.A = d->in; p.cH = H; p.cW = W; p.zero_page = geom.zero_page;
    split_conv_a(geom, p, Cin_p, 3);
    p.epi = EPI_HEAD_UP2; p.bias[0] = cw[0].b; p.head_w = d->head_w;
    p.head_b = d->head_b;
    p.out = d->out;
  }
  // the tiles the call sites fix: tail() launches TILE_256x32, the composed head TILE_128x128; everything else TILE_AUTO
  int tile = d->tile;
  if (tile == TILE_AUTO && head) tile = TILE_256x32;
  if (tile == TILE_AUTO && up2) tile = TILE_128x128;
  gemm_forget_form();
  MD_TRY(launch_gemm(p, amode, prec, tile, st));
  return s.finish();
}

// ---- the gathered-row GEMM forms alone (A_INDEXED; index == NULL: the same parameters as A_DENSE) ----
int md_op_indexed_gemm(md_device_t dev, const md_indexed_gemm* d, void* stream) {
  if (!dev || !d || !d->a || !d->w || !d->out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const int prec = d->precision, kind = d->kind, M = d->M, N = d->N, K = d->K;
  if (!token_op_prec(prec)) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: gathered rows run in bf16, f16, f16x2 and f32, not in precision %d", prec);
  if (kind < MD_INDEXED_GEMM_ROWS || kind > MD_INDEXED_GEMM_PIXSHUF) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: kind %d", kind);
  const bool res = kind == MD_INDEXED_GEMM_ROWS_RES, ps = kind == MD_INDEXED_GEMM_PIXSHUF;
  const int f = ps ? d->ps_f : 1, coff = ps ? d->ps_coff : 0;
  if (M <= 0 || N <= 0 || K <= 0 || (d->index && d->rows_a <= 0)) MD_FAIL(MD_ERR_SHAPE, "indexed_gemm: M=%d N=%d K=%d over %d rows", M, N, K, d->rows_a);
  if (K % ke_of(prec) != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "indexed_gemm: K=%d must be whole k-tiles of %d", K, ke_of(prec));
  if (N % 4 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "indexed_gemm: N=%d (x4)", N);
  if (ps && ((f != 2 && f != 4) || coff < 0 || !d->bias || d->B <= 0 || d->ph <= 0 || d->pw <= 0 || (long)d->B * d->ph * d->pw != M))
    MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: pixel shuffle f=%d coff=%d (+ bias) of a [%d, %d, %d] map of %d rows", f, coff, d->B, d->ph, d->pw, M);
  if (ps && d->out_f32) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: the pixel shuffle stores T");
  if (res && (!d->res1 || d->res_mod <= 0 || d->out_f32)) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: ROWS_RES needs a T-typed output and res1 [res_mod, ldo]");
  if (!res && (d->res1 || d->res_mod)) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: a residual table belongs to ROWS_RES");
  if (d->ldo < coff + N) MD_FAIL(MD_ERR_SHAPE, "indexed_gemm: %d channels at %d do not fit a row of %d", N, coff, d->ldo);
  const long rows_out = (long)M * f * f;
  if (rows_out >= (1L << 31) || d->out_rows < rows_out || (double)d->out_rows * d->ldo >= 2147483648.0)
    MD_FAIL(MD_ERR_SHAPE, "indexed_gemm: the launch writes %ld rows, out holds %ld of %d", rows_out, (long)d->out_rows, d->ldo);
  const KsplitScope ksplit(res ? 1 : 0);  // (the stage projection is Depth-Anything-v3's, whose engine allows the k-split form; Depth Pro's does not)
  OpStage s;
  MD_TRY(s.open(dev, stream, prec));
  // every table entry inside a, checked on the host: a test's mistake must not become a stray device read
  if (d->index) {
    std::vector<int32_t> h((size_t)M);
    MD_HIP(hipStreamSynchronize(s.st));  // (the caller's table may still be in flight on its stream)
    MD_HIP(hipMemcpy(h.data(), d->index, (size_t)M * 4, hipMemcpyDeviceToHost));
    for (int m = 0; m < M; ++m)
      if (h[m] < 0 || h[m] >= d->rows_a) MD_FAIL(MD_ERR_INVALID_ARG, "indexed_gemm: index[%d] = %d outside [0, %d)", m, h[m], d->rows_a);
  }
  DevBuf xa, wa, ws, r1;
  StorageOut ob;
  float unused_scale = 0.f;
  MD_TRY(s.terms_of(d->w, (long)N * K * f * f));
  MD_TRY(s.dense_a(d->a, d->index ? d->rows_a : M, K, xa, &unused_scale));
  PackEntry e;
  e.kp = K;
  if (ps) { e.kind = PACK_DECONV; e.d0 = K; e.d1 = N; e.k = f; }
  else { e.kind = PACK_NK; e.d0 = N; e.d1 = K; e.k = 1; }
  MD_TRY(wa.alloc(pack_elems(e, split_terms(s.geom, 0)) * esz_of(prec)));
  MD_TRY(s.conv_w(d->w, e, wa));
  void* out = d->out;
  if (!d->out_f32) {
    MD_TRY(ob.open(d->out, (long)d->out_rows * d->ldo, d->ldo, prec, s.st));
    out = ob.buf.p;
  }
  if (res) {
    MD_TRY(r1.alloc((size_t)d->res_mod * d->ldo * s.es()));
    MD_TRY(launch_f32_to_rows(d->res1, (long)d->res_mod * d->ldo, r1.p, prec, s.st, d->ldo));
  }
  // lda == K in every engine launch of this mode (token rows of the ViT width)
  const GemmParams p = ps ? deconv2_params(s.geom, d->B, xa.p, K, d->index, d->ph, d->pw, wa.p, K, N, d->bias, out, d->ldo, coff, nullptr, f)
                          : rows_params(s.geom, xa.p, K, d->index, M, wa.p, N, K, d->bias, out, d->ldo, d->out_f32 ? 1 : 0, ACT_NONE, 0, r1.p, d->res_mod);
  gemm_forget_form();
  MD_TRY(launch_gemm(p, d->index ? A_INDEXED : A_DENSE, prec, d->tile, s.st));
  MD_TRY(ob.close(s.st));
  return s.finish();
}

int md_op_merge_index_table(int B, int g, int steps, int pad, int SS, int seq0, int32_t* out, int64_t capacity) {
  if (B <= 0 || g <= 0 || steps <= 0 || pad < 0 || seq0 < 0 || SS < 1 + g * g || (steps > 1 && 2 * pad >= g))
    MD_FAIL(MD_ERR_SHAPE, "merge_index_table: B=%d g=%d steps=%d pad=%d SS=%d seq0=%d", B, g, steps, pad, SS, seq0);
  const int E = merged_extent(g, steps, pad);
  const double n = (double)B * E * E;
  if (n >= 2147483648.0 || ((double)seq0 + (double)steps * steps * B) * SS >= 2147483648.0) MD_FAIL(MD_ERR_UNSUPPORTED, "merge_index_table: rows beyond 2^31");
  if (out && capacity < (int64_t)n) MD_FAIL(MD_ERR_SHAPE, "merge_index_table: %ld entries, capacity %ld", (long)n, (long)capacity);
  if (out) merge_index_table(B, g, steps, pad, SS, seq0, out);
  return (int)n;
}

int md_op_token_index_table(int B, int P, int SS, int seq0, int32_t* out, int64_t capacity) {
  if (B <= 0 || P <= 0 || seq0 < 0 || SS < 1 + P) MD_FAIL(MD_ERR_SHAPE, "token_index_table: B=%d P=%d SS=%d seq0=%d", B, P, SS, seq0);
  if (((double)seq0 + B) * SS >= 2147483648.0) MD_FAIL(MD_ERR_UNSUPPORTED, "token_index_table: rows beyond 2^31");
  const int64_t n = (int64_t)B * P;
  if (out && capacity < n) MD_FAIL(MD_ERR_SHAPE, "token_index_table: %ld entries, capacity %ld", (long)n, (long)capacity);
  if (out) token_index_table(B, P, SS, seq0, out);
  return (int)n;
}

// ---- the camera path alone (launcher scratch: raw DevBufs, so that a call the launcher refuses has started no device work) ----
int md_op_camera_encode(md_device_t dev, const md_camera_encode* d, void* stream) {
  if (!dev || !d || !d->extr || !d->intr || !d->out) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  const int B = d->B, V = d->V, D = d->D;
  if (B <= 0 || D <= 0 || d->H <= 0 || d->W <= 0) MD_FAIL(MD_ERR_SHAPE, "camera_encode: B=%d D=%d image %dx%d", B, D, d->H, d->W);
  CamEncW w{};
  w.fc1_w = d->w[0]; w.fc1_b = d->w[1]; w.fc2_w = d->w[2]; w.fc2_b = d->w[3];
  w.tn_g = d->w[4]; w.tn_b = d->w[5]; w.on_g = d->w[6]; w.on_b = d->w[7];
  w.depth = d->depth;
  for (int i = 0; i < 8; ++i)
    if (!d->w[i]) MD_FAIL(MD_ERR_INVALID_ARG, "camera_encode: weight %d missing", i);
  for (int i = 0; i < std::min(std::max(d->depth, 0), (int)CamEncW::kMaxDepth); ++i) {
    const float* const* b = d->blk[i];
    for (int j = 0; j < 14; ++j)
      if (!b[j]) MD_FAIL(MD_ERR_INVALID_ARG, "camera_encode: block %d weight %d missing", i, j);
    w.blk[i] = CamEncW::Blk{b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10], b[11], b[12], b[13]};
  }
  OpStage s;
  MD_TRY(s.open(dev, stream));
  DevBuf scratch;
  MD_TRY(scratch.alloc((V > 0 ? camera_encoder_scratch_floats(B, V, D) : 0) * 4, true));
  MD_TRY(launch_camera_encoder(d->extr, d->intr, B, V, D, d->heads, d->H, d->W, d->eps_tok, d->eps_blk, w, (float*)scratch.p, d->out, s.st));
  if (d->pose_out) {  // camera_encoder_kernel: per image `pose [V][12]` leads the scratch
    const size_t per_image = camera_encoder_scratch_floats(1, V, D);
    for (int b = 0; b < B; ++b)
      MD_HIP(hipMemcpy2DAsync(d->pose_out + (size_t)b * V * 9, 9 * 4, (float*)scratch.p + b * per_image, 12 * 4, 9 * 4, V, hipMemcpyDeviceToDevice, s.st));
  }
  return s.finish();
}

int md_op_camera_decode(md_device_t dev, const md_camera_decode* d, void* stream) {
  if (!dev || !d || !d->cam || !d->pose) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  for (int i = 0; i < 10; ++i)
    if (!d->w[i]) MD_FAIL(MD_ERR_INVALID_ARG, "camera_decode: weight %d missing", i);
  const int B = d->B, din = d->din;
  if (din <= 0 || d->H <= 0 || d->W <= 0) MD_FAIL(MD_ERR_SHAPE, "camera_decode: din=%d image %dx%d", din, d->H, d->W);
  const CamDecW w{d->w[0], d->w[1], d->w[2], d->w[3], d->w[4], d->w[5], d->w[6], d->w[7], d->w[8], d->w[9]};
  OpStage s;
  MD_TRY(s.open(dev, stream));
  DevBuf h;  // h1 | h2
  const size_t n = B > 0 ? (size_t)B * din : 0;
  MD_TRY(h.alloc(2 * n * 4, true));
  MD_TRY(launch_camera_decoder(d->cam, B, din, w, d->H, d->W, (float*)h.p, (float*)h.p + n, d->pose, d->extr, d->intr, s.st));
  return s.finish();
}

int md_op_pose_to_camera(md_device_t dev, const float* pose, int B, int H, int W, float* extr, float* intr, void* stream) {
  if (!dev || !pose) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (B <= 0 || H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "pose_to_camera: B=%d image %dx%d", B, H, W);
  OpStage s;
  MD_TRY(s.open(dev, stream));
  MD_TRY(launch_pose_to_camera(pose, B, H, W, extr, intr, s.st));
  return s.finish();
}

int md_debug_gemm_last_launch(int out[4]) {
  if (!out) return MD_ERR_INVALID_ARG;
  const LaunchNote n = gemm_last_launch();
  out[0] = n.tile; out[1] = n.ps_fast; out[2] = n.K; out[3] = 0;
  return MD_OK;
}

int md_debug_gemm_last_form(int out[8]) {
  if (!out) return MD_ERR_INVALID_ARG;
  const Form256 f = gemm_last_form();
  out[0] = f.family; out[1] = f.ek; out[2] = f.fold; out[3] = f.qkv; out[4] = f.conv; out[5] = f.diag;
  out[6] = (int)std::min<long>(f.blocks, 0x7fffffffL); out[7] = f.grid;
  return MD_OK;
}

int md_op_conv2d_direct_ex(md_device_t dev, const float* x_dev, const float* w_dev, const float* bias_dev, const float* add_dev, int B,
                           int Cin, int H, int W, int Cout, int k, int stride, int pad, int relu, int in_precision, int out_ld,
                           float* out_dev, void* stream) {
  if (!dev || !x_dev || !w_dev || !out_dev) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  if (!token_op_prec(in_precision)) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", in_precision);
  if (B <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || k <= 0 || stride <= 0 || pad < 0) MD_FAIL(MD_ERR_SHAPE, "invalid shape");
  if (H + 2 * pad < k || W + 2 * pad < k) MD_FAIL(MD_ERR_SHAPE, "input %dx%d smaller than kernel %d", H, W, k);
  OpStage s;
  MD_TRY(s.open(dev, stream, in_precision));
  DevBuf xa, wa;
  MD_TRY(wa.alloc((size_t)Cout * k * k * Cin * 4));
  MD_TRY(s.nhwc_a(x_dev, B, Cin, H, W, 0, xa));
  PackEntry e;
  e.kind = PACK_DIRECT; e.d0 = Cout; e.d1 = Cin; e.k = k; e.kp = Cin; e.f32 = 1;
  MD_TRY(s.conv_w(w_dev, e, wa));
  MD_TRY(launch_conv_direct(xa.p, in_precision, add_dev, B, H, W, Cin, (const float*)wa.p, bias_dev, Cout, k, stride, pad, relu, out_dev, s.st,
                            out_ld));
  return s.finish();
}

int md_op_fov_to_focal(float fovx_deg, int H, int W, float* focal_px, float* fovy_rad) {
  if (H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid image size");
  fov_scalar_host(fovx_deg, H, W, focal_px, fovy_rad);
  return MD_OK;
}

int md_op_focal_to_fov(float f_px, int H, int W, float* fovx_deg, float* fovy_rad) {
  if (H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid image size");
  if (!std::isfinite(f_px) || !(f_px > 0.f)) MD_FAIL(MD_ERR_INVALID_ARG, "f_px = %g: a focal length must be finite and > 0", (double)f_px);
  focal_scalar_host(f_px, H, W, fovx_deg, fovy_rad);
  return MD_OK;
}

namespace {
__attribute__((unused)) int fill_random(void* dst, size_t elems, int precision, uint64_t seed, float scale, hipStream_t st) {
  std::vector<float> h(std::min<size_t>(elems, (size_t)1 << 22));
  uniform_stream("bench", seed, h.size(), -scale, scale, h.data());
  DevBuf tmp;
  MD_TRY(tmp.alloc(h.size() * 4));
  MD_HIP(hipMemcpy(tmp.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  const size_t es = esz_of(precision);
  for (size_t off = 0; off < elems; off += h.size()) {
    const size_t n = std::min(h.size(), elems - off);
    if (precision == MD_PREC_FP8)
      MD_TRY(launch_f32_to_fp8((const float*)tmp.p, (long)(n & ~(size_t)3), 448.0f / scale * 0.25f, (char*)dst + off, st));
    else
      MD_TRY(launch_f32_to_rows((const float*)tmp.p, (long)n, (char*)dst + off * es, precision, st));
  }
  MD_HIP(hipStreamSynchronize(st));
  return MD_OK;
}
}  // namespace

int md_debug_gemm_direct_store(int on) { return md::gemm_direct_store(on); }
int md_debug_gemm_persistent(int on) { return md::gemm_persistent(on); }
int md_debug_gemm_stagger(int which, int ticks) {
  if (which < 0 || which > 3 || ticks < 0) return MD_ERR_INVALID_ARG;
  md::gemm_stagger(which, ticks);
  return MD_OK;
}

int md_debug_gemm_stagger_ticks(int which) { return which < 0 || which > 3 ? MD_ERR_INVALID_ARG : md::gemm_stagger_ticks(which); }

int md_gemm_ksplit_launches(void) { return (int)(md::gemm_ksplit_launches() & 0x7fffffff); }

int md_gemm_pick_tile(int M, int N, int K, int precision) {
  if (M <= 0 || N <= 0 || K <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "md_gemm_pick_tile: M=%d N=%d K=%d", M, N, K);
  md::GemmParams p;
  p.N = N; p.K = K; p.ngroups = 1; p.g_rows[0] = M;
  return md::gemm_pick_tile(p, precision);
}

int md_bench_gemm(md_device_t dev, int mode, int M, int N, int K, int aux0, int aux1, int precision, int tile, int iters,
                  float* avg_ms) {
  const int dbg = tile >> 8;  // timing-only ablation flags ride in the upper bits of `tile`
  tile &= 0xff;
  if (!dev || !avg_ms || M <= 0 || N <= 0 || K <= 0 || iters <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "invalid argument");
  OpStage s;
  MD_TRY(s.open(dev, nullptr, precision));
  hipStream_t st = s.st;
  const size_t es = esz_of(precision);
  DevBuf a, w, o;
  const size_t kw = mode == 1 ? (size_t)9 * K : (size_t)K;
  MD_TRY(a.alloc((size_t)M * K * es));
  MD_TRY(w.alloc((size_t)N * kw * es));
  MD_TRY(o.alloc((size_t)M * N * (es < 2 ? 2 : es)));
  MD_TRY(s.zero_page());
  MD_TRY(fill_random(a.p, (size_t)M * K, precision, 1, 1.0f, st));
  MD_TRY(fill_random(w.p, (size_t)N * kw, precision, 2, 0.05f, st));
  GemmParams p;
  p.N = N; p.ngroups = 1; p.g_rows[0] = M; p.W[0] = w.p; p.A = a.p;
  p.epi = EPI_STORE; p.out = o.p; p.ldo = N; p.debug_flags = (dbg & 3) | ((dbg & 64) ? 4 : 0) | ((dbg & 128) ? 8 : 0);
  DevBuf bias;
  DevBuf xres, lsc;
  if (dbg & 16) {  // proj / fc2-style epilogue: x(f32) += scale * (acc + bias)
    MD_TRY(xres.alloc((size_t)M * N * 4));
    MD_TRY(lsc.alloc((size_t)N * 8));
    MD_TRY(fill_random(lsc.p, (size_t)N * 2, MD_PREC_F32, 6, 0.1f, st));
    p.epi = EPI_RESID_LS; p.out = xres.p; p.ldo = N; p.scale[0] = (const float*)lsc.p; p.bias[0] = (const float*)lsc.p + N;
  }
  if (dbg & 4) {  // fc1-style epilogue: bias + GELU
    MD_TRY(bias.alloc((size_t)N * 4));
    MD_TRY(fill_random(bias.p, (size_t)N, MD_PREC_F32, 5, 0.1f, st));
    p.bias[0] = (const float*)bias.p; p.act = ACT_GELU;
  }
  if ((dbg & 8) && mode != 1) {  // deconv k2s2 epilogue: pixel shuffle of N = 4 * psC columns; aux0 x aux1 = input pixel grid (batch folded into H)
    if ((long)aux0 * aux1 != M || N % 4 != 0) MD_FAIL(MD_ERR_SHAPE, "pixel-shuffle bench: aux0*aux1 must equal M, N = 4*C");
    MD_TRY(bias.alloc((size_t)N * 4));
    MD_TRY(fill_random(bias.p, (size_t)N, MD_PREC_F32, 5, 0.1f, st));
    p.epi = EPI_PIXSHUF; p.bias[0] = (const float*)bias.p; p.psH = aux0; p.psW = aux1; p.psC = N / 4; p.ps_f = 2; p.ldo = N / 4; p.ps_coff = 0;
  }
  int amode = A_DENSE;
  if (mode == 1) {
    if ((long)aux0 * aux1 != M) MD_FAIL(MD_ERR_SHAPE, "conv bench: H*W must equal M");
    amode = A_CONV3; p.K = 9 * K; p.cH = aux0; p.cW = aux1; p.cC = K; p.zero_page = s.geom.zero_page;
  } else {
    p.K = K; p.lda = K;
  }
  for (int i = 0; i < 2; ++i) MD_TRY(launch_gemm(p, amode, precision, tile, st));
  if (dbg & 32) {  // per-block phase stamps of ONE launch (100 MHz s_memrealtime), printed to stderr
    const long blocks = (long)((M + 255) / 256) * ((N + 255) / 256);
    DevBuf sb;
    MD_TRY(sb.alloc((size_t)blocks * 128));
    p.stamps = (unsigned long long*)sb.p;
    MD_TRY(launch_gemm(p, amode, precision, tile, st));
    MD_HIP(hipStreamSynchronize(st));
    std::vector<unsigned long long> h((size_t)blocks * 16);
    MD_HIP(hipMemcpy(h.data(), sb.p, h.size() * 8, hipMemcpyDeviceToHost));
    p.stamps = nullptr;
    double d[7] = {0, 0, 0, 0, 0, 0, 0}, cyc = 0;
    unsigned long long tmin = ~0ull, tmax = 0;
    for (long b = 0; b < blocks; ++b) {
      const unsigned long long* q = &h[(size_t)b * 16];
      for (int k = 0; k < 7; ++k) d[k] += (double)(q[k + 1] - q[k]);
      cyc += (double)(q[9] - q[8]);
      tmin = std::min(tmin, q[0]);
      tmax = std::max(tmax, q[7]);
    }
    fprintf(stderr, "[stamps] blocks=%ld  setup %.2f  issue %.2f  first-wait %.2f  mainloop %.2f  epi-barrier %.2f  epi-body %.2f  store-drain %.2f us "
                    "(wave 0, mean per block); kernel span %.1f us; mainloop %.0f shader cycles = %.3f GHz\n",
            blocks, d[0] / blocks / 100.0, d[1] / blocks / 100.0, d[2] / blocks / 100.0, d[3] / blocks / 100.0, d[4] / blocks / 100.0,
            d[5] / blocks / 100.0, d[6] / blocks / 100.0, (double)(tmax - tmin) / 100.0, cyc / blocks, cyc / (d[3] * 10.0));
  }
  hipEvent_t e0, e1;
  MD_HIP(hipEventCreate(&e0));
  MD_HIP(hipEventCreate(&e1));
  MD_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) MD_TRY(launch_gemm(p, amode, precision, tile, st));
  MD_HIP(hipEventRecord(e1, st));
  MD_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MD_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = ms / iters;
  return MD_OK;
}

int md_bench_attention_ex(md_device_t dev, int T, int n_tokens, int heads, int precision, float qk_scale, int iters, float* avg_ms) {
  if (!dev || !avg_ms || T <= 0 || n_tokens <= 0 || heads <= 0 || iters <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "invalid argument");
  if (precision != MD_PREC_BF16 && precision != MD_PREC_F16) MD_FAIL(MD_ERR_INVALID_ARG, "attention bench: bf16 or f16");
  MD_HIP(hipSetDevice(dev->ordinal));
  hipStream_t st = dev->stream;
  const int D = heads * 64, SS = (n_tokens + 3) / 4 * 4, kpad = (n_tokens + 63) / 64 * 64;
  DevBuf qk, vT, ao;
  MD_TRY(qk.alloc(((size_t)T * SS + 64) * 2 * D * 2));
  MD_TRY(vT.alloc((size_t)T * heads * 64 * kpad * 2));
  MD_TRY(ao.alloc(((size_t)T * SS + 64) * D * 2));
  MD_TRY(fill_random(qk.p, (size_t)T * SS * 2 * D, precision, 3, qk_scale, st));
  MD_TRY(fill_random(vT.p, (size_t)T * heads * 64 * kpad, precision, 4, 1.0f, st));
  DevBuf redo;
  MD_TRY(redo.alloc((size_t)attention_redo_ints(T * heads) * 4));
  if (precision == MD_PREC_BF16) MD_TRY(attention_asm_prepare());
  for (int i = 0; i < 2; ++i) MD_TRY(launch_attention(qk.p, vT.p, ao.p, T, SS, n_tokens, heads, D, kpad, precision, st, 0.f, 0, (int*)redo.p));
  hipEvent_t e0, e1;
  MD_HIP(hipEventCreate(&e0));
  MD_HIP(hipEventCreate(&e1));
  MD_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) MD_TRY(launch_attention(qk.p, vT.p, ao.p, T, SS, n_tokens, heads, D, kpad, precision, st, 0.f, 0, (int*)redo.p));
  MD_HIP(hipEventRecord(e1, st));
  MD_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MD_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = ms / iters;
  return MD_OK;
}

int md_bench_attention_qkv(md_device_t dev, const float* qkv_dev, int T, int n_tokens, int heads, int precision, int iters, float* avg_ms,
                           long* redo_units_per_launch) {
  if (!dev || !qkv_dev || !avg_ms || T <= 0 || n_tokens <= 0 || heads <= 0 || iters <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "invalid argument");
  if (precision != MD_PREC_BF16 && precision != MD_PREC_F16) MD_FAIL(MD_ERR_INVALID_ARG, "attention bench: bf16 or f16");
  MD_HIP(hipSetDevice(dev->ordinal));
  hipStream_t st = dev->stream;
  const int D = heads * 64, SS = (n_tokens + 3) / 4 * 4, kpad = (n_tokens + 63) / 64 * 64;
  DevBuf qk, vT, ao, redo;
  MD_TRY(qk.alloc(((size_t)T * SS + 64) * 2 * D * 2));
  MD_TRY(vT.alloc((size_t)T * heads * 64 * kpad * 2));
  MD_TRY(ao.alloc(((size_t)T * SS + 64) * D * 2));
  MD_TRY(redo.alloc((size_t)attention_redo_ints(T * heads) * 4));
  MD_TRY(launch_qkv_split(qkv_dev, T, n_tokens, heads, SS, kpad, qk.p, vT.p, attn_qscale(precision), precision, st));
  if (precision == MD_PREC_BF16) MD_TRY(attention_asm_prepare());
  for (int i = 0; i < 2; ++i) MD_TRY(launch_attention(qk.p, vT.p, ao.p, T, SS, n_tokens, heads, D, kpad, precision, st, 0.f, 0, (int*)redo.p));
  MD_HIP(hipStreamSynchronize(st));
  (void)attention_asm_redo_units(1);
  hipEvent_t e0, e1;
  MD_HIP(hipEventCreate(&e0));
  MD_HIP(hipEventCreate(&e1));
  MD_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < iters; ++i) MD_TRY(launch_attention(qk.p, vT.p, ao.p, T, SS, n_tokens, heads, D, kpad, precision, st, 0.f, 0, (int*)redo.p));
  MD_HIP(hipEventRecord(e1, st));
  MD_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MD_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = ms / iters;
  if (redo_units_per_launch) {
    const long u = attention_asm_redo_units(1);
    *redo_units_per_launch = u < 0 ? -1 : u / iters;
  }
  return MD_OK;
}

int md_debug_attention_asm(int on) { return attention_allow_asm(on); }
long md_debug_attention_asm_launches(void) { return attention_asm_launches(); }
long md_debug_attention_redo_units(md_device_t dev, int reset) {
  if (!dev || hipSetDevice(dev->ordinal) != hipSuccess) return -1;
  return attention_asm_redo_units(reset);
}

int md_bench_attention(md_device_t dev, int T, int n_tokens, int heads, int iters, float* avg_ms) {
  return md_bench_attention_ex(dev, T, n_tokens, heads, MD_PREC_BF16, 0.7f, iters, avg_ms);
}

namespace {
int parse_da3_cfg(const md_da3_cfg* c, Da3Cfg* out) {
  if (!c || !c->variant) MD_FAIL(MD_ERR_INVALID_ARG, "config is null");
  Da3Cfg d;
  d.variant = c->variant;
  ViTDims v;
  v.in_chans = 3; v.mlp_ratio = 4; v.ps = 14;
  if (d.variant == "metric_large") {  // depth_anything3/mod.rs:153-156, dpt.rs:41-58
    v.preset = "da3_vitl14"; v.D = 1024; v.depth = 24; v.heads = 16; v.img = 518;
    d.image_size = 518; d.features = 256;
    const int oc[4] = {256, 512, 1024, 1024}, hk[4] = {4, 11, 17, 23};
    for (int i = 0; i < 4; ++i) { d.out_channels[i] = oc[i]; d.hook_ids[i] = hk[i]; }
  } else if (d.variant == "tiny") {
    v.preset = "da3_tiny14"; v.D = 256; v.depth = 4; v.heads = 4; v.img = 70;
    d.image_size = 70; d.features = 64;
    const int oc[4] = {64, 128, 256, 256}, hk[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; ++i) { d.out_channels[i] = oc[i]; d.hook_ids[i] = hk[i]; }
  } else if (d.variant == "small") {  // mod.rs:158-171,190-196; dpt.rs:60-79
    v.preset = "da3_vits14"; v.D = 384; v.depth = 12; v.heads = 6; v.img = 518;
    d.image_size = 518; d.features = 64; d.output_dim = 2; d.dual_head = true; d.ext_block_start = 4;
    d.camera_encoder = true;
    const int oc[4] = {48, 96, 192, 384}, hk[4] = {5, 7, 9, 11};
    for (int i = 0; i < 4; ++i) { d.out_channels[i] = oc[i]; d.hook_ids[i] = hk[i]; }
  } else if (d.variant == "tiny_dual") {  // test-only: same topology, 6 blocks of width 128
    v.preset = "da3_tinydual14"; v.D = 128; v.depth = 6; v.heads = 2; v.img = 70;
    d.image_size = 70; d.features = 64; d.output_dim = 2; d.dual_head = true; d.ext_block_start = 2;
    d.camera_encoder = true; d.cam_trunk_depth = 2;
    const int oc[4] = {48, 96, 64, 128}, hk[4] = {2, 3, 4, 5};
    for (int i = 0; i < 4; ++i) { d.out_channels[i] = oc[i]; d.hook_ids[i] = hk[i]; }
  } else {
    MD_FAIL(MD_ERR_INVALID_ARG, "unknown Depth-Anything-v3 variant `%s`", c->variant);
  }
  for (int i = 0; i < 4; ++i) { v.hook_ids[i] = d.hook_ids[i]; v.feat_dims[i] = d.out_channels[i]; }
  d.vit = v;
  if (c->image_size > 0) {
    if (c->image_size % v.ps != 0) MD_FAIL(MD_ERR_SHAPE, "image size %d must be divisible by patch size %d", c->image_size, v.ps);
    d.image_size = c->image_size;
  }
  if (c->image_width > 0) {
    if (c->image_width % v.ps != 0) MD_FAIL(MD_ERR_SHAPE, "image width %d must be divisible by patch size %d", c->image_width, v.ps);
    d.image_width = c->image_width;
  }
  d.precision = c->precision;
  d.max_batch = c->max_batch > 0 ? c->max_batch : 1;
  d.ln_eps = c->ln_eps > 0.f ? c->ln_eps : 1e-6f;
  if (!token_op_prec(d.precision) && d.precision != MD_PREC_FP8) MD_FAIL(MD_ERR_INVALID_ARG, "unknown precision %d", d.precision);
  *out = d;
  return MD_OK;
}
}  // namespace

void md_da3_cfg_default(md_da3_cfg* cfg) {
  if (!cfg) return;
  cfg->variant = "metric_large";
  cfg->image_size = 0;
  cfg->image_width = 0;
  cfg->precision = MD_PREC_BF16;
  cfg->max_batch = 1;
  cfg->ln_eps = 1e-6f;
}

int md_da3_create(md_device_t dev, const md_da3_cfg* cfg, uint64_t seed, int init_scheme, md_model_t* out) {
  if (!dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "device/out is null");
  Da3Cfg dc;
  MD_TRY(parse_da3_cfg(cfg, &dc));
  md_model_t m = nullptr;
  MD_TRY(da3_create(dev, dc, &m));
  int s = model_init_seeded(m, seed, init_scheme);
  if (s != MD_OK) {
    model_destroy(m);
    return s;
  }
  *out = m;
  return MD_OK;
}

int md_da3_load(md_device_t dev, const md_da3_cfg* cfg, const char* path, md_model_t* out) {
  if (!dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "device/out is null");
  Da3Cfg dc;
  MD_TRY(parse_da3_cfg(cfg, &dc));
  {
    Container probe;
    MD_TRY(read_container(path, &probe));
  }
  md_model_t m = nullptr;
  MD_TRY(da3_create(dev, dc, &m));
  int s = model_load_container(m, path);
  if (s != MD_OK) {
    model_destroy(m);
    return s;
  }
  *out = m;
  return MD_OK;
}

int md_da3_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, int out_kind, void* stream) {
  return da3_infer(m, nchw, B, H, W, in_kind, depth, out_kind, (hipStream_t)stream);
}

int md_da3_infer_ex(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const md_da3_outputs* out, int out_kind,
                    void* stream) {
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "outputs struct is null");
  Da3Outputs o;
  o.depth = out->depth; o.depth_confidence = out->depth_confidence; o.aux = out->aux; o.aux_confidence = out->aux_confidence;
  o.pose_encoding = out->pose_encoding; o.extrinsics = out->extrinsics; o.intrinsics = out->intrinsics;
  return da3_infer_ex(m, nchw, B, H, W, in_kind, o, out_kind, (hipStream_t)stream);
}

int md_da3_infer_views(md_model_t m, const float* nchw, int B, int V, int H, int W, int in_kind, const md_da3_outputs* out, int out_kind,
                       void* stream) {
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "outputs struct is null");
  if (B <= 0 || V <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid input shape [%d,%d,3,%d,%d]", B, V, H, W);
  if ((long)B * V > 0x7fffffffL) MD_FAIL(MD_ERR_SHAPE, "%d scenes of %d views", B, V);
  Da3Outputs o;
  o.depth = out->depth; o.depth_confidence = out->depth_confidence; o.aux = out->aux; o.aux_confidence = out->aux_confidence;
  o.pose_encoding = out->pose_encoding; o.extrinsics = out->extrinsics; o.intrinsics = out->intrinsics;
  o.views = V;
  return da3_infer_ex(m, nchw, B * V, H, W, in_kind, o, out_kind, (hipStream_t)stream);
}

int md_da3_infer_with_camera(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const float* extrinsics,
                             const float* intrinsics, int views, const md_da3_outputs* out, int out_kind, void* stream) {
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "outputs struct is null");
  if (!extrinsics || !intrinsics) MD_FAIL(MD_ERR_INVALID_ARG, "extrinsics/intrinsics is null (md_da3_infer_ex is the call without camera inputs)");
  if (views < 1) MD_FAIL(MD_ERR_SHAPE, "camera inputs need at least one view, got %d", views);
  Da3Outputs o;
  o.depth = out->depth; o.depth_confidence = out->depth_confidence; o.aux = out->aux; o.aux_confidence = out->aux_confidence;
  o.pose_encoding = out->pose_encoding; o.extrinsics = out->extrinsics; o.intrinsics = out->intrinsics;
  o.cam_extrinsics = extrinsics; o.cam_intrinsics = intrinsics; o.cam_views = views;
  return da3_infer_ex(m, nchw, B, H, W, in_kind, o, out_kind, (hipStream_t)stream);
}

int md_da3_infer_raw(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* logits, int out_kind, void* stream) {
  if (!logits) MD_FAIL(MD_ERR_INVALID_ARG, "logits is null");
  Da3Outputs o;
  o.raw_logits = logits;
  return da3_infer_ex(m, nchw, B, H, W, in_kind, o, out_kind, (hipStream_t)stream);
}

int md_da3_infer_from_tokens(md_model_t m, const float* const* tokens, int tokens_per_image, int B, int H, int W, int in_kind,
                             const md_da3_outputs* out, int out_kind, void* stream) {
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "outputs struct is null");
  if (!tokens) MD_FAIL(MD_ERR_INVALID_ARG, "tokens is null");
  Da3Outputs o;
  o.depth = out->depth; o.depth_confidence = out->depth_confidence; o.aux = out->aux; o.aux_confidence = out->aux_confidence;
  o.pose_encoding = out->pose_encoding; o.extrinsics = out->extrinsics; o.intrinsics = out->intrinsics;
  for (int i = 0; i < 4; ++i) o.tokens[i] = tokens[i];
  if (!o.tokens[0]) MD_FAIL(MD_ERR_LEVELS, "Backbone returned fewer hooks (0) than requested (4)");
  o.tokens_per_image = tokens_per_image;
  return da3_infer_ex(m, nullptr, B, H, W, in_kind, o, out_kind, (hipStream_t)stream);
}

int md_da3_param_inventory(const md_da3_cfg* cfg, int init_scheme, int index, const char** name, size_t* count, float* lo,
                           float* hi) {
  Da3Cfg dc;
  MD_TRY(parse_da3_cfg(cfg, &dc));
  static thread_local std::vector<ParamSpec> specs;
  specs = da3_param_specs(dc, init_scheme);
  if (index >= 0 && index < (int)specs.size()) {
    if (name) *name = specs[index].name.c_str();
    if (count) *count = specs[index].count();
    if (lo) *lo = specs[index].lo;
    if (hi) *hi = specs[index].hi;
  }
  return (int)specs.size();
}

int md_param_inventory(const md_depth_pro_cfg* cfg, int init_scheme, int index, const char** name, size_t* count, float* lo,
                       float* hi) {
  ModelCfg mc;
  MD_TRY(parse_cfg(cfg, &mc));
  static thread_local std::vector<ParamSpec> specs;
  specs = depth_pro_param_specs(mc, init_scheme);
  if (index >= 0 && index < (int)specs.size()) {
    if (name) *name = specs[index].name.c_str();
    if (count) *count = specs[index].count();
    if (lo) *lo = specs[index].lo;
    if (hi) *hi = specs[index].hi;
  }
  return (int)specs.size();
}

int md_uniform_stream(const char* name, uint64_t seed, size_t count, float lo, float hi, float* out_host) {
  if (!name || !out_host) MD_FAIL(MD_ERR_INVALID_ARG, "null argument");
  uniform_stream(name, seed, count, lo, hi, out_host);
  return MD_OK;
}

int md_split_geometry(int image_size, int window, float overlap, int* stride, int* steps) {
  if (!stride || !steps || image_size <= 0 || window <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "invalid argument");
  split_geometry(image_size, window, overlap, stride, steps);
  return MD_OK;
}

int md_feature_padding(int window, int stride, int feature_size) { return feature_padding(window, stride, feature_size); }

}  // extern "C"
