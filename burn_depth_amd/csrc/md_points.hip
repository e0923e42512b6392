// The point path: md_op_unproject (depth + cameras -> point map / mask / ordered cloud on caller tensors) and md_infer_points
// (the model's infer body, then the same kernels on its results, in one call); md_op_unproject_normals / md_infer_points_normals
// are the same two calls with the normals forms of the kernels. model (model_infer / da3_infer_ex bodies) ->
// classify / scan / scatter (kernels/points.hip); one captured graph per replay key when the model replays graphs.
// md_op_filter_views / md_infer_points_filtered put the view filter (kernels/view_filter.hip: confidence percentile, cross-view
// support) in front of those launches: it hands them a depth in which rejected pixels are 0.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "md_engine.h"
#include "md_engine_util.h"

// Device homes of what the call needs on the device and the caller did not hand over there. Grow-only (md::grow): a captured
// graph bakes their addresses.
struct md_model_s::PointsState {
  md::GrowBuf<void> scratch;      // bit mask | block counts | block offsets
  md::GrowBuf<float> depth, conf; // the model's depth (no device `depth` output) and confidence
  md::GrowBuf<float> raw;         // md_infer_points_filtered: the model's depth; `depth` / the caller's buffer take the filtered one
  md::GrowBuf<void> filter;       // the view filter's histogram table and select state
  md::GrowBuf<float> cams;        // K [B,9] | E [B,12] | focal [B]: the model's cameras, or the device copy of host ones
  md::GrowBuf<float> x;           // host input image
  md::GrowBuf<uint8_t> rgb;       // host rgb
  md::GrowBuf<void> out;          // device homes of host outputs
};

namespace md {

void points_destroy_state(md_model_t m) {
  delete m->points;
  m->points = nullptr;
}

namespace {

struct Sources {  // what the kernels will read, known before the model runs
  bool rgb = false, conf = false, K = false, focal = false, E = false;
};

int check_points(const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm, const Sources& s, int B, int H, int W) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "point options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  if (nrm) {
    if (!std::isfinite(nrm->min_cos) || nrm->min_cos < 0.f || nrm->min_cos > 1.f)
      MD_FAIL(MD_ERR_INVALID_ARG, "min_cos = %g: must lie in [0, 1]", (double)nrm->min_cos);
    if (nrm->normals && !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "the compacted normals need `count`");
  }
  if (o->stride < 1) MD_FAIL(MD_ERR_INVALID_ARG, "stride %d: at least 1", o->stride);
  if (out->capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "capacity %lld is negative", (long long)out->capacity);
  if ((out->xyz || out->rgb || out->conf) && !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "the compacted outputs need `count`");
  if (out->rgb && !s.rgb) MD_FAIL(MD_ERR_INVALID_ARG, "an rgb output needs an rgb input");
  if (out->conf && !s.conf) MD_FAIL(MD_ERR_INVALID_ARG, "a conf output needs a confidence map");
  if (!std::isfinite(o->pixel_offset)) MD_FAIL(MD_ERR_INVALID_ARG, "pixel_offset is not finite");
  const float nn[4] = {o->edge_rtol, o->conf_min, o->depth_min, o->depth_max};
  const char* names[4] = {"edge_rtol", "conf_min", "depth_min", "depth_max"};
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(nn[i]) || nn[i] < 0.f) MD_FAIL(MD_ERR_INVALID_ARG, "%s = %g: must be finite and >= 0", names[i], (double)nn[i]);
  if (o->depth_min > 0.f && o->depth_max > 0.f && o->depth_max < o->depth_min)
    MD_FAIL(MD_ERR_INVALID_ARG, "depth_max %g < depth_min %g", (double)o->depth_max, (double)o->depth_min);
  if (o->world && !s.E) MD_FAIL(MD_ERR_INVALID_ARG, "world = 1 needs extrinsics");
  if (!s.K && !s.focal) MD_FAIL(MD_ERR_INVALID_ARG, "neither intrinsics nor a focal length");
  if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1l << 31)) MD_FAIL(MD_ERR_SHAPE, "invalid depth shape [%d,%d,%d]", B, H, W);
  return MD_OK;
}

// 0 = the default of that bound
float depth_min_of(float v) { return v > 0.f ? v : FLT_MIN; }
float depth_max_of(float v) { return v > 0.f ? v : FLT_MAX; }

PointsParams make_params(int B, int H, int W, const md_points_opts& o) {
  PointsParams p;
  p.B = B; p.H = H; p.W = W;
  p.off = o.pixel_offset;
  p.dmin = depth_min_of(o.depth_min);
  p.dmax = depth_max_of(o.depth_max);
  p.conf_min = o.conf_min;
  p.edge_rtol = o.edge_rtol;
  p.stride = o.stride;
  p.world = o.world ? 1 : 0;
  return p;
}

NormalsParams make_normals(const md_points_normals* nrm) {
  NormalsParams q;
  if (nrm) { q.normal_map = nrm->normal_map; q.normals = nrm->normals; q.min_cos = nrm->min_cos; }
  return q;
}

// has_conf / has_intr / has_E: what the filter will find on the device (the caller's or the model's)
int check_filter(const md_view_filter_opts* o, bool has_conf, bool has_intr, bool has_E, int B, int H, int W) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (o->conf_percentile < 0 || o->conf_percentile > 99) MD_FAIL(MD_ERR_INVALID_ARG, "conf_percentile %d outside 0..99", o->conf_percentile);
  if (o->conf_percentile > 0 && !has_conf) MD_FAIL(MD_ERR_INVALID_ARG, "conf_percentile > 0 needs a confidence map");
  if (!std::isfinite(o->view_rtol) || o->view_rtol < 0.f) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol = %g: must be finite and >= 0", (double)o->view_rtol);
  if (!std::isfinite(o->pixel_offset)) MD_FAIL(MD_ERR_INVALID_ARG, "pixel_offset is not finite");
  if (!std::isfinite(o->depth_min) || o->depth_min < 0.f || !std::isfinite(o->depth_max) || o->depth_max < 0.f)
    MD_FAIL(MD_ERR_INVALID_ARG, "depth bounds %g, %g: must be finite and >= 0", (double)o->depth_min, (double)o->depth_max);
  if (o->depth_min > 0.f && o->depth_max > 0.f && o->depth_max < o->depth_min)
    MD_FAIL(MD_ERR_INVALID_ARG, "depth_max %g < depth_min %g", (double)o->depth_max, (double)o->depth_min);
  const bool views = o->view_rtol > 0.f;
  if (!views && o->min_views != 0) MD_FAIL(MD_ERR_INVALID_ARG, "min_views %d without view_rtol", o->min_views);
  if (views && o->min_views < 1) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs min_views >= 1, got %d", o->min_views);
  if (views && !has_E) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs extrinsics");
  if (views && !has_intr) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs intrinsics or a focal length");
  if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1l << 31) || B >= 65536) MD_FAIL(MD_ERR_SHAPE, "invalid depth shape [%d,%d,%d]", B, H, W);
  if (views && (B < 2 || B > kViewFilterMaxViews)) MD_FAIL(MD_ERR_SHAPE, "view_rtol > 0 takes 2..%d views, got %d", kViewFilterMaxViews, B);
  if (views && (H >= (1 << 24) || W >= (1 << 24))) MD_FAIL(MD_ERR_SHAPE, "view_rtol > 0: image sides below 2^24, got %d x %d", H, W);
  if (views && o->min_views > B - 1) MD_FAIL(MD_ERR_INVALID_ARG, "min_views %d: only %d other views", o->min_views, B - 1);
  return MD_OK;
}

ViewFilterParams make_filter_params(int B, int H, int W, const md_view_filter_opts& o) {
  ViewFilterParams p;
  p.B = B; p.H = H; p.W = W;
  p.off = o.pixel_offset;
  p.dmin = depth_min_of(o.depth_min);
  p.dmax = depth_max_of(o.depth_max);
  p.q = o.conf_percentile;
  p.rtol = o.view_rtol;
  p.min_views = o.min_views;
  return p;
}

uintptr_t fbits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

}  // namespace

int op_unproject(md_device_t dev, const float* depth_dev, const float* conf_dev, const uint8_t* rgb_dev, int B, int H, int W,
                 const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out, hipStream_t stream,
                 const md_points_normals* nrm) {
  if (!cam) MD_FAIL(MD_ERR_INVALID_ARG, "cameras are null");
  Sources s;
  s.rgb = rgb_dev != nullptr; s.conf = conf_dev != nullptr;
  s.K = cam->intrinsics != nullptr; s.focal = cam->focal_px != nullptr; s.E = cam->extrinsics != nullptr;
  MD_TRY(check_points(o, out, nrm, s, B, H, W));
  if (!depth_dev) MD_FAIL(MD_ERR_INVALID_ARG, "depth pointer is null");
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  MD_HIP(hipSetDevice(dev->ordinal));
  hipStream_t st = stream ? stream : dev->stream;
  PointsParams p = make_params(B, H, W, *o);
  p.depth = depth_dev; p.conf = conf_dev; p.rgb = rgb_dev;
  p.K = cam->intrinsics; p.focal = cam->focal_px; p.E = cam->extrinsics;
  p.point_map = out->point_map; p.mask = out->mask;
  p.xyz = out->xyz; p.rgb_out = out->rgb; p.conf_out = out->conf; p.count = out->count; p.capacity = out->capacity;
  void* scratch = nullptr;
  if (p.count) MD_HIP(hipMalloc(&scratch, points_scratch_bytes(B, H, W)));
  const NormalsParams q = make_normals(nrm);
  const int rc = launch_unproject(p, scratch, st, &q);
  if (scratch) {  // the scratch is freed on return
    const hipError_t se = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (rc == MD_OK) MD_HIP(se);
  }
  return rc;
}

int op_filter_views(md_device_t dev, const float* depth_dev, const float* conf_dev, int B, int H, int W, const md_points_cameras* cam,
                    const md_view_filter_opts* o, const md_view_filter_outputs* out, hipStream_t stream) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "view filter outputs are null");
  if (!out->depth && !out->support && !out->conf_threshold && !out->kept) MD_FAIL(MD_ERR_INVALID_ARG, "every view filter output is null");
  if (out->depth && out->depth == depth_dev) MD_FAIL(MD_ERR_INVALID_ARG, "the filtered depth may not be the input");
  const md_points_cameras none = {nullptr, nullptr, nullptr};
  const md_points_cameras& c = cam ? *cam : none;
  MD_TRY(check_filter(o, conf_dev != nullptr, c.intrinsics || c.focal_px, c.extrinsics != nullptr, B, H, W));
  if (!depth_dev) MD_FAIL(MD_ERR_INVALID_ARG, "depth pointer is null");
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  MD_HIP(hipSetDevice(dev->ordinal));
  hipStream_t st = stream ? stream : dev->stream;
  ViewFilterParams p = make_filter_params(B, H, W, *o);
  p.depth = depth_dev; p.conf = conf_dev;
  p.K = c.intrinsics; p.focal = c.intrinsics ? nullptr : c.focal_px; p.E = c.extrinsics;
  p.depth_out = out->depth; p.support = out->support; p.tau = out->conf_threshold; p.kept = out->kept;
  void* scratch = nullptr;
  MD_HIP(hipMalloc(&scratch, view_filter_scratch_bytes()));
  const int rc = launch_view_filter(p, scratch, st);
  const hipError_t se = hipStreamSynchronize(st);  // the scratch is freed on return
  (void)hipFree(scratch);
  if (rc == MD_OK) MD_HIP(se);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// the model call
// ------------------------------------------------------------------------------------------------
static int points_eager(md_model_s* m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras& cam,
                        const md_points_opts& o, const md_points_outputs& out, int out_kind, bool dual, hipStream_t st,
                        const md_view_filter_opts* fo, const md_points_normals* nrm) {
  if (!m->points) m->points = new md_model_s::PointsState();
  md_model_s::PointsState* f = m->points;
  const bool host_in = in_kind == MD_MEM_HOST, host_out = out_kind == MD_MEM_HOST;
  const size_t npx = (size_t)B * H * W;
  const size_t cap = (size_t)out.capacity;
  // ---- device homes (grow-only, before anything is enqueued) ----
  float* depth = out.depth;
  if (!depth || host_out) {
    MD_TRY(grow(m, st, f->depth, npx * 4));
    depth = f->depth.p;
  }
  float* raw = depth;  // what the model writes; with the filter, `depth` takes the filtered map
  const bool views = fo && fo->view_rtol > 0.f;
  if (fo) {
    MD_TRY(grow(m, st, f->raw, npx * 4));
    raw = f->raw.p;
    MD_TRY(grow(m, st, f->filter, view_filter_scratch_bytes()));
  }
  float* conf = nullptr;
  if (dual) {
    MD_TRY(grow(m, st, f->conf, npx * 4));
    conf = f->conf.p;
  }
  MD_TRY(grow(m, st, f->cams, (size_t)B * 22 * 4));
  float *k_home = f->cams.p, *e_home = f->cams.p + (size_t)B * 9, *f_home = f->cams.p + (size_t)B * 21;
  if (out.count) MD_TRY(grow(m, st, f->scratch, points_scratch_bytes(B, H, W)));
  PointsParams p = make_params(B, H, W, o);
  p.capacity = out.capacity;
  NormalsParams q = make_normals(nrm);
  size_t off_map = 0, off_mask = 0, off_xyz = 0, off_rgb = 0, off_conf = 0, off_count = 0, off_nmap = 0, off_nrm = 0, total = 0;
  if (host_out) {
    auto take = [&](bool want, size_t bytes) {
      const size_t at = total;
      if (want) total += align_up(bytes, 256);
      return at;
    };
    off_map = take(out.point_map, npx * 12);
    off_mask = take(out.mask, npx);
    off_xyz = take(out.xyz, cap * 12);
    off_rgb = take(out.rgb, cap * 3);
    off_conf = take(out.conf, cap * 4);
    off_count = take(out.count, (size_t)(B + 1) * 4);
    off_nmap = take(q.normal_map, npx * 12);
    off_nrm = take(q.normals, cap * 12);
    if (total) MD_TRY(grow(m, st, f->out, total));
    char* base = (char*)f->out.p;
    p.point_map = out.point_map ? (float*)(base + off_map) : nullptr;
    p.mask = out.mask ? (uint8_t*)(base + off_mask) : nullptr;
    p.xyz = out.xyz ? (float*)(base + off_xyz) : nullptr;
    p.rgb_out = out.rgb ? (uint8_t*)(base + off_rgb) : nullptr;
    p.conf_out = out.conf ? (float*)(base + off_conf) : nullptr;
    p.count = out.count ? (int32_t*)(base + off_count) : nullptr;
    if (q.normal_map) q.normal_map = (float*)(base + off_nmap);
    if (q.normals) q.normals = (float*)(base + off_nrm);
  } else {
    p.point_map = out.point_map; p.mask = out.mask;
    p.xyz = out.xyz; p.rgb_out = out.rgb; p.conf_out = out.conf; p.count = out.count;
  }
  // ---- inputs on the device ----
  const float* x_dev = nchw;
  const uint8_t* rgb_dev = rgb;
  const float *k_dev = cam.intrinsics, *e_dev = cam.extrinsics, *f_dev = cam.focal_px;
  if (host_in) {
    MD_TRY(grow(m, st, f->x, npx * 3 * 4));
    if (rgb) MD_TRY(grow(m, st, f->rgb, npx * 3));
    auto h2d = [&](void* dst, const void* src, size_t bytes) -> int {
      MD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
      return MD_OK;
    };
    MD_TRY(h2d(f->x.p, nchw, npx * 3 * 4));
    x_dev = f->x.p;
    if (rgb) {
      MD_TRY(h2d(f->rgb.p, rgb, npx * 3));
      rgb_dev = f->rgb.p;
    }
    if (k_dev) { MD_TRY(h2d(k_home, k_dev, (size_t)B * 36)); k_dev = k_home; }
    if (e_dev) { MD_TRY(h2d(e_home, e_dev, (size_t)B * 48)); e_dev = e_home; }
    if (f_dev) { MD_TRY(h2d(f_home, f_dev, (size_t)B * 4)); f_dev = f_home; }
  }
  // ---- the model: its cameras land in the homes of those the caller did not give ----
  const bool need_k = !k_dev && !f_dev, need_e = (o.world || views) && !e_dev;
  if (m->kind == 1) {
    Da3Outputs d;
    d.depth = raw;
    d.depth_confidence = conf;
    if (dual && need_k) { d.intrinsics = k_home; k_dev = k_home; }
    if (dual && need_e) { d.extrinsics = e_home; e_dev = e_home; }
    MD_TRY(da3_infer_ex_direct(m, x_dev, B, H, W, d, st));
  } else if (cam.focal_px) {
    MD_TRY(model_infer_direct(m, x_dev, B, H, W, raw, nullptr, nullptr, st, f_dev));
  } else {
    MD_TRY(model_infer_direct(m, x_dev, B, H, W, raw, need_k ? f_home : nullptr, nullptr, st));
    if (need_k) f_dev = f_home;
  }
  Run r{m, st, B};
  // ---- view filter: raw -> depth, rejected pixels 0 ----
  if (fo) {
    ViewFilterParams v = make_filter_params(B, H, W, *fo);
    v.depth = raw; v.conf = conf;
    v.K = k_dev; v.focal = k_dev ? nullptr : f_dev; v.E = views ? e_dev : nullptr;
    v.depth_out = depth;
    r.begin("points_view_filter");
    MD_TRY(launch_view_filter(v, f->filter.p, st));
    r.end();
  }
  // ---- points ----
  p.depth = depth; p.conf = conf; p.rgb = rgb_dev;
  p.K = k_dev; p.focal = k_dev ? nullptr : f_dev; p.E = o.world ? e_dev : nullptr;
  r.begin("points_unproject");
  MD_TRY(launch_unproject(p, f->scratch.p, st, &q));
  r.end();
  if (!host_out) return MD_OK;
  auto d2h = [&](void* dst, const void* srcp, size_t bytes) -> int {
    if (dst && bytes) MD_HIP(hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, st));
    return MD_OK;
  };
  MD_TRY(d2h(out.depth, depth, npx * 4));
  MD_TRY(d2h(out.point_map, p.point_map, npx * 12));
  MD_TRY(d2h(out.mask, p.mask, npx));
  if (nrm) MD_TRY(d2h(nrm->normal_map, q.normal_map, npx * 12));
  MD_TRY(d2h(out.count, p.count, (size_t)(B + 1) * 4));
  MD_HIP(hipStreamSynchronize(st));  // host outputs are complete when the call returns
  if (out.count) {  // only the points that exist travel: the caller's memory beyond them stays as it was
    const size_t n = std::min((size_t)out.count[B], cap);
    MD_TRY(d2h(out.xyz, p.xyz, n * 12));
    MD_TRY(d2h(out.rgb, p.rgb_out, n * 3));
    MD_TRY(d2h(out.conf, p.conf_out, n * 4));
    if (nrm) MD_TRY(d2h(nrm->normals, q.normals, n * 12));
    MD_HIP(hipStreamSynchronize(st));
  }
  return MD_OK;
}

int infer_points(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                 const md_points_opts* o, const md_points_outputs* out, int out_kind, hipStream_t stream, const md_view_filter_opts* fo,
                 bool filtered, const md_points_normals* nrm) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  if (!nchw) MD_FAIL(MD_ERR_INVALID_ARG, "input pointer is null");
  if ((in_kind != MD_MEM_HOST && in_kind != MD_MEM_DEVICE) || (out_kind != MD_MEM_HOST && out_kind != MD_MEM_DEVICE))
    MD_FAIL(MD_ERR_INVALID_ARG, "unknown memory kind");
  const md_points_cameras none = {nullptr, nullptr, nullptr};
  const md_points_cameras& c = cam ? *cam : none;
  const bool dual = m->kind == 1 && da3_cfg(m).dual_head;
  const bool own_cams = m->kind == 0 || dual;  // Depth Pro predicts a focal length, the dual head's camera decoder K and E
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "point options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  if (filtered && !fo) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (!own_cams && !c.intrinsics && !c.focal_px)
    MD_FAIL(MD_ERR_UNSUPPORTED, "this Depth-Anything-v3 variant has no camera decoder: intrinsics or a focal length are required");
  Sources s;
  s.rgb = rgb != nullptr;
  s.conf = dual;
  s.K = c.intrinsics != nullptr || dual;
  s.focal = c.focal_px != nullptr || m->kind == 0;
  s.E = c.extrinsics != nullptr || dual;
  MD_TRY(check_points(o, out, nrm, s, B, H, W));
  if (fo) {
    MD_TRY(check_filter(fo, s.conf, s.K || s.focal, s.E, B, H, W));
    if (fbits(fo->pixel_offset) != fbits(o->pixel_offset) || depth_min_of(fo->depth_min) != depth_min_of(o->depth_min) ||
        depth_max_of(fo->depth_max) != depth_max_of(o->depth_max))
      MD_FAIL(MD_ERR_INVALID_ARG, "pixel_offset and the depth bounds of the view filter and the point options differ");
  }
  if (B > m->cfg.max_batch) MD_FAIL(MD_ERR_SHAPE, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
  if (m->kind == 0 && c.focal_px && in_kind == MD_MEM_HOST)
    for (int i = 0; i < B; ++i)
      if (!std::isfinite(c.focal_px[i]) || !(c.focal_px[i] > 0.f))
        MD_FAIL(MD_ERR_INVALID_ARG, "f_px[%d] = %g: a focal length must be finite and > 0", i, (double)c.focal_px[i]);
  if (!model_root(m)->committed) MD_FAIL(MD_ERR_INVALID_ARG, "weights were modified; call md_model_commit_weights first");
  MD_HIP(hipSetDevice(m->dev->ordinal));
  hipStream_t st = model_stream(m, stream);
  auto body = [&]() { return points_eager(m, nchw, B, H, W, in_kind, rgb, c, *o, *out, out_kind, dual, st, fo, nrm); };
  if (!m->graph_enabled) return body();
  // the key: stream, shape, every option, every in / out pointer and the commit generation (md_frame.hip); a graph only
  // replays at the model's current input size (its workspace plan)
  const unsigned gen = model_root(m)->commit_gen;
  bool eligible = in_kind == MD_MEM_DEVICE && out_kind == MD_MEM_DEVICE;
  if (m->kind == 1) {
    int ps = 0, ch = 0, cw = 0;
    da3_frame_info(m, &ps, &ch, &cw);
    eligible = eligible && ch == H && cw == W;
  } else {
    eligible = eligible && H == m->S && W == m->S;
  }
  std::vector<uintptr_t> key = {(uintptr_t)0x504f494eu, (uintptr_t)st, (uintptr_t)B, (uintptr_t)H, (uintptr_t)W, (uintptr_t)nchw,
                                      (uintptr_t)rgb, (uintptr_t)c.intrinsics, (uintptr_t)c.extrinsics, (uintptr_t)c.focal_px,
                                      fbits(o->pixel_offset), fbits(o->depth_min), fbits(o->depth_max), fbits(o->conf_min),
                                      fbits(o->edge_rtol), (uintptr_t)o->stride, (uintptr_t)(o->world ? 1 : 0),
                                      (uintptr_t)out->point_map, (uintptr_t)out->mask, (uintptr_t)out->xyz, (uintptr_t)out->rgb,
                                      (uintptr_t)out->conf, (uintptr_t)out->count, (uintptr_t)out->capacity, (uintptr_t)out->depth,
                                      (uintptr_t)gen};
  if (fo) key.insert(key.end(), {(uintptr_t)0x56464c54u, (uintptr_t)fo->conf_percentile, fbits(fo->view_rtol), (uintptr_t)fo->min_views});
  if (nrm && (nrm->normal_map || nrm->normals || nrm->min_cos > 0.f))  // all zero: the key, and the graph, of the call without normals
    key.insert(key.end(), {(uintptr_t)0x4e524d4cu, (uintptr_t)nrm->normal_map, (uintptr_t)nrm->normals, fbits(nrm->min_cos)});
  return run_with_graph(m, st, key, eligible, body);
}

}  // namespace md
