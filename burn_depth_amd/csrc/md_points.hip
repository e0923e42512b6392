// The point path: md_op_unproject (depth + cameras -> point map / mask / ordered cloud on caller tensors) and md_infer_points
// (the model's infer body, then the same kernels on its results, in one call); md_op_unproject_normals / md_infer_points_normals
// are the same two calls with the normals forms of the kernels. model (model_infer / da3_infer_ex bodies) ->
// classify / scan / scatter (kernels/points.hip); one captured graph per replay key when the model replays graphs.
// md_op_filter_views / md_infer_points_filtered put the view filter (kernels/view_filter.hip: confidence percentile, cross-view
// support) in front of those launches: it hands them a depth in which rejected pixels are 0.
// md_op_voxel_thin / md_infer_points_voxel put the voxel thinning (kernels/voxel.hip) behind them: the scatter then fills a list
// of the model's own, and the thinned list goes to the caller.
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
  md::GrowBuf<void> vlist;        // md_infer_points_voxel: the unthinned list (xyz | conf | rgb | normals | count)
  md::GrowBuf<void> vtable;       // its hash table and compaction scratch (voxel_scratch_bytes)
  int vox_rows = 0;               // rows the last thinning call covered (where its flags lie in vtable); 0 = none ran
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

// rows the unthinned list of a model call can have
long list_rows(int B, int H, int W, int stride) { return (long)B * ((H + stride - 1) / stride) * ((W + stride - 1) / stride); }

bool voxel_on(const md_points_voxel* vox) { return vox && vox->voxel != 0.f; }

// model call: voxel == 0 is the call without thinning and takes no thinning output
int check_voxel(const md_points_voxel* vox, const md_points_outputs* out, bool op) {
  if (!vox) return MD_OK;
  if (!std::isfinite(vox->voxel) || vox->voxel < 0.f || (op && vox->voxel == 0.f))
    MD_FAIL(MD_ERR_INVALID_ARG, "voxel = %g: must be finite and %s 0", (double)vox->voxel, op ? ">" : ">=");
  if ((vox->index || vox->weight) && !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "index / weight need `count`");
  if (vox->voxel == 0.f && (vox->index || vox->weight || vox->dropped))
    MD_FAIL(MD_ERR_INVALID_ARG, "index / weight / dropped without a voxel size");
  return MD_OK;
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

int op_voxel_thin(md_device_t dev, const float* xyz_dev, const float* conf_dev, const uint8_t* rgb_dev, const float* normals_dev, int64_t N,
                  const md_points_voxel* vox, const md_points_outputs* out, float* normals_out, hipStream_t stream) {
  if (!vox) MD_FAIL(MD_ERR_INVALID_ARG, "voxel options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_voxel(vox, out, true));
  if (N < 0) MD_FAIL(MD_ERR_INVALID_ARG, "N = %lld is negative", (long long)N);
  if (out->capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "capacity %lld is negative", (long long)out->capacity);
  if (out->point_map || out->mask || out->depth) MD_FAIL(MD_ERR_INVALID_ARG, "voxel thinning has no dense output");
  if ((out->xyz || out->rgb || out->conf || normals_out) && !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "the compacted outputs need `count`");
  if (out->rgb && !rgb_dev) MD_FAIL(MD_ERR_INVALID_ARG, "an rgb output needs an rgb row");
  if (out->conf && !conf_dev) MD_FAIL(MD_ERR_INVALID_ARG, "a conf output needs a confidence row");
  if (normals_out && !normals_dev) MD_FAIL(MD_ERR_INVALID_ARG, "a normals output needs a normals row");
  if (N >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "voxel thinning takes fewer than 2^30 rows, got %lld", (long long)N);
  if (N > 0 && !xyz_dev) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  MD_HIP(hipSetDevice(dev->ordinal));
  hipStream_t st = stream ? stream : dev->stream;
  VoxelParams p;
  p.xyz = xyz_dev; p.conf = conf_dev; p.rgb = rgb_dev; p.normals = normals_dev;
  p.n = (int)N; p.B = 1; p.voxel = vox->voxel;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.index = vox->index; p.weight = vox->weight; p.count = out->count; p.dropped = vox->dropped; p.capacity = out->capacity;
  void* scratch = nullptr;
  MD_HIP(hipMalloc(&scratch, voxel_scratch_bytes(p.n)));
  int rc = launch_voxel_thin(p, scratch, st);
  int32_t flag = 0;
  hipError_t se = hipSuccess;
  if (rc == MD_OK) se = hipMemcpyAsync(&flag, voxel_flags(scratch, p.n), 4, hipMemcpyDeviceToHost, st);
  const hipError_t sy = hipStreamSynchronize(st);  // the scratch is freed on return
  (void)hipFree(scratch);
  if (rc != MD_OK) return rc;
  MD_HIP(se);
  MD_HIP(sy);
  if (flag) MD_FAIL(MD_ERR_HIP, "voxel thinning: the probe loop ran out of table slots");
  return MD_OK;
}

int points_voxel_overflow(md_model_t m, int64_t* out) {
  *out = 0;
  md_model_s::PointsState* f = m->points;
  if (!f || !f->vox_rows || !f->vtable.p) return MD_OK;
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipDeviceSynchronize());  // the call may have run on any stream
  int32_t flag = 0;
  MD_HIP(hipMemcpy(&flag, voxel_flags(f->vtable.p, f->vox_rows), 4, hipMemcpyDeviceToHost));
  *out = flag;
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------
// the model call
// ------------------------------------------------------------------------------------------------
static int points_eager(md_model_s* m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras& cam,
                        const md_points_opts& o, const md_points_outputs& out, int out_kind, bool dual, hipStream_t st,
                        const md_view_filter_opts* fo, const md_points_normals* nrm, const md_points_voxel* vox) {
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
  const bool thin = voxel_on(vox) && out.count;  // without the list there is nothing to thin
  int32_t *v_index = thin ? vox->index : nullptr, *v_weight = thin ? vox->weight : nullptr, *v_dropped = thin ? vox->dropped : nullptr;
  size_t off_map = 0, off_mask = 0, off_xyz = 0, off_rgb = 0, off_conf = 0, off_count = 0, off_nmap = 0, off_nrm = 0, total = 0;
  size_t off_index = 0, off_weight = 0, off_dropped = 0;
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
    off_index = take(v_index, cap * 4);
    off_weight = take(v_weight, cap * 4);
    off_dropped = take(v_dropped, 4);
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
    if (v_index) v_index = (int32_t*)(base + off_index);
    if (v_weight) v_weight = (int32_t*)(base + off_weight);
    if (v_dropped) v_dropped = (int32_t*)(base + off_dropped);
  } else {
    p.point_map = out.point_map; p.mask = out.mask;
    p.xyz = out.xyz; p.rgb_out = out.rgb; p.conf_out = out.conf; p.count = out.count;
  }
  // ---- voxel thinning: the scatter fills the model's own list, the thinning writes where the list would have gone ----
  const PointsParams dst = p;  // the list outputs of the call, on the device
  const NormalsParams dstq = q;
  const long rows = thin ? list_rows(B, H, W, o.stride) : 0;
  if (thin) {
    const size_t b_xyz = align_up((size_t)rows * 12, 256), b_conf = dual ? align_up((size_t)rows * 4, 256) : 0;
    const size_t b_rgb = dst.rgb_out ? align_up((size_t)rows * 3, 256) : 0, b_nrm = dstq.normals ? b_xyz : 0;
    MD_TRY(grow(m, st, f->vlist, b_xyz + b_conf + b_rgb + b_nrm + align_up((size_t)(B + 1) * 4, 256)));
    MD_TRY(grow(m, st, f->vtable, voxel_scratch_bytes((int)rows)));
    char* base = (char*)f->vlist.p;
    p.xyz = (float*)base;
    p.conf_out = dual ? (float*)(base + b_xyz) : nullptr;  // the rank reads the confidence whether or not the caller takes it
    p.rgb_out = dst.rgb_out ? (uint8_t*)(base + b_xyz + b_conf) : nullptr;
    q.normals = dstq.normals ? (float*)(base + b_xyz + b_conf + b_rgb) : nullptr;
    p.count = (int32_t*)(base + b_xyz + b_conf + b_rgb + b_nrm);
    p.capacity = rows;
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
  if (thin) {
    VoxelParams v;
    v.xyz = p.xyz; v.conf = p.conf_out; v.rgb = p.rgb_out; v.normals = q.normals; v.in_count = p.count;
    v.n = (int)rows; v.B = B; v.voxel = vox->voxel;
    v.xyz_out = dst.xyz; v.conf_out = dst.conf_out; v.rgb_out = dst.rgb_out; v.normals_out = dstq.normals;
    v.index = v_index; v.weight = v_weight; v.count = dst.count; v.dropped = v_dropped; v.capacity = dst.capacity;
    r.begin("points_voxel");
    MD_TRY(launch_voxel_thin(v, f->vtable.p, st));
    r.end();
    f->vox_rows = (int)rows;
  }
  if (!host_out) return MD_OK;
  auto d2h = [&](void* dst, const void* srcp, size_t bytes) -> int {
    if (dst && bytes) MD_HIP(hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, st));
    return MD_OK;
  };
  MD_TRY(d2h(out.depth, depth, npx * 4));
  MD_TRY(d2h(out.point_map, p.point_map, npx * 12));
  MD_TRY(d2h(out.mask, p.mask, npx));
  if (nrm) MD_TRY(d2h(nrm->normal_map, q.normal_map, npx * 12));
  MD_TRY(d2h(out.count, dst.count, (size_t)(B + 1) * 4));
  int32_t overflow = 0;
  if (thin) {
    MD_TRY(d2h(vox->dropped, v_dropped, 4));
    MD_TRY(d2h(&overflow, voxel_flags(f->vtable.p, (int)rows), 4));
  }
  MD_HIP(hipStreamSynchronize(st));  // host outputs are complete when the call returns
  if (overflow) MD_FAIL(MD_ERR_HIP, "voxel thinning: the probe loop ran out of table slots");
  if (out.count) {  // only the points that exist travel: the caller's memory beyond them stays as it was
    const size_t n = std::min((size_t)out.count[B], cap);
    MD_TRY(d2h(out.xyz, dst.xyz, n * 12));
    MD_TRY(d2h(out.rgb, dst.rgb_out, n * 3));
    MD_TRY(d2h(out.conf, dst.conf_out, n * 4));
    if (nrm) MD_TRY(d2h(nrm->normals, dstq.normals, n * 12));
    if (thin) {
      MD_TRY(d2h(vox->index, v_index, n * 4));
      MD_TRY(d2h(vox->weight, v_weight, n * 4));
    }
    MD_HIP(hipStreamSynchronize(st));
  }
  return MD_OK;
}

int infer_points(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const uint8_t* rgb, const md_points_cameras* cam,
                 const md_points_opts* o, const md_points_outputs* out, int out_kind, hipStream_t stream, const md_view_filter_opts* fo,
                 bool filtered, const md_points_normals* nrm, const md_points_voxel* vox) {
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
  MD_TRY(check_voxel(vox, out, false));
  if (voxel_on(vox) && list_rows(B, H, W, o->stride) >= (1l << 30))
    MD_FAIL(MD_ERR_SHAPE, "voxel thinning takes fewer than 2^30 rows, the list may have %ld", list_rows(B, H, W, o->stride));
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
  auto body = [&]() { return points_eager(m, nchw, B, H, W, in_kind, rgb, c, *o, *out, out_kind, dual, st, fo, nrm, vox); };
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
  if (voxel_on(vox))  // voxel == 0: the key, and the graph, of the call without thinning
    key.insert(key.end(), {(uintptr_t)0x564f584cu, fbits(vox->voxel), (uintptr_t)vox->index, (uintptr_t)vox->weight, (uintptr_t)vox->dropped});
  return run_with_graph(m, st, key, eligible, body);
}

}  // namespace md
