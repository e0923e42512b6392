// The point path: md_op_unproject (depth + cameras -> point map / mask / ordered cloud on caller tensors) and md_infer_points
// (the model's infer body, then the same kernels on its results, in one call); md_op_unproject_normals / md_infer_points_normals
// are the same two calls with the normals forms of the kernels. model (model_infer / da3_infer_ex bodies) ->
// classify / scan / scatter (kernels/points.hip); one captured graph per replay key when the model replays graphs.
// md_op_filter_views / md_infer_points_filtered put the view filter (kernels/view_filter.hip: confidence percentile, cross-view
// support) in front of those launches: it hands them a depth in which rejected pixels are 0.
// md_op_voxel_thin / md_infer_points_voxel put the voxel thinning (kernels/voxel.hip) behind them: the scatter then fills a list
// of the model's own, and the thinned list goes to the caller.
// md_op_render_points / md_infer_points_render put the rendering (kernels/render.hip) behind those: the list the call ends with,
// thinned or not, is z-buffered into the caller's target cameras.
// md_op_mesh_grid / md_op_unproject_mesh / md_infer_points_mesh put the depth-grid mesh (kernels/mesh.hip) directly behind the
// unprojection: the map pixel -> list row from the scratch the list's launches left, then the faces over the list's rows.
// md_op_render_mesh / md_infer_points_raster put the mesh rasterisation (kernels/raster.hip) behind the rendering: the faces of the
// mesh stage over the list's rows are drawn into the caller's target cameras.
// md_op_radius_outliers / md_infer_points_outlier put the radius outlier removal (kernels/outlier.hip) between the scatter and the
// thinning: the scatter fills a list of the model's own, the filter writes the caller's, or with thinning a second list of the model's.
// md_op_decimate_mesh / md_infer_points_decimate (kernels/decimate.hip), md_op_mesh_components / md_infer_points_components
// (kernels/components.hip) and md_op_smooth_mesh / md_infer_points_smooth (kernels/smooth.hip) work on the mesh stage's faces:
// the decimation writes the list and the faces the call ends with, the other two leave the list as it is.
// md_op_fit_planes / md_infer_points_planes (kernels/planes.hip) label the rows of the list the call ends with by the planes a RANSAC
// finds in it; with mode 1 / 2 the stage is the last one that writes a list.
// md_op_cluster_points / md_infer_points_clusters (kernels/clusters.hip) label the rows of the list the plane stage ends with by
// their DBSCAN cluster; with mode 1 the stage is the last one that writes a list.
// md_op_match_points / md_infer_points_match (kernels/match.hip) give every row of the list the plane stage ends with its nearest
// row of a reference cloud; with mode 1 / 2 the stage is a link of the list chain, between the plane stage and the clustering.
// The fourteen md_infer_points* entries are one request (PointsCall); its stages share one plan of device pointers (PointsPlan),
// which holds the list the call ends with once (PointsPlan::fin, wired to the last list stage in plan_homes).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "md_engine.h"
#include "md_engine_util.h"
#include "kernels/planes_math.h"  // the limits of the plane stage

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
  md::GrowBuf<void> flist;        // md_infer_points_outlier with thinning: the filtered list, laid out as vlist (without it vlist holds the unfiltered one)
  md::GrowBuf<void> otable;       // its table, buckets and ballot words (outlier_scratch_bytes)
  md::GrowBuf<void> rkeys;        // md_infer_points_render: the z-buffer keys (render_scratch_bytes)
  md::GrowBuf<void> mesh;         // md_infer_points_mesh: the face scratch (mesh_scratch_bytes) | pixel_index when the caller takes none
  md::GrowBuf<float> rcams;       // the device copy of host target cameras: K [T,9] | E [T,12] | focal [T]
  md::GrowBuf<void> skeys;        // md_infer_points_raster: the z-buffer keys and the face queue (raster_scratch_bytes)
  md::GrowBuf<float> scams;       // the device copy of its host target cameras, laid out as rcams
  md::GrowBuf<void> dtable;       // md_infer_points_decimate: the decimation's scratch (decimate_scratch_bytes)
  md::GrowBuf<void> dfaces;       // its input: the faces of the unthinned list [2 rows,3] | their face_count [B+1]
                                  // (md_infer_points_components: the unfiltered faces of the call's list, likewise)
  md::GrowBuf<void> ctable;       // md_infer_points_components: the components' scratch (components_scratch_bytes)
  md::GrowBuf<void> stable;       // md_infer_points_smooth: the smoothing's scratch (smooth_scratch_bytes)
  md::GrowBuf<void> ptable;       // md_infer_points_planes: the plane extraction's scratch (planes_scratch_bytes)
  md::GrowBuf<void> plist;        // its input with mode 1 / 2 behind the thinning: the thinned list, laid out as vlist
  md::GrowBuf<void> ktable;       // md_infer_points_clusters: the clustering's scratch (clusters_scratch_bytes)
  md::GrowBuf<void> klist;        // its input with mode 1 behind a plane stage that cuts: that stage's list, laid out as vlist
  md::GrowBuf<void> mtable;       // md_infer_points_match: the matching's scratch (match_scratch_bytes)
  md::GrowBuf<void> mlist;        // the list it writes with mode 1 / 2 when the clustering (mode 1) follows, laid out as vlist
  md::GrowBuf<float> mtarget;     // the device copy of a host target [T,3]
  md::GrowBuf<void> rtable;       // md_infer_points_register: the registration's scratch (register_scratch_bytes)
  md::GrowBuf<float> rtarget;     // the device copy of its host target [T,3]
  md::GrowBuf<float> rnormals;    // md_infer_points_register_plane: the device copy of the host target's normals [T,3]
  int dec_rows = 0, dec_faces = 0, dec_views = 0;  // what the last decimation covered (where its flags lie in dtable); 0 = none ran.
                                                   // Like vox_rows / outl_rows it is set where the stage is enqueued: a graph replay does not move it
  int vox_rows = 0;               // rows the last thinning call covered (where its flags lie in vtable); 0 = none ran
  int outl_rows = 0;              // likewise for the outlier removal and otable
  int clu_rows = 0;               // likewise for the clustering and ktable,
  long clu_table = 0;             // with the table capacity its scratch was carved for
  int mat_rows = 0, mat_target = 0;  // likewise for the matching and mtable: the source rows and the target rows; mat_ran: a call ran
  bool mat_ran = false;
  int reg_rows = 0, reg_target = 0;  // likewise for the registration and rtable
  bool reg_ran = false;
  bool reg_plane = false;  // that registration ran in the point-to-plane form: its flags lie behind 29-leaf tile sums
  float* k_home() const { return cams.p; }
  float* e_home(int B) const { return cams.p + (size_t)B * 9; }
  float* f_home(int B) const { return cams.p + (size_t)B * 21; }
};

namespace md {

void points_destroy_state(md_model_t m) {
  delete m->points;
  m->points = nullptr;
}

namespace {

// ---- the refusals the operators and the model call share, each worded once ----
int check_shape(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1l << 31)) MD_FAIL(MD_ERR_SHAPE, "invalid depth shape [%d,%d,%d]", B, H, W);
  return MD_OK;
}
int check_offset(float v) { if (!std::isfinite(v)) MD_FAIL(MD_ERR_INVALID_ARG, "pixel_offset is not finite"); return MD_OK; }
int check_nonneg(const char* name, float v) {
  if (!std::isfinite(v) || v < 0.f) MD_FAIL(MD_ERR_INVALID_ARG, "%s = %g: must be finite and >= 0", name, (double)v);
  return MD_OK;
}
int check_depth_range(float dmin, float dmax) {
  MD_TRY(check_nonneg("depth_min", dmin));
  MD_TRY(check_nonneg("depth_max", dmax));
  if (dmin > 0.f && dmax > 0.f && dmax < dmin) MD_FAIL(MD_ERR_INVALID_ARG, "depth_max %g < depth_min %g", (double)dmax, (double)dmin);
  return MD_OK;
}
int check_capacity(const md_points_outputs* out) {
  if (out->capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "capacity %lld is negative", (long long)out->capacity);
  return MD_OK;
}
// `what`: list outputs the caller asked for; they are written behind the scan, which needs `count`
int need_count(bool wanted, const md_points_outputs* out, const char* what) {
  if (wanted && !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "%s need `count`", what);
  return MD_OK;
}

struct Sources {  // what the kernels will read, known before the model runs
  bool rgb, conf, K, focal, E;
};

// (the shape is check_shape's, which both callers run next)
int check_points(const md_points_opts* o, const md_points_outputs* out, const md_points_normals* nrm, const Sources& s) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "point options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  if (nrm) {
    if (!std::isfinite(nrm->min_cos) || nrm->min_cos < 0.f || nrm->min_cos > 1.f)
      MD_FAIL(MD_ERR_INVALID_ARG, "min_cos = %g: must lie in [0, 1]", (double)nrm->min_cos);
    MD_TRY(need_count(nrm->normals, out, "the compacted normals"));
  }
  if (o->stride < 1) MD_FAIL(MD_ERR_INVALID_ARG, "stride %d: at least 1", o->stride);
  MD_TRY(check_capacity(out));
  MD_TRY(need_count(out->xyz || out->rgb || out->conf, out, "the compacted outputs"));
  if (out->rgb && !s.rgb) MD_FAIL(MD_ERR_INVALID_ARG, "an rgb output needs an rgb input");
  if (out->conf && !s.conf) MD_FAIL(MD_ERR_INVALID_ARG, "a conf output needs a confidence map");
  MD_TRY(check_offset(o->pixel_offset));
  MD_TRY(check_nonneg("edge_rtol", o->edge_rtol));
  MD_TRY(check_nonneg("conf_min", o->conf_min));
  MD_TRY(check_depth_range(o->depth_min, o->depth_max));
  if (o->world && !s.E) MD_FAIL(MD_ERR_INVALID_ARG, "world = 1 needs extrinsics");
  if (!s.K && !s.focal) MD_FAIL(MD_ERR_INVALID_ARG, "neither intrinsics nor a focal length");
  return MD_OK;
}

// 0 = the default of that bound
float depth_min_of(float v) { return v > 0.f ? v : FLT_MIN; }
float depth_max_of(float v) { return v > 0.f ? v : FLT_MAX; }

PointsParams make_params(int B, int H, int W, const md_points_opts& o) {
  PointsParams p;
  p.B = B; p.H = H; p.W = W;
  p.off = o.pixel_offset; p.dmin = depth_min_of(o.depth_min); p.dmax = depth_max_of(o.depth_max);
  p.conf_min = o.conf_min; p.edge_rtol = o.edge_rtol; p.stride = o.stride; p.world = o.world ? 1 : 0;
  return p;
}

NormalsParams make_normals(const md_points_normals* nrm) {
  NormalsParams q;
  if (nrm) { q.normal_map = nrm->normal_map; q.normals = nrm->normals; q.min_cos = nrm->min_cos; }
  return q;
}

// s.conf / s.K, s.focal / s.E: what the filter will find on the device (the caller's or the model's)
int check_filter(const md_view_filter_opts* o, const Sources& s, int B, int H, int W) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (o->conf_percentile < 0 || o->conf_percentile > 99) MD_FAIL(MD_ERR_INVALID_ARG, "conf_percentile %d outside 0..99", o->conf_percentile);
  if (o->conf_percentile > 0 && !s.conf) MD_FAIL(MD_ERR_INVALID_ARG, "conf_percentile > 0 needs a confidence map");
  MD_TRY(check_nonneg("view_rtol", o->view_rtol));
  MD_TRY(check_offset(o->pixel_offset));
  MD_TRY(check_depth_range(o->depth_min, o->depth_max));
  const bool views = o->view_rtol > 0.f;
  if (!views && o->min_views != 0) MD_FAIL(MD_ERR_INVALID_ARG, "min_views %d without view_rtol", o->min_views);
  if (views && o->min_views < 1) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs min_views >= 1, got %d", o->min_views);
  if (views && !s.E) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs extrinsics");
  if (views && !s.K && !s.focal) MD_FAIL(MD_ERR_INVALID_ARG, "view_rtol > 0 needs intrinsics or a focal length");
  MD_TRY(check_shape(B, H, W));
  if (B >= 65536) MD_FAIL(MD_ERR_SHAPE, "invalid depth shape [%d,%d,%d]", B, H, W);
  if (views && (B < 2 || B > kViewFilterMaxViews)) MD_FAIL(MD_ERR_SHAPE, "view_rtol > 0 takes 2..%d views, got %d", kViewFilterMaxViews, B);
  if (views && (H >= (1 << 24) || W >= (1 << 24))) MD_FAIL(MD_ERR_SHAPE, "view_rtol > 0: image sides below 2^24, got %d x %d", H, W);
  if (views && o->min_views > B - 1) MD_FAIL(MD_ERR_INVALID_ARG, "min_views %d: only %d other views", o->min_views, B - 1);
  return MD_OK;
}

ViewFilterParams make_filter_params(int B, int H, int W, const md_view_filter_opts& o) {
  ViewFilterParams p;
  p.B = B; p.H = H; p.W = W;
  p.off = o.pixel_offset; p.dmin = depth_min_of(o.depth_min); p.dmax = depth_max_of(o.depth_max);
  p.q = o.conf_percentile; p.rtol = o.view_rtol; p.min_views = o.min_views;
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
  MD_TRY(need_count(vox->index || vox->weight, out, "index / weight"));
  if (vox->voxel == 0.f && (vox->index || vox->weight || vox->dropped))
    MD_FAIL(MD_ERR_INVALID_ARG, "index / weight / dropped without a voxel size");
  return MD_OK;
}

bool decimate_on(const md_points_decimate* d) { return d && d->voxel != 0.f; }

// model call: voxel == 0 is the call without decimation and takes none of its outputs
int check_decimate(const md_points_decimate* d, const md_points_outputs* out, bool op) {
  if (!d) return MD_OK;
  if (!std::isfinite(d->voxel) || d->voxel < 0.f || (op && d->voxel == 0.f))
    MD_FAIL(MD_ERR_INVALID_ARG, "voxel = %g: must be finite and %s 0", (double)d->voxel, op ? ">" : ">=");
  if (d->voxel == 0.f) {
    if (d->index || d->weight || d->dropped || d->remap || d->faces || d->face_index || d->face_count || d->faces_dropped)
      MD_FAIL(MD_ERR_INVALID_ARG, "decimation outputs without a voxel size");
    return MD_OK;
  }
  if (d->face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "face_capacity %lld is negative", (long long)d->face_capacity);
  if ((d->faces || d->face_index) && !d->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "faces / face_index need `face_count`");
  MD_TRY(need_count(d->index || d->weight, out, "index / weight"));
  return MD_OK;
}

bool components_on(const md_points_components* k) { return k && k->min_faces != 0; }

// model call: min_faces == 0 is the call without the stage and takes none of its outputs; the in-call stage is face-only
int check_components_part(const md_points_components* k) {
  if (!k) return MD_OK;
  if (k->min_faces < 0) MD_FAIL(MD_ERR_INVALID_ARG, "min_faces = %d: must be >= 0", k->min_faces);
  if (k->compact) MD_FAIL(MD_ERR_INVALID_ARG, "the model call does not compact the list: `compact` must be 0");
  if (k->index || k->remap) MD_FAIL(MD_ERR_INVALID_ARG, "index / remap without `compact`");
  if (k->min_faces == 0) {
    if (k->label || k->component_faces || k->faces || k->face_index || k->face_count || k->stats)
      MD_FAIL(MD_ERR_INVALID_ARG, "component outputs without min_faces");
    return MD_OK;
  }
  if (k->face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "face_capacity %lld is negative", (long long)k->face_capacity);
  if ((k->faces || k->face_index) && !k->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "faces / face_index need `face_count`");
  return MD_OK;
}

bool smooth_on(const md_points_smooth* s) { return s && s->iterations != 0; }

// the contract's limits of a stage that is on; the negated forms refuse a NaN
int check_smooth_values(const md_points_smooth* s) {
  if (!(s->step > 0.f) || !std::isfinite(s->step)) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: step = %g must be finite and > 0", (double)s->step);
  if (!(s->lambda > 0.f && s->lambda <= 1.f)) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: lambda = %g must lie in (0, 1]", (double)s->lambda);
  if (!(s->mu >= -1.f && s->mu <= 0.f)) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: mu = %g must lie in [-1, 0]", (double)s->mu);
  if (s->iterations < 1 || s->iterations > 1024) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: iterations = %d must lie in 1..1024", s->iterations);
  return MD_OK;
}

// model call: iterations == 0 is the call without the stage and takes none of its outputs
int check_smooth_part(const md_points_smooth* s) {
  if (!s) return MD_OK;
  if (s->iterations == 0) {
    if (s->xyz || s->normals || s->stats) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing outputs without iterations");
    return MD_OK;
  }
  return check_smooth_values(s);
}

bool planes_on(const md_points_planes* f) { return f && f->planes != 0; }

// model call: planes == 0 is the call without the stage and takes none of its outputs. has_normals: there is a normals row
int check_planes(const md_points_planes* f, const md_points_outputs* out, bool has_normals, bool op) {
  if (!f) return MD_OK;
  if (f->planes == 0 && !op) {
    if (f->plane || f->plane_count || f->hypothesis || f->label || f->index || f->dropped) MD_FAIL(MD_ERR_INVALID_ARG, "plane outputs without planes");
    return MD_OK;
  }
  if (f->planes < 1 || f->planes > kPlanesMax) MD_FAIL(MD_ERR_INVALID_ARG, "planes = %d: must lie in 1..%d", f->planes, kPlanesMax);
  if (f->hypotheses < 1 || f->hypotheses > kPlaneHypothesesMax)
    MD_FAIL(MD_ERR_INVALID_ARG, "hypotheses = %d: must lie in 1..%d", f->hypotheses, kPlaneHypothesesMax);
  if (!(f->tol > 0.f) || !std::isfinite(f->tol)) MD_FAIL(MD_ERR_INVALID_ARG, "tol = %g: must be finite and > 0", (double)f->tol);
  if (f->min_inliers < 3) MD_FAIL(MD_ERR_INVALID_ARG, "min_inliers = %d: must be >= 3", f->min_inliers);
  if (!(f->normal_min_cos >= 0.f && f->normal_min_cos <= 1.f)) MD_FAIL(MD_ERR_INVALID_ARG, "normal_min_cos = %g: must lie in [0, 1]", (double)f->normal_min_cos);
  if (!(f->axis_min_cos >= 0.f && f->axis_min_cos <= 1.f)) MD_FAIL(MD_ERR_INVALID_ARG, "axis_min_cos = %g: must lie in [0, 1]", (double)f->axis_min_cos);
  if (f->mode < 0 || f->mode > 2) MD_FAIL(MD_ERR_INVALID_ARG, "mode = %d: 0, 1 or 2", f->mode);
  if (f->normal_min_cos > 0.f && !has_normals) MD_FAIL(MD_ERR_INVALID_ARG, "normal_min_cos > 0 needs the normals rows");
  if (f->axis_min_cos > 0.f && !(std::isfinite(f->axis[0]) && std::isfinite(f->axis[1]) && std::isfinite(f->axis[2])))
    MD_FAIL(MD_ERR_INVALID_ARG, "axis_min_cos > 0 needs a finite axis");
  if (f->index && f->mode == 0) MD_FAIL(MD_ERR_INVALID_ARG, "index needs mode 1 or 2");
  MD_TRY(need_count(f->index, out, "index"));
  return MD_OK;
}

// the options and the outputs of the stage's own; the caller adds the rows
PlanesParams make_planes(const md_points_planes& f) {
  PlanesParams q;
  q.planes = f.planes; q.hypotheses = f.hypotheses; q.min_inliers = f.min_inliers; q.mode = f.mode; q.seed = f.seed;
  q.tol = f.tol; q.normal_min_cos = f.normal_min_cos; q.axis_min_cos = f.axis_min_cos;
  q.axis[0] = f.axis[0]; q.axis[1] = f.axis[1]; q.axis[2] = f.axis[2];
  q.plane = f.plane; q.plane_count = f.plane_count; q.hypothesis = f.hypothesis; q.label = f.label; q.dropped = f.dropped; q.index = f.index;
  return q;
}

bool clusters_on(const md_points_clusters* q) { return q && q->radius != 0.f; }

// model call: radius == 0 is the call without the stage and takes none of its outputs
int check_clusters(const md_points_clusters* q, const md_points_outputs* out, bool op) {
  if (!q) return MD_OK;
  if (!std::isfinite(q->radius) || q->radius < 0.f || (op && q->radius == 0.f))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: must be finite and %s 0", (double)q->radius, op ? ">" : ">=");
  if (q->radius == 0.f) {
    if (q->label || q->cluster_size || q->cluster || q->table_label || q->table_size || q->box || q->stats || q->index || q->dropped)
      MD_FAIL(MD_ERR_INVALID_ARG, "cluster outputs without a radius");
    return MD_OK;
  }
  if (q->min_neighbours < 0 || q->min_neighbours > kClusterMaxNeighbours)
    MD_FAIL(MD_ERR_INVALID_ARG, "min_neighbours %d outside 0..%d", q->min_neighbours, kClusterMaxNeighbours);
  if (q->min_points < 1) MD_FAIL(MD_ERR_INVALID_ARG, "min_points = %d: must be >= 1", q->min_points);
  if (q->max_points < 0 || (q->max_points > 0 && q->max_points < q->min_points))
    MD_FAIL(MD_ERR_INVALID_ARG, "max_points = %d: 0 or >= min_points = %d", q->max_points, q->min_points);
  if (q->mode < 0 || q->mode > 1) MD_FAIL(MD_ERR_INVALID_ARG, "mode = %d: 0 or 1", q->mode);
  if (q->table_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "table_capacity = %lld is negative", (long long)q->table_capacity);
  if (q->index && q->mode == 0) MD_FAIL(MD_ERR_INVALID_ARG, "index needs mode 1");
  MD_TRY(need_count(q->index, out, "index"));
  return MD_OK;
}

// the options and the outputs of the stage's own; the caller adds the rows
ClustersParams make_clusters(const md_points_clusters& f) {
  ClustersParams q;
  q.radius = f.radius; q.k = f.min_neighbours; q.min_points = f.min_points; q.max_points = f.max_points; q.mode = f.mode;
  q.label = f.label; q.cluster_size = f.cluster_size; q.cluster = f.cluster;
  q.table_label = f.table_label; q.table_size = f.table_size; q.box = f.box; q.table_capacity = (long)f.table_capacity;
  q.stats = f.stats; q.index = f.index; q.dropped = f.dropped;
  return q;
}

bool match_on(const md_points_match* q) { return q && q->radius != 0.f; }
bool register_on(const md_points_register* q) { return q && q->radius != 0.f; }
bool register_plane_on(const md_points_register_plane* q) { return q && q->target_normals; }

// model call: radius == 0 is the call without the stage and takes none of its outputs; the operator takes a device target only
int check_match(const md_points_match* q, const md_points_outputs* out, bool op) {
  if (!q) return MD_OK;
  if (!std::isfinite(q->radius) || q->radius < 0.f || (op && q->radius == 0.f) || !std::isfinite(q->radius * q->radius))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: it and its square must be finite and %s 0", (double)q->radius, op ? ">" : ">=");
  if (q->radius == 0.f) {
    if (q->nearest || q->dist2 || q->stats || q->index || q->dropped) MD_FAIL(MD_ERR_INVALID_ARG, "match outputs without a radius");
    return MD_OK;
  }
  for (int t = 0; t < 4; ++t)
    if (!(q->tol[t] >= 0.f) || !(q->tol[t] <= q->radius))
      MD_FAIL(MD_ERR_INVALID_ARG, "tol[%d] = %g: 0 or in (0, radius = %g]", t, (double)q->tol[t], (double)q->radius);
  if (q->mode < 0 || q->mode > 2) MD_FAIL(MD_ERR_INVALID_ARG, "mode = %d: 0, 1 or 2", q->mode);
  if (q->target_rows < 0) MD_FAIL(MD_ERR_INVALID_ARG, "target_rows = %lld is negative", (long long)q->target_rows);
  if (q->target_rows > 0 && !q->target) MD_FAIL(MD_ERR_INVALID_ARG, "target pointer is null");
  if (q->target_kind != MD_MEM_DEVICE && (op || q->target_kind != MD_MEM_HOST))
    MD_FAIL(MD_ERR_INVALID_ARG, "target_kind = %d: %s", q->target_kind, op ? "the operator takes a device target" : "unknown memory kind");
  if (q->index && q->mode == 0) MD_FAIL(MD_ERR_INVALID_ARG, "index needs mode 1 or 2");
  MD_TRY(need_count(q->index, out, "index"));
  if (q->target_rows >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "matching takes fewer than 2^30 target rows, got %lld", (long long)q->target_rows);
  return MD_OK;
}

// the options and the outputs of the stage's own; the caller adds the rows (and a host target's device copy)
MatchParams make_match(const md_points_match& f) {
  MatchParams q;
  q.radius = f.radius; q.target = f.target; q.t = (int)f.target_rows; q.mode = f.mode;
  for (int t = 0; t < 4; ++t) q.tol[t] = f.tol[t];
  q.nearest = f.nearest; q.dist2 = f.dist2; q.stats = f.stats; q.index = f.index; q.dropped = f.dropped;
  return q;
}

bool outlier_on(const md_points_outlier* q) { return q && q->radius != 0.f; }

// model call: radius == 0 is the call without outlier removal and takes none of its outputs. The operator's `neighbours` covers
// the input rows and needs no list; in the model call nothing is filtered without `count`.
int check_outlier(const md_points_outlier* q, const md_points_outputs* out, bool op) {
  if (!q) return MD_OK;
  if (!std::isfinite(q->radius) || q->radius < 0.f || (op && q->radius == 0.f))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: must be finite and %s 0", (double)q->radius, op ? ">" : ">=");
  if (q->radius == 0.f) {
    if (q->neighbours || q->index || q->dropped) MD_FAIL(MD_ERR_INVALID_ARG, "neighbours / index / dropped without a radius");
    return MD_OK;
  }
  if (q->min_neighbours < 1 || q->min_neighbours > kOutlierMaxNeighbours)
    MD_FAIL(MD_ERR_INVALID_ARG, "min_neighbours %d outside 1..%d", q->min_neighbours, kOutlierMaxNeighbours);
  MD_TRY(need_count(q->index || (!op && q->neighbours), out, op ? "index" : "neighbours / index"));
  return MD_OK;
}

// The refusals the rendering and the rasterising share, in two halves around the options of their own. what / done: "render" /
// "rendered" or "raster" / "rasterised"; has_rgb: there is an rgb row to gather from
bool any_output(const md_render_outputs& o) { return o.depth || o.index || o.rgb || o.filled; }
bool any_output(const md_raster_outputs& o) { return o.depth || o.face || o.rgb || o.filled || o.skipped; }
template <typename Opts, typename Outs>
int check_target_args(const char* what, const char* done, const md_points_cameras* cam, const Opts* o, const Outs* out, bool has_rgb) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "%s options are null", what);
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "%s outputs are null", what);
  if (!cam) MD_FAIL(MD_ERR_INVALID_ARG, "target cameras are null");
  if (!any_output(*out)) MD_FAIL(MD_ERR_INVALID_ARG, "every %s output is null", what);
  if (out->rgb && !has_rgb) MD_FAIL(MD_ERR_INVALID_ARG, "a %s rgb output needs an rgb row", done);
  if (!cam->intrinsics && !cam->focal_px) MD_FAIL(MD_ERR_INVALID_ARG, "neither intrinsics nor a focal length for the target cameras");
  return MD_OK;
}
template <typename Opts>
int check_target_view(const char* what, int T, int H, int W, const Opts& o) {
  MD_TRY(check_offset(o.pixel_offset));
  MD_TRY(check_nonneg("z_near", o.z_near));
  MD_TRY(check_nonneg("z_far", o.z_far));
  if (o.z_near > 0.f && o.z_far > 0.f && o.z_far < o.z_near) MD_FAIL(MD_ERR_INVALID_ARG, "z_far %g < z_near %g", (double)o.z_far, (double)o.z_near);
  if (T <= 0 || H <= 0 || W <= 0 || (long)T * H * W >= (1l << 31) || H >= (1 << 24) || W >= (1 << 24))
    MD_FAIL(MD_ERR_SHAPE, "invalid %s target shape [%d,%d,%d]", what, T, H, W);
  return MD_OK;
}

// the rendering part of the operator and of the model call
int check_render(int T, int H, int W, const md_points_cameras* cam, const md_render_opts* o, const md_render_outputs* out, bool has_rgb) {
  MD_TRY(check_target_args("render", "rendered", cam, o, out, has_rgb));
  if (o->radius < 0 || o->radius > kRenderMaxRadius) MD_FAIL(MD_ERR_INVALID_ARG, "radius %d outside 0..%d", o->radius, kRenderMaxRadius);
  return check_target_view("render", T, H, W, *o);
}

RenderParams make_render(int T, int H, int W, const md_render_opts& o) {
  RenderParams r;
  r.T = T; r.H = H; r.W = W;
  r.off = o.pixel_offset; r.znear = depth_min_of(o.z_near); r.zfar = depth_max_of(o.z_far); r.radius = o.radius;
  return r;
}

// the rasterising part of md_op_render_mesh and of the model call
int check_raster(int T, int H, int W, const md_points_cameras* cam, const md_raster_opts* o, const md_raster_outputs* out, bool has_rgb) {
  MD_TRY(check_target_args("raster", "rasterised", cam, o, out, has_rgb));
  if (o->cull != 0 && o->cull != 1) MD_FAIL(MD_ERR_INVALID_ARG, "cull %d: 0 or 1", o->cull);
  if (o->max_extent < 0 || o->max_extent > kRasterMaxExtent) MD_FAIL(MD_ERR_INVALID_ARG, "max_extent %d outside 0..%d", o->max_extent, kRasterMaxExtent);
  return check_target_view("raster", T, H, W, *o);
}

RasterParams make_raster(int T, int H, int W, const md_raster_opts& o, const md_raster_outputs& out) {
  RasterParams r;
  r.T = T; r.H = H; r.W = W;
  r.off = o.pixel_offset; r.znear = depth_min_of(o.z_near); r.zfar = depth_max_of(o.z_far);
  r.cull = o.cull; r.max_extent = o.max_extent ? o.max_extent : kRasterDefaultExtent;
  r.depth = out.depth; r.face = out.face; r.rgb_out = out.rgb; r.filled = out.filled; r.skipped = out.skipped;
  return r;
}

// a mesh part whose three outputs are null is the call without it
bool mesh_on(const md_points_mesh* g) { return g && (g->faces || g->face_count || g->pixel_index); }

// the mesh part of the operators and of the model call. has_count: the list's `count` is written (md_op_mesh_grid has no list:
// true); thin: voxel thinning is on. The shape is check_shape's, which every caller runs first.
int check_mesh(const md_points_mesh* g, bool has_count, bool thin, int B, int H, int W) {
  if (!g) return MD_OK;
  MD_TRY(check_nonneg("max_rtol", g->max_rtol));
  if (g->face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "face_capacity %lld is negative", (long long)g->face_capacity);
  if (g->faces && !g->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "faces need `face_count`");
  if (!mesh_on(g)) return MD_OK;
  if (!has_count) MD_FAIL(MD_ERR_INVALID_ARG, "a mesh needs the list's `count`");
  if (thin) MD_FAIL(MD_ERR_INVALID_ARG, "a mesh together with voxel thinning: the rows its faces name no longer exist");
  if ((long)B * H * W >= (1l << 30)) MD_FAIL(MD_ERR_SHAPE, "a mesh takes fewer than 2^30 pixels, got [%d,%d,%d]", B, H, W);
  return MD_OK;
}

// limit: a corner is usable below it (the list's capacity, or md_op_mesh_grid's vertex_limit with 0 already resolved)
MeshParams make_mesh(int B, int H, int W, int stride, long limit, const md_points_mesh& g) {
  MeshParams q;
  q.B = B; q.H = H; q.W = W; q.stride = stride; q.limit = limit; q.max_rtol = g.max_rtol;
  q.faces = g.faces; q.face_count = g.face_count; q.face_capacity = (long)g.face_capacity;
  return q;
}

// bytes behind the list's scratch that the mesh stage needs: the face scratch, and a pixel_index home when faces are wanted and
// the caller takes no map
size_t mesh_home_bytes(const md_points_mesh& g, int B, int H, int W, int stride) {
  if (!g.face_count) return 0;
  return mesh_scratch_bytes(B, H, W, stride) + (g.pixel_index ? 0 : align_up((size_t)B * H * W * 4, 256));
}

// The mesh stage: pixel_index from the bits and offsets the list's launches left in `points_scratch`, then the faces. q.depth is
// set; `pix`: where the map goes (null: the tail of `home`, behind the face scratch).
int launch_mesh(MeshParams q, int32_t* pix, const void* points_scratch, void* home, hipStream_t st) {
  if (!pix && !q.face_count) return MD_OK;
  if (!pix) pix = (int32_t*)((char*)home + mesh_scratch_bytes(q.B, q.H, q.W, q.stride));
  MD_TRY(launch_mesh_index(q.B, q.H, q.W, points_scratch, pix, st));
  q.pixel_index = pix;
  return launch_mesh_grid(q, home, st);
}

uint32_t fbits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// A graph replay key grows word by word: pointers by address, integers by value, floats by bit pattern.
uintptr_t key_word(float v) { return fbits(v); }
uintptr_t key_word(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  return (uintptr_t)u;
}
template <typename T>
uintptr_t key_word(T v) { return (uintptr_t)v; }
template <typename... T>
void key_add(std::vector<uintptr_t>& key, T... v) { (key.push_back(key_word(v)), ...); }

// The scratch of a stand-alone operator: allocated for the call and gone when it returns. finish() waits for the stream (the
// launches read the scratch), frees it and folds the launch's code, a readback's error and the wait's error, in that order.
// Nothing allocated: nothing to wait for, finish() hands `rc` on. An early return between alloc and finish ends the same way.
struct OpScratch {
  hipStream_t st;
  void* p = nullptr;
  explicit OpScratch(hipStream_t s) : st(s) {}
  OpScratch(const OpScratch&) = delete;
  OpScratch& operator=(const OpScratch&) = delete;
  ~OpScratch() { (void)finish(MD_OK); }
  int alloc(size_t bytes) { MD_HIP(hipMalloc(&p, bytes)); return MD_OK; }
  int finish(int rc, hipError_t copy = hipSuccess) {
    if (!p) return rc;
    const hipError_t sync = hipStreamSynchronize(st);
    (void)hipFree(p);
    p = nullptr;
    if (rc != MD_OK) return rc;
    MD_HIP(copy);
    MD_HIP(sync);
    return MD_OK;
  }
  // finish() behind launches that leave probe-loop flags in the scratch: the words at `a` and `b` (null: never reset, not read)
  // are read before the scratch they lie in is freed; a set one is the refusal `ran_out`
  int finish_flags(int rc, const int32_t* a, const int32_t* b, const char* ran_out) {
    int32_t flag[2] = {0, 0};
    hipError_t copy = hipSuccess;
    if (rc == MD_OK && a) copy = hipMemcpyAsync(&flag[0], a, 4, hipMemcpyDeviceToHost, st);
    if (rc == MD_OK && copy == hipSuccess && b) copy = hipMemcpyAsync(&flag[1], b, 4, hipMemcpyDeviceToHost, st);
    MD_TRY(finish(rc, copy));
    if (flag[0] || flag[1]) MD_FAIL(MD_ERR_HIP, "%s", ran_out);
    return MD_OK;
  }
};

// a set probe-loop flag, as the operators and the model call report it
const char kVoxelRanOut[] = "voxel thinning: the probe loop ran out of table slots";
const char kOutlierRanOut[] = "outlier removal: a probe loop ran out of table slots";
const char kDecimateRanOut[] = "decimation: a probe loop ran out of table slots";
const char kClustersRanOut[] = "clustering: a probe loop ran out of table slots";
const char kMatchRanOut[] = "matching: a probe loop ran out of table slots";
const char kRegisterRanOut[] = "registration: a probe loop ran out of table slots";

// Every operator's last refusal and first act: the device, made current, and the stream its launches take.
int op_begin(md_device_t dev, hipStream_t stream, hipStream_t* st) {
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  MD_HIP(hipSetDevice(dev->ordinal));
  *st = stream ? stream : dev->stream;
  return MD_OK;
}

// The refusals of the operators that take a list (and faces over its rows: F given) and write a list, in the order all of them
// keep: the sizes, the outputs, the limits. `noun` names the operator; the components, a plural with outputs of their own
// between these, call the parts.
int check_list_sizes(const PointList& in, const int64_t* F) {
  if (in.N < 0) MD_FAIL(MD_ERR_INVALID_ARG, "N = %lld is negative", (long long)in.N);
  if (F && *F < 0) MD_FAIL(MD_ERR_INVALID_ARG, "F = %lld is negative", (long long)*F);
  return MD_OK;
}
int check_list_rows(const PointList& in, const md_points_outputs* out, const float* normals_out) {
  if (out->rgb && !in.rgb) MD_FAIL(MD_ERR_INVALID_ARG, "an rgb output needs an rgb row");
  if (out->conf && !in.conf) MD_FAIL(MD_ERR_INVALID_ARG, "a conf output needs a confidence row");
  if (normals_out && !in.normals) MD_FAIL(MD_ERR_INVALID_ARG, "a normals output needs a normals row");
  return MD_OK;
}
int check_list_limits(const char* noun, const char* takes, const PointList& in, bool reads_xyz, const int32_t* faces, const int64_t* F) {
  if (in.N >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "%s %s fewer than 2^30 rows, got %lld", noun, takes, (long long)in.N);
  if (F && *F >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "%s %s fewer than 2^30 faces, got %lld", noun, takes, (long long)*F);
  if (reads_xyz && in.N > 0 && !in.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  if (F && *F > 0 && !faces) MD_FAIL(MD_ERR_INVALID_ARG, "faces pointer is null");
  return MD_OK;
}
int check_list_op(const char* noun, const PointList& in, const md_points_outputs* out, const float* normals_out,
                  const int32_t* faces = nullptr, const int64_t* F = nullptr) {
  MD_TRY(check_list_sizes(in, F));
  MD_TRY(check_capacity(out));
  if (out->point_map || out->mask || out->depth) MD_FAIL(MD_ERR_INVALID_ARG, "%s has no dense output", noun);
  MD_TRY(need_count(out->xyz || out->rgb || out->conf || normals_out, out, "the compacted outputs"));
  MD_TRY(check_list_rows(in, out, normals_out));
  return check_list_limits(noun, "takes", in, true, faces, F);
}

}  // namespace

int op_unproject(md_device_t dev, const DepthMaps& in, const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out,
                 const md_points_normals* nrm, hipStream_t stream, const md_points_mesh* mesh) {
  if (!cam) MD_FAIL(MD_ERR_INVALID_ARG, "cameras are null");
  const Sources s{in.rgb != nullptr, in.conf != nullptr, cam->intrinsics != nullptr, cam->focal_px != nullptr, cam->extrinsics != nullptr};
  MD_TRY(check_points(o, out, nrm, s));
  MD_TRY(check_shape(in.B, in.H, in.W));
  MD_TRY(check_mesh(mesh, out->count != nullptr, false, in.B, in.H, in.W));
  if (!in.depth) MD_FAIL(MD_ERR_INVALID_ARG, "depth pointer is null");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  PointsParams p = make_params(in.B, in.H, in.W, *o);
  p.depth = in.depth; p.conf = in.conf; p.rgb = in.rgb;
  p.K = cam->intrinsics; p.focal = cam->focal_px; p.E = cam->extrinsics;
  p.point_map = out->point_map; p.mask = out->mask;
  p.xyz = out->xyz; p.rgb_out = out->rgb; p.conf_out = out->conf; p.count = out->count; p.capacity = out->capacity;
  OpScratch scratch(st);
  const size_t b_list = p.count ? points_scratch_bytes(in.B, in.H, in.W) : 0;
  const size_t b_mesh = mesh_on(mesh) ? mesh_home_bytes(*mesh, in.B, in.H, in.W, o->stride) : 0;
  if (b_list) MD_TRY(scratch.alloc(b_list + b_mesh));
  const NormalsParams q = make_normals(nrm);
  int rc = launch_unproject(p, scratch.p, st, &q);
  if (rc == MD_OK && mesh_on(mesh)) {  // the vertices are the rows the list outputs hold
    MeshParams g = make_mesh(in.B, in.H, in.W, o->stride, (long)out->capacity, *mesh);
    g.depth = in.depth;
    rc = launch_mesh(g, mesh->pixel_index, scratch.p, (char*)scratch.p + b_list, st);
  }
  return scratch.finish(rc);
}

int op_mesh_grid(md_device_t dev, const DepthMaps& in, const int32_t* pixel_index, int stride, int64_t vertex_limit, const md_points_mesh* mesh,
                 hipStream_t stream) {
  if (!mesh) MD_FAIL(MD_ERR_INVALID_ARG, "mesh is null");
  if (stride < 1) MD_FAIL(MD_ERR_INVALID_ARG, "stride %d: at least 1", stride);
  if (vertex_limit < 0) MD_FAIL(MD_ERR_INVALID_ARG, "vertex_limit %lld is negative", (long long)vertex_limit);
  if (!in.depth || !pixel_index) MD_FAIL(MD_ERR_INVALID_ARG, "depth or pixel_index pointer is null");
  MD_TRY(check_shape(in.B, in.H, in.W));
  md_points_mesh faces_only = *mesh;
  faces_only.pixel_index = nullptr;
  MD_TRY(check_mesh(&faces_only, true, false, in.B, in.H, in.W));
  if (!dev) MD_FAIL(MD_ERR_INVALID_ARG, "device is null");
  if (!mesh->face_count) return MD_OK;  // nothing to launch: the device stays as it was
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  MeshParams g = make_mesh(in.B, in.H, in.W, stride, vertex_limit ? (long)vertex_limit : LONG_MAX, *mesh);
  g.depth = in.depth; g.pixel_index = pixel_index;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(mesh_scratch_bytes(in.B, in.H, in.W, stride)));
  return scratch.finish(launch_mesh_grid(g, scratch.p, st));
}

int op_filter_views(md_device_t dev, const DepthMaps& in, const md_points_cameras* cam, const md_view_filter_opts* o,
                    const md_view_filter_outputs* out, hipStream_t stream) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "view filter outputs are null");
  if (!out->depth && !out->support && !out->conf_threshold && !out->kept) MD_FAIL(MD_ERR_INVALID_ARG, "every view filter output is null");
  if (out->depth && out->depth == in.depth) MD_FAIL(MD_ERR_INVALID_ARG, "the filtered depth may not be the input");
  const md_points_cameras none = {nullptr, nullptr, nullptr};
  const md_points_cameras& c = cam ? *cam : none;
  const Sources s{false, in.conf != nullptr, c.intrinsics != nullptr, c.focal_px != nullptr, c.extrinsics != nullptr};
  MD_TRY(check_filter(o, s, in.B, in.H, in.W));
  if (!in.depth) MD_FAIL(MD_ERR_INVALID_ARG, "depth pointer is null");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  ViewFilterParams p = make_filter_params(in.B, in.H, in.W, *o);
  p.depth = in.depth; p.conf = in.conf;
  p.K = c.intrinsics; p.focal = c.intrinsics ? nullptr : c.focal_px; p.E = c.extrinsics;
  p.depth_out = out->depth; p.support = out->support; p.tau = out->conf_threshold; p.kept = out->kept;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(view_filter_scratch_bytes()));
  return scratch.finish(launch_view_filter(p, scratch.p, st));
}

int op_voxel_thin(md_device_t dev, const PointList& in, const md_points_voxel* vox, const md_points_outputs* out, float* normals_out,
                  hipStream_t stream) {
  if (!vox) MD_FAIL(MD_ERR_INVALID_ARG, "voxel options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_voxel(vox, out, true));
  MD_TRY(check_list_op("voxel thinning", in, out, normals_out));
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  VoxelParams p;
  p.xyz = in.xyz; p.conf = in.conf; p.rgb = in.rgb; p.normals = in.normals;
  p.n = (int)in.N; p.B = 1; p.voxel = vox->voxel;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.index = vox->index; p.weight = vox->weight; p.count = out->count; p.dropped = vox->dropped; p.capacity = out->capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(voxel_scratch_bytes(p.n)));
  return scratch.finish_flags(launch_voxel_thin(p, scratch.p, st), voxel_flags(scratch.p, p.n), nullptr, kVoxelRanOut);
}

int op_radius_outliers(md_device_t dev, const PointList& in, const md_points_outlier* outl, const md_points_outputs* out, float* normals_out,
                       hipStream_t stream) {
  if (!outl) MD_FAIL(MD_ERR_INVALID_ARG, "outlier options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_outlier(outl, out, true));
  MD_TRY(check_list_op("outlier removal", in, out, normals_out));
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  OutlierParams p;
  p.xyz = in.xyz; p.conf = in.conf; p.rgb = in.rgb; p.normals = in.normals;
  p.n = (int)in.N; p.B = 1; p.radius = outl->radius; p.k = outl->min_neighbours;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.index = outl->index; p.neighbours = outl->neighbours; p.count = out->count; p.dropped = outl->dropped; p.capacity = out->capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(outlier_scratch_bytes(p.n)));
  return scratch.finish_flags(launch_radius_outliers(p, scratch.p, st), outlier_flags(scratch.p, p.n), nullptr, kOutlierRanOut);
}

int op_fit_planes(md_device_t dev, const PointList& in, const md_points_planes* pln, const md_points_outputs* out, float* normals_out,
                  hipStream_t stream) {
  if (!pln) MD_FAIL(MD_ERR_INVALID_ARG, "plane options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_planes(pln, out, in.normals != nullptr, true));
  MD_TRY(check_list_op("plane extraction", in, out, normals_out));
  if (pln->mode == 0 && (out->xyz || out->rgb || out->conf || normals_out)) MD_FAIL(MD_ERR_INVALID_ARG, "mode 0 writes no list: the compacted outputs need mode 1 or 2");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  PlanesParams p = make_planes(*pln);
  p.xyz = in.xyz; p.conf = in.conf; p.rgb = in.rgb; p.normals = in.normals;
  p.n = (int)in.N; p.B = 1;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.count = pln->mode ? out->count : nullptr; p.capacity = out->capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(planes_scratch_bytes(p.n, p.hypotheses)));
  return scratch.finish(launch_fit_planes(p, scratch.p, st));
}

int op_cluster_points(md_device_t dev, const PointList& in, const md_points_clusters* clu, const md_points_outputs* out, float* normals_out,
                      hipStream_t stream) {
  if (!clu) MD_FAIL(MD_ERR_INVALID_ARG, "cluster options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_clusters(clu, out, true));
  MD_TRY(check_list_op("clustering", in, out, normals_out));
  if (clu->mode == 0 && (out->xyz || out->rgb || out->conf || normals_out)) MD_FAIL(MD_ERR_INVALID_ARG, "mode 0 writes no list: the compacted outputs need mode 1");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  ClustersParams p = make_clusters(*clu);
  p.xyz = in.xyz; p.conf = in.conf; p.rgb = in.rgb; p.normals = in.normals;
  p.n = (int)in.N; p.B = 1;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.count = clu->mode ? out->count : nullptr; p.capacity = out->capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(clusters_scratch_bytes(p.n, p.table_capacity)));
  return scratch.finish_flags(launch_cluster_points(p, scratch.p, st), clusters_flags(scratch.p, p.n, p.table_capacity), nullptr, kClustersRanOut);
}

int op_match_points(md_device_t dev, const PointList& in, const md_points_match* mat, const md_points_outputs* out, float* normals_out,
                    hipStream_t stream) {
  if (!mat) MD_FAIL(MD_ERR_INVALID_ARG, "match options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_match(mat, out, true));
  MD_TRY(check_list_op("matching", in, out, normals_out));
  if (mat->mode == 0 && (out->xyz || out->rgb || out->conf || normals_out)) MD_FAIL(MD_ERR_INVALID_ARG, "mode 0 writes no list: the compacted outputs need mode 1 or 2");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  MatchParams p = make_match(*mat);
  p.xyz = in.xyz; p.conf = in.conf; p.rgb = in.rgb; p.normals = in.normals;
  p.n = (int)in.N; p.B = 1;
  p.xyz_out = out->xyz; p.conf_out = out->conf; p.rgb_out = out->rgb; p.normals_out = normals_out;
  p.count = mat->mode ? out->count : nullptr; p.capacity = out->capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(match_scratch_bytes(p.n, p.t)));
  return scratch.finish_flags(launch_match_points(p, scratch.p, st), match_flags(scratch.p, p.n, p.t), nullptr, kMatchRanOut);
}

namespace {

// The refusals of md_points_register before any launch: the matching's of radius, target and sizes, then the stage's own.
int check_register(const md_points_register* q, bool op) {
  if (!q) return MD_OK;
  if (!std::isfinite(q->radius) || q->radius < 0.f || (op && q->radius == 0.f) || !std::isfinite(q->radius * q->radius))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: it and its square must be finite and %s 0", (double)q->radius, op ? ">" : ">=");
  if (q->radius == 0.f) {
    if (q->transform || q->pairs || q->sum_d2 || q->stats || q->dropped || q->nearest || q->dist2)
      MD_FAIL(MD_ERR_INVALID_ARG, "register outputs without a radius");
    return MD_OK;
  }
  if (q->target_rows < 0) MD_FAIL(MD_ERR_INVALID_ARG, "target_rows = %lld is negative", (long long)q->target_rows);
  if (q->target_rows > 0 && !q->target) MD_FAIL(MD_ERR_INVALID_ARG, "target pointer is null");
  if (q->target_kind != MD_MEM_DEVICE && (op || q->target_kind != MD_MEM_HOST))
    MD_FAIL(MD_ERR_INVALID_ARG, "target_kind = %d: %s", q->target_kind, op ? "the operator takes a device target" : "unknown memory kind");
  if (q->apply != 0 && q->apply != 1) MD_FAIL(MD_ERR_INVALID_ARG, "apply = %d: 0 or 1", q->apply);
  if (q->target_rows >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "registration takes fewer than 2^30 target rows, got %lld", (long long)q->target_rows);
  if (q->iterations < 1 || q->iterations > 64) MD_FAIL(MD_ERR_INVALID_ARG, "iterations = %d outside 1..64", q->iterations);
  if (q->min_pairs < 3) MD_FAIL(MD_ERR_INVALID_ARG, "min_pairs = %d: at least 3", q->min_pairs);
  if (!(q->rot_eps >= 0.) || !std::isfinite(q->rot_eps) || !(q->trans_eps >= 0.) || !std::isfinite(q->trans_eps))
    MD_FAIL(MD_ERR_INVALID_ARG, "rot_eps = %g, trans_eps = %g: finite and >= 0", q->rot_eps, q->trans_eps);
  if (q->init)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(q->init[i])) MD_FAIL(MD_ERR_INVALID_ARG, "init[%d] = %g is not finite", i, q->init[i]);
  return MD_OK;
}

// The refusals of md_points_register_plane before any launch, behind check_register's. Without target_normals the part is off
// and nothing of it is read.
int check_register_plane(const md_points_register* q, const md_points_register_plane* pl) {
  if (!register_plane_on(pl)) return MD_OK;
  if (!register_on(q) || !q->target) MD_FAIL(MD_ERR_INVALID_ARG, "target_normals without a target");
  if (q->min_pairs < 6) MD_FAIL(MD_ERR_INVALID_ARG, "min_pairs = %d: the point-to-plane form takes at least 6", q->min_pairs);
  return MD_OK;
}

// the options and the outputs of the stage's own; the caller adds the rows. pl on: the point-to-plane form
RegisterParams make_register(const md_points_register& f, const md_points_register_plane* pl = nullptr) {
  RegisterParams q;
  if (register_plane_on(pl)) {
    q.plane = true; q.target_normals = pl->target_normals; q.sum_r2 = pl->sum_r2;
  }
  q.radius = f.radius; q.target = f.target; q.t = (int)f.target_rows;
  q.iterations = f.iterations; q.min_pairs = f.min_pairs; q.rot_eps = f.rot_eps; q.trans_eps = f.trans_eps;
  if (f.init)
    for (int i = 0; i < 12; ++i) q.init[i] = f.init[i];
  q.transform = f.transform; q.pairs = f.pairs; q.sum_d2 = f.sum_d2; q.stats = f.stats; q.dropped = f.dropped;
  q.nearest = f.nearest; q.dist2 = f.dist2;
  return q;
}

}  // namespace

int op_register_points(md_device_t dev, const float* xyz, const float* normals, int64_t N, const md_points_register* reg, float* xyz_out,
                       float* normals_out, hipStream_t stream, const md_points_register_plane* plane) {
  if (!reg) MD_FAIL(MD_ERR_INVALID_ARG, "register options are null");
  MD_TRY(check_register(reg, true));
  MD_TRY(check_register_plane(reg, plane));
  if (N < 0) MD_FAIL(MD_ERR_INVALID_ARG, "N = %lld is negative", (long long)N);
  if (normals_out && !normals) MD_FAIL(MD_ERR_INVALID_ARG, "a normals output needs a normals row");
  if (N >= (1ll << 30)) MD_FAIL(MD_ERR_SHAPE, "registration takes fewer than 2^30 rows, got %lld", (long long)N);
  if (N > 0 && !xyz) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  RegisterParams p = make_register(*reg, plane);
  p.xyz = xyz; p.normals = normals; p.n = (int)N; p.B = 1;
  p.xyz_out = xyz_out; p.normals_out = normals_out;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(p.plane ? register_plane_scratch_bytes(p.n, p.t) : register_scratch_bytes(p.n, p.t)));
  const int32_t* flags = p.plane ? register_plane_flags(scratch.p, p.n, p.t) : register_flags(scratch.p, p.n, p.t);
  return scratch.finish_flags(launch_register_points(p, scratch.p, st), flags, nullptr, kRegisterRanOut);
}

int op_decimate_mesh(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const md_points_decimate* dec,
                     const md_points_outputs* out, float* normals_out, hipStream_t stream) {
  if (!dec) MD_FAIL(MD_ERR_INVALID_ARG, "decimation options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  MD_TRY(check_decimate(dec, out, true));
  MD_TRY(check_list_op("decimation", in, out, normals_out, faces, &F));
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  DecimateParams p;
  p.v.xyz = in.xyz; p.v.conf = in.conf; p.v.rgb = in.rgb; p.v.normals = in.normals;
  p.v.n = (int)in.N; p.v.B = 1; p.v.voxel = dec->voxel;
  p.v.xyz_out = out->xyz; p.v.conf_out = out->conf; p.v.rgb_out = out->rgb; p.v.normals_out = normals_out;
  p.v.index = dec->index; p.v.weight = dec->weight; p.v.count = out->count; p.v.dropped = dec->dropped; p.v.capacity = out->capacity;
  p.remap = dec->remap; p.faces = faces; p.nf = (int)F;
  p.faces_out = dec->faces; p.face_index = dec->face_index; p.face_count = dec->face_count; p.faces_dropped = dec->faces_dropped;
  p.face_capacity = (long)dec->face_capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(decimate_scratch_bytes(p.v.n, p.nf, 1)));
  const bool face_side = p.faces_out || p.face_index || p.face_count || p.faces_dropped;  // otherwise the face table was never reset
  return scratch.finish_flags(launch_decimate_mesh(p, scratch.p, st), voxel_flags(scratch.p, p.v.n),
                              face_side ? decimate_flags(scratch.p, p.v.n, p.nf, 1) : nullptr, kDecimateRanOut);
}

int op_mesh_components(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const md_points_components* comp,
                       const md_points_outputs* out, float* normals_out, hipStream_t stream) {
  if (!comp) MD_FAIL(MD_ERR_INVALID_ARG, "component options are null");
  if (comp->min_faces < 1) MD_FAIL(MD_ERR_INVALID_ARG, "min_faces = %d: must be >= 1", comp->min_faces);
  MD_TRY(check_list_sizes(in, &F));
  if (comp->face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "face_capacity %lld is negative", (long long)comp->face_capacity);
  if ((comp->faces || comp->face_index) && !comp->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "faces / face_index need `face_count`");
  if (out && (out->point_map || out->mask || out->depth)) MD_FAIL(MD_ERR_INVALID_ARG, "components have no dense output");
  if (!comp->compact) {
    if (comp->index || comp->remap || normals_out || (out && (out->xyz || out->rgb || out->conf || out->count)))
      MD_FAIL(MD_ERR_INVALID_ARG, "vertex outputs, index, remap and count need `compact`");
  } else {
    if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
    MD_TRY(check_capacity(out));
    MD_TRY(need_count(out->xyz || out->rgb || out->conf || normals_out || comp->index, out, "the compacted outputs"));
    if (out->xyz && !in.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "an xyz output needs the xyz rows");
    MD_TRY(check_list_rows(in, out, normals_out));
  }
  MD_TRY(check_list_limits("components", "take", in, false, faces, &F));  // in.N bounds the corners: the rows themselves may be absent
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  ComponentsParams p;
  p.v.n = (int)in.N; p.v.B = 1;
  if (comp->compact) {
    p.v.xyz = in.xyz; p.v.conf = in.conf; p.v.rgb = in.rgb; p.v.normals = in.normals;
    p.v.xyz_out = out->xyz; p.v.conf_out = out->conf; p.v.rgb_out = out->rgb; p.v.normals_out = normals_out;
    p.v.index = comp->index; p.v.count = out->count; p.v.capacity = out->capacity;
    p.compact = 1; p.remap = comp->remap;
  }
  p.faces = faces; p.nf = (int)F; p.min_faces = comp->min_faces;
  p.label = comp->label; p.component_faces = comp->component_faces;
  p.faces_out = comp->faces; p.face_index = comp->face_index; p.face_count = comp->face_count; p.stats = comp->stats;
  p.face_capacity = (long)comp->face_capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(components_scratch_bytes(p.v.n, p.nf, 1)));
  return scratch.finish(launch_mesh_components(p, scratch.p, st));
}

int op_smooth_mesh(md_device_t dev, const float* xyz, int64_t N, const int32_t* faces, int64_t F, const md_points_smooth* smooth, int64_t capacity,
                   hipStream_t stream) {
  if (!smooth) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing options are null");
  MD_TRY(check_smooth_values(smooth));
  PointList in;
  in.xyz = xyz; in.N = N;
  MD_TRY(check_list_sizes(in, &F));
  if (capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "capacity %lld is negative", (long long)capacity);
  MD_TRY(check_list_limits("smoothing", "takes", in, true, faces, &F));
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  SmoothParams p;
  p.xyz = xyz; p.n = (int)N; p.faces = faces; p.nf = (int)F;
  p.step = smooth->step; p.lambda = smooth->lambda; p.mu = smooth->mu; p.iterations = smooth->iterations; p.pin_boundary = smooth->pin_boundary;
  p.xyz_out = smooth->xyz; p.normals_out = smooth->normals; p.stats = smooth->stats; p.capacity = (long)capacity;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(smooth_scratch_bytes(p.n)));
  return scratch.finish(launch_smooth_mesh(p, scratch.p, st));
}

int op_render_points(md_device_t dev, const PointList& in, const int32_t* count, int T, int H, int W, const md_points_cameras* cam,
                     const md_render_opts* o, const md_render_outputs* out, hipStream_t stream) {
  MD_TRY(check_render(T, H, W, cam, o, out, in.rgb != nullptr));
  if (in.N < 0 || in.N >= (1ll << 31)) MD_FAIL(MD_ERR_SHAPE, "rendering takes 0 .. 2^31 - 1 rows, got %lld", (long long)in.N);
  if (in.N > 0 && !in.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  RenderParams r = make_render(T, H, W, *o);
  r.xyz = in.xyz; r.rgb = in.rgb; r.count = count; r.n = (int)in.N;
  r.K = cam->intrinsics; r.focal = cam->intrinsics ? nullptr : cam->focal_px; r.E = cam->extrinsics;
  r.depth = out->depth; r.index = out->index; r.rgb_out = out->rgb; r.filled = out->filled;
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(render_scratch_bytes(T, H, W)));
  return scratch.finish(launch_render_points(r, scratch.p, st));
}

int op_render_mesh(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const int32_t* face_count, int T, int H, int W,
                   const md_points_cameras* cam, const md_raster_opts* o, const md_raster_outputs* out, hipStream_t stream) {
  MD_TRY(check_raster(T, H, W, cam, o, out, in.rgb != nullptr));
  if (in.N < 0 || in.N >= (1ll << 31)) MD_FAIL(MD_ERR_SHAPE, "rasterising takes 0 .. 2^31 - 1 rows, got %lld", (long long)in.N);
  if (F < 0 || F >= (1ll << 31)) MD_FAIL(MD_ERR_SHAPE, "rasterising takes 0 .. 2^31 - 1 faces, got %lld", (long long)F);
  if (in.N > 0 && !in.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  if (F > 0 && !faces) MD_FAIL(MD_ERR_INVALID_ARG, "faces pointer is null");
  hipStream_t st;
  MD_TRY(op_begin(dev, stream, &st));
  RasterParams r = make_raster(T, H, W, *o, *out);
  r.xyz = in.xyz; r.rgb = in.rgb; r.n = (int)in.N; r.faces = faces; r.nf = (int)F; r.count = face_count;
  r.K = cam->intrinsics; r.focal = cam->intrinsics ? nullptr : cam->focal_px; r.E = cam->extrinsics;
  const int entries = raster_queue_entries();
  OpScratch scratch(st);
  MD_TRY(scratch.alloc(raster_scratch_bytes(T, H, W, entries)));
  return scratch.finish(launch_render_mesh(r, scratch.p, entries, st));
}

namespace {

// The probe-loop flags the model's last call of a stage left in its table: the word at `a`, and with `b` whether either is set.
// a null: the stage never ran, 0.
int read_overflow(md_model_t m, const int32_t* a, const int32_t* b, int64_t* out) {
  *out = 0;
  if (!a) return MD_OK;
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipDeviceSynchronize());  // the call may have run on any stream
  int32_t flag[2] = {0, 0};
  MD_HIP(hipMemcpy(&flag[0], a, 4, hipMemcpyDeviceToHost));
  if (b) MD_HIP(hipMemcpy(&flag[1], b, 4, hipMemcpyDeviceToHost));
  *out = b ? (flag[0] || flag[1]) : flag[0];
  return MD_OK;
}

}  // namespace

int points_voxel_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  return read_overflow(m, f && f->vox_rows && f->vtable.p ? voxel_flags(f->vtable.p, f->vox_rows) : nullptr, nullptr, out);
}

int points_outlier_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  return read_overflow(m, f && f->outl_rows && f->otable.p ? outlier_flags(f->otable.p, f->outl_rows) : nullptr, nullptr, out);
}

int points_clusters_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  return read_overflow(m, f && f->clu_rows && f->ktable.p ? clusters_flags(f->ktable.p, f->clu_rows, f->clu_table) : nullptr, nullptr, out);
}

int points_register_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  if (!f || !f->reg_ran || !f->rtable.p) return read_overflow(m, nullptr, nullptr, out);
  return read_overflow(m, f->reg_plane ? register_plane_flags(f->rtable.p, f->reg_rows, f->reg_target) : register_flags(f->rtable.p, f->reg_rows, f->reg_target),
                       nullptr, out);
}

int points_match_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  return read_overflow(m, f && f->mat_ran && f->mtable.p ? match_flags(f->mtable.p, f->mat_rows, f->mat_target) : nullptr, nullptr, out);
}

int points_decimate_overflow(md_model_t m, int64_t* out) {
  const md_model_s::PointsState* f = m->points;
  if (!f || !f->dec_views || !f->dtable.p) return read_overflow(m, nullptr, nullptr, out);
  return read_overflow(m, voxel_flags(f->dtable.p, f->dec_rows), decimate_flags(f->dtable.p, f->dec_rows, f->dec_faces, f->dec_views), out);
}

// ------------------------------------------------------------------------------------------------
// the model call
// ------------------------------------------------------------------------------------------------
namespace {

// A list's rows on the device: what one list stage writes and the next one, or the caller, reads.
struct ListRows {
  float* xyz = nullptr;
  float* conf = nullptr;
  uint8_t* rgb = nullptr;
  float* normals = nullptr;
  int32_t* count = nullptr;  // [B + 1]
};

// the launch parameters that read a list and write one: VoxelParams (the decimation's vertex side too), OutlierParams, PlanesParams, MatchParams and ClustersParams
template <typename P>
void reads(P& p, const ListRows& l) { p.xyz = l.xyz; p.conf = l.conf; p.rgb = l.rgb; p.normals = l.normals; p.in_count = l.count; }
template <typename P>
void writes(P& p, const ListRows& l) { p.xyz_out = l.xyz; p.conf_out = l.conf; p.rgb_out = l.rgb; p.normals_out = l.normals; p.count = l.count; }

struct OutSlot {  // a host output's way back: rows of `row_bytes` from its device home to the caller
  void* caller;
  const void* home;
  size_t row_bytes, rows;
  const int32_t* live;  // null: all `rows` travel, with the dense maps and the counts. Else the host word that holds the live
                        // rows once those have arrived (a count's last word): min(*live, rows) rows travel behind them
};

// What the stages of one call share: its device pointers, resolved by plan_homes, stage_inputs and run_model. It lives in
// points_eager and is never copied: a slot may point at `unfiltered`.
struct PointsPlan {
  hipStream_t st = nullptr;
  bool dual = false;
  bool thin = false, mesh = false, filt = false, deci = false, comp = false, smo = false, pln = false;  // the stages that are on
  bool pcut = false;  // pln with mode 1 / 2: the plane stage writes a list
  bool clu = false, ccut = false;  // the clustering is on; with mode 1: it is the last stage that writes a list
  bool mat = false, mcut = false;  // the matching is on; with mode 1 / 2: it writes a list, between the plane stage and the clustering
  bool own_faces = false;  // deci / comp / smo: a later stage reads the faces, so the mesh stage writes the model's own (`gd`)
  size_t npx = 0;
  long rows = 0;  // rows the unthinned list of the call can have (list_rows); its mesh has at most 2 * rows faces
  float *depth = nullptr, *raw = nullptr, *conf = nullptr;  // depth: what is unprojected; raw: what the model writes
  const float* x = nullptr;                                 // the image on the device
  ListRows fin;     // the list the call ends with: the caller's pointers or their host-output homes (place_outputs). plan_homes
                    // hands it to the last stage that writes a list; the rendering and the rasterising read it
  const int32_t* faces = nullptr;       // mesh: the faces the call ends with, which the rasterising reads: the mesh stage's,
  const int32_t* face_count = nullptr;  // the decimated or those of the kept components (the caller's pointers or their homes)
  long face_capacity = 0;
  PointsParams p;   // launch_unproject's; the device inputs gather in p.rgb / K / E / focal (all kept until run_unproject)
  NormalsParams q;
  VoxelParams v;    // thin: launch_voxel_thin's
  OutlierParams u;  // filt: launch_radius_outliers'
  RenderParams r;   // c.rnd given: launch_render_points', from `fin`
  MeshParams g;     // mesh: launch_mesh's, from the depth that is unprojected and the scratch of `p`'s launches
  RasterParams s;   // c.rst given: launch_render_mesh's, from `fin` and `faces`
  DecimateParams d; // deci: launch_decimate_mesh's, from the model's own list and the faces `gd` wrote
  MeshParams gd;    // own_faces: the mesh stage's second set of face outputs, the model's own, complete and with the true count
  ComponentsParams k;  // comp: launch_mesh_components', from the list's count and the faces `gd` wrote
  SmoothParams sm;     // smo: launch_smooth_mesh's, from `fin` and the faces of `k`, or else those `gd` wrote
  PlanesParams pn;     // pln: launch_fit_planes', from `fin` (mode 0) or the model's own list in front of it (pcut)
  ClustersParams cn;   // clu: launch_cluster_points', from `fin` (mode 0) or the model's own list in front of it (ccut)
  MatchParams mn;      // mat: launch_match_points', from `fin` (mode 0) or the model's own list in front of it (mcut)
  const float* host_target = nullptr;  // mat with a host target: the caller's rows, which stage_inputs copies to mtarget
  int queue = 0;    // the raster's queue entries: what skeys was sized for
  int32_t* pix = nullptr;  // where pixel_index goes: the caller's map or its home; null: behind the face scratch
  int32_t unfiltered = 0;  // filt with host outputs: the rows of the unfiltered list, read back for outl->neighbours' slot
  int32_t plane_rows = 0;  // pcut with host outputs: the rows of the plane stage's input list, read back for pln->label's slot
  int32_t cluster_rows = 0;  // ccut with host outputs: the rows of the clustering's input list, for the slots of its row outputs
  int32_t clusters_kept = 0; // clu with host outputs: the kept clusters, for the slots of the table
  bool reg = false;          // the registration is on, directly in front of the matching
  RegisterParams rg;         // reg: launch_register_points', on the list the matching reads (or would read)
  const float* host_reg_target = nullptr;  // reg with a host target: the caller's rows, which stage_inputs copies to rtarget
  const float* host_reg_normals = nullptr; // reg in the point-to-plane form with a host target: its normals, copied to rnormals
  int32_t register_rows = 0; // reg on a list of the model's own, with host outputs: its rows, for the slots of nearest / dist2
  int32_t match_rows = 0;    // mcut with host outputs: the rows of the matching's input list, for the slots of its row outputs
  std::vector<OutSlot> slots;
};

bool views_on(const PointsCall& c) { return c.fo && c.fo->view_rtol > 0.f; }

// The outputs a caller may hold in host memory, in the order they travel: the dense maps and the counts, then the list. Device
// outputs: the kernel parameter takes the caller's pointer. Host outputs: it takes a home inside `base` (PointsState::out, at
// 256-byte steps) and a slot records the way back; base null = the sizes only, so plan_homes runs the table twice around the
// grow. A row's second argument is the parameter itself, by reference. The list rows name `fin`, whichever stage writes it; a
// stage's own outputs follow under its flag. -> bytes of the homes
size_t place_outputs(const PointsCall& c, PointsPlan& pl, char* base) {
  const md_points_outputs& out = *c.out;
  const bool host = c.out_kind == MD_MEM_HOST;
  const size_t cap = (size_t)out.capacity, views = (size_t)c.B + 1, list = (size_t)pl.rows;
  float* const no_f = nullptr;
  auto total_of = [&](const int32_t* count) { return count ? count + c.B : nullptr; };  // the live rows of all views
  const int32_t* const n = total_of(out.count);
  size_t total = 0;
  pl.slots.clear();
  auto slot = [&](auto* caller, auto*& param, size_t row_bytes, size_t rows, const int32_t* live = nullptr) {
    param = caller;
    if (!caller || !host) return;
    if (base) {
      param = (decltype(caller))(base + total);
      pl.slots.push_back(OutSlot{caller, param, row_bytes, rows, live});
    }
    total += align_up(row_bytes * rows, 256);
  };
  slot(out.point_map, pl.p.point_map, 12, pl.npx);
  slot(out.mask, pl.p.mask, 1, pl.npx);
  slot(c.nrm ? c.nrm->normal_map : no_f, pl.q.normal_map, 12, pl.npx);
  slot(out.count, pl.fin.count, 4, views);
  if (pl.thin) slot(c.vox->dropped, pl.v.dropped, 4, 1);
  if (pl.filt) slot(c.outl->dropped, pl.u.dropped, 4, 1);
  if (pl.pln) {
    const size_t P = (size_t)c.pln->planes;
    slot(c.pln->plane, pl.pn.plane, 16, P);
    slot(c.pln->plane_count, pl.pn.plane_count, 4, P + 1);
    slot(c.pln->hypothesis, pl.pn.hypothesis, 4, P);
    slot(c.pln->dropped, pl.pn.dropped, 4, 1);
  }
  if (pl.deci) {
    slot(c.dec->dropped, pl.d.v.dropped, 4, 1);
    slot(c.dec->face_count, pl.d.face_count, 4, views);
    slot(c.dec->faces_dropped, pl.d.faces_dropped, 4, 3);
    slot(c.dec->remap, pl.d.remap, 4, list);
  }
  slot(out.xyz, pl.fin.xyz, 12, cap, n);
  slot(out.rgb, pl.fin.rgb, 3, cap, n);
  slot(out.conf, pl.fin.conf, 4, cap, n);
  slot(c.nrm ? c.nrm->normals : no_f, pl.fin.normals, 12, cap, n);
  if (pl.thin) {
    slot(c.vox->index, pl.v.index, 4, cap, n);
    slot(c.vox->weight, pl.v.weight, 4, cap, n);
  }
  if (pl.filt) {  // index: rows parallel to the filtered list, which the thinning replaces; neighbours: to the unfiltered one
    if (!pl.thin) slot(c.outl->index, pl.u.index, 4, cap, n);
    slot(c.outl->neighbours, pl.u.neighbours, 4, list, &pl.unfiltered);
  }
  if (pl.deci) {
    const size_t fcap = (size_t)c.dec->face_capacity;
    slot(c.dec->index, pl.d.v.index, 4, cap, n);
    slot(c.dec->weight, pl.d.v.weight, 4, cap, n);
    slot(c.dec->faces, pl.d.faces_out, 12, fcap, total_of(c.dec->face_count));
    slot(c.dec->face_index, pl.d.face_index, 4, fcap, total_of(c.dec->face_count));
  }
  if (c.rnd) {  // rendered images are dense outputs: they travel whole
    RenderParams& r = pl.r;
    const size_t rpx = (size_t)r.T * r.H * r.W;
    slot(c.rnd->out.depth, r.depth, 4, rpx);
    slot(c.rnd->out.index, r.index, 4, rpx);
    slot(c.rnd->out.rgb, r.rgb_out, 3, rpx);
    slot(c.rnd->out.filled, r.filled, 4, (size_t)r.T + 1);
  }
  if (c.rst) {  // as the rendered images
    RasterParams& s = pl.s;
    const size_t spx = (size_t)s.T * s.H * s.W;
    slot(c.rst->out.depth, s.depth, 4, spx);
    slot(c.rst->out.face, s.face, 4, spx);
    slot(c.rst->out.rgb, s.rgb_out, 3, spx);
    slot(c.rst->out.filled, s.filled, 4, (size_t)s.T + 1);
    slot(c.rst->out.skipped, s.skipped, 4, (size_t)s.T + 1);
  }
  if (pl.mesh) {
    slot(c.mesh->pixel_index, pl.pix, 4, pl.npx);
    slot(c.mesh->face_count, pl.g.face_count, 4, views);
    slot(c.mesh->faces, pl.g.faces, 12, (size_t)c.mesh->face_capacity, total_of(c.mesh->face_count));
  }
  if (pl.comp) {
    const md_points_components& k = *c.comp;
    slot(k.label, pl.k.label, 4, list);
    slot(k.component_faces, pl.k.component_faces, 4, list);
    slot(k.face_count, pl.k.face_count, 4, views);
    slot(k.stats, pl.k.stats, 4, 5);
    slot(k.faces, pl.k.faces_out, 12, (size_t)k.face_capacity, total_of(k.face_count));
    slot(k.face_index, pl.k.face_index, 4, (size_t)k.face_capacity, total_of(k.face_count));
  }
  if (pl.pln) {  // label: rows parallel to the stage's input, which is the list of the call (mode 0) or the list in front of it
    if (pl.pcut) slot(c.pln->label, pl.pn.label, 4, list, &pl.plane_rows);
    else slot(c.pln->label, pl.pn.label, 4, cap, n);
    slot(c.pln->index, pl.pn.index, 4, cap, n);
  }
  if (pl.clu) {  // the row outputs as the plane stage's label; the table's rows that exist
    const md_points_clusters& k = *c.clu;
    const size_t tcap = (size_t)k.table_capacity;
    slot(k.stats, pl.cn.stats, 4, 4);
    slot(k.dropped, pl.cn.dropped, 4, 1);
    if (pl.ccut) {
      slot(k.label, pl.cn.label, 4, list, &pl.cluster_rows);
      slot(k.cluster_size, pl.cn.cluster_size, 4, list, &pl.cluster_rows);
      slot(k.cluster, pl.cn.cluster, 4, list, &pl.cluster_rows);
    } else {
      slot(k.label, pl.cn.label, 4, cap, n);
      slot(k.cluster_size, pl.cn.cluster_size, 4, cap, n);
      slot(k.cluster, pl.cn.cluster, 4, cap, n);
    }
    slot(k.index, pl.cn.index, 4, cap, n);
    slot(k.table_label, pl.cn.table_label, 4, tcap, &pl.clusters_kept);
    slot(k.table_size, pl.cn.table_size, 4, tcap, &pl.clusters_kept);
    slot(k.box, pl.cn.box, 24, tcap, &pl.clusters_kept);
  }
  if (pl.reg) {  // nearest / dist2 lie over the rows of the list the stage reads, as the matching's
    const md_points_register& q = *c.reg;
    const size_t history = (size_t)q.iterations + 1;
    slot(q.transform, pl.rg.transform, 8, 12);
    slot(q.pairs, pl.rg.pairs, 4, history);
    slot(q.sum_d2, pl.rg.sum_d2, 8, history);
    if (pl.rg.plane) slot(c.rpl->sum_r2, pl.rg.sum_r2, 8, history);
    slot(q.stats, pl.rg.stats, 4, 8);
    slot(q.dropped, pl.rg.dropped, 4, 1);
    if (pl.mcut || pl.ccut) {
      slot(q.nearest, pl.rg.nearest, 4, list, &pl.register_rows);
      slot(q.dist2, pl.rg.dist2, 4, list, &pl.register_rows);
    } else {
      slot(q.nearest, pl.rg.nearest, 4, cap, n);
      slot(q.dist2, pl.rg.dist2, 4, cap, n);
    }
  }
  if (pl.mat) {  // the row outputs as the plane stage's label
    const md_points_match& q = *c.mat;
    slot(q.stats, pl.mn.stats, 4, 8);
    slot(q.dropped, pl.mn.dropped, 4, 1);
    if (pl.mcut) {
      slot(q.nearest, pl.mn.nearest, 4, list, &pl.match_rows);
      slot(q.dist2, pl.mn.dist2, 4, list, &pl.match_rows);
    } else {
      slot(q.nearest, pl.mn.nearest, 4, cap, n);
      slot(q.dist2, pl.mn.dist2, 4, cap, n);
    }
    slot(q.index, pl.mn.index, 4, cap, n);
  }
  if (pl.smo) {  // rows parallel to the list: they travel as its rows do
    slot(c.smooth->xyz, pl.sm.xyz_out, 12, cap, n);
    slot(c.smooth->normals, pl.sm.normals_out, 12, cap, n);
    slot(c.smooth->stats, pl.sm.stats, 4, 5);
  }
  return total;
}

// The model's face home, carved from dfaces: every face the mesh of the unthinned list can have [2 rows,3] and their counts
// [B + 1]. `gd` is `g` writing there.
int carve_faces(md_model_s* m, PointsPlan& pl, int B) {
  md_model_s::PointsState* f = m->points;
  const long nf = 2 * pl.rows;
  const size_t b_faces = align_up((size_t)nf * 12, 256);
  MD_TRY(grow(m, pl.st, f->dfaces, b_faces + align_up((size_t)(B + 1) * 4, 256)));
  pl.gd = pl.g;
  pl.gd.faces = (int32_t*)f->dfaces.p; pl.gd.face_count = (int32_t*)((char*)f->dfaces.p + b_faces); pl.gd.face_capacity = nf;
  return MD_OK;
}

// Device homes, grow-only, in a fixed order and before anything is enqueued: the maps, the cameras, the scratch, the host
// outputs, the model's own lists and faces. Then the wiring of the list stages.
int plan_homes(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  md_model_s::PointsState* f = m->points;
  hipStream_t st = pl.st;
  const md_points_outputs& out = *c.out;
  const int B = c.B, H = c.H, W = c.W, stride = c.o->stride;
  const long rows = pl.rows, nf = 2 * rows;
  pl.depth = out.depth;
  if (!pl.depth || c.out_kind == MD_MEM_HOST) {
    MD_TRY(grow(m, st, f->depth, pl.npx * 4));
    pl.depth = f->depth.p;
  }
  pl.raw = pl.depth;  // with the filter, `depth` takes the filtered map
  if (c.fo) {
    MD_TRY(grow(m, st, f->raw, pl.npx * 4));
    pl.raw = f->raw.p;
    MD_TRY(grow(m, st, f->filter, view_filter_scratch_bytes()));
  }
  if (pl.dual) {
    MD_TRY(grow(m, st, f->conf, pl.npx * 4));
    pl.conf = f->conf.p;
  }
  MD_TRY(grow(m, st, f->cams, (size_t)B * 22 * 4));
  if (out.count) MD_TRY(grow(m, st, f->scratch, points_scratch_bytes(B, H, W)));
  PointsParams& p = pl.p = make_params(B, H, W, *c.o);
  p.capacity = out.capacity;
  pl.q = make_normals(c.nrm);
  pl.thin = voxel_on(c.vox) && out.count;  // without the list there is nothing to thin
  pl.filt = outlier_on(c.outl) && out.count;
  pl.pln = planes_on(c.pln);  // the count is there: infer_points refuses the stage without it
  pl.pcut = pl.pln && c.pln->mode != 0;
  if (pl.pln) pl.pn = make_planes(*c.pln);
  pl.clu = clusters_on(c.clu);
  pl.ccut = pl.clu && c.clu->mode != 0;
  if (pl.clu) pl.cn = make_clusters(*c.clu);
  pl.mat = match_on(c.mat);
  pl.mcut = pl.mat && c.mat->mode != 0;
  if (pl.mat) {
    pl.mn = make_match(*c.mat);
    if (c.mat->target_kind == MD_MEM_HOST && pl.mn.t > 0) {
      MD_TRY(grow(m, st, f->mtarget, (size_t)pl.mn.t * 12));
      pl.host_target = c.mat->target;
      pl.mn.target = f->mtarget.p;
    }
  }
  pl.reg = register_on(c.reg);
  if (pl.reg) {
    pl.rg = make_register(*c.reg, c.rpl);
    if (c.reg->target_kind == MD_MEM_HOST && pl.rg.t > 0) {
      MD_TRY(grow(m, st, f->rtarget, (size_t)pl.rg.t * 12));
      pl.host_reg_target = c.reg->target;
      pl.rg.target = f->rtarget.p;
      if (pl.rg.plane) {  // the normals are of the target's kind
        MD_TRY(grow(m, st, f->rnormals, (size_t)pl.rg.t * 12));
        pl.host_reg_normals = c.rpl->target_normals;
        pl.rg.target_normals = f->rnormals.p;
      }
    }
  }
  if (c.rnd) {
    pl.r = make_render(c.rnd->T, c.rnd->H, c.rnd->W, c.rnd->opts);
    MD_TRY(grow(m, st, f->rkeys, render_scratch_bytes(c.rnd->T, c.rnd->H, c.rnd->W)));
    if (c.in_kind == MD_MEM_HOST) MD_TRY(grow(m, st, f->rcams, (size_t)c.rnd->T * 22 * 4));
  }
  if (c.rst) {
    pl.s = make_raster(c.rst->T, c.rst->H, c.rst->W, c.rst->opts, c.rst->out);
    pl.queue = raster_queue_entries();
    MD_TRY(grow(m, st, f->skeys, raster_scratch_bytes(c.rst->T, c.rst->H, c.rst->W, pl.queue)));
    if (c.in_kind == MD_MEM_HOST) MD_TRY(grow(m, st, f->scams, (size_t)c.rst->T * 22 * 4));
  }
  pl.deci = decimate_on(c.dec);
  pl.comp = components_on(c.comp);
  pl.smo = smooth_on(c.smooth);
  pl.own_faces = pl.deci || pl.comp || pl.smo;
  pl.mesh = mesh_on(c.mesh) || pl.own_faces;
  if (pl.mesh) {
    // a corner is usable below the capacity of the list the faces name: the caller's, or with the decimation the model's own,
    // unthinned, of which every row is. Faces that a later stage reads: the map always has a home
    pl.g = make_mesh(B, H, W, stride, pl.deci ? rows : (long)out.capacity, *c.mesh);
    const size_t bytes = pl.own_faces ? mesh_scratch_bytes(B, H, W, stride) + align_up(pl.npx * 4, 256) : mesh_home_bytes(*c.mesh, B, H, W, stride);
    if (bytes) MD_TRY(grow(m, st, f->mesh, bytes));
  }
  if (const size_t total = place_outputs(c, pl, nullptr)) {
    MD_TRY(grow(m, st, f->out, total));
    place_outputs(c, pl, (char*)f->out.p);
  }
  if (pl.mesh) {  // the faces the call ends with: those of the kept components, the decimated ones, else the mesh stage's
    auto ends_with = [&](const int32_t* faces, const int32_t* count, int64_t capacity) {
      pl.faces = faces; pl.face_count = count; pl.face_capacity = (long)capacity;
    };
    if (pl.comp) ends_with(pl.k.faces_out, pl.k.face_count, c.comp->face_capacity);
    else if (pl.deci) ends_with(pl.d.faces_out, pl.d.face_count, c.dec->face_capacity);
    else ends_with(pl.g.faces, pl.g.face_count, c.mesh->face_capacity);
  }
  const bool own_list = pl.thin || pl.filt || pl.deci || pl.pcut || pl.mcut || pl.ccut;  // the scatter fills a list of the model's own: a later stage writes `fin`
  auto scatter_to = [&](const ListRows& l) { p.xyz = l.xyz; p.conf_out = l.conf; p.rgb_out = l.rgb; pl.q.normals = l.normals; p.count = l.count; };
  if (!own_list) scatter_to(pl.fin);
  if (pl.comp || pl.smo) {  // all faces of the call's list go to the model's face home; the stages read them and the list's device count
    MD_TRY(carve_faces(m, pl, B));
    if (pl.comp) {
      ComponentsParams& k = pl.k;
      MD_TRY(grow(m, st, f->ctable, components_scratch_bytes((int)rows, (int)nf, B)));
      k.v.in_count = pl.fin.count; k.v.n = (int)rows; k.v.B = B;
      k.faces = pl.gd.faces; k.in_face_count = pl.gd.face_count; k.nf = (int)nf;
      k.min_faces = c.comp->min_faces; k.face_capacity = (long)c.comp->face_capacity;
    }
    if (pl.smo) {  // the rows of the call's list below its capacity; the faces the rasteriser reads
      SmoothParams& sm = pl.sm;
      const md_points_smooth& o = *c.smooth;
      sm.xyz = pl.fin.xyz; sm.in_count = pl.fin.count; sm.B = B; sm.n = (int)std::min<long>((long)out.capacity, rows);
      sm.faces = pl.comp ? pl.k.faces_out : pl.gd.faces; sm.in_face_count = pl.comp ? pl.k.face_count : pl.gd.face_count;
      sm.nf = (int)(pl.comp ? std::min<long>((long)c.comp->face_capacity, nf) : nf);
      sm.step = o.step; sm.lambda = o.lambda; sm.mu = o.mu; sm.iterations = o.iterations; sm.pin_boundary = o.pin_boundary;
      sm.capacity = (long)out.capacity;
      MD_TRY(grow(m, st, f->stable, smooth_scratch_bytes(sm.n)));
    }
  }
  if (pl.pln) {
    PlanesParams& f = pl.pn;
    f.B = B; f.n = (int)(pl.pcut ? rows : std::min<long>((long)out.capacity, rows));
    MD_TRY(grow(m, st, m->points->ptable, planes_scratch_bytes(f.n, f.hypotheses)));
    if (!pl.pcut) reads(f, pl.fin);  // mode 0: the rows of the call's list below its capacity
  }
  if (pl.clu) {
    ClustersParams& k = pl.cn;
    k.B = B; k.n = (int)(pl.ccut ? rows : std::min<long>((long)out.capacity, rows));
    MD_TRY(grow(m, st, m->points->ktable, clusters_scratch_bytes(k.n, k.table_capacity)));
    if (!pl.ccut) reads(k, pl.fin);  // mode 0: the rows of the call's list below its capacity
  }
  if (pl.mat) {
    MatchParams& q = pl.mn;
    q.B = B; q.n = (int)(pl.mcut ? rows : std::min<long>((long)out.capacity, rows));
    MD_TRY(grow(m, st, m->points->mtable, match_scratch_bytes(q.n, q.t)));
    if (!pl.mcut) reads(q, pl.fin);  // mode 0: the rows of the call's list below its capacity
  }
  // The registration reads the list the matching reads: the call's list below its capacity, or, when the matching or the
  // clustering cuts, the model's own list in front of them, of which every row is usable. apply: the moved rows replace it.
  auto registers = [&](const ListRows& l, bool own) -> int {
    RegisterParams& q = pl.rg;
    q.B = B; q.n = (int)(own ? rows : std::min<long>((long)out.capacity, rows));
    q.xyz = l.xyz; q.normals = l.normals; q.in_count = l.count;
    if (c.reg->apply) {
      q.xyz_out = l.xyz;
      q.normals_out = l.normals;
    }
    return grow(m, st, m->points->rtable, q.plane ? register_plane_scratch_bytes(q.n, q.t) : register_scratch_bytes(q.n, q.t));
  };
  if (pl.reg && !(pl.mcut || pl.ccut)) MD_TRY(registers(pl.fin, false));
  if (!own_list) return MD_OK;
  const bool want_rgb = out.rgb != nullptr, want_nrm = c.nrm && c.nrm->normals;
  const size_t b_xyz = align_up((size_t)rows * 12, 256), b_conf = pl.dual ? align_up((size_t)rows * 4, 256) : 0;
  const size_t b_rgb = want_rgb ? align_up((size_t)rows * 3, 256) : 0, b_nrm = want_nrm ? b_xyz : 0;
  const size_t b_list = b_xyz + b_conf + b_rgb + b_nrm + align_up((size_t)(B + 1) * 4, 256);
  auto rows_of = [&](void* home) {  // the rank reads the confidence whether or not the caller takes it
    char* base = (char*)home;
    return ListRows{(float*)base, pl.dual ? (float*)(base + b_xyz) : nullptr, want_rgb ? (uint8_t*)(base + b_xyz + b_conf) : nullptr,
                    want_nrm ? (float*)(base + b_xyz + b_conf + b_rgb) : nullptr, (int32_t*)(base + b_xyz + b_conf + b_rgb + b_nrm)};
  };
  MD_TRY(grow(m, st, f->vlist, b_list));
  if (pl.thin) MD_TRY(grow(m, st, f->vtable, voxel_scratch_bytes((int)rows)));
  if (pl.filt) MD_TRY(grow(m, st, f->otable, outlier_scratch_bytes((int)rows)));
  if (pl.filt && (pl.thin || pl.pcut || pl.mcut || pl.ccut)) MD_TRY(grow(m, st, f->flist, b_list));
  if (pl.thin && (pl.pcut || pl.mcut || pl.ccut)) MD_TRY(grow(m, st, f->plist, b_list));
  if (pl.pcut && (pl.mcut || pl.ccut)) MD_TRY(grow(m, st, f->klist, b_list));
  if (pl.mcut && pl.ccut) MD_TRY(grow(m, st, f->mlist, b_list));
  // The chain scatter -> outlier removal -> voxel thinning -> plane extraction (mode 1 / 2) -> matching (mode 1 / 2) -> clustering (mode 1), or scatter -> decimation (the decimation is the thinning, with the
  // faces of the model's face home): every stage but the last writes a list of the model's own, of which every row is usable;
  // the last one writes `fin` below the caller's capacity. Nothing else knows which stage that is.
  ListRows l = rows_of(f->vlist.p);
  scatter_to(l);
  p.capacity = rows;
  if (pl.filt) {
    OutlierParams& u = pl.u;
    reads(u, l);
    const bool last = !pl.thin && !pl.pcut && !pl.mcut && !pl.ccut;
    if (!last) l = rows_of(f->flist.p);
    writes(u, last ? pl.fin : l);
    u.n = (int)rows; u.B = B; u.radius = c.outl->radius; u.k = c.outl->min_neighbours; u.capacity = last ? (long)out.capacity : rows;
  }
  if (pl.thin) {
    VoxelParams& v = pl.v;
    reads(v, l);
    const bool last = !pl.pcut && !pl.mcut && !pl.ccut;
    if (!last) l = rows_of(f->plist.p);
    writes(v, last ? pl.fin : l);
    v.n = (int)rows; v.B = B; v.voxel = c.vox->voxel; v.capacity = last ? (long)out.capacity : rows;
  }
  if (pl.pcut) {
    reads(pl.pn, l);
    const bool last = !pl.mcut && !pl.ccut;
    if (!last) l = rows_of(f->klist.p);
    writes(pl.pn, last ? pl.fin : l);
    pl.pn.capacity = last ? (long)out.capacity : rows;
  }
  if (pl.reg && (pl.mcut || pl.ccut)) MD_TRY(registers(l, true));
  if (pl.mcut) {
    reads(pl.mn, l);
    if (pl.ccut) l = rows_of(f->mlist.p);
    writes(pl.mn, pl.ccut ? l : pl.fin);
    pl.mn.capacity = pl.ccut ? rows : (long)out.capacity;
  }
  if (pl.ccut) {
    reads(pl.cn, l);
    writes(pl.cn, pl.fin);
    pl.cn.capacity = (long)out.capacity;
  }
  if (pl.deci) {
    DecimateParams& d = pl.d;
    MD_TRY(carve_faces(m, pl, B));
    MD_TRY(grow(m, st, f->dtable, decimate_scratch_bytes((int)rows, (int)nf, B)));
    reads(d.v, l);
    writes(d.v, pl.fin);
    d.v.n = (int)rows; d.v.B = B; d.v.voxel = c.dec->voxel; d.v.capacity = out.capacity;
    d.faces = pl.gd.faces; d.in_face_count = pl.gd.face_count; d.nf = (int)nf; d.face_capacity = (long)c.dec->face_capacity;
  }
  return MD_OK;
}

// The image, rgb and cameras on the device: the caller's pointers, or copies of host ones.
int stage_inputs(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  md_model_s::PointsState* f = m->points;
  PointsParams& p = pl.p;
  pl.x = c.nchw;
  p.rgb = c.rgb; p.K = c.cam->intrinsics; p.E = c.cam->extrinsics; p.focal = c.cam->focal_px;
  if (c.rnd) {
    const md_points_cameras& t = c.rnd->cam;
    pl.r.K = t.intrinsics; pl.r.focal = t.intrinsics ? nullptr : t.focal_px; pl.r.E = t.extrinsics;
  }
  if (c.rst) {
    const md_points_cameras& t = c.rst->cam;
    pl.s.K = t.intrinsics; pl.s.focal = t.intrinsics ? nullptr : t.focal_px; pl.s.E = t.extrinsics;
  }
  if (pl.host_reg_target)
    MD_HIP(hipMemcpyAsync(f->rtarget.p, pl.host_reg_target, (size_t)pl.rg.t * 12, hipMemcpyHostToDevice, pl.st));
  if (pl.host_reg_normals)
    MD_HIP(hipMemcpyAsync(f->rnormals.p, pl.host_reg_normals, (size_t)pl.rg.t * 12, hipMemcpyHostToDevice, pl.st));
  if (pl.host_target)  // the target has a kind of its own
    MD_HIP(hipMemcpyAsync(f->mtarget.p, pl.host_target, (size_t)pl.mn.t * 12, hipMemcpyHostToDevice, pl.st));
  if (c.in_kind != MD_MEM_HOST) return MD_OK;
  MD_TRY(grow(m, pl.st, f->x, pl.npx * 3 * 4));
  if (c.rgb) MD_TRY(grow(m, pl.st, f->rgb, pl.npx * 3));
  auto h2d = [&](auto*& src, auto* home, size_t bytes) -> int {  // a host input, where given, moves to its device home
    if (!src) return MD_OK;
    MD_HIP(hipMemcpyAsync(home, src, bytes, hipMemcpyHostToDevice, pl.st));
    src = home;
    return MD_OK;
  };
  MD_TRY(h2d(pl.x, f->x.p, pl.npx * 3 * 4));
  MD_TRY(h2d(p.rgb, f->rgb.p, pl.npx * 3));
  MD_TRY(h2d(p.K, f->k_home(), (size_t)c.B * 36));
  MD_TRY(h2d(p.E, f->e_home(c.B), (size_t)c.B * 48));
  MD_TRY(h2d(p.focal, f->f_home(c.B), (size_t)c.B * 4));
  if (c.rnd) {
    const size_t T = (size_t)c.rnd->T;
    MD_TRY(h2d(pl.r.K, f->rcams.p, T * 36));
    MD_TRY(h2d(pl.r.E, f->rcams.p + T * 9, T * 48));
    MD_TRY(h2d(pl.r.focal, f->rcams.p + T * 21, T * 4));
  }
  if (c.rst) {
    const size_t T = (size_t)c.rst->T;
    MD_TRY(h2d(pl.s.K, f->scams.p, T * 36));
    MD_TRY(h2d(pl.s.E, f->scams.p + T * 9, T * 48));
    MD_TRY(h2d(pl.s.focal, f->scams.p + T * 21, T * 4));
  }
  return MD_OK;
}

// The model: its cameras land in the homes of those the caller did not give.
int run_model(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  md_model_s::PointsState* f = m->points;
  PointsParams& p = pl.p;
  const bool need_k = !p.K && !p.focal, need_e = (c.o->world || views_on(c)) && !p.E;
  if (m->kind == 1) {
    Da3Outputs d;
    d.depth = pl.raw;
    d.depth_confidence = pl.conf;
    if (pl.dual && need_k) p.K = d.intrinsics = f->k_home();
    if (pl.dual && need_e) p.E = d.extrinsics = f->e_home(c.B);
    return da3_infer_ex_direct(m, pl.x, c.B, c.H, c.W, d, pl.st);
  }
  if (c.cam->focal_px) return model_infer_direct(m, pl.x, c.B, c.H, c.W, pl.raw, nullptr, nullptr, pl.st, p.focal);
  if (need_k) p.focal = f->f_home(c.B);
  return model_infer_direct(m, pl.x, c.B, c.H, c.W, pl.raw, need_k ? f->f_home(c.B) : nullptr, nullptr, pl.st);
}

// View filter: raw -> depth, rejected pixels 0.
int run_filter(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  const PointsParams& p = pl.p;
  ViewFilterParams v = make_filter_params(c.B, c.H, c.W, *c.fo);
  v.depth = pl.raw; v.conf = pl.conf;
  v.K = p.K; v.focal = p.K ? nullptr : p.focal; v.E = views_on(c) ? p.E : nullptr;
  v.depth_out = pl.depth;
  return launch_view_filter(v, m->points->filter.p, pl.st);
}

int run_unproject(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  PointsParams& p = pl.p;
  p.depth = pl.depth; p.conf = pl.conf;
  if (p.K) p.focal = nullptr;
  if (!c.o->world) p.E = nullptr;
  return launch_unproject(p, m->points->scratch.p, pl.st, &pl.q);
}

// The mesh of the list: needs the scratch of run_unproject's launches before anything reuses it.
int run_mesh(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  pl.g.depth = pl.depth;
  if (pl.own_faces) {  // the map, then the model's own faces, complete, for the decimation / the components / the smoothing; the
                       // caller's, if it takes them, are a copy: both have the same rows of the list as usable corners, so
                       // they are the same faces
    void* home = m->points->mesh.p;
    int32_t* pix = pl.pix ? pl.pix : (int32_t*)((char*)home + mesh_scratch_bytes(c.B, c.H, c.W, c.o->stride));
    MD_TRY(launch_mesh_index(c.B, c.H, c.W, m->points->scratch.p, pix, pl.st));
    pl.gd.depth = pl.depth; pl.gd.pixel_index = pix;
    MD_TRY(launch_mesh_grid(pl.gd, home, pl.st));
    return launch_copy_faces(pl.gd.faces, pl.gd.face_count, c.B, pl.gd.face_capacity, pl.g.faces, pl.g.face_count, pl.g.face_capacity, pl.st);
  }
  return launch_mesh(pl.g, pl.pix, m->points->scratch.p, m->points->mesh.p, pl.st);
}

// Outlier removal: the model's own list -> the list outputs of the call, or the list the thinning reads.
int run_outlier(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_radius_outliers(pl.u, m->points->otable.p, pl.st));
  m->points->outl_rows = pl.u.n;  // only a launched run has flags to read (points_outlier_overflow)
  return MD_OK;
}

// Voxel thinning: the model's own list -> the list outputs of the call.
int run_thin(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_voxel_thin(pl.v, m->points->vtable.p, pl.st));
  m->points->vox_rows = pl.v.n;  // only a launched run has flags to read (points_voxel_overflow)
  return MD_OK;
}

// Decimation: the model's own list and faces -> the list outputs of the call and dec's face outputs.
int run_decimate(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_decimate_mesh(pl.d, m->points->dtable.p, pl.st));
  m->points->dec_rows = pl.d.v.n; m->points->dec_faces = pl.d.nf; m->points->dec_views = pl.d.v.B;  // points_decimate_overflow
  return MD_OK;
}

// Island removal: the faces the mesh stage left in the model's home -> comp's outputs. The list is not touched.
int run_components(md_model_s* m, const PointsCall&, PointsPlan& pl) { return launch_mesh_components(pl.k, m->points->ctable.p, pl.st); }

// Smoothing: the list of the call and the faces the rasteriser reads -> smooth's outputs. The list is not touched.
int run_smooth(md_model_s* m, const PointsCall&, PointsPlan& pl) { return launch_smooth_mesh(pl.sm, m->points->stable.p, pl.st); }

// Plane extraction: the list of the call -> pln's outputs; with mode 1 / 2 the model's own list -> the list outputs of the call.
int run_planes(md_model_s* m, const PointsCall&, PointsPlan& pl) { return launch_fit_planes(pl.pn, m->points->ptable.p, pl.st); }

// Clustering: the list of the call -> clu's outputs; with mode 1 the model's own list -> the list outputs of the call.
int run_clusters(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_cluster_points(pl.cn, m->points->ktable.p, pl.st));
  m->points->clu_rows = pl.cn.n; m->points->clu_table = pl.cn.table_capacity;  // only a launched run has flags to read (points_clusters_overflow)
  return MD_OK;
}

// Matching: the list of the call -> mat's outputs; with mode 1 / 2 the model's own list -> the list outputs of the call, or the
// list the clustering reads.
int run_match(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_match_points(pl.mn, m->points->mtable.p, pl.st));
  m->points->mat_rows = pl.mn.n; m->points->mat_target = pl.mn.t; m->points->mat_ran = true;  // only a launched run has flags to read (points_match_overflow)
  return MD_OK;
}

// Registration: the list the matching reads -> reg's outputs; with apply the moved rows replace that list's in place.
int run_register(md_model_s* m, const PointsCall&, PointsPlan& pl) {
  MD_TRY(launch_register_points(pl.rg, m->points->rtable.p, pl.st));
  m->points->reg_rows = pl.rg.n; m->points->reg_target = pl.rg.t; m->points->reg_plane = pl.rg.plane; m->points->reg_ran = true;  // only a launched run has flags to read (points_register_overflow)
  return MD_OK;
}

// Rendering: the list the call ends with and its device count -> the target images.
int run_render(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  RenderParams& r = pl.r;
  r.xyz = pl.fin.xyz; r.rgb = pl.fin.rgb; r.count = pl.fin.count + c.B;
  r.n = (int)std::min<long>((long)c.out->capacity, pl.rows);
  return launch_render_points(r, m->points->rkeys.p, pl.st);
}

// Rasterising: the list the call ends with as vertices (smoothed: the smoothed rows of the same list), the faces it ends with
// and their device count -> the target images. The rows beyond min(count[B], capacity) are never named: neither the mesh stage
// nor the decimation emits a face with a corner at or above `capacity`.
int run_raster(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  RasterParams& s = pl.s;
  s.xyz = pl.smo ? pl.sm.xyz_out : pl.fin.xyz; s.rgb = pl.fin.rgb;
  s.n = (int)std::min<long>((long)c.out->capacity, pl.rows);
  s.faces = pl.faces; s.count = pl.face_count + c.B;
  s.nf = (int)std::min<long>(pl.face_capacity, 2 * pl.rows);
  return launch_render_mesh(s, m->points->skeys.p, pl.queue, pl.st);
}

// Host outputs, complete when the call returns: the depth, the dense maps and the counts first, then, once `count` is known,
// only the live rows of each list output: the caller's memory beyond them stays as it was.
int copy_outputs(md_model_s* m, const PointsCall& c, PointsPlan& pl) {
  if (c.out_kind != MD_MEM_HOST) return MD_OK;
  auto d2h = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst && bytes) MD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, pl.st));
    return MD_OK;
  };
  MD_TRY(d2h(c.out->depth, pl.depth, pl.npx * 4));
  for (const OutSlot& s : pl.slots)
    if (!s.live) MD_TRY(d2h(s.caller, s.home, s.rows * s.row_bytes));
  int32_t overflow = 0, outl_overflow = 0, dec_overflow[2] = {0, 0}, clu_overflow = 0, mat_overflow = 0, reg_overflow = 0;
  if (pl.deci) MD_TRY(d2h(&dec_overflow[0], voxel_flags(m->points->dtable.p, pl.d.v.n), 4));
  if (pl.deci) MD_TRY(d2h(&dec_overflow[1], decimate_flags(m->points->dtable.p, pl.d.v.n, pl.d.nf, pl.d.v.B), 4));
  if (pl.thin) MD_TRY(d2h(&overflow, voxel_flags(m->points->vtable.p, pl.v.n), 4));
  if (pl.filt) MD_TRY(d2h(&outl_overflow, outlier_flags(m->points->otable.p, pl.u.n), 4));
  if (pl.filt) MD_TRY(d2h(&pl.unfiltered, pl.u.in_count + c.B, 4));
  if (pl.pcut) MD_TRY(d2h(&pl.plane_rows, pl.pn.in_count + c.B, 4));
  if (pl.clu) {
    const int32_t* flags = clusters_flags(m->points->ktable.p, pl.cn.n, pl.cn.table_capacity);
    MD_TRY(d2h(&clu_overflow, flags, 4));
    MD_TRY(d2h(&pl.clusters_kept, (pl.cn.stats ? pl.cn.stats : flags + kClusterStatsFlag) + 1, 4));
    if (pl.ccut) MD_TRY(d2h(&pl.cluster_rows, pl.cn.in_count + c.B, 4));
  }
  if (pl.reg) {
    MD_TRY(d2h(&reg_overflow, pl.rg.plane ? register_plane_flags(m->points->rtable.p, pl.rg.n, pl.rg.t) : register_flags(m->points->rtable.p, pl.rg.n, pl.rg.t), 4));
    if (pl.mcut || pl.ccut) MD_TRY(d2h(&pl.register_rows, pl.rg.in_count + c.B, 4));
  }
  if (pl.mat) {
    MD_TRY(d2h(&mat_overflow, match_flags(m->points->mtable.p, pl.mn.n, pl.mn.t), 4));
    if (pl.mcut) MD_TRY(d2h(&pl.match_rows, pl.mn.in_count + c.B, 4));
  }
  MD_HIP(hipStreamSynchronize(pl.st));
  if (reg_overflow) MD_FAIL(MD_ERR_HIP, "%s", kRegisterRanOut);
  if (mat_overflow) MD_FAIL(MD_ERR_HIP, "%s", kMatchRanOut);
  if (clu_overflow) MD_FAIL(MD_ERR_HIP, "%s", kClustersRanOut);
  if (dec_overflow[0] || dec_overflow[1]) MD_FAIL(MD_ERR_HIP, "%s", kDecimateRanOut);
  if (outl_overflow) MD_FAIL(MD_ERR_HIP, "%s", kOutlierRanOut);
  if (overflow) MD_FAIL(MD_ERR_HIP, "%s", kVoxelRanOut);
  if (!c.out->count) return MD_OK;  // no list: nothing has live rows
  for (const OutSlot& s : pl.slots)
    if (s.live) MD_TRY(d2h(s.caller, s.home, std::min((size_t)std::max(*s.live, 0), s.rows) * s.row_bytes));
  MD_HIP(hipStreamSynchronize(pl.st));
  return MD_OK;
}

// The stages in the order a captured graph bakes: every grow of the device path before anything is enqueued, then the work.
int points_eager(md_model_s* m, const PointsCall& c, bool dual, long rows, hipStream_t st) {
  if (!m->points) m->points = new md_model_s::PointsState();
  PointsPlan pl;
  pl.st = st; pl.dual = dual; pl.npx = (size_t)c.B * c.H * c.W; pl.rows = rows;
  auto timed = [&](const char* name, int (*stage)(md_model_s*, const PointsCall&, PointsPlan&)) -> int {
    Run r{m, st, c.B};
    r.begin(name);
    MD_TRY(stage(m, c, pl));
    r.end();
    return MD_OK;
  };
  MD_TRY(plan_homes(m, c, pl));
  MD_TRY(stage_inputs(m, c, pl));
  MD_TRY(run_model(m, c, pl));
  if (c.fo) MD_TRY(timed("points_view_filter", run_filter));
  MD_TRY(timed("points_unproject", run_unproject));
  if (pl.mesh) MD_TRY(timed("points_mesh", run_mesh));
  if (pl.filt) MD_TRY(timed("points_outlier", run_outlier));
  if (pl.thin) MD_TRY(timed("points_voxel", run_thin));
  if (pl.deci) MD_TRY(timed("points_decimate", run_decimate));
  if (pl.comp) MD_TRY(timed("points_components", run_components));
  if (pl.smo) MD_TRY(timed("points_smooth", run_smooth));
  if (pl.pln) MD_TRY(timed("points_planes", run_planes));
  if (pl.reg) MD_TRY(timed("points_register", run_register));
  if (pl.mat) MD_TRY(timed("points_match", run_match));
  if (pl.clu) MD_TRY(timed("points_clusters", run_clusters));
  if (c.rnd) MD_TRY(timed("points_render", run_render));
  if (c.rst) MD_TRY(timed("points_raster", run_raster));
  return copy_outputs(m, c, pl);
}

// The graph replay key of a call: stream, shape, every option, every in / out pointer and the commit generation
// (md_frame.hip). A part that is off adds nothing: the key, and the graph, of the call without it. c.cam is not null.
std::vector<uintptr_t> points_graph_key(md_model_t m, const PointsCall& c, hipStream_t st) {
  const md_points_cameras& cam = *c.cam;
  const md_points_opts* o = c.o;
  const md_points_outputs* out = c.out;
  std::vector<uintptr_t> key;
  key_add(key, 0x504f494eu, st, c.B, c.H, c.W, c.nchw, c.rgb, cam.intrinsics, cam.extrinsics, cam.focal_px);
  key_add(key, o->pixel_offset, o->depth_min, o->depth_max, o->conf_min, o->edge_rtol, o->stride, o->world ? 1 : 0);
  key_add(key, out->point_map, out->mask, out->xyz, out->rgb, out->conf, out->count, out->capacity, out->depth, model_root(m)->commit_gen);
  if (c.fo) key_add(key, 0x56464c54u, c.fo->conf_percentile, c.fo->view_rtol, c.fo->min_views);
  if (c.nrm && (c.nrm->normal_map || c.nrm->normals || c.nrm->min_cos > 0.f))  // all zero: the call without normals
    key_add(key, 0x4e524d4cu, c.nrm->normal_map, c.nrm->normals, c.nrm->min_cos);
  if (voxel_on(c.vox)) key_add(key, 0x564f584cu, c.vox->voxel, c.vox->index, c.vox->weight, c.vox->dropped);
  if (outlier_on(c.outl)) key_add(key, 0x4f55544cu, c.outl->radius, c.outl->min_neighbours, c.outl->neighbours, c.outl->index, c.outl->dropped);
  if (c.rnd) {
    const md_points_render& r = *c.rnd;
    key_add(key, 0x524e4452u, r.T, r.H, r.W, r.cam.intrinsics, r.cam.extrinsics, r.cam.focal_px);
    key_add(key, r.opts.pixel_offset, r.opts.z_near, r.opts.z_far, r.opts.radius, r.out.depth, r.out.index, r.out.rgb, r.out.filled);
  }
  // the three stages behind the mesh each add its max_rtol: a mesh request without outputs still sets the edge test
  if (decimate_on(c.dec)) {
    const md_points_decimate& d = *c.dec;
    key_add(key, 0x44454349u, d.voxel, d.index, d.weight, d.dropped, d.remap, d.faces, d.face_index, d.face_count, d.face_capacity, d.faces_dropped);
    key_add(key, c.mesh->max_rtol);
  }
  if (components_on(c.comp)) {
    const md_points_components& k = *c.comp;
    key_add(key, 0x434f4d50u, k.min_faces, k.label, k.component_faces, k.faces, k.face_index, k.face_count, k.face_capacity, k.stats);
    key_add(key, c.mesh->max_rtol);
  }
  if (smooth_on(c.smooth)) {
    const md_points_smooth& q = *c.smooth;
    key_add(key, 0x534d5448u, q.step, q.lambda, q.mu, q.iterations, q.pin_boundary, q.xyz, q.normals, q.stats);
    key_add(key, c.mesh->max_rtol);
  }
  if (planes_on(c.pln)) {
    const md_points_planes& f = *c.pln;
    key_add(key, 0x504c414eu, f.planes, f.hypotheses, f.tol, f.min_inliers, f.seed, f.normal_min_cos, f.axis[0], f.axis[1], f.axis[2], f.axis_min_cos, f.mode);
    key_add(key, f.plane, f.plane_count, f.hypothesis, f.label, f.index, f.dropped);
  }
  if (clusters_on(c.clu)) {
    const md_points_clusters& k = *c.clu;
    key_add(key, 0x434c5553u, k.radius, k.min_neighbours, k.min_points, k.max_points, k.mode, k.table_capacity);
    key_add(key, k.label, k.cluster_size, k.cluster, k.table_label, k.table_size, k.box, k.stats, k.index, k.dropped);
  }
  if (match_on(c.mat)) {
    const md_points_match& q = *c.mat;
    key_add(key, 0x4d415443u, q.radius, q.target, q.target_rows, q.target_kind, q.mode, q.tol[0], q.tol[1], q.tol[2], q.tol[3]);
    key_add(key, q.nearest, q.dist2, q.stats, q.index, q.dropped);
  }
  if (register_on(c.reg)) {
    const md_points_register& q = *c.reg;
    key_add(key, 0x52454753u, q.radius, q.target, q.target_rows, q.target_kind, q.iterations, q.min_pairs, q.apply, q.rot_eps, q.trans_eps);
    key_add(key, q.init != nullptr, q.transform, q.pairs, q.sum_d2, q.stats, q.dropped, q.nearest, q.dist2);
    if (q.init)
      for (int i = 0; i < 12; ++i) key_add(key, q.init[i]);  // init travels by value: its values are part of the captured launches
    if (register_plane_on(c.rpl)) key_add(key, 0x5245474eu, c.rpl->target_normals, c.rpl->sum_r2);
  }
  if (mesh_on(c.mesh))  // every output null: the call without a mesh
    key_add(key, 0x4d455348u, c.mesh->max_rtol, c.mesh->faces, c.mesh->face_count, c.mesh->face_capacity, c.mesh->pixel_index);
  if (c.rst) {
    const md_points_raster& r = *c.rst;
    key_add(key, 0x52415354u, r.T, r.H, r.W, r.cam.intrinsics, r.cam.extrinsics, r.cam.focal_px, raster_queue_entries());
    key_add(key, r.opts.pixel_offset, r.opts.z_near, r.opts.z_far, r.opts.cull, r.opts.max_extent);
    key_add(key, r.out.depth, r.out.face, r.out.rgb, r.out.filled, r.out.skipped);
  }
  return key;
}

}  // namespace

int infer_points(md_model_t m, const PointsCall& call, hipStream_t stream) {
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  if (!call.nchw) MD_FAIL(MD_ERR_INVALID_ARG, "input pointer is null");
  if ((call.in_kind != MD_MEM_HOST && call.in_kind != MD_MEM_DEVICE) || (call.out_kind != MD_MEM_HOST && call.out_kind != MD_MEM_DEVICE))
    MD_FAIL(MD_ERR_INVALID_ARG, "unknown memory kind");
  const md_points_cameras none = {nullptr, nullptr, nullptr};
  PointsCall c = call;  // the stages read the cameras without a null test
  if (!c.cam) c.cam = &none;
  const md_points_cameras& cam = *c.cam;
  const md_points_opts* o = c.o;
  const md_points_outputs* out = c.out;
  const int B = c.B, H = c.H, W = c.W;
  const bool dual = m->kind == 1 && da3_cfg(m).dual_head;
  const bool own_cams = m->kind == 0 || dual;  // Depth Pro predicts a focal length, the dual head's camera decoder K and E
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "point options are null");
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "point outputs are null");
  if (c.need_filter && !c.fo) MD_FAIL(MD_ERR_INVALID_ARG, "view filter options are null");
  if (!own_cams && !cam.intrinsics && !cam.focal_px)
    MD_FAIL(MD_ERR_UNSUPPORTED, "this Depth-Anything-v3 variant has no camera decoder: intrinsics or a focal length are required");
  const Sources s{c.rgb != nullptr, dual, cam.intrinsics != nullptr || dual, cam.focal_px != nullptr || m->kind == 0, cam.extrinsics != nullptr || dual};
  MD_TRY(check_points(o, out, c.nrm, s));
  MD_TRY(check_shape(B, H, W));
  const long rows = list_rows(B, H, W, o->stride);  // the stride is check_points'
  MD_TRY(check_voxel(c.vox, out, false));
  if (voxel_on(c.vox) && rows >= (1l << 30))
    MD_FAIL(MD_ERR_SHAPE, "voxel thinning takes fewer than 2^30 rows, the list may have %ld", rows);
  MD_TRY(check_decimate(c.dec, out, false));
  if (decimate_on(c.dec)) {
    if (!c.mesh) MD_FAIL(MD_ERR_INVALID_ARG, "decimation needs a mesh request");
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "decimation needs the list's `count`");
    if (voxel_on(c.vox)) MD_FAIL(MD_ERR_INVALID_ARG, "decimation together with voxel thinning: two grids; the decimation is the thinning");
    if (outlier_on(c.outl)) MD_FAIL(MD_ERR_INVALID_ARG, "decimation together with outlier removal: the rows the faces name no longer exist");
    if (2 * rows >= (1l << 30))
      MD_FAIL(MD_ERR_SHAPE, "decimation takes fewer than 2^30 faces, the mesh may have %ld", 2 * rows);
  }
  MD_TRY(check_components_part(c.comp));
  if (components_on(c.comp)) {
    if (!c.mesh) MD_FAIL(MD_ERR_INVALID_ARG, "components need a mesh request");
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "components need the list's `count`");
    if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "components together with decimation: the components of the decimated mesh are not built");
    if (voxel_on(c.vox) || outlier_on(c.outl))
      MD_FAIL(MD_ERR_INVALID_ARG, "components together with voxel thinning or outlier removal: the rows the faces name no longer exist");
    if (2 * rows >= (1l << 30))
      MD_FAIL(MD_ERR_SHAPE, "components take fewer than 2^30 faces, the mesh may have %ld", 2 * rows);
  }
  MD_TRY(check_smooth_part(c.smooth));
  if (smooth_on(c.smooth)) {
    if (!c.mesh) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing needs a mesh request");
    if (!out->count || !out->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing needs the list outputs `xyz` and `count`");
    if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing together with decimation: md_op_smooth_mesh serves the decimated mesh");
    if (voxel_on(c.vox) || outlier_on(c.outl))
      MD_FAIL(MD_ERR_INVALID_ARG, "smoothing together with voxel thinning or outlier removal: the rows the faces name no longer exist");
    if (components_on(c.comp) && (!c.comp->faces || !c.comp->face_count))
      MD_FAIL(MD_ERR_INVALID_ARG, "smoothing behind the components needs their outputs `faces` and `face_count`");
    if (c.rst && !c.smooth->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "rasterising the smoothed mesh needs the smoothing output `xyz`");
    if (2 * rows >= (1l << 30))
      MD_FAIL(MD_ERR_SHAPE, "smoothing takes fewer than 2^30 faces, the mesh may have %ld", 2 * rows);
  }
  MD_TRY(check_planes(c.pln, out, c.nrm && c.nrm->normals, false));
  if (planes_on(c.pln)) {
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction needs the list's `count`");
    if (c.pln->mode != 0) {
      if (mesh_on(c.mesh) || decimate_on(c.dec) || components_on(c.comp) || smooth_on(c.smooth))
        MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction with mode 1 / 2 together with a mesh stage: the rows the faces name would vanish");
      if ((voxel_on(c.vox) && (c.vox->index || c.vox->weight)) || (outlier_on(c.outl) && c.outl->index))
        MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction with mode 1 / 2 together with index / weight of an earlier stage: the rows they are parallel to are not returned");
    } else {
      if (!out->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction with mode 0 needs the list output `xyz`");
      if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction together with decimation: the rows are renumbered; md_op_fit_planes serves the decimated list");
    }
    if (rows >= (1l << 30)) MD_FAIL(MD_ERR_SHAPE, "plane extraction takes fewer than 2^30 rows, the list may have %ld", rows);
  }
  MD_TRY(check_clusters(c.clu, out, false));
  if (clusters_on(c.clu)) {
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "clustering needs the list's `count`");
    if (c.clu->mode != 0) {
      if (mesh_on(c.mesh) || decimate_on(c.dec) || components_on(c.comp) || smooth_on(c.smooth))
        MD_FAIL(MD_ERR_INVALID_ARG, "clustering with mode 1 together with a mesh stage: the rows the faces name would vanish");
      if ((voxel_on(c.vox) && (c.vox->index || c.vox->weight)) || (outlier_on(c.outl) && c.outl->index) || (planes_on(c.pln) && c.pln->index) ||
          (match_on(c.mat) && c.mat->index))
        MD_FAIL(MD_ERR_INVALID_ARG, "clustering with mode 1 together with index / weight of an earlier stage: the rows they are parallel to are not returned");
      if (planes_on(c.pln) && c.pln->mode == 0)
        MD_FAIL(MD_ERR_INVALID_ARG, "clustering with mode 1 behind plane extraction with mode 0: the rows its label is parallel to are not returned");
      if (match_on(c.mat) && c.mat->mode == 0)
        MD_FAIL(MD_ERR_INVALID_ARG, "clustering with mode 1 behind matching with mode 0: the rows `nearest` is parallel to are not returned");
    } else {
      if (!out->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "clustering with mode 0 needs the list output `xyz`");
      if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "clustering together with decimation: the rows are renumbered; md_op_cluster_points serves the decimated list");
    }
    if (rows >= (1l << 30)) MD_FAIL(MD_ERR_SHAPE, "clustering takes fewer than 2^30 rows, the list may have %ld", rows);
  }
  MD_TRY(check_match(c.mat, out, false));
  if (match_on(c.mat)) {
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "matching needs the list's `count`");
    if (c.mat->mode != 0) {
      if (mesh_on(c.mesh) || decimate_on(c.dec) || components_on(c.comp) || smooth_on(c.smooth))
        MD_FAIL(MD_ERR_INVALID_ARG, "matching with mode 1 / 2 together with a mesh stage: the rows the faces name would vanish");
      if ((voxel_on(c.vox) && (c.vox->index || c.vox->weight)) || (outlier_on(c.outl) && c.outl->index) || (planes_on(c.pln) && c.pln->index))
        MD_FAIL(MD_ERR_INVALID_ARG, "matching with mode 1 / 2 together with index / weight of an earlier stage: the rows they are parallel to are not returned");
      if (planes_on(c.pln) && c.pln->mode == 0)
        MD_FAIL(MD_ERR_INVALID_ARG, "matching with mode 1 / 2 behind plane extraction with mode 0: the rows its label is parallel to are not returned");
    } else {
      if (!out->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "matching with mode 0 needs the list output `xyz`");
      if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "matching together with decimation: the rows are renumbered; md_op_match_points serves the decimated list");
    }
    if (rows >= (1l << 30)) MD_FAIL(MD_ERR_SHAPE, "matching takes fewer than 2^30 rows, the list may have %ld", rows);
  }
  MD_TRY(check_register(c.reg, false));
  MD_TRY(check_register_plane(c.reg, c.rpl));
  if (register_on(c.reg)) {
    if (!out->count) MD_FAIL(MD_ERR_INVALID_ARG, "registration needs the list's `count`");
    if (!out->xyz) MD_FAIL(MD_ERR_INVALID_ARG, "registration needs the list output `xyz`");
    if (decimate_on(c.dec)) MD_FAIL(MD_ERR_INVALID_ARG, "registration together with decimation: the rows are renumbered; md_op_register_points serves the decimated list");
    if (c.reg->apply && (mesh_on(c.mesh) || components_on(c.comp) || smooth_on(c.smooth)))
      MD_FAIL(MD_ERR_INVALID_ARG, "registration with apply together with a mesh stage: its faces and smoothed rows belong to the rows before they moved");
    if (rows >= (1l << 30)) MD_FAIL(MD_ERR_SHAPE, "registration takes fewer than 2^30 rows, the list may have %ld", rows);
  }
  MD_TRY(check_mesh(c.mesh, out->count != nullptr, voxel_on(c.vox), B, H, W));
  MD_TRY(check_outlier(c.outl, out, false));
  if (outlier_on(c.outl)) {
    if (mesh_on(c.mesh)) MD_FAIL(MD_ERR_INVALID_ARG, "a mesh together with outlier removal: the rows its faces name no longer exist");
    if (c.outl->index && voxel_on(c.vox))
      MD_FAIL(MD_ERR_INVALID_ARG, "the outlier removal's index together with voxel thinning: the rows it is parallel to are not returned");
    if (rows >= (1l << 30))
      MD_FAIL(MD_ERR_SHAPE, "outlier removal takes fewer than 2^30 rows, the list may have %ld", rows);
  }
  if (c.rnd) {
    MD_TRY(check_render(c.rnd->T, c.rnd->H, c.rnd->W, &c.rnd->cam, &c.rnd->opts, &c.rnd->out, out->rgb != nullptr));
    if (!out->xyz || !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "rendering needs the list outputs `xyz` and `count`");
  }
  if (c.rst) {
    MD_TRY(check_raster(c.rst->T, c.rst->H, c.rst->W, &c.rst->cam, &c.rst->opts, &c.rst->out, out->rgb != nullptr));
    if (!out->xyz || !out->count) MD_FAIL(MD_ERR_INVALID_ARG, "rasterising needs the list outputs `xyz` and `count`");
    if (decimate_on(c.dec)) {
      if (!c.dec->faces || !c.dec->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "rasterising needs the decimation outputs `faces` and `face_count`");
    } else if (components_on(c.comp)) {
      if (!c.comp->faces || !c.comp->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "rasterising needs the component outputs `faces` and `face_count`");
    } else if (!c.mesh || !c.mesh->faces || !c.mesh->face_count) MD_FAIL(MD_ERR_INVALID_ARG, "rasterising needs the mesh outputs `faces` and `face_count`");
  }
  if (c.fo) {
    MD_TRY(check_filter(c.fo, s, B, H, W));
    if (fbits(c.fo->pixel_offset) != fbits(o->pixel_offset) || depth_min_of(c.fo->depth_min) != depth_min_of(o->depth_min) ||
        depth_max_of(c.fo->depth_max) != depth_max_of(o->depth_max))
      MD_FAIL(MD_ERR_INVALID_ARG, "pixel_offset and the depth bounds of the view filter and the point options differ");
  }
  if (B > m->cfg.max_batch) MD_FAIL(MD_ERR_SHAPE, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
  if (m->kind == 0 && cam.focal_px && c.in_kind == MD_MEM_HOST)
    for (int i = 0; i < B; ++i)
      if (!std::isfinite(cam.focal_px[i]) || !(cam.focal_px[i] > 0.f))
        MD_FAIL(MD_ERR_INVALID_ARG, "f_px[%d] = %g: a focal length must be finite and > 0", i, (double)cam.focal_px[i]);
  if (!model_root(m)->committed) MD_FAIL(MD_ERR_INVALID_ARG, "weights were modified; call md_model_commit_weights first");
  MD_HIP(hipSetDevice(m->dev->ordinal));
  hipStream_t st = model_stream(m, stream);
  auto body = [&]() { return points_eager(m, c, dual, rows, st); };
  if (!m->graph_enabled) return body();
  // a graph only replays at the model's current input size (its workspace plan)
  bool eligible = c.in_kind == MD_MEM_DEVICE && c.out_kind == MD_MEM_DEVICE;
  if (match_on(c.mat) && c.mat->target_kind == MD_MEM_HOST) eligible = false;  // a host target is copied with every call
  if (register_on(c.reg) && c.reg->target_kind == MD_MEM_HOST) eligible = false;
  if (m->kind == 1) {
    int ps = 0, ch = 0, cw = 0;
    da3_frame_info(m, &ps, &ch, &cw);
    eligible = eligible && ch == H && cw == W;
  } else {
    eligible = eligible && H == m->S && W == m->S;
  }
  return run_with_graph(m, st, points_graph_key(m, c, st), eligible, body);
}

}  // namespace md
