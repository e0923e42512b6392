// Launchers for the HBM-bound and small kernels of the Depth Pro path (device pointers only).
#pragma once

#include "../md_common.h"

namespace md {

// a1  rgb_to_input_tensor (src/inference.rs:79-121): u8 HWC -> f32 NCHW, one image.
int launch_rgb_to_input(const uint8_t* rgb, int w, int h, float* out, hipStream_t s);

// ---- frame path (kernels/frame.hip; md_process_frame) ----
// One axis of the separable Catmull-Rom resampler on the device: win[o] = (left, count), weights w[o * maxc + k].
struct CrAxis {
  const int2* win;
  const float* w;
  int maxc;
};
// host: window and normalised weights of output o of an in_len -> out_len pass (pipeline._sample_axis; weights may be null)
void catmull_rom_window(int in_len, int out_len, int o, int* left, int* count, float* weights);
int catmull_rom_max_taps(int in_len, int out_len);
// host: the byte columns [xb0, xb0 + 4 nq) of an input row that output columns [cx, cx + tw) read
void catmull_rom_span(const int* left, const int* count, int cx, int tw, int* xb0, int* nq);
// u8 [B,h,w,3] -> vertical pass over output rows [cy, cy + th) into tmp [B,th,4 nq] f32 -> horizontal pass over output
// columns [cx, cx + tw) -> out_u8 [B,th,tw,3] and / or out_nchw [B,3,th,tw] (rgb_to_input normalisation); either may be null
int launch_resize_catmull_rom(const uint8_t* rgb, int B, int h, int w, const CrAxis& ax_v, int cy, int th, const CrAxis& ax_h, int cx,
                              int tw, int xb0, int nq, float* tmp, uint8_t* out_u8, float* out_nchw, hipStream_t s);
// depth [B,h,w] -> crop (cx, cy, cw, ch) -> resize = 1: bilinear restore to ow x oh with sx = cw / ow, sy = ch / oh
// (pipeline.resize_depth_field); resize = 0: ow = cw, oh = ch
struct DisplayGeom {
  int B, h, w, cx, cy, cw, ch, ow, oh, resize;
  float sx, sy;
};
int display_parts(const DisplayGeom& g);  // partial min / max pairs per frame (parts needs B * display_parts(g) float2)
int launch_depth_display(const float* depth, const DisplayGeom& g, int normalize, int format, void* out, float* range, float2* parts,
                         hipStream_t s);

// ---- point path (kernels/points.hip; md_op_unproject, md_infer_points) ----
// depth [B,H,W] (+ confidence, + u8 rgb [B,H,W,3]) and pinhole cameras -> dense point map / mask and the ordered, compacted
// cloud. Every pointer is a device pointer; the cameras are read in the kernels. K [B,3,3] or focal [B] (K = f, f, W/2, H/2);
// E [B,3,4] world-to-camera when world = 1.
struct PointsParams {
  const float* depth = nullptr;
  const float* conf = nullptr;
  const uint8_t* rgb = nullptr;
  const float *K = nullptr, *E = nullptr, *focal = nullptr;
  int B = 0, H = 0, W = 0;
  float off = 0.f, dmin = 0.f, dmax = 0.f, conf_min = 0.f, edge_rtol = 0.f;  // dmin / dmax already resolved (no 0 = default here)
  int stride = 1, world = 0;
  float* point_map = nullptr;
  uint8_t* mask = nullptr;
  float* xyz = nullptr;
  uint8_t* rgb_out = nullptr;
  float* conf_out = nullptr;
  int32_t* count = nullptr;  // [B + 1]; non-null = the list passes run
  long capacity = 0;
};
// the normals forms of classify / scatter (md_op_unproject_normals): all zero = the forms without normals
struct NormalsParams {
  float* normal_map = nullptr;  // [B,H,W,3]
  float* normals = nullptr;     // [capacity,3], rows parallel to xyz; needs p.count
  float min_cos = 0.f;          // > 0: the grazing-angle test enters the validity
};
// bytes of the list's scratch (bit mask, block counts, block offsets) for B views of H x W; 256-byte aligned parts
size_t points_scratch_bytes(int B, int H, int W);
// classify (+ scan + scatter when p.count is set); scratch may be null when p.count is. nrm null or all zero: the launches
// and kernels of the point path without normals
int launch_unproject(const PointsParams& p, void* scratch, hipStream_t s, const NormalsParams* nrm = nullptr);

// ---- view filter (kernels/view_filter.hip; md_op_filter_views, md_infer_points_filtered) ----
// depth [B,H,W] (+ confidence) and the cameras of the point path -> the depth with rejected pixels set to 0: an exact
// confidence percentile over all candidates of the call (radix select, four histogram + select launch pairs), then the
// cross-view support count. Every pointer is a device pointer. E is read only when rtol > 0.
struct ViewFilterParams {
  const float* depth = nullptr;
  const float* conf = nullptr;
  const float *K = nullptr, *E = nullptr, *focal = nullptr;
  int B = 0, H = 0, W = 0;
  float off = 0.f, dmin = 0.f, dmax = 0.f;  // dmin / dmax already resolved
  int q = 0;                                // percentile, 0 = off (tau = 0)
  float rtol = 0.f;                         // 0 = no cross-view test (support = 0, every survivor is kept)
  int min_views = 0;
  float* depth_out = nullptr;
  uint8_t* support = nullptr;
  float* tau = nullptr;     // [1]
  int32_t* kept = nullptr;  // [B + 1]
};
constexpr int kViewFilterMaxViews = 64;  // support is u8 and the B cameras sit in LDS
// bytes of the filter's scratch (histogram table, select state)
size_t view_filter_scratch_bytes();
int launch_view_filter(const ViewFilterParams& p, void* scratch, hipStream_t s);

// ---- voxel thinning (kernels/voxel.hip; md_op_voxel_thin, md_infer_points_voxel) ----
// A point list xyz [n,3] (+ conf [n], u8 rgb [n,3], normals [n,3]) -> one row per occupied voxel, the rows in ascending input
// index: reset, insert (hash table of 64-bit cell keys; atomicMax of a rank word, integer count), select (ballot words), scan,
// scatter. Every pointer is a device pointer. Selection only: no float is summed, nothing depends on the order of arrival.
struct VoxelParams {
  const float* xyz = nullptr;
  const float* conf = nullptr;       // null: every weight is 0 and the smallest index of a voxel wins
  const uint8_t* rgb = nullptr;      // carried to rgb_out
  const float* normals = nullptr;    // carried to normals_out
  const int32_t* in_count = nullptr; // [B + 1] per-view rows of the input, then their total = the live rows (read on the device); null: n rows, one view
  int n = 0;                         // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  float voxel = 0.f;
  float* xyz_out = nullptr;
  float* conf_out = nullptr;
  uint8_t* rgb_out = nullptr;
  float* normals_out = nullptr;
  int32_t* index = nullptr;    // [capacity] source row
  int32_t* weight = nullptr;   // [capacity] in-range points of the survivor's voxel
  int32_t* count = nullptr;    // [B + 1] survivors per view, then their total
  int32_t* dropped = nullptr;  // [1] rows that are not finite or out of range
  long capacity = 0;
};
// table slots for n rows: the power of two >= max(2 n, 1024)
size_t voxel_table_slots(int n);
// bytes of the scratch (table 20 B per slot | slot of every row | ballot words | block counts | block offsets | flags)
size_t voxel_scratch_bytes(int n);
// five launches on s. flags (device, inside the scratch): voxel_flags(scratch, n)[0] != 0 after the launches = the probe loop ran out
int launch_voxel_thin(const VoxelParams& p, void* scratch, hipStream_t s);
const int32_t* voxel_flags(const void* scratch, int n);
// the tail of launch_voxel_thin, for any keep decision in its ballot layout (row = tile * 4096 + step * 256 + thread, word =
// step * 4 + wave; counts[tile] = the set bits of the tile): scan (offsets, p.count per view) and scatter (the rows, p.index;
// p.weight from cnt[slot[i]], both may be null without it). Nothing is launched without p.count; counts only without a row output.
int launch_list_compact(const VoxelParams& p, const unsigned* cnt, const int* slot, const unsigned long long* bits, const int* counts,
                        int* offsets, hipStream_t s);
// what launch_voxel_thin (with p.count) left in its scratch about every row, for the decimation's remap: the slot of a live row
// (-1 out of range), the rank word of a slot (its low word names the survivor), the keep bits and the tile offsets
struct VoxelRanks {
  const int* slot;
  const unsigned long long* rank;
  const unsigned long long* bits;
  const int* offsets;
};
VoxelRanks voxel_ranks(const void* scratch, int n);

// ---- vertex-clustering decimation (kernels/decimate.hip; md_op_decimate_mesh) ----
// Vertices: launch_voxel_thin on `v`, unchanged, then remap [n] from the scratch it leaves (two launches). Faces [nf,3] over the
// input rows -> mapped through remap and classified, a hash set of oriented triangles that holds face ids, select (ballot
// words), scan (launch_list_compact's), scatter. Every pointer is a device pointer. Selection only: integer atomics, nothing
// depends on the order of arrival.
struct DecimateParams {
  VoxelParams v;                           // the vertex side; v.count null: the counts go to the scratch
  int32_t* remap = nullptr;                // [v.n]; null: it lives in the scratch
  const int32_t* faces = nullptr;          // [nf,3]
  const int32_t* in_face_count = nullptr;  // [v.B + 1] per-view faces of the input, then their total = the live faces; null: nf faces, one view
  int nf = 0;                              // faces the launches cover: the live count is min(in_face_count[B], nf)
  int32_t* faces_out = nullptr;            // [face_capacity,3]
  int32_t* face_index = nullptr;           // [face_capacity]
  int32_t* face_count = nullptr;           // [v.B + 1]; null: no select / scan / scatter
  int32_t* faces_dropped = nullptr;        // [3]
  long face_capacity = 0;
};
// bytes of the scratch: voxel thinning's for n rows, then counts / remap homes, the face table (4 B per slot), the mapped
// triples 12 nf, the slot of every face, ballot words, block counts, block offsets, flags
size_t decimate_scratch_bytes(int n, int nf, int B);
// flags[0] != 0 after the launches = a probe loop of the face table ran out (the vertex table's flag: voxel_flags(scratch, n))
int launch_decimate_mesh(const DecimateParams& p, void* scratch, hipStream_t s);
const int32_t* decimate_flags(const void* scratch, int n, int nf, int B);
// one launch: a face list [rows,3] with its device counts [B + 1] copied to a caller's buffers: the counts, and the
// first min(count[B], rows, capacity) faces; the memory behind them stays untouched. Nothing without count_out; faces_out may be null
int launch_copy_faces(const int32_t* faces, const int32_t* count, int B, long rows, int32_t* faces_out, int32_t* count_out, long capacity,
                      hipStream_t s);
// the decimation's rank step for any keep bits in the ballot layout with the tile offsets of their scan: remap[i] = the output
// row of every kept row i < n; the other rows of remap are not written
int launch_rank_rows(const unsigned long long* bits, const int* offsets, int n, int32_t* remap, hipStream_t s);

// ---- connected components of a mesh, island removal (kernels/components.hip, kernels/components_math.h; md_op_mesh_components) ----
// Faces [nf,3] over n rows -> label (the smallest row of every row's component, by a lock-free union-find), the valid faces of
// every component, and the faces of the components with at least min_faces faces, in input order. With `compact` the rows those
// faces name are compacted through launch_list_compact (v's row outputs, v.index, v.count) and the faces are written through
// remap. Every pointer is a device pointer. Integers only: nothing depends on the order of arrival.
struct ComponentsParams {
  VoxelParams v;                           // the rows: v.n, v.B, v.in_count; with `compact` also the row inputs / outputs, v.index, v.count, v.capacity
  const int32_t* faces = nullptr;          // [nf,3]
  const int32_t* in_face_count = nullptr;  // [v.B + 1] per-view faces of the input, then their total = the live faces; null: nf faces, one view
  int nf = 0;                              // faces the launches cover: the live count is min(in_face_count[B], nf)
  int min_faces = 1;
  int compact = 0;
  int32_t* label = nullptr;                // [v.n]; rows behind the live count: -1
  int32_t* component_faces = nullptr;      // [v.n]; rows behind the live count: 0
  int32_t* remap = nullptr;                // [v.n], compact only; null: it lives in the scratch
  int32_t* faces_out = nullptr;            // [face_capacity,3]
  int32_t* face_index = nullptr;           // [face_capacity]
  int32_t* face_count = nullptr;           // [v.B + 1]; null: no face scan / scatter
  int32_t* stats = nullptr;                // [5] invalid, dropped, clipped, components, components kept; null: they go to the scratch
  long face_capacity = 0;
};
// bytes of the scratch: parent and size 4 B per row each, a remap and row count home, ballot words / tile counts / tile offsets of
// the faces and of the rows, the counters
size_t components_scratch_bytes(int n, int nf, int B);
int launch_mesh_components(const ComponentsParams& p, void* scratch, hipStream_t s);

// ---- Taubin / Laplacian smoothing of a mesh and its vertex normals (kernels/smooth.hip, kernels/smooth_math.h; md_op_smooth_mesh) ----
// Rows xyz [n,3] and faces [nf,3] over them -> the smoothed rows and the area-weighted normals of the smoothed faces. The rows
// move on an integer lattice of side `step` and every sum is an int64 sum, so nothing depends on the order of arrival
// (include/mi_depth.h states the contract, pipeline.smooth_mesh restates it). Every pointer is a device pointer.
struct SmoothParams {
  const float* xyz = nullptr;              // [n,3]
  const int32_t* in_count = nullptr;       // [B + 1] the list's device count: the live rows are min(in_count[B], n); null: n rows
  int n = 0;                               // rows the launches cover
  int B = 1;
  const int32_t* faces = nullptr;          // [nf,3]
  const int32_t* in_face_count = nullptr;  // [B + 1] likewise for the faces; null: nf faces
  int nf = 0;
  float step = 0.f, lambda = 0.f, mu = 0.f;
  int iterations = 0, pin_boundary = 0;
  float* xyz_out = nullptr;                // [capacity,3]; null: skip
  float* normals_out = nullptr;            // [capacity,3]; null: no normal launches
  int32_t* stats = nullptr;                // [5] invalid faces, degenerate faces, rows not in range, open rows, moved rows; null: scratch
  long capacity = 0;                       // rows of the outputs that may be written
};
// bytes of the scratch: per row the lattice position and the accumulator (3 int64 each), open (uint64), deg and the range flag
size_t smooth_scratch_bytes(int n);
int launch_smooth_mesh(const SmoothParams& p, void* scratch, hipStream_t s);

// ---- radius outlier removal (kernels/outlier.hip; md_op_radius_outliers, md_infer_points_outlier) ----
// A point list xyz [n,3] (+ conf, rgb, normals rows) -> the rows with at least k other rows within `radius`, in ascending input
// index: reset, insert (voxel thinning's table with a count per slot), bucket allocation, fill (the positions bucket by
// bucket), search (27 cells around the row's, saturating at k; ballot words), then launch_list_compact. Every pointer is a
// device pointer. Selection only: integer counts of an f32 predicate, nothing depends on the order of arrival.
struct OutlierParams {
  const float* xyz = nullptr;
  const float* conf = nullptr;        // carried to conf_out
  const uint8_t* rgb = nullptr;       // carried to rgb_out
  const float* normals = nullptr;     // carried to normals_out
  const int32_t* in_count = nullptr;  // as VoxelParams::in_count
  int n = 0;                          // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  float radius = 0.f;
  int k = 1;                          // min_neighbours
  float* xyz_out = nullptr;
  float* conf_out = nullptr;
  uint8_t* rgb_out = nullptr;
  float* normals_out = nullptr;
  int32_t* index = nullptr;       // [capacity] source row
  int32_t* neighbours = nullptr;  // [n] min(neighbours, k) of every live input row, -1 out of range
  int32_t* count = nullptr;       // [B + 1] survivors per view, then their total
  int32_t* dropped = nullptr;     // [1] rows that are not finite or out of range
  long capacity = 0;
};
constexpr int kOutlierMaxNeighbours = 1 << 20;
// bytes of the scratch (table 20 B per slot | slot and bucket position of every row | buckets 12 n | ballot words | block counts |
// block offsets | flags)
size_t outlier_scratch_bytes(int n);
// flags[0] != 0 after the launches = a probe loop ran out of table
int launch_radius_outliers(const OutlierParams& p, void* scratch, hipStream_t s);
const int32_t* outlier_flags(const void* scratch, int n);

// ---- RANSAC plane extraction (kernels/planes.hip, kernels/planes_math.h; md_op_fit_planes, md_infer_points_planes) ----
// A point list xyz [n,3] (+ conf, rgb, normals rows) -> up to `planes` planes, one per round: the live rows are indexed in row
// order (classify / scan / scatter), `hypotheses` triples are drawn from them by a fixed mixer, every live row is tested against
// every hypothesis (the count kernel), the largest count wins (ties: the smallest hypothesis) and its inliers get the round as
// label and leave the live set. mode 1 / 2 then compacts the rows without / with a plane through launch_list_compact. Every
// pointer is a device pointer. Selection only: integer counts of an f32 predicate, nothing depends on the order of arrival.
struct PlanesParams {
  const float* xyz = nullptr;
  const float* conf = nullptr;        // carried to conf_out
  const uint8_t* rgb = nullptr;       // carried to rgb_out
  const float* normals = nullptr;     // the normals predicate (normal_min_cos > 0); carried to normals_out
  const int32_t* in_count = nullptr;  // as VoxelParams::in_count
  int n = 0;                          // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  int planes = 0, hypotheses = 0, min_inliers = 0, mode = 0;
  unsigned seed = 0u;
  float tol = 0.f, normal_min_cos = 0.f, axis_min_cos = 0.f;
  float axis[3] = {0.f, 0.f, 0.f};
  float* plane = nullptr;          // [planes,4]; null: skip
  int32_t* plane_count = nullptr;  // [planes + 1]; null: skip
  int32_t* hypothesis = nullptr;   // [planes]; null: skip
  int32_t* label = nullptr;        // [n]; null: it lives in the scratch
  int32_t* dropped = nullptr;      // [1]; null: skip
  float* xyz_out = nullptr;        // mode 1 / 2: the compacted rows
  float* conf_out = nullptr;
  uint8_t* rgb_out = nullptr;
  float* normals_out = nullptr;
  int32_t* index = nullptr;  // [capacity] source row
  int32_t* count = nullptr;  // [B + 1] survivors per view, then their total
  long capacity = 0;
};
constexpr int kPlaneCountRows = 8;   // rows a thread of the count kernel keeps in registers
constexpr int kPlaneCountChunk = 4;  // hypotheses of one trip of its loop: their planes are loaded together; a tail loop takes the rest
// bytes of the scratch (label home | ballot words | tile counts | tile offsets | live index 4 n | hypotheses 16 B + count 4 B | state)
size_t planes_scratch_bytes(int n, int hypotheses);
int launch_fit_planes(const PlanesParams& p, void* scratch, hipStream_t s);

// ---- DBSCAN / Euclidean clustering (kernels/clusters.hip; md_op_cluster_points, md_infer_points_clusters) ----
// A point list xyz [n,3] (+ conf, rgb, normals rows) -> the cluster of every row: the outlier removal's cell buckets with the
// source row beside xyz (16-byte entries), count (core rows: at least k neighbours), union (a lock-free union-find over the core
// rows, one hook per neighbour pair of core rows), flatten, border (a non-core row takes the smallest label among its core
// neighbours), sizes, the size filter, dense ids by the ordered compaction, boxes by integer atomics on ordered keys. mode 1
// then compacts the rows of kept clusters through launch_list_compact. Every pointer is a device pointer. Integers on an f32
// predicate: nothing depends on the order of arrival.
struct ClustersParams {
  const float* xyz = nullptr;
  const float* conf = nullptr;        // carried to conf_out
  const uint8_t* rgb = nullptr;       // carried to rgb_out
  const float* normals = nullptr;     // carried to normals_out
  const int32_t* in_count = nullptr;  // as VoxelParams::in_count
  int n = 0;                          // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  float radius = 0.f;
  int k = 0, min_points = 1, max_points = 0, mode = 0;
  int32_t* label = nullptr;         // [n]; null: skip
  int32_t* cluster_size = nullptr;  // [n]; null: skip
  int32_t* cluster = nullptr;       // [n]; null: skip
  int32_t* table_label = nullptr;   // [table_capacity]; null: skip
  int32_t* table_size = nullptr;    // [table_capacity]; null: skip
  float* box = nullptr;             // [table_capacity,6]; null: skip
  long table_capacity = 0;
  int32_t* stats = nullptr;    // [4] clusters found, clusters kept, noise rows, rows in kept clusters; null: they live in the scratch
  int32_t* dropped = nullptr;  // [1]; null: skip
  float* xyz_out = nullptr;    // mode 1: the compacted rows
  float* conf_out = nullptr;
  uint8_t* rgb_out = nullptr;
  float* normals_out = nullptr;
  int32_t* index = nullptr;  // [capacity] source row
  int32_t* count = nullptr;  // [B + 1] survivors per view, then their total
  long capacity = 0;
};
constexpr int kClusterMaxNeighbours = 1 << 20;
constexpr int kClusterStatsFlag = 8;  // clusters_flags(..)[8 .. 12): the four counters when `stats` is null
// bytes of the scratch (table 20 B per slot | slot, bucket row, parent, size, rank, dense id of every row | buckets 16 n |
// box keys 24 B per table row | ballot words | tile counts | tile offsets | flags)
size_t clusters_scratch_bytes(int n, long table_capacity);
// flags[0] != 0 after the launches = a probe loop ran out of table
int launch_cluster_points(const ClustersParams& p, void* scratch, hipStream_t s);
const int32_t* clusters_flags(const void* scratch, int n, long table_capacity);

// ---- nearest row of a reference cloud (kernels/match.hip; md_op_match_points, md_infer_points_match) ----
// A point list xyz [n,3] (+ conf, rgb, normals rows) and a target list [t,3] -> the nearest target row of every row: the
// clustering's cell buckets with 16-byte entries, built from the target and sized by it, then one launch over the tiles of the
// source: 27 probes with loads only, the running minimum of (bits(d2) << 32) | target row, the ballot bit of the mode and the
// counters. mode 1 / 2 then compacts the matched / unmatched rows through launch_list_compact. Every pointer is a device pointer.
// A selection on a deterministic f32 value: nothing depends on the order of arrival.
struct MatchParams {
  const float* xyz = nullptr;
  const float* conf = nullptr;        // carried to conf_out
  const uint8_t* rgb = nullptr;       // carried to rgb_out
  const float* normals = nullptr;     // carried to normals_out
  const int32_t* in_count = nullptr;  // as VoxelParams::in_count
  int n = 0;                          // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  const float* target = nullptr;  // [t,3]
  int t = 0;
  float radius = 0.f;
  float tol[4] = {0.f, 0.f, 0.f, 0.f};  // 0: unused
  int mode = 0;
  int32_t* nearest = nullptr;  // [n]; null: skip
  float* dist2 = nullptr;      // [n]; null: skip
  int32_t* stats = nullptr;    // [8] in-range rows, matched rows, target rows in the grid, 0, rows within tol[0..4); null: they live in the scratch
  int32_t* dropped = nullptr;  // [1]; null: skip
  float* xyz_out = nullptr;    // mode 1 / 2: the compacted rows
  float* conf_out = nullptr;
  uint8_t* rgb_out = nullptr;
  float* normals_out = nullptr;
  int32_t* index = nullptr;  // [capacity] source row
  int32_t* count = nullptr;  // [B + 1] survivors per view, then their total
  long capacity = 0;
};
constexpr int kMatchStatsFlag = 8;  // match_flags(..)[8 .. 16): the eight counters when `stats` is null
// bytes of the scratch (table 20 B per slot of the target's table | slot of every target row | buckets 16 t | ballot words |
// tile counts | tile offsets of the source | flags)
size_t match_scratch_bytes(int n, int t);
// flags[0] != 0 after the launches = a probe loop ran out of table
int launch_match_points(const MatchParams& p, void* scratch, hipStream_t s);
const int32_t* match_flags(const void* scratch, int n, int t);

// ---- rigid ICP registration onto a reference cloud (kernels/register.hip; md_op_register_points) ----
// A source list xyz [n,3] (+ normals rows) and a target list [t,3] -> the 3x4 transform (R row-major, then t; f64) that moves the
// source onto the target: the matching's grid (match_grid.h) built once from the target, then `iterations` times a step launch
// (move every row under A, walk the 27 cells, fold the sixteen f64 leaves of every pair into fixed-shape tile sums) and a
// one-workgroup reduce-and-solve launch (register_math.h), then an evaluation step under the final A and its reduce without a
// solve. The sums have a fixed tree shape: nothing depends on the order of arrival. Every pointer is a device pointer.
struct RegisterParams {
  const float* xyz = nullptr;
  const float* normals = nullptr;     // rotated into normals_out
  const int32_t* in_count = nullptr;  // as VoxelParams::in_count
  int n = 0;                          // rows the launches cover: the live count is min(in_count[B], n)
  int B = 1;
  const float* target = nullptr;  // [t,3]
  int t = 0;
  float radius = 0.f;
  int iterations = 0;  // K, 1..64
  int min_pairs = 3;
  double rot_eps = 0., trans_eps = 0.;  // both 0: no stop test
  double init[12] = {1., 0., 0., 0., 1., 0., 0., 0., 1., 0., 0., 0.};  // A_0
  double* transform = nullptr;  // [12]; null: skip
  int32_t* pairs = nullptr;     // [K + 1]; null: skip
  double* sum_d2 = nullptr;     // [K + 1]; null: skip
  int32_t* stats = nullptr;     // [8] solves done, status, in-range rows and pairs of the evaluation pass, target rows in the grid, 0, 0, 0; null: they live in the scratch
  int32_t* dropped = nullptr;   // [1]; null: skip
  float* xyz_out = nullptr;     // [n,3] the moved rows of the evaluation pass; may be xyz; null: skip
  float* normals_out = nullptr; // [n,3]; null: skip
  int32_t* nearest = nullptr;   // [n] as MatchParams::nearest under the final transform; null: skip
  float* dist2 = nullptr;       // [n]; null: skip
  // the point-to-plane form: off by default, and then nothing of it is read
  bool plane = false;                     // the step sums the 29 leaves of every usable pair, the solve is reg_solve_plane
  const float* target_normals = nullptr;  // [t,3]; plane: required with t > 0
  double* sum_r2 = nullptr;               // [K + 1] the sum of squared point-to-plane residuals; plane only; null: skip
};
// bytes of the scratch (the matching's table and buckets of the target | 128 B of tile sums and 4 B of pair count per source
// tile | the transform | flags)
size_t register_scratch_bytes(int n, int t);
// the same for the point-to-plane form: 232 B of tile sums per source tile
size_t register_plane_scratch_bytes(int n, int t);
// flags[0] != 0 after the launches = a probe loop ran out of table. p.plane picks the form; the scratch is that form's.
int launch_register_points(const RegisterParams& p, void* scratch, hipStream_t s);
const int32_t* register_flags(const void* scratch, int n, int t);
const int32_t* register_plane_flags(const void* scratch, int n, int t);

// ---- point rendering (kernels/render.hip; md_op_render_points, md_infer_points_render) ----
// A point list xyz [n,3] (+ u8 rgb [n,3]) and T pinhole target cameras -> per target a z-buffered depth / source row / colour
// image: clear, splat (atomicMin of (bits(p.z) << 32) | row over the footprint), resolve. Every pointer is a device pointer.
// Selection only: nothing depends on the order of arrival.
struct RenderParams {
  const float* xyz = nullptr;
  const uint8_t* rgb = nullptr;       // gathered to rgb_out
  const int32_t* count = nullptr;     // one word, read on the device: the live rows are min(max(*count, 0), n); null: n rows
  int n = 0;                          // rows the splat launch covers
  int T = 0, H = 0, W = 0;            // targets and their size
  const float *K = nullptr, *E = nullptr, *focal = nullptr;  // [T,3,3] or [T]; [T,3,4] world-to-camera, null: p = X
  float off = 0.f, znear = 0.f, zfar = 0.f;                  // znear / zfar already resolved
  int radius = 0;
  float* depth = nullptr;      // [T,H,W]
  int32_t* index = nullptr;    // [T,H,W]
  uint8_t* rgb_out = nullptr;  // [T,H,W,3]
  int32_t* filled = nullptr;   // [T + 1]
};
constexpr int kRenderMaxRadius = 16;
// bytes of the key buffer: 8 per pixel, 256-byte aligned
size_t render_scratch_bytes(int T, int H, int W);
// three launches on s (the splat is skipped when n == 0)
int launch_render_points(const RenderParams& p, void* scratch, hipStream_t s);

// ---- triangle mesh of the depth grid (kernels/mesh.hip; md_op_mesh_grid, md_op_unproject_mesh, md_infer_points_mesh) ----
// depth [B,H,W] and the map pixel -> list row [B,H,W] -> the faces of the strided lattice as rows of the list, ordered by
// (view, row, column, triangle): classify (two ballot words per wave and step), scan, scatter. Every pointer is a device
// pointer. Selection only: no atomics, no float sums.
struct MeshParams {
  const float* depth = nullptr;
  const int32_t* pixel_index = nullptr;  // [B,H,W]: the list row of a pixel, -1 = not in the list
  int B = 0, H = 0, W = 0, stride = 1;
  long limit = 0;                        // a corner is usable when 0 <= index < limit (already resolved: no 0 = none here)
  float max_rtol = 0.f;                  // 0 = every edge passes
  int32_t* faces = nullptr;              // [face_capacity,3]
  int32_t* face_count = nullptr;         // [B + 1]; null = no face launches
  long face_capacity = 0;
};
// bytes of the face scratch (ballot word pairs, block counts, block offsets); 256-byte aligned parts
size_t mesh_scratch_bytes(int B, int H, int W, int stride);
// one launch: pixel_index [B,H,W] from the bits and offsets launch_unproject (with p.count) left in `points_scratch` for this shape
int launch_mesh_index(int B, int H, int W, const void* points_scratch, int32_t* pixel_index, hipStream_t s);
// classify (skipped on a lattice without quads), scan, scatter (skipped without p.faces); nothing without p.face_count
int launch_mesh_grid(const MeshParams& p, void* scratch, hipStream_t s);

// ---- mesh rasterisation (kernels/raster.hip; md_op_render_mesh, md_infer_points_raster) ----
// A vertex list xyz [n,3] (+ u8 rgb [n,3]), faces [nf,3] over its rows and T pinhole target cameras -> per target a z-buffered
// depth / face / colour image: clear, setup (small faces drawn in place, larger ones queued), large (the queue), resolve. Every
// pointer is a device pointer. Selection only: nothing depends on the order of arrival.
struct RasterParams {
  const float* xyz = nullptr;
  const uint8_t* rgb = nullptr;       // interpolated to rgb_out
  const int32_t* faces = nullptr;     // [nf,3] rows of xyz; an index outside 0..n-1 skips the face (tested on the device)
  const int32_t* count = nullptr;     // one word, read on the device: the live faces are min(max(*count, 0), nf); null: nf faces
  int n = 0, nf = 0;                  // rows of xyz; faces the setup launch covers
  int T = 0, H = 0, W = 0;            // targets and their size
  const float *K = nullptr, *E = nullptr, *focal = nullptr;  // [T,3,3] or [T]; [T,3,4] world-to-camera, null: p = X
  float off = 0.f, znear = 0.f, zfar = 0.f;                  // znear / zfar already resolved
  int cull = 0, max_extent = 64;                             // max_extent already resolved: 1..kRasterMaxExtent
  float* depth = nullptr;      // [T,H,W]
  int32_t* face = nullptr;     // [T,H,W]
  uint8_t* rgb_out = nullptr;  // [T,H,W,3]
  int32_t* filled = nullptr;   // [T + 1]
  int32_t* skipped = nullptr;  // [T + 1]
};
constexpr int kRasterMaxExtent = 1024;
constexpr int kRasterDefaultExtent = 64;
// the box size up to which the setup kernel draws a face in its own thread (a compile-time constant of kernels/raster.hip)
int raster_inline_pixels();
// md_debug_raster_queue: sets the queue capacity of later calls (0 = the default; negative: no change) -> the previous setting
int raster_queue_capacity(int capacity);
// the capacity in force, in (face, target) pairs
int raster_queue_entries();
// bytes of keys (8 per pixel) | queue counter | queue (8 per entry); 256-byte aligned parts
size_t raster_scratch_bytes(int T, int H, int W, int queue_entries);
// four launches on s (setup and large are skipped when nf == 0); queue_entries: what the scratch was sized for
int launch_render_mesh(const RasterParams& p, void* scratch, int queue_entries, hipStream_t s);

// a2  bilinear resize, fp32 NCHW (interpolate.rs:54-121). method: MD_INTERP_*.
// post: 0 none, 1 = 1/clamp(v,1e-4,1e4) (DepthPro::infer tail, mod.rs:356).
int launch_resize_bilinear(const float* in, int planes, int H, int W, float* out, int OH, int OW, int method,
                           int post, hipStream_t s);

// a2+a3 fused: image pyramid (x1 = resize 0.5, x2 = resize 0.25; encoder.rs:326-327), sliding
// window split (encoder.rs:190-232) and 16x16 patch extraction, written as the A matrix of the
// patch-embed GEMM: out[(tile*P + py*g + px)][c*ps*ps + ky*ps + kx], T = bf16 or float.
// Tile order = reference cat order: level0 (j*steps0+i)*B+b, then level1, then level2 (x2).
struct PyramidGeom {
  int B, S, win, ps;         // S = 4*win input size, ps = ViT patch size
  int steps0, stride0;       // level 0 (overlap .25)
  int steps1, stride1;       // level 1 (overlap .5)
  int method;                // MD_INTERP_*
};
// force_generic: the grid-stride kernel that serves InterpolationMethod::Burn / odd geometries also for Custom (parity tests).
int launch_pyramid_patchify(const float* x, const PyramidGeom& g, void* patches, int prec, hipStream_t s, bool force_generic = false);

// Generic ViT patch extraction (any patch size, e.g. 14 for DA3): fp32 NCHW [B,3,H,W] ->
// A[(b*ph + py)*pw + px][c*ps*ps + ky*ps + kx], row length Kp >= 3*ps*ps (tail zero-filled).
// cls_x != nullptr: the launch also writes the cls rows (cls + pos0) and zero padding rows of the fp32 residual stream cls_x
// [B * S, D] (launch_cls_init's work for one sequence group)
int launch_patchify(const float* x, int B, int H, int W, int ps, int Kp, void* out, int prec, hipStream_t s, float* cls_x = nullptr,
                    int S = 0, int n_tokens = 0, int D = 0, const float* cls = nullptr, const float* pos0 = nullptr);

// Bilinear resize of an NHWC tensor (element type by prec), align_corners per `method`
// (MD_INTERP_BURN = align_corners=True, depth_anything3/interpolate.rs:7-47), optional per-pixel
// fp32 addend table [OH*OW, C] (already scaled; the DA3 UV position embedding, dpt.rs:799-828).
int launch_resize_nhwc(const void* in, int B, int H, int W, int C, long ld_in, void* out, int OH, int OW, long ld_out,
                       int method, const float* addend, int prec, hipStream_t s);

// Border correction of a 3x3 convolution (pad 1) that was composed with a preceding biased 1x1 convolution: the 1x1's bias
// reaches the output only through taps inside the map, so the composed bias is one of nine position-class vectors
// bias9[3*ry + rx][C] (ry, rx: 0 first, 1 interior, 2 last row / column). The convolution itself adds the interior vector;
// this adds bias9[class] - bias9[4] to the 2H + 2W - 4 border pixels of every image of the NHWC map (needs H, W >= 2).
int launch_border_bias_fix(void* map, int B, int H, int W, int C, long ld, const float* bias9, int prec, hipStream_t s);

// a3 stand-alone split on fp32 NCHW (debug tap / md_op_split).
int launch_split(const float* x, int B, int C, int S, int win, int stride, int steps, float* out, hipStream_t s);
// a6 stand-alone merge on fp32 NCHW (encoder.rs:234-282).
int launch_merge(const float* tiles, int B, int C, int h, int w, int steps, int pad, float* out, int OH, int OW,
                 hipStream_t s);

// cls token + pos_embed[0] rows and zero padding rows of the fp32 residual stream.
// x[seq*S + 0] = cls_g + pos_g[0]; x[seq*S + n_tokens ..] = 0, group g by sequence ranges.
struct SeqGroups {
  int ngroups;
  int seq0[4];  // first sequence of each group
  int nseq[4];
  const float* a[4];  // per-group pointers (meaning depends on the kernel)
  const float* b[4];
};
int launch_cls_init(float* x, int nseq_total, int S, int n_tokens, int D, const SeqGroups& g, hipStream_t s);

// K3 LayerNorm over D (biased variance), fp32 rows -> T rows (bf16/f32) or fp32 (out_f32).
// gamma/beta per group (a = gamma, b = beta); NULL gamma = non-affine. Rows grouped by sequence.
// prec == MD_PREC_FP8 (and !out_f32): rows of OCP e4m3 bytes, value * fp8_inv_scale, saturating.
// tok0 != nullptr: row 0 of every sequence is first replaced by tok0[seq * tok0_stride ..] (written back through x_rw == x)
int launch_layernorm(const float* x, void* out, long rows, int D, float eps, int S, const SeqGroups& g, int prec,
                     int out_f32, hipStream_t s, float fp8_inv_scale = 1.f, const float* tok0 = nullptr, int tok0_stride = 0,
                     float* x_rw = nullptr);
// The vectors of a LayerNorm folded into the linear layer behind it (gemm.h GemmParams::ln_*): c[n] = sum_k gamma[k] Wr[n][k],
// d[n] = bias[n] + sum_k beta[k] Wr[n][k] with Wr = the weight as its MFMA operand holds it (rounded to bf16 / f16; split-half: hi + lo),
// so that mu * c cancels the mean's share of the accumulators exactly as the operands produced it. W = fp32 master [N][K]; fp64 sums.
int launch_ln_fold_vectors(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, int prec, float* c,
                           float* d, hipStream_t s);
// LayerNorm fold: the per-row partials the producer GEMM wrote ([rows][4][2]: mean and centred sum of squares of each 256-column tile)
// combined (Chan: every term non-negative) into ab[row] = (rstd, -mu * rstd) for the consumer GEMM's epilogue. D = 1024.
// ab[row] = (a, b) for `rows` rows (the diagnostic form of the fold: neutral statistics)
int launch_fill_pairs(float* ab, long rows, float a, float b, hipStream_t s);
int launch_ln_finish(const float* parts, float* ab, long rows, float inv_n, float eps, hipStream_t s);
// fp32 rows -> T rows (hooks: un-normalised tokens), same row layout.
int launch_convert_rows(const float* x, void* out, long count, int prec, hipStream_t s, int width = 0);

// layout converters (debug taps, stand-alone ops)
// ld: logical elements between consecutive output pixels (0 = C); padding columns are left untouched
int launch_nchw_to_nhwc(const float* in, int B, int C, int H, int W, void* out, int prec, int relu, hipStream_t s, long ld = 0);
// head_debug's un-fused tail: pre_out = <relu_map pixel, w> + bias, canonical = relu(pre_out); fp32 [pixels] each (either may be NULL)
int launch_head_tail_debug(const void* relu_map, long ld, long pixels, int C, const float* w, const float* bias, float* pre_out,
                           float* canonical, int prec, hipStream_t s);
int launch_nhwc_to_nchw(const void* in, int B, int C, int H, int W, long ld, int coff, float* out, int prec,
                        hipStream_t s);
// width: logical row width -- needed by MD_PREC_F16X2, whose rows are [hi: width | lo: width] (ignored otherwise)
int launch_rows_to_f32(const void* in, long count, float* out, int prec, hipStream_t s, int width = 0);
int launch_f32_to_rows(const float* in, long count, void* out, int prec, hipStream_t s, int width = 0);

// Small direct convolution, NHWC, fp32 accumulate (FOV head, fov.rs:16-49).
// in: element type by in_prec (MD_PREC_BF16 -> bf16, MD_PREC_F32 -> float); w packed
// [Cout][kh][kw][Cin] f32; add: optional f32 NHWC tensor added to the INPUT (fov.rs:185).
// out_ld: elements between consecutive output pixels (0 = Cout): lets several small heads write the columns of one row.
int launch_conv_direct(const void* in, int in_prec, const float* add, int B, int H, int W, int Cin, const float* w,
                       const float* bias, int Cout, int k, int stride, int pad, int relu, float* out, hipStream_t s, int out_ld = 0);

// ---- fp8 (OCP e4m3) MFMA operands (MD_PREC_FP8) ----
// out[i] = e4m3(clamp(in[i] * inv_scale, +-448)); n a multiple of 4.
int launch_f32_to_fp8(const float* in, long n, float inv_scale, void* out, hipStream_t s);
// W [N][K] f32 -> e4m3 [N][Kp] (K zero-padded to Kp) with one scale per output row: scale[n] = amax_n / 448 (1 for an
// all-zero row); the GEMM epilogue multiplies the accumulator by activation_scale * scale[n].
int launch_pack_fp8_rows(const float* w, int N, int K, int Kp, void* out, float* scale, hipStream_t s);

// ---- Depth-Anything-v3 `small` backbone extras (burn_dino, restated -- see oracle/da3_ref.py) ----
// Per-head affine LayerNorm(64) of q and k followed by the 2-D rotary embedding, in place on qk [rows, 2D] T.
// rope_cos/rope_sin: [max_pos + 1][16] tables (angle = pos * base^(-f/16)). global_pos: every patch at (1,1).
// The q rows arrive scaled by q_scale (the QKV epilogue's) and leave scaled by it; their LayerNorm runs with eps * q_scale^2, which
// is LN(q; eps) of the unscaled projection. Rows t >= n_tokens are left alone.
int launch_qk_norm_rope(void* qk, long rows, int S, int n_tokens, int D, int heads, int pw, const float* q_gamma,
                        const float* q_beta, const float* k_gamma, const float* k_beta, float eps, const float* rope_cos,
                        const float* rope_sin, int global_pos, float q_scale, int prec, hipStream_t s);
// x[b*S + 0, :] = src[b*src_stride + 0:D] for every sequence (the camera token replaces the cls slot): src_stride 0 = the one
// learned token for all, D = one encoded token per image (`infer_with_camera`)
int launch_set_token0(float* x, int nseq, int S, int D, const float* src, hipStream_t s, int src_stride = 0);

// ---- Depth-Anything-v3 camera encoder (kernels/camera.hip; camera.rs:50-110) ----
#define MD_CAM_MAX_VIEWS 16
struct CamEncW {
  static constexpr int kMaxDepth = 8;
  const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;  // PoseBranch: [D/2, 9], [D, D/2]
  const float *tn_g, *tn_b, *on_g, *on_b;      // token_norm, trunk_norm
  struct Blk {
    const float *n1g, *n1b, *n2g, *n2b, *qkv_w, *qkv_b, *proj_w, *proj_b, *ls1, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ls2;
  } blk[kMaxDepth];
  int depth;
};
// camera DECODER (camera.rs:143-199, 281-358): cam [B, din] fp32 -> pose [B, 9] (+ extrinsics [B, 12], intrinsics [B, 9], either may be
// null); h1 / h2 = [B, din] scratch. Three launches: two multi-workgroup din x din linears (+ReLU), one heads + tail kernel.
struct CamDecW {
  const float *w1, *b1, *w2, *b2, *wt, *bt, *wq, *bq, *wf, *bf;
};
int launch_camera_decoder(const float* cam, int B, int din, const CamDecW& w, int H, int W, float* h1, float* h2, float* pose, float* extr,
                          float* intr, hipStream_t s);
size_t camera_encoder_scratch_floats(int B, int V, int D);
// extr [B, V, 3, 4] world-to-camera, intr [B, V, 3, 3] (device) -> out [B, D] (device); one workgroup per image
int launch_camera_encoder(const float* extr, const float* intr, int B, int V, int D, int heads, int H, int W, float eps_tok, float eps_blk,
                          const CamEncW& w, float* scratch, float* out, hipStream_t s);
// hook = LayerNorm_head( cat( x_local, LayerNorm_final(x) ) ) -> T rows [rows, 2D]; optional raw token-0 concat
// [nseq, 2D] f32 (the camera feature).
int launch_hook_cat_ln(const float* x_local, const float* x, long rows, int S, int n_tokens, int D, const float* norm_g,
                       const float* norm_b, float eps_final, const float* head_g, const float* head_b, float eps_head,
                       void* out, float* cam_out, int prec, hipStream_t s);
// pose encoding [B,9] = (t3, quat xyzw, fov_h, fov_w) -> world-to-camera extrinsics [B,3,4], intrinsics [B,3,3]
// (camera.rs:281-416)
int launch_pose_to_camera(const float* pose, int B, int H, int W, float* extrinsics, float* intrinsics, hipStream_t s);

// fov degrees -> focal length / fovy / ratio (mod.rs:330-346, 370-414). All [B] f32.
int launch_fov_post(const float* fov_deg, int B, int H, int W, float* focal_px, float* fovy_rad, float* ratio,
                    hipStream_t s);
// the caller's focal length f_px[B] (device memory, read at run time) -> focal_px = f_px, fovx / fovy / ratio (the known-focal tail).
int launch_focal_post(const float* f_px, int B, int H, int W, float* focal_px, float* fovx_deg, float* fovy_rad, float* ratio,
                      hipStream_t s);
// inv = canonical * ratio[b]; post 1: depth = 1/clamp(inv); post 0: keep inv (then resize).
int launch_depth_post(const float* canonical, const float* ratio, int B, long hw, float* out, int post, hipStream_t s);

// softmax over rows of fp32 scores (fp32 attention path): row length ld, valid n, scale.
int launch_softmax_rows(float* s, long rows, int n_valid, int ld, float scale, hipStream_t st);

// test helpers for the stand-alone attention op: fused fp32 qkv [T, N, 3*heads*64] (timm layout) ->
// engine layout (qk rows padded to SS per sequence, V transposed), and padded rows -> [T, N, D] fp32.
int launch_qkv_split(const float* qkv, int T, int N, int heads, int SS, int kpad, void* qk, void* vT, float q_scale, int prec,
                     hipStream_t s);
int launch_unpad_rows(const void* in, int T, int N, int SS, int D, float* out, int prec, hipStream_t s);

// The softmax scale the fused attention expects to find folded into q: head_dim^-0.5 * log2(e) (head_dim = 64). The QKV
// epilogue (GemmParams::qscale), the q/k-norm + RoPE kernel and the stand-alone op's splitter apply it before q's one
// rounding to the operand type; the kernel then computes p = 2^(q'.k - m). The fp32 three-kernel path keeps q unscaled.
constexpr float kAttnQScale = 0.125f * 1.4426950408889634f;
inline float attn_qscale(int prec) { return prec == MD_PREC_F32 ? 1.0f : kAttnQScale; }

// fused multi-head attention on bf16 / f16 operands (K5; prec = MD_PREC_BF16 | MD_PREC_F16): qk [rows, 2D] (q | k),
// q PRE-SCALED by kAttnQScale, vT [seq][heads][64][kpad], out [rows, D].
// out_fp8_inv > 0 (bf16 only): the output rows are OCP e4m3 bytes (value * out_fp8_inv, saturating).
// prec = MD_PREC_F16X2: split-half operands -- qk rows [q_hi | q_lo | k_hi | k_lo] (4D wide), the lo plane of V^T `v_plane`
// elements behind its hi plane, out rows [hi: D | lo: D]; scores on three MFMA terms, P.V on two or three (attention.hip).
// redo: attention_redo_ints(redo_units) zero-initialised ints owned by the caller's context (one buffer per stream that may run attention
// at a time: redo_units flags, then the compacted list of raised ones at redo + redo_units), or null. redo_units is the buffer's capacity in
// (sequence, head) units (0: exactly nseq * heads); it must not change between the launches that share the buffer, so that no launch's
// list lands on the flags of a later, larger launch. With it, bf16 launches of exactly 577 tokens take the assembly-owned kernel (attn577_gfx950.s)
// once attention_asm_prepare() has loaded its code object on the device; the flags it raises are consumed and cleared inside the same call.
int launch_attention(const void* qk, const void* vT, void* out, int nseq, int S, int n_tokens, int heads, int D,
                     int kpad, int prec, hipStream_t s, float out_fp8_inv = 0.f, long v_plane = 0, int* redo = nullptr,
                     int redo_units = 0);
// Loads the embedded code object on the CURRENT device (idempotent; not capturable -- call it when a context is created).
int attention_asm_prepare();
// Cross-view keys: the nseq sequences come in groups of `views` consecutive ones and every query attends over
// the n_tokens keys of each sequence of its group, in sequence order (one softmax over views * n_tokens keys). Same layout contract as
// launch_attention; bf16 / f16 / split-half operands, plain output rows. views = 1 is launch_attention (same launch, same bits).
int launch_attention_views(const void* qk, const void* vT, void* out, int nseq, int views, int S, int n_tokens, int heads, int D,
                           int kpad, int prec, hipStream_t s, long v_plane = 0, int* redo = nullptr, int redo_units = 0);
// Process-wide: may launch_attention take the assembly kernel? Default 1; returns the previous value (A/B runs, the bench).
int attention_allow_asm(int on);
// launches of the assembly kernel since the library was loaded (what a bench line says about the form it measured)
long attention_asm_launches();
// ints of a `redo` buffer for nunits = nseq * heads units
int attention_redo_ints(int nunits);
// units the assembly kernel flagged on the current device since the last reset (synchronises the device; -1: not loaded)
long attention_asm_redo_units(int reset);
// Per host thread: may launch_attention pick its small-launch form (64 queries x two key groups per workgroup for launches of few
// workgroups over long sequences -- another summation order than the plain form's)? Default 1. Returns the previous value. A model
// in batch-invariant mode (md_model_set_option) runs with 0: one image gives the same bits alone and inside a batch.
int attention_allow_small(int on);
struct AttnSmallScope {
  explicit AttnSmallScope(int on) : prev_(attention_allow_small(on)) {}
  ~AttnSmallScope() { attention_allow_small(prev_); }
  AttnSmallScope(const AttnSmallScope&) = delete;
  AttnSmallScope& operator=(const AttnSmallScope&) = delete;

 private:
  int prev_;
};
// Host-only, per host thread: the form the thread's last attention launch took (md_debug_attention_last_form). launch_attention,
// launch_attention_views and the fp32 three-launch path note it with one thread-local store; no kernel reads it.
enum { ATTN_FORM_NONE = -1, ATTN_FORM_PLAIN = 0, ATTN_FORM_KEYSPLIT = 1, ATTN_FORM_ASM = 2, ATTN_FORM_VIEWS = 3, ATTN_FORM_FP8OUT = 4, ATTN_FORM_F32 = 5 };
struct AttnForm {
  int form = ATTN_FORM_NONE;
  int grid = 0, qw = 0, ks = 0;  // workgroups of the main launch, query waves and key groups per workgroup (fp32 path: units, 0, 0)
};
void attention_note_form(int form, long grid, int qw, int ks);
AttnForm attention_last_form();

}  // namespace md
