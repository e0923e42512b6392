// Nearest row of a reference cloud for every row of a point list, for gfx950 (md_op_match_points, md_infer_points_match; DESIGN
// 12.13, include/mi_depth.h states the contract): the cells are the outlier removal's on both lists, a target row is a candidate
// of a source row when their cells differ by at most 1 on every axis AND (dx*dx + dy*dy) + dz*dz <= radius*radius, and the
// nearest is the candidate with the smallest 64-bit key (bits(d2) << 32) | target row: ties go to the smallest row. A selection
// on a deterministic f32 value: nothing depends on the order of arrival. Contraction is off in the whole file (Makefile); the
// float steps are outlier.hip's and pipeline.match_points restates them in numpy.
//
// The grid is built from the TARGET and sized by it; the source rows only read it. The build kernels' bodies and the 27-cell
// walk live in match_grid.h, which kernels/register.hip shares. The launches:
//   reset    table keys to all ones, per-slot count / start / fill to 0, the flags, the eight counters and `dropped`
//   insert, alloc   as in outlier.hip, over the target rows: the cell table and the start of every cell's bucket. A target row
//            that is not finite or out of range is in no bucket
//   fill     one thread per target row: the bucket entry is 16 bytes, xyz and the target row, as clusters.hip writes them
//   nearest  tiles of the source, the classify side of tile_compact.h: the cell key of the source row, the 27 cells around it
//            probed with loads only (the source row is in no bucket: no cell is "its own" and no entry is skipped), one 16-byte
//            load per candidate, the running minimum of the key in registers. nearest, dist2, the ballot bit of the mode, and
//            the counters: popcounts summed over the steps, one integer add per wave and counter at the end
//   scan, scatter   (mode 1 / 2) launch_list_compact
// No thread waits on another: every loop is bounded by the table size or a bucket size. Vector stores and integer atomics only.
#include <algorithm>
#include <cmath>

#include "match_grid.h"

namespace md {

namespace {

constexpr int kFlagWords = 64;
constexpr unsigned kNoDistance = 0x7F800000u;  // dist2 of a row without a nearest

struct MatchScratch {  // the parts of the scratch buffer, 256-byte aligned
  MatchGrid g;
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int* flags;  // [0] a probe loop ran out, [1] dropped (when the caller takes none), [2] the bucket cursor, [8..16) the counters
  size_t bytes;
};

MatchScratch carve(void* base, int n, int t) {
  const size_t nb = (size_t)tiles_of(n);
  MatchScratch s;
  Carver c(base);
  s.g = carve_match_grid(c, t);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.flags = c.take<int>(kFlagWords);
  s.bytes = c.bytes;
  return s;
}

// The four build kernels are match_grid.h's bodies with this file's flag words.
__global__ void __launch_bounds__(kTileThreads) match_reset_kernel(ulonglong2* __restrict__ keys, uint4* __restrict__ cnt, uint4* __restrict__ start,
                                                               uint4* __restrict__ fill, size_t quads, int* __restrict__ flags,
                                                               int32_t* __restrict__ stats, int32_t* __restrict__ dropped) {
  match_grid_reset(keys, cnt, start, fill, quads);
  if (blockIdx.x == 0 && threadIdx.x < 8) stats[threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = 0;
    flags[1] = 0;
    flags[2] = 0;
    if (dropped) dropped[0] = 0;
  }
}

// stats[2] counts the rows that enter the grid
__global__ void __launch_bounds__(kTileThreads) match_insert_kernel(const float* __restrict__ target, int t, float radius,
                                                                unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt,
                                                                int* __restrict__ slot, unsigned long long mask, int* __restrict__ flags,
                                                                int32_t* __restrict__ stats) {
  match_grid_insert(target, t, radius, keys, cnt, slot, mask, flags, stats + 2);
}

__global__ void __launch_bounds__(kTileThreads) match_alloc_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ start,
                                                               int* __restrict__ flags) {
  match_grid_alloc(cnt, start, flags + 2);
}

__global__ void __launch_bounds__(kTileThreads) match_fill_kernel(const float* __restrict__ target, int t, const unsigned* __restrict__ start,
                                                              unsigned* __restrict__ fill, const int* __restrict__ slot,
                                                              uint4* __restrict__ bucket, int* __restrict__ flags) {
  match_grid_fill(target, t, start, fill, slot, bucket, flags);
}

// grid tiles of the source, the classify side of tile_compact.h. The table and the buckets no longer change: loads only.
// `bucket_rows` = t bounds every bucket walk even if a count were wrong. counters: [0] in range, [1] matched, [4..8) within tol.
__global__ void __launch_bounds__(kTileThreads) match_nearest_kernel(MatchParams p, const unsigned long long* __restrict__ keys,
                                                                 const unsigned* __restrict__ cnt, const unsigned* __restrict__ start,
                                                                 const uint4* __restrict__ bucket, unsigned long long mask,
                                                                 unsigned long long* __restrict__ bits, int* __restrict__ counts,
                                                                 int32_t* __restrict__ stats, int32_t* __restrict__ dropped) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.in_count, p.B, p.n);
  const float r2 = p.radius * p.radius;
  float tol2[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) tol2[t] = p.tol[t] * p.tol[t];
  const unsigned bucket_rows = (unsigned)p.t;
  int kept = 0, n_in = 0, n_hit = 0, n_out = 0, n_tol[4] = {0, 0, 0, 0};
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool in_range = false, hit = false, row = false;
    float best_d2 = 0.f;
    if (i < live) {
      row = true;
      const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
      unsigned long long own = 0ull;
      in_range = grid_cell_key(x, y, z, p.radius, &own);
      unsigned long long best = ~0ull;
      if (in_range) best = match_grid_nearest(x, y, z, own, r2, keys, cnt, start, bucket, mask, bucket_rows);
      hit = best != ~0ull;
      best_d2 = __uint_as_float(hit ? (unsigned)(best >> 32) : kNoDistance);
      if (p.nearest) p.nearest[i] = hit ? (int32_t)(unsigned)(best & 0xFFFFFFFFull) : (in_range ? -1 : -2);
      if (p.dist2) p.dist2[i] = best_d2;
    }
    const bool keep = p.mode == 1 ? hit : (p.mode == 2 ? (in_range && !hit) : false);
    kept += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
    n_in += __popcll(__ballot(in_range));
    n_hit += __popcll(__ballot(hit));
    n_out += __popcll(__ballot(row && !in_range));
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (p.tol[t] > 0.f) n_tol[t] += __popcll(__ballot(hit && best_d2 <= tol2[t]));  // a kernel argument: the whole wave takes the branch
  }
  if (lane == 0) {  // one add per wave and counter
    if (n_in) atomicAdd(stats, n_in);
    if (n_hit) atomicAdd(stats + 1, n_hit);
    if (n_out) atomicAdd(dropped, n_out);
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (n_tol[t]) atomicAdd(stats + 4 + t, n_tol[t]);
  }
  const int sum = tile_sum(kept, wave_n);
  if (tid == 0) counts[tile] = sum;
}

}  // namespace

size_t match_scratch_bytes(int n, int t) { return carve(nullptr, n > 0 ? n : 0, t > 0 ? t : 0).bytes; }

const int32_t* match_flags(const void* scratch, int n, int t) { return carve((void*)scratch, n > 0 ? n : 0, t > 0 ? t : 0).flags; }

int launch_match_points(const MatchParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "matching needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "matching takes fewer than 2^30 rows, got %d", p.n);
  if (p.t < 0 || p.t >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "matching takes fewer than 2^30 target rows, got %d", p.t);
  if (!(p.radius > 0.f) || !std::isfinite(p.radius) || !std::isfinite(p.radius * p.radius))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: it and its square must be finite and > 0", (double)p.radius);
  for (int t = 0; t < 4; ++t)
    if (!(p.tol[t] >= 0.f) || !(p.tol[t] <= p.radius)) MD_FAIL(MD_ERR_INVALID_ARG, "tol[%d] = %g: 0 or in (0, radius]", t, (double)p.tol[t]);
  if (p.mode < 0 || p.mode > 2) MD_FAIL(MD_ERR_INVALID_ARG, "mode = %d: 0, 1 or 2", p.mode);
  if (p.t > 0 && !p.target) MD_FAIL(MD_ERR_INVALID_ARG, "target pointer is null");
  if (p.capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "matching: a negative capacity");
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "matching of %d views", p.B);
  const MatchScratch v = carve(scratch, p.n, p.t);
  const size_t slots = voxel_table_slots(p.t);
  const int nb = tiles_of(p.n);
  const size_t quads = slots / 4;
  const unsigned long long mask = (unsigned long long)(slots - 1);
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kTileThreads - 1) / kTileThreads, 256 * 32);
  int32_t* stats = p.stats ? p.stats : v.flags + kMatchStatsFlag;
  int32_t* dropped = p.dropped ? p.dropped : v.flags + 1;
  hipLaunchKernelGGL(match_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, (ulonglong2*)v.g.keys, (uint4*)v.g.cnt, (uint4*)v.g.start,
                     (uint4*)v.g.fill, quads, v.flags, stats, p.dropped);
  MD_HIP(hipGetLastError());
  if (p.t > 0) {
    const unsigned target_grid = (unsigned)((p.t + kTileThreads - 1) / kTileThreads);
    hipLaunchKernelGGL(match_insert_kernel, dim3(target_grid), dim3(kTileThreads), 0, s, p.target, p.t, p.radius, v.g.keys, v.g.cnt, v.g.slot, mask, v.flags,
                       stats);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(match_alloc_kernel, dim3((unsigned)(slots / kTileThreads)), dim3(kTileThreads), 0, s, v.g.cnt, v.g.start, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(match_fill_kernel, dim3(target_grid), dim3(kTileThreads), 0, s, p.target, p.t, v.g.start, v.g.fill, v.g.slot, v.g.bucket, v.flags);
    MD_HIP(hipGetLastError());
  }
  if (p.n > 0) {
    hipLaunchKernelGGL(match_nearest_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, v.g.keys, v.g.cnt, v.g.start, v.g.bucket, mask, v.bits, v.counts, stats,
                       dropped);
    MD_HIP(hipGetLastError());
  }
  if (p.mode == 0) return MD_OK;
  VoxelParams c;  // the compaction reads the rows, the counts and the outputs; it knows no target
  c.xyz = p.xyz; c.conf = p.conf; c.rgb = p.rgb; c.normals = p.normals; c.in_count = p.in_count; c.n = p.n; c.B = p.B;
  c.xyz_out = p.xyz_out; c.conf_out = p.conf_out; c.rgb_out = p.rgb_out; c.normals_out = p.normals_out;
  c.index = p.index; c.count = p.count; c.capacity = p.capacity;
  return launch_list_compact(c, nullptr, nullptr, v.bits, v.counts, v.offsets, s);
}

}  // namespace md
