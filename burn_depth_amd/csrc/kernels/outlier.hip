// Radius outlier removal of a point list for gfx950 (md_op_radius_outliers, md_infer_points_outlier; DESIGN 12.7, include/mi_depth.h
// states the contract): a row survives when at least k other rows lie within `radius` of it AND in the 27 cells around its own;
// the survivors keep the input order. Selection only: the decision is an integer count of an f32 predicate. Contraction is off in
// the whole file (Makefile); the float steps, floorf(p / radius) and (dx*dx + dy*dy) + dz*dz <= radius*radius, are what
// pipeline.radius_outliers restates in numpy.
//
// Voxel thinning's table (voxel_math.h) knows how many points a cell holds; here it is extended to cell buckets that also know
// which ones. Seven launches:
//   reset    table keys to all ones, per-slot count / start / fill to 0, the cursor, the flags and the dropped counter to 0
//   insert   one thread per row: the cell key, linear probing (atomicCAS on an empty slot only), an integer atomicAdd on the slot's
//            count; the row's slot (or -1) is recorded
//   alloc    one thread per slot: start = atomicAdd(cursor, count), one atomic per wave on the wave's prefix sums. The order of the
//            buckets follows the order of arrival: it is layout and reaches no output
//   fill     one thread per row: pos = start[slot] + atomicAdd(fill[slot], 1); the row's xyz goes to bucket row pos, pos is
//            recorded. The search then reads contiguous positions instead of gathering through an index
//   search   one thread per row: the 27 keys around the row's cell (a coordinate outside the grid: skipped), each probed with loads
//            only; the bucket is walked, the row's own entry skipped by its position (never by its coordinates: duplicates count),
//            and the walk stops at k. neighbours[i], one 64-bit ballot word per wave and step, one count per workgroup
//   scan, scatter   voxel thinning's order-preserving compaction on those words (launch_list_compact)
// No thread waits on another: every loop is bounded by the table size or a bucket size. Vector stores and integer atomics only.
#include <algorithm>
#include <cmath>

#include "voxel_math.h"

namespace md {

namespace {

struct OutlierScratch {  // the parts of the scratch buffer, 256-byte aligned
  unsigned long long* keys;
  unsigned* cnt;    // in-range rows of the slot's cell
  unsigned* start;  // first bucket row of the cell
  unsigned* fill;   // rows of the cell placed so far
  int* slot;        // [n] the row's slot, -1 out of range
  int* pos;         // [n] the row's bucket row
  float* bucket;    // [n,3] the in-range positions, cell by cell
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int* flags;  // [0] a probe loop ran out, [1] dropped (when the caller takes none), [2] the bucket cursor
  size_t bytes;
};

OutlierScratch carve(void* base, int n) {
  const size_t slots = voxel_table_slots(n), nb = (size_t)tiles_of(n);
  OutlierScratch s;
  Carver c(base);
  s.keys = c.take<unsigned long long>(slots);
  s.cnt = c.take<unsigned>(slots);
  s.start = c.take<unsigned>(slots);
  s.fill = c.take<unsigned>(slots);
  s.slot = c.take<int>((size_t)n);
  s.pos = c.take<int>((size_t)n);
  s.bucket = c.take<float>((size_t)n * 3);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.flags = c.take<int>(64);
  s.bytes = c.bytes;
  return s;
}

// slots is a multiple of 1024: every thread writes four slots with 16-byte stores
__global__ void __launch_bounds__(kTileThreads) outlier_reset_kernel(ulonglong2* __restrict__ keys, uint4* __restrict__ cnt, uint4* __restrict__ start,
                                                                 uint4* __restrict__ fill, size_t quads, int* __restrict__ flags,
                                                                 int32_t* __restrict__ dropped) {
  fill_keys(keys, 2 * quads);
  const size_t stride = (size_t)gridDim.x * kTileThreads;
  for (size_t q = (size_t)blockIdx.x * kTileThreads + threadIdx.x; q < quads; q += stride) {
    cnt[q] = make_uint4(0u, 0u, 0u, 0u);
    start[q] = make_uint4(0u, 0u, 0u, 0u);
    fill[q] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = 0;
    flags[1] = 0;
    flags[2] = 0;
    if (dropped) dropped[0] = 0;
  }
}

// grid ceil(n / 256). mask = slots - 1.
__global__ void __launch_bounds__(kTileThreads) outlier_insert_kernel(OutlierParams p, unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt,
                                                                  int* __restrict__ slot, unsigned long long mask, int* __restrict__ flags) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
  unsigned long long key = 0ull;
  const bool in_range = grid_cell_key(x, y, z, p.radius, &key);
  wave_count_add(!in_range, p.dropped ? p.dropped : flags + 1);  // lanes have already left: the first active one adds
  if (!in_range) {
    slot[i] = -1;
    return;
  }
  const long h = grid_claim(keys, mask, key);
  if (h < 0) {
    flags[0] = 1;  // every slot holds another key: cannot happen at load <= 0.5
    slot[i] = -1;
    return;
  }
  atomicAdd(cnt + h, 1u);
  slot[i] = (int)h;
}

// grid slots / 256 (slots is a multiple of 1024: every wave is full). The buckets of a wave's 64 slots lie behind one another.
__global__ void __launch_bounds__(kTileThreads) outlier_alloc_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ start,
                                                                 int* __restrict__ flags) {
  const size_t h = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned c = cnt[h];
  unsigned incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  const unsigned total = __shfl(incl, 63, 64);
  if (total == 0u) return;  // the whole wave
  unsigned base = 0u;
  if (lane == 0) base = (unsigned)atomicAdd(flags + 2, (int)total);
  base = __shfl(base, 0, 64);
  if (c) start[h] = base + (incl - c);
}

// grid ceil(n / 256). The in-range rows are at most n, so is every bucket row; a row beyond that would mean the counts changed
// under the launches and raises the flag instead of being written.
__global__ void __launch_bounds__(kTileThreads) outlier_fill_kernel(OutlierParams p, const unsigned* __restrict__ start, unsigned* __restrict__ fill,
                                                                const int* __restrict__ slot, int* __restrict__ pos, float* __restrict__ bucket,
                                                                int* __restrict__ flags) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const int h = slot[i];
  if (h < 0) return;
  const unsigned at = start[h] + atomicAdd(fill + h, 1u);
  if (at >= (unsigned)p.n) {
    flags[0] = 1;
    pos[i] = -1;
    return;
  }
  const float* src = p.xyz + i * 3;
  float* dst = bucket + (size_t)at * 3;
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
  pos[i] = (int)at;
}

// grid tiles, the classify side of tile_compact.h. The table and the buckets no longer change: loads only.
__global__ void __launch_bounds__(kTileThreads) outlier_search_kernel(OutlierParams p, const unsigned long long* __restrict__ keys,
                                                                  const unsigned* __restrict__ cnt, const unsigned* __restrict__ start,
                                                                  const int* __restrict__ slot, const int* __restrict__ pos,
                                                                  const float* __restrict__ bucket, unsigned long long mask,
                                                                  unsigned long long* __restrict__ bits, int* __restrict__ counts) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int live = live_count(p.in_count, p.B, p.n);
  const float r2 = p.radius * p.radius;
  const int k = p.k;
  int kept = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool keep = false;
    if (i < live) {
      const int h = slot[i];
      int n = -1;
      if (h >= 0) {
        n = 0;
        const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
        const unsigned long long own = keys[h];  // the row's cell, biased: 21 bits per axis
        const int bx = (int)(own >> 42), by = (int)((own >> 21) & 0x1FFFFFull), bz = (int)(own & 0x1FFFFFull);
        const unsigned self = (unsigned)pos[i];
        for (int c = 0; c < 27 && n < k; ++c) {
          const int qx = bx + c / 9 - 1, qy = by + (c / 3) % 3 - 1, qz = bz + c % 3 - 1;
          if ((unsigned)qx >= 2u * kGridHalfInt || (unsigned)qy >= 2u * kGridHalfInt || (unsigned)qz >= 2u * kGridHalfInt) continue;
          const long g = c == 13 ? (long)h : grid_find(keys, mask, grid_key(qx, qy, qz));
          if (g < 0) continue;
          const unsigned first = start[g], last = first + cnt[g];
          for (unsigned at = first; at < last && n < k; ++at) {
            if (at == self) continue;  // the row's own entry, exactly once
            const float* q = bucket + (size_t)at * 3;
            const float dx = q[0] - x, dy = q[1] - y, dz = q[2] - z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= r2) ++n;
          }
        }
        keep = n == k;
      }
      if (p.neighbours) p.neighbours[i] = n;
    }
    kept += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
  }
  const int sum = tile_sum(kept, wave_n);
  if (tid == 0) counts[tile] = sum;
}

}  // namespace

size_t outlier_scratch_bytes(int n) { return carve(nullptr, n > 0 ? n : 0).bytes; }

const int32_t* outlier_flags(const void* scratch, int n) { return carve((void*)scratch, n > 0 ? n : 0).flags; }

int launch_radius_outliers(const OutlierParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "outlier removal needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "outlier removal takes fewer than 2^30 rows, got %d", p.n);
  if (!(p.radius > 0.f) || !std::isfinite(p.radius)) MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: must be finite and > 0", (double)p.radius);
  if (p.k < 1 || p.k > kOutlierMaxNeighbours) MD_FAIL(MD_ERR_INVALID_ARG, "min_neighbours %d outside 1..%d", p.k, kOutlierMaxNeighbours);
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "outlier removal of %d views", p.B);
  const OutlierScratch v = carve(scratch, p.n);
  const size_t slots = voxel_table_slots(p.n);
  const int nb = tiles_of(p.n);
  const size_t quads = slots / 4;
  const unsigned long long mask = (unsigned long long)(slots - 1);
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kTileThreads - 1) / kTileThreads, 256 * 32);
  hipLaunchKernelGGL(outlier_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, (ulonglong2*)v.keys, (uint4*)v.cnt, (uint4*)v.start,
                     (uint4*)v.fill, quads, v.flags, p.dropped);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    const unsigned rows_grid = (unsigned)((p.n + kTileThreads - 1) / kTileThreads);
    hipLaunchKernelGGL(outlier_insert_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.keys, v.cnt, v.slot, mask, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(outlier_alloc_kernel, dim3((unsigned)(slots / kTileThreads)), dim3(kTileThreads), 0, s, v.cnt, v.start, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(outlier_fill_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.start, v.fill, v.slot, v.pos, v.bucket, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(outlier_search_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, v.keys, v.cnt, v.start, v.slot, v.pos, v.bucket, mask, v.bits,
                       v.counts);
    MD_HIP(hipGetLastError());
  }
  VoxelParams c;  // the compaction reads the rows, the counts and the outputs; it knows no voxel
  c.xyz = p.xyz; c.conf = p.conf; c.rgb = p.rgb; c.normals = p.normals; c.in_count = p.in_count; c.n = p.n; c.B = p.B;
  c.xyz_out = p.xyz_out; c.conf_out = p.conf_out; c.rgb_out = p.rgb_out; c.normals_out = p.normals_out;
  c.index = p.index; c.count = p.count; c.capacity = p.capacity;
  return launch_list_compact(c, nullptr, nullptr, v.bits, v.counts, v.offsets, s);
}

}  // namespace md
