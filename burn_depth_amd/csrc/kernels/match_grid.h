// What the kernels that search a reference cloud share (kernels/match.hip, kernels/register.hip): the cell grid built from the
// TARGET and the 27-cell walk of a source row through it. The grid is the clustering's: the outlier removal's cell table and,
// cell by cell, 16-byte bucket entries (x y z bits and the target row). The bodies below are the four build kernels of
// DESIGN 12.13 and the walk of its nearest kernel; a file wraps them in launches of its own. The files that include this compile
// with contraction off (Makefile). No thread waits on another: every loop is bounded by the table size or a bucket size.
#pragma once

#include "voxel_math.h"

namespace md {

struct MatchGrid {  // the grid's parts of a scratch buffer, 256-byte aligned
  unsigned long long* keys;
  unsigned* cnt;    // target rows of the slot's cell
  unsigned* start;  // first bucket row of the cell
  unsigned* fill;   // rows of the cell placed so far
  int* slot;        // [t] the target row's slot, -1 not in the grid
  uint4* bucket;    // [t] x y z bits and the target row, cell by cell
};

inline MatchGrid carve_match_grid(Carver& c, int t) {
  const size_t slots = voxel_table_slots(t);
  MatchGrid g;
  g.keys = c.take<unsigned long long>(slots);
  g.cnt = c.take<unsigned>(slots);
  g.start = c.take<unsigned>(slots);
  g.fill = c.take<unsigned>(slots);
  g.slot = c.take<int>((size_t)t);
  g.bucket = c.take<uint4>((size_t)t);
  return g;
}

// reset: table keys to all ones, per-slot count / start / fill to 0. slots is a multiple of 1024: every thread writes four
// slots with 16-byte stores; quads = slots / 4. Any grid of kTileThreads.
__device__ __forceinline__ void match_grid_reset(ulonglong2* __restrict__ keys, uint4* __restrict__ cnt, uint4* __restrict__ start,
                                                 uint4* __restrict__ fill, size_t quads) {
  fill_keys(keys, 2 * quads);
  const size_t stride = (size_t)gridDim.x * kTileThreads;
  for (size_t q = (size_t)blockIdx.x * kTileThreads + threadIdx.x; q < quads; q += stride) {
    cnt[q] = make_uint4(0u, 0u, 0u, 0u);
    start[q] = make_uint4(0u, 0u, 0u, 0u);
    fill[q] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// insert: grid ceil(t / 256) over the target rows. mask = slots - 1. *in_grid counts the rows that enter the grid; *ran_out is
// set when every slot holds another key (cannot happen at load <= 0.5). The last statement of its kernel: lanes leave early.
__device__ __forceinline__ void match_grid_insert(const float* __restrict__ target, int t, float radius, unsigned long long* __restrict__ keys,
                                                  unsigned* __restrict__ cnt, int* __restrict__ slot, unsigned long long mask,
                                                  int* __restrict__ ran_out, int32_t* __restrict__ in_grid) {
  const long j = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (j >= t) return;
  const float x = target[j * 3], y = target[j * 3 + 1], z = target[j * 3 + 2];
  unsigned long long key = 0ull;
  const bool in_range = grid_cell_key(x, y, z, radius, &key);
  long h = -1;
  if (in_range) {
    h = grid_claim(keys, mask, key);
    if (h < 0) *ran_out = 1;
  }
  wave_count_add(h >= 0, in_grid);  // lanes have already left: the first active one adds
  if (h >= 0) atomicAdd(cnt + h, 1u);
  slot[j] = (int)h;
}

// alloc: grid slots / 256 (slots is a multiple of 1024: every wave is full). The buckets of a wave's 64 slots lie behind one
// another; *cursor is the next free bucket row.
__device__ __forceinline__ void match_grid_alloc(const unsigned* __restrict__ cnt, unsigned* __restrict__ start, int* __restrict__ cursor) {
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
  if (lane == 0) base = (unsigned)atomicAdd(cursor, (int)total);
  base = __shfl(base, 0, 64);
  if (c) start[h] = base + (incl - c);
}

// fill: grid ceil(t / 256). A bucket row at or beyond t would mean the counts changed under the launches: *ran_out, and the row
// is in no bucket (the cell's count then names a row nobody wrote, so the call is refused by its flag).
__device__ __forceinline__ void match_grid_fill(const float* __restrict__ target, int t, const unsigned* __restrict__ start,
                                                unsigned* __restrict__ fill, const int* __restrict__ slot, uint4* __restrict__ bucket,
                                                int* __restrict__ ran_out) {
  const long j = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (j >= t) return;
  const int h = slot[j];
  if (h < 0) return;
  const unsigned at = start[h] + atomicAdd(fill + h, 1u);
  if (at >= (unsigned)t) {
    *ran_out = 1;
    return;
  }
  const float* src = target + j * 3;
  bucket[at] = make_uint4(__float_as_uint(src[0]), __float_as_uint(src[1]), __float_as_uint(src[2]), (unsigned)j);
}

// The walk of an in-range source row x y z with the cell key `own`: the 27 cells around it probed with loads only (the source
// row is in no bucket: no cell is "its own" and no entry is skipped), one 16-byte load per candidate, the running minimum of
// (bits(d2) << 32) | target row over the candidates with d2 <= r2. -> that minimum, all ones without a candidate. The table and
// the buckets no longer change. `bucket_rows` = t bounds every bucket walk even if a count were wrong.
__device__ __forceinline__ unsigned long long match_grid_nearest(float x, float y, float z, unsigned long long own, float r2,
                                                                 const unsigned long long* __restrict__ keys, const unsigned* __restrict__ cnt,
                                                                 const unsigned* __restrict__ start, const uint4* __restrict__ bucket,
                                                                 unsigned long long mask, unsigned bucket_rows) {
  unsigned long long best = ~0ull;
  const int bx = (int)(own >> 42), by = (int)((own >> 21) & 0x1FFFFFull), bz = (int)(own & 0x1FFFFFull);
  for (int c = 0; c < 27; ++c) {
    const int qx = bx + c / 9 - 1, qy = by + (c / 3) % 3 - 1, qz = bz + c % 3 - 1;
    if ((unsigned)qx >= 2u * kGridHalfInt || (unsigned)qy >= 2u * kGridHalfInt || (unsigned)qz >= 2u * kGridHalfInt) continue;
    const long g = grid_find(keys, mask, grid_key(qx, qy, qz));
    if (g < 0) continue;
    const unsigned first = start[g];
    unsigned last = first + cnt[g];
    last = last < bucket_rows ? last : bucket_rows;
    for (unsigned at = first; at < last; ++at) {
      const uint4 e = bucket[at];
      const float dx = __uint_as_float(e.x) - x, dy = __uint_as_float(e.y) - y, dz = __uint_as_float(e.z) - z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= r2) {  // d2 >= +0 and not NaN: the bit order is the numeric order
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)e.w;
        best = key < best ? key : best;
      }
    }
  }
  return best;
}

}  // namespace md
