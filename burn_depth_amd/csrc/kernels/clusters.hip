// DBSCAN / Euclidean clustering of a point list for gfx950 (md_op_cluster_points, md_infer_points_clusters; DESIGN 12.12,
// include/mi_depth.h states the contract): cells and neighbours are the outlier removal's, a core row has at least k neighbours,
// a cluster is a connected component of the core rows under the neighbour relation and is named by its smallest core row, a
// non-core row with a core neighbour takes the smallest label among them, every other in-range row is noise. Integers on a
// deterministic f32 predicate: nothing depends on the order of arrival. Contraction is off in the whole file (Makefile); the
// float steps are outlier.hip's and pipeline.cluster_points restates them in numpy.
//
// The launches:
//   reset    table keys to all ones, per-slot count / start / fill to 0, the flags, the counters and the box keys
//   insert, alloc   as in outlier.hip: the cell table and the start of every cell's bucket
//   fill     one thread per row: the bucket entry is 16 bytes, xyz and the source row, so a walk costs one 16-byte load per
//            candidate; bit 31 of the row word says "core" (n < 2^30 leaves it free) and is set here when k == 0.
//            parent[i] = i, -2 for a dropped row
//   count    (k > 0) one thread per row: the search of outlier.hip with its stop at k; a core row sets bit 31 of its own entry
//   union    one thread per core row: the 27 buckets to their ends, a hook to every core neighbour j < i (the predicate is
//            symmetric: half the edges suffice). The row's root is kept in a register and a neighbour with the same root is
//            skipped: in a dense cloud nearly every edge after the first is redundant
//   flatten  parent[i] = the root of i, with loads only on the way (components_math.h says why)
//   border   (k > 0) one thread per non-core row: the minimum of its core neighbours' labels, or -1, goes to parent[i], which no
//            other thread reads: only core rows are looked up
//   sizes    size[label] += 1 per labelled row, one add per wave when it shares the label
//   rows     tiles of the rows: label, cluster_size, the four counters, and the bits "row is the label of a kept cluster"
//   scan, rank   launch_list_compact's scan on those bits and the decimation's rank step: the dense id of every kept label
//   assign   tiles of the rows: cluster[i] through the rank of label[i], the table rows, the box keys (atomicMin / atomicMax
//            on ordered keys, one lane per wave when it shares the cluster) and, for mode 1, the bits "row of a kept cluster"
//   boxes    the keys back to floats, for the table rows that exist
//   scan, scatter   (mode 1) launch_list_compact
// No thread waits on another: every loop is bounded by the table size or a bucket size, or is the hook loop of components_math.h.
// Vector stores and integer atomics only.
#include <algorithm>
#include <cmath>

#include "components_math.h"
#include "voxel_math.h"

namespace md {

namespace {

constexpr unsigned kCoreBit = 0x80000000u;
constexpr int kFlagWords = 64;

struct ClustersScratch {  // the parts of the scratch buffer, 256-byte aligned
  unsigned long long* keys;
  unsigned* cnt;    // in-range rows of the slot's cell
  unsigned* start;  // first bucket row of the cell
  unsigned* fill;   // rows of the cell placed so far
  int* slot;        // [n] the row's slot, -1 out of range
  int* pos;         // [n] the row's bucket row
  int* parent;      // [n] the union-find; after flatten and border the label of every row
  int* size;        // [n] rows of the cluster, at its label
  int32_t* rank;    // [n] the dense id, at the label of a kept cluster
  int32_t* dense;   // [n] when the caller takes no `cluster`
  uint4* bucket;    // [n] x y z bits and the source row (bit 31: core), cell by cell
  unsigned* bkeys;  // [table_capacity,6] ordered keys of the boxes
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int32_t* total;  // [2] the scan's count words for the dense ids
  int* flags;      // [0] a probe loop ran out, [1] dropped (when the caller takes none), [2] the bucket cursor, [8..12) the counters
  size_t bytes;
};

ClustersScratch carve(void* base, int n, long cap) {
  const size_t slots = voxel_table_slots(n), nb = (size_t)tiles_of(n);
  ClustersScratch s;
  Carver c(base);
  s.keys = c.take<unsigned long long>(slots);
  s.cnt = c.take<unsigned>(slots);
  s.start = c.take<unsigned>(slots);
  s.fill = c.take<unsigned>(slots);
  s.slot = c.take<int>((size_t)n);
  s.pos = c.take<int>((size_t)n);
  s.parent = c.take<int>((size_t)n);
  s.size = c.take<int>((size_t)n);
  s.rank = c.take<int32_t>((size_t)n);
  s.dense = c.take<int32_t>((size_t)n);
  s.bucket = c.take<uint4>((size_t)n);
  s.bkeys = c.take<unsigned>((size_t)cap * 6);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.total = c.take<int32_t>(2);
  s.flags = c.take<int>(kFlagWords);
  s.bytes = c.bytes;
  return s;
}

// the usual ordered key of an f32: unsigned order of the keys = numeric order of the floats, -0 below +0
__device__ __forceinline__ unsigned ordered_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

__device__ __forceinline__ bool cluster_kept(int size, int min_points, int max_points) {
  return size >= min_points && (max_points == 0 || size <= max_points);
}

// slots is a multiple of 1024: every thread writes four slots with 16-byte stores. box_words = table_capacity * 6 or 0.
__global__ void __launch_bounds__(kTileThreads) clusters_reset_kernel(ulonglong2* __restrict__ keys, uint4* __restrict__ cnt, uint4* __restrict__ start,
                                                                  uint4* __restrict__ fill, size_t quads, unsigned* __restrict__ bkeys,
                                                                  size_t box_words, int* __restrict__ flags, int32_t* __restrict__ stats,
                                                                  int32_t* __restrict__ dropped) {
  fill_keys(keys, 2 * quads);
  const size_t stride = (size_t)gridDim.x * kTileThreads, first = (size_t)blockIdx.x * kTileThreads + threadIdx.x;
  for (size_t q = first; q < quads; q += stride) {
    cnt[q] = make_uint4(0u, 0u, 0u, 0u);
    start[q] = make_uint4(0u, 0u, 0u, 0u);
    fill[q] = make_uint4(0u, 0u, 0u, 0u);
  }
  for (size_t w = first; w < box_words; w += stride) bkeys[w] = (w % 6) < 3 ? 0xFFFFFFFFu : 0u;  // minima, then maxima
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = 0;
    flags[1] = 0;
    flags[2] = 0;
    stats[0] = 0; stats[1] = 0; stats[2] = 0; stats[3] = 0;
    if (dropped) dropped[0] = 0;
  }
}

// grid ceil(n / 256). mask = slots - 1.
__global__ void __launch_bounds__(kTileThreads) clusters_insert_kernel(ClustersParams p, unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt,
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
__global__ void __launch_bounds__(kTileThreads) clusters_alloc_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ start,
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

// grid ceil(n / 256). A bucket row at or beyond n would mean the counts changed under the launches: the flag, and the row is
// treated as dropped by every later launch (pos -1).
__global__ void __launch_bounds__(kTileThreads) clusters_fill_kernel(ClustersParams p, const unsigned* __restrict__ start, unsigned* __restrict__ fill,
                                                                 const int* __restrict__ slot, int* __restrict__ pos, uint4* __restrict__ bucket,
                                                                 int* __restrict__ parent, int* __restrict__ size, int* __restrict__ flags) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  size[i] = 0;
  const int h = slot[i];
  unsigned at = 0u;
  bool placed = h >= 0;
  if (placed) {
    at = start[h] + atomicAdd(fill + h, 1u);
    placed = at < (unsigned)p.n;
    if (!placed) flags[0] = 1;
  }
  if (!placed) {
    pos[i] = -1;
    parent[i] = -2;
    return;
  }
  const float* src = p.xyz + i * 3;
  bucket[at] = make_uint4(__float_as_uint(src[0]), __float_as_uint(src[1]), __float_as_uint(src[2]), (unsigned)i | (p.k == 0 ? kCoreBit : 0u));
  pos[i] = (int)at;
  parent[i] = (int)i;
}

struct Grid {  // the table and the buckets once they no longer change
  const unsigned long long* keys;
  const unsigned* cnt;
  const unsigned* start;
  const uint4* bucket;
  unsigned long long mask;
};

// Calls visit(row word) for every neighbour of in-range row i (slot h, bucket row self) until it returns false: the 27 cells
// around the row's (a coordinate outside the grid: skipped), each probed with loads only and walked, the row's own entry skipped
// by its position (never by its coordinates: duplicates are neighbours).
template <class F>
__device__ __forceinline__ void for_each_neighbour(const Grid& g, const float* __restrict__ xyz, long i, int h, unsigned self, float r2, F visit) {
  const float x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const unsigned long long own = g.keys[h];  // the row's cell, biased: 21 bits per axis
  const int bx = (int)(own >> 42), by = (int)((own >> 21) & 0x1FFFFFull), bz = (int)(own & 0x1FFFFFull);
  for (int c = 0; c < 27; ++c) {
    const int qx = bx + c / 9 - 1, qy = by + (c / 3) % 3 - 1, qz = bz + c % 3 - 1;
    if ((unsigned)qx >= 2u * kGridHalfInt || (unsigned)qy >= 2u * kGridHalfInt || (unsigned)qz >= 2u * kGridHalfInt) continue;
    const long s = c == 13 ? (long)h : grid_find(g.keys, g.mask, grid_key(qx, qy, qz));
    if (s < 0) continue;
    const unsigned first = g.start[s], last = first + g.cnt[s];
    for (unsigned at = first; at < last; ++at) {
      if (at == self) continue;  // the row's own entry, exactly once
      const uint4 e = g.bucket[at];
      const float dx = __uint_as_float(e.x) - x, dy = __uint_as_float(e.y) - y, dz = __uint_as_float(e.z) - z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= r2 && !visit(e.w)) return;
    }
  }
}

// grid ceil(n / 256), k > 0. The only store is the row word of the thread's own entry. Other threads of this launch load that
// entry whole, 16 bytes, while the store may be in flight: they use its xyz, which nobody writes, and the visitor here ignores
// the row word, so either value of it gives the same count. The row word is read for its meaning only in later launches.
__global__ void __launch_bounds__(kTileThreads) clusters_count_kernel(ClustersParams p, Grid g, const int* __restrict__ slot, const int* __restrict__ pos,
                                                                  unsigned* row_words) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const int at = pos[i];
  if (at < 0) return;
  const int k = p.k;
  int n = 0;
  for_each_neighbour(g, p.xyz, i, slot[i], (unsigned)at, p.radius * p.radius, [&](unsigned) { return ++n < k; });
  if (n >= k) row_words[(size_t)at * 4 + 3] = (unsigned)i | kCoreBit;
}

// grid ceil(n / 256)
__global__ void __launch_bounds__(kTileThreads) clusters_union_kernel(ClustersParams p, Grid g, const int* __restrict__ slot, const int* __restrict__ pos,
                                                                  int* parent) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const int at = pos[i];
  if (at < 0 || !(g.bucket[at].w & kCoreBit)) return;
  int root = (int)i;  // of row i at some moment: a stale one only costs a hook that finds nothing to do
  for_each_neighbour(g, p.xyz, i, slot[i], (unsigned)at, p.radius * p.radius, [&](unsigned w) {
    const int j = (int)(w & ~kCoreBit);
    if (!(w & kCoreBit) || j > (int)i) return true;
    if (components_find<DeviceAtomics>(parent, j) == root) return true;  // j's root was once i's: one tree already
    components_hook<DeviceAtomics>(parent, (int)i, j);
    root = components_find<DeviceAtomics>(parent, (int)i);
    return true;
  });
}

// grid ceil(n / 256). In place, while other threads of this launch walk the same chains: the only stores are roots.
__global__ void __launch_bounds__(kTileThreads) clusters_flatten_kernel(ClustersParams p, int* parent) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  if (DeviceAtomics::load(parent + i) < 0) return;  // dropped
  DeviceAtomics::store(parent + i, components_root<DeviceAtomics>(parent, (int)i));
}

// grid ceil(n / 256), k > 0. Reads parent[] of core rows, writes parent[] of non-core rows: no word is both read and written.
__global__ void __launch_bounds__(kTileThreads) clusters_border_kernel(ClustersParams p, Grid g, const int* __restrict__ slot, const int* __restrict__ pos,
                                                                   int* parent) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const int at = pos[i];
  if (at < 0 || (g.bucket[at].w & kCoreBit)) return;
  int best = 0x7FFFFFFF;
  for_each_neighbour(g, p.xyz, i, slot[i], (unsigned)at, p.radius * p.radius, [&](unsigned w) {
    if (w & kCoreBit) best = min(best, parent[w & ~kCoreBit]);
    return true;
  });
  parent[i] = best == 0x7FFFFFFF ? -1 : best;
}

// grid ceil(n / 256); no thread leaves before the ballots
__global__ void __launch_bounds__(kTileThreads) clusters_size_kernel(ClustersParams p, const int* __restrict__ label, int* __restrict__ size) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int l = -1;
  if (i < live_count(p.in_count, p.B, p.n)) l = label[i];
  const bool valid = l >= 0;
  const unsigned long long act = __ballot(valid);
  if (!act) return;  // the whole wave
  const int leader = __ffsll((long long)act) - 1;
  const int first = __shfl(l, leader, 64);
  const unsigned long long same = __ballot(valid && l == first);
  if (same == act) {
    if (lane == leader) atomicAdd(size + first, (int)__popcll(act));
  } else if (valid) {
    atomicAdd(size + l, 1);
  }
}

// grid tiles of the rows
__global__ void __launch_bounds__(kTileThreads) clusters_rows_kernel(ClustersParams p, const int* __restrict__ label, const int* __restrict__ size,
                                                                 unsigned long long* __restrict__ bits, int* __restrict__ counts,
                                                                 int32_t* __restrict__ stats) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.in_count, p.B, p.n);
  int n = 0, found = 0, noise = 0, rows = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool root = false, keep = false, lone = false;
    if (i < live) {
      const int l = label[i];
      const int sz = l >= 0 ? size[l] : 0;
      keep = cluster_kept(sz, p.min_points, p.max_points);  // min_points >= 1: never for size 0
      root = l == (int)i;
      lone = l == -1;
      if (p.label) p.label[i] = l;
      if (p.cluster_size) p.cluster_size[i] = sz;
    }
    n += ballot_step(root && keep, bits + (long)tile * kTileWords + tile_word(s));
    found += __popcll(__ballot(root));
    noise += __popcll(__ballot(lone));
    rows += __popcll(__ballot(keep));
  }
  if (lane == 0) {
    if (found) atomicAdd(stats, found);
    if (n) atomicAdd(stats + 1, n);
    if (noise) atomicAdd(stats + 2, noise);
    if (rows) atomicAdd(stats + 3, rows);
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

// the minimum (kMin) or maximum over the wave's lanes
template <bool kMin>
__device__ __forceinline__ unsigned wave_extreme(unsigned v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, d, 64);
    v = kMin ? min(v, o) : max(v, o);
  }
  return v;
}

// grid tiles of the rows. rank[l] is read only at the labels of kept clusters, where the rank step wrote it. The bits of the
// rows kernel are used up by then: this launch writes the bits of mode 1 over them.
__global__ void __launch_bounds__(kTileThreads) clusters_assign_kernel(ClustersParams p, const int* __restrict__ label, const int* __restrict__ size,
                                                                   const int32_t* __restrict__ rank, unsigned* __restrict__ bkeys,
                                                                   unsigned long long* __restrict__ bits, int* __restrict__ counts) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.in_count, p.B, p.n);
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    int id = -1;
    if (i < live) {
      const int l = label[i];
      if (l >= 0) {
        const int sz = size[l];
        if (cluster_kept(sz, p.min_points, p.max_points)) {
          id = rank[l];
          if (l == (int)i && id < p.table_capacity) {
            if (p.table_label) p.table_label[id] = l;
            if (p.table_size) p.table_size[id] = sz;
          }
        }
      } else if (l == -2) {
        id = -2;
      }
      if (p.cluster) p.cluster[i] = id;
    }
    n += ballot_step(id >= 0, bits + (long)tile * kTileWords + tile_word(s));
    if (!p.box) continue;
    const bool boxed = id >= 0 && id < p.table_capacity;
    const unsigned long long act = __ballot(boxed);
    if (!act) continue;  // the whole wave
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (boxed) {
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = hi[a] = ordered_key(p.xyz[i * 3 + a]);
    }
    const int leader = __ffsll((long long)act) - 1;
    const int first = __shfl(id, leader, 64);
    unsigned* dst = bkeys + (size_t)(boxed ? id : 0) * 6;
    if (__ballot(boxed && id == first) == act) {  // a floor-sized cluster would otherwise serialise on six words
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = wave_extreme<true>(lo[a]);
        hi[a] = wave_extreme<false>(hi[a]);
      }
      if (lane != leader) continue;
    } else if (!boxed) {
      continue;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(dst + a, lo[a]);
      atomicMax(dst + 3 + a, hi[a]);
    }
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

// grid ceil(table_capacity * 6 / 256): the table rows that exist, min(kept, table_capacity)
__global__ void __launch_bounds__(kTileThreads) clusters_box_kernel(ClustersParams p, const unsigned* __restrict__ bkeys, const int32_t* __restrict__ stats) {
  const long w = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (w >= p.table_capacity * 6 || w / 6 >= stats[1]) return;
  p.box[w] = ordered_value(bkeys[w]);
}

}  // namespace

size_t clusters_scratch_bytes(int n, long table_capacity) { return carve(nullptr, n > 0 ? n : 0, table_capacity > 0 ? table_capacity : 0).bytes; }

const int32_t* clusters_flags(const void* scratch, int n, long table_capacity) {
  return carve((void*)scratch, n > 0 ? n : 0, table_capacity > 0 ? table_capacity : 0).flags;
}

int launch_cluster_points(const ClustersParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "clustering needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "clustering takes fewer than 2^30 rows, got %d", p.n);
  if (!(p.radius > 0.f) || !std::isfinite(p.radius)) MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: must be finite and > 0", (double)p.radius);
  if (p.k < 0 || p.k > kClusterMaxNeighbours) MD_FAIL(MD_ERR_INVALID_ARG, "min_neighbours %d outside 0..%d", p.k, kClusterMaxNeighbours);
  if (p.min_points < 1 || p.max_points < 0 || (p.max_points > 0 && p.max_points < p.min_points))
    MD_FAIL(MD_ERR_INVALID_ARG, "min_points %d / max_points %d: 1 <= min_points, and max_points 0 or >= min_points", p.min_points, p.max_points);
  if (p.mode < 0 || p.mode > 1) MD_FAIL(MD_ERR_INVALID_ARG, "mode = %d: 0 or 1", p.mode);
  if (p.table_capacity < 0 || p.capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "clustering: a negative capacity");
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "clustering of %d views", p.B);
  const ClustersScratch v = carve(scratch, p.n, p.table_capacity);
  const size_t slots = voxel_table_slots(p.n);
  const int nb = tiles_of(p.n);
  const size_t quads = slots / 4, box_words = p.box ? (size_t)p.table_capacity * 6 : 0;
  const unsigned long long mask = (unsigned long long)(slots - 1);
  const unsigned reset_grid = (unsigned)std::min<size_t>((std::max(quads, box_words) + kTileThreads - 1) / kTileThreads, 256 * 32);
  int32_t* stats = p.stats ? p.stats : v.flags + kClusterStatsFlag;
  int32_t* dense = p.cluster ? p.cluster : v.dense;
  hipLaunchKernelGGL(clusters_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, (ulonglong2*)v.keys, (uint4*)v.cnt, (uint4*)v.start,
                     (uint4*)v.fill, quads, v.bkeys, box_words, v.flags, stats, p.dropped);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    const unsigned rows_grid = (unsigned)((p.n + kTileThreads - 1) / kTileThreads);
    const Grid g{v.keys, v.cnt, v.start, v.bucket, mask};
    ClustersParams q = p;  // the assign kernel always leaves the dense id somewhere: mode 1 needs no second pass over it
    q.cluster = dense;
    hipLaunchKernelGGL(clusters_insert_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.keys, v.cnt, v.slot, mask, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(clusters_alloc_kernel, dim3((unsigned)(slots / kTileThreads)), dim3(kTileThreads), 0, s, v.cnt, v.start, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(clusters_fill_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.start, v.fill, v.slot, v.pos, v.bucket, v.parent, v.size,
                       v.flags);
    MD_HIP(hipGetLastError());
    if (p.k > 0) {
      hipLaunchKernelGGL(clusters_count_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, g, v.slot, v.pos, (unsigned*)v.bucket);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(clusters_union_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, g, v.slot, v.pos, v.parent);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(clusters_flatten_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.parent);
    MD_HIP(hipGetLastError());
    if (p.k > 0) {
      hipLaunchKernelGGL(clusters_border_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, g, v.slot, v.pos, v.parent);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(clusters_size_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, v.parent, v.size);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(clusters_rows_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, v.parent, v.size, v.bits, v.counts, stats);
    MD_HIP(hipGetLastError());
    VoxelParams ids;  // the scan alone: the tile offsets of the kept labels
    ids.n = p.n; ids.count = v.total;
    MD_TRY(launch_list_compact(ids, nullptr, nullptr, v.bits, v.counts, v.offsets, s));
    MD_TRY(launch_rank_rows(v.bits, v.offsets, p.n, v.rank, s));
    hipLaunchKernelGGL(clusters_assign_kernel, dim3(nb), dim3(kTileThreads), 0, s, q, v.parent, v.size, v.rank, v.bkeys, v.bits, v.counts);
    MD_HIP(hipGetLastError());
    if (box_words) {
      hipLaunchKernelGGL(clusters_box_kernel, dim3((unsigned)((box_words + kTileThreads - 1) / kTileThreads)), dim3(kTileThreads), 0, s, p, v.bkeys, stats);
      MD_HIP(hipGetLastError());
    }
  }
  if (p.mode == 0) return MD_OK;
  VoxelParams c;  // the compaction reads the rows, the counts and the outputs; it knows no cluster
  c.xyz = p.xyz; c.conf = p.conf; c.rgb = p.rgb; c.normals = p.normals; c.in_count = p.in_count; c.n = p.n; c.B = p.B;
  c.xyz_out = p.xyz_out; c.conf_out = p.conf_out; c.rgb_out = p.rgb_out; c.normals_out = p.normals_out;
  c.index = p.index; c.count = p.count; c.capacity = p.capacity;
  return launch_list_compact(c, nullptr, nullptr, v.bits, v.counts, v.offsets, s);
}

}  // namespace md
