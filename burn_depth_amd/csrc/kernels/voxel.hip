// Voxel thinning of a point list for gfx950 (md_op_voxel_thin, md_infer_points_voxel; DESIGN 12.3, include/mi_depth.h states
// the contract): one input row survives per occupied voxel, chosen by a rule that does not depend on the order of arrival, and
// the survivors keep the input order. Selection only: no float is summed. Contraction is off in the whole file (Makefile); the
// one float step, floorf(p / voxel), is what pipeline.voxel_thin restates in numpy.
//
// Five launches, all HBM-bound:
//   reset    table keys to all ones, rank and count words to 0, the flags and the dropped counter to 0
//   insert   one thread per row: the cell key, linear probing over the power-of-two table (atomicCAS on the key), then on the
//            slot atomicMax of (bits(w) << 32) | (0xFFFFFFFF - i) and an integer atomicAdd; the row's slot (or -1) is recorded
//   select   keep[i] = the low word of the slot's rank names i; one 64-bit ballot word per wave and step, one count per workgroup
//   scan     one workgroup: exclusive offsets of the workgroup counts; the survivors of every view from the ballot words at
//            the view boundaries of the input (the unthinned count[] prefix)
//   scatter  output row = offset + popcounts below; copies the rows, index and weight
// select, scan and scatter are tile_compact.h's ordered compaction over a one-dimensional grid of tiles; decimate.hip and
// components.hip read the words and offsets it leaves. No thread waits on another: a probe claims a slot, finds its key or moves on, and the loop
// is bounded by the table size.
#include <algorithm>
#include <cmath>

#include "voxel_math.h"

namespace md {

namespace {

// the cell key and the probe are shared with the outlier removal (voxel_math.h)

struct VoxelScratch {  // the parts of the scratch buffer, 256-byte aligned
  unsigned long long* keys;
  unsigned long long* rank;
  unsigned* cnt;
  int* slot;
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int* flags;  // [0] the probe loop ran out, [1] dropped (when the caller takes none)
  size_t bytes;
};

VoxelScratch carve(void* base, int n) {
  const size_t slots = voxel_table_slots(n), nb = (size_t)tiles_of(n);
  VoxelScratch s;
  Carver c(base);
  s.keys = c.take<unsigned long long>(slots);
  s.rank = c.take<unsigned long long>(slots);
  s.cnt = c.take<unsigned>(slots);
  s.slot = c.take<int>((size_t)n);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.flags = c.take<int>(64);
  s.bytes = c.bytes;
  return s;
}

// slots is a multiple of 1024: every thread writes four slots with 16-byte stores
__global__ void __launch_bounds__(kTileThreads) voxel_reset_kernel(ulonglong2* __restrict__ keys, ulonglong2* __restrict__ rank,
                                                               uint4* __restrict__ cnt, size_t quads, int* __restrict__ flags,
                                                               int32_t* __restrict__ dropped) {
  fill_keys(keys, 2 * quads);
  const size_t stride = (size_t)gridDim.x * kTileThreads;
  for (size_t q = (size_t)blockIdx.x * kTileThreads + threadIdx.x; q < quads; q += stride) {
    rank[2 * q] = make_ulonglong2(0ull, 0ull);
    rank[2 * q + 1] = make_ulonglong2(0ull, 0ull);
    cnt[q] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = 0;
    flags[1] = 0;
    if (dropped) dropped[0] = 0;
  }
}

// grid ceil(n / 256). mask = slots - 1.
__global__ void __launch_bounds__(kTileThreads) voxel_insert_kernel(VoxelParams p, unsigned long long* __restrict__ keys,
                                                                unsigned long long* __restrict__ rank, unsigned* __restrict__ cnt,
                                                                int* __restrict__ slot, unsigned long long mask, int* __restrict__ flags) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
  unsigned long long key = 0ull;
  const bool in_range = grid_cell_key(x, y, z, p.voxel, &key);
  wave_count_add(!in_range, p.dropped ? p.dropped : flags + 1);  // lanes have already left: the first active one adds
  if (!in_range) {
    slot[i] = -1;
    return;
  }
  unsigned wbits = 0u;
  if (p.conf) {
    const float c = p.conf[i];
    if (isfinite(c) && c >= 0.f) wbits = __float_as_uint(c);
    if (wbits == 0x80000000u) wbits = 0u;  // -0 counts as +0
  }
  const unsigned long long word = ((unsigned long long)wbits << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
  const long h = grid_claim(keys, mask, key);
  if (h < 0) {
    flags[0] = 1;  // every slot holds another key: cannot happen at load <= 0.5
    slot[i] = -1;
    return;
  }
  atomicMax(rank + h, word);
  atomicAdd(cnt + h, 1u);
  slot[i] = (int)h;
}

// grid tiles. A row is kept when its slot's rank word names it.
__global__ void __launch_bounds__(kTileThreads) voxel_select_kernel(VoxelParams p, const unsigned long long* __restrict__ rank,
                                                                const int* __restrict__ slot, unsigned long long* __restrict__ bits,
                                                                int* __restrict__ counts) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x;
  const int live = live_count(p.in_count, p.B, p.n);
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool keep = false;
    if (i < live) {
      const int h = slot[i];
      if (h >= 0) keep = (0xFFFFFFFFu - (unsigned)rank[h]) == (unsigned)i;
    }
    n += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

// one workgroup: offsets[i] = sum of counts[0 .. i), offsets[nb] = the total (scan_tile_counts, the scan of points_scan_kernel);
// then count[b] = the survivors among the rows of view b, count[B] = the total
__global__ void __launch_bounds__(kTileThreads) voxel_scan_kernel(VoxelParams p, const int* __restrict__ counts, int nb,
                                                              const unsigned long long* __restrict__ bits, int* __restrict__ offsets) {
  __shared__ int part[kTileThreads];
  const int tid = threadIdx.x;
  scan_tile_counts(counts, nb, offsets, part);
  if (!p.count) return;
  const int live = live_count(p.in_count, p.B, p.n);
  for (int b = tid; b < p.B; b += kTileThreads) {
    long first = 0;  // rows of the views before b
    if (p.in_count)
      for (int k = 0; k < b; ++k) first += p.in_count[k];
    long last = p.in_count ? first + p.in_count[b] : live;
    first = first < 0 ? 0 : (first < live ? first : live);
    last = last < first ? first : (last < live ? last : live);
    p.count[b] = rank_of_row(bits, offsets, last) - rank_of_row(bits, offsets, first);
  }
  if (tid == 0) p.count[p.B] = offsets[nb];
}

__global__ void __launch_bounds__(kTileThreads) voxel_scatter_kernel(VoxelParams p, const unsigned* __restrict__ cnt, const int* __restrict__ slot,
                                                                 const unsigned long long* __restrict__ bits, const int* __restrict__ offsets) {
  __shared__ int word_off[kTileWords];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const unsigned long long* words = bits + (long)tile * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const long base = offsets[tile];
  if (base >= p.capacity) return;  // everything of this workgroup lies beyond the capacity
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    const long idx = base + word_off[w] + lane_rank(word);
    if (idx >= p.capacity) continue;
    const long i = tile_item(tile, s);  // a live row: the bit is only ever set for one
    if (p.xyz_out) {
      const float* src = p.xyz + i * 3;
      float* dst = p.xyz_out + idx * 3;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    if (p.conf_out) p.conf_out[idx] = p.conf[i];
    if (p.rgb_out) {
      const uint8_t* src = p.rgb + i * 3;
      uint8_t* dst = p.rgb_out + idx * 3;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    if (p.normals_out) {
      const float* src = p.normals + i * 3;
      float* dst = p.normals_out + idx * 3;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    if (p.index) p.index[idx] = (int32_t)i;
    if (p.weight) p.weight[idx] = (int32_t)cnt[slot[i]];
  }
}

}  // namespace

size_t voxel_table_slots(int n) {
  size_t slots = 1024;
  while (slots < 2 * (size_t)(n > 0 ? n : 0)) slots <<= 1;
  return slots;
}

size_t voxel_scratch_bytes(int n) { return carve(nullptr, n > 0 ? n : 0).bytes; }

const int32_t* voxel_flags(const void* scratch, int n) { return carve((void*)scratch, n > 0 ? n : 0).flags; }

VoxelRanks voxel_ranks(const void* scratch, int n) {
  const VoxelScratch v = carve((void*)scratch, n > 0 ? n : 0);
  return VoxelRanks{v.slot, v.rank, v.bits, v.offsets};
}

int launch_voxel_thin(const VoxelParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "voxel thinning needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "voxel thinning takes fewer than 2^30 rows, got %d", p.n);
  if (!(p.voxel > 0.f) || !std::isfinite(p.voxel)) MD_FAIL(MD_ERR_INVALID_ARG, "voxel = %g: must be finite and > 0", (double)p.voxel);
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "voxel thinning of %d views", p.B);
  const VoxelScratch v = carve(scratch, p.n);
  const size_t slots = voxel_table_slots(p.n);
  const int nb = tiles_of(p.n);
  const size_t quads = slots / 4;
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kTileThreads - 1) / kTileThreads, 256 * 32);
  hipLaunchKernelGGL(voxel_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, (ulonglong2*)v.keys, (ulonglong2*)v.rank, (uint4*)v.cnt,
                     quads, v.flags, p.dropped);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    hipLaunchKernelGGL(voxel_insert_kernel, dim3((p.n + kTileThreads - 1) / kTileThreads), dim3(kTileThreads), 0, s, p, v.keys, v.rank, v.cnt, v.slot,
                       (unsigned long long)(slots - 1), v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(voxel_select_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, v.rank, v.slot, v.bits, v.counts);
    MD_HIP(hipGetLastError());
  }
  return launch_list_compact(p, v.cnt, v.slot, v.bits, v.counts, v.offsets, s);
}

int launch_list_compact(const VoxelParams& p, const unsigned* cnt, const int* slot, const unsigned long long* bits, const int* counts,
                        int* offsets, hipStream_t s) {
  const int nb = tiles_of(p.n);
  if (!p.count) return MD_OK;  // dropped only
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(kTileThreads), 0, s, p, counts, nb, bits, offsets);
  MD_HIP(hipGetLastError());
  if (p.n == 0 || (!p.xyz_out && !p.conf_out && !p.rgb_out && !p.normals_out && !p.index && !p.weight)) return MD_OK;  // counts only
  hipLaunchKernelGGL(voxel_scatter_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, cnt, slot, bits, offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
