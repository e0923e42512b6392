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
//   scatter  output row = offset + popcounts below (mbcnt), as points.hip's scatter; copies the rows, index and weight
// The tile layout of select / scatter is points.hip's (row = tile * 4096 + step * 256 + thread, word = step * 4 + wave), so the
// words of a tile are in row order. No thread waits on another: a probe claims a slot, finds its key or moves on, and the loop
// is bounded by the table size.
#include <algorithm>
#include <cmath>

#include "voxel_math.h"

namespace md {

namespace {

// the tile layout, the cell key and the probe are shared with the outlier removal (voxel_math.h)
constexpr int kThreads = kGridThreads, kSteps = kGridSteps, kTile = kGridTile, kWords = kGridWords;
constexpr unsigned long long kEmpty = kGridEmpty;

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

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
inline int tiles_of(int n) { return (n + kTile - 1) / kTile; }

VoxelScratch carve(void* base, int n) {
  const size_t slots = voxel_table_slots(n), nb = (size_t)tiles_of(n);
  VoxelScratch s;
  char* p = (char*)base;
  auto take = [&](size_t bytes) {
    char* at = p;
    p += up256(bytes);
    return at;
  };
  s.keys = (unsigned long long*)take(slots * 8);
  s.rank = (unsigned long long*)take(slots * 8);
  s.cnt = (unsigned*)take(slots * 4);
  s.slot = (int*)take((size_t)n * 4);
  s.bits = (unsigned long long*)take(nb * kWords * 8);
  s.counts = (int*)take(nb * 4);
  s.offsets = (int*)take((nb + 1) * 4);
  s.flags = (int*)take(256);
  s.bytes = (size_t)(p - (char*)base);
  return s;
}

// the live rows of the call: the device total of the input list, never more than the rows the launches cover
__device__ __forceinline__ int live_rows(const VoxelParams& p) {
  if (!p.in_count) return p.n;
  const int t = p.in_count[p.B];
  return t < 0 ? 0 : (t < p.n ? t : p.n);
}

// slots is a multiple of 1024: every thread writes four slots with 16-byte stores
__global__ void __launch_bounds__(kThreads) voxel_reset_kernel(ulonglong2* __restrict__ keys, ulonglong2* __restrict__ rank,
                                                               uint4* __restrict__ cnt, size_t quads, int* __restrict__ flags,
                                                               int32_t* __restrict__ dropped) {
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t q = (size_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
    keys[2 * q] = make_ulonglong2(kEmpty, kEmpty);
    keys[2 * q + 1] = make_ulonglong2(kEmpty, kEmpty);
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
__global__ void __launch_bounds__(kThreads) voxel_insert_kernel(VoxelParams p, unsigned long long* __restrict__ keys,
                                                                unsigned long long* __restrict__ rank, unsigned* __restrict__ cnt,
                                                                int* __restrict__ slot, unsigned long long mask, int* __restrict__ flags) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= live_rows(p)) return;
  const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
  unsigned long long key = 0ull;
  const bool in_range = grid_cell_key(x, y, z, p.voxel, &key);
  const unsigned long long out_of_range = __ballot(!in_range);  // the lanes of the wave that are still here
  if (out_of_range && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)__ballot(1)) - 1))
    atomicAdd(p.dropped ? p.dropped : flags + 1, (int)__popcll(out_of_range));
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
__global__ void __launch_bounds__(kThreads) voxel_select_kernel(VoxelParams p, const unsigned long long* __restrict__ rank,
                                                                const int* __restrict__ slot, unsigned long long* __restrict__ bits,
                                                                int* __restrict__ counts) {
  __shared__ int wave_n[kThreads / 64];
  const int tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int live = live_rows(p);
  int n = 0;
  for (int s = 0; s < kSteps; ++s) {
    const long i = (long)tile * kTile + s * kThreads + tid;
    bool keep = false;
    if (i < live) {
      const int h = slot[i];
      if (h >= 0) keep = (0xFFFFFFFFu - (unsigned)rank[h]) == (unsigned)i;
    }
    const unsigned long long word = __ballot(keep);
    if (lane == 0) bits[(long)tile * kWords + s * (kThreads / 64) + wave] = word;
    n += __popcll(word);
  }
  if (lane == 0) wave_n[wave] = n;
  __syncthreads();
  if (tid == 0) counts[tile] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// survivors among rows [0, r), r <= nb * kTile: the offset of r's tile and the popcounts of the words before r in it
__device__ __forceinline__ int rank_of_row(const unsigned long long* __restrict__ bits, const int* __restrict__ offsets, long r) {
  const long t = r / kTile;
  const int in_tile = (int)(r % kTile);
  int sum = offsets[t];
  if (in_tile == 0) return sum;
  const unsigned long long* words = bits + t * kWords;
  for (int w = 0; w < in_tile / 64; ++w) sum += __popcll(words[w]);
  if (in_tile % 64) sum += __popcll(words[in_tile / 64] & ((1ull << (in_tile % 64)) - 1ull));
  return sum;
}

// one workgroup: offsets[i] = sum of counts[0 .. i), offsets[nb] = the total (points.hip's scan); then count[b] = the survivors
// among the rows of view b, count[B] = the total
__global__ void __launch_bounds__(kThreads) voxel_scan_kernel(VoxelParams p, const int* __restrict__ counts, int nb,
                                                              const unsigned long long* __restrict__ bits, int* __restrict__ offsets) {
  __shared__ int part[kThreads];
  const int tid = threadIdx.x;
  const int per = (nb + kThreads - 1) / kThreads;
  const int lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += counts[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - sum;
  for (int i = lo; i < hi; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (tid == kThreads - 1) offsets[nb] = part[tid];
  __syncthreads();  // the offsets this workgroup wrote are visible to all of it
  if (!p.count) return;
  const int live = live_rows(p);
  for (int b = tid; b < p.B; b += kThreads) {
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

__global__ void __launch_bounds__(kThreads) voxel_scatter_kernel(VoxelParams p, const unsigned* __restrict__ cnt, const int* __restrict__ slot,
                                                                 const unsigned long long* __restrict__ bits, const int* __restrict__ offsets) {
  __shared__ int word_off[kWords];
  const int tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned long long* words = bits + (long)tile * kWords;
  if (tid < kWords) {  // wave 0: exclusive scan of the 64 word popcounts (word order = row order)
    const int c = __popcll(words[tid]);
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    word_off[tid] = incl - c;
  }
  __syncthreads();
  const long base = offsets[tile];
  if (base >= p.capacity) return;  // everything of this workgroup lies beyond the capacity
  for (int s = 0; s < kSteps; ++s) {
    const int w = s * (kThreads / 64) + wave;
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
    const long idx = base + word_off[w] + below;
    if (idx >= p.capacity) continue;
    const long i = (long)tile * kTile + s * kThreads + tid;  // a live row: the bit is only ever set for one
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
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kThreads - 1) / kThreads, 256 * 32);
  hipLaunchKernelGGL(voxel_reset_kernel, dim3(reset_grid), dim3(kThreads), 0, s, (ulonglong2*)v.keys, (ulonglong2*)v.rank, (uint4*)v.cnt,
                     quads, v.flags, p.dropped);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    hipLaunchKernelGGL(voxel_insert_kernel, dim3((p.n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, p, v.keys, v.rank, v.cnt, v.slot,
                       (unsigned long long)(slots - 1), v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(voxel_select_kernel, dim3(nb), dim3(kThreads), 0, s, p, v.rank, v.slot, v.bits, v.counts);
    MD_HIP(hipGetLastError());
  }
  return launch_list_compact(p, v.cnt, v.slot, v.bits, v.counts, v.offsets, s);
}

int launch_list_compact(const VoxelParams& p, const unsigned* cnt, const int* slot, const unsigned long long* bits, const int* counts,
                        int* offsets, hipStream_t s) {
  const int nb = tiles_of(p.n);
  if (!p.count) return MD_OK;  // dropped only
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(kThreads), 0, s, p, counts, nb, bits, offsets);
  MD_HIP(hipGetLastError());
  if (p.n == 0 || (!p.xyz_out && !p.conf_out && !p.rgb_out && !p.normals_out && !p.index && !p.weight)) return MD_OK;  // counts only
  hipLaunchKernelGGL(voxel_scatter_kernel, dim3(nb), dim3(kThreads), 0, s, p, cnt, slot, bits, offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
