// What the point path's list kernels share (points, view_filter, voxel, outlier, decimate, components, smooth, mesh, render, raster):
// the tile layout of the ballot words and the pieces of the order-preserving compaction built on it. This file states the layout
// contract once; a kernel that writes ballot words and a kernel that reads them agree on it by including this file.
//
// The layout. A workgroup has 256 threads, 4 waves of 64, and owns one tile of 4096 items (pixels, rows, quads or faces), 16 per
// thread:  item = tile * 4096 + step * 256 + thread  (tile_item). In every step each wave leaves one 64-bit ballot word, bit l = lane
// l's item enters the list:  word = step * 4 + wave  (tile_word), 64 words per tile at  bits + tile * 64. So the words of a tile,
// and the bits inside a word, are in item order, and a list keeps the order of its input without atomics:
//   classify  ballot_step per step, tile_sum at the end: the tile's words and its count
//   scan      one workgroup, scan_tile_counts: exclusive offsets of the tile counts, offsets[tiles] = the total
//   scatter   scan_word_counts, then per step  row = offsets[tile] + word_off[word] + lane_rank(word)
// rank_of_row is the same rank for an arbitrary row, from the words and the offsets alone.
// Every device function here is called by all threads of a 256-thread workgroup unless it says otherwise.
#pragma once

#include "ops.h"

namespace md {

constexpr int kTileThreads = 256;                        // 4 waves of 64
constexpr int kTileWaves = kTileThreads / 64;
constexpr int kTileSteps = 16;                           // items per thread
constexpr int kTileItems = kTileThreads * kTileSteps;    // 4096 items per workgroup
constexpr int kTileWords = kTileItems / 64;              // 64 ballot words per workgroup

// ---- host ----
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
inline int tiles_of(long n) { return (int)((n + kTileItems - 1) / kTileItems); }

// Carves a scratch buffer into 256-byte aligned parts, in the order of the take calls. base = null: only the sizes are wanted.
struct Carver {
  char* base;
  size_t bytes;  // carved so far
  explicit Carver(void* b, size_t skip = 0) : base((char*)b), bytes(skip) {}
  template <class T>
  T* take(size_t count) {
    T* at = base ? (T*)(base + bytes) : nullptr;
    bytes += up256(count * sizeof(T));
    return at;
  }
};

// ---- device: the layout ----
__device__ __forceinline__ long tile_item(long tile, int step) { return tile * kTileItems + step * kTileThreads + (int)threadIdx.x; }
__device__ __forceinline__ int tile_word(int step) { return step * kTileWaves + (int)(threadIdx.x >> 6); }

// the live items of a call: the device total count[at], clamped to the n items the launches cover; count = null: n
__device__ __forceinline__ int live_count(const int32_t* __restrict__ count, int at, int n) {
  if (!count) return n;
  const int t = count[at];
  return t < 0 ? 0 : (t < n ? t : n);
}

// ---- device: classify ----
// One step of a wave: the ballot word of `bit` goes to *slot (the caller's bits + tile * kTileWords + tile_word(step)).
// -> its popcount, the same in every lane.
__device__ __forceinline__ int ballot_step(bool bit, unsigned long long* __restrict__ slot) {
  const unsigned long long word = __ballot(bit);
  if ((threadIdx.x & 63) == 0) *slot = word;
  return __popcll(word);
}

// The end of a tile: n is a wave's sum over its steps (the same in every lane) -> the sum of the four waves. Holds a barrier.
__device__ __forceinline__ int tile_sum(int n, int* wave_n /* LDS [kTileWaves] */) {
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  return (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// ---- device: scan ----
// The body of a one-workgroup scan launch: offsets[i] = sum of counts[0 .. i), offsets[n] = the total. Every thread sums a chunk
// of ceil(n / 256) counts, the 256 chunk sums are scanned in LDS. Ends in a barrier: the offsets are visible to the workgroup.
__device__ __forceinline__ void scan_tile_counts(const int* __restrict__ counts, int n, int* __restrict__ offsets,
                                                 int* part /* LDS [kTileThreads] */) {
  const int tid = threadIdx.x;
  const int per = (n + kTileThreads - 1) / kTileThreads;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += counts[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kTileThreads; d <<= 1) {  // inclusive scan of the 256 chunk sums
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
  if (tid == kTileThreads - 1) offsets[n] = part[tid];
  __syncthreads();
}

// behind scan_tile_counts, for a grid of B views of `tiles` tiles each (n = B * tiles): count[b] = the items of view b, count[B] = the total
__device__ __forceinline__ void view_totals(const int* __restrict__ offsets, int n, int tiles, int B, int32_t* __restrict__ count) {
  for (int b = threadIdx.x; b < B; b += kTileThreads) count[b] = offsets[(b + 1) * tiles] - offsets[b * tiles];
  if (threadIdx.x == 0) count[B] = offsets[n];
}

// list items among the items [0, r) of a one-dimensional grid of tiles, r <= tiles * kTileItems: the offset of r's tile and the
// popcounts of the words before r in it. One thread.
__device__ __forceinline__ int rank_of_row(const unsigned long long* __restrict__ bits, const int* __restrict__ offsets, long r) {
  const long t = r / kTileItems;
  const int in_tile = (int)(r % kTileItems);
  int sum = offsets[t];
  if (in_tile == 0) return sum;
  const unsigned long long* words = bits + t * kTileWords;
  for (int w = 0; w < in_tile / 64; ++w) sum += __popcll(words[w]);
  if (in_tile % 64) sum += __popcll(words[in_tile / 64] & ((1ull << (in_tile % 64)) - 1ull));
  return sum;
}

// ---- device: scatter ----
// Wave 0 only (call under threadIdx.x < kTileWords, barrier behind it): c = the list items of word threadIdx.x, one popcount or,
// for the mesh's word pairs, two -> word_off[w] = the sum of c over the words before w.
__device__ __forceinline__ void scan_word_counts(int c, int* word_off /* LDS [kTileWords] */) {
  const int lane = threadIdx.x;
  int incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  word_off[lane] = incl - c;
}

// the set bits of the wave's word below this lane's bit
__device__ __forceinline__ unsigned lane_rank(unsigned long long word) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
}

// ---- device: counters and keys ----
// *counter += the lanes of the wave with `bit`: one integer add per wave, by its first active lane, so it is right both where no
// thread leaves before the call and where lanes have already returned. Every lane that is still in the kernel calls it.
__device__ __forceinline__ void wave_count_add(bool bit, int32_t* counter) {
  const unsigned long long word = __ballot(bit);  // of the lanes that are still here
  if (word && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)__ballot(1)) - 1)) atomicAdd(counter, (int)__popcll(word));
}

// grid-stride fill of a buffer of 64-bit keys with all ones, `pairs` 16-byte stores in all; any grid of kTileThreads
__device__ __forceinline__ void fill_keys(ulonglong2* __restrict__ keys, size_t pairs) {
  const size_t stride = (size_t)gridDim.x * kTileThreads;
  for (size_t q = (size_t)blockIdx.x * kTileThreads + threadIdx.x; q < pairs; q += stride) keys[q] = make_ulonglong2(~0ull, ~0ull);
}

}  // namespace md
