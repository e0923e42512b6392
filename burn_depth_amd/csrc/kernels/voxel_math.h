// What the hash-grid kernels share (kernels/voxel.hip, kernels/outlier.hip): the cell and key of a point, the table's hash and
// its two probes. include/mi_depth.h states the contract of the cell and the key; the files that compute a cell compile with
// contraction off (Makefile). The tile layout of the ballot words is tile_compact.h's.
#pragma once

#include "tile_compact.h"

namespace md {

constexpr unsigned long long kGridEmpty = ~0ull;
constexpr float kGridHalf = 1048576.f;                // 2^20 cells on either side of the origin, 21 bits per axis
constexpr int kGridHalfInt = 1048576;

// splitmix64's finaliser: spreads neighbouring cells over the table. It decides where a key lives, never what a kernel outputs.
__device__ __forceinline__ unsigned long long grid_mix64(unsigned long long x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// the key of the cell with the biased coordinates bx, by, bz in [0, 2^21)
__device__ __forceinline__ unsigned long long grid_key(int bx, int by, int bz) {
  return ((unsigned long long)bx << 42) | ((unsigned long long)by << 21) | (unsigned long long)bz;
}

// c_a = floorf(p_a / side); in range: the coordinates finite and -2^20 <= c_a < 2^20 on every axis, compared in float
__device__ __forceinline__ bool grid_cell_key(float x, float y, float z, float side, unsigned long long* key) {
  const float cx = floorf(x / side), cy = floorf(y / side), cz = floorf(z / side);
  const bool in_range = isfinite(x) && isfinite(y) && isfinite(z) && cx >= -kGridHalf && cx < kGridHalf && cy >= -kGridHalf &&
                        cy < kGridHalf && cz >= -kGridHalf && cz < kGridHalf;
  if (in_range) *key = grid_key((int)cx + kGridHalfInt, (int)cy + kGridHalfInt, (int)cz + kGridHalfInt);
  return in_range;
}

// The slot of `key`, claiming an empty one on the way (atomicCAS only on an empty slot); -1: every slot holds another key.
// Linear probing; the loop is bounded by the table size and waits on nobody. mask = slots - 1.
__device__ __forceinline__ long grid_claim(unsigned long long* __restrict__ keys, unsigned long long mask, unsigned long long key) {
  unsigned long long h = grid_mix64(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    unsigned long long cur = __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kGridEmpty) cur = atomicCAS(keys + h, kGridEmpty, key);  // returns what was there: all ones = this thread claimed the slot
    if (cur == kGridEmpty || cur == key) return (long)h;
    h = (h + 1) & mask;
  }
  return -1;
}

// The slot of `key` in a table that no longer changes, with loads only; -1: the key is not in it.
__device__ __forceinline__ long grid_find(const unsigned long long* __restrict__ keys, unsigned long long mask, unsigned long long key) {
  unsigned long long h = grid_mix64(key) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    const unsigned long long cur = keys[h];
    if (cur == key) return (long)h;
    if (cur == kGridEmpty) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

}  // namespace md
