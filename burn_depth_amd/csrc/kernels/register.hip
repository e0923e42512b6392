// Rigid point-to-point ICP of a point list onto a reference cloud, for gfx950 (md_op_register_points; DESIGN 12.14,
// include/mi_depth.h states the contract, register_math.h holds its arithmetic): K times "pair every moved source row with its
// nearest target row (the matching's definition), sum sixteen f64 leaves over the pairs, solve for the transform",
// then one evaluation pass under the final transform. The sums have a fixed shape over tile_compact.h's layout -- a thread's left
// fold over its 16 steps, the halving tree over a wave's lanes, (W0 + W1) + (W2 + W3) over a tile, then the same again over the
// tile sums in one workgroup -- so nothing depends on the order of arrival and pipeline.register_points gives the same bits.
// Contraction is off in the whole file (Makefile).
//
// The grid is built from the TARGET once per call (match_grid.h: the matching's build kernels and its walk). The launches:
//   reset    the grid's table, the flags, the counters, `dropped`, the histories; A = init
//   insert, alloc, fill   match_grid.h, over the target rows
//   step     K times, tiles of the source: A and the status word are read from device memory (uniform: scalar loads); a set
//            status ends the launch at once. The row is moved in f64 and cast once, the 27 cells are walked with loads only, the
//            winner's target row is loaded again (12 bytes: carrying its coordinates beside the key would cost three more
//            registers and a select per candidate inside the walk), the sixteen leaves go into sixteen f64 accumulators. At the end
//            a butterfly over the wave (legal: all leaves are finite, so the addition commutes bit for bit and lane 0 sees the
//            halving tree's operand order), 512 bytes of LDS, the tile's sixteen sums and its pair count
//   solve    K times, one workgroup: thread u folds the tile sums u, u + 256, .. in ascending order, the same wave tree and
//            four-wave combine, then thread 0 runs register_math.h's solve, writes A, the history entry, the status
//   the evaluation step (template flag: also the row outputs and the counters) and the reduce without a solve, which fills
//            entry K of the histories, the last counters and `transform`
// All K iterations are always enqueued: the sequence is static. No float atomics; integer atomics for counters, one per wave.
// No thread waits on another: every loop is bounded by the table size, a bucket size or the tile count. Vector stores only.
//
// The point-to-plane form (RegisterParams::plane) runs the same launches on sibling step and reduce kernels at the
// end of this file: 29 leaves of every pair whose target normal is usable, reg_solve_plane, status 3 for a degenerate system.
#include <algorithm>
#include <cmath>

#include "match_grid.h"
#include "register_math.h"

namespace md {

namespace {

constexpr int kFlagWords = 64;
constexpr int kRegStatsFlag = 8;               // flags[8 .. 16): the eight counters when `stats` is null
constexpr unsigned kNoDistance = 0x7F800000u;  // dist2 of a row without a nearest

struct RegisterScratch {  // the parts of the scratch buffer, 256-byte aligned
  MatchGrid g;
  double* sums;  // [tiles, 16] the tile sums of the last step ([tiles, 29] in the point-to-plane form)
  int* pairs;    // [tiles] its pair counts
  double* A;     // [12] the running transform
  int* flags;    // [0] a probe loop ran out, [1] dropped (when the caller takes none), [2] the bucket cursor, [8..16) the counters
  size_t bytes;
};

RegisterScratch carve(void* base, int n, int t, int leaves = kRegLeaves) {
  const size_t nb = (size_t)tiles_of(n);
  RegisterScratch s;
  Carver c(base);
  s.g = carve_match_grid(c, t);
  s.sums = c.take<double>(nb * (size_t)leaves);
  s.pairs = c.take<int>(nb);
  s.A = c.take<double>(12);
  s.flags = c.take<int>(kFlagWords);
  s.bytes = c.bytes;
  return s;
}

// slots is a multiple of 1024 (match_grid_reset). history = K + 1 <= 65 entries.
__global__ void __launch_bounds__(kTileThreads) register_reset_kernel(RegisterParams p, ulonglong2* __restrict__ keys, uint4* __restrict__ cnt,
                                                                  uint4* __restrict__ start, uint4* __restrict__ fill, size_t quads,
                                                                  int* __restrict__ flags, int32_t* __restrict__ stats, double* __restrict__ A) {
  match_grid_reset(keys, cnt, start, fill, quads);
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  if (tid < 8) stats[tid] = 0;
  if (tid < 12) A[tid] = p.init[tid];
  if (tid <= p.iterations) {
    if (p.pairs) p.pairs[tid] = 0;
    if (p.sum_d2) p.sum_d2[tid] = 0.;
  }
  if (tid == 0) {
    flags[0] = 0;
    flags[1] = 0;
    flags[2] = 0;
    if (p.dropped) p.dropped[0] = 0;
  }
}

// stats[4] counts the target rows that enter the grid
__global__ void __launch_bounds__(kTileThreads) register_insert_kernel(const float* __restrict__ target, int t, float radius,
                                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ cnt,
                                                                   int* __restrict__ slot, unsigned long long mask, int* __restrict__ flags,
                                                                   int32_t* __restrict__ stats) {
  match_grid_insert(target, t, radius, keys, cnt, slot, mask, flags, stats + 4);
}

__global__ void __launch_bounds__(kTileThreads) register_alloc_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ start,
                                                                  int* __restrict__ flags) {
  match_grid_alloc(cnt, start, flags + 2);
}

__global__ void __launch_bounds__(kTileThreads) register_fill_kernel(const float* __restrict__ target, int t, const unsigned* __restrict__ start,
                                                                 unsigned* __restrict__ fill, const int* __restrict__ slot,
                                                                 uint4* __restrict__ bucket, int* __restrict__ flags) {
  match_grid_fill(target, t, start, fill, slot, bucket, flags);
}

// The wave's value of every leaf and of the integer n, in lane 0 (a butterfly: every lane ends with a sum, lane 0 with the
// halving tree's), then the four-wave combine through LDS. Holds a barrier; -> thread 0..15 hold leaf `tid` of the workgroup in
// *leaf, every thread the workgroup's n.
__device__ __forceinline__ int workgroup_sums(double* acc, int n, double (*wave_sum)[kRegLeaves], int* wave_n, double* leaf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
    for (int l = 0; l < kRegLeaves; ++l) acc[l] = acc[l] + __shfl_xor(acc[l], h, 64);
    n += __shfl_xor(n, h, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < kRegLeaves; ++l) wave_sum[wave][l] = acc[l];
    wave_n[wave] = n;
  }
  __syncthreads();
  if (tid < kRegLeaves) *leaf = (wave_sum[0][tid] + wave_sum[1][tid]) + (wave_sum[2][tid] + wave_sum[3][tid]);
  return (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// grid tiles of the source. The table and the buckets no longer change: loads only. stats[1] is the status of the call: a set
// one ends an iteration's launch before it reads anything else. kEval: the pass under the final A, which always runs and also
// writes the row outputs and the counters stats[2] (in-range rows) and `dropped`.
template <bool kEval>
__global__ void __launch_bounds__(kTileThreads) register_step_kernel(RegisterParams p, const double* __restrict__ A_dev,
                                                                 const unsigned long long* __restrict__ keys, const unsigned* __restrict__ cnt,
                                                                 const unsigned* __restrict__ start, const uint4* __restrict__ bucket,
                                                                 unsigned long long mask, double* __restrict__ sums, int* __restrict__ pairs,
                                                                 int32_t* stats, int32_t* dropped) {
  __shared__ double wave_sum[kTileWaves][kRegLeaves];
  __shared__ int wave_n[kTileWaves];
  if (!kEval && stats[1] != 0) return;  // the whole grid
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  double A[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) A[i] = A_dev[i];
  const int live = live_count(p.in_count, p.B, p.n);
  const float r2 = p.radius * p.radius;
  const unsigned bucket_rows = (unsigned)p.t;
  double acc[kRegLeaves];
#pragma unroll
  for (int l = 0; l < kRegLeaves; ++l) acc[l] = 0.;
  int n_pair = 0, n_in = 0, n_out = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool in_range = false, hit = false, row = false;
    if (i < live) {
      row = true;
      const float src[3] = {p.xyz[i * 3], p.xyz[i * 3 + 1], p.xyz[i * 3 + 2]};
      const float mx = reg_move_axis(A, 0, src[0], src[1], src[2]), my = reg_move_axis(A, 1, src[0], src[1], src[2]),
                  mz = reg_move_axis(A, 2, src[0], src[1], src[2]);
      unsigned long long own = 0ull, best = ~0ull;
      in_range = grid_cell_key(mx, my, mz, p.radius, &own);
      if (in_range) best = match_grid_nearest(mx, my, mz, own, r2, keys, cnt, start, bucket, mask, bucket_rows);
      hit = best != ~0ull;
      const unsigned d2_bits = hit ? (unsigned)(best >> 32) : kNoDistance;
      if (hit) {
        const float* q = p.target + (long)(unsigned)(best & 0xFFFFFFFFull) * 3;
        const float dst[3] = {q[0], q[1], q[2]};
        reg_add_leaves(acc, src, dst, __uint_as_float(d2_bits));
      }
      if (kEval) {
        if (p.normals_out) {
          const float nx = p.normals[i * 3], ny = p.normals[i * 3 + 1], nz = p.normals[i * 3 + 2];
          unsigned* o = (unsigned*)p.normals_out + i * 3;
          o[0] = reg_out_bits(reg_turn_axis(A, 0, nx, ny, nz));
          o[1] = reg_out_bits(reg_turn_axis(A, 1, nx, ny, nz));
          o[2] = reg_out_bits(reg_turn_axis(A, 2, nx, ny, nz));
        }
        if (p.xyz_out) {  // may be xyz: this thread has read its row
          unsigned* o = (unsigned*)p.xyz_out + i * 3;
          o[0] = reg_out_bits(mx);
          o[1] = reg_out_bits(my);
          o[2] = reg_out_bits(mz);
        }
        if (p.nearest) p.nearest[i] = hit ? (int32_t)(unsigned)(best & 0xFFFFFFFFull) : (in_range ? -1 : -2);
        if (p.dist2) ((unsigned*)p.dist2)[i] = d2_bits;
      }
    }
    n_pair += hit ? 1 : 0;
    if (kEval) {
      n_in += __popcll(__ballot(in_range));
      n_out += __popcll(__ballot(row && !in_range));
    }
  }
  if (kEval && lane == 0) {  // one add per wave and counter
    if (n_in) atomicAdd(stats + 2, n_in);
    if (n_out) atomicAdd(dropped, n_out);
  }
  double leaf = 0.;
  const int n = workgroup_sums(acc, n_pair, wave_sum, wave_n, &leaf);
  if (tid < kRegLeaves) sums[(long)tile * kRegLeaves + tid] = leaf;
  if (tid == 0) pairs[tile] = n;
}

// One workgroup. kSolve: iteration k -- a set status ends the launch at once; otherwise the sums of the step before it, the
// history entry k, and the solve or status 2. !kSolve: behind the evaluation step -- entry k = K, stats[3], `transform`.
template <bool kSolve>
__global__ void __launch_bounds__(kTileThreads) register_reduce_kernel(RegisterParams p, int k, int tiles, const double* __restrict__ sums,
                                                                   const int* __restrict__ pairs, double* A_dev, int32_t* stats) {
  __shared__ double wave_sum[kTileWaves][kRegLeaves];
  __shared__ int wave_n[kTileWaves];
  __shared__ double S[kRegLeaves];
  if (kSolve && stats[1] != 0) return;  // the whole workgroup
  const int tid = threadIdx.x;
  double acc[kRegLeaves];
#pragma unroll
  for (int l = 0; l < kRegLeaves; ++l) acc[l] = 0.;
  int n_thread = 0;
  for (int tile = tid; tile < tiles; tile += kTileThreads) {
#pragma unroll
    for (int l = 0; l < kRegLeaves; ++l) acc[l] = acc[l] + sums[(long)tile * kRegLeaves + l];
    n_thread += pairs[tile];
  }
  double leaf = 0.;
  const int n = workgroup_sums(acc, n_thread, wave_sum, wave_n, &leaf);
  if (tid < kRegLeaves) S[tid] = leaf;
  __syncthreads();
  if (tid != 0) return;
  if (p.pairs) p.pairs[k] = n;
  if (p.sum_d2) p.sum_d2[k] = S[15];
  if (kSolve) {
    if (n < p.min_pairs) {
      stats[1] = 2;
      return;
    }
    double A_old[12], A_new[12];
    for (int i = 0; i < 12; ++i) A_old[i] = A_dev[i];
    reg_solve(n, S, A_new);
    for (int i = 0; i < 12; ++i) A_dev[i] = A_new[i];
    stats[0] = stats[0] + 1;
    if ((p.rot_eps > 0. || p.trans_eps > 0.) && reg_converged(A_new, A_old, p.rot_eps, p.trans_eps)) stats[1] = 1;
  } else {
    stats[3] = n;
    if (p.transform)
      for (int i = 0; i < 12; ++i) p.transform[i] = A_dev[i];
  }
}

// ---- the point-to-plane form: sibling kernels, so the point form's code above is what it was ----
// The same tree over kRegPlaneLeaves = 29 values: a pair enters only when its target normal is usable (finite, not all zero), so
// every leaf is finite -- a usable pair has finite q and n, and m of a paired row is finite -- and the butterfly argument of the
// point form holds unchanged: the addition commutes bit for bit and lane 0 sees the halving tree's operand order. LDS 4 x 29 x 8
// bytes. No float atomics, integer atomics for the per-wave counters only, vector stores only, no thread waits on another.
__device__ __forceinline__ int plane_workgroup_sums(double* acc, int n, double (*wave_sum)[kRegPlaneLeaves], int* wave_n, double* leaf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
    for (int l = 0; l < kRegPlaneLeaves; ++l) acc[l] = acc[l] + __shfl_xor(acc[l], h, 64);
    n += __shfl_xor(n, h, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < kRegPlaneLeaves; ++l) wave_sum[wave][l] = acc[l];
    wave_n[wave] = n;
  }
  __syncthreads();
  if (tid < kRegPlaneLeaves) *leaf = (wave_sum[0][tid] + wave_sum[1][tid]) + (wave_sum[2][tid] + wave_sum[3][tid]);
  return (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// register_step_kernel with the winner's normal loaded behind its row (12 more bytes per paired row) and the 29 leaves of the
// MOVED row. nearest / dist2 report the pair whatever its normal; only usable pairs are summed and counted.
template <bool kEval>
__global__ void __launch_bounds__(kTileThreads) register_plane_step_kernel(RegisterParams p, const double* __restrict__ A_dev,
                                                                       const unsigned long long* __restrict__ keys,
                                                                       const unsigned* __restrict__ cnt, const unsigned* __restrict__ start,
                                                                       const uint4* __restrict__ bucket, unsigned long long mask,
                                                                       double* __restrict__ sums, int* __restrict__ pairs, int32_t* stats,
                                                                       int32_t* dropped) {
  __shared__ double wave_sum[kTileWaves][kRegPlaneLeaves];
  __shared__ int wave_n[kTileWaves];
  if (!kEval && stats[1] != 0) return;  // the whole grid
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  double A[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) A[i] = A_dev[i];
  const int live = live_count(p.in_count, p.B, p.n);
  const float r2 = p.radius * p.radius;
  const unsigned bucket_rows = (unsigned)p.t;
  double acc[kRegPlaneLeaves];
#pragma unroll
  for (int l = 0; l < kRegPlaneLeaves; ++l) acc[l] = 0.;
  int n_pair = 0, n_in = 0, n_out = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool in_range = false, hit = false, row = false, usable = false;
    if (i < live) {
      row = true;
      const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
      const float m[3] = {reg_move_axis(A, 0, x, y, z), reg_move_axis(A, 1, x, y, z), reg_move_axis(A, 2, x, y, z)};
      unsigned long long own = 0ull, best = ~0ull;
      in_range = grid_cell_key(m[0], m[1], m[2], p.radius, &own);
      if (in_range) best = match_grid_nearest(m[0], m[1], m[2], own, r2, keys, cnt, start, bucket, mask, bucket_rows);
      hit = best != ~0ull;
      const unsigned d2_bits = hit ? (unsigned)(best >> 32) : kNoDistance;
      if (hit) {
        const long j = (long)(unsigned)(best & 0xFFFFFFFFull) * 3;
        const float nrm[3] = {p.target_normals[j], p.target_normals[j + 1], p.target_normals[j + 2]};
        usable = reg_normal_usable(nrm);
        if (usable) {
          const float dst[3] = {p.target[j], p.target[j + 1], p.target[j + 2]};
          reg_add_plane_leaves(acc, m, dst, nrm, __uint_as_float(d2_bits));
        }
      }
      if (kEval) {
        if (p.normals_out) {
          const float nx = p.normals[i * 3], ny = p.normals[i * 3 + 1], nz = p.normals[i * 3 + 2];
          unsigned* o = (unsigned*)p.normals_out + i * 3;
          o[0] = reg_out_bits(reg_turn_axis(A, 0, nx, ny, nz));
          o[1] = reg_out_bits(reg_turn_axis(A, 1, nx, ny, nz));
          o[2] = reg_out_bits(reg_turn_axis(A, 2, nx, ny, nz));
        }
        if (p.xyz_out) {  // may be xyz: this thread has read its row
          unsigned* o = (unsigned*)p.xyz_out + i * 3;
          o[0] = reg_out_bits(m[0]);
          o[1] = reg_out_bits(m[1]);
          o[2] = reg_out_bits(m[2]);
        }
        if (p.nearest) p.nearest[i] = hit ? (int32_t)(unsigned)(best & 0xFFFFFFFFull) : (in_range ? -1 : -2);
        if (p.dist2) ((unsigned*)p.dist2)[i] = d2_bits;
      }
    }
    n_pair += usable ? 1 : 0;
    if (kEval) {
      n_in += __popcll(__ballot(in_range));
      n_out += __popcll(__ballot(row && !in_range));
    }
  }
  if (kEval && lane == 0) {  // one add per wave and counter
    if (n_in) atomicAdd(stats + 2, n_in);
    if (n_out) atomicAdd(dropped, n_out);
  }
  double leaf = 0.;
  const int n = plane_workgroup_sums(acc, n_pair, wave_sum, wave_n, &leaf);
  if (tid < kRegPlaneLeaves) sums[(long)tile * kRegPlaneLeaves + tid] = leaf;
  if (tid == 0) pairs[tile] = n;
}

// register_reduce_kernel over 29 sums with reg_solve_plane; a degenerate system is status 3 and A stays. An iteration that a
// set status skips writes its 0 into sum_r2 here, so the reset kernel is the point form's.
template <bool kSolve>
__global__ void __launch_bounds__(kTileThreads) register_plane_reduce_kernel(RegisterParams p, int k, int tiles, const double* __restrict__ sums,
                                                                         const int* __restrict__ pairs, double* A_dev, int32_t* stats) {
  __shared__ double wave_sum[kTileWaves][kRegPlaneLeaves];
  __shared__ int wave_n[kTileWaves];
  __shared__ double S[kRegPlaneLeaves];
  const int tid = threadIdx.x;
  if (kSolve && stats[1] != 0) {  // the whole workgroup
    if (tid == 0 && p.sum_r2) p.sum_r2[k] = 0.;
    return;
  }
  double acc[kRegPlaneLeaves];
#pragma unroll
  for (int l = 0; l < kRegPlaneLeaves; ++l) acc[l] = 0.;
  int n_thread = 0;
  for (int tile = tid; tile < tiles; tile += kTileThreads) {
#pragma unroll
    for (int l = 0; l < kRegPlaneLeaves; ++l) acc[l] = acc[l] + sums[(long)tile * kRegPlaneLeaves + l];
    n_thread += pairs[tile];
  }
  double leaf = 0.;
  const int n = plane_workgroup_sums(acc, n_thread, wave_sum, wave_n, &leaf);
  if (tid < kRegPlaneLeaves) S[tid] = leaf;
  __syncthreads();
  if (tid != 0) return;
  if (p.pairs) p.pairs[k] = n;
  if (p.sum_d2) p.sum_d2[k] = S[28];
  if (p.sum_r2) p.sum_r2[k] = S[27];
  if (kSolve) {
    if (n < p.min_pairs) {
      stats[1] = 2;
      return;
    }
    double A_old[12], A_new[12];
    for (int i = 0; i < 12; ++i) A_old[i] = A_dev[i];
    if (!reg_solve_plane(n, S, A_old, A_new)) {
      stats[1] = 3;
      return;
    }
    for (int i = 0; i < 12; ++i) A_dev[i] = A_new[i];
    stats[0] = stats[0] + 1;
    if ((p.rot_eps > 0. || p.trans_eps > 0.) && reg_converged(A_new, A_old, p.rot_eps, p.trans_eps)) stats[1] = 1;
  } else {
    stats[3] = n;
    if (p.transform)
      for (int i = 0; i < 12; ++i) p.transform[i] = A_dev[i];
  }
}

}  // namespace

size_t register_plane_scratch_bytes(int n, int t) { return carve(nullptr, n > 0 ? n : 0, t > 0 ? t : 0, kRegPlaneLeaves).bytes; }

const int32_t* register_plane_flags(const void* scratch, int n, int t) {
  return carve((void*)scratch, n > 0 ? n : 0, t > 0 ? t : 0, kRegPlaneLeaves).flags;
}

size_t register_scratch_bytes(int n, int t) { return carve(nullptr, n > 0 ? n : 0, t > 0 ? t : 0).bytes; }

const int32_t* register_flags(const void* scratch, int n, int t) { return carve((void*)scratch, n > 0 ? n : 0, t > 0 ? t : 0).flags; }

int launch_register_points(const RegisterParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "registration needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "registration takes fewer than 2^30 rows, got %d", p.n);
  if (p.t < 0 || p.t >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "registration takes fewer than 2^30 target rows, got %d", p.t);
  if (!(p.radius > 0.f) || !std::isfinite(p.radius) || !std::isfinite(p.radius * p.radius))
    MD_FAIL(MD_ERR_INVALID_ARG, "radius = %g: it and its square must be finite and > 0", (double)p.radius);
  if (p.iterations < 1 || p.iterations > 64) MD_FAIL(MD_ERR_INVALID_ARG, "iterations = %d outside 1..64", p.iterations);
  if (p.min_pairs < 3) MD_FAIL(MD_ERR_INVALID_ARG, "min_pairs = %d: at least 3", p.min_pairs);
  if (p.plane && p.min_pairs < 6) MD_FAIL(MD_ERR_INVALID_ARG, "min_pairs = %d: the point-to-plane form takes at least 6", p.min_pairs);
  if (p.plane && p.t > 0 && !p.target_normals) MD_FAIL(MD_ERR_INVALID_ARG, "the point-to-plane form needs the target's normals");
  if (!p.plane && p.sum_r2) MD_FAIL(MD_ERR_INVALID_ARG, "sum_r2 is the point-to-plane form's");
  if (!(p.rot_eps >= 0.) || !std::isfinite(p.rot_eps) || !(p.trans_eps >= 0.) || !std::isfinite(p.trans_eps))
    MD_FAIL(MD_ERR_INVALID_ARG, "rot_eps = %g, trans_eps = %g: finite and >= 0", p.rot_eps, p.trans_eps);
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(p.init[i])) MD_FAIL(MD_ERR_INVALID_ARG, "init[%d] = %g is not finite", i, p.init[i]);
  if (p.t > 0 && !p.target) MD_FAIL(MD_ERR_INVALID_ARG, "target pointer is null");
  if (p.n > 0 && !p.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "xyz pointer is null");
  if (p.normals_out && !p.normals) MD_FAIL(MD_ERR_INVALID_ARG, "a normals output needs a normals row");
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "registration of %d views", p.B);
  const RegisterScratch v = carve(scratch, p.n, p.t, p.plane ? kRegPlaneLeaves : kRegLeaves);
  const size_t slots = voxel_table_slots(p.t);
  const int nb = tiles_of(p.n);
  const size_t quads = slots / 4;
  const unsigned long long mask = (unsigned long long)(slots - 1);
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kTileThreads - 1) / kTileThreads, 256 * 32);
  int32_t* stats = p.stats ? p.stats : v.flags + kRegStatsFlag;
  int32_t* dropped = p.dropped ? p.dropped : v.flags + 1;
  hipLaunchKernelGGL(register_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, p, (ulonglong2*)v.g.keys, (uint4*)v.g.cnt, (uint4*)v.g.start,
                     (uint4*)v.g.fill, quads, v.flags, stats, v.A);
  MD_HIP(hipGetLastError());
  if (p.t > 0) {
    const unsigned target_grid = (unsigned)((p.t + kTileThreads - 1) / kTileThreads);
    hipLaunchKernelGGL(register_insert_kernel, dim3(target_grid), dim3(kTileThreads), 0, s, p.target, p.t, p.radius, v.g.keys, v.g.cnt, v.g.slot, mask,
                       v.flags, stats);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(register_alloc_kernel, dim3((unsigned)(slots / kTileThreads)), dim3(kTileThreads), 0, s, v.g.cnt, v.g.start, v.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(register_fill_kernel, dim3(target_grid), dim3(kTileThreads), 0, s, p.target, p.t, v.g.start, v.g.fill, v.g.slot, v.g.bucket,
                       v.flags);
    MD_HIP(hipGetLastError());
  }
  if (p.plane) {  // the same sequence on the sibling kernels
    for (int k = 0; k < p.iterations; ++k) {
      if (nb > 0) {
        hipLaunchKernelGGL(register_plane_step_kernel<false>, dim3(nb), dim3(kTileThreads), 0, s, p, v.A, v.g.keys, v.g.cnt, v.g.start, v.g.bucket,
                           mask, v.sums, v.pairs, stats, dropped);
        MD_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(register_plane_reduce_kernel<true>, dim3(1), dim3(kTileThreads), 0, s, p, k, nb, v.sums, v.pairs, v.A, stats);
      MD_HIP(hipGetLastError());
    }
    if (nb > 0) {
      hipLaunchKernelGGL(register_plane_step_kernel<true>, dim3(nb), dim3(kTileThreads), 0, s, p, v.A, v.g.keys, v.g.cnt, v.g.start, v.g.bucket, mask,
                         v.sums, v.pairs, stats, dropped);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(register_plane_reduce_kernel<false>, dim3(1), dim3(kTileThreads), 0, s, p, p.iterations, nb, v.sums, v.pairs, v.A, stats);
    MD_HIP(hipGetLastError());
    return MD_OK;
  }
  for (int k = 0; k < p.iterations; ++k) {
    if (nb > 0) {
      hipLaunchKernelGGL(register_step_kernel<false>, dim3(nb), dim3(kTileThreads), 0, s, p, v.A, v.g.keys, v.g.cnt, v.g.start, v.g.bucket, mask, v.sums,
                         v.pairs, stats, dropped);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(register_reduce_kernel<true>, dim3(1), dim3(kTileThreads), 0, s, p, k, nb, v.sums, v.pairs, v.A, stats);
    MD_HIP(hipGetLastError());
  }
  if (nb > 0) {
    hipLaunchKernelGGL(register_step_kernel<true>, dim3(nb), dim3(kTileThreads), 0, s, p, v.A, v.g.keys, v.g.cnt, v.g.start, v.g.bucket, mask, v.sums,
                       v.pairs, stats, dropped);
    MD_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(register_reduce_kernel<false>, dim3(1), dim3(kTileThreads), 0, s, p, p.iterations, nb, v.sums, v.pairs, v.A, stats);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
