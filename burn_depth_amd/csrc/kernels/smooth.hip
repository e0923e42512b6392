// Taubin (lambda | mu) and Laplacian smoothing of a mesh, and the area-weighted vertex normals of the smoothed faces, for gfx950
// (md_op_smooth_mesh, md_infer_points_smooth; DESIGN 12.10, include/mi_depth.h states the contract). The rows are rounded to an
// integer lattice of side `step` once; every step sums neighbour coordinates in int64 and moves a row by a whole number of
// lattice steps, so the result does not depend on the order in which the faces arrive. pipeline.smooth_mesh restates it, and
// smooth_math.h holds the arithmetic of a row and of a face.
//
// The launches:
//   quantise    rows: k = rint(p / step), the range flag; deg, open, S and the five counters to 0
//   topology    one thread per face: deg[v] += 2 and open[v] += mix(next) - mix(prev) for the corners of a live face; invalid and
//               degenerate faces counted with one integer add per wave
//   per step    accumulate, one thread per live face: S[v] += k[next] + k[prev] per axis, nine 64-bit adds (a corner that every
//               live lane of the wave shares is summed across the wave first and added once: the fan);
//               update, rows: k += rint(factor (S / deg - k)) for the rows that are not pinned, S back to 0
//   normals     one thread per live face: the int64 cross product of the final lattice positions into S of its three corners
//   write       rows: the input bits of a row that ended where it began, k * step of the others, the normals, and the row
//               counters (not in range, open, moved) with one add per wave
// The row counters are added in `write` and not in `quantise`, which zeroes them: an add of one workgroup could otherwise
// arrive before the zero of another. No thread waits on another. Vector stores and integer global atomics only.
#include <algorithm>

#include "smooth_math.h"
#include "tile_compact.h"

namespace md {

namespace {

typedef unsigned long long u64;

struct SmoothScratch {  // 256-byte aligned parts
  int64_t* k;       // [n,3] the lattice position
  u64* S;           // [n,3] the accumulator of a step; after the last step the summed face normals
  u64* open;        // [n]
  uint32_t* deg;    // [n]
  int32_t* flag;    // [n] 1 = in range
  int32_t* stats;   // [5] when the caller takes none
  size_t bytes;
};

SmoothScratch carve(void* base, int n) {
  SmoothScratch s;
  Carver c(base);
  s.k = c.take<int64_t>((size_t)n * 3);
  s.S = c.take<u64>((size_t)n * 3);
  s.open = c.take<u64>((size_t)n);
  s.deg = c.take<uint32_t>((size_t)n);
  s.flag = c.take<int32_t>((size_t)n);
  s.stats = c.take<int32_t>(64);
  s.bytes = c.bytes;
  return s;
}

// grid max(ceil(n / 256), 1)
__global__ void __launch_bounds__(kTileThreads) smooth_quantise_kernel(SmoothParams p, SmoothScratch c, int32_t* __restrict__ stats) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 5) stats[threadIdx.x] = 0;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  int64_t k[3] = {0, 0, 0};
  const bool in_range = smooth_quantise(p.xyz[i * 3], p.xyz[i * 3 + 1], p.xyz[i * 3 + 2], p.step, k);
  c.flag[i] = in_range ? 1 : 0;
  c.deg[i] = 0;
  c.open[i] = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c.k[i * 3 + a] = k[a];
    c.S[i * 3 + a] = 0;
  }
}

// grid ceil(nf / 256); no thread leaves before the ballots
__global__ void __launch_bounds__(kTileThreads) smooth_topology_kernel(SmoothParams p, SmoothScratch c, int32_t* __restrict__ stats) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  int kind = 0;
  if (f < live_count(p.in_face_count, p.B, p.nf)) {
    const int n = live_count(p.in_count, p.B, p.n);
    const int v[3] = {p.faces[f * 3], p.faces[f * 3 + 1], p.faces[f * 3 + 2]};
    kind = smooth_face_kind(v[0], v[1], v[2], n, c.flag);
    if (kind == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        atomicAdd(c.deg + v[j], 2u);
        atomicAdd(c.open + v[j], (u64)smooth_open_term(v[(j + 1) % 3], v[(j + 2) % 3]));
      }
    }
  }
  wave_count_add(kind == 1, stats);
  wave_count_add(kind == 2, stats + 1);
}

// the sum of x over the wave, in every lane
__device__ __forceinline__ u64 wave_sum(u64 x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += (u64)__shfl_xor((long long)x, d, 64);
  return x;
}

// grid ceil(nf / 256). kCross: the summed face normals instead of the neighbour sums. No thread leaves before the ballots.
template <bool kCross>
__global__ void __launch_bounds__(kTileThreads) smooth_accumulate_kernel(SmoothParams p, SmoothScratch c) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool live = false;
  int v[3] = {-1, -1, -1};
  u64 add[3][3] = {};  // [corner][axis]
  if (f < live_count(p.in_face_count, p.B, p.nf)) {
    const int n = live_count(p.in_count, p.B, p.n);
    v[0] = p.faces[f * 3]; v[1] = p.faces[f * 3 + 1]; v[2] = p.faces[f * 3 + 2];
    live = smooth_face_kind(v[0], v[1], v[2], n, c.flag) == 0;
    if (live) {
      int64_t k[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < 3; ++a) k[j][a] = c.k[(long)v[j] * 3 + a];
      if (kCross) {
        uint64_t x[3];
        smooth_cross(k[0], k[1], k[2], x);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int a = 0; a < 3; ++a) add[j][a] = x[a];
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int a = 0; a < 3; ++a) add[j][a] = (u64)k[(j + 1) % 3][a] + (u64)k[(j + 2) % 3][a];
      }
    }
  }
  const u64 act = __ballot(live);
  if (!act) return;  // the whole wave
  const int leader = __ffsll((long long)act) - 1;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int first = __shfl(v[j], leader, 64);
    const bool shared = __ballot(live && v[j] == first) == act && __popcll(act) > 1;
    if (shared) {  // every live lane names this row: one sum across the wave, one add each axis (the other lanes hold zeros)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const u64 sum = wave_sum(add[j][a]);
        if (lane == leader) atomicAdd(c.S + (long)v[j] * 3 + a, sum);
      }
    } else if (live) {
#pragma unroll
      for (int a = 0; a < 3; ++a) atomicAdd(c.S + (long)v[j] * 3 + a, add[j][a]);
    }
  }
}

// grid ceil(n / 256)
__global__ void __launch_bounds__(kTileThreads) smooth_update_kernel(SmoothParams p, SmoothScratch c, double factor) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const uint32_t deg = c.deg[i];
  const bool pinned = smooth_pinned(deg, c.open[i], c.flag[i] != 0, p.pin_boundary);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!pinned) c.k[i * 3 + a] = smooth_step_axis((int64_t)c.S[i * 3 + a], deg, c.k[i * 3 + a], factor);
    c.S[i * 3 + a] = 0;
  }
}

// grid ceil(n / 256); no thread leaves before the ballots
__global__ void __launch_bounds__(kTileThreads) smooth_write_kernel(SmoothParams p, SmoothScratch c, int32_t* __restrict__ stats) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  bool outside = false, open = false, moved = false;
  if (i < live_count(p.in_count, p.B, p.n)) {
    const float x[3] = {p.xyz[i * 3], p.xyz[i * 3 + 1], p.xyz[i * 3 + 2]};
    int64_t k0[3] = {0, 0, 0}, k[3];
    const bool in_range = smooth_quantise(x[0], x[1], x[2], p.step, k0);
    const uint32_t deg = c.deg[i];
#pragma unroll
    for (int a = 0; a < 3; ++a) k[a] = c.k[i * 3 + a];
    outside = !in_range;
    open = deg > 0 && c.open[i] != 0;
    moved = in_range && (k[0] != k0[0] || k[1] != k0[1] || k[2] != k0[2]);
    if (i < p.capacity) {
      if (p.xyz_out) {
#pragma unroll
        for (int a = 0; a < 3; ++a) p.xyz_out[i * 3 + a] = moved ? smooth_position(k[a], p.step) : x[a];
      }
      if (p.normals_out) {
        const int64_t nrm[3] = {(int64_t)c.S[i * 3], (int64_t)c.S[i * 3 + 1], (int64_t)c.S[i * 3 + 2]};
        float out[3];
        smooth_normal(deg, nrm, out);
#pragma unroll
        for (int a = 0; a < 3; ++a) p.normals_out[i * 3 + a] = out[a];
      }
    }
  }
  wave_count_add(outside, stats + 2);
  wave_count_add(open, stats + 3);
  wave_count_add(moved, stats + 4);
}

}  // namespace

size_t smooth_scratch_bytes(int n) { return carve(nullptr, n > 0 ? n : 0).bytes; }

int launch_smooth_mesh(const SmoothParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "smoothing takes fewer than 2^30 rows, got %d", p.n);
  if (p.nf < 0 || p.nf >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "smoothing takes fewer than 2^30 faces, got %d", p.nf);
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "smoothing of %d views", p.B);
  if (!(p.step > 0.f) || !std::isfinite(p.step)) MD_FAIL(MD_ERR_INVALID_ARG, "step = %g: must be finite and > 0", (double)p.step);
  if (!(p.lambda > 0.f && p.lambda <= 1.f)) MD_FAIL(MD_ERR_INVALID_ARG, "lambda = %g: must lie in (0, 1]", (double)p.lambda);
  if (!(p.mu >= -1.f && p.mu <= 0.f)) MD_FAIL(MD_ERR_INVALID_ARG, "mu = %g: must lie in [-1, 0]", (double)p.mu);
  if (p.iterations < 1 || p.iterations > 1024) MD_FAIL(MD_ERR_INVALID_ARG, "iterations = %d: must lie in 1..1024", p.iterations);
  if (p.capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: a negative capacity");
  if (p.n > 0 && !p.xyz) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: the rows are null");
  if (p.nf > 0 && !p.faces) MD_FAIL(MD_ERR_INVALID_ARG, "smoothing: the faces are null");
  const int n = p.n, nf = p.nf;
  const SmoothScratch c = carve(scratch, n);
  int32_t* stats = p.stats ? p.stats : c.stats;
  const unsigned rows_grid = (unsigned)((n + kTileThreads - 1) / kTileThreads), faces_grid = (unsigned)((nf + kTileThreads - 1) / kTileThreads);
  hipLaunchKernelGGL(smooth_quantise_kernel, dim3(std::max(rows_grid, 1u)), dim3(kTileThreads), 0, s, p, c, stats);
  MD_HIP(hipGetLastError());
  if (nf > 0) {
    hipLaunchKernelGGL(smooth_topology_kernel, dim3(faces_grid), dim3(kTileThreads), 0, s, p, c, stats);
    MD_HIP(hipGetLastError());
  }
  if (n == 0) return MD_OK;
  if (nf > 0) {
    const int steps = p.mu != 0.f ? 2 * p.iterations : p.iterations;
    for (int t = 0; t < steps; ++t) {
      const double factor = (double)((p.mu != 0.f && (t & 1)) ? p.mu : p.lambda);
      hipLaunchKernelGGL(smooth_accumulate_kernel<false>, dim3(faces_grid), dim3(kTileThreads), 0, s, p, c);
      MD_HIP(hipGetLastError());
      hipLaunchKernelGGL(smooth_update_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, c, factor);
      MD_HIP(hipGetLastError());
    }
    if (p.normals_out) {
      hipLaunchKernelGGL(smooth_accumulate_kernel<true>, dim3(faces_grid), dim3(kTileThreads), 0, s, p, c);
      MD_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(smooth_write_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, c, stats);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
