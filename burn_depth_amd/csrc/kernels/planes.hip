// RANSAC plane extraction from a point list for gfx950 (md_op_fit_planes, md_infer_points_planes; DESIGN 12.11, include/mi_depth.h
// states the contract): up to P planes, one per round; a round draws Hh triples from the live rows, counts the live rows within
// `tol` of every triple's plane, and the plane with the largest count (ties: the smallest hypothesis) takes its inliers out of
// the live set. Selection only: a count is an integer sum of an f32 predicate and the winner an arg-max with a fixed tie rule.
// Contraction is off in the whole file (Makefile); the float steps are planes_math.h's, which pipeline.fit_planes restates.
//
// reset, init (label -1 / -2, dropped), then per round seven launches, all of them enqueued whatever the rounds before found:
//   classify   the live rows (label -1) as ballot words and tile counts (tile_compact.h)
//   scan       one workgroup: the tile offsets; offsets[tiles] = M, the live rows of the round
//   scatter    live[rank] = row: the live index in ascending row order
//   hypothesis one thread per h: three mixed positions of the live index, the plane of those rows, or the plane nothing is near
//              (n = 0, d = inf) when the triple is invalid, the round has fewer than 3 live rows or an earlier round failed
//   count      the hot one: every live row against every hypothesis (below)
//   winner     one workgroup: arg-max of count << 32 | ~h; writes the round's outputs, or raises the failed flag
//   label      the winner's inliers get the round as label
// and with mode 1 / 2 a classify on the labels and voxel thinning's scan / scatter (launch_list_compact).
// No thread waits on another. Vector stores and integer atomics only.
#include <algorithm>
#include <cmath>

#include "planes_math.h"
#include "tile_compact.h"

namespace md {

namespace {

enum { kFailed = 0, kDroppedHome = 1, kWinner = 2 };  // words of the state

constexpr int kCountTileRows = kTileThreads * kPlaneCountRows;  // live rows of one pass of a count workgroup
constexpr int kCountMaxGrid = 1024;                             // its workgroups stride over the tiles beyond that

struct PlanesScratch {  // the parts of the scratch buffer, 256-byte aligned
  int32_t* label;       // [n], used when the caller takes no label
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int* live;            // [n] the live index of the round
  Plane* hyp;           // [hypotheses]
  int* hcount;          // [hypotheses]
  int* state;           // [64]
  size_t bytes;
};

PlanesScratch carve(void* base, int n, int hypotheses) {
  const size_t nb = (size_t)tiles_of(n);
  PlanesScratch s;
  Carver c(base);
  s.label = c.take<int32_t>((size_t)n);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.live = c.take<int>((size_t)n);
  s.hyp = c.take<Plane>((size_t)hypotheses);
  s.hcount = c.take<int>((size_t)hypotheses);
  s.state = c.take<int>(64);
  s.bytes = c.bytes;
  return s;
}

// one workgroup: the state and the outputs of a call in which no round has succeeded yet
__global__ void __launch_bounds__(kTileThreads) planes_reset_kernel(PlanesParams p, int* __restrict__ state) {
  const int tid = threadIdx.x;
  if (tid < 64) state[tid] = 0;
  if (tid == 0 && p.dropped) p.dropped[0] = 0;
  if (tid <= p.planes && p.plane_count) p.plane_count[tid] = 0;
  if (tid < p.planes && p.hypothesis) p.hypothesis[tid] = -1;
  if (tid < 4 * p.planes && p.plane) p.plane[tid] = 0.f;
}

// grid ceil(n / 256): a row with a coordinate that is not finite is dropped (-2), every other one is live (-1)
__global__ void __launch_bounds__(kTileThreads) planes_init_kernel(PlanesParams p, int32_t* __restrict__ label, int* __restrict__ state) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= live_count(p.in_count, p.B, p.n)) return;
  const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
  const bool ok = std::isfinite(x) && std::isfinite(y) && std::isfinite(z);
  wave_count_add(!ok, p.dropped ? p.dropped : state + kDroppedHome);  // lanes have already left: the first active one adds
  label[i] = ok ? -1 : -2;
}

// grid tiles. what = 0: the live rows; 1: the rows without a plane (mode 1); 2: the rows of a plane (mode 2)
__global__ void __launch_bounds__(kTileThreads) planes_classify_kernel(PlanesParams p, int what, const int32_t* __restrict__ label,
                                                                   unsigned long long* __restrict__ bits, int* __restrict__ counts) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x;
  const int live = live_count(p.in_count, p.B, p.n);
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool bit = false;
    if (i < live) {
      const int32_t l = label[i];
      bit = what == 2 ? l >= 0 : l == -1;
    }
    n += ballot_step(bit, bits + (long)tile * kTileWords + tile_word(s));
  }
  const int sum = tile_sum(n, wave_n);
  if (threadIdx.x == 0) counts[tile] = sum;
}

__global__ void __launch_bounds__(kTileThreads) planes_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ offsets) {
  __shared__ int part[kTileThreads];
  scan_tile_counts(counts, nb, offsets, part);
}

// grid tiles: live[rank of the row among the live rows] = the row
__global__ void __launch_bounds__(kTileThreads) planes_scatter_kernel(const unsigned long long* __restrict__ bits, const int* __restrict__ offsets,
                                                                  int* __restrict__ live) {
  __shared__ int word_off[kTileWords];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const unsigned long long* words = bits + (long)tile * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const long base = offsets[tile];
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    live[base + word_off[w] + lane_rank(word)] = (int)tile_item(tile, s);  // below M <= n: the bit is only ever set for a live row
  }
}

// grid ceil(Hh / 256). An invalid hypothesis is the plane nothing is near: 0 * q + inf <= tol is false for every finite q, so
// the count kernel needs no valid bit and counts 0.
__global__ void __launch_bounds__(kTileThreads) planes_hypothesis_kernel(PlanesParams p, int round, const int* __restrict__ live,
                                                                     const int* __restrict__ offsets, int nb, Plane* __restrict__ hyp,
                                                                     int* __restrict__ hcount, const int* __restrict__ state) {
  const int h = blockIdx.x * kTileThreads + threadIdx.x;
  if (h >= p.hypotheses) return;
  hcount[h] = 0;
  Plane w{0.f, 0.f, 0.f, INFINITY};
  const int M = offsets[nb];
  if (!state[kFailed] && M >= 3) {
    const int a = live[plane_sample(p.seed, round, h, 0, (uint64_t)M)];
    const int b = live[plane_sample(p.seed, round, h, 1, (uint64_t)M)];
    const int c = live[plane_sample(p.seed, round, h, 2, (uint64_t)M)];
    Plane t;
    if (a != b && a != c && b != c && plane_of_rows(p.xyz + (long)a * 3, p.xyz + (long)b * 3, p.xyz + (long)c * 3, p.axis, p.axis_min_cos, &t)) w = t;
  }
  hyp[h] = w;
}

// One hypothesis against the rows a thread holds: h is the same in every lane, so its plane comes through scalar loads and the
// wave's count is a sum of ballot popcounts on the scalar side. -> that count, the same in every lane.
template <bool kNormals>
__device__ __forceinline__ int count_one(const Plane w, const float (&q)[kPlaneCountRows][3], const float (&m)[kPlaneCountRows][3], float tol,
                                         float min_cos) {
  int c = 0;
#pragma unroll
  for (int r = 0; r < kPlaneCountRows; ++r) {
    bool in = plane_near(w, q[r][0], q[r][1], q[r][2], tol);
    if (kNormals) in = in && plane_normal_agrees(w, m[r][0], m[r][1], m[r][2], min_cos);
    c += (int)__popcll(__ballot(in));
  }
  return c;
}

// The count kernel. grid min(ceil(n / kCountTileRows), kCountMaxGrid); a workgroup strides over tiles of kCountTileRows positions
// of the live index. Per tile a thread gathers kPlaneCountRows rows (and their normals) into registers once, then walks all Hh
// hypotheses, kPlaneCountChunk of them per trip so that their scalar loads are in flight together. A wave's count of a hypothesis
// goes to the workgroup's LDS counters (one ds add per wave, hypothesis and tile, never one per row), and those leave the
// workgroup once, at the end, as one integer atomic per hypothesis with a count. A position at or beyond M holds NaN: near nothing.
template <bool kNormals>
__global__ void __launch_bounds__(kTileThreads) planes_count_kernel(PlanesParams p, const int* __restrict__ live, const int* __restrict__ offsets,
                                                                int nb, const Plane* __restrict__ hyp, int* __restrict__ hcount,
                                                                const int* __restrict__ state) {
  __shared__ int acc[kPlaneHypothesesMax];
  if (state[kFailed]) return;
  const int M = offsets[nb];
  const int tiles = (M + kCountTileRows - 1) / kCountTileRows;
  if ((int)blockIdx.x >= tiles) return;
  const int tid = threadIdx.x, Hh = p.hypotheses;
  const bool first_lane = (tid & 63) == 0;
  for (int h = tid; h < Hh; h += kTileThreads) acc[h] = 0;
  __syncthreads();
  const float tol = p.tol, min_cos = p.normal_min_cos;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    float q[kPlaneCountRows][3], m[kPlaneCountRows][3];
#pragma unroll
    for (int r = 0; r < kPlaneCountRows; ++r) {
      const long j = (long)t * kCountTileRows + r * kTileThreads + tid;
      q[r][0] = q[r][1] = q[r][2] = NAN;
      m[r][0] = m[r][1] = m[r][2] = 0.f;
      if (j < M) {
        const long i = live[j];
        q[r][0] = p.xyz[i * 3]; q[r][1] = p.xyz[i * 3 + 1]; q[r][2] = p.xyz[i * 3 + 2];
        if (kNormals) { m[r][0] = p.normals[i * 3]; m[r][1] = p.normals[i * 3 + 1]; m[r][2] = p.normals[i * 3 + 2]; }
      }
    }
    int h = 0;
    for (; h + kPlaneCountChunk <= Hh; h += kPlaneCountChunk) {
      int c[kPlaneCountChunk];
#pragma unroll
      for (int u = 0; u < kPlaneCountChunk; ++u) c[u] = count_one<kNormals>(hyp[h + u], q, m, tol, min_cos);
#pragma unroll
      for (int u = 0; u < kPlaneCountChunk; ++u)
        if (first_lane && c[u]) atomicAdd(&acc[h + u], c[u]);
    }
    for (; h < Hh; ++h) {
      const int c = count_one<kNormals>(hyp[h], q, m, tol, min_cos);
      if (first_lane && c) atomicAdd(&acc[h], c);
    }
  }
  __syncthreads();
  for (int h = tid; h < Hh; h += kTileThreads)
    if (acc[h]) atomicAdd(hcount + h, acc[h]);
}

// one workgroup: the largest count, among equal counts the smallest h (the key's low word is ~h). A count of at least
// min_inliers >= 3 is a valid hypothesis's: an invalid one counts 0.
__global__ void __launch_bounds__(kTileThreads) planes_winner_kernel(PlanesParams p, int round, const int* __restrict__ offsets, int nb,
                                                                 const Plane* __restrict__ hyp, const int* __restrict__ hcount,
                                                                 int* __restrict__ state) {
  __shared__ unsigned long long best[kTileThreads];
  const int tid = threadIdx.x;
  unsigned long long key = 0ull;
  for (int h = tid; h < p.hypotheses; h += kTileThreads) {
    const unsigned long long k = ((unsigned long long)(unsigned)hcount[h] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
    key = k > key ? k : key;
  }
  best[tid] = key;
  __syncthreads();
  for (int d = kTileThreads / 2; d > 0; d >>= 1) {
    if (tid < d && best[tid + d] > best[tid]) best[tid] = best[tid + d];
    __syncthreads();
  }
  if (tid != 0) return;
  const int count = (int)(best[0] >> 32), h = (int)(0xFFFFFFFFu - (unsigned)best[0]);
  if (state[kFailed] || offsets[nb] < 3 || count < p.min_inliers) {
    state[kFailed] = 1;
    state[kWinner] = -1;
    return;
  }
  state[kWinner] = h;
  const Plane w = hyp[h];
  if (p.plane) {
    float* dst = p.plane + round * 4;
    dst[0] = w.nx; dst[1] = w.ny; dst[2] = w.nz; dst[3] = w.d;
  }
  if (p.hypothesis) p.hypothesis[round] = h;
  if (p.plane_count) {
    p.plane_count[round] = count;
    p.plane_count[p.planes] = round + 1;
  }
}

// grid ceil(n / 256) over the live index: the predicate of the count kernel on the winner's plane
template <bool kNormals>
__global__ void __launch_bounds__(kTileThreads) planes_label_kernel(PlanesParams p, int round, const int* __restrict__ live,
                                                                const int* __restrict__ offsets, int nb, const Plane* __restrict__ hyp,
                                                                const int* __restrict__ state, int32_t* __restrict__ label) {
  const int h = state[kWinner];
  if (h < 0) return;
  const long j = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (j >= offsets[nb]) return;
  const long i = live[j];
  const Plane w = hyp[h];
  bool in = plane_near(w, p.xyz[i * 3], p.xyz[i * 3 + 1], p.xyz[i * 3 + 2], p.tol);
  if (kNormals) in = in && plane_normal_agrees(w, p.normals[i * 3], p.normals[i * 3 + 1], p.normals[i * 3 + 2], p.normal_min_cos);
  if (in) label[i] = round;
}

}  // namespace

size_t planes_scratch_bytes(int n, int hypotheses) { return carve(nullptr, n > 0 ? n : 0, hypotheses > 0 ? hypotheses : 0).bytes; }

int launch_fit_planes(const PlanesParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "plane extraction needs its scratch buffer");
  if (p.n < 0 || p.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "plane extraction takes fewer than 2^30 rows, got %d", p.n);
  if (p.planes < 1 || p.planes > kPlanesMax) MD_FAIL(MD_ERR_INVALID_ARG, "planes %d outside 1..%d", p.planes, kPlanesMax);
  if (p.hypotheses < 1 || p.hypotheses > kPlaneHypothesesMax)
    MD_FAIL(MD_ERR_INVALID_ARG, "hypotheses %d outside 1..%d", p.hypotheses, kPlaneHypothesesMax);
  if (p.normal_min_cos > 0.f && !p.normals) MD_FAIL(MD_ERR_INVALID_ARG, "normal_min_cos > 0 needs the normals rows");
  if (p.B < 1) MD_FAIL(MD_ERR_SHAPE, "plane extraction of %d views", p.B);
  const PlanesScratch v = carve(scratch, p.n, p.hypotheses);
  int32_t* label = p.label ? p.label : v.label;
  const int nb = tiles_of(p.n);
  const unsigned rows_grid = (unsigned)((p.n + kTileThreads - 1) / kTileThreads);
  const unsigned hyp_grid = (unsigned)((p.hypotheses + kTileThreads - 1) / kTileThreads);
  const unsigned count_grid = (unsigned)std::min((p.n + kCountTileRows - 1) / kCountTileRows, kCountMaxGrid);
  const bool nrm = p.normal_min_cos > 0.f;
  hipLaunchKernelGGL(planes_reset_kernel, dim3(1), dim3(kTileThreads), 0, s, p, v.state);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    hipLaunchKernelGGL(planes_init_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, p, label, v.state);
    MD_HIP(hipGetLastError());
  }
  for (int round = 0; round < p.planes; ++round) {
    if (p.n > 0) {
      hipLaunchKernelGGL(planes_classify_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, 0, label, v.bits, v.counts);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(planes_scan_kernel, dim3(1), dim3(kTileThreads), 0, s, v.counts, nb, v.offsets);
    MD_HIP(hipGetLastError());
    if (p.n > 0) {
      hipLaunchKernelGGL(planes_scatter_kernel, dim3(nb), dim3(kTileThreads), 0, s, v.bits, v.offsets, v.live);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(planes_hypothesis_kernel, dim3(hyp_grid), dim3(kTileThreads), 0, s, p, round, v.live, v.offsets, nb, v.hyp, v.hcount, v.state);
    MD_HIP(hipGetLastError());
    if (p.n > 0) {
      if (nrm) hipLaunchKernelGGL(planes_count_kernel<true>, dim3(count_grid), dim3(kTileThreads), 0, s, p, v.live, v.offsets, nb, v.hyp, v.hcount, v.state);
      else hipLaunchKernelGGL(planes_count_kernel<false>, dim3(count_grid), dim3(kTileThreads), 0, s, p, v.live, v.offsets, nb, v.hyp, v.hcount, v.state);
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(planes_winner_kernel, dim3(1), dim3(kTileThreads), 0, s, p, round, v.offsets, nb, v.hyp, v.hcount, v.state);
    MD_HIP(hipGetLastError());
    if (p.n > 0) {
      if (nrm) hipLaunchKernelGGL(planes_label_kernel<true>, dim3(rows_grid), dim3(kTileThreads), 0, s, p, round, v.live, v.offsets, nb, v.hyp, v.state, label);
      else hipLaunchKernelGGL(planes_label_kernel<false>, dim3(rows_grid), dim3(kTileThreads), 0, s, p, round, v.live, v.offsets, nb, v.hyp, v.state, label);
      MD_HIP(hipGetLastError());
    }
  }
  if (p.mode == 0) return MD_OK;
  if (p.n > 0) {
    hipLaunchKernelGGL(planes_classify_kernel, dim3(nb), dim3(kTileThreads), 0, s, p, p.mode, label, v.bits, v.counts);
    MD_HIP(hipGetLastError());
  }
  VoxelParams c;  // the compaction reads the rows, the counts and the outputs; it knows no plane
  c.xyz = p.xyz; c.conf = p.conf; c.rgb = p.rgb; c.normals = p.normals; c.in_count = p.in_count; c.n = p.n; c.B = p.B;
  c.xyz_out = p.xyz_out; c.conf_out = p.conf_out; c.rgb_out = p.rgb_out; c.normals_out = p.normals_out;
  c.index = p.index; c.count = p.count; c.capacity = p.capacity;
  return launch_list_compact(c, nullptr, nullptr, v.bits, v.counts, v.offsets, s);
}

}  // namespace md
