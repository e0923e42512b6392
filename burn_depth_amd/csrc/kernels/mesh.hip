// Triangle mesh of the depth grid for gfx950 (md_op_mesh_grid, md_op_unproject_mesh, md_infer_points_mesh; DESIGN 12.5;
// include/mi_depth.h states the contract). The vertices are the rows of the point path's list; a face is three of them.
// Selection with integer outputs: a triangle is emitted or not from f32 comparisons of one rounded operation per step
// (contraction is off in the whole file, Makefile), so pipeline.mesh_grid restates it in numpy bit for bit.
//
// index: the map pixel -> list row, from the ballot words and workgroup offsets launch_unproject left in its scratch (the rank
// points_scatter_kernel computes, for every pixel instead of only the listed ones).
// classify / scan / scatter: the point path's ordered compaction with two ballot words per wave and step, one per triangle of
// the quad, so the faces keep the (view, row, column, triangle) order without atomics.
#include <climits>

#include "ops.h"

namespace md {

namespace {

constexpr int kThreads = 256;             // 4 waves of 64
constexpr int kSteps = 16;                // pixels (index) or quads (faces) per thread
constexpr int kTile = kThreads * kSteps;  // 4096 per workgroup: item = tile * 4096 + step * 256 + thread
constexpr int kWords = kTile / 64;        // ballot words (index) or word pairs (faces) per workgroup: word = step * 4 + wave

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }
inline int tiles_of(long n) { return (int)((n + kTile - 1) / kTile); }

// wave 0: word_off[w] = the sum of c over the words before w (word order = item order); call with tid < 64
__device__ __forceinline__ void scan_words(int c, int lane, int* word_off) {
  int incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  word_off[lane] = incl - c;
}

// grid (tiles, B) and the tile of points_scatter_kernel: pixel_index [B,H,W] = the true rank of a listed pixel, -1 elsewhere
__global__ void __launch_bounds__(kThreads) mesh_index_kernel(int H, int W, const unsigned long long* __restrict__ bits,
                                                              const int* __restrict__ offsets, int32_t* __restrict__ pixel_index) {
  __shared__ int word_off[kWords];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long blk = (long)b * gridDim.x + tile;
  const unsigned long long* words = bits + blk * kWords;
  if (tid < kWords) scan_words(__popcll(words[tid]), lane, word_off);
  __syncthreads();
  const int base = offsets[blk];
  const long hw = (long)H * W;
  for (int s = 0; s < kSteps; ++s) {
    const long i = (long)tile * kTile + s * kThreads + tid;
    if (i >= hw) continue;
    const int w = s * (kThreads / 64) + wave;
    const unsigned long long word = words[w];
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
    pixel_index[(long)b * hw + i] = ((word >> lane) & 1ull) ? base + word_off[w] + (int)below : -1;
  }
}

__device__ __forceinline__ bool edge_passes(float rtol, float dx, float dy) {
  if (rtol == 0.f) return true;
  return fabsf(dx - dy) <= rtol * fminf(dx, dy);
}

// The contract for quad q of view b's lattice: f[0], f[1] = the rows of its first and second triangle;
// -> bit 0 / bit 1 = that triangle is emitted. classify and scatter both call this, so a rank always has its face.
__device__ __forceinline__ unsigned quad_faces(const MeshParams& p, const int32_t* __restrict__ pi, const float* __restrict__ dv, int wq,
                                               long q, int f[2][3]) {
  const int i = (int)(q / wq), j = (int)(q % wq);
  const long a = (long)i * p.stride * p.W + (long)j * p.stride, c = a + (long)p.stride * p.W;  // b = a + stride, d = c + stride
  const int ia = pi[a], ib = pi[a + p.stride], ic = pi[c], id = pi[c + p.stride];
  const float da = dv[a], db = dv[a + p.stride], dc = dv[c], dd = dv[c + p.stride];
  const bool ua = ia >= 0 && ia < p.limit, ub = ib >= 0 && ib < p.limit, uc = ic >= 0 && ic < p.limit, ud = id >= 0 && id < p.limit;
  bool ad;
  if (ua && ub && uc && ud) ad = fabsf(da - dd) <= fabsf(db - dc);
  else ad = ua && ud;
  const float r = p.max_rtol;
  unsigned m = 0;
  if (ad) {  // (a, c, d), (a, d, b)
    f[0][0] = ia; f[0][1] = ic; f[0][2] = id;
    f[1][0] = ia; f[1][1] = id; f[1][2] = ib;
    const bool diag = ua && ud && edge_passes(r, da, dd);
    if (diag && uc && edge_passes(r, da, dc) && edge_passes(r, dc, dd)) m |= 1u;
    if (diag && ub && edge_passes(r, dd, db) && edge_passes(r, db, da)) m |= 2u;
  } else {   // (a, c, b), (b, c, d)
    f[0][0] = ia; f[0][1] = ic; f[0][2] = ib;
    f[1][0] = ib; f[1][1] = ic; f[1][2] = id;
    const bool diag = ub && uc && edge_passes(r, db, dc);
    if (diag && ua && edge_passes(r, da, dc) && edge_passes(r, db, da)) m |= 1u;
    if (diag && ud && edge_passes(r, dc, dd) && edge_passes(r, dd, db)) m |= 2u;
  }
  return m;
}

// grid (tiles of the quad lattice, B): bits [B][tiles][64][2] (first, second triangle), counts [B * tiles]
__global__ void __launch_bounds__(kThreads) mesh_classify_kernel(MeshParams p, int wq, long quads, unsigned long long* __restrict__ bits,
                                                                 int* __restrict__ counts) {
  __shared__ int wave_n[kThreads / 64];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long hw = (long)p.H * p.W, blk = (long)b * gridDim.x + tile;
  const int32_t* pi = p.pixel_index + (long)b * hw;
  const float* dv = p.depth + (long)b * hw;
  int n = 0;
  for (int s = 0; s < kSteps; ++s) {
    const long q = (long)tile * kTile + s * kThreads + tid;
    unsigned m = 0;
    int f[2][3];
    if (q < quads) m = quad_faces(p, pi, dv, wq, q, f);
    const unsigned long long w0 = __ballot(m & 1u), w1 = __ballot(m & 2u);
    if (lane == 0) {
      unsigned long long* dst = bits + (blk * kWords + s * (kThreads / 64) + wave) * 2;
      dst[0] = w0; dst[1] = w1;
    }
    n += __popcll(w0) + __popcll(w1);  // the same in every lane of the wave
  }
  if (lane == 0) wave_n[wave] = n;
  __syncthreads();
  if (tid == 0) counts[blk] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// one workgroup: offsets[i] = sum of counts[0 .. i), offsets[n] = the total; count[b] = faces of view b, count[B] = total.
// n = 0 (a lattice without quads): every count is 0.
__global__ void __launch_bounds__(kThreads) mesh_scan_kernel(const int* __restrict__ counts, int n, int tiles, int B,
                                                             int* __restrict__ offsets, int32_t* __restrict__ count) {
  __shared__ int part[kThreads];
  const int tid = threadIdx.x;
  const int per = (n + kThreads - 1) / kThreads;
  const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += counts[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {  // inclusive scan of the 256 chunk sums
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
  if (tid == kThreads - 1) offsets[n] = part[tid];
  __syncthreads();  // the offsets this workgroup wrote are visible to all of it
  for (int b = tid; b < B; b += kThreads) count[b] = offsets[(b + 1) * tiles] - offsets[b * tiles];
  if (tid == 0) count[B] = offsets[n];
}

__global__ void __launch_bounds__(kThreads) mesh_scatter_kernel(MeshParams p, int wq, const unsigned long long* __restrict__ bits,
                                                                const int* __restrict__ offsets) {
  __shared__ int word_off[kWords];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long blk = (long)b * gridDim.x + tile;
  const unsigned long long* words = bits + blk * kWords * 2;
  if (tid < kWords) scan_words(__popcll(words[tid * 2]) + __popcll(words[tid * 2 + 1]), lane, word_off);  // wave 0: the word pairs
  __syncthreads();
  const long base = offsets[blk];
  if (base >= p.face_capacity) return;  // everything of this workgroup lies beyond the capacity
  const long hw = (long)p.H * p.W;
  const int32_t* pi = p.pixel_index + (long)b * hw;
  const float* dv = p.depth + (long)b * hw;
  for (int s = 0; s < kSteps; ++s) {
    const int w = s * (kThreads / 64) + wave;
    const unsigned long long w0 = words[w * 2], w1 = words[w * 2 + 1];
    const unsigned mine = (unsigned)((w0 >> lane) & 1ull) | ((unsigned)((w1 >> lane) & 1ull) << 1);
    if (!mine) continue;
    const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(w0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)w0, 0u)) +
                           __builtin_amdgcn_mbcnt_hi((unsigned)(w1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)w1, 0u));
    long idx = base + word_off[w] + below;
    const long q = (long)tile * kTile + s * kThreads + tid;  // < quads: a bit is only ever set for a quad of the lattice
    int f[2][3];
    quad_faces(p, pi, dv, wq, q, f);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (!((mine >> t) & 1u)) continue;
      if (idx < p.face_capacity) {
        int32_t* dst = p.faces + idx * 3;
        dst[0] = f[t][0]; dst[1] = f[t][1]; dst[2] = f[t][2];
      }
      ++idx;
    }
  }
}

struct Lattice {
  int hs, ws, wq, tiles;
  long quads;
};
Lattice lattice_of(int H, int W, int stride) {
  Lattice l;
  l.hs = (H + stride - 1) / stride;
  l.ws = (W + stride - 1) / stride;
  l.wq = l.ws - 1;
  l.quads = (long)(l.hs - 1) * l.wq;
  l.tiles = tiles_of(l.quads);
  return l;
}

}  // namespace

size_t mesh_scratch_bytes(int B, int H, int W, int stride) {
  const size_t nb = (size_t)B * lattice_of(H, W, stride).tiles;
  return up256(nb * kWords * 16) + up256(nb * 4) + up256((nb + 1) * 4);
}

int launch_mesh_index(int B, int H, int W, const void* points_scratch, int32_t* pixel_index, hipStream_t s) {
  if (!points_scratch || !pixel_index) MD_FAIL(MD_ERR_INVALID_ARG, "mesh index: no scratch of the list or no output");
  // the layout points_scratch_bytes describes: bit mask | block counts | block offsets
  const int tiles = tiles_of((long)H * W);
  const size_t nb = (size_t)B * tiles;
  const size_t b_bits = up256(nb * kWords * 8), b_counts = up256(nb * 4);
  if (b_bits + b_counts + up256((nb + 1) * 4) != points_scratch_bytes(B, H, W)) MD_FAIL(MD_ERR_UNSUPPORTED, "mesh index: not the scratch layout of the list");
  const unsigned long long* bits = (const unsigned long long*)points_scratch;
  const int* offsets = (const int*)((const char*)points_scratch + b_bits + b_counts);
  hipLaunchKernelGGL(mesh_index_kernel, dim3(tiles, B), dim3(kThreads), 0, s, H, W, bits, offsets, pixel_index);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

int launch_mesh_grid(const MeshParams& p, void* scratch, hipStream_t s) {
  if (!p.face_count) return MD_OK;  // faces need the counts: nothing was asked for
  if (!scratch || !p.depth || !p.pixel_index) MD_FAIL(MD_ERR_INVALID_ARG, "mesh grid: a null buffer");
  if (p.B <= 0 || p.H <= 0 || p.W <= 0 || p.stride < 1 || (long)p.B * p.H * p.W >= (1l << 30))
    MD_FAIL(MD_ERR_SHAPE, "mesh grid: invalid shape [%d,%d,%d] / stride %d", p.B, p.H, p.W, p.stride);
  const Lattice l = lattice_of(p.H, p.W, p.stride);
  const size_t nb = (size_t)p.B * l.tiles;
  unsigned long long* bits = (unsigned long long*)scratch;
  int* counts = (int*)((char*)scratch + up256(nb * kWords * 16));
  int* offsets = (int*)((char*)counts + up256(nb * 4));
  const dim3 grid(l.tiles, p.B);
  if (l.tiles > 0) {
    hipLaunchKernelGGL(mesh_classify_kernel, grid, dim3(kThreads), 0, s, p, l.wq, l.quads, bits, counts);
    MD_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kThreads), 0, s, counts, (int)nb, l.tiles, p.B, offsets, p.face_count);
  MD_HIP(hipGetLastError());
  if (!p.faces || p.face_capacity <= 0 || l.tiles == 0) return MD_OK;  // counts only
  hipLaunchKernelGGL(mesh_scatter_kernel, grid, dim3(kThreads), 0, s, p, l.wq, bits, offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
