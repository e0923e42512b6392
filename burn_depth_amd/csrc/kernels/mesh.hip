// Triangle mesh of the depth grid for gfx950 (md_op_mesh_grid, md_op_unproject_mesh, md_infer_points_mesh; DESIGN 12.5;
// include/mi_depth.h states the contract). The vertices are the rows of the point path's list; a face is three of them.
// Selection with integer outputs: a triangle is emitted or not from f32 comparisons of one rounded operation per step
// (contraction is off in the whole file, Makefile), so pipeline.mesh_grid restates it in numpy bit for bit.
//
// index: the map pixel -> list row, from the ballot words and workgroup offsets launch_unproject left in its scratch (the scatter
// step of tile_compact.h, for every pixel instead of only the listed ones).
// classify / scan / scatter: tile_compact.h's ordered compaction with a PAIR of ballot words per wave and step, one per triangle
// of the quad (pair = step * 4 + wave, 64 pairs per tile), so the faces keep the (view, row, column, triangle) order without atomics.
#include <climits>

#include "tile_compact.h"

namespace md {

namespace {

// grid (tiles, B) and the tile of points_scatter_kernel: pixel_index [B,H,W] = the true rank of a listed pixel, -1 elsewhere
__global__ void __launch_bounds__(kTileThreads) mesh_index_kernel(int H, int W, const unsigned long long* __restrict__ bits,
                                                              const int* __restrict__ offsets, int32_t* __restrict__ pixel_index) {
  __shared__ int word_off[kTileWords];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const long blk = (long)b * gridDim.x + tile;
  const unsigned long long* words = bits + blk * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const int base = offsets[blk];
  const long hw = (long)H * W;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    if (i >= hw) continue;
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    pixel_index[(long)b * hw + i] = ((word >> lane) & 1ull) ? base + word_off[w] + (int)lane_rank(word) : -1;
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
__global__ void __launch_bounds__(kTileThreads) mesh_classify_kernel(MeshParams p, int wq, long quads, unsigned long long* __restrict__ bits,
                                                                 int* __restrict__ counts) {
  __shared__ int wave_n[kTileWaves];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const long hw = (long)p.H * p.W, blk = (long)b * gridDim.x + tile;
  const int32_t* pi = p.pixel_index + (long)b * hw;
  const float* dv = p.depth + (long)b * hw;
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long q = tile_item(tile, s);
    unsigned m = 0;
    int f[2][3];
    if (q < quads) m = quad_faces(p, pi, dv, wq, q, f);
    unsigned long long* pair = bits + (blk * kTileWords + tile_word(s)) * 2;
    n += ballot_step(m & 1u, pair) + ballot_step(m & 2u, pair + 1);
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[blk] = sum;
}

// one workgroup: offsets[i] = sum of counts[0 .. i), offsets[n] = the total; count[b] = faces of view b, count[B] = total.
// n = 0 (a lattice without quads): every count is 0.
__global__ void __launch_bounds__(kTileThreads) mesh_scan_kernel(const int* __restrict__ counts, int n, int tiles, int B,
                                                             int* __restrict__ offsets, int32_t* __restrict__ count) {
  __shared__ int part[kTileThreads];
  scan_tile_counts(counts, n, offsets, part);
  view_totals(offsets, n, tiles, B, count);
}

__global__ void __launch_bounds__(kTileThreads) mesh_scatter_kernel(MeshParams p, int wq, const unsigned long long* __restrict__ bits,
                                                                const int* __restrict__ offsets) {
  __shared__ int word_off[kTileWords];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const long blk = (long)b * gridDim.x + tile;
  const unsigned long long* words = bits + blk * kTileWords * 2;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid * 2]) + __popcll(words[tid * 2 + 1]), word_off);  // the word pairs
  __syncthreads();
  const long base = offsets[blk];
  if (base >= p.face_capacity) return;  // everything of this workgroup lies beyond the capacity
  const long hw = (long)p.H * p.W;
  const int32_t* pi = p.pixel_index + (long)b * hw;
  const float* dv = p.depth + (long)b * hw;
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long w0 = words[w * 2], w1 = words[w * 2 + 1];
    const unsigned mine = (unsigned)((w0 >> lane) & 1ull) | ((unsigned)((w1 >> lane) & 1ull) << 1);
    if (!mine) continue;
    long idx = base + word_off[w] + lane_rank(w0) + lane_rank(w1);
    const long q = tile_item(tile, s);  // < quads: a bit is only ever set for a quad of the lattice
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
  return up256(nb * kTileWords * 16) + up256(nb * 4) + up256((nb + 1) * 4);
}

int launch_mesh_index(int B, int H, int W, const void* points_scratch, int32_t* pixel_index, hipStream_t s) {
  if (!points_scratch || !pixel_index) MD_FAIL(MD_ERR_INVALID_ARG, "mesh index: no scratch of the list or no output");
  // the layout points_scratch_bytes describes: bit mask | block counts | block offsets
  const int tiles = tiles_of((long)H * W);
  const size_t nb = (size_t)B * tiles;
  const size_t b_bits = up256(nb * kTileWords * 8), b_counts = up256(nb * 4);
  if (b_bits + b_counts + up256((nb + 1) * 4) != points_scratch_bytes(B, H, W)) MD_FAIL(MD_ERR_UNSUPPORTED, "mesh index: not the scratch layout of the list");
  const unsigned long long* bits = (const unsigned long long*)points_scratch;
  const int* offsets = (const int*)((const char*)points_scratch + b_bits + b_counts);
  hipLaunchKernelGGL(mesh_index_kernel, dim3(tiles, B), dim3(kTileThreads), 0, s, H, W, bits, offsets, pixel_index);
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
  int* counts = (int*)((char*)scratch + up256(nb * kTileWords * 16));
  int* offsets = (int*)((char*)counts + up256(nb * 4));
  const dim3 grid(l.tiles, p.B);
  if (l.tiles > 0) {
    hipLaunchKernelGGL(mesh_classify_kernel, grid, dim3(kTileThreads), 0, s, p, l.wq, l.quads, bits, counts);
    MD_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kTileThreads), 0, s, counts, (int)nb, l.tiles, p.B, offsets, p.face_count);
  MD_HIP(hipGetLastError());
  if (!p.faces || p.face_capacity <= 0 || l.tiles == 0) return MD_OK;  // counts only
  hipLaunchKernelGGL(mesh_scatter_kernel, grid, dim3(kTileThreads), 0, s, p, l.wq, bits, offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
