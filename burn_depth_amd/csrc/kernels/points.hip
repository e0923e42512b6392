// Point path kernels for gfx950 (md_op_unproject, md_infer_points): depth + pinhole cameras -> a dense world / camera space
// point map with its validity mask, and the same points as an ordered, compacted cloud. HBM-bound: three launches
// (classify, scan, scatter). Contraction is off in the whole file (Makefile): every step below is one rounded f32 operation,
// in the order pipeline.unproject_depth restates in numpy, so the two agree bit for bit.
//
// The normals forms (md_op_unproject_normals) are compile-time forms of classify and scatter: the same loops with
// the surface normal of the pixel's one ring (pixel_normal) and the grazing-angle test in them. The forms without normals are
// the kernels they were before and compile to the same instructions.
//
// The list keeps the (view, row, column) order without atomics: tile_compact.h's ordered compaction (classify, scan, scatter)
// over a grid of (tiles, B) workgroups, a tile's words at bits + (b * tiles + tile) * 64.
#include <cfloat>
#include <cmath>

#include "points_math.h"
#include "tile_compact.h"

namespace md {

namespace {

// a neighbour that is not finite or <= 0 is ignored
__device__ __forceinline__ bool edge_ok(float d, float dn, float rtol) {
  if (!isfinite(dn) || !(dn > 0.f)) return true;
  return fabsf(d - dn) <= rtol * fminf(d, dn);
}

__device__ __forceinline__ bool pixel_valid(const PointsParams& p, const float* __restrict__ dv, const float* __restrict__ cv, int v, int u,
                                            float d) {
  if (!isfinite(d) || !(d >= p.dmin) || !(d <= p.dmax)) return false;
  const long i = (long)v * p.W + u;
  if (cv && !(cv[i] >= p.conf_min)) return false;
  if (p.edge_rtol > 0.f) {
    if (v > 0 && !edge_ok(d, dv[i - p.W], p.edge_rtol)) return false;
    if (v + 1 < p.H && !edge_ok(d, dv[i + p.W], p.edge_rtol)) return false;
    if (u > 0 && !edge_ok(d, dv[i - 1], p.edge_rtol)) return false;
    if (u + 1 < p.W && !edge_ok(d, dv[i + 1], p.edge_rtol)) return false;
  }
  return true;
}

// ---- surface normal (include/mi_depth.h states the contract) ----
// a neighbour inside the image whose depth dn the normal of a pixel of depth d may use
__device__ __forceinline__ bool neighbour_usable(const PointsParams& p, const float* __restrict__ cv, long j, float d, float dn) {
  if (!isfinite(dn) || !(dn >= p.dmin) || !(dn <= p.dmax)) return false;
  if (cv && !(cv[j] >= p.conf_min)) return false;
  if (p.edge_rtol > 0.f && !(fabsf(d - dn) <= p.edge_rtol * fminf(d, dn))) return false;
  return true;
}

// Camera-space unit normal of pixel (v, u) with a valid depth d: the sum of the cross products of the edge vectors to the usable
// neighbours, pairs (S,E), (E,N), (N,W), (W,S), summed from the first usable pair on. false = not defined, n = (0,0,0).
// cosv = -n.p / |p|, the cosine between the normal and the ray back to the camera. With x right, y down, z forward every
// cross points at the camera: for positive depths the sign of p.(e_a x e_b) is the sign of det(r_c, r_a, r_b) of the three
// pixel rays, whatever the depths, so cosv > 0 in exact arithmetic and no flip step exists.
__device__ __forceinline__ bool pixel_normal(const PointsParams& p, const Camera& cam, const float* __restrict__ dv,
                                             const float* __restrict__ cv, int v, int u, float d, float* n, float* cosv) {
  n[0] = n[1] = n[2] = 0.f;
  *cosv = 0.f;
  const long i = (long)v * p.W + u;
  float pc[3];
  unproject(cam, 0, p.off, v, u, d, pc);
  const int nv[4] = {0, 1, 0, -1}, nu[4] = {1, 0, -1, 0};  // E, S, W, N
  float e[4][3];
  bool use[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int vn = v + nv[k], un = u + nu[k];
    use[k] = false;
    e[k][0] = e[k][1] = e[k][2] = 0.f;
    if (vn < 0 || vn >= p.H || un < 0 || un >= p.W) continue;
    const long j = i + (long)nv[k] * p.W + nu[k];
    const float dn = dv[j];
    if (!neighbour_usable(p, cv, j, d, dn)) continue;
    float q[3];
    unproject(cam, 0, p.off, vn, un, dn, q);
    e[k][0] = q[0] - pc[0]; e[k][1] = q[1] - pc[1]; e[k][2] = q[2] - pc[2];
    use[k] = true;
  }
  const int pa[4] = {1, 0, 3, 2}, pb[4] = {0, 3, 2, 1};  // (S,E), (E,N), (N,W), (W,S)
  float m[3] = {0.f, 0.f, 0.f};
  bool have = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!use[pa[k]] || !use[pb[k]]) continue;
    const float* a = e[pa[k]];
    const float* b = e[pb[k]];
    const float cx = (a[1] * b[2]) - (a[2] * b[1]);
    const float cy = (a[2] * b[0]) - (a[0] * b[2]);
    const float cz = (a[0] * b[1]) - (a[1] * b[0]);
    if (have) {
      m[0] = m[0] + cx; m[1] = m[1] + cy; m[2] = m[2] + cz;
    } else {
      m[0] = cx; m[1] = cy; m[2] = cz;
      have = true;
    }
  }
  if (!have) return false;
  const float len2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  if (!isfinite(len2) || !(len2 >= FLT_MIN)) return false;
  const float s = sqrtf(len2);
  n[0] = m[0] / s; n[1] = m[1] / s; n[2] = m[2] / s;
  *cosv = -((n[0] * pc[0] + n[1] * pc[1]) + n[2] * pc[2]) / sqrtf((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
  return true;
}

// world = 1: n_w = R^T n in unproject's operation order, not renormalised
__device__ __forceinline__ void normal_out(const Camera& c, int world, const float* n, float* out) {
  if (world) {
    out[0] = (c.r[0] * n[0] + c.r[3] * n[1]) + c.r[6] * n[2];
    out[1] = (c.r[1] * n[0] + c.r[4] * n[1]) + c.r[7] * n[2];
    out[2] = (c.r[2] * n[0] + c.r[5] * n[1]) + c.r[8] * n[2];
  } else {
    out[0] = n[0]; out[1] = n[1]; out[2] = n[2];
  }
}

// the trailing kernel argument of a normals form; a form without normals has none
__device__ __forceinline__ NormalsParams normals_of() { return NormalsParams(); }
__device__ __forceinline__ NormalsParams normals_of(const NormalsParams& q) { return q; }

// grid (tiles, B). bits [B][tiles * 64] and counts [B * tiles] are written only when the list is wanted.
// Q = {NormalsParams}: the normals form (q.min_cos enters the validity, q.normal_map is written beside the point map).
// Q = {}: the form without normals, with the arguments, and so the instructions, the kernel had before the normals existed.
template <class... Q>
__global__ void __launch_bounds__(kTileThreads) points_classify_kernel(PointsParams p, unsigned long long* __restrict__ bits,
                                                                   int* __restrict__ counts, Q... qs) {
  constexpr bool kN = sizeof...(Q) == 1;
  const NormalsParams q = normals_of(qs...);
  __shared__ int wave_n[kTileWaves];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const long hw = (long)p.H * p.W, blk = (long)b * gridDim.x + tile;
  const float* dv = p.depth + (long)b * hw;
  const float* cv = p.conf ? p.conf + (long)b * hw : nullptr;
  const bool dense = p.point_map || p.mask || (kN && q.normal_map);
  const bool list = p.count != nullptr;
  Camera cam;
  if (kN || p.point_map) cam = load_camera(p.K, p.focal, p.world ? p.E : nullptr, p.H, p.W, b);
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool ok = false, in_list = false;
    if (i < hw) {
      const int v = (int)(i / p.W), u = (int)(i % p.W);
      const float d = dv[i];
      ok = pixel_valid(p, dv, cv, v, u, d);
      float nrm[3] = {0.f, 0.f, 0.f};
      if constexpr (kN) {
        if (ok) {
          float nc[3], cosv;
          const bool defined = pixel_normal(p, cam, dv, cv, v, u, d, nc, &cosv);
          if (q.min_cos > 0.f && !(defined && cosv >= q.min_cos)) ok = false;
          else if (defined) normal_out(cam, p.world, nc, nrm);
        }
      }
      in_list = ok && u % p.stride == 0 && v % p.stride == 0;
      if (dense) {
        const long o = (long)b * hw + i;
        if (p.mask) p.mask[o] = ok ? 1 : 0;
        if (p.point_map) {
          float q[3] = {0.f, 0.f, 0.f};
          if (ok) unproject(cam, p.world, p.off, v, u, d, q);
          float* dst = p.point_map + o * 3;
          dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
        }
        if constexpr (kN) {
          if (q.normal_map) {
            float* dst = q.normal_map + o * 3;
            dst[0] = nrm[0]; dst[1] = nrm[1]; dst[2] = nrm[2];
          }
        }
      }
    }
    if (list) n += ballot_step(in_list, bits + blk * kTileWords + tile_word(s));
  }
  if (!list) return;
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[blk] = sum;
}

// one workgroup: offsets[i] = sum of counts[0 .. i), offsets[n] = the total; count[b] = points of view b, count[B] = total
__global__ void __launch_bounds__(kTileThreads) points_scan_kernel(const int* __restrict__ counts, int n, int tiles, int B,
                                                               int* __restrict__ offsets, int32_t* __restrict__ count) {
  __shared__ int part[kTileThreads];
  scan_tile_counts(counts, n, offsets, part);
  view_totals(offsets, n, tiles, B, count);
}

// Q = {NormalsParams}: the normals form writes q.normals; it recomputes the normal of a listed pixel with classify's own function, so a list
// row equals the dense map at its pixel
template <class... Q>
__global__ void __launch_bounds__(kTileThreads) points_scatter_kernel(PointsParams p, const unsigned long long* __restrict__ bits,
                                                                  const int* __restrict__ offsets, Q... qs) {
  constexpr bool kN = sizeof...(Q) == 1;
  const NormalsParams q = normals_of(qs...);
  __shared__ int word_off[kTileWords];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const long blk = (long)b * gridDim.x + tile;
  const unsigned long long* words = bits + blk * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const long base = offsets[blk];
  if (base >= p.capacity) return;  // everything of this workgroup lies beyond the capacity
  const long hw = (long)p.H * p.W;
  const float* dv = p.depth + (long)b * hw;
  const Camera cam = load_camera(p.K, p.focal, p.world ? p.E : nullptr, p.H, p.W, b);
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    const long idx = base + word_off[w] + lane_rank(word);
    if (idx >= p.capacity) continue;
    const long i = tile_item(tile, s);  // < hw: the bit is only ever set for a pixel of the image
    const int v = (int)(i / p.W), u = (int)(i % p.W);
    if (p.xyz) {
      float q[3];
      unproject(cam, p.world, p.off, v, u, dv[i], q);
      float* dst = p.xyz + idx * 3;
      dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
    }
    const long o = (long)b * hw + i;
    if (p.rgb_out) {
      const uint8_t* src = p.rgb + o * 3;
      uint8_t* dst = p.rgb_out + idx * 3;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    if (p.conf_out) p.conf_out[idx] = p.conf[o];
    if constexpr (kN) {
      if (q.normals) {
        float nc[3], cosv, nrm[3] = {0.f, 0.f, 0.f};
        if (pixel_normal(p, cam, dv, p.conf ? p.conf + (long)b * hw : nullptr, v, u, dv[i], nc, &cosv)) normal_out(cam, p.world, nc, nrm);
        float* dst = q.normals + idx * 3;
        dst[0] = nrm[0]; dst[1] = nrm[1]; dst[2] = nrm[2];
      }
    }
  }
}

}  // namespace

size_t points_scratch_bytes(int B, int H, int W) {
  const size_t nb = (size_t)B * tiles_of((long)H * W);
  return up256(nb * kTileWords * 8) + up256(nb * 4) + up256((nb + 1) * 4);
}

int launch_unproject(const PointsParams& p, void* scratch, hipStream_t s, const NormalsParams* nrm) {
  const NormalsParams q = nrm ? *nrm : NormalsParams();
  // classify needs the normal only for the dense map or the grazing-angle test: a call that wants the list's normals alone
  // classifies with the form without normals and computes them once, in scatter
  const bool classify_normals = q.normal_map || q.min_cos > 0.f;
  const bool dense = p.point_map || p.mask || q.normal_map, list = p.count != nullptr;
  if (!dense && !list) return MD_OK;
  if (list && !scratch) MD_FAIL(MD_ERR_INVALID_ARG, "unproject: the list needs its scratch buffer");
  const int tiles = tiles_of((long)p.H * p.W);
  const size_t nb = (size_t)p.B * tiles;
  unsigned long long* bits = (unsigned long long*)scratch;
  int* counts = list ? (int*)((char*)scratch + up256(nb * kTileWords * 8)) : nullptr;
  int* offsets = list ? (int*)((char*)counts + up256(nb * 4)) : nullptr;
  const dim3 grid(tiles, p.B);
  if (classify_normals) hipLaunchKernelGGL(points_classify_kernel<NormalsParams>, grid, dim3(kTileThreads), 0, s, p, bits, counts, q);
  else hipLaunchKernelGGL(points_classify_kernel<>, grid, dim3(kTileThreads), 0, s, p, bits, counts);
  MD_HIP(hipGetLastError());
  if (!list) return MD_OK;
  hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kTileThreads), 0, s, counts, (int)nb, tiles, p.B, offsets, p.count);
  MD_HIP(hipGetLastError());
  if (!p.xyz && !p.rgb_out && !p.conf_out && !q.normals) return MD_OK;  // counts only
  if (q.normals) hipLaunchKernelGGL(points_scatter_kernel<NormalsParams>, grid, dim3(kTileThreads), 0, s, p, bits, offsets, q);
  else hipLaunchKernelGGL(points_scatter_kernel<>, grid, dim3(kTileThreads), 0, s, p, bits, offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
