// Point rendering for gfx950 (md_op_render_points, md_infer_points_render; DESIGN 12.4, include/mi_depth.h states the contract):
// a point list projected into T target cameras and z-buffered, the inverse direction of kernels/points.hip. Selection only: a
// pixel keeps the smallest 64-bit key (bits(p.z) << 32) | row of the points whose footprint covers it, so nothing depends on
// the order of arrival and no float is summed. Contraction is off in the whole file (Makefile): the projection is the view
// filter's, one rounded f32 operation per step, which pipeline.render_points restates in numpy.
//
// Three launches:
//   clear    all-ones keys over T*H*W words (16-byte stores), the filled counts to 0
//   splat    one thread per list row; the live row count is read from device memory. The cameras of up to 64 targets sit in
//            LDS; the thread walks them and the (2 radius + 1)^2 footprint with atomicMin on the key. Keys only decrease, so a
//            plain load that finds a key not above the candidate skips the atomic (MD_RENDER_PEEK, DESIGN 12.4 has both forms)
//   resolve  one thread per pixel and step, 4096 pixels per workgroup: key -> depth, index, gathered rgb; filled pixels by
//            one ballot popcount per wave and step and one integer add per workgroup and count word (with 256 pixels per
//            workgroup the adds, all on two words, were the kernel: DESIGN 12.4)
// No float is converted to int before the float comparison against the image has passed.
#include <algorithm>
#include <cmath>

#include "points_math.h"
#include "tile_compact.h"

#ifndef MD_RENDER_PEEK
#define MD_RENDER_PEEK 1  // 1: load the pixel's key first and skip the atomic when the candidate cannot win
#endif

namespace md {

namespace {

constexpr int kCams = 64;  // target cameras of one splat workgroup (4 KiB of LDS)
constexpr int kMaxGridY = 65535;
constexpr unsigned long long kEmpty = ~0ull;

// pairs = ceil(T*H*W / 2): the key buffer is a multiple of 16 bytes (render_scratch_bytes)
__global__ void __launch_bounds__(kTileThreads) render_clear_kernel(ulonglong2* __restrict__ keys, size_t pairs, int32_t* __restrict__ filled,
                                                                int T) {
  fill_keys(keys, pairs);
  if (filled && blockIdx.x == 0)
    for (int t = threadIdx.x; t <= T; t += kTileThreads) filled[t] = 0;
}

// grid (ceil(n / 256), groups of 64 targets); t0 = the first target of group 0 of this launch
__global__ void __launch_bounds__(kTileThreads) render_splat_kernel(RenderParams p, unsigned long long* __restrict__ keys, int t0) {
  __shared__ Camera cams[kCams];
  const int tid = threadIdx.x;
  const int tbase = t0 + (int)blockIdx.y * kCams;
  const int nt = p.T - tbase < kCams ? p.T - tbase : kCams;
  if (tid < nt) cams[tid] = load_camera(p.K, p.focal, p.E, p.H, p.W, tbase + tid);
  __syncthreads();
  const long i = (long)blockIdx.x * kTileThreads + tid;
  if (i >= live_count(p.count, 0, p.n)) return;
  const float x = p.xyz[i * 3], y = p.xyz[i * 3 + 1], z = p.xyz[i * 3 + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const float fw = (float)p.W, fh = (float)p.H;
  const long hw = (long)p.H * p.W;
  for (int j = 0; j < nt; ++j) {
    const Camera& c = cams[j];
    float px = x, py = y, pz = z;
    if (p.E) {
      px = ((c.r[0] * x + c.r[1] * y) + c.r[2] * z) + c.t[0];
      py = ((c.r[3] * x + c.r[4] * y) + c.r[5] * z) + c.t[1];
      pz = ((c.r[6] * x + c.r[7] * y) + c.r[8] * z) + c.t[2];
    }
    if (!(isfinite(pz) && pz >= p.znear && pz <= p.zfar)) continue;
    const float uf = ((c.fx * (px / pz)) + c.cx) - p.off;
    const float vf = ((c.fy * (py / pz)) + c.cy) - p.off;
    const float uu = floorf(uf + 0.5f), vv = floorf(vf + 0.5f);
    if (!(uu >= 0.f && uu < fw && vv >= 0.f && vv < fh)) continue;  // in float: a NaN or a huge value never converts
    const int u = (int)uu, v = (int)vv;
    const unsigned long long key = ((unsigned long long)__float_as_uint(pz) << 32) | (unsigned long long)(unsigned)i;
    unsigned long long* img = keys + (long)(tbase + j) * hw;
    const int v0 = v - p.radius > 0 ? v - p.radius : 0, v1 = v + p.radius < p.H - 1 ? v + p.radius : p.H - 1;
    const int u0 = u - p.radius > 0 ? u - p.radius : 0, u1 = u + p.radius < p.W - 1 ? u + p.radius : p.W - 1;
    for (int vy = v0; vy <= v1; ++vy)
      for (int ux = u0; ux <= u1; ++ux) {
        unsigned long long* at = img + (long)vy * p.W + ux;
#if MD_RENDER_PEEK
        if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) continue;  // keys only decrease
#endif
        atomicMin(at, key);
      }
  }
}

// grid T * ceil(H W / 4096): a workgroup lies inside one target
__global__ void __launch_bounds__(kTileThreads) render_resolve_kernel(RenderParams p, const unsigned long long* __restrict__ keys, int per_target) {
  __shared__ int wave_n[kTileWaves];
  const int tid = threadIdx.x;
  const int t = (int)(blockIdx.x / (unsigned)per_target);
  const long hw = (long)p.H * p.W;
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long px = tile_item(blockIdx.x % (unsigned)per_target, s);
    bool hit = false;
    if (px < hw) {
      const long o = (long)t * hw + px;
      const unsigned long long key = keys[o];
      hit = key != kEmpty;
      const int row = (int)(unsigned)key;
      if (p.depth) p.depth[o] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
      if (p.index) p.index[o] = hit ? row : -1;
      if (p.rgb_out) {
        uint8_t* dst = p.rgb_out + o * 3;
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (hit) {  // a hole names no row
          const uint8_t* src = p.rgb + (long)row * 3;
          c0 = src[0]; c1 = src[1]; c2 = src[2];
        }
        dst[0] = c0; dst[1] = c1; dst[2] = c2;
      }
    }
    if (p.filled) n += __popcll(__ballot(hit));  // the same in every lane of the wave
  }
  if (!p.filled) return;
  const int sum = tile_sum(n, wave_n);
  if (tid == 0 && sum) {
    atomicAdd(&p.filled[t], sum);
    atomicAdd(&p.filled[p.T], sum);
  }
}

}  // namespace

size_t render_scratch_bytes(int T, int H, int W) { return up256((size_t)T * H * W * 8); }

int launch_render_points(const RenderParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "render_points: no scratch buffer");
  if (p.n < 0) MD_FAIL(MD_ERR_SHAPE, "render_points: %d rows", p.n);
  if (p.T <= 0 || p.H <= 0 || p.W <= 0 || (long)p.T * p.H * p.W >= (1l << 31))
    MD_FAIL(MD_ERR_SHAPE, "render_points: invalid target shape [%d,%d,%d]", p.T, p.H, p.W);
  if (p.radius < 0 || p.radius > kRenderMaxRadius) MD_FAIL(MD_ERR_INVALID_ARG, "render_points: radius %d outside 0..%d", p.radius, kRenderMaxRadius);
  if (!p.K && !p.focal) MD_FAIL(MD_ERR_INVALID_ARG, "render_points: neither intrinsics nor a focal length");
  if (p.rgb_out && !p.rgb) MD_FAIL(MD_ERR_INVALID_ARG, "render_points: an rgb output needs an rgb row");
  unsigned long long* keys = (unsigned long long*)scratch;
  const size_t total = (size_t)p.T * p.H * p.W, pairs = (total + 1) / 2;
  const unsigned clear_grid = (unsigned)std::min<size_t>((pairs + kTileThreads - 1) / kTileThreads, 256 * 32);
  hipLaunchKernelGGL(render_clear_kernel, dim3(clear_grid), dim3(kTileThreads), 0, s, (ulonglong2*)keys, pairs, p.filled, p.T);
  MD_HIP(hipGetLastError());
  if (p.n > 0) {
    const unsigned blocks = (unsigned)(((long)p.n + kTileThreads - 1) / kTileThreads);
    const long groups = ((long)p.T + kCams - 1) / kCams;
    for (long g = 0; g < groups; g += kMaxGridY) {
      const unsigned gy = (unsigned)std::min<long>(groups - g, kMaxGridY);
      hipLaunchKernelGGL(render_splat_kernel, dim3(blocks, gy), dim3(kTileThreads), 0, s, p, keys, (int)(g * kCams));
      MD_HIP(hipGetLastError());
    }
  }
  const int per_target = tiles_of((long)p.H * p.W);
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((long)p.T * per_target)), dim3(kTileThreads), 0, s, p, keys, per_target);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
