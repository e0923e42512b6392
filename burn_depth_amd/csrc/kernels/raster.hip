// Mesh rasterisation for gfx950 (md_op_render_mesh, md_infer_points_raster; DESIGN 12.6, include/mi_depth.h states the contract):
// the faces kernels/mesh.hip wrote over the list, drawn into T target cameras. A render without holes: where kernels/render.hip
// z-buffers points, this z-buffers the triangles between them. Selection only: a pixel keeps the smallest 64-bit key
// (bits(z) << 32) | face of the faces that cover it, so nothing depends on the order of arrival and no float is summed. The
// vertices are projected with the render's arithmetic and snapped to 1/256 pixel; from there coverage is int64 arithmetic, and
// the depth of a covered pixel is a fixed sequence of one f64 division and rounded f32 operations (contraction is off in the
// whole file, Makefile), which pipeline.render_mesh restates bit for bit.
//
// Four launches:
//   clear    all-ones keys over T*H*W words (16-byte stores); the filled and skipped counts and the queue counter to 0
//   setup    one thread per face; the cameras of up to 64 targets sit in LDS. setup_face holds the per-face steps of the
//            contract. A face whose clipped box has at most kInlinePixels pixels is drawn by its thread; a larger one is pushed
//            as a (face, target) pair into a fixed-capacity queue with one integer atomicAdd. A push that finds the queue full
//            draws the face in place, so the capacity never changes the image. Faces beyond max_extent are counted in LDS and
//            leave the workgroup as one add per count word
//   large    a fixed grid of waves strides over the queue up to the device counter; a wave recomputes the face with setup_face
//            and its 64 lanes walk the box
//   resolve  one thread per pixel and step, 4096 pixels per workgroup: key -> depth, face; for rgb the winner's weights are
//            recomputed at the pixel. Filled pixels by one ballot popcount per wave and step and one add per workgroup and word
// Keys only decrease, so a plain load that finds a key not above the candidate skips the atomic.
// No float is converted to an integer before its float range test has passed.
#include <algorithm>
#include <cmath>

#include "points_math.h"
#include "tile_compact.h"

#ifndef MD_RASTER_INLINE_PIXELS
#define MD_RASTER_INLINE_PIXELS 64  // the best of 4, 16 and 64
#endif

namespace md {

namespace {

constexpr int kCams = 64;  // target cameras of one setup workgroup (4 KiB of LDS)
constexpr int kMaxGridY = 65535;
constexpr int kInlinePixels = MD_RASTER_INLINE_PIXELS;
constexpr int kLargeBlocks = 1024;               // the fixed grid of the large kernel: 4096 waves
constexpr int kDefaultQueue = 1 << 20;           // (face, target) pairs, 8 bytes each
constexpr unsigned long long kEmpty = ~0ull;

int g_queue_capacity = 0;  // md_debug_raster_queue: 0 = kDefaultQueue

struct Face {
  long X[3], Y[3];  // the vertices, snapped to 1/256 pixel
  long A;           // twice the area in snapped units, > 0 (after the flip)
  float iz[3];      // 1 / p.z of the vertices
  int idx[3];       // their rows
  int sign;         // -1: the weights were negated (A < 0 before)
  int u0, u1, v0, v1;
};

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }
__device__ __forceinline__ long edge_fn(long ax, long ay, long bx, long by, long px, long py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// Steps 1-5 of the contract for face f and camera c. 0: the face is not drawn; 1: drawn, `s` is set; 2: its box is wider or
// taller than max_extent (counted by the caller)
__device__ int setup_face(const RasterParams& p, const Camera& c, int f, Face& s) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = p.faces[(long)f * 3 + k];
    if ((unsigned)i >= (unsigned)p.n) return 0;  // also i < 0; n = 0: every index fails
    s.idx[k] = i;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* q = p.xyz + (long)s.idx[k] * 3;
    const float x = q[0], y = q[1], z = q[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return 0;
    float px = x, py = y, pz = z;
    if (p.E) {
      px = ((c.r[0] * x + c.r[1] * y) + c.r[2] * z) + c.t[0];
      py = ((c.r[3] * x + c.r[4] * y) + c.r[5] * z) + c.t[1];
      pz = ((c.r[6] * x + c.r[7] * y) + c.r[8] * z) + c.t[2];
    }
    if (!(isfinite(pz) && pz >= p.znear && pz <= p.zfar)) return 0;
    const float uf = ((c.fx * (px / pz)) + c.cx) - p.off;
    const float vf = ((c.fy * (py / pz)) + c.cy) - p.off;
    const float sx = floorf(uf * 256.f + 0.5f), sy = floorf(vf * 256.f + 0.5f);
    if (!(fabsf(sx) < 16777216.f && fabsf(sy) < 16777216.f)) return 0;  // in float: a NaN or a huge value never converts
    s.X[k] = (long)sx; s.Y[k] = (long)sy;
    s.iz[k] = 1.f / pz;
  }
  long A = (s.X[1] - s.X[0]) * (s.Y[2] - s.Y[0]) - (s.Y[1] - s.Y[0]) * (s.X[2] - s.X[0]);  // below 2^51
  if (A == 0) return 0;
  if (p.cull && A > 0) return 0;
  s.sign = A < 0 ? -1 : 1;
  s.A = A < 0 ? -A : A;
  const long xmin = lmin(s.X[0], lmin(s.X[1], s.X[2])), xmax = lmax(s.X[0], lmax(s.X[1], s.X[2]));
  const long ymin = lmin(s.Y[0], lmin(s.Y[1], s.Y[2])), ymax = lmax(s.Y[0], lmax(s.Y[1], s.Y[2]));
  s.u0 = (int)lmax(0, (xmin + 255) >> 8); s.u1 = (int)lmin((long)p.W - 1, xmax >> 8);  // |X| < 2^24: the shifts fit an int
  s.v0 = (int)lmax(0, (ymin + 255) >> 8); s.v1 = (int)lmin((long)p.H - 1, ymax >> 8);
  if (s.u0 > s.u1 || s.v0 > s.v1) return 0;
  if (s.u1 - s.u0 + 1 > p.max_extent || s.v1 - s.v0 + 1 > p.max_extent) return 2;
  return 1;
}

// the barycentric weights of pixel (u, v), in float; false: the pixel is not covered
__device__ __forceinline__ bool weights(const Face& s, int u, int v, float& b0, float& b1, float& b2) {
  const long px = 256l * u, py = 256l * v;
  const long w0 = s.sign * edge_fn(s.X[1], s.Y[1], s.X[2], s.Y[2], px, py);
  const long w1 = s.sign * edge_fn(s.X[2], s.Y[2], s.X[0], s.Y[0], px, py);
  const long w2 = s.sign * edge_fn(s.X[0], s.Y[0], s.X[1], s.Y[1], px, py);
  if (w0 < 0 || w1 < 0 || w2 < 0) return false;
  const double a = (double)s.A;
  b0 = (float)((double)w0 / a); b1 = (float)((double)w1 / a); b2 = (float)((double)w2 / a);
  return true;
}

// steps 6-8 for one pixel of the box; img: the keys of the target; (u, v) lies in the image (setup_face clipped the box)
__device__ __forceinline__ void draw_pixel(const RasterParams& p, const Face& s, int f, int u, int v, unsigned long long* img) {
  float b0, b1, b2;
  if (!weights(s, u, v, b0, b1, b2)) return;
  const float iz = (b0 * s.iz[0] + b1 * s.iz[1]) + b2 * s.iz[2];
  const float z = 1.f / iz;
  if (!(isfinite(z) && z >= p.znear && z <= p.zfar)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(unsigned)f;
  unsigned long long* at = img + (long)v * p.W + u;
  if (__hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;  // keys only decrease
  atomicMin(at, key);
}

// pairs = ceil(T*H*W / 2): the key buffer is a multiple of 16 bytes (raster_scratch_bytes)
__global__ void __launch_bounds__(kTileThreads) raster_clear_kernel(ulonglong2* __restrict__ keys, size_t pairs, int32_t* __restrict__ filled,
                                                                int32_t* __restrict__ skipped, int* __restrict__ queue_n, int T) {
  fill_keys(keys, pairs);
  if (blockIdx.x != 0) return;
  for (int t = threadIdx.x; t <= T; t += kTileThreads) {
    if (filled) filled[t] = 0;
    if (skipped) skipped[t] = 0;
  }
  if (threadIdx.x == 0) *queue_n = 0;
}

// grid (ceil(nf / 256), groups of 64 targets); t0 = the first target of group 0 of this launch
__global__ void __launch_bounds__(kTileThreads) raster_setup_kernel(RasterParams p, unsigned long long* __restrict__ keys, int* __restrict__ queue_n,
                                                                int2* __restrict__ queue, int capacity, int t0) {
  __shared__ Camera cams[kCams];
  __shared__ int skip_n[kCams];
  const int tid = threadIdx.x;
  const int tbase = t0 + (int)blockIdx.y * kCams;
  const int nt = p.T - tbase < kCams ? p.T - tbase : kCams;
  if (tid < nt) {
    cams[tid] = load_camera(p.K, p.focal, p.E, p.H, p.W, tbase + tid);
    skip_n[tid] = 0;
  }
  __syncthreads();
  const long f = (long)blockIdx.x * kTileThreads + tid;
  const long hw = (long)p.H * p.W;
  if (f < live_count(p.count, 0, p.nf)) {
    for (int j = 0; j < nt; ++j) {
      Face s;
      const int rc = setup_face(p, cams[j], (int)f, s);
      if (rc == 2) atomicAdd(&skip_n[j], 1);  // LDS; rare
      if (rc != 1) continue;
      const int bw = s.u1 - s.u0 + 1, bh = s.v1 - s.v0 + 1;
      if (bw * bh > kInlinePixels) {  // at most 1024 x 1024
        const int slot = atomicAdd(queue_n, 1);
        if (slot < capacity) {
          queue[slot] = make_int2((int)f, tbase + j);
          continue;
        }
      }
      unsigned long long* img = keys + (long)(tbase + j) * hw;
      for (int v = s.v0; v <= s.v1; ++v)
        for (int u = s.u0; u <= s.u1; ++u) draw_pixel(p, s, (int)f, u, v, img);
    }
  }
  if (!p.skipped) return;
  __syncthreads();
  if (tid < nt && skip_n[tid]) {
    atomicAdd(&p.skipped[tbase + tid], skip_n[tid]);
    atomicAdd(&p.skipped[p.T], skip_n[tid]);
  }
}

// grid kLargeBlocks: wave w of the grid takes the queue entries w, w + waves, ...
__global__ void __launch_bounds__(kTileThreads) raster_large_kernel(RasterParams p, unsigned long long* __restrict__ keys, const int* __restrict__ queue_n,
                                                                const int2* __restrict__ queue, int capacity) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)blockIdx.x * kTileWaves + (threadIdx.x >> 6), waves = (int)gridDim.x * kTileWaves;
  int n = *queue_n;  // pushes beyond the capacity were drawn in place
  n = n < capacity ? n : capacity;
  const long hw = (long)p.H * p.W;
  for (int e = wave; e < n; e += waves) {
    const int2 job = queue[e];
    if ((unsigned)job.y >= (unsigned)p.T || (unsigned)job.x >= (unsigned)p.nf) continue;  // what setup wrote: never taken
    const Camera c = load_camera(p.K, p.focal, p.E, p.H, p.W, job.y);
    Face s;
    if (setup_face(p, c, job.x, s) != 1) continue;
    const int bw = s.u1 - s.u0 + 1, total = bw * (s.v1 - s.v0 + 1);
    unsigned long long* img = keys + (long)job.y * hw;
    for (int k = lane; k < total; k += 64) draw_pixel(p, s, job.x, s.u0 + k % bw, s.v0 + k / bw, img);
  }
}

// grid T * ceil(H W / 4096): a workgroup lies inside one target
__global__ void __launch_bounds__(kTileThreads) raster_resolve_kernel(RasterParams p, const unsigned long long* __restrict__ keys, int per_target) {
  __shared__ int wave_n[kTileWaves];
  const int tid = threadIdx.x;
  const int t = (int)(blockIdx.x / (unsigned)per_target);
  const long hw = (long)p.H * p.W;
  Camera c = {};
  if (p.rgb_out) c = load_camera(p.K, p.focal, p.E, p.H, p.W, t);
  int n = 0;
  for (int st = 0; st < kTileSteps; ++st) {
    const long px = tile_item(blockIdx.x % (unsigned)per_target, st);
    bool hit = false;
    if (px < hw) {
      const long o = (long)t * hw + px;
      const unsigned long long key = keys[o];
      hit = key != kEmpty;
      const int f = (int)(unsigned)key;
      if (p.depth) p.depth[o] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.f;
      if (p.face) p.face[o] = hit ? f : -1;
      if (p.rgb_out) {
        uint8_t out[3] = {0, 0, 0};
        Face s;
        float b0, b1, b2;
        // the winner covered this pixel, so both calls succeed; a hole names no face
        if (hit && (unsigned)f < (unsigned)p.nf && setup_face(p, c, f, s) == 1 && weights(s, (int)(px % p.W), (int)(px / p.W), b0, b1, b2)) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const float c0 = (float)p.rgb[(long)s.idx[0] * 3 + ch], c1 = (float)p.rgb[(long)s.idx[1] * 3 + ch];
            const float c2 = (float)p.rgb[(long)s.idx[2] * 3 + ch];
            out[ch] = (uint8_t)fminf(floorf(((b0 * c0 + b1 * c1) + b2 * c2) + 0.5f), 255.f);  // >= 0: the weights are
          }
        }
        uint8_t* dst = p.rgb_out + o * 3;
        dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
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

size_t keys_bytes(int T, int H, int W) { return up256((size_t)T * H * W * 8); }

}  // namespace

int raster_inline_pixels() { return kInlinePixels; }

int raster_queue_capacity(int capacity) {
  const int prev = g_queue_capacity;
  if (capacity >= 0) g_queue_capacity = capacity;
  return prev;
}

int raster_queue_entries() { return g_queue_capacity > 0 ? g_queue_capacity : kDefaultQueue; }

size_t raster_scratch_bytes(int T, int H, int W, int queue_entries) {
  return keys_bytes(T, H, W) + 256 + up256((size_t)queue_entries * 8);
}

int launch_render_mesh(const RasterParams& p, void* scratch, int queue_entries, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: no scratch buffer");
  if (p.n < 0 || p.nf < 0) MD_FAIL(MD_ERR_SHAPE, "render_mesh: %d rows, %d faces", p.n, p.nf);
  if (p.nf > 0 && (!p.faces || (p.n > 0 && !p.xyz))) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: faces without a faces or an xyz pointer");
  if (p.T <= 0 || p.H <= 0 || p.W <= 0 || (long)p.T * p.H * p.W >= (1l << 31))
    MD_FAIL(MD_ERR_SHAPE, "render_mesh: invalid target shape [%d,%d,%d]", p.T, p.H, p.W);
  if (p.max_extent < 1 || p.max_extent > kRasterMaxExtent) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: max_extent %d outside 1..%d", p.max_extent, kRasterMaxExtent);
  if (queue_entries < 1) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: a queue of %d entries", queue_entries);
  if (!p.K && !p.focal) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: neither intrinsics nor a focal length");
  if (p.rgb_out && !p.rgb) MD_FAIL(MD_ERR_INVALID_ARG, "render_mesh: an rgb output needs an rgb row");
  unsigned long long* keys = (unsigned long long*)scratch;
  int* queue_n = (int*)((char*)scratch + keys_bytes(p.T, p.H, p.W));
  int2* queue = (int2*)((char*)queue_n + 256);
  const size_t total = (size_t)p.T * p.H * p.W, pairs = (total + 1) / 2;
  const unsigned clear_grid = (unsigned)std::min<size_t>((pairs + kTileThreads - 1) / kTileThreads, 256 * 32);
  hipLaunchKernelGGL(raster_clear_kernel, dim3(clear_grid), dim3(kTileThreads), 0, s, (ulonglong2*)keys, pairs, p.filled, p.skipped, queue_n, p.T);
  MD_HIP(hipGetLastError());
  if (p.nf > 0) {
    const unsigned blocks = (unsigned)(((long)p.nf + kTileThreads - 1) / kTileThreads);
    const long groups = ((long)p.T + kCams - 1) / kCams;
    for (long g = 0; g < groups; g += kMaxGridY) {
      const unsigned gy = (unsigned)std::min<long>(groups - g, kMaxGridY);
      hipLaunchKernelGGL(raster_setup_kernel, dim3(blocks, gy), dim3(kTileThreads), 0, s, p, keys, queue_n, queue, queue_entries, (int)(g * kCams));
      MD_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(raster_large_kernel, dim3(kLargeBlocks), dim3(kTileThreads), 0, s, p, keys, queue_n, queue, queue_entries);
    MD_HIP(hipGetLastError());
  }
  const int per_target = tiles_of((long)p.H * p.W);
  hipLaunchKernelGGL(raster_resolve_kernel, dim3((unsigned)((long)p.T * per_target)), dim3(kTileThreads), 0, s, p, keys, per_target);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
