// Frame path kernels for gfx950 (md_process_frame): the Catmull-Rom resize + centre crop + input normalisation of a u8 RGB
// camera frame, and the depth display step (crop, bilinear restore, per-frame min-max, grey u8 / RGBA f32). HBM- and
// launch-bound: two launches each side of the model. Contraction is off in the whole file (Makefile): every tap is a
// separate f32 multiply then add, in the order the host references use.
#include <cfloat>
#include <cmath>

#include "ops.h"

namespace md {

// ------------------------------------------------------------------------------------------------
// Catmull-Rom taps (pipeline._catmull_rom / _sample_axis, the image crate's separable resampler), built on the host
// ------------------------------------------------------------------------------------------------
// glibc powf through a volatile exponent: the compiler may not rewrite pow(a, 3) into multiplies
static volatile float g_three = 3.0f;

static float catmull_rom_host(float x) {
  const float a = fabsf(x), a2 = a * a, a3 = powf(a, g_three);
  float k;
  if (a < 1.0f) k = (9.0f * a3 + -15.0f * a2) + 6.0f;                     // (12 - 9b - 6c) a^3 + (-18 + 12b + 6c) a^2 + (6 - 2b)
  else if (a < 2.0f) k = ((-3.0f * a3 + 15.0f * a2) + -24.0f * a) + 12.0f;  // (-b - 6c) a^3 + (6b + 30c) a^2 + (-12b - 48c) a + (8b + 24c)
  else k = 0.0f;
  return k / 6.0f;
}

void catmull_rom_window(int in_len, int out_len, int o, int* left, int* count, float* weights) {
  const float ratio = (float)in_len / (float)out_len;
  const float sratio = ratio >= 1.0f ? ratio : 1.0f;
  const float support = 2.0f * sratio;
  const float centre = ((float)o + 0.5f) * ratio;
  float l = floorf(centre - support);
  l = l > 0.0f ? l : 0.0f;
  l = l < (float)(in_len - 1) ? l : (float)(in_len - 1);
  const int lo = (int)l;
  float r = ceilf(centre + support);
  r = r > (float)(lo + 1) ? r : (float)(lo + 1);
  r = r < (float)in_len ? r : (float)in_len;
  const int n = (int)r - lo;
  *left = lo;
  *count = n;
  if (!weights) return;
  const float c = centre - 0.5f;
  float sum = 0.0f;
  for (int k = 0; k < n; ++k) {
    weights[k] = catmull_rom_host(((float)(lo + k) - c) / sratio);
    sum = sum + weights[k];  // left to right
  }
  for (int k = 0; k < n; ++k) weights[k] = weights[k] / sum;
}

int catmull_rom_max_taps(int in_len, int out_len) {
  int mx = 1;
  for (int o = 0; o < out_len; ++o) {
    int l = 0, n = 0;
    catmull_rom_window(in_len, out_len, o, &l, &n, nullptr);
    mx = n > mx ? n : mx;
  }
  return mx;
}

// ------------------------------------------------------------------------------------------------
// vertical pass: u8 rows -> f32 rows of the byte columns [xb0, xb0 + 4 nq) that the horizontal pass reads. One thread
// per 4 bytes of a row (a dword load per tap when rows are dword aligned).
// ------------------------------------------------------------------------------------------------
template <bool DW>
__global__ void __launch_bounds__(256) cr_vertical_kernel(const uint8_t* __restrict__ rgb, int B, int h, int rowb, int xb0, int nq,
                                                          int th, int oy0, CrAxis ax, float* __restrict__ tmp) {
  const long total = (long)B * th * nq;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i % nq);
    const long t = i / nq;
    const int oy = (int)(t % th), b = (int)(t / th);
    const int2 win = ax.win[oy0 + oy];
    const float* w = ax.w + (long)(oy0 + oy) * ax.maxc;
    const int j = xb0 + 4 * q;
    const uint8_t* src = rgb + ((long)b * h + win.x) * rowb + j;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < win.y; ++k, src += rowb) {
      const float wk = w[k];
      uint32_t v;
      if (DW) {
        v = *(const uint32_t*)src;
      } else {
        v = 0;
        for (int e = 0; e < 4; ++e)
          if (j + e < rowb) v |= (uint32_t)src[e] << (8 * e);
      }
      a0 = a0 + wk * (float)(v & 0xff);
      a1 = a1 + wk * (float)((v >> 8) & 0xff);
      a2 = a2 + wk * (float)((v >> 16) & 0xff);
      a3 = a3 + wk * (float)(v >> 24);
    }
    *(float4*)(tmp + (((long)b * th + oy) * nq + q) * 4) = make_float4(a0, a1, a2, a3);
  }
}

// horizontal pass: f32 rows -> clamp + round-to-nearest-even u8 -> optional u8 [B,th,tw,3] and the rgb_to_input normalisation
// into NCHW f32 [B,3,th,tw]. One thread per output pixel.
__global__ void __launch_bounds__(256) cr_horizontal_kernel(const float* __restrict__ tmp, int B, int th, int tw, int ld, int xb0, int ox0,
                                                            CrAxis ax, uint8_t* __restrict__ out_u8, float* __restrict__ out_nchw) {
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float sd[3] = {0.229f, 0.224f, 0.225f};
  const long hw = (long)th * tw, total = (long)B * hw;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % tw);
    const long t = i / tw;
    const int oy = (int)(t % th), b = (int)(t / th);
    const int2 win = ax.win[ox0 + ox];
    const float* w = ax.w + (long)(ox0 + ox) * ax.maxc;
    const float* row = tmp + ((long)b * th + oy) * ld + 3 * win.x - xb0;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < win.y; ++k, row += 3) {
      const float wk = w[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = acc[c] + wk * row[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float r = fminf(fmaxf(rintf(acc[c]), 0.f), 255.f);
      const uint8_t u = (uint8_t)r;
      if (out_u8) out_u8[i * 3 + c] = u;
      if (out_nchw) {
        const float v = (float)u / 255.0f;
        out_nchw[((long)b * 3 + c) * hw + oy * (long)tw + ox] = (v - mean[c]) / sd[c];
      }
    }
  }
}

static inline int frame_grid(long items, int cap = 256 * 8) {
  long g = (items + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

void catmull_rom_span(const int* left, const int* count, int cx, int tw, int* xb0, int* nq) {
  int lo = 1 << 30, hi = 0;
  for (int ox = cx; ox < cx + tw; ++ox) {
    lo = left[ox] < lo ? left[ox] : lo;
    hi = left[ox] + count[ox] > hi ? left[ox] + count[ox] : hi;
  }
  *xb0 = (3 * lo) & ~3;
  *nq = (3 * hi - *xb0 + 3) / 4;
}

int launch_resize_catmull_rom(const uint8_t* rgb, int B, int h, int w, const CrAxis& ax_v, int cy, int th, const CrAxis& ax_h, int cx,
                              int tw, int xb0, int nq, float* tmp, uint8_t* out_u8, float* out_nchw, hipStream_t s) {
  const int rowb = 3 * w;
  const bool dw = rowb % 4 == 0 && ((uintptr_t)rgb & 3) == 0;
  const long nv = (long)B * th * nq;
  if (dw)
    hipLaunchKernelGGL(cr_vertical_kernel<true>, dim3(frame_grid(nv)), dim3(256), 0, s, rgb, B, h, rowb, xb0, nq, th, cy, ax_v, tmp);
  else
    hipLaunchKernelGGL(cr_vertical_kernel<false>, dim3(frame_grid(nv)), dim3(256), 0, s, rgb, B, h, rowb, xb0, nq, th, cy, ax_v, tmp);
  MD_HIP(hipGetLastError());
  hipLaunchKernelGGL(cr_horizontal_kernel, dim3(frame_grid((long)B * th * tw)), dim3(256), 0, s, tmp, B, th, tw, 4 * nq, xb0, cx, ax_h,
                     out_u8, out_nchw);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------
// display: crop -> optional bilinear restore (pipeline.resize_depth_field) -> min-max over the finite values of each frame
// (pipeline.depth_to_u8) -> u8 grey or RGBA f32. Two launches: per-block partial min / max, then a consumer that folds the
// partials of its frame and writes the pixels (the restore is recomputed, not stored).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float disp_sample(const float* __restrict__ d, const DisplayGeom& g, int b, int oy, int ox) {
  const float* f = d + (long)b * g.h * g.w;
  if (!g.resize) return f[(long)(g.cy + oy) * g.w + g.cx + ox];
  const float xs = g.ow > 1 ? ((float)ox + 0.5f) * g.sx - 0.5f : 0.f;
  const float ys = g.oh > 1 ? ((float)oy + 0.5f) * g.sy - 0.5f : 0.f;
  const int x0 = (int)fminf(fmaxf(floorf(xs), 0.f), (float)(g.cw - 1));
  const int y0 = (int)fminf(fmaxf(floorf(ys), 0.f), (float)(g.ch - 1));
  const int x1 = x0 + 1 < g.cw - 1 ? x0 + 1 : g.cw - 1;
  const int y1 = y0 + 1 < g.ch - 1 ? y0 + 1 : g.ch - 1;
  const float fx = xs - (float)x0, fy = ys - (float)y0;
  const float* r0 = f + (long)(g.cy + y0) * g.w + g.cx;
  const float* r1 = f + (long)(g.cy + y1) * g.w + g.cx;
  const float top = r0[x0] * (1.0f - fx) + r0[x1] * fx;
  const float bot = r1[x0] * (1.0f - fx) + r1[x1] * fx;
  return top * (1.0f - fy) + bot * fy;
}

__global__ void __launch_bounds__(256) display_minmax_kernel(const float* __restrict__ d, DisplayGeom g, float2* __restrict__ part) {
  __shared__ float smin[256], smax[256];
  const int b = blockIdx.y;
  const long n = (long)g.oh * g.ow;
  float lo = INFINITY, hi = -INFINITY;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = disp_sample(d, g, b, (int)(i / g.ow), (int)(i % g.ow));
    if (isfinite(v)) {
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  smin[threadIdx.x] = lo;
  smax[threadIdx.x] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]);
      smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = make_float2(smin[0], smax[0]);
}

__global__ void __launch_bounds__(256) display_write_kernel(const float* __restrict__ d, DisplayGeom g, const float2* __restrict__ part,
                                                            int nparts, int normalize, int format, void* __restrict__ out,
                                                            float* __restrict__ range) {
  __shared__ float smin[256], smax[256];
  const int b = blockIdx.y;
  float lo = 0.f, rng = 1.f;
  if (part) {
    float l = INFINITY, h = -INFINITY;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) {
      const float2 p = part[(long)b * nparts + i];
      l = fminf(l, p.x);
      h = fmaxf(h, p.y);
    }
    smin[threadIdx.x] = l;
    smax[threadIdx.x] = h;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) {
        smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + s]);
        smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + s]);
      }
      __syncthreads();
    }
    float hi = smax[0];
    lo = smin[0];
    if (!(lo <= hi)) {  // no finite value in the frame
      lo = 0.f;
      hi = 1.f;
    }
    rng = fmaxf(hi - lo, FLT_EPSILON);
    if (range && blockIdx.x == 0 && threadIdx.x == 0) {
      range[2 * b] = lo;
      range[2 * b + 1] = hi;
    }
  }
  const long n = (long)g.oh * g.ow;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = disp_sample(d, g, b, (int)(i / g.ow), (int)(i % g.ow));
    float x = v;
    if (normalize) x = isfinite(v) ? fminf(fmaxf((v - lo) / rng, 0.f), 1.f) : 0.f;
    if (format == MD_FRAME_U8_GRAY) {
      ((uint8_t*)out)[(long)b * n + i] = (uint8_t)fminf(fmaxf(floorf(x * 255.0f + 0.5f), 0.f), 255.f);
    } else {
      ((float4*)out)[(long)b * n + i] = make_float4(x, x, x, 1.0f);
    }
  }
}

int display_parts(const DisplayGeom& g) {
  const long n = (long)g.oh * g.ow;
  long p = (n + 4 * 256 - 1) / (4 * 256);
  return (int)(p < 1 ? 1 : (p > 256 ? 256 : p));
}

int launch_depth_display(const float* depth, const DisplayGeom& g, int normalize, int format, void* out, float* range, float2* parts,
                         hipStream_t s) {
  const int np = display_parts(g);
  const bool reduce = normalize || range;
  if (reduce) {
    hipLaunchKernelGGL(display_minmax_kernel, dim3(np, g.B), dim3(256), 0, s, depth, g, parts);
    MD_HIP(hipGetLastError());
  }
  if (!out && !range) return MD_OK;
  // the consumer runs at least one block per frame so that `range` is written even without a display output
  const long n = (long)g.oh * g.ow;
  const int nb = out ? frame_grid(n, 512) : 1;
  DisplayGeom gg = g;
  if (!out) gg.oh = 0;  // range only: no pixel loop
  hipLaunchKernelGGL(display_write_kernel, dim3(nb, g.B), dim3(256), 0, s, depth, gg, reduce ? parts : (const float2*)nullptr, np,
                     normalize, format, out, range);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
