// The pinhole camera of the point path and its back-projection, shared by kernels/points.hip and
// kernels/view_filter.hip: one definition, so a point the filter projects into the other views is the point the unprojection
// writes. Both files are built with contraction off (Makefile): every step is one rounded f32 operation.
#pragma once

#include <hip/hip_runtime.h>

namespace md {

struct Camera {
  float fx, fy, cx, cy;
  float r[9], t[3];
};

// K [B,3,3] or focal [B] (K = f, f, W/2, H/2); E [B,3,4] world-to-camera, null = r and t are left unset
__device__ __forceinline__ Camera load_camera(const float* __restrict__ K, const float* __restrict__ focal, const float* __restrict__ E,
                                              int H, int W, int b) {
  Camera c;
  if (K) {
    const float* k = K + (long)b * 9;
    c.fx = k[0]; c.fy = k[4]; c.cx = k[2]; c.cy = k[5];
  } else {
    c.fx = c.fy = focal[b];
    c.cx = (float)W / 2.0f;
    c.cy = (float)H / 2.0f;
  }
  if (E) {
    const float* e = E + (long)b * 12;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c.r[3 * i + j] = e[4 * i + j];
      c.t[i] = e[4 * i + 3];
    }
  }
  return c;
}

// the arithmetic contract: back-projection, then p_w = R^T (p_c - t)
__device__ __forceinline__ void unproject(const Camera& c, int world, float off, int v, int u, float d, float* out) {
  const float rx = (((float)u + off) - c.cx) / c.fx;
  const float ry = (((float)v + off) - c.cy) / c.fy;
  float x = rx * d, y = ry * d, z = d;
  if (world) {
    const float qx = x - c.t[0], qy = y - c.t[1], qz = z - c.t[2];
    x = (c.r[0] * qx + c.r[3] * qy) + c.r[6] * qz;
    y = (c.r[1] * qx + c.r[4] * qy) + c.r[7] * qz;
    z = (c.r[2] * qx + c.r[5] * qy) + c.r[8] * qz;
  }
  out[0] = x; out[1] = y; out[2] = z;
}

}  // namespace md
