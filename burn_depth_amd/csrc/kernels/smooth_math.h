// The per-row and per-face arithmetic of the mesh smoothing (kernels/smooth.hip; include/mi_depth.h states the
// contract), as text that compiles for the device and for a host program alike (tests/native/smooth_host.cpp runs these lines
// sequentially). Positions live on an integer lattice of side `step`; every sum is an integer sum, modulo 2^64, so nothing
// depends on the order in which the addends arrive. The only floating-point values are the lattice coordinate of a row (one f32
// division and a round), the step of a row (f64: one division, one subtraction, one product, one round, each rounded once) and
// the outputs. The files that include this compile with contraction off (Makefile).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_SMOOTH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MD_SMOOTH_HD inline
#endif

namespace md {

constexpr float kSmoothHalf = 4194304.f;                 // 2^22 lattice steps on either side of the origin
constexpr double kSmoothMaxMove = 4611686018427387904.;  // 2^62: the largest move of one step (keeps the f64 -> int64 cast defined)

// splitmix64's finaliser, the mixer of the hash grids (voxel_math.h). Here it IS part of the output: open[v] sums mix(next) - mix(prev).
MD_SMOOTH_HD uint64_t smooth_mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// k_a = rintf(p_a / step), half to even; in range: the coordinates finite and |k_a| <= 2^22 on every axis, compared in float.
// k is written only for a row in range.
MD_SMOOTH_HD bool smooth_quantise(float x, float y, float z, float step, int64_t* k) {
  const float kx = rintf(x / step), ky = rintf(y / step), kz = rintf(z / step);
  const bool in_range = std::isfinite(x) && std::isfinite(y) && std::isfinite(z) && fabsf(kx) <= kSmoothHalf && fabsf(ky) <= kSmoothHalf &&
                        fabsf(kz) <= kSmoothHalf;
  if (in_range) {
    k[0] = (int64_t)kx; k[1] = (int64_t)ky; k[2] = (int64_t)kz;
  }
  return in_range;
}

// 0 live, 1 invalid (a corner outside 0..n-1 or on a row that is not in range), 2 degenerate (valid, two corners equal)
MD_SMOOTH_HD int smooth_face_kind(int a, int b, int c, int n, const int32_t* in_range) {
  if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n) return 1;
  if (!in_range[a] || !in_range[b] || !in_range[c]) return 1;
  return (a == b || b == c || a == c) ? 2 : 0;
}

// what corner v of a live face adds to open[v]: its successor `next` and predecessor `prev` in the winding
MD_SMOOTH_HD uint64_t smooth_open_term(int next, int prev) { return smooth_mix64((uint64_t)next) - smooth_mix64((uint64_t)prev); }

MD_SMOOTH_HD bool smooth_pinned(uint32_t deg, uint64_t open, bool in_range, int pin_boundary) {
  return deg == 0 || !in_range || (pin_boundary != 0 && open != 0);
}

// one axis of one Jacobi step of an unpinned row: S = the sum of the deg neighbour coordinates, k the row's own
MD_SMOOTH_HD int64_t smooth_step_axis(int64_t S, uint32_t deg, int64_t k, double factor) {
  const double d = (double)S / (double)deg - (double)k;
  double r = rint(factor * d);
  r = r > kSmoothMaxMove ? kSmoothMaxMove : (r < -kSmoothMaxMove ? -kSmoothMaxMove : r);
  return (int64_t)((uint64_t)k + (uint64_t)(int64_t)r);
}

MD_SMOOTH_HD float smooth_position(int64_t k, float step) { return (float)((double)k * (double)step); }

// (kb - ka) x (kc - ka), modulo 2^64
MD_SMOOTH_HD void smooth_cross(const int64_t* ka, const int64_t* kb, const int64_t* kc, uint64_t* out) {
  const uint64_t ux = (uint64_t)kb[0] - (uint64_t)ka[0], uy = (uint64_t)kb[1] - (uint64_t)ka[1], uz = (uint64_t)kb[2] - (uint64_t)ka[2];
  const uint64_t vx = (uint64_t)kc[0] - (uint64_t)ka[0], vy = (uint64_t)kc[1] - (uint64_t)ka[1], vz = (uint64_t)kc[2] - (uint64_t)ka[2];
  out[0] = uy * vz - uz * vy;
  out[1] = uz * vx - ux * vz;
  out[2] = ux * vy - uy * vx;
}

// the unit normal of a row from its summed face normals; (0,0,0) for a row without a live face or with a zero sum
MD_SMOOTH_HD void smooth_normal(uint32_t deg, const int64_t* nrm, float* out) {
  if (deg == 0 || (nrm[0] == 0 && nrm[1] == 0 && nrm[2] == 0)) {
    out[0] = out[1] = out[2] = 0.f;
    return;
  }
  const double x = (double)nrm[0], y = (double)nrm[1], z = (double)nrm[2];
  const double l = sqrt((x * x + y * y) + z * z);
  out[0] = (float)(x / l); out[1] = (float)(y / l); out[2] = (float)(z / l);
}

}  // namespace md
