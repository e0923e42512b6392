// The arithmetic of the RANSAC plane extraction (kernels/planes.hip; include/mi_depth.h states the contract): the
// sample word of a corner, the plane of three rows and the two inlier predicates, once. The hypothesis kernel, the count kernel
// and the label kernel call these, so an inlier counted is an inlier labelled. f32, one rounded operation per step, in the order
// written; the files that include this compile with contraction off (Makefile). pipeline.fit_planes restates every line in numpy.
#pragma once

#include <cmath>
#include <cstdint>

#include "smooth_math.h"

namespace md {

constexpr float kPlaneMinLen2 = 1e-30f;  // a cross product at or below it is a degenerate triple
constexpr int kPlanesMax = 8;            // planes of one call
constexpr int kPlaneHypothesesMax = 4096;

struct Plane {  // n . q + d = 0, |n| = 1, the normal facing the origin
  float nx, ny, nz, d;
};

// the word whose mix64 picks corner j of hypothesis h in round p; the mixer is smoothing's (smooth_math.h)
MD_SMOOTH_HD uint64_t plane_sample_word(uint32_t seed, int p, int h, int j) {
  return ((uint64_t)seed << 32) | ((uint64_t)p << 28) | ((uint64_t)h << 2) | (uint64_t)j;
}
// the position in the live index, M > 0 live rows
MD_SMOOTH_HD uint64_t plane_sample(uint32_t seed, int p, int h, int j, uint64_t M) { return smooth_mix64(plane_sample_word(seed, p, h, j)) % M; }

// The plane through p0, p1, p2. -> false: the triple is degenerate or the axis constraint (min_cos > 0) rejects it; *out is then
// not written.
MD_SMOOTH_HD bool plane_of_rows(const float* p0, const float* p1, const float* p2, const float* axis, float axis_min_cos, Plane* out) {
  const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  float nx = e1y * e2z - e1z * e2y;
  float ny = e1z * e2x - e1x * e2z;
  float nz = e1x * e2y - e1y * e2x;
  const float len2 = (nx * nx + ny * ny) + nz * nz;
  if (!(std::isfinite(len2) && len2 > kPlaneMinLen2)) return false;
  const float s = sqrtf(len2);
  nx = nx / s; ny = ny / s; nz = nz / s;
  float d = -((nx * p0[0] + ny * p0[1]) + nz * p0[2]);
  bool flip = d < 0.f;
  if (d == 0.f) {  // either zero: the first non-zero component of n decides
    const float first = nx != 0.f ? nx : (ny != 0.f ? ny : nz);
    flip = first < 0.f;
  }
  if (flip) { nx = -nx; ny = -ny; nz = -nz; d = -d; }
  if (axis_min_cos > 0.f && !(fabsf((nx * axis[0] + ny * axis[1]) + nz * axis[2]) >= axis_min_cos)) return false;
  out->nx = nx; out->ny = ny; out->nz = nz; out->d = d;
  return true;
}

// row q lies within tol of the plane (inclusive)
MD_SMOOTH_HD bool plane_near(const Plane& w, float qx, float qy, float qz, float tol) {
  return fabsf(((w.nx * qx + w.ny * qy) + w.nz * qz) + w.d) <= tol;
}
// the row's normal m is within the cone around the plane's normal, either way round; an all-zero normal fails
MD_SMOOTH_HD bool plane_normal_agrees(const Plane& w, float mx, float my, float mz, float min_cos) {
  return fabsf((w.nx * mx + w.ny * my) + w.nz * mz) >= min_cos;
}

}  // namespace md
