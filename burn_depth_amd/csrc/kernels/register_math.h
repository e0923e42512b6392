// The arithmetic of the rigid registration (kernels/register.hip; include/mi_depth.h states the contract), as text
// that compiles for the device and for a host program alike (tests/native/register_host.cpp runs these lines sequentially;
// pipeline.register_points restates them in numpy line for line). Everything is f64 with one rounded operation per step: only
// + - * /, sqrt and comparisons, all of them correctly rounded on the device and on the host. The files that include this
// compile with contraction off (Makefile).
//
// The transform A is twelve f64: R row-major in A[0..9), then t in A[9..12). A row p moves to R p + t.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_REG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MD_REG_HD inline
#endif

namespace md {

constexpr int kRegLeaves = 16;  // per pair: p (3), q (3), p_a * q_b (9, at 6 + 3 a + b), d2 (1)
constexpr int kRegPlaneLeaves = 29;  // per usable pair of the point-to-plane form: J J^T (21), J r (6), r r (1), d2 (1)
// Cyclic Jacobi sweeps of the 4x4 solve. Convergence is quadratic; tests/test_register_host.py measures the distance to an SVD
// solve of the same sums at this count (DESIGN 12.14 records it).
constexpr int kRegSweeps = 8;
constexpr uint32_t kRegNaN = 0x7FC00000u;  // what a NaN component of a moved row or normal is written as

// axis a of the moved row: (float)(((R_a0 x + R_a1 y) + R_a2 z) + t_a), the inputs widened exactly, one cast at the end
MD_REG_HD float reg_move_axis(const double* A, int a, float x, float y, float z) {
  return (float)(((A[3 * a] * (double)x + A[3 * a + 1] * (double)y) + A[3 * a + 2] * (double)z) + A[9 + a]);
}

// axis a of a rotated normal: (float)((R_a0 x + R_a1 y) + R_a2 z)
MD_REG_HD float reg_turn_axis(const double* A, int a, float x, float y, float z) {
  return (float)((A[3 * a] * (double)x + A[3 * a + 1] * (double)y) + A[3 * a + 2] * (double)z);
}

// the bits a moved component is written with: a NaN has no portable payload, so every NaN becomes kRegNaN
MD_REG_HD uint32_t reg_out_bits(float v) {
  uint32_t bits;
  __builtin_memcpy(&bits, &v, 4);
  return v != v ? kRegNaN : bits;
}

// acc[0..16) += the leaves of the pair (source row p, target row q, squared distance d2), each leaf exact in f64
MD_REG_HD void reg_add_leaves(double* acc, const float* p, const float* q, float d2) {
  for (int a = 0; a < 3; ++a) acc[a] = acc[a] + (double)p[a];
  for (int b = 0; b < 3; ++b) acc[3 + b] = acc[3 + b] + (double)q[b];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) acc[6 + 3 * a + b] = acc[6 + 3 * a + b] + (double)p[a] * (double)q[b];
  acc[15] = acc[15] + (double)d2;
}

// One Jacobi rotation of the symmetric 4x4 `a` in the plane (p, q), accumulated into the eigenvector columns of `v`.
// A pivot that is exactly 0 is skipped. theta may overflow to infinity: t is then 0 and the rotation the identity.
MD_REG_HD void reg_jacobi_rotate(double a[4][4], double v[4][4], int p, int q) {
  const double apq = a[p][q];
  if (apq == 0.0) return;
  const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
  const double sign = theta >= 0.0 ? 1.0 : -1.0;
  const double t = sign / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  for (int k = 0; k < 4; ++k) {  // columns p and q
    const double akp = a[k][p], akq = a[k][q];
    a[k][p] = c * akp - s * akq;
    a[k][q] = s * akp + c * akq;
  }
  for (int k = 0; k < 4; ++k) {  // rows p and q
    const double apk = a[p][k], aqk = a[q][k];
    a[p][k] = c * apk - s * aqk;
    a[q][k] = s * apk + c * aqk;
  }
  for (int k = 0; k < 4; ++k) {
    const double vkp = v[k][p], vkq = v[k][q];
    v[k][p] = c * vkp - s * vkq;
    v[k][q] = s * vkp + c * vkq;
  }
}

// The rotation matrix of the unit quaternion (w, x, y, z), row-major into R[0..9). Both solves end in these lines.
MD_REG_HD void reg_quat_matrix(double w, double x, double y, double z, double* R) {
  const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
  const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = ((ww + xx) - yy) - zz; R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);       R[4] = ((ww - xx) + yy) - zz; R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = ((ww - xx) - yy) + zz;
}

// The transform that moves the n paired source rows onto their target rows in the least-squares sense (Horn's quaternion
// solve), from the pair count n >= 1 and the sixteen sums S. Writes A[0..12).
MD_REG_HD void reg_solve(int n, const double* S, double* A) {
  const double dn = (double)n;
  double pbar[3], qbar[3], H[3][3];
  for (int a = 0; a < 3; ++a) pbar[a] = S[a] / dn;
  for (int b = 0; b < 3; ++b) qbar[b] = S[3 + b] / dn;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) H[a][b] = S[6 + 3 * a + b] - S[a] * qbar[b];
  double m[4][4], v[4][4];
  m[0][0] = (H[0][0] + H[1][1]) + H[2][2];
  m[1][1] = (H[0][0] - H[1][1]) - H[2][2];
  m[2][2] = (H[1][1] - H[0][0]) - H[2][2];
  m[3][3] = (H[2][2] - H[0][0]) - H[1][1];
  m[0][1] = m[1][0] = H[1][2] - H[2][1];
  m[0][2] = m[2][0] = H[2][0] - H[0][2];
  m[0][3] = m[3][0] = H[0][1] - H[1][0];
  m[1][2] = m[2][1] = H[0][1] + H[1][0];
  m[1][3] = m[3][1] = H[2][0] + H[0][2];
  m[2][3] = m[3][2] = H[1][2] + H[2][1];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kRegSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) reg_jacobi_rotate(m, v, p, q);
  int top = 0;  // the largest eigenvalue; ties go to the smallest index
  for (int k = 1; k < 4; ++k)
    if (m[k][k] > m[top][top]) top = k;
  double w = v[0][top], x = v[1][top], y = v[2][top], z = v[3][top];
  const double len = sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / len; x = x / len; y = y / len; z = z / len;
  if (w < 0.0) {
    w = -w; x = -x; y = -y; z = -z;
  }
  reg_quat_matrix(w, x, y, z, A);
  for (int a = 0; a < 3; ++a) A[9 + a] = qbar[a] - ((A[3 * a] * pbar[0] + A[3 * a + 1] * pbar[1]) + A[3 * a + 2] * pbar[2]);
}

// the stop test: max |R'_ab - R_ab| <= rot_eps and max |t'_a - t_a| <= trans_eps
MD_REG_HD bool reg_converged(const double* A_new, const double* A_old, double rot_eps, double trans_eps) {
  double dr = 0.0, dt = 0.0;
  for (int i = 0; i < 9; ++i) {
    const double d = fabs(A_new[i] - A_old[i]);
    dr = d > dr ? d : dr;
  }
  for (int i = 9; i < 12; ++i) {
    const double d = fabs(A_new[i] - A_old[i]);
    dt = d > dt ? d : dt;
  }
  return dr <= rot_eps && dt <= trans_eps;
}

// ---- the point-to-plane form ----
// A usable pair is a pair whose target normal has three finite components that are not all zero.
MD_REG_HD bool reg_normal_usable(const float* n) {
  const bool finite = n[0] - n[0] == 0.f && n[1] - n[1] == 0.f && n[2] - n[2] == 0.f;
  return finite && (n[0] != 0.f || n[1] != 0.f || n[2] != 0.f);
}

// acc[0..29) += the leaves of the usable pair (moved source row m, target row q, its normal n, squared distance d2):
// J = (m x n, n), leaves 0..20 the upper triangle of J J^T in row-major order, 21..26 J_i * r with r = (q - m) . n, 27 r * r,
// 28 d2. The products of widened f32 are exact; every other operation rounds once.
MD_REG_HD void reg_add_plane_leaves(double* acc, const float* m, const float* q, const float* n, float d2) {
  const double m0 = (double)m[0], m1 = (double)m[1], m2 = (double)m[2];
  const double n0 = (double)n[0], n1 = (double)n[1], n2 = (double)n[2];
  double J[6];
  J[0] = m1 * n2 - m2 * n1;
  J[1] = m2 * n0 - m0 * n2;
  J[2] = m0 * n1 - m1 * n0;
  J[3] = n0; J[4] = n1; J[5] = n2;
  const double d0 = (double)q[0] - m0, d1 = (double)q[1] - m1, dd2 = (double)q[2] - m2;
  const double r = (d0 * n0 + d1 * n1) + dd2 * n2;
  int l = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++l) acc[l] = acc[l] + J[i] * J[j];
  for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + J[i] * r;
  acc[27] = acc[27] + r * r;
  acc[28] = acc[28] + (double)d2;
}

// The increment of the point-to-plane step from the 29 sums S, composed onto A_old: M x = b with M the symmetric 6x6 of leaves
// 0..20 and b leaves 21..26, by a Cholesky factorisation in the order j = 0..5 and the two substitutions; x = (w, tau). The
// rotation of the increment is that of the quaternion (1, w/2) normalised. -> false when the system is degenerate (a pivot that
// is not > 0, or a component of x that is not finite); A_new is then not written. n is the usable pair count (>= 1; unused by
// the arithmetic: the normal equations carry no mean).
MD_REG_HD bool reg_solve_plane(int n, const double* S, const double* A_old, double* A_new) {
  (void)n;
  double M[6][6], L[6][6], x[6], y[6];
  int l = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++l) M[i][j] = M[j][i] = S[l];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
  for (int j = 0; j < 6; ++j) {
    double s = M[j][j];
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double v = M[i][j];
      for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {  // L y = b
    double v = S[21 + i];
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {  // L^T x = y
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (!(x[i] - x[i] == 0.0)) return false;
  double qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2];
  const double len = sqrt(((1.0 + qx * qx) + qy * qy) + qz * qz);
  const double qw = 1.0 / len;
  qx = qx / len; qy = qy / len; qz = qz / len;
  double dR[9];
  reg_quat_matrix(qw, qx, qy, qz, dR);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) A_new[3 * a + b] = (dR[3 * a] * A_old[b] + dR[3 * a + 1] * A_old[3 + b]) + dR[3 * a + 2] * A_old[6 + b];
    A_new[9 + a] = ((dR[3 * a] * A_old[9] + dR[3 * a + 1] * A_old[10]) + dR[3 * a + 2] * A_old[11]) + x[3 + a];
  }
  return true;
}

}  // namespace md
