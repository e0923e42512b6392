// Host program of tests/test_register_plane_host.py: the point-to-plane contract run sequentially on the host from
// kernels/register_math.h, with a literal O(N T) nearest search in the contract's cells and the sums in the contract's fixed tree
// written as literal loops. Built with -ffp-contract=off under the address and undefined-behaviour sanitizers. One input file
// per argument:
//   int32 N, T, K, min_pairs | f32 radius | f64 rot_eps, trans_eps, init[12] | f32 xyz [N,3] | f32 target [T,3] | f32 normals [T,3]
// One output line per file: the hex bits of the transform, the histories, the stats, `dropped`, then per row `nearest`, the bits
// of `dist2` and the bits of the moved row of the evaluation pass.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/register_math.h"

namespace {

constexpr float kHalf = 1048576.f;
constexpr int kL = md::kRegPlaneLeaves;

bool cell_of(const float* p, float side, long* c) {
  const float cx = floorf(p[0] / side), cy = floorf(p[1] / side), cz = floorf(p[2] / side);
  const bool ok = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && cx >= -kHalf && cx < kHalf && cy >= -kHalf && cy < kHalf &&
                  cz >= -kHalf && cz < kHalf;
  if (ok) {
    c[0] = (long)cx; c[1] = (long)cy; c[2] = (long)cz;
  }
  return ok;
}

uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

// a 256-thread workgroup's value of one leaf: the halving tree over every wave's 64 lanes, then (W0 + W1) + (W2 + W3)
double workgroup(double* v /* [256] */) {
  for (int w = 0; w < 4; ++w)
    for (int h = 32; h >= 1; h >>= 1)
      for (int l = 0; l < h; ++l) v[w * 64 + l] = v[w * 64 + l] + v[w * 64 + l + h];
  return (v[0] + v[64]) + (v[128] + v[192]);
}

struct Pass {
  int n = 0, in_range = 0, dropped = 0;
  double S[kL];
  std::vector<int32_t> nearest;
  std::vector<uint32_t> dist2, moved;
};

Pass one_pass(const double* A, const std::vector<float>& xyz, const std::vector<float>& target, const std::vector<float>& normals,
              const std::vector<char>& t_ok, const std::vector<long>& t_cell, float radius) {
  const long N = (long)xyz.size() / 3, T = (long)target.size() / 3;
  const long tiles = (N + 4095) / 4096;
  const float r2 = radius * radius;
  std::vector<double> leaves((size_t)tiles * 4096 * kL, 0.0);
  Pass out;
  out.nearest.assign((size_t)N, -2);
  out.dist2.assign((size_t)N, 0x7F800000u);
  out.moved.assign((size_t)N * 3, 0u);
  for (long i = 0; i < N; ++i) {
    const float* p = &xyz[i * 3];
    const float m[3] = {md::reg_move_axis(A, 0, p[0], p[1], p[2]), md::reg_move_axis(A, 1, p[0], p[1], p[2]), md::reg_move_axis(A, 2, p[0], p[1], p[2])};
    for (int a = 0; a < 3; ++a) out.moved[(size_t)i * 3 + a] = md::reg_out_bits(m[a]);
    long c[3];
    if (!cell_of(m, radius, c)) {
      ++out.dropped;
      continue;
    }
    ++out.in_range;
    out.nearest[i] = -1;
    uint64_t best = ~0ull;
    for (long j = 0; j < T; ++j) {
      if (!t_ok[j]) continue;
      const long* tc = &t_cell[j * 3];
      if (labs(tc[0] - c[0]) > 1 || labs(tc[1] - c[1]) > 1 || labs(tc[2] - c[2]) > 1) continue;
      const float dx = target[j * 3] - m[0], dy = target[j * 3 + 1] - m[1], dz = target[j * 3 + 2] - m[2];
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= r2) {
        uint32_t b;
        memcpy(&b, &d2, 4);
        const uint64_t key = ((uint64_t)b << 32) | (uint64_t)j;
        best = key < best ? key : best;
      }
    }
    if (best == ~0ull) continue;
    const uint32_t b = (uint32_t)(best >> 32);
    const size_t j = (size_t)(best & 0xFFFFFFFFull);
    out.nearest[i] = (int32_t)j;
    out.dist2[i] = b;
    if (!md::reg_normal_usable(&normals[j * 3])) continue;
    ++out.n;
    float d2;
    memcpy(&d2, &b, 4);
    md::reg_add_plane_leaves(&leaves[(size_t)i * kL], m, &target[j * 3], &normals[j * 3], d2);
  }
  std::vector<double> tile_sum((size_t)tiles * kL, 0.0);
  double v[256];
  for (long t = 0; t < tiles; ++t)
    for (int l = 0; l < kL; ++l) {
      for (int u = 0; u < 256; ++u) {
        double acc = 0.0;
        for (int s = 0; s < 16; ++s) acc = acc + leaves[((size_t)t * 4096 + s * 256 + u) * kL + l];
        v[u] = acc;
      }
      tile_sum[(size_t)t * kL + l] = workgroup(v);
    }
  for (int l = 0; l < kL; ++l) {
    for (int u = 0; u < 256; ++u) {
      double acc = 0.0;
      for (long t = u; t < tiles; t += 256) acc = acc + tile_sum[(size_t)t * kL + l];
      v[u] = acc;
    }
    out.S[l] = workgroup(v);
  }
  return out;
}

int run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 1;
  int32_t head[4];
  float radius;
  double eps[2], A[12];
  if (fread(head, 4, 4, f) != 4 || fread(&radius, 4, 1, f) != 1 || fread(eps, 8, 2, f) != 2 || fread(A, 8, 12, f) != 12) return 1;
  const int N = head[0], T = head[1], K = head[2], min_pairs = head[3];
  std::vector<float> xyz((size_t)N * 3), target((size_t)T * 3), normals((size_t)T * 3);
  if (fread(xyz.data(), 4, xyz.size(), f) != xyz.size() || fread(target.data(), 4, target.size(), f) != target.size() ||
      fread(normals.data(), 4, normals.size(), f) != normals.size())
    return 1;
  fclose(f);
  std::vector<char> t_ok((size_t)T);
  std::vector<long> t_cell((size_t)T * 3, 0);
  int in_grid = 0;
  for (int j = 0; j < T; ++j) {
    t_ok[j] = cell_of(&target[(size_t)j * 3], radius, &t_cell[(size_t)j * 3]);
    in_grid += t_ok[j];
  }
  std::vector<int> pairs((size_t)K + 1, 0);
  std::vector<double> sum_d2((size_t)K + 1, 0.0), sum_r2((size_t)K + 1, 0.0);
  int solves = 0, status = 0;
  for (int k = 0; k < K && status == 0; ++k) {
    const Pass ps = one_pass(A, xyz, target, normals, t_ok, t_cell, radius);
    pairs[k] = ps.n;
    sum_d2[k] = ps.S[28];
    sum_r2[k] = ps.S[27];
    if (ps.n < min_pairs) {
      status = 2;
      break;
    }
    double A_new[12];
    if (!md::reg_solve_plane(ps.n, ps.S, A, A_new)) {
      status = 3;
      break;
    }
    ++solves;
    if ((eps[0] > 0. || eps[1] > 0.) && md::reg_converged(A_new, A, eps[0], eps[1])) status = 1;
    memcpy(A, A_new, sizeof(A));
  }
  const Pass ps = one_pass(A, xyz, target, normals, t_ok, t_cell, radius);
  pairs[K] = ps.n;
  sum_d2[K] = ps.S[28];
  sum_r2[K] = ps.S[27];
  printf("A");
  for (int i = 0; i < 12; ++i) printf(" %016" PRIx64, bits_of(A[i]));
  printf(" pairs");
  for (int k = 0; k <= K; ++k) printf(" %d", pairs[k]);
  printf(" sum_d2");
  for (int k = 0; k <= K; ++k) printf(" %016" PRIx64, bits_of(sum_d2[k]));
  printf(" sum_r2");
  for (int k = 0; k <= K; ++k) printf(" %016" PRIx64, bits_of(sum_r2[k]));
  printf(" stats %d %d %d %d %d 0 0 0 dropped %d rows", solves, status, ps.in_range, ps.n, in_grid, ps.dropped);
  for (int i = 0; i < N; ++i)
    printf(" %d %08x %08x %08x %08x", ps.nearest[i], ps.dist2[i], ps.moved[(size_t)i * 3], ps.moved[(size_t)i * 3 + 1], ps.moved[(size_t)i * 3 + 2]);
  printf("\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (run(argv[i])) {
      fprintf(stderr, "cannot read %s\n", argv[i]);
      return 1;
    }
  return 0;
}
