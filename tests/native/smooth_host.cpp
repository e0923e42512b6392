// Host program over kernels/smooth_math.h: the mesh smoothing run sequentially with the lines the device kernels
// run (quantise, topology, accumulate / update per step, normal accumulate, write), on the meshes that
// tests/test_smooth_host.py writes and names on the command line. Built by that test with -fsanitize=address,undefined. One
// line per mesh: an FNV-1a checksum of the bytes of the smoothed rows, one of the normals, and the five counters; the test
// compares them with pipeline.smooth_mesh.
// A mesh file: int32 N, F, iterations, pin_boundary; float step, lambda, mu; then float xyz [N,3]; then int32 faces [F,3].
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels/smooth_math.h"

namespace {

uint64_t fnv1a(const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h;
}

template <class T>
bool read_all(std::FILE* f, T* out, size_t count) { return count == 0 || std::fread(out, sizeof(T), count, f) == count; }

int run(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 1;
  int32_t head[4];
  float opts[3];
  bool ok = read_all(f, head, 4) && read_all(f, opts, 3);
  const int n = ok ? head[0] : 0, nf = ok ? head[1] : 0, iterations = head[2], pin = head[3];
  const float step = opts[0], lambda = opts[1], mu = opts[2];
  std::vector<float> xyz((size_t)n * 3);
  std::vector<int32_t> faces((size_t)nf * 3);
  ok = ok && read_all(f, xyz.data(), xyz.size()) && read_all(f, faces.data(), faces.size());
  std::fclose(f);
  if (!ok) return 1;

  std::vector<int64_t> k((size_t)n * 3, 0);
  std::vector<uint64_t> S((size_t)n * 3, 0), open(n, 0);
  std::vector<uint32_t> deg(n, 0);
  std::vector<int32_t> flag(n, 0);
  int32_t stats[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) flag[i] = md::smooth_quantise(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], step, &k[(size_t)i * 3]) ? 1 : 0;
  std::vector<int> live;  // the live faces
  for (int t = 0; t < nf; ++t) {
    const int32_t* v = &faces[(size_t)t * 3];
    const int kind = md::smooth_face_kind(v[0], v[1], v[2], n, flag.data());
    if (kind == 1) ++stats[0];
    if (kind == 2) ++stats[1];
    if (kind != 0) continue;
    live.push_back(t);
    for (int j = 0; j < 3; ++j) {
      deg[v[j]] += 2u;
      open[v[j]] += md::smooth_open_term(v[(j + 1) % 3], v[(j + 2) % 3]);
    }
  }
  const int steps = mu != 0.f ? 2 * iterations : iterations;
  for (int t = 0; t < steps; ++t) {
    const double factor = (double)((mu != 0.f && (t & 1)) ? mu : lambda);
    for (int face : live) {
      const int32_t* v = &faces[(size_t)face * 3];
      for (int j = 0; j < 3; ++j)
        for (int a = 0; a < 3; ++a)
          S[(size_t)v[j] * 3 + a] += (uint64_t)k[(size_t)v[(j + 1) % 3] * 3 + a] + (uint64_t)k[(size_t)v[(j + 2) % 3] * 3 + a];
    }
    for (int i = 0; i < n; ++i) {
      const bool pinned = md::smooth_pinned(deg[i], open[i], flag[i] != 0, pin);
      for (int a = 0; a < 3; ++a) {
        const size_t at = (size_t)i * 3 + a;
        if (!pinned) k[at] = md::smooth_step_axis((int64_t)S[at], deg[i], k[at], factor);
        S[at] = 0;
      }
    }
  }
  for (int face : live) {
    const int32_t* v = &faces[(size_t)face * 3];
    uint64_t x[3];
    md::smooth_cross(&k[(size_t)v[0] * 3], &k[(size_t)v[1] * 3], &k[(size_t)v[2] * 3], x);
    for (int j = 0; j < 3; ++j)
      for (int a = 0; a < 3; ++a) S[(size_t)v[j] * 3 + a] += x[a];
  }
  std::vector<float> out((size_t)n * 3), normals((size_t)n * 3);
  for (int i = 0; i < n; ++i) {
    int64_t k0[3] = {0, 0, 0};
    const bool in_range = md::smooth_quantise(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], step, k0);
    const int64_t* ki = &k[(size_t)i * 3];
    const bool moved = in_range && (ki[0] != k0[0] || ki[1] != k0[1] || ki[2] != k0[2]);
    stats[2] += !in_range;
    stats[3] += deg[i] > 0 && open[i] != 0;
    stats[4] += moved;
    for (int a = 0; a < 3; ++a) out[(size_t)i * 3 + a] = moved ? md::smooth_position(ki[a], step) : xyz[(size_t)i * 3 + a];
    const int64_t nrm[3] = {(int64_t)S[(size_t)i * 3], (int64_t)S[(size_t)i * 3 + 1], (int64_t)S[(size_t)i * 3 + 2]};
    md::smooth_normal(deg[i], nrm, &normals[(size_t)i * 3]);
  }
  std::printf("xyz %016llx normals %016llx stats %d %d %d %d %d\n", (unsigned long long)fnv1a(out.data(), out.size() * 4),
              (unsigned long long)fnv1a(normals.data(), normals.size() * 4), stats[0], stats[1], stats[2], stats[3], stats[4]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i)
    if (run(argv[i])) {
      std::fprintf(stderr, "cannot read %s\n", argv[i]);
      return 1;
    }
  return 0;
}
