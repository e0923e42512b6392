// Host program over kernels/components_math.h: the union-find of the connected components with a std::atomic
// policy, run as the device runs it (hook over every valid face, then flatten over every row), once on one thread and once on up
// to 16 std::threads that take interleaved faces, and compared with a sequential union-find. Built by
// tests/test_components_host.py with -fsanitize=address,undefined; prints one line per shape and returns 0 when every label
// agrees and the invariant parent[v] <= v held wherever it was looked at.
// What this shows: find and hook end, keep the invariant and give the sequential labels on host threads. What it does not show:
// that the flatten pass is free of races. Sixteen host threads interleave far less than a GPU's waves, and a flatten that
// compressed paths in place, which loses a root to a late compression store on the device, passed here. The two loops below
// restate the hook and flatten kernels (one face / one row per step); only find, root and hook are shared with the device.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <thread>
#include <vector>

#include "kernels/components_math.h"

namespace {

struct StdAtomics {  // relaxed accesses of an int in memory
  static int load(const int* p) { return std::atomic_ref<int>(*const_cast<int*>(p)).load(std::memory_order_relaxed); }
  static void store(int* p, int v) { std::atomic_ref<int>(*p).store(v, std::memory_order_relaxed); }
  static bool cas(int* p, int expected, int desired) {
    return std::atomic_ref<int>(*p).compare_exchange_strong(expected, desired, std::memory_order_relaxed, std::memory_order_relaxed);
  }
};

struct Rng {  // a fixed 64-bit LCG (Knuth's MMIX constants): the shapes are the same on every run
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

struct Shape {
  const char* name;
  int n;
  std::vector<int> faces;  // [F,3]
};

bool valid(const int* f, int n) { return f[0] >= 0 && f[0] < n && f[1] >= 0 && f[1] < n && f[2] >= 0 && f[2] < n; }

void shuffle_faces(std::vector<int>& faces, Rng& r) {
  const int F = (int)faces.size() / 3;
  for (int i = F - 1; i > 0; --i) {
    const int j = r.below(i + 1);
    for (int k = 0; k < 3; ++k) std::swap(faces[i * 3 + k], faces[j * 3 + k]);
  }
}

Shape random_faces(const char* name, int F, Rng& r) {  // sparse enough to leave many components
  Shape s{name, std::max(2 * F, 4), {}};
  for (int f = 0; f < F; ++f) {
    const int a = r.below(s.n);
    s.faces.insert(s.faces.end(), {a, std::min(a + 1 + r.below(3), s.n - 1), r.below(s.n)});
  }
  return s;
}

Shape strip(const char* name, int F, int order, Rng& r) {  // 0-1-2, 1-2-3, ...: one long chain
  Shape s{name, F + 2, {}};
  for (int f = 0; f < F; ++f) {
    const int g = order == 1 ? F - 1 - f : f;
    s.faces.insert(s.faces.end(), {g, g + 1, g + 2});
  }
  if (order == 2) shuffle_faces(s.faces, r);
  return s;
}

Shape fan(const char* name, int F) {  // every face names row 0
  Shape s{name, F + 2, {}};
  for (int f = 0; f < F; ++f) s.faces.insert(s.faces.end(), {0, f + 1, f + 2});
  return s;
}

Shape islands(const char* name, int count, Rng& r) {  // disjoint strips of 1..8 faces, with a row between them that no face names
  Shape s{name, 0, {}};
  for (int i = 0; i < count; ++i) {
    const int k = 1 + i % 8;
    for (int f = 0; f < k; ++f) s.faces.insert(s.faces.end(), {s.n + f, s.n + f + 1, s.n + f + 2});
    s.n += k + 3;
  }
  shuffle_faces(s.faces, r);
  return s;
}

Shape invalid_corners(const char* name, Rng& r) {
  Shape s = random_faces(name, 500, r);
  for (int f = 0; f < 500; f += 7) s.faces[f * 3 + f % 3] = (f % 2) ? -1 : s.n;
  s.faces.insert(s.faces.end(), {3, 3, 9});  // degenerate faces join what they name
  s.faces.insert(s.faces.end(), {9, 9, 9});
  return s;
}

std::vector<int> sequential_labels(const Shape& s) {
  std::vector<int> parent(s.n);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int v) {
    while (parent[v] != v) v = parent[v];
    return v;
  };
  auto join = [&](int u, int v) {
    u = find(u); v = find(v);
    if (u != v) parent[std::max(u, v)] = std::min(u, v);
  };
  for (size_t f = 0; f * 3 < s.faces.size(); ++f) {
    const int* c = &s.faces[f * 3];
    if (!valid(c, s.n)) continue;
    join(c[0], c[1]);
    join(c[1], c[2]);
  }
  std::vector<int> label(s.n);
  for (int i = 0; i < s.n; ++i) label[i] = find(i);
  return label;
}

// the device's launches on `threads` threads: thread t takes the faces (rows) t, t + threads, ...
bool run(const Shape& s, int threads, const std::vector<int>& want) {
  std::vector<int> parent(s.n);
  std::iota(parent.begin(), parent.end(), 0);
  const int F = (int)s.faces.size() / 3;
  std::atomic<bool> broken{false};
  auto each = [&](auto body) {
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(body, t);
    body(0);
    for (std::thread& th : pool) th.join();
  };
  each([&](int t) {  // hook
    for (int f = t; f < F; f += threads) {
      const int* c = &s.faces[f * 3];
      if (!valid(c, s.n)) continue;
      md::components_hook<StdAtomics>(parent.data(), c[0], c[1]);
      md::components_hook<StdAtomics>(parent.data(), c[1], c[2]);
      for (int k = 0; k < 3; ++k)
        if (StdAtomics::load(&parent[c[k]]) > c[k]) broken = true;
    }
  });
  each([&](int t) {  // flatten
    for (int i = t; i < s.n; i += threads) {
      const int root = md::components_root<StdAtomics>(parent.data(), i);
      StdAtomics::store(&parent[i], root);
    }
  });
  int wrong = 0;
  for (int i = 0; i < s.n; ++i) wrong += parent[i] != want[i];
  std::printf("%-24s rows %6d faces %6d threads %2d : %s\n", s.name, s.n, F, threads, wrong || broken ? "WRONG" : "ok");
  return !wrong && !broken;
}

}  // namespace

int main() {
  Rng r{20261019ull};
  std::vector<Shape> shapes;
  shapes.push_back(Shape{"no faces", 5, {}});
  static const int sizes[] = {1, 63, 64, 65, 4095, 4096, 4097};
  static const char* names[] = {"F = 1", "F = 63", "F = 64", "F = 65", "F = 4095", "F = 4096", "F = 4097"};
  for (int i = 0; i < 7; ++i) shapes.push_back(random_faces(names[i], sizes[i], r));
  shapes.push_back(strip("strip ascending", 5000, 0, r));
  shapes.push_back(strip("strip descending", 5000, 1, r));
  shapes.push_back(strip("strip shuffled", 5000, 2, r));
  shapes.push_back(fan("fan", 10000));
  shapes.push_back(islands("islands", 2000, r));
  shapes.push_back(invalid_corners("invalid corners", r));
  const int threads = (int)std::min(16u, std::max(2u, std::thread::hardware_concurrency()));
  bool ok = true;
  for (const Shape& s : shapes) {
    const std::vector<int> want = sequential_labels(s);
    ok &= run(s, 1, want);
    ok &= run(s, threads, want);
  }
  return ok ? 0 : 1;
}
