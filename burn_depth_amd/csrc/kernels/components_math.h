// The union-find of the connected components (kernels/components.hip): `find` and `hook` over an atomic-access
// policy, so that the same text runs in the device kernels and in a host program (tests/native/components_host.cpp, where the
// policy is std::atomic and the threads are std::thread). A policy A has three static members over an int in memory, all relaxed:
//   int  A::load(const int* p)
//   void A::store(int* p, int v)
//   bool A::cas(int* p, int expected, int desired)     true = this call made the swap
//
// THE invariant: parent[v] <= v at all times. parent[v] == v: v is a root. Only three writes exist, and all keep it:
//   hook      a compare-and-swap parent[hi]: hi -> lo with lo < hi, on a root only;
//   compress  a store parent[v] = g where g was read as the parent of v's parent: g < v, in v's tree;
//   flatten   (after every hook) a store parent[v] = the root of v.
// A row that stopped being a root never becomes one again (every write stores a value below the row). Chains strictly descend,
// so `find` ends. What every write keeps, and what suffices: a value ever stored in parent[v] is below v and lies in v's tree,
// so it has v's root. (Halving may take a row OFF the path of v, so "once an ancestor, always an ancestor" does not hold; "same
// tree" does, because a tree only ever loses its root by being hooked, whole, under a row of another tree.) A compression
// that lands late therefore stores a row that still leads to v's root. The root of a finished component is its smallest row
// whatever the order of arrival, because a root is only ever hooked under a smaller row.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_COMPONENTS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MD_COMPONENTS_HD inline
#endif

namespace md {

// The root of v's tree at some moment of the call, with path halving: every row on the way is pointed at its grandparent.
// parent[] is read through the policy: a plain load may be hoisted out of the loop or served from a stale line.
template <class A>
MD_COMPONENTS_HD int components_find(int* parent, int v) {
  int p = A::load(parent + v);
  while (p != v) {
    const int g = A::load(parent + p);
    if (g != p) A::store(parent + v, g);  // g < p < v, a row of v's tree
    v = p;
    p = g;
  }
  return v;
}

// The root of v's tree with loads only. The flatten pass runs in place, parent[i] = root of i, while other threads still walk the
// same chains: a compression by one of them that lands after the root was stored would leave a row that is not the root in its
// place, so that pass stores roots and nothing else. Every value it meets lies in v's tree below the last, so the walk ends at
// the root all the same.
template <class A>
MD_COMPONENTS_HD int components_root(const int* parent, int v) {
  for (int p = A::load(parent + v); p != v; p = A::load(parent + v)) v = p;
  return v;
}

// Joins the trees of u and v. Lock-free: the swap fails only when another thread hooked `hi` in the meantime, which is progress
// of the whole; the loop then goes on from the two rows it holds, which are still members of their components. Nothing here
// waits for a value that another thread has yet to store.
template <class A>
MD_COMPONENTS_HD void components_hook(int* parent, int u, int v) {
  for (;;) {
    u = components_find<A>(parent, u);
    v = components_find<A>(parent, v);
    if (u == v) return;
    const int hi = u > v ? u : v, lo = u > v ? v : u;
    if (A::cas(parent + hi, hi, lo)) return;
  }
}

#if defined(__HIPCC__)
struct DeviceAtomics {  // the policy on device memory (kernels/components.hip, kernels/clusters.hip): relaxed, agent scope (served by L2)
  static MD_COMPONENTS_HD int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static MD_COMPONENTS_HD void store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static MD_COMPONENTS_HD bool cas(int* p, int expected, int desired) {
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
#endif

}  // namespace md
