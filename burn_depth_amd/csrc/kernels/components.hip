// Connected components of a mesh and island removal for gfx950 (md_op_mesh_components, md_infer_points_components; DESIGN 12.9,
// include/mi_depth.h states the contract): two rows are connected when a valid face names both, label[i] is the smallest row of
// row i's component, a component's size is its number of valid faces, and a face is kept when its component has at least
// min_faces faces. Integers only: no float is computed here at all, and nothing depends on the order of arrival.
// pipeline.mesh_components restates it.
//
// The labelling is a lock-free union-find (components_math.h: find with path halving, hook by compare-and-swap on a root; the
// invariant parent[v] <= v makes the root of a finished component its smallest row). The launches:
//   init     parent[i] = i, size[i] = 0, the five counters to 0
//   hook     one thread per live face: hook(p, q), hook(q, r); invalid faces counted with one integer add per wave
//   flatten  parent[i] = the root of i, in place and with loads only on the way (a compression racing with the store of a root
//            could leave an ancestor behind): a launch of its own, so the kernel boundary orders it behind every hook
//   count    size[label[p]] += 1 per valid face: ONE add of the popcount by the first lane when every valid lane of the wave
//            names the same root (the neighbouring faces of a depth-grid mesh mostly share a component), per-lane adds otherwise
//   rows     grid tiles of the rows: label, component_faces, the components (rows with label[i] == i and size > 0) counted in
//            total and kept, remap preset to -1, and the keep bits of the ROWS in the ballot layout (tile_compact.h): a row that a valid face
//            names lies in a component with size > 0 and a row that none names is alone with size 0, so "a face of a kept
//            component names row i" is size[label[i]] >= min_faces. No mark launch over the faces and no atomicOr is needed
//   (compact) launch_list_compact's scan and scatter on those bits, then the decimation's rank step for remap
//   select   grid tiles of the faces: keep = valid, its component large enough and, with compact, no mapped corner at or above
//            the capacity; dropped and clipped faces counted per wave
//   scan     launch_list_compact's scan on those words: tile offsets and face_count per view of the input faces
//   scatter  12-byte rows (through remap with compact) and face_index with plain stores
// No thread waits on another. Vector stores and integer global atomics only.
#include <algorithm>

#include "components_math.h"
#include "tile_compact.h"

namespace md {

namespace {

struct ComponentsScratch {  // 256-byte aligned parts
  int* parent;  // [n] the union-find; after flatten the label of every row
  int* size;    // [n] valid faces of the component, at its root
  int32_t* remap;   // [n] when the caller takes none
  int32_t* vcount;  // [B + 1] the row counts when the caller takes none
  unsigned long long* fbits;
  int* fcounts;
  int* foffsets;
  unsigned long long* vbits;
  int* vcounts;
  int* voffsets;
  int32_t* stats;  // [5] when the caller takes none
  size_t bytes;
};

ComponentsScratch carve(void* base, int n, int nf, int B) {
  const size_t nbf = (size_t)tiles_of(nf), nbv = (size_t)tiles_of(n);
  ComponentsScratch s;
  Carver c(base);
  s.parent = c.take<int>((size_t)n);
  s.size = c.take<int>((size_t)n);
  s.remap = c.take<int32_t>((size_t)n);
  s.vcount = c.take<int32_t>((size_t)(B + 1));
  s.fbits = c.take<unsigned long long>(nbf * kTileWords);
  s.fcounts = c.take<int>(nbf);
  s.foffsets = c.take<int>(nbf + 1);
  s.vbits = c.take<unsigned long long>(nbv * kTileWords);
  s.vcounts = c.take<int>(nbv);
  s.voffsets = c.take<int>(nbv + 1);
  s.stats = c.take<int32_t>(64);
  s.bytes = c.bytes;
  return s;
}

__device__ __forceinline__ bool valid_face(int a, int b, int c, int n) { return a >= 0 && a < n && b >= 0 && b < n && c >= 0 && c < n; }

// grid max(ceil(n / 256), 1)
__global__ void __launch_bounds__(kTileThreads) components_init_kernel(int n, int* __restrict__ parent, int* __restrict__ size,
                                                                   int32_t* __restrict__ stats) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i < n) {
    parent[i] = (int)i;
    size[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 5) stats[threadIdx.x] = 0;
}

// grid ceil(nf / 256); no thread leaves before the ballot
__global__ void __launch_bounds__(kTileThreads) components_hook_kernel(ComponentsParams p, int* parent, int32_t* __restrict__ stats) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  const bool live = f < live_count(p.in_face_count, p.v.B, p.nf);
  bool invalid = false;
  if (live) {
    const int n = live_count(p.v.in_count, p.v.B, p.v.n);
    const int a = p.faces[f * 3], b = p.faces[f * 3 + 1], c = p.faces[f * 3 + 2];
    invalid = !valid_face(a, b, c, n);
    if (!invalid) {
      components_hook<DeviceAtomics>(parent, a, b);
      components_hook<DeviceAtomics>(parent, b, c);
    }
  }
  wave_count_add(invalid, stats);
}

// grid ceil(n / 256). In place, while other threads of this launch walk the same chains: the walk compresses nothing, so the
// only stores of the launch are roots and parent[i] ends as the root of i whichever store comes last.
__global__ void __launch_bounds__(kTileThreads) components_flatten_kernel(int n, int* parent) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= n) return;
  const int root = components_root<DeviceAtomics>(parent, (int)i);
  DeviceAtomics::store(parent + i, root);
}

// grid ceil(nf / 256); no thread leaves before the ballots
__global__ void __launch_bounds__(kTileThreads) components_count_kernel(ComponentsParams p, const int* __restrict__ label, int* __restrict__ size) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool valid = false;
  int root = -1;
  if (f < live_count(p.in_face_count, p.v.B, p.nf)) {
    const int n = live_count(p.v.in_count, p.v.B, p.v.n);
    const int a = p.faces[f * 3], b = p.faces[f * 3 + 1], c = p.faces[f * 3 + 2];
    valid = valid_face(a, b, c, n);
    if (valid) root = label[a];
  }
  const unsigned long long act = __ballot(valid);
  if (!act) return;  // the whole wave
  const int leader = __ffsll((long long)act) - 1;
  const int first = __shfl(root, leader, 64);
  const unsigned long long same = __ballot(valid && root == first);
  if (same == act) {
    if (lane == leader) atomicAdd(size + first, (int)__popcll(act));
  } else if (valid) {
    atomicAdd(size + root, 1);
  }
}

// grid tiles of the rows
__global__ void __launch_bounds__(kTileThreads) components_rows_kernel(ComponentsParams p, const int* __restrict__ parent, const int* __restrict__ size,
                                                                   int32_t* __restrict__ remap, unsigned long long* __restrict__ bits,
                                                                   int* __restrict__ counts, int32_t* __restrict__ stats) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.v.in_count, p.v.B, p.v.n);
  int n = 0, total = 0, kept = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool keep = false, root = false;
    if (i < p.v.n) {
      int l = -1, sz = 0;
      if (i < live) {
        l = parent[i];
        sz = size[l];
        keep = sz >= p.min_faces;
        root = l == (int)i && sz > 0;
      }
      if (p.label) p.label[i] = l;
      if (p.component_faces) p.component_faces[i] = sz;
      if (remap) remap[i] = -1;  // the rank step overwrites the kept rows
    }
    n += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
    total += __popcll(__ballot(root));
    kept += __popcll(__ballot(root && keep));
  }
  if (lane == 0) {
    if (total) atomicAdd(stats + 3, total);
    if (kept) atomicAdd(stats + 4, kept);
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

// grid tiles of the faces. remap: null without compact.
__global__ void __launch_bounds__(kTileThreads) components_select_kernel(ComponentsParams p, const int* __restrict__ label, const int* __restrict__ size,
                                                                     const int32_t* __restrict__ remap, unsigned long long* __restrict__ bits,
                                                                     int* __restrict__ counts, int32_t* __restrict__ stats) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.in_face_count, p.v.B, p.nf), rows = live_count(p.v.in_count, p.v.B, p.v.n);
  int n = 0, dropped = 0, clipped = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long f = tile_item(tile, s);
    bool keep = false, drop = false, clip = false;
    if (f < live) {
      const int a = p.faces[f * 3], b = p.faces[f * 3 + 1], c = p.faces[f * 3 + 2];
      if (valid_face(a, b, c, rows)) {
        keep = size[label[a]] >= p.min_faces;
        drop = !keep;
        if (keep && remap) {
          clip = remap[a] >= p.v.capacity || remap[b] >= p.v.capacity || remap[c] >= p.v.capacity;
          keep = !clip;
        }
      }
    }
    n += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
    dropped += __popcll(__ballot(drop));
    clipped += __popcll(__ballot(clip));
  }
  if (lane == 0) {
    if (dropped) atomicAdd(stats + 1, dropped);
    if (clipped) atomicAdd(stats + 2, clipped);
  }
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

__global__ void __launch_bounds__(kTileThreads) components_scatter_kernel(ComponentsParams p, const int32_t* __restrict__ remap,
                                                                      const unsigned long long* __restrict__ bits, const int* __restrict__ offsets) {
  __shared__ int word_off[kTileWords];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const unsigned long long* words = bits + (long)tile * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const long base = offsets[tile];
  if (base >= p.face_capacity) return;  // everything of this workgroup lies beyond the capacity
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;
    const long idx = base + word_off[w] + lane_rank(word);
    if (idx >= p.face_capacity) continue;
    const long f = tile_item(tile, s);  // a live, valid face: the bit is only ever set for one
    if (p.faces_out) {
      const int32_t* src = p.faces + f * 3;
      int32_t* dst = p.faces_out + idx * 3;
      if (remap) {
        dst[0] = remap[src[0]]; dst[1] = remap[src[1]]; dst[2] = remap[src[2]];
      } else {
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
      }
    }
    if (p.face_index) p.face_index[idx] = (int32_t)f;
  }
}

}  // namespace

size_t components_scratch_bytes(int n, int nf, int B) { return carve(nullptr, n > 0 ? n : 0, nf > 0 ? nf : 0, B > 0 ? B : 1).bytes; }

int launch_mesh_components(const ComponentsParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "components need their scratch buffer");
  if (p.v.n < 0 || p.v.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "components take fewer than 2^30 rows, got %d", p.v.n);
  if (p.nf < 0 || p.nf >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "components take fewer than 2^30 faces, got %d", p.nf);
  if (p.v.B < 1) MD_FAIL(MD_ERR_SHAPE, "components of %d views", p.v.B);
  if (p.min_faces < 1) MD_FAIL(MD_ERR_INVALID_ARG, "min_faces = %d: must be >= 1", p.min_faces);
  if (p.v.capacity < 0 || p.face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "components: a negative capacity");
  if ((p.faces_out || p.face_index) && !p.face_count) MD_FAIL(MD_ERR_INVALID_ARG, "kept faces need `face_count`");
  if (p.nf > 0 && !p.faces) MD_FAIL(MD_ERR_INVALID_ARG, "components: the faces are null");
  if (!p.compact && (p.remap || p.v.xyz_out || p.v.conf_out || p.v.rgb_out || p.v.normals_out || p.v.index || p.v.count))
    MD_FAIL(MD_ERR_INVALID_ARG, "components: row outputs without `compact`");
  if (p.v.weight || p.v.dropped) MD_FAIL(MD_ERR_INVALID_ARG, "components have no weight and no dropped rows");
  const int n = p.v.n, nf = p.nf;
  const ComponentsScratch c = carve(scratch, n, nf, p.v.B);
  int32_t* stats = p.stats ? p.stats : c.stats;
  int32_t* remap = p.compact ? (p.remap ? p.remap : c.remap) : nullptr;
  const unsigned rows_grid = (unsigned)((n + kTileThreads - 1) / kTileThreads), faces_grid = (unsigned)((nf + kTileThreads - 1) / kTileThreads);
  hipLaunchKernelGGL(components_init_kernel, dim3(std::max(rows_grid, 1u)), dim3(kTileThreads), 0, s, n, c.parent, c.size, stats);
  MD_HIP(hipGetLastError());
  if (nf > 0) {
    hipLaunchKernelGGL(components_hook_kernel, dim3(faces_grid), dim3(kTileThreads), 0, s, p, c.parent, stats);
    MD_HIP(hipGetLastError());
  }
  if (n > 0 && nf > 0) {
    hipLaunchKernelGGL(components_flatten_kernel, dim3(rows_grid), dim3(kTileThreads), 0, s, n, c.parent);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(components_count_kernel, dim3(faces_grid), dim3(kTileThreads), 0, s, p, c.parent, c.size);
    MD_HIP(hipGetLastError());
  }
  if (n > 0) {
    hipLaunchKernelGGL(components_rows_kernel, dim3(tiles_of(n)), dim3(kTileThreads), 0, s, p, c.parent, c.size, remap, c.vbits, c.vcounts, stats);
    MD_HIP(hipGetLastError());
  }
  if (p.compact) {  // the rows: scan and scatter on the row bits, then the true rank of every kept row
    VoxelParams v = p.v;
    if (!v.count) v.count = c.vcount;  // the scan leaves the tile offsets only with a count to write
    MD_TRY(launch_list_compact(v, nullptr, nullptr, c.vbits, c.vcounts, c.voffsets, s));
    MD_TRY(launch_rank_rows(c.vbits, c.voffsets, n, remap, s));
  }
  if (nf > 0) {
    hipLaunchKernelGGL(components_select_kernel, dim3(tiles_of(nf)), dim3(kTileThreads), 0, s, p, c.parent, c.size, remap, c.fbits, c.fcounts, stats);
    MD_HIP(hipGetLastError());
  }
  if (!p.face_count) return MD_OK;
  VoxelParams fc;  // the scan reads the counts and the view boundaries of the input faces; without a row output it scatters nothing
  fc.in_count = p.in_face_count; fc.n = nf; fc.B = p.v.B; fc.count = p.face_count;
  MD_TRY(launch_list_compact(fc, nullptr, nullptr, c.fbits, c.fcounts, c.foffsets, s));
  if (nf == 0 || (!p.faces_out && !p.face_index)) return MD_OK;
  hipLaunchKernelGGL(components_scatter_kernel, dim3(tiles_of(nf)), dim3(kTileThreads), 0, s, p, remap, c.fbits, c.foffsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
