// Vertex-clustering decimation of a mesh for gfx950 (md_op_decimate_mesh; DESIGN 12.8, include/mi_depth.h states the contract):
// one vertex per occupied voxel, chosen by voxel thinning's rule, the faces re-indexed to those vertices, collapsed faces and
// later copies of an oriented triangle dropped, the kept faces in input order. Selection only: no float is computed here at
// all (the cell of a vertex is voxel.hip's), and nothing depends on the order of arrival. pipeline.decimate_mesh restates it.
//
// The vertex side is launch_voxel_thin, unchanged, then two launches for remap[i] = the output row of the survivor of row i's
// voxel, from the scratch the thinning leaves:
//   rank     grid tiles: a kept row's output row = tile offset + popcounts below its bit (the scatter step of tile_compact.h)
//   remap    one thread per row that is not kept: the low word of its slot's rank names the survivor s; remap[i] = remap[s]
// The face side, six launches:
//   reset    table slots to -1, the class counters and the flag to 0
//   map      one thread per face: the mapped triple (or -1 in its first word when the face is invalid or degenerate); the two
//            class counters rise by one integer add per wave (ballot popcount)
//   insert   one thread per live face: the triple rotated so that its smallest index comes first, hashed, then linear probing
//            over a table whose slots hold FACE IDS (three indices below 2^30 do not fit a 64-bit compare-and-swap). An empty
//            slot is claimed with atomicCAS(-1 -> f); a slot that holds id g is compared through g's mapped triple, which the
//            map launch wrote (a plain load); on a match atomicMin(slot, f), otherwise the next slot. Every id that ever sits in
//            a slot has the same triple, so the slot's identity never changes and it ends as the smallest f of that triangle.
//            The face's slot is recorded
//   select   keep[f] = live and its slot holds f; ballot words in tile_compact.h's layout; duplicates counted per wave
//   scan     launch_list_compact's scan on those words: tile offsets and face_count per view of the input faces
//   scatter  12-byte rows and face_index with plain stores
// No thread waits on another: the probe loop is bounded by the table size and a lost compare-and-swap hands back the winner's
// id, which is examined like any other. Vector stores and integer global atomics only.
#include <algorithm>

#include "voxel_math.h"

namespace md {

namespace {

struct DecimateScratch {  // the parts behind voxel thinning's scratch, 256-byte aligned
  int32_t* count;     // [B + 1] the vertex counts when the caller takes none (the scan that leaves the tile offsets needs a home)
  int32_t* remap;     // [n] when the caller takes none
  int* table;         // [slots] face ids, -1 = empty
  int32_t* mapped;    // [nf,3] the mapped triple in the input's rotation; [0] = -1: invalid or degenerate
  int* fslot;         // [nf] the face's slot, -1: not live (or the probe loop ran out)
  unsigned long long* bits;
  int* counts;
  int* offsets;
  int* flags;  // [0] the probe loop ran out, [1..3] the class counters (when the caller takes none)
  size_t bytes;
};

// The two homes are carved whether or not the caller brings its own count and remap: the layout then depends on the shape alone,
// which is what decimate_flags and a model's grow-only buffer need. Untouched bytes of a scratch cost an allocation, no traffic.
DecimateScratch carve(void* base, int n, int nf, int B) {
  const size_t slots = voxel_table_slots(nf), nb = (size_t)tiles_of(nf);
  DecimateScratch s;
  Carver c(base, voxel_scratch_bytes(n));
  s.count = c.take<int32_t>((size_t)(B + 1));
  s.remap = c.take<int32_t>((size_t)n);
  s.table = c.take<int>(slots);
  s.mapped = c.take<int32_t>((size_t)nf * 3);
  s.fslot = c.take<int>((size_t)nf);
  s.bits = c.take<unsigned long long>(nb * kTileWords);
  s.counts = c.take<int>(nb);
  s.offsets = c.take<int>(nb + 1);
  s.flags = c.take<int>(64);
  s.bytes = c.bytes;
  return s;
}

// grid tiles of the rows. The output row of every kept row; the other rows are the next launch's.
__global__ void __launch_bounds__(kTileThreads) decimate_rank_kernel(const unsigned long long* __restrict__ bits, const int* __restrict__ offsets,
                                                                 int32_t* __restrict__ remap) {
  __shared__ int word_off[kTileWords];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const unsigned long long* words = bits + (long)tile * kTileWords;
  if (tid < kTileWords) scan_word_counts(__popcll(words[tid]), word_off);
  __syncthreads();
  const int base = offsets[tile];
  for (int s = 0; s < kTileSteps; ++s) {
    const int w = tile_word(s);
    const unsigned long long word = words[w];
    if (!((word >> lane) & 1ull)) continue;  // the bit is only ever set for a live row
    remap[tile_item(tile, s)] = base + word_off[w] + (int)lane_rank(word);
  }
}

// grid ceil(n / 256). A kept row keeps what the rank launch wrote; this launch reads only such rows and writes only the others.
__global__ void __launch_bounds__(kTileThreads) decimate_remap_kernel(const int32_t* __restrict__ in_count, int B, int n, const int* __restrict__ slot,
                                                                  const unsigned long long* __restrict__ rank, int32_t* remap) {
  const long i = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (i >= n) return;
  if (i >= live_count(in_count, B, n)) {
    remap[i] = -1;
    return;
  }
  const int h = slot[i];
  if (h < 0) {
    remap[i] = -1;
    return;
  }
  const unsigned s = 0xFFFFFFFFu - (unsigned)rank[h];  // the survivor of the row's voxel, a live row
  if (s != (unsigned)i) remap[i] = remap[s];
}

// slots is a multiple of 1024: every thread writes four slots with one 16-byte store
__global__ void __launch_bounds__(kTileThreads) decimate_reset_kernel(int4* __restrict__ table, size_t quads, int* __restrict__ flags,
                                                                  int32_t* __restrict__ dropped) {
  const size_t stride = (size_t)gridDim.x * kTileThreads;
  for (size_t q = (size_t)blockIdx.x * kTileThreads + threadIdx.x; q < quads; q += stride) table[q] = make_int4(-1, -1, -1, -1);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    flags[0] = 0;
    dropped[0] = 0;
    dropped[1] = 0;
    dropped[2] = 0;
  }
}

// grid ceil(nf / 256); no thread leaves before the ballots. n: the live rows, cap: the rows the vertex outputs hold.
__global__ void __launch_bounds__(kTileThreads) decimate_map_kernel(DecimateParams p, const int32_t* __restrict__ remap, int32_t* __restrict__ mapped,
                                                                int32_t* __restrict__ dropped) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  const bool live = f < live_count(p.in_face_count, p.v.B, p.nf);
  bool invalid = false, degenerate = false;
  if (live) {
    const int n = live_count(p.v.in_count, p.v.B, p.v.n);
    const int a = p.faces[f * 3], b = p.faces[f * 3 + 1], c = p.faces[f * 3 + 2];
    int ma = -1, mb = -1, mc = -1;
    if (a >= 0 && a < n && b >= 0 && b < n && c >= 0 && c < n) {
      ma = remap[a]; mb = remap[b]; mc = remap[c];
    }
    invalid = ma < 0 || mb < 0 || mc < 0 || ma >= p.v.capacity || mb >= p.v.capacity || mc >= p.v.capacity;
    degenerate = !invalid && (ma == mb || mb == mc || ma == mc);
    int32_t* dst = mapped + f * 3;
    dst[0] = (invalid || degenerate) ? -1 : ma; dst[1] = mb; dst[2] = mc;
  }
  wave_count_add(invalid, dropped);
  wave_count_add(degenerate, dropped + 1);
}

// the triple with its smallest index first; the three are distinct
__device__ __forceinline__ void rotate_min_first(int a, int b, int c, int* x, int* y, int* z) {
  if (a < b && a < c) { *x = a; *y = b; *z = c; }
  else if (b < a && b < c) { *x = b; *y = c; *z = a; }
  else { *x = c; *y = a; *z = b; }
}

// grid ceil(nf / 256). mask = slots - 1.
__global__ void __launch_bounds__(kTileThreads) decimate_insert_kernel(DecimateParams p, const int32_t* __restrict__ mapped, int* table,
                                                                   unsigned long long mask, int* __restrict__ fslot, int* __restrict__ flags) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (f >= live_count(p.in_face_count, p.v.B, p.nf)) return;
  if (mapped[f * 3] < 0) {
    fslot[f] = -1;
    return;
  }
  int a, b, c;
  rotate_min_first(mapped[f * 3], mapped[f * 3 + 1], mapped[f * 3 + 2], &a, &b, &c);
  unsigned long long h = grid_mix64(grid_mix64(((unsigned long long)a << 30) | (unsigned long long)b) ^ (unsigned long long)c) & mask;
  for (unsigned long long probe = 0; probe <= mask; ++probe) {
    int cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < 0) cur = atomicCAS(table + h, -1, (int)f);  // returns what was there: -1 = this thread claimed the slot
    if (cur < 0) {
      fslot[f] = (int)h;
      return;
    }
    int x, y, z;  // the slot's triangle: the triple of whichever id it holds
    rotate_min_first(mapped[(long)cur * 3], mapped[(long)cur * 3 + 1], mapped[(long)cur * 3 + 2], &x, &y, &z);
    if (x == a && y == b && z == c) {
      atomicMin(table + h, (int)f);
      fslot[f] = (int)h;
      return;
    }
    h = (h + 1) & mask;
  }
  flags[0] = 1;  // every slot holds another triangle: cannot happen at load <= 0.5
  fslot[f] = -1;
}

// grid tiles of the faces. A face is kept when it is live and the slot it ended in holds it.
__global__ void __launch_bounds__(kTileThreads) decimate_select_kernel(DecimateParams p, const int32_t* __restrict__ mapped, const int* __restrict__ table,
                                                                   const int* __restrict__ fslot, unsigned long long* __restrict__ bits,
                                                                   int* __restrict__ counts, int32_t* __restrict__ dropped) {
  __shared__ int wave_n[kTileWaves];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int live = live_count(p.in_face_count, p.v.B, p.nf);
  int n = 0, dup = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long f = tile_item(tile, s);
    bool keep = false, copy = false;
    if (f < live && mapped[f * 3] >= 0) {
      const int h = fslot[f];
      keep = h >= 0 && table[h] == (int)f;
      copy = h >= 0 && !keep;
    }
    n += ballot_step(keep, bits + (long)tile * kTileWords + tile_word(s));
    dup += __popcll(__ballot(copy));
  }
  if (lane == 0 && dup) atomicAdd(dropped + 2, dup);
  const int sum = tile_sum(n, wave_n);
  if (tid == 0) counts[tile] = sum;
}

__global__ void __launch_bounds__(kTileThreads) decimate_scatter_kernel(DecimateParams p, const int32_t* __restrict__ mapped,
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
    const long f = tile_item(tile, s);  // a live face: the bit is only ever set for one
    if (p.faces_out) {
      const int32_t* src = mapped + f * 3;
      int32_t* dst = p.faces_out + idx * 3;
      dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    if (p.face_index) p.face_index[idx] = (int32_t)f;
  }
}

// grid ceil(rows / 256), at least one workgroup: the first min(count[B], capacity) faces and the B + 1 counts, nothing behind them
__global__ void __launch_bounds__(kTileThreads) decimate_copy_faces_kernel(const int32_t* __restrict__ faces, const int32_t* __restrict__ count, int B,
                                                                       long rows, int32_t* __restrict__ faces_out, int32_t* __restrict__ count_out,
                                                                       long capacity) {
  const long f = (long)blockIdx.x * kTileThreads + threadIdx.x;
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b <= B; b += kTileThreads) count_out[b] = count[b];
  if (!faces_out) return;
  long live = count[B];
  live = live < rows ? live : rows;
  live = live < capacity ? live : capacity;
  if (f >= live) return;
  faces_out[f * 3] = faces[f * 3]; faces_out[f * 3 + 1] = faces[f * 3 + 1]; faces_out[f * 3 + 2] = faces[f * 3 + 2];
}

}  // namespace

int launch_copy_faces(const int32_t* faces, const int32_t* count, int B, long rows, int32_t* faces_out, int32_t* count_out, long capacity,
                      hipStream_t s) {
  if (!count_out) return MD_OK;
  if (!faces || !count || B < 1 || rows < 0 || capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "face copy: a bad argument");
  const long covered = faces_out ? std::min(rows, capacity) : 0;
  const unsigned grid = (unsigned)std::max<long>((covered + kTileThreads - 1) / kTileThreads, 1);
  hipLaunchKernelGGL(decimate_copy_faces_kernel, dim3(grid), dim3(kTileThreads), 0, s, faces, count, B, rows, faces_out, count_out, capacity);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

int launch_rank_rows(const unsigned long long* bits, const int* offsets, int n, int32_t* remap, hipStream_t s) {
  if (n <= 0) return MD_OK;
  if (!bits || !offsets || !remap) MD_FAIL(MD_ERR_INVALID_ARG, "rank step: a null argument");
  hipLaunchKernelGGL(decimate_rank_kernel, dim3(tiles_of(n)), dim3(kTileThreads), 0, s, bits, offsets, remap);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

size_t decimate_scratch_bytes(int n, int nf, int B) { return carve(nullptr, n > 0 ? n : 0, nf > 0 ? nf : 0, B > 0 ? B : 1).bytes; }

const int32_t* decimate_flags(const void* scratch, int n, int nf, int B) {
  return carve((void*)scratch, n > 0 ? n : 0, nf > 0 ? nf : 0, B > 0 ? B : 1).flags;
}

int launch_decimate_mesh(const DecimateParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "decimation needs its scratch buffer");
  if (p.v.n < 0 || p.v.n >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "decimation takes fewer than 2^30 rows, got %d", p.v.n);
  if (p.nf < 0 || p.nf >= (1 << 30)) MD_FAIL(MD_ERR_SHAPE, "decimation takes fewer than 2^30 faces, got %d", p.nf);
  if (p.v.B < 1) MD_FAIL(MD_ERR_SHAPE, "decimation of %d views", p.v.B);
  if (p.v.capacity < 0 || p.face_capacity < 0) MD_FAIL(MD_ERR_INVALID_ARG, "decimation: a negative capacity");
  if ((p.faces_out || p.face_index) && !p.face_count) MD_FAIL(MD_ERR_INVALID_ARG, "decimated faces need `face_count`");
  if (p.nf > 0 && !p.faces) MD_FAIL(MD_ERR_INVALID_ARG, "decimation: the faces are null");
  const DecimateScratch d = carve(scratch, p.v.n, p.nf, p.v.B);
  DecimateParams q = p;
  if (!q.v.count) q.v.count = d.count;  // the scan leaves the tile offsets only with a count to write
  MD_TRY(launch_voxel_thin(q.v, scratch, s));
  const bool face_side = p.faces_out || p.face_index || p.face_count || p.faces_dropped;
  if (!p.remap && !face_side) return MD_OK;
  int32_t* remap = p.remap ? p.remap : d.remap;
  if (p.v.n > 0) {
    const VoxelRanks r = voxel_ranks(scratch, p.v.n);
    hipLaunchKernelGGL(decimate_rank_kernel, dim3(tiles_of(p.v.n)), dim3(kTileThreads), 0, s, r.bits, r.offsets, remap);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(decimate_remap_kernel, dim3((p.v.n + kTileThreads - 1) / kTileThreads), dim3(kTileThreads), 0, s, p.v.in_count, p.v.B, p.v.n, r.slot,
                       r.rank, remap);
    MD_HIP(hipGetLastError());
  }
  if (!face_side) return MD_OK;
  const size_t slots = voxel_table_slots(p.nf), quads = slots / 4;
  const int nb = tiles_of(p.nf);
  int32_t* dropped = p.faces_dropped ? p.faces_dropped : d.flags + 1;
  const unsigned reset_grid = (unsigned)std::min<size_t>((quads + kTileThreads - 1) / kTileThreads, 256 * 32);
  hipLaunchKernelGGL(decimate_reset_kernel, dim3(reset_grid), dim3(kTileThreads), 0, s, (int4*)d.table, quads, d.flags, dropped);
  MD_HIP(hipGetLastError());
  if (p.nf > 0) {
    const unsigned faces_grid = (unsigned)((p.nf + kTileThreads - 1) / kTileThreads);
    hipLaunchKernelGGL(decimate_map_kernel, dim3(faces_grid), dim3(kTileThreads), 0, s, q, remap, d.mapped, dropped);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(decimate_insert_kernel, dim3(faces_grid), dim3(kTileThreads), 0, s, q, d.mapped, d.table, (unsigned long long)(slots - 1),
                       d.fslot, d.flags);
    MD_HIP(hipGetLastError());
    hipLaunchKernelGGL(decimate_select_kernel, dim3(nb), dim3(kTileThreads), 0, s, q, d.mapped, d.table, d.fslot, d.bits, d.counts, dropped);
    MD_HIP(hipGetLastError());
  }
  if (!p.face_count) return MD_OK;
  VoxelParams c;  // the scan reads the counts and the view boundaries of the input faces; without a row output it scatters nothing
  c.in_count = p.in_face_count; c.n = p.nf; c.B = p.v.B; c.count = p.face_count;
  MD_TRY(launch_list_compact(c, nullptr, nullptr, d.bits, d.counts, d.offsets, s));
  if (p.nf == 0 || (!p.faces_out && !p.face_index)) return MD_OK;
  hipLaunchKernelGGL(decimate_scatter_kernel, dim3(nb), dim3(kTileThreads), 0, s, q, d.mapped, d.bits, d.offsets);
  MD_HIP(hipGetLastError());
  return MD_OK;
}

}  // namespace md
