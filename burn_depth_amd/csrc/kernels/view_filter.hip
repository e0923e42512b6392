// View filter kernels for gfx950 (md_op_filter_views, md_infer_points_filtered): an exact confidence percentile over all
// candidate pixels of the call, then the cross-view support count, in front of the unchanged point path. The output is the
// depth with rejected pixels set to 0, which the unprojection already treats as invalid. Contraction is off in the whole
// file (Makefile): every step is one rounded f32 operation, in the order pipeline.filter_views restates in numpy.
//
// tau (the k-th smallest candidate confidence, k = (N - 1) q / 100) comes from a radix select on the bit patterns, which
// order like the values for non-negative f32: four passes of 8 bits, top byte first, each a histogram launch (256 LDS bins
// per workgroup, one global add per non-empty bin: integer sums, so deterministic) and a one-workgroup select launch that
// narrows {prefix, mask, k} in device memory and clears the table. Passes 1..3 read the depth only of pixels whose
// confidence still matches the prefix. The support kernel reads tau from device memory: nothing returns to the host.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "points_math.h"
#include "tile_compact.h"

namespace md {

namespace {

constexpr int kBins = 256;
constexpr int kHistBlocks = 1024;  // 4 workgroups per CU: at most 1024 x 256 global adds per pass

struct SelectState {
  unsigned prefix, mask;  // the bits of tau's pattern fixed so far
  long long k, n;         // rank still to find among the matching candidates; candidates of the call
  float tau;
  int pad;
};

__device__ __forceinline__ bool depth_ok(const ViewFilterParams& p, float d) { return isfinite(d) && d >= p.dmin && d <= p.dmax; }
__device__ __forceinline__ bool conf_ok(float c) { return isfinite(c) && c >= 0.f; }
// -0 orders with +0
__device__ __forceinline__ unsigned conf_key(float c) { return c == 0.f ? 0u : __float_as_uint(c); }

__global__ void __launch_bounds__(kTileThreads) view_filter_hist_kernel(ViewFilterParams p, long total, int shift, unsigned* __restrict__ table,
                                                                    const SelectState* __restrict__ st) {
  __shared__ unsigned bins[kBins];
  const int tid = threadIdx.x, lane = tid & 63;
  bins[tid] = 0u;
  __syncthreads();
  const unsigned prefix = st->prefix, mask = st->mask;
  for (long base = (long)blockIdx.x * kTileThreads; base < total; base += (long)gridDim.x * kTileThreads) {  // uniform per workgroup
    const long i = base + tid;
    bool act = false;
    unsigned bin = 0u;
    if (i < total) {
      const float c = p.conf[i];
      if (conf_ok(c)) {
        const unsigned key = conf_key(c);
        if ((key & mask) == prefix && depth_ok(p, p.depth[i])) {
          act = true;
          bin = (key >> shift) & 255u;
        }
      }
    }
    // confidences share their top bytes: lanes of one bin add once per wave, for up to four bins; the rest add alone
    unsigned long long todo = __ballot(act);
    for (int round = 0; round < 4 && todo; ++round) {
      const int first = __ffsll((long long)todo) - 1;
      const unsigned fb = (unsigned)__shfl((int)bin, first, 64);
      const unsigned long long same = __ballot(act && bin == fb);
      if (lane == first) atomicAdd(&bins[fb], (unsigned)__popcll(same));
      if (act && bin == fb) act = false;
      todo &= ~same;
    }
    if (act) atomicAdd(&bins[bin], 1u);
  }
  __syncthreads();
  const unsigned c = bins[tid];
  if (c) atomicAdd(&table[tid], c);
}

// one workgroup: the bin that holds rank k, then the table is cleared for the next pass. shift = 24 also counts N and derives k.
__global__ void __launch_bounds__(kTileThreads) view_filter_select_kernel(unsigned* __restrict__ table, SelectState* __restrict__ st, int shift,
                                                                      int q, float* __restrict__ tau_out) {
  __shared__ long long incl[kBins];
  const int tid = threadIdx.x;
  const long long c = table[tid];
  table[tid] = 0u;
  incl[tid] = c;
  __syncthreads();
  for (int d = 1; d < kBins; d <<= 1) {
    const long long v = tid >= d ? incl[tid - d] : 0;
    __syncthreads();
    incl[tid] += v;
    __syncthreads();
  }
  long long n = st->n, k = st->k;
  const unsigned prefix = st->prefix, mask = st->mask;
  if (shift == 24) {
    n = incl[kBins - 1];
    k = n > 0 ? ((n - 1) * (long long)q) / 100 : 0;
  }
  __syncthreads();  // every thread has read the state
  const long long hi = incl[tid], lo = hi - c;
  if (n > 0 ? (c > 0 && lo <= k && k < hi) : tid == 0) {  // exactly one thread
    const unsigned pre = n > 0 ? (prefix | ((unsigned)tid << shift)) : 0u;
    st->prefix = pre;
    st->mask = mask | (255u << shift);
    st->k = n > 0 ? k - lo : 0;
    st->n = n;
    if (shift == 0) {
      const float tau = __uint_as_float(pre);
      st->tau = tau;
      if (tau_out) *tau_out = tau;
    }
  }
}

__device__ __forceinline__ bool survivor(const ViewFilterParams& p, long o, float d, float tau) {
  if (!depth_ok(p, d)) return false;
  if (!p.conf) return true;
  const float c = p.conf[o];
  return conf_ok(c) && c >= tau;
}

// grid (tiles, B), the grid of points_classify_kernel. The B cameras sit in LDS; a thread walks its 16 pixels and, for each survivor, the B - 1 other views.
__global__ void __launch_bounds__(kTileThreads) view_filter_support_kernel(ViewFilterParams p, const SelectState* __restrict__ st) {
  __shared__ Camera cams[kViewFilterMaxViews];
  __shared__ int wave_n[kTileWaves];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const bool views = p.rtol > 0.f;
  if (views && tid < p.B) cams[tid] = load_camera(p.K, p.focal, p.E, p.H, p.W, tid);
  __syncthreads();
  const float tau = st->tau;
  const long hw = (long)p.H * p.W;
  const float fw = (float)p.W, fh = (float)p.H;
  int n = 0;
  for (int s = 0; s < kTileSteps; ++s) {
    const long i = tile_item(tile, s);
    bool keep = false;
    if (i < hw) {
      const long o = (long)b * hw + i;
      const float d = p.depth[o];
      const bool surv = survivor(p, o, d, tau);
      int sup = 0;
      if (surv && views) {
        const int v = (int)(i / p.W), u = (int)(i % p.W);
        float x[3];
        unproject(cams[b], 1, p.off, v, u, d, x);
        for (int j = 0; j < p.B; ++j) {
          if (j == b) continue;
          const Camera& c = cams[j];
          const float px = ((c.r[0] * x[0] + c.r[1] * x[1]) + c.r[2] * x[2]) + c.t[0];
          const float py = ((c.r[3] * x[0] + c.r[4] * x[1]) + c.r[5] * x[2]) + c.t[1];
          const float pz = ((c.r[6] * x[0] + c.r[7] * x[1]) + c.r[8] * x[2]) + c.t[2];
          if (!(pz > 0.f)) continue;
          const float uf = ((c.fx * (px / pz)) + c.cx) - p.off;
          const float vf = ((c.fy * (py / pz)) + c.cy) - p.off;
          const float uu = floorf(uf + 0.5f), vv = floorf(vf + 0.5f);
          if (!(uu >= 0.f && uu < fw && vv >= 0.f && vv < fh)) continue;  // in float: a NaN or a huge value never converts
          const long oj = (long)j * hw + (long)(int)vv * p.W + (int)uu;
          const float dj = p.depth[oj];
          if (!survivor(p, oj, dj, tau)) continue;
          if (fabsf(pz - dj) <= p.rtol * fminf(pz, dj)) ++sup;
        }
      }
      keep = surv && sup >= p.min_views;
      if (p.depth_out) p.depth_out[o] = keep ? d : 0.f;
      if (p.support) p.support[o] = (uint8_t)sup;
    }
    if (p.kept) n += __popcll(__ballot(keep));  // the same in every lane of the wave
  }
  if (!p.kept) return;
  const int sum = tile_sum(n, wave_n);
  if (tid == 0 && sum) atomicAdd(&p.kept[b], sum);
}

__global__ void view_filter_total_kernel(int32_t* __restrict__ kept, int B) {
  if (threadIdx.x != 0) return;
  int sum = 0;
  for (int b = 0; b < B; ++b) sum += kept[b];
  kept[B] = sum;
}

constexpr size_t kStateAt = kBins * sizeof(unsigned);

}  // namespace

size_t view_filter_scratch_bytes() { return kStateAt + sizeof(SelectState); }

int launch_view_filter(const ViewFilterParams& p, void* scratch, hipStream_t s) {
  if (!scratch) MD_FAIL(MD_ERR_INVALID_ARG, "filter_views: no scratch buffer");
  if (p.rtol > 0.f && p.B > kViewFilterMaxViews) MD_FAIL(MD_ERR_SHAPE, "filter_views: %d views, at most %d", p.B, kViewFilterMaxViews);
  const long total = (long)p.B * p.H * p.W;
  unsigned* table = (unsigned*)scratch;
  SelectState* st = (SelectState*)((char*)scratch + kStateAt);
  // the table, the select state (tau = 0) and the counts are zeroed on the stream
  MD_HIP(hipMemsetAsync(scratch, 0, view_filter_scratch_bytes(), s));
  if (p.kept) MD_HIP(hipMemsetAsync(p.kept, 0, (size_t)(p.B + 1) * 4, s));
  if (p.q > 0) {
    const int blocks = (int)std::min<long>((total + kTileThreads - 1) / kTileThreads, kHistBlocks);
    for (int shift = 24; shift >= 0; shift -= 8) {
      hipLaunchKernelGGL(view_filter_hist_kernel, dim3(blocks), dim3(kTileThreads), 0, s, p, total, shift, table, st);
      MD_HIP(hipGetLastError());
      hipLaunchKernelGGL(view_filter_select_kernel, dim3(1), dim3(kTileThreads), 0, s, table, st, shift, p.q, p.tau);
      MD_HIP(hipGetLastError());
    }
  } else if (p.tau) {
    MD_HIP(hipMemsetAsync(p.tau, 0, 4, s));
  }
  if (!p.depth_out && !p.support && !p.kept) return MD_OK;  // tau only
  const int tiles = tiles_of((long)p.H * p.W);
  hipLaunchKernelGGL(view_filter_support_kernel, dim3(tiles, p.B), dim3(kTileThreads), 0, s, p, st);
  MD_HIP(hipGetLastError());
  if (p.kept) {
    hipLaunchKernelGGL(view_filter_total_kernel, dim3(1), dim3(64), 0, s, p.kept, p.B);
    MD_HIP(hipGetLastError());
  }
  return MD_OK;
}

}  // namespace md
