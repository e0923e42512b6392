// K5: fused multi-head attention for gfx950, bf16 MFMA operands / fp32 softmax and accumulation.
//
//   out[q, h*64 + d] = sum_k softmax_k(q.k / 8) * v[k, d]        head_dim = 64 (ViT-L/16, ViT-S/14)
//
// Layout contract (produced by the QKV GEMM epilogue, gemm.hip EPI_QKV):
//   qk  [rows, 2D]  bf16 / f16, row = seq*S + token; q (pre-scaled by kAttnQScale) at column h*64, k at column D + h*64
//   vT  [seq][head][64][kpad] bf16: V transposed so that keys are contiguous (the P.V MFMA wants
//       both operands K-contiguous; the transpose is paid once in the GEMM epilogue).
//
// One workgroup = 4 waves = 128 consecutive queries of one (sequence, head); a wave owns 32
// queries. K and V^T tiles of 64 keys are streamed through a 2-stage LDS ring with
// global_load_lds (swizzled on the source address like the GEMM), shared by the 4 waves.
// "Swapped" QK^T: S^T = K.Q^T puts one query per lane (column) and 16 keys per lane in the
// accumulator registers, so the online-softmax max/sum are in-register reductions plus ONE
// cross-half exchange, and the exponentiated accumulator registers are -- after a bf16 pack --
// directly the B operand of the P.V MFMA (no LDS round trip, no cross-lane movement). The key
// order inside a 32-key sub-tile is permuted (bits 2 and 3 of the key index swapped when K rows
// are read from LDS) so that registers 8s..8s+7 hold the 8 consecutive keys the V^T fragment
// of k-step s holds.
#include <atomic>
#include <mutex>
#include "ops.h"
#include "elem.h"

namespace md {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// v_mfma_f32_32x32x16 on bf16 or IEEE half fragments (same rate, same layout)
template <typename T>
__device__ __forceinline__ f32x16_t mfma32(const i32x4_t& a, const i32x4_t& b, const f32x16_t& c) {
  typedef typename Native<T>::v8 v8;
  if constexpr (std::is_same<T, bf16_t>::value)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  else  // f16_t and the planes of f16s_t
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void glds16a(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// grid: 1-D, workgroups of 4 waves = 4 x 32 queries of one (sequence, head); block 256. The block -> (unit, q block) map is
// XCD-aware: blocks b and b+8 share an XCD, so logical ids are dealt in contiguous ranges per XCD and
// the q blocks of one (sequence, head) run on ONE XCD -- its K and V^T (148 KB) are fetched into that
// L2 once instead of once per q block (measured before the remap: 1.0 GB fetched per launch against
// 0.27 GB of q/k/v).
//
// Softmax arithmetic. q arrives PRE-SCALED by head_dim^-0.5 * log2(e) (ops.h kAttnQScale), so the MFMA result is the
// logit in log2 units and p = 2^(s - m) is one v_exp_f32 with no multiply. Two softmax bodies:
//  * FAST (bf16 operands): m = 0 for the whole row -- p = 2^s, no running maximum, no subtraction, no rescale of O.
//    bf16 has the fp32 exponent range, so p, the fp32 sums l and O and the final O / l are exact in the same sense as
//    with a maximum subtracted as long as nothing leaves the fp32 range. That is CHECKED, not assumed: the true row
//    maxima of tile 0 must lie within +-64 log2 units = +-44 in natural logit units (no underflow of a whole row: some
//    p >= 2^-64), and the row sums must stay below 2^100 (an overflow to inf or a NaN fails that test too; with the sums
//    below 2^100 and |v| far below 2^27 nothing in O overflows either). Trained ViT logits sit well inside +-44. A wave that fails raises a flag in LDS and the WHOLE workgroup (the
//    tiles are shared through LDS) runs the pass again in the safe body: rare by construction, and tested with inputs
//    that force it (tools/gpu_diag.py check_attention).
//    f16 operands run the same body with ONE fixed offset per row, m = the row's maximum over tile 0 (the range check
//    computes it anyway): p = 2^(s - m) costs a subtraction per score but still no running maximum, no dependent
//    reduction in front of the exponentials and no rescale. P must fit f16 (65504): checked through the row sums, which
//    bound every p and must stay below 57000.
//  * SAFE (workgroups that failed a check): running maximum with deferred rescale (raised, and O, l rescaled, only when
//    some row of the wave saw a score more than 2^kDefer above it); p <= 2^kDefer fits f16.
// Either way the result is softmax(q k^T / 8) v; which body ran only changes rounding.
//
// What bounds it (MI355X; DESIGN.md section 5.2, tools/probes/attn_mix_probe.hip, profiles/r03_attention_mix_ceiling.txt): on random
// operands the bare MFMA sequence of a tile sustains 1703 TFLOP/s (the clock under load), with the softmax's vector work 1394,
// with the sixteen fragment reads 1250, with LDS-DMA + vmcnt(0) + barrier per tile from an L2-resident source 1056-1107, with the
// kernel's real traffic (five workgroups share the tiles of a (sequence, head)) 876-1077 -- the kernel executes 820-920: it sits at
// the rate of its own structure under hipcc. Variants that measured slower (each correct): deeper rings, an intra-wave software
// pipeline, a two-group schedule, 64 queries per wave, one or five waves per SIMD, row sums on the matrix pipe or on v_dot2c,
// 8-wave workgroups, whole-tile fragment prefetch at three waves per SIMD, register-staged K / V^T tiles.
//
// Split-half operands (T = f16s_t, MD_PREC_F16X2): q, k and v arrive as hi + lo planes -- qk rows are
// [q_hi | q_lo | k_hi | k_lo] (each D wide), V^T has its lo plane `v_plane` elements behind the hi plane. The scores run on
// three terms, S = k_hi.q_hi + k_lo.q_hi + k_hi.q_lo (the lo.lo term is below 2^-22), and O on P.(v_hi + v_lo) with P rounded
// to one half (PTERMS = 1: its rounding averages over the keys; tools/precision_study.py prices it) or as hi + lo as well
// (PTERMS = 2: a third MFMA, P_lo.v_hi). A stage holds the four tiles (32 KB), two stages 64 KB: two workgroups per CU, so the
// kernel is built for two waves per SIMD (256 registers) instead of four. Softmax, row sums and O stay fp32 as before.
//
// Small launches (KS = 2, QW = 2; one-plane types; >= 1024 keys and at most kKeySplitBlocks workgroups of the plain form): a single image
// of a thousand-odd tokens gives far fewer workgroups than the chip has CUs (DA3 `small` at 518^2: 6 heads x 11 blocks of 128 queries =
// 66), one wave per SIMD, and that wave runs the MFMAs and the softmax of its 22 key tiles one after the other (0.44 us per tile: the
// launch is that chain plus ~7 us of floor, prologue and epilogue). Here a workgroup is QW = 2 query waves (64 queries: twice the
// workgroups) x KS = 2 key groups: group g walks the g-th half of the key tiles through its own two-stage ring for the same queries;
// the fast body keeps no running maximum, so the partial (O, l) of the groups simply add (f16: after moving to a common fixed offset),
// through the idle rings once the walks are done -- each SIMD still holds one wave, with half the chain. (KS = 4 groups of four query
// waves on the same 66 workgroups gained 9 % stand-alone and nothing in the model: profiles/r04_attention_key_split.txt -- the CU does
// the same work either way; spreading it over twice the CUs is what shortens the chain.) The rule depends on the launch size, so the
// last bits of a DA3 result may differ between one image and a batch; Depth Pro's 577-key sequences never take it. The rare safe pass
// runs un-split on group 0.
// (Round 5 measured and removed -- commit 6e0680d has the code: a loader-wave form, a fifth wave per workgroup issuing every LDS-DMA piece so that
// the query waves never touch the vector-memory pipe: correct, 0.84x, profiles/r05_attention_loader_wave.txt; s_setprio placements: nothing,
// profiles/r05_attention_prio.txt.)
// The body of one workgroup: `id` = its logical (unit, query block) index. Two kernels run it: attention_kernel (one workgroup per
// index, XCD-aware block order) and attention_redo_kernel (the safe body over the units the assembly kernel flagged).
//
// Cross-view keys (MV; attention_views_kernel): the sequences come in groups of `views` consecutive ones (the views
// of one scene) and a query of any of them attends over the n_tokens keys of EVERY sequence of its group, in sequence order -- one softmax
// over views * n_tokens keys. The walk is the same walk over views * NT tiles (tile u = view * NT + t sits in ring stage u & 1): K and V^T
// are addressed from the group's first sequence through ONE descriptor each, a view adds a scalar offset (view * S rows of q | k, view *
// heads * 64 * kpad elements of V^T), and every view's last tile masks its own rows past n_tokens (behind them lie the padding rows up to S
// and then the NEXT view's rows: they are read, so the mask is what keeps them out). Row sums, the O accumulator, the fast body's range
// check (first tile of the first view; a score in a later view that leaves the range shows in the row sums like one in a later tile) and
// the safe body's running maximum carry across the view boundary unchanged. One key group only (KS = 1): a launch over V views has V
// times the workgroups of the single-view launch, which is what the key split was there to provide.
template <typename T, bool FP8OUT, bool FAST, int PTERMS = 1, int KS = 1, int QW = 4, bool MV = false>
__device__ __forceinline__ void attention_body(const T* __restrict__ qk, const T* __restrict__ vT, T* __restrict__ out,
                                               int S, int n_tokens, int heads, int D, int kpad, int qblocks,
                                               float out_fp8_inv, long v_plane, const int id, const int views = 1) {
  constexpr bool SP = is_split<T>::value;
  static_assert(!MV || (KS == 1 && QW == 4 && !FP8OUT), "cross-view keys run in the plain form");
  constexpr int STAGE = SP ? 32768 : 16384;  // K tile 64x128B + V^T tile 64x128B (split-half: hi tiles, then the lo tiles 16 KB behind)
  // Split-half, one key group (the Depth Pro form): the four tiles of a stage are 32 KB, two stages 64 KB = two workgroups per CU, two
  // waves per SIMD, although the 148 registers allow three. CK (compact K): ONE K buffer (hi | lo, 16 KB) + TWO V^T stages (hi | lo,
  // 16 KB each) = 48 KB, three workgroups per CU. K is needed only by the score MFMAs at the head of a tile: behind them a second
  // workgroup barrier ("mid") frees the K buffer and the next tile's K is requested there -- it has the softmax and the P.V MFMAs of
  // this tile to land --, V^T stays double-buffered and is requested a whole tile ahead as before.
  constexpr bool CK = SP && KS == 1;
  constexpr int RING = CK ? 49152 : 2 * STAGE;  // LDS bytes of one key group's buffers
  // byte offsets inside a stage (CK: inside the K buffer / a V^T stage) of the lo planes, and of the V^T tile
  constexpr int KLO = CK ? 8192 : 16384, VLO = CK ? 8192 : 16384, VOFF = CK ? 0 : 8192;
  // one-plane types: static LDS (two stages | redo flag); split-half: 48 / 64 KB + flag as dynamic LDS (above the static limit)
  constexpr bool DYN = SP || KS > 1;
  static_assert(KS == 1 || (!FP8OUT && FAST && KS * RING <= 131072), "the key split is built for the fast body; the rings must fit the LDS");
  static_assert(QW == 4 || (QW == 2 && KS > 1), "two query waves per workgroup come with the key split");
  constexpr int NJ = 4 / QW;  // 8-row groups of a 32-row half tile each wave of a key group moves (4 waves: one each)
  __shared__ __attribute__((aligned(16))) char smem_static[DYN ? 16 : 2 * STAGE + 16];
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  char* const smem = DYN ? smem_dyn : smem_static;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = KS > 1 ? (wave_all % QW) : wave_all;  // the query wave: 32 queries
  const int grp = KS > 1 ? (wave_all / QW) : 0;          // the key group (own ring)
  char* const ring = smem + grp * RING;
  // K buffer / V^T stage of tile t
  auto kbuf = [&](int t) __attribute__((always_inline)) { return CK ? ring : ring + (t & 1) * STAGE; };
  auto vbuf = [&](int t) __attribute__((always_inline)) { return CK ? ring + 16384 + (t & 1) * 16384 : ring + (t & 1) * STAGE + VOFF; };
  const int unit = id / qblocks, qb = id - unit * qblocks;
  int seq = unit / heads, head = unit - seq * heads;
  int seq0 = seq;  // the sequence K and V^T are addressed from
  if constexpr (MV) {  // units in (group, head, view) order: the workgroups that walk the same keys are neighbours (one XCD's L2)
    const int per = views * heads, g = unit / per, w = unit - g * per;
    head = w / views;
    seq0 = g * views;
    seq = seq0 + (w - head * views);
  }
  const int q0 = qb * (32 * QW) + wave * 32;
  const bool active = q0 < n_tokens;  // wave-uniform
  const int h = lane >> 5, c = lane & 31;
  const long two_d = 2L * D * kPlanes<T>;  // elements per q | k row (split-half: [q_hi | q_lo | k_hi | k_lo])
  const long seq_row0 = (long)seq * S;

  // ---- Q fragments (B operand of S^T = K.Q^T): lane (c,h) holds Q[q0+c][16s + 8h + j] ----
  i32x4_t qf[4], qfl[SP ? 4 : 1];
  {
    int q = q0 + c;
    q = q < n_tokens ? q : n_tokens - 1;
    const char* qp = (const char*)(qk + (seq_row0 + q) * two_d + head * 64) + h * 16;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *(const i32x4_t*)(qp + s * 32);
    if constexpr (SP) {
#pragma unroll
      for (int s = 0; s < 4; ++s) qfl[s] = *(const i32x4_t*)(qp + (long)D * sizeof(T) + s * 32);
    }
  }

  // ---- global->LDS: 16 row-groups of 8 rows per stage (8 K + 8 V^T), 2 + 2 per wave of a four-wave key group (4 + 4 with two
  //      query waves): rows r0 .. r0+7 and r0+32 .. r0+39 of
  //      each tile (the two share one swizzled chunk index). LDS-DMA through buffer descriptors of this (sequence, head):
  //      the per-lane byte offset is tile-invariant (one VGPR each for K and V^T) and the tile's offset is a scalar, so
  //      issuing a tile costs no vector instruction (with per-lane 64-bit addresses it cost 12, and 3-6 % of the kernel) ----
  const unsigned krow_bytes = (unsigned)(two_d * sizeof(T));
  // K descriptor: the n_tokens key rows of this (sequence, head). The last tile addresses up to 63 rows past them: whether the
  // hardware's range check (which covers the vector offset; the scalar offset is implementation-defined) returns zeros for
  // them or reads them, they are masked below -- the callers keep >= 64 rows of slack behind the last sequence for the latter.
  // (split-half: k_hi starts 2D into the row and k_lo D behind it: one descriptor, its range extended by that D)
  const int klo_bytes = SP ? D * (int)sizeof(T) : 0;
  // MV: both descriptors start at the group's first sequence and reach to the last view's rows (the launcher keeps that below 2 GB)
  const long key_row0 = MV ? (long)seq0 * S : seq_row0;
  const int vview_bytes = MV ? heads * 64 * kpad * (int)sizeof(T) : 0;  // V^T: from one sequence to the next
  const int kviews_rows = MV ? (views - 1) * S : 0, vviews_bytes = MV ? (views - 1) * vview_bytes : 0;
  const auto ksrd = __builtin_amdgcn_make_buffer_rsrc((void*)(qk + key_row0 * two_d + (SP ? 2 * D : D) + head * 64), 0, (int)((unsigned)(n_tokens - 1 + kviews_rows) * krow_bytes + 128u) + klo_bytes, 0x00020000);
  const auto vsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(vT + ((long)seq0 * heads + head) * 64 * kpad), 0, 64 * kpad * (int)sizeof(T) + vviews_bytes, 0x00020000);
  const auto vsrd_lo = __builtin_amdgcn_make_buffer_rsrc((void*)(vT + (SP ? v_plane : 0) + ((long)seq0 * heads + head) * 64 * kpad), 0, 64 * kpad * (int)sizeof(T) + vviews_bytes, 0x00020000);
  int kvoff[2], vvoff[2];  // NJ <= 2 (a fixed bound: an array of template-dependent size captured by the lambdas below loses the kernel's host stub)
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int r0 = (wave + QW * j) * 8 + (lane >> 3);
    const int lc0 = (lane & 7) ^ ((r0 >> 1) & 7);
    kvoff[j] = r0 * (int)krow_bytes + lc0 * 16;
    vvoff[j] = r0 * kpad * (int)sizeof(T) + lc0 * 16;
  }
  const int NT = (n_tokens + 63) / 64;
  // Tile t of view `vw` into the ring stage of walk position u (one view: u = t, vw = 0).
  auto issue_k = [&](int u, int t, int vw) __attribute__((always_inline)) {
    const int row0 = MV ? vw * S : 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      __attribute__((address_space(3))) char* kb = (__attribute__((address_space(3))) char*)(kbuf(u) + (wave + QW * j) * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ksrd, kb + i * 4096, 16, kvoff[j], (row0 + t * 64 + i * 32) * (int)krow_bytes, 0, 0);
        if constexpr (SP) __builtin_amdgcn_raw_ptr_buffer_load_lds(ksrd, kb + KLO + i * 4096, 16, kvoff[j], (row0 + t * 64 + i * 32) * (int)krow_bytes + klo_bytes, 0, 0);
      }
    }
  };
  auto issue_v = [&](int u, int t, int vw) __attribute__((always_inline)) {
    const int v0 = MV ? vw * vview_bytes : 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      __attribute__((address_space(3))) char* vb = (__attribute__((address_space(3))) char*)(vbuf(u) + (wave + QW * j) * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(vsrd, vb + i * 4096, 16, vvoff[j], v0 + t * 128 + i * 32 * kpad * (int)sizeof(T), 0, 0);
        if constexpr (SP) __builtin_amdgcn_raw_ptr_buffer_load_lds(vsrd_lo, vb + VLO + i * 4096, 16, vvoff[j], v0 + t * 128 + i * 32 * kpad * (int)sizeof(T), 0, 0);
      }
    }
  };
  // the whole tile's requests (CK: only the V^T half; K follows at the previous tile's mid barrier)
  auto issue = [&](int u, int t, int vw) __attribute__((always_inline)) {
    if constexpr (!CK) issue_k(u, t, vw);
    issue_v(u, t, vw);
  };

  // LDS read offsets. K rows are read through the bit-2/bit-3 swap; V^T rows (= d) directly.
  const int pk = (c & 0x13) | ((c & 4) << 1) | ((c & 8) >> 1);
  int koff[2], voff[2];
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    const int R = sub * 32 + pk;
    koff[sub] = R * 128 + ((((R >> 1) & 7) ^ h) << 4);  // chunk (2s+h) ^ swz -> xor (s<<5) per k-step
  }
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    const int R = dt * 32 + c;
    voff[dt] = R * 128 + ((((R >> 1) & 7) ^ h) << 4);  // chunk (sub*4 + 2s' + h) ^ swz, inside the V^T tile
  }

  constexpr float kDefer = 6.0f;        // log2 units: p <= 64 in the safe body
  constexpr float kFastRange = 64.0f;   // |row max of tile 0| allowed for the fast body (log2 units)
  constexpr bool kOffsetFast = is_half<T>::value;  // fast body with the tile-0 row maximum as a fixed offset
  // a (partial) row sum at or above this (inf / NaN included) fails the fast body: 2^100 for bf16; f16: every p < 65504
  constexpr float kFastSumMax = kOffsetFast ? 57000.0f : 1.2676506e30f;

  f32x16_t o[2];
  float m_run, l_run;
  bool bad = false;  // wave-uniform: a fast-body range check failed

  int cv = 0;  // MV: the view whose tiles are being walked
  // what follows tile t of view cv in the walk, handed to `f(u + 1, tile, view)`: the view's next tile, or the next view's first
  auto with_next = [&](int u, int t, auto f) __attribute__((always_inline)) {
    if constexpr (MV) {
      const bool wrap = t + 1 >= NT;
      const int nv = wrap ? cv + 1 : cv;
      if (nv < views) f(u + 1, wrap ? 0 : t + 1, nv);
    } else {
      if (t + 1 < NT) f(t + 1, t + 1, 0);
    }
  };
  // every wave of the workgroup runs these statements exactly once per tile
  auto top = [&](int u, int t) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    with_next(u, t, issue);
  };
  // CK: behind a tile's score MFMAs -- every wave has read its K fragments (the MFMAs that consumed them are issued) -- the single K
  // buffer takes the next tile's K. An inactive wave (no valid query) meets the same barrier from `idle_mid`.
  auto mid = [&](int u, int t) __attribute__((always_inline)) {
    if constexpr (CK) {
      // a raw barrier behind the wave's own LDS reads: __syncthreads() would also drain vmcnt, i.e. wait for the V^T tile requested
      // a few hundred cycles ago at the top of this tile
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      with_next(u, t, issue_k);
    }
  };
  // S^T[sub] = K[sub] . Q^T (log2 units: q is pre-scaled); register r of lane half h holds local key (r&7) + 8h + 16(r>>3)
  auto scores_sub = [&](int u, int sub, f32x16_t& st) __attribute__((always_inline)) {
    const char* sb = kbuf(u);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const i32x4_t kf = *(const i32x4_t*)(sb + (koff[sub] ^ (s << 5)));
      const f32x16_t cin = s == 0 ? (f32x16_t){0.f} : st;  // first k-step: inline-constant 0 as C
      st = mfma32<T>(kf, qf[s], cin);
      if constexpr (SP) {  // + k_lo.q_hi + k_hi.q_lo
        const i32x4_t kl = *(const i32x4_t*)(sb + KLO + (koff[sub] ^ (s << 5)));
        st = mfma32<T>(kl, qf[s], st);
        st = mfma32<T>(kf, qfl[s], st);
      }
    }
  };
  // keys beyond the sequence get -inf (2^-inf = 0); last tile only
  auto mask_sub = [&](int t, int sub, f32x16_t& st) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = t * 64 + sub * 32 + (r & 7) + 8 * h + 16 * (r >> 3);
      if (key >= n_tokens) st[r] = -INFINITY;
    }
  };
  auto max16 = [&](const f32x16_t& st) __attribute__((always_inline)) {
    float mx = fmaxf(fmaxf(st[0], st[1]), st[2]);
#pragma unroll
    for (int r = 3; r + 1 < 16; r += 2) mx = fmaxf(fmaxf(mx, st[r]), st[r + 1]);
    return fmaxf(mx, st[15]);
  };
  // p = 2^(s - m) for 32 keys, packed as the B operand of the P.V MFMAs; adds the lane's partial row sums into ps[4]
  auto exp_pack_sub = [&](const f32x16_t& st, float m, i32x4_t (&pf)[2], i32x4_t (&pfl)[2], float (&ps)[4], auto no_offset) __attribute__((always_inline)) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      float p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = __builtin_amdgcn_exp2f(decltype(no_offset)::value ? st[8 * s2 + j] : st[8 * s2 + j] - m);
        ps[j & 3] += p[j];
      }
      pf[s2][0] = pack2_nosat<T>(p[0], p[1]);
      pf[s2][1] = pack2_nosat<T>(p[2], p[3]);
      pf[s2][2] = pack2_nosat<T>(p[4], p[5]);
      pf[s2][3] = pack2_nosat<T>(p[6], p[7]);
      if constexpr (SP && PTERMS == 2) {  // P as hi + lo: lo = f16(p - f16(p))
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
          float a, b;
          widen2<T>((unsigned)pf[s2][j2], a, b);
          pfl[s2][j2] = pack2_nosat<T>(p[2 * j2] - a, p[2 * j2 + 1] - b);
        }
      }
    }
  };
  // O^T[dt] += V^T[dt][keys of sub] . P^T[sub]: k-step s2 holds local keys 16 s2 .. 16 s2 + 15 of the 32-key block
  auto pv_sub = [&](int u, int sub, const i32x4_t (&pf)[2], const i32x4_t (&pfl)[2], int nsteps) __attribute__((always_inline)) {
    const char* sb = vbuf(u);
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      if (s2 < nsteps) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const i32x4_t vf = *(const i32x4_t*)(sb + (voff[dt] ^ ((sub * 4 + 2 * s2) << 4)));
          o[dt] = mfma32<T>(vf, pf[s2], o[dt]);
          if constexpr (SP) {  // + v_lo.P (+ v_hi.P_lo)
            const i32x4_t vl = *(const i32x4_t*)(sb + VLO + (voff[dt] ^ ((sub * 4 + 2 * s2) << 4)));
            o[dt] = mfma32<T>(vl, pf[s2], o[dt]);
            if constexpr (PTERMS == 2) o[dt] = mfma32<T>(vf, pfl[s2], o[dt]);
          }
        }
      }
    }
  };
  // One 64-key tile. SAFE: running maximum; PARTIAL: the sequence ends inside the tile -- blocks and k-steps without a
  // valid key are skipped (Depth Pro: 577 = 9 x 64 + 1 keys, the last tile costs 4 + 2 MFMAs instead of 16); CHECK: the
  // fast body's one-time range check on the true row maxima (first tile: key 0 is always valid: finite, +inf or NaN).
  // (u: the ring stage's walk position, t: the tile inside its sequence -- what the mask counts from)
  auto tile = [&](int u, int t, auto safe_c, auto partial_c, auto check_c) __attribute__((always_inline)) {
    constexpr bool SAFE = decltype(safe_c)::value, PARTIAL = decltype(partial_c)::value, CHECK = decltype(check_c)::value;
    const int rem = PARTIAL ? n_tokens - t * 64 : 64;  // valid keys of this tile (wave-uniform)
    const bool two = !PARTIAL || rem > 32;             // the second 32-key block holds valid keys
    f32x16_t st0, st1;
    i32x4_t pf0[2], pf1[2], pfl0[2], pfl1[2];
    float ps[4] = {0.f, 0.f, 0.f, 0.f};
    scores_sub(u, 0, st0);
    if (two) scores_sub(u, 1, st1);
    mid(u, t);
    if constexpr (PARTIAL) {
      mask_sub(t, 0, st0);
      if (two) mask_sub(t, 1, st1);
    }
    if constexpr (SAFE || CHECK) {
      float mx = max16(st0);
      if (two) mx = fmaxf(mx, max16(st1));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      if constexpr (CHECK) {
        bad = __any(!(fabsf(mx) <= kFastRange));
        if constexpr (kOffsetFast && !SAFE) m_run = mx;  // the row's fixed offset for the rest of the pass
      }
      if constexpr (SAFE) {
        if (__any((mx - m_run) > kDefer)) {  // wave-uniform branch
          const float m_new = fmaxf(m_run, mx);
          const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
          m_run = m_new;
          l_run *= alpha;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
      }
    }
    typedef std::integral_constant<bool, !SAFE && !kOffsetFast> no_offset_t;
    exp_pack_sub(st0, m_run, pf0, pfl0, ps, no_offset_t());
    pv_sub(u, 0, pf0, pfl0, PARTIAL && rem <= 16 ? 1 : 2);
    if (two) {
      exp_pack_sub(st1, m_run, pf1, pfl1, ps, no_offset_t());
      pv_sub(u, 1, pf1, pfl1, PARTIAL && rem <= 48 ? 1 : 2);
    }
    l_run += (ps[0] + ps[1]) + (ps[2] + ps[3]);
  };
  const bool last_partial = (n_tokens & 63) != 0;
  const int NFULL = last_partial ? NT - 1 : NT;  // tiles without masked keys
  // one pass over the keys in the fast (m = 0) or the safe body
  auto pass = [&](auto safe_c) __attribute__((always_inline)) {
    constexpr bool SAFE = decltype(safe_c)::value;
    typedef std::integral_constant<bool, !SAFE> check_t;  // the fast pass checks its first tile
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    m_run = SAFE ? -INFINITY : 0.f;  // safe: alpha = 2^-inf = 0 multiplies zeros at the first tile
    l_run = 0.f;
    if constexpr (MV) {
      // views * NT tiles, the first one peeled for the range check; the stage alternates with the walk position u, not with t
      cv = 0;
      if constexpr (CK) issue_k(0, 0, 0);
      issue(0, 0, 0);
      top(0, 0);
      if (active) {
        if (NFULL == 0) tile(0, 0, safe_c, std::true_type(), check_t());
        else tile(0, 0, safe_c, std::false_type(), check_t());
      } else {
        mid(0, 0);
      }
      int u = 1;
      for (; cv < views; ++cv) {
        for (int t = cv == 0 ? 1 : 0; t < NFULL; ++t, ++u) {
          top(u, t);
          if (active) tile(u, t, safe_c, std::false_type(), std::false_type());
          else mid(u, t);
        }
        if (last_partial && (cv > 0 || NT > 1)) {
          top(u, NT - 1);
          if (active) tile(u, NT - 1, safe_c, std::true_type(), std::false_type());
          else mid(u, NT - 1);
          ++u;
        }
      }
    } else if constexpr (KS == 1) {
      if constexpr (CK) issue_k(0, 0, 0);
      issue(0, 0, 0);
      top(0, 0);
      if (active) {
        if (NFULL == 0) tile(0, 0, safe_c, std::true_type(), check_t());
        else tile(0, 0, safe_c, std::false_type(), check_t());
      } else {
        mid(0, 0);
      }
      for (int t = 1; t < NFULL; ++t) {
        top(t, t);
        if (active) tile(t, t, safe_c, std::false_type(), std::false_type());
        else mid(t, t);
      }
      if (last_partial && NT > 1) {
        top(NT - 1, NT - 1);
        if (active) tile(NT - 1, NT - 1, safe_c, std::true_type(), std::false_type());
        else mid(NT - 1, NT - 1);
      }
    } else {
      // this group's tiles [tb, te): a quarter of the keys in the fast pass; the safe pass runs on group 0 alone. Every wave of
      // the workgroup meets the same `per` barriers (a group with fewer tiles idles through the rest).
      const int per = SAFE ? NT : (NT + KS - 1) / KS;
      const int tb = grp * per < NT ? grp * per : NT;
      const int te = SAFE ? (grp == 0 ? NT : 0) : (tb + per < NT ? tb + per : NT);
      const int n = te > tb ? te - tb : 0;  // an idle group (safe pass: every group but 0) takes exactly `per` barriers below
      const int nfull = (last_partial && te == NT) ? n - 1 : n;  // this group's tiles without masked keys
      auto top_g = [&](int t) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < te) issue(t + 1, t + 1, 0);
      };
      if (n > 0) {
        issue(tb, tb, 0);
        top_g(tb);
        if (active) {
          if (nfull == 0) tile(tb, tb, safe_c, std::true_type(), check_t());
          else tile(tb, tb, safe_c, std::false_type(), check_t());
        }
        for (int t = tb + 1; t < tb + nfull; ++t) {
          top_g(t);
          if (active) tile(t, t, safe_c, std::false_type(), std::false_type());
        }
        if (nfull < n && n > 1) {
          top_g(te - 1);
          if (active) tile(te - 1, te - 1, safe_c, std::true_type(), std::false_type());
        }
      }
      for (int i = n; i < per; ++i) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  };
  bool use_safe = !FAST;
  if constexpr (FAST) {
    int* redo = (int*)(smem + KS * RING);  // behind the buffers in every LDS form
    if (tid == 0) *redo = 0;
    pass(std::false_type());
    if (active) bad = bad || __any(!(l_run < kFastSumMax));  // a tile row sum >= 2^100, inf or NaN shows in the total
    if (bad && lane == 0) *redo = 1;
    __syncthreads();
    use_safe = *(volatile int*)redo != 0;  // workgroup-uniform
    if (use_safe) __syncthreads();        // everyone has read the flag and left the last tiles before stage 0 is reloaded
  }
  if (use_safe) pass(std::true_type());
  if constexpr (KS > 1) {
    if (use_safe) {
      if (grp > 0) return;  // the safe pass ran on group 0
    } else {
      // the groups' partial sums meet in the (now idle) ring: 34 floats per lane and wave, lane-contiguous
      float* const xch = (float*)smem;
      __syncthreads();  // every group has left its last tile
      if (grp > 0 && active) {
        float* px = xch + ((grp - 1) * QW + wave) * (34 * 64) + lane;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) px[(dt * 16 + r) * 64] = o[dt][r];
        px[32 * 64] = l_run;
        px[33 * 64] = m_run;
      }
      __syncthreads();
      if (grp > 0) return;
      if (active) {
#pragma unroll
        for (int g = 1; g < KS; ++g) {
          const float* px = xch + ((g - 1) * QW + wave) * (34 * 64) + lane;
          float a = 1.f, b = 1.f;
          if constexpr (kOffsetFast) {  // f16: each group ran on its own fixed offset (the row maximum of its first tile)
            const float mg = px[33 * 64];
            const float mn = fmaxf(m_run, mg);
            a = __builtin_amdgcn_exp2f(m_run - mn);
            b = __builtin_amdgcn_exp2f(mg - mn);
            m_run = mn;
          }
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = kOffsetFast ? o[dt][r] * a + px[(dt * 16 + r) * 64] * b : o[dt][r] + px[(dt * 16 + r) * 64];
          l_run = kOffsetFast ? l_run * a + px[32 * 64] * b : l_run + px[32 * 64];
        }
      }
    }
  }

  if (!active) return;
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv_l = 1.0f / l_tot;
  const int q = q0 + c;
  if constexpr (FP8OUT) {  // e4m3 rows for an fp8-operand output projection
    if (q < n_tokens) {
      char* orow8 = (char*)out + (seq_row0 + q) * (long)D + head * 64;
      const float sc = inv_l * out_fp8_inv;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int d = dt * 32 + 8 * q4 + 4 * h;
          auto cl = [&](float a) { return __builtin_amdgcn_fmed3f(a * sc, -448.f, 448.f); };
          int w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(o[dt][4 * q4]), cl(o[dt][4 * q4 + 1]), 0, false);
          w = __builtin_amdgcn_cvt_pk_fp8_f32(cl(o[dt][4 * q4 + 2]), cl(o[dt][4 * q4 + 3]), w, true);
          *(int*)(orow8 + d) = w;
        }
    }
  } else if (q < n_tokens) {
    T* orow = out + (seq_row0 + q) * (long)(D * kPlanes<T>) + head * 64;  // split-half rows: [hi: D | lo: D]
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int d = dt * 32 + 8 * q4 + 4 * h;
        store4p<T>(orow + d, D, (f32x4_t){o[dt][4 * q4] * inv_l, o[dt][4 * q4 + 1] * inv_l, o[dt][4 * q4 + 2] * inv_l, o[dt][4 * q4 + 3] * inv_l});
      }
  }
}

template <typename T, bool FP8OUT, bool FAST, int PTERMS = 1, int KS = 1, int QW = 4>
__global__ __launch_bounds__(64 * QW * KS, is_split<T>::value ? (KS == 1 ? 3 : 2) : 4) void attention_kernel(const T* __restrict__ qk, const T* __restrict__ vT, T* __restrict__ out,
                                                           int S, int n_tokens, int heads, int D, int kpad, int qblocks,
                                                           float out_fp8_inv, long v_plane) {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  attention_body<T, FP8OUT, FAST, PTERMS, KS, QW>(qk, vT, out, S, n_tokens, heads, D, kpad, qblocks, out_fp8_inv, v_plane, id);
}

// Cross-view keys: the same grid and block order; units are (group of `views` sequences, head, view).
template <typename T, int PTERMS = 1>
__global__ __launch_bounds__(256, is_split<T>::value ? 3 : 4) void attention_views_kernel(const T* __restrict__ qk, const T* __restrict__ vT, T* __restrict__ out,
                                                           int S, int n_tokens, int heads, int D, int kpad, int qblocks, long v_plane, int views) {
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  attention_body<T, false, true, PTERMS, 1, 4, true>(qk, vT, out, S, n_tokens, heads, D, kpad, qblocks, 0.f, v_plane, id, views);
}

// The units (sequence, head) whose row sums left the fast body's range in the assembly kernel (attn577_gfx950.s raises redo[unit]) run
// again in the running-maximum body. Two launches behind the assembly kernel (round 6; one serial walk of 4 units x 5 query blocks per
// workgroup before: a single flagged unit cost five query blocks one after the other, every unit flagged 2.2x the HIP kernel at 37 sequences):
//   attention_redo_scan_kernel   ONE workgroup compacts the raised flags into list[2..] (list[0] = their count), clears them and adds the count
//                                to the per-device diagnostic counter (md_debug_attention_redo_units);
//   attention_redo_kernel        a grid of at most four workgroups per CU walks the (flagged unit, query block) items, grid-strided: with no
//                                flag raised -- every launch on the seeded weights -- each workgroup is one load; with every flag raised it
//                                is the HIP kernel's own launch shape.
// `redo` holds cap >= nunits flags followed by the list (2 + cap ints): attention_redo_ints(cap). The list sits behind the buffer's whole
// capacity, not behind this launch's units: a launch over fewer sequences (a smaller batch, a call without the FOV encoder) would otherwise
// leave its list on flag slots that a later, larger launch reads as raised.
__global__ __launch_bounds__(1024) void attention_redo_scan_kernel(int* __restrict__ redo, int nunits, int cap, unsigned long long* __restrict__ stats) {
  __shared__ int count;
  int* list = redo + cap;
  if (threadIdx.x == 0) count = 0;
  __syncthreads();
  for (int u = threadIdx.x; u < nunits; u += 1024) {
    if (redo[u]) {
      list[2 + atomicAdd(&count, 1)] = u;  // the order of the list is not deterministic; every item is computed independently of it
      redo[u] = 0;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    list[0] = count;
    if (stats && count) atomicAdd(stats, (unsigned long long)count);
  }
}

__global__ __launch_bounds__(256) void attention_redo_kernel(const bf16_t* __restrict__ qk, const bf16_t* __restrict__ vT, bf16_t* __restrict__ out,
                                                             int S, int n_tokens, int heads, int D, int kpad, int qblocks, const int* __restrict__ list) {
  const int items = list[0] * qblocks;  // workgroup-uniform
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    if (it != (int)blockIdx.x) __syncthreads();  // the previous item's last tile has been read by every wave before the stages are refilled
    const int j = it / qblocks;
    attention_body<bf16_t, false, false>(qk, vT, out, S, n_tokens, heads, D, kpad, qblocks, 0.f, 0L, list[2 + j] * qblocks + (it - j * qblocks));
  }
}

// split-half attention: P as one half (1) or as hi + lo (2: what the product runs, every test and every published number).
// The two A/B switches below exist in DIAGNOSTIC builds only (`make DIAG=1` defines MD_DIAG_KNOBS): the shipped library reads no
// environment variable that changes numerics or kernel choice.
//   MD_ATTN_PTERMS=1    P in one plane (depth L_inf 3.2e-4 instead of 1.3e-4 for +1 % frames/s)
//                        (round 5: taking the row sums from the ROUNDED probabilities as well -- a consistent normaliser -- changes nothing:
//                        L_inf 3.0e-4 against 3.3e-4, profiles/r05_attention_f16x2_pterms.txt)
//   MD_ATTN_KEYSPLIT=0  the small-launch form off
#ifdef MD_DIAG_KNOBS
static int diag_env(const char* name, int dflt) {
  const char* e = getenv(name);
  return (e && e[0] >= '0' && e[0] <= '9') ? e[0] - '0' : dflt;
}
static int attn_pterms() {
  static const int v = diag_env("MD_ATTN_PTERMS", 2) == 1 ? 1 : 2;
  return v;
}
static bool key_split_enabled() {
  static const int v = diag_env("MD_ATTN_KEYSPLIT", 1);
  return v != 0;
}
#else
static constexpr int attn_pterms() { return 2; }
static constexpr bool key_split_enabled() { return true; }
#endif

// launches that take the small-launch form: sequences of >= 16 key tiles, and so few workgroups of the plain form (128 queries each)
// that most CUs would idle
static constexpr int kKeySplitMin = 1024, kKeySplitBlocks = 128;

static thread_local int g_attn_small_ok = 1;
int attention_allow_small(int on) {
  const int prev = g_attn_small_ok;
  g_attn_small_ok = on ? 1 : 0;
  return prev;
}

static thread_local AttnForm g_attn_last_form;
void attention_note_form(int form, long grid, int qw, int ks) {
  g_attn_last_form.form = form;
  g_attn_last_form.grid = (int)(grid < 0x7fffffffL ? grid : 0x7fffffffL);
  g_attn_last_form.qw = qw;
  g_attn_last_form.ks = ks;
}
AttnForm attention_last_form() { return g_attn_last_form; }

// ---- the assembly-owned Depth Pro form (kernels/attn577_gfx950.s, generated by tools/attn_asm/gen_attn577.py) ----
// bf16, exactly 577 tokens (576 patches + the class token), head_dim 64: one workgroup of four waves per (sequence, head), one wave
// per SIMD with the whole register file. Its code object is embedded in this library (attn577_blob.S) and loaded per device by
// attention_asm_prepare() -- hipModuleLoadData is not capturable, so the model calls that when it is created, not at first launch.
extern "C" const unsigned char md_attn577_co[];
namespace {
struct AsmKernel {
  std::atomic<int> state{0};  // 0 not loaded, 1 loaded, -1 failed
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  int cus = 0;  // one persistent workgroup per CU (it owns the CU: 512 registers per wave, one wave per SIMD)
  unsigned long long* stats = nullptr;  // device counter: units the assembly kernel flagged since the last reset (diagnostic)
};
AsmKernel g_asm[64];
std::mutex g_asm_mu;
// the A/B switch is process-wide (round 5's was per host thread: the bench's worker threads kept the assembly kernel while the
// line said "hip kernel"); graphs captured before a change keep their form
std::atomic<int> g_attn_asm_ok{1};
std::atomic<long> g_attn_asm_launches{0};
}  // namespace

int attention_allow_asm(int on) { return g_attn_asm_ok.exchange(on ? 1 : 0, std::memory_order_acq_rel); }

long attention_asm_launches() { return g_attn_asm_launches.load(std::memory_order_relaxed); }

int attention_redo_ints(int nunits) { return 2 * nunits + 2; }

long attention_asm_redo_units(int reset) {
  int ordinal = 0;
  if (hipGetDevice(&ordinal) != hipSuccess || ordinal < 0 || ordinal >= 64) return -1;
  AsmKernel& k = g_asm[ordinal];
  if (k.state.load(std::memory_order_acquire) != 1 || !k.stats) return -1;
  unsigned long long v = 0;
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, k.stats, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (reset && hipMemset(k.stats, 0, sizeof(v)) != hipSuccess) return -1;
  return (long)v;
}

int attention_asm_prepare() {
  int ordinal = 0;
  MD_HIP(hipGetDevice(&ordinal));
  if (ordinal < 0 || ordinal >= 64) return MD_OK;  // such a device runs the HIP kernel
  AsmKernel& k = g_asm[ordinal];
  if (k.state.load(std::memory_order_acquire) != 0) return MD_OK;
  std::lock_guard<std::mutex> lock(g_asm_mu);
  if (k.state.load(std::memory_order_acquire) != 0) return MD_OK;
  // One policy for a code object that does not load: the HIP kernel is a complete replacement, so the failure is recorded
  // (state -1: every later call returns here at once), reported once on stderr and through attention_asm_state(), and is never an error
  // of model_create / md_op_attention -- round 5 failed the first call and silently succeeded on the retry.
  hipDeviceProp_t prop;
  if (hipModuleLoadData(&k.mod, md_attn577_co) != hipSuccess || hipModuleGetFunction(&k.fn, k.mod, "md_attn577_bf16") != hipSuccess ||
      hipGetDeviceProperties(&prop, ordinal) != hipSuccess || hipMalloc((void**)&k.stats, sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(k.stats, 0, sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    k.state.store(-1, std::memory_order_release);
    fprintf(stderr, "mi_depth: the embedded gfx950 attention code object did not load on device %d; 577-token bf16 attention runs the HIP kernel\n", ordinal);
    return MD_OK;
  }
  k.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  k.state.store(1, std::memory_order_release);
  return MD_OK;
}

static bool attention_asm_eligible(int n_tokens, int D, int heads, int kpad, int prec, float out_fp8_inv, const int* redo) {
  if (!redo || !g_attn_asm_ok.load(std::memory_order_acquire) || prec != MD_PREC_BF16 || n_tokens != 577 || D != heads * 64 || kpad < 640 || out_fp8_inv > 0.f) return false;
  if ((heads & (heads - 1)) != 0) return false;  // unit -> (sequence, head) is a shift and a mask
  int ordinal = 0;
  if (hipGetDevice(&ordinal) != hipSuccess || ordinal < 0 || ordinal >= 64) return false;
  return g_asm[ordinal].state.load(std::memory_order_acquire) == 1;
}

static int launch_attention_asm(const void* qk, const void* vT, void* out, int nseq, int S, int n_tokens, int heads, int D, int kpad,
                                int* redo, int redo_units, hipStream_t s) {
  int ordinal = 0;
  MD_HIP(hipGetDevice(&ordinal));
  const int nunits = nseq * heads;
  const int redo_cap = redo_units > 0 ? redo_units : nunits;  // where the compacted list sits: behind the buffer's capacity
  if (redo_cap < nunits) MD_FAIL(MD_ERR_INVALID_ARG, "attention: redo buffer of %d units for a launch of %d", redo_cap, nunits);
  int hlog = 0;
  while ((1 << hlog) < heads) ++hlog;
  const int grid = nunits < g_asm[ordinal].cus ? nunits : g_asm[ordinal].cus;
  struct Args {
    const void *qk, *vT;
    void* out;
    int* redo;
    int S, n_tokens, heads, D, kpad, heads_log2, nunits, grid;
  } args = {qk, vT, out, redo, S, n_tokens, heads, D, kpad, hlog, nunits, grid};
  static_assert(sizeof(Args) == 64, "the kernel reads this layout (gen_attn577.py)");
  size_t size = sizeof(args);
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  MD_HIP(hipModuleLaunchKernel(g_asm[ordinal].fn, (unsigned)grid, 1, 1, 256, 1, 1, 0, s, nullptr, extra));
  g_attn_asm_launches.fetch_add(1, std::memory_order_relaxed);
  attention_note_form(ATTN_FORM_ASM, grid, 4, 1);
  // the units it flagged (a row sum outside [2^-64, 2^100)) run again in the running-maximum body: compacted, then four workgroups per CU
  const int qblocks = (n_tokens + 127) / 128;
  hipLaunchKernelGGL(attention_redo_scan_kernel, dim3(1), dim3(1024), 0, s, redo, nunits, redo_cap, g_asm[ordinal].stats);
  const long items = (long)nunits * qblocks, cap = 4L * g_asm[ordinal].cus;
  hipLaunchKernelGGL(attention_redo_kernel, dim3((unsigned)(items < cap ? items : cap)), dim3(256), 0, s, (const bf16_t*)qk, (const bf16_t*)vT,
                     (bf16_t*)out, S, n_tokens, heads, D, kpad, qblocks, (const int*)(redo + redo_cap));
  MD_HIP(hipGetLastError());
  return MD_OK;
}

int launch_attention(const void* qk, const void* vT, void* out, int nseq, int S, int n_tokens, int heads, int D,
                     int kpad, int prec, hipStream_t s, float out_fp8_inv, long v_plane, int* redo, int redo_units) {
  if (prec != MD_PREC_BF16 && prec != MD_PREC_F16 && prec != MD_PREC_F16X2) MD_FAIL(MD_ERR_UNSUPPORTED, "fused attention takes bf16, f16 or split-half operands (precision %d)", prec);
  if (D != heads * 64) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: head_dim must be 64 (D=%d heads=%d)", D, heads);
  if (kpad % 64 != 0 || kpad < (n_tokens + 63) / 64 * 64)
    MD_FAIL(MD_ERR_INVALID_ARG, "attention: kpad=%d must be a multiple of 64 covering %d keys", kpad, n_tokens);
  if ((long)S * 2 * D * 2 * (prec == MD_PREC_F16X2 ? 2 : 1) >= (1L << 31)) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: one sequence of q|k rows exceeds the 2-GB descriptor range");
  const int qblocks = (n_tokens + 127) / 128;
  const long blocks = (long)qblocks * heads * nseq;
  if (nseq <= 0 || blocks > 0x7fffffffL) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: %d sequences", nseq);
  if (attention_asm_eligible(n_tokens, D, heads, kpad, prec, out_fp8_inv, redo))
    return launch_attention_asm(qk, vT, out, nseq, S, n_tokens, heads, D, kpad, redo, redo_units, s);
  const dim3 grid((unsigned)blocks), block(256);
  // small launches over long sequences: 64 queries x two key groups per workgroup (the kernel's header)
  const bool small = n_tokens >= kKeySplitMin && blocks <= kKeySplitBlocks && out_fp8_inv <= 0.f && key_split_enabled() && g_attn_small_ok != 0;
  const int qblocks_s = (n_tokens + 63) / 64;
  const dim3 grid_s((unsigned)((long)qblocks_s * heads * nseq));
  auto set_smem = [&](const void* kern, std::atomic<unsigned long>* attr_set, int smem) -> int {  // the attribute is per DEVICE: once per (kernel, device ordinal)
    int ordinal = 0;
    MD_HIP(hipGetDevice(&ordinal));
    const unsigned long bit = (ordinal >= 0 && ordinal < 64) ? 1ul << ordinal : 0ul;
    if (!bit || !(attr_set->load(std::memory_order_acquire) & bit)) {  // concurrent first launches at worst both set the attribute
      MD_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
      attr_set->fetch_or(bit, std::memory_order_release);
    }
    return MD_OK;
  };
  if (prec == MD_PREC_F16X2) {
    if (out_fp8_inv > 0.f || v_plane <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "attention: split-half operands need the V^T plane offset and write split-half rows");
    auto go = [&](auto kern, auto ks_c) -> int {
      constexpr int KS = decltype(ks_c)::value, smem = (KS == 1 ? 49152 : KS * 2 * 32768) + 16;  // one key group: the compact-K form
      static std::atomic<unsigned long> attr_set{0};
      MD_TRY(set_smem((const void*)kern, &attr_set, smem));
      const dim3 g = KS == 1 ? grid : grid_s;
      const int qb = KS == 1 ? qblocks : qblocks_s;
      hipLaunchKernelGGL(kern, g, block, smem, s, (const f16s_t*)qk, (const f16s_t*)vT, (f16s_t*)out, S, n_tokens, heads, D, kpad, qb, 0.f, v_plane);
      return MD_OK;
    };
    typedef std::integral_constant<int, 1> ks1;
    typedef std::integral_constant<int, 2> ks2;
    if (attn_pterms() == 1) {
      if (small) MD_TRY(go(attention_kernel<f16s_t, false, true, 1, 2, 2>, ks2()));
      else MD_TRY(go(attention_kernel<f16s_t, false, true, 1>, ks1()));
    } else {
      if (small) MD_TRY(go(attention_kernel<f16s_t, false, true, 2, 2, 2>, ks2()));
      else MD_TRY(go(attention_kernel<f16s_t, false, true, 2>, ks1()));
    }
  } else if (out_fp8_inv > 0.f) {
    if (prec != MD_PREC_BF16) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: e4m3 output rows are built for bf16 operands");
    hipLaunchKernelGGL((attention_kernel<bf16_t, true, true>), grid, block, 0, s, (const bf16_t*)qk, (const bf16_t*)vT, (bf16_t*)out, S,
                       n_tokens, heads, D, kpad, qblocks, out_fp8_inv, 0L);
  } else if (small) {
    constexpr int smem = 2 * 2 * 16384 + 16;
    auto go = [&](auto kern, auto tag) -> int {
      typedef decltype(tag) TT;
      static std::atomic<unsigned long> attr_set{0};
      MD_TRY(set_smem((const void*)kern, &attr_set, smem));
      hipLaunchKernelGGL(kern, grid_s, block, smem, s, (const TT*)qk, (const TT*)vT, (TT*)out, S, n_tokens, heads, D, kpad, qblocks_s, 0.f, 0L);
      return MD_OK;
    };
    if (prec == MD_PREC_F16) MD_TRY(go(attention_kernel<f16_t, false, true, 1, 2, 2>, f16_t()));
    else MD_TRY(go(attention_kernel<bf16_t, false, true, 1, 2, 2>, bf16_t()));
  } else if (prec == MD_PREC_F16) {
    hipLaunchKernelGGL((attention_kernel<f16_t, false, true>), grid, block, 0, s, (const f16_t*)qk, (const f16_t*)vT, (f16_t*)out, S,
                       n_tokens, heads, D, kpad, qblocks, out_fp8_inv, 0L);
  } else {
    hipLaunchKernelGGL((attention_kernel<bf16_t, false, true>), grid, block, 0, s, (const bf16_t*)qk, (const bf16_t*)vT, (bf16_t*)out, S,
                       n_tokens, heads, D, kpad, qblocks, out_fp8_inv, 0L);
  }
  MD_HIP(hipGetLastError());
  if (small) attention_note_form(ATTN_FORM_KEYSPLIT, grid_s.x, 2, 2);
  else attention_note_form(out_fp8_inv > 0.f ? ATTN_FORM_FP8OUT : ATTN_FORM_PLAIN, grid.x, 4, 1);
  return MD_OK;
}

// Cross-view keys: `nseq` sequences in groups of `views` consecutive ones; every query attends over the keys of its whole group
// (attention_body, MV). views = 1 is launch_attention itself.
int launch_attention_views(const void* qk, const void* vT, void* out, int nseq, int views, int S, int n_tokens, int heads, int D,
                           int kpad, int prec, hipStream_t s, long v_plane, int* redo, int redo_units) {
  if (views == 1) return launch_attention(qk, vT, out, nseq, S, n_tokens, heads, D, kpad, prec, s, 0.f, v_plane, redo, redo_units);
  if (prec != MD_PREC_BF16 && prec != MD_PREC_F16 && prec != MD_PREC_F16X2) MD_FAIL(MD_ERR_UNSUPPORTED, "cross-view attention takes bf16, f16 or split-half operands (precision %d)", prec);
  if (views < 1 || nseq <= 0 || nseq % views != 0) MD_FAIL(MD_ERR_SHAPE, "cross-view attention: %d sequences in groups of %d", nseq, views);
  if (D != heads * 64) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: head_dim must be 64 (D=%d heads=%d)", D, heads);
  if (n_tokens <= 0 || S < n_tokens) MD_FAIL(MD_ERR_SHAPE, "attention: %d tokens in sequences of %d rows", n_tokens, S);
  if (kpad % 64 != 0 || kpad < (n_tokens + 63) / 64 * 64)
    MD_FAIL(MD_ERR_INVALID_ARG, "attention: kpad=%d must be a multiple of 64 covering %d keys", kpad, n_tokens);
  const int planes = prec == MD_PREC_F16X2 ? 2 : 1;
  // one descriptor spans the q | k rows of a whole group, another its V^T tiles
  if ((long)views * S * 2 * D * 2 * planes >= (1L << 31) || (long)views * heads * 64 * kpad * 2 >= (1L << 31))
    MD_FAIL(MD_ERR_UNSUPPORTED, "cross-view attention: %d views of %d rows exceed the 2-GB descriptor range", views, S);
  const int qblocks = (n_tokens + 127) / 128;
  const long blocks = (long)qblocks * heads * nseq;
  if (blocks > 0x7fffffffL) MD_FAIL(MD_ERR_UNSUPPORTED, "attention: %d sequences", nseq);
  const dim3 grid((unsigned)blocks), block(256);
  if (prec == MD_PREC_F16X2) {
    if (v_plane <= 0) MD_FAIL(MD_ERR_INVALID_ARG, "attention: split-half operands need the V^T plane offset");
    constexpr int smem = 49152 + 16;  // the compact-K form
    auto go = [&](auto kern) -> int {
      static std::atomic<unsigned long> attr_set{0};  // the attribute is per device: once per (kernel, device ordinal)
      int ordinal = 0;
      MD_HIP(hipGetDevice(&ordinal));
      const unsigned long bit = (ordinal >= 0 && ordinal < 64) ? 1ul << ordinal : 0ul;
      if (!bit || !(attr_set.load(std::memory_order_acquire) & bit)) {
        MD_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set.fetch_or(bit, std::memory_order_release);
      }
      hipLaunchKernelGGL(kern, grid, block, smem, s, (const f16s_t*)qk, (const f16s_t*)vT, (f16s_t*)out, S, n_tokens, heads, D, kpad, qblocks, v_plane, views);
      return MD_OK;
    };
    if (attn_pterms() == 1) MD_TRY(go(attention_views_kernel<f16s_t, 1>));
    else MD_TRY(go(attention_views_kernel<f16s_t, 2>));
  } else if (prec == MD_PREC_F16) {
    hipLaunchKernelGGL((attention_views_kernel<f16_t>), grid, block, 0, s, (const f16_t*)qk, (const f16_t*)vT, (f16_t*)out, S, n_tokens, heads, D,
                       kpad, qblocks, 0L, views);
  } else {
    hipLaunchKernelGGL((attention_views_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)qk, (const bf16_t*)vT, (bf16_t*)out, S, n_tokens, heads, D,
                       kpad, qblocks, 0L, views);
  }
  MD_HIP(hipGetLastError());
  attention_note_form(ATTN_FORM_VIEWS, grid.x, 4, 1);
  return MD_OK;
}

}  // namespace md
