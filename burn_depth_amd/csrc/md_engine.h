// Depth Pro engine: device-resident weights, static workspace plan, forward schedule.
#pragma once

#include <atomic>
#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "kernels/gemm.h"
#include "kernels/ops.h"
#include "md_common.h"
#include "md_weights.h"

struct md_device_s {
  int ordinal = 0;
  hipStream_t stream = nullptr;
};

namespace md {

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  void* take(size_t bytes) {
    size_t o = align_up(off, 256);
    if (o + bytes > cap) return nullptr;
    off = o + bytes;
    return base + o;
  }
};

// split geometry (encoder.rs:196-206) and feature padding (encoder.rs:28-38)
void split_geometry(int image_size, int patch_size, float overlap, int* stride, int* steps);
int feature_padding(int patch_size, int stride, int feature_patch_size);
// merged-map pixel -> (tile j, tile i, ty, tx) (encoder.rs:234-282 inverted)
void merge_source(int Y, int X, int h, int w, int steps, int pad, int* j, int* i, int* ty, int* tx);
int merged_extent(int h, int steps, int pad);
// The gather tables of the encoder tail, pure host functions. merge_index_table: the [B, E, E] merged map (E = merged_extent(g, steps,
// pad)) of g x g token grids in sequences of SS rows (row 0: cls), tile (j, i) of image b being sequence seq0 + (j steps + i) B + b:
// entry = (seq0 + (j steps + i) B + b) SS + 1 + ty g + tx. token_index_table: the P patch rows of sequences seq0 .. seq0 + B - 1,
// entry b P + p = (seq0 + b) SS + 1 + p.
void merge_index_table(int B, int g, int steps, int pad, int SS, int seq0, int32_t* out);
void token_index_table(int B, int P, int SS, int seq0, int32_t* out);

// PACK_HEAD_W / PACK_HEAD_B: the depth head's `deconv k2s2 (+bias) -> conv 3x3` pair (mod.rs:105-108, nothing between
// them) composed at commit into ONE 3x3 convolution on the deconv's input grid with 4 x Cout output columns (one group
// per output parity) and its nine position-class bias vectors (compose_head_kernel in md_engine.hip).
// PACK_C1C3_W / PACK_C1C3_B: a biased 1x1 convolution followed by a 3x3 convolution (the decoder's last `out_conv` and the
// head's `conv0`, decoder.rs:137 -> mod.rs:105: nothing between them) composed into one 3x3 convolution and its nine
// position-class bias vectors (compose_c1c3_kernel; the border classes are applied by launch_border_bias_fix).
enum PackKind : int { PACK_NK = 0, PACK_CONV3 = 1, PACK_DECONV = 2, PACK_DIRECT = 3, PACK_HEAD_W = 4, PACK_HEAD_B = 5, PACK_C1C3_W = 6, PACK_C1C3_B = 7 };

struct PackEntry {
  int param = -1;   // index into params (PACK_HEAD_*: the deconv weight [Cin,Cmid,2,2]; PACK_C1C3_*: the 1x1 weight [Cmid,Cin])
  int param2 = -1;  // PACK_DECONV only: 1x1 conv weight [Cout,Cout] composed behind the deconv at commit; PACK_HEAD_*: conv weight [Cout,Cmid,3,3]
  int param3 = -1, param4 = -1;  // PACK_HEAD_B / C1C3_B: bias of the first layer [Cmid], bias of the second [Cout]; PACK_DECONV pair (k == 4): param3 = Cmid
  int kind = PACK_NK;
  int d0 = 0, d1 = 0, k = 1;  // NK: N, K | CONV3: Cout, Cin | DECONV: Cin, Cout | DIRECT: Cout, Cin, k | HEAD_W/B, C1C3_W/B: Cout, Cin (k = Cmid)
  int kp = 0;       // padded contraction length per tap (elements)
  int terms = 1;    // MD_PREC_F16X2: copies of the contraction per row -- 2 = [W | W] (f16-exact weight), 3 = [Wh | Wh | Wl]; set at commit
  int f32 = 0;      // packed as f32 regardless of precision (direct conv)
  void* dst = nullptr;
  size_t bytes = 0;
};

// One DINOv2 block's tables, bound at create (vit_bind; md_engine_util.h). The four linear layers are indexed qkv | proj | fc1 | fc2.
struct VitBlockW {
  const float *n1g, *n1b, *n2g, *n2b, *qkv_b, *proj_b, *ls1, *fc1_b, *fc2_b, *ls2;
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;
  const float* w32[4] = {nullptr, nullptr, nullptr, nullptr};  // fp32 masters of the linear weights (commit: fold vectors, fp8 pack)
  // LayerNorm fold (gemm.h GemmParams::ln_*; null when the model cannot fold): c / d of norm1 -> qkv [3D] and of norm2 -> fc1 [4D]
  const float *qkv_c = nullptr, *qkv_d = nullptr, *fc1_c = nullptr, *fc1_d = nullptr;
  // per-head q / k LayerNorm + 2-D RoPE behind the qkv GEMM (Depth-Anything-v3's extended blocks; null when absent): q, k
  const float *qkn_g[2] = {nullptr, nullptr}, *qkn_b[2] = {nullptr, nullptr};
  // MD_PREC_FP8: e4m3 copies of the linear weights and their per-output-channel scales (null otherwise)
  void* w8[4] = {nullptr, nullptr, nullptr, nullptr};
  float* s8[4] = {nullptr, nullptr, nullptr, nullptr};
  // a global block of the extended backbone: its proj GEMM keeps the input stream for the hook (GemmParams::resid_src) and
  // writes the other residual buffer
  bool global = false;
};
struct VitW {
  const void* pe_w;
  const float *pe_b, *cls, *pos, *norm_g, *norm_b;
  std::vector<VitBlockW> blk;
};
// Every weight behind the ViT is bound at create too (dp_bind in md_engine.hip, da3_bind in md_da3.hip): a packed convolution /
// linear weight and its fp32 bias (null: none), and the residual unit of both heads (ResidualBlock, ResidualConvUnit)
struct ConvW { const void* w = nullptr; const float* b = nullptr; };
struct ResUnitW { ConvW c1, c2; };
struct DepthProW {
  // encoder tail: projection and first deconvolution of upsample_latent0 | upsample_latent1 (its composed 0x1 pair) | upsample0 |
  // upsample1 | upsample2, latent0's composed 1x2 pair, upsample_lowres, fuse_lowres
  const void *enc_proj[5] = {}, *enc_up[5] = {}, *latent0_1x2 = nullptr;
  ConvW lowres, fuse;
  // decoder: convs[1..4], fusions[l].resnet1 | resnet2, fusions[l]'s out_conv (l > 0: the composed deconv_out_conv)
  const void* convs[5] = {};
  ResUnitW res[5][2];
  ConvW out[5];
  // head (outconv_conv0.b, deconv_conv1.b: the nine bias classes; outconv_conv0 and conv1 are optional forms)
  ConvW conv0, outconv_conv0, deconv, deconv_conv1, conv1, conv_out;
  // FOV: the stride-2 downsample (direct form; down_gemm: its implicit-GEMM operand, optional), encoder_proj, head_blocks
  ConvW down, fov_proj, head[4];
  const void* down_gemm = nullptr;
};

struct Tap {
  float* dev = nullptr;
  int64_t dims[4] = {0, 0, 0, 0};
  size_t count = 0;
};

struct TimingEntry {
  std::string name;
  hipEvent_t a, b;
};

// The captured hipGraphs of one model, keyed by stream, shapes and every in / out pointer of a call. No captured graph may outlive
// a device address it baked in: whatever frees or moves such an address (a staging growth, a workspace re-plan) clears the cache.
struct GraphCache {
  GraphCache() = default;
  GraphCache(const GraphCache&) = delete;
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() { clear(); }
  void clear() {
    for (auto& kv : entries)
      if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    entries.clear();
  }
  // `root_gen`: the root's commit_gen. Entries captured under an older generation can never be replayed again (the root clears
  // its own cache in model_commit; a fork's cannot be reached from there)
  void track_generation(unsigned root_gen) {
    if (gen == root_gen) return;
    clear();
    gen = root_gen;
  }
  // Runs `body` (the launch schedule of one call) eagerly the first time `key` is seen -- that call allocates index tables and
  // sets function attributes --, captures it into a hipGraph the second time and replays the instantiated graph from then on.
  template <typename F>
  int run(hipStream_t st, const std::vector<uintptr_t>& key, F&& body) {
    {
      Entry& e = entries[key];  // not held across body(): a body that grows a buffer clears the cache (this entry included)
      if (e.exec) {
        MD_HIP(hipGraphLaunch(e.exec, st));
        return MD_OK;
      }
      if (e.seen++ == 0) return body();
    }
    MD_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    const int s = body();
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(st, &g);
    if (s != MD_OK || ce != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      entries.erase(key);
      if (s != MD_OK) return s;
      MD_FAIL(MD_ERR_HIP, "stream capture failed: %s", hipGetErrorString(ce));
    }
    hipGraphExec_t ex = nullptr;
    const hipError_t ie = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess || !ex) {
      entries.erase(key);
      MD_FAIL(MD_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie));
    }
    entries[key].exec = ex;
    MD_HIP(hipGraphLaunch(ex, st));
    return MD_OK;
  }

 private:
  struct Entry {
    int seen = 0;
    hipGraphExec_t exec = nullptr;
  };
  std::map<std::vector<uintptr_t>, Entry> entries;
  unsigned gen = 0;  // the root's commit_gen the entries were captured under
};

// A model-owned grow-only buffer of device memory (or of pinned host memory: the bounce buffers between pageable caller memory and
// the DMA engine). grow() below is its one way to (re)allocate; the owner's destructor frees it.
template <typename T, bool Pinned = false>
struct GrowBuf {
  T* p = nullptr;
  size_t cap = 0;  // bytes
  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { release(); }
  void release() {
    if (p) (void)(Pinned ? hipHostFree((void*)p) : hipFree((void*)p));
    p = nullptr;
    cap = 0;
  }
};
using PinnedBuf = GrowBuf<void, true>;

}  // namespace md

struct md_model_s {
  md_device_t dev = nullptr;
  md::ModelCfg cfg;
  int prec = MD_PREC_BF16;
  int esz = 2;  // bytes per operand element
  int ke = 64;  // contraction elements per 128-byte LDS row
  int xm = 1;   // planes per activation element: 2 in MD_PREC_F16X2 (rows are [hi | lo])
  int wterms = 1;  // MD_PREC_F16X2: MFMA terms of a product with a plain (not composed) weight -- 2 when every such weight is
                   // f16-exact (an f16 checkpoint, mod.rs:206), else 3; decided by model_commit. 1 in the one-plane modes
  size_t vt_plane = 0;  // MD_PREC_F16X2: elements from the hi to the lo plane of V^T

  // ---- parameters ----
  std::vector<md::ParamSpec> params;
  std::unordered_map<std::string, int> pindex;
  std::vector<float*> w32;  // fp32 master copy on device, one per param
  char* w32_base = nullptr;
  size_t w32_bytes = 0;
  std::vector<md::PackEntry> packs;
  std::unordered_map<std::string, int> pack_index;
  char* wpk_base = nullptr;
  size_t wpk_bytes = 0;
  bool committed = false;
  unsigned commit_gen = 0;  // bumped by every model_commit (part of the graph-replay key)
  int ngroups = 2;
  md::VitW vit[3];
  md::DepthProW dp;
  float head_b_host = 0.f;

  // ---- workspace ----
  md::Arena ws;
  struct Buffers;
  Buffers* buf = nullptr;
  void* zero_page = nullptr;
  long alloc_count = 0;  // device / pinned-host allocations made by infer calls (staging growth, index tables): md_model_query("allocs")
  std::map<int, int*> index_tables;  // per batch size B: device int32 blob
  struct IndexSet {
    int *hi = nullptr, *mid = nullptr, *x2 = nullptr, *img = nullptr, *fov = nullptr;
  };
  std::map<int, IndexSet> index_sets;

  // ---- debug ----
  bool taps_enabled = false;
  std::map<std::string, md::Tap> taps;
  bool timing_enabled = false;
  std::string timing_filter;  // non-empty: only launches of this family are timed
  std::vector<md::TimingEntry> timing;
  std::vector<std::string> timing_names_out;

  // ---- hipGraph replay of the launch schedule (md_model_enable_graph) ----
  bool graph_enabled = false;
  // md_model_set_option("batch_invariant"): no launch-size-dependent kernel form (k-split GEMM, small-launch attention): an image's result
  // has the same bits alone and inside a batch, like the reference's `infer` (a pure batch map, encoder.rs:216-225)
  bool batch_invariant = false;
  // md_model_set_option("ln_fold"): the LayerNorms between the ViT's GEMMs folded into those GEMMs (run_vit_block; gemm.h GemmParams::ln_*).
  // 1 = automatic (on for 16-bit Depth Pro models of width % 256 == 0 whose sequences have >= 256 tokens: the launches that run the
  // 256 x 256 tiles anyway), 0 = off, 2 = on whenever the model can (small presets too: the four GEMMs of a block then keep to the
  // 256 x 256 kernel). A MODEL-level choice, never a per-launch one: a window of a call computes the same bits as the whole call.
  int ln_fold_opt = 1;
  bool ln_fold_can = false;    // 16-bit Depth Pro, D % 256 == 0: the workspace and the fold vectors exist
  float* lnfold_base = nullptr;  // root: the c / d vectors of every block (VitBlockW points into it)
  bool ln_fold_on() const { return ln_fold_can && (ln_fold_opt == 2 || ln_fold_opt == 4 || (ln_fold_opt == 1 && NT >= 256)); }  // (3, 4: bench diagnostics, run_vit)
  md::GraphCache graphs;

  // ---- md_model_fork: a fork shares the parameter / packed-weight arenas of its root model (never frees them) and
  //      owns its workspace, index tables, taps, timing, graphs and default stream ----
  md_model_s* parent = nullptr;   // root model of a fork (forks of forks attach to the root)
  std::atomic<int> forks{0};      // live forks of this root (model_fork / model_destroy may run on different threads)
  hipStream_t own_stream = nullptr;  // a fork's default stream (stream == NULL in infer)

  // ---- model kind: 0 = Depth Pro, 1 = Depth-Anything-v3 (state in md_da3.hip) ----
  int kind = 0;
  struct Da3State;
  Da3State* da3 = nullptr;
  // ---- md_process_frame: tap tables, staging and scratch of the frame path (md_frame.hip); per model, so per fork ----
  struct FrameState;
  FrameState* frame = nullptr;
  // ---- md_infer_points: device homes and scratch of the point path (md_points.hip); per model, so per fork ----
  struct PointsState;
  PointsState* points = nullptr;
  // geometry shared by create/infer
  int S = 0, win = 0, g = 0, P = 0, NT = 0, SS = 0, kpad = 0;
  int steps0 = 0, stride0 = 0, steps1 = 0, stride1 = 0, pad_hi = 0, pad_mid = 0;
  int mh_hi = 0, mh_mid = 0;  // merged extents
};

namespace md {

int model_create(md_device_t dev, const ModelCfg& cfg, md_model_t* out);
int model_init_seeded(md_model_t m, uint64_t seed, int scheme);
int model_load_container(md_model_t m, const char* path);
int model_commit(md_model_t m);
int model_round_weights_f16(md_model_t m);
int model_destroy(md_model_t m);
int model_fork(md_model_t src, md_model_t* out);
inline md_model_s* model_root(md_model_s* m) { return m->parent ? m->parent : m; }
// the stream of a call: the caller's, else the model's default (a fork's own stream, else the device's)
inline hipStream_t model_stream(const md_model_s* m, hipStream_t stream) { return stream ? stream : (m->own_stream ? m->own_stream : m->dev->stream); }
// Grow-only staging: makes `b` hold at least `bytes`, and allocates only when it does not. hipFree is a device-wide synchronisation
// and hipMalloc takes the allocator lock, so a steady stream of same-sized calls must not pay either. A growth first waits for `st`
// (nothing may still read the buffer being replaced) and clears the model's captured graphs (they bake the old address); it never
// happens inside a capture, since the eager first call of a replay key has grown every buffer the key needs. It counts in
// md_model_query("allocs"). *grown (if given) tells whether it reallocated.
template <typename T, bool Pinned>
int grow(md_model_s* m, hipStream_t st, GrowBuf<T, Pinned>& b, size_t bytes, bool* grown = nullptr) {
  if (grown) *grown = false;
  if (b.cap >= bytes) return MD_OK;
  MD_HIP(hipStreamSynchronize(st));
  m->graphs.clear();
  b.release();
  void* p = nullptr;
  const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
  if (e != hipSuccess) MD_FAIL(MD_ERR_OOM, "%s(%zu) of a staging buffer failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
  b.p = (T*)p;
  b.cap = bytes;
  m->alloc_count += 1;
  if (grown) *grown = true;
  return MD_OK;
}
// f_px non-null: the caller's focal lengths [B] (memory kind f_kind) replace the FOV network's (md_depth_pro_infer_with_focal)
int model_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, float* focal,
                float* fovx, float* fovy, int out_kind, hipStream_t stream, const uint8_t* rgb, size_t rgb_len,
                const float* f_px = nullptr, int f_kind = 0);
// DepthPro::decoder_from_features / head_debug (depth_pro/mod.rs:262-307): the decoder / the depth head alone on caller tensors
int model_decoder_from_features(md_model_t m, const md_nchw_view* features, int levels, int B, int in_kind, float* out_features,
                                float* out_lowres, float* const* out_fusions, int out_kind, hipStream_t stream);
int model_head_debug(md_model_t m, const md_nchw_view* feature, int B, int in_kind, const md_head_debug* out, int out_kind,
                     hipStream_t stream);
// "decoder_levels" / "decoder_features" / "decoder_level{l}_channels" / "decoder_level{l}_size" of md_model_query; false = not such a key
bool model_decoder_query(md_model_t m, const std::string& key, int64_t* out);
// Tile-parallel mode (SURVEY 8(e) "optional second mode": the 35 + 2 ViT sequences of one image never interact before
// `merge`, layers/encoder.rs:329-348, 379-390): the ViT stage of ONE call is split into `parts` windows of the sequence
// range; a rank runs its window, every other part's final tokens and hook rows travel to the root, the root runs the rest.
struct ShardSegment {
  void* ptr;
  size_t bytes;
};
struct ShardPlan {
  int parts = 1;
  int part = 0;  // this rank's window; -1 = every window one after the other on this device (diagnostic / single-GPU test)
  int root = 0;  // the part whose rank runs encoder tail, decoder, head and FOV and owns the outputs
  // called once behind this rank's window, on the engine's stream: seg[p] = {final tokens, hook 0, hook 1} rows of part p
  int (*exchange)(void* ctx, int parts, const ShardSegment (*seg)[3], hipStream_t st) = nullptr;
  void* ctx = nullptr;
  float* window_ms = nullptr;  // part == -1: GPU milliseconds of each window [parts] ...
  float* tail_ms = nullptr;    // ... and of everything behind the ViT stage
};
int model_infer_sharded(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, float* focal,
                        float* fovx, float* fovy, int out_kind, hipStream_t stream, const ShardPlan& sp);
// the model's grow-only input staging buffer, holding `elems` floats: filled from `nchw` (host or device) when it is given
int model_stage_input(md_model_t m, const float* nchw, size_t elems, int in_kind, hipStream_t stream, float** dev);
// md_process_frame's pieces: model_infer / da3_infer_ex without the graph layer (the frame call captures its own graph around
// them), the grow-only pinned staging of a host u8 frame (`bytes` of `rgb` -> the model's device copy *dev), and the frame
// path's state (md_frame.hip)
// (f_px_dev: the caller's focal lengths [B] on the device = md_depth_pro_infer_with_focal's body)
int model_infer_direct(md_model_t m, const float* nchw, int B, int H, int W, float* depth, float* focal, float* fovy, hipStream_t stream,
                       const float* f_px_dev = nullptr);
int model_stage_rgb(md_model_t m, const uint8_t* rgb, size_t bytes, hipStream_t stream, const uint8_t** dev);
void frame_destroy_state(md_model_t m);
int frame_geometry(md_model_t m, int w, int h, const md_frame_opts* o, int* th, int* tw, int* oh, int* ow);
int process_frame(md_model_t m, const uint8_t* rgb, int B, int w, int h, int in_kind, const md_frame_opts* o, const md_frame_outputs* out,
                  int out_kind, hipStream_t stream);
// crop (cx, cy, cw, ch) of a [B,h,w] map, restored to ow x oh (no restore at the crop's own size)
DisplayGeom display_geom(int B, int h, int w, int cx, int cy, int cw, int ch, int ow, int oh);
// the point path (md_points.hip): the stand-alone operators on caller tensors, the model -> points call and its state
struct DepthMaps {  // an operator's input maps on the device: depth [B,H,W], conf [B,H,W] or null, u8 rgb [B,H,W,3] or null
  const float* depth = nullptr;
  const float* conf = nullptr;
  const uint8_t* rgb = nullptr;
  int B = 0, H = 0, W = 0;
};
struct PointList {  // md_op_voxel_thin's input rows on the device: xyz [N,3], conf [N] / u8 rgb [N,3] / normals [N,3] or null
  const float* xyz = nullptr;
  const float* conf = nullptr;
  const uint8_t* rgb = nullptr;
  const float* normals = nullptr;
  int64_t N = 0;
};
// One md_infer_points* request: what the widest entry (md_infer_points_register_plane) takes. A narrower entry leaves the parts it lacks
// null, and a null part is the call without it (nrm all zero and voxel == 0 likewise).
struct PointsCall {
  const float* nchw = nullptr;  // the image [B,3,H,W], of in_kind
  int B = 0, H = 0, W = 0;
  int in_kind = MD_MEM_DEVICE;
  const uint8_t* rgb = nullptr;  // of in_kind
  const md_points_cameras* cam = nullptr;
  const md_points_opts* o = nullptr;
  const md_points_outputs* out = nullptr;  // pointers of out_kind, as are nrm's and vox's
  int out_kind = MD_MEM_DEVICE;
  const md_view_filter_opts* fo = nullptr;  // given: the view filter runs between the model and the unprojection
  const md_points_normals* nrm = nullptr;
  const md_points_voxel* vox = nullptr;
  bool need_filter = false;  // the md_infer_points_filtered entry: a null `fo` is refused
  const md_points_render* rnd = nullptr;  // given: the list the call ends with is rendered into its targets (cameras of in_kind)
  const md_points_mesh* mesh = nullptr;   // given: the faces of the depth grid over the list's rows (pointers of out_kind)
  const md_points_raster* rst = nullptr;  // given: those faces are rasterised into its targets (cameras of in_kind)
  const md_points_outlier* outl = nullptr;  // given: radius outlier removal between the unprojection and the thinning (pointers of out_kind)
  const md_points_decimate* dec = nullptr;  // given: vertex-clustering decimation behind the mesh (pointers of out_kind); needs `mesh`
  const md_points_components* comp = nullptr;  // given: island removal behind the mesh, face-only (pointers of out_kind); needs `mesh`
  const md_points_smooth* smooth = nullptr;    // given: smoothing of the list over the faces the rasteriser reads (pointers of out_kind); needs `mesh`
  const md_points_planes* pln = nullptr;       // given: plane extraction from the list the call ends with (pointers of out_kind); mode 1 / 2 writes that list
  const md_points_clusters* clu = nullptr;     // given: clustering of the list behind the plane stage (pointers of out_kind); mode 1 writes that list
  const md_points_match* mat = nullptr;        // given: matching against a reference cloud between the plane stage and the clustering (pointers of out_kind, the target of its own kind); mode 1 / 2 writes the list
  const md_points_register* reg = nullptr;     // given: rigid registration onto a reference cloud directly in front of the matching, on the list it reads; apply moves that list in place
  const md_points_register_plane* rpl = nullptr;  // given with target_normals: `reg` runs in the point-to-plane form (normals of reg's target_kind, sum_r2 of out_kind)
};
// nrm (md_op_unproject_normals): null or all zero = md_op_unproject
int op_unproject(md_device_t dev, const DepthMaps& in, const md_points_cameras* cam, const md_points_opts* o, const md_points_outputs* out,
                 const md_points_normals* nrm, hipStream_t stream, const md_points_mesh* mesh = nullptr);
// the face kernels alone: in.depth and pixel_index [B,H,W] on the device
int op_mesh_grid(md_device_t dev, const DepthMaps& in, const int32_t* pixel_index, int stride, int64_t vertex_limit, const md_points_mesh* mesh,
                 hipStream_t stream);
int infer_points(md_model_t m, const PointsCall& call, hipStream_t stream);
int op_voxel_thin(md_device_t dev, const PointList& in, const md_points_voxel* vox, const md_points_outputs* out, float* normals_out,
                  hipStream_t stream);
int op_radius_outliers(md_device_t dev, const PointList& in, const md_points_outlier* outl, const md_points_outputs* out, float* normals_out,
                       hipStream_t stream);
// in: the vertices; faces [F,3] over their rows
int op_decimate_mesh(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const md_points_decimate* dec,
                     const md_points_outputs* out, float* normals_out, hipStream_t stream);
// in: the vertices (in.N bounds the corners; the rows themselves only with comp->compact); faces [F,3] over their rows
int op_mesh_components(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const md_points_components* comp,
                       const md_points_outputs* out, float* normals_out, hipStream_t stream);
// xyz [N,3] and faces [F,3] over its rows; rows >= capacity of smooth's outputs are not written
int op_smooth_mesh(md_device_t dev, const float* xyz, int64_t N, const int32_t* faces, int64_t F, const md_points_smooth* smooth, int64_t capacity,
                   hipStream_t stream);
// in: the rows, one view; out's list fields and normals_out with pln->mode 1 / 2 only
int op_fit_planes(md_device_t dev, const PointList& in, const md_points_planes* pln, const md_points_outputs* out, float* normals_out,
                  hipStream_t stream);
// in: the rows, one view; out's list fields and normals_out with clu->mode 1 only
int op_cluster_points(md_device_t dev, const PointList& in, const md_points_clusters* clu, const md_points_outputs* out, float* normals_out,
                      hipStream_t stream);
// in: the rows, one view; out's list fields and normals_out with mat->mode 1 / 2 only
int op_match_points(md_device_t dev, const PointList& in, const md_points_match* mat, const md_points_outputs* out, float* normals_out,
                    hipStream_t stream);
// xyz [N,3] (+ normals): the rows, one view; xyz_out (may be xyz) / normals_out [N,3] or null
// plane with target_normals: the point-to-plane form (md_op_register_points_plane)
int op_register_points(md_device_t dev, const float* xyz, const float* normals, int64_t N, const md_points_register* reg, float* xyz_out,
                       float* normals_out, hipStream_t stream, const md_points_register_plane* plane = nullptr);
// in.xyz / in.rgb: the list; count: its device count word or null
int op_render_points(md_device_t dev, const PointList& in, const int32_t* count, int T, int H, int W, const md_points_cameras* cam,
                     const md_render_opts* o, const md_render_outputs* out, hipStream_t stream);
// in.xyz / in.rgb: the vertices; faces [F,3] over their rows; face_count: the device face-count word or null
int op_render_mesh(md_device_t dev, const PointList& in, const int32_t* faces, int64_t F, const int32_t* face_count, int T, int H, int W,
                   const md_points_cameras* cam, const md_raster_opts* o, const md_raster_outputs* out, hipStream_t stream);
// the probe-loop flag of the model's last md_infer_points_voxel (waits for its stream); 0 when it never ran
int points_voxel_overflow(md_model_t m, int64_t* out);
// likewise for the outlier removal of the model's last md_infer_points_outlier
int points_outlier_overflow(md_model_t m, int64_t* out);
int points_clusters_overflow(md_model_t m, int64_t* out);
int points_match_overflow(md_model_t m, int64_t* out);
int points_register_overflow(md_model_t m, int64_t* out);
// likewise for the decimation of the model's last md_infer_points_decimate (the vertex table's flag or the face table's)
int points_decimate_overflow(md_model_t m, int64_t* out);
int op_filter_views(md_device_t dev, const DepthMaps& in, const md_points_cameras* cam, const md_view_filter_opts* o,
                    const md_view_filter_outputs* out, hipStream_t stream);
void points_destroy_state(md_model_t m);
int pack_weight(const float* src, const PackEntry& e, int prec, hipStream_t s);
// PACK_HEAD_W / PACK_HEAD_B as model_commit composes them: `out` fp32 [4 * cout][cin][3][3] (pack_weight's PACK_CONV3 source) and
// fp32 [9][cout]
int compose_head(const float* wd, const float* w1, int cin, int cmid, int cout, float* out, hipStream_t s);
int compose_head_bias(const float* w1, const float* bd, const float* b1, int cmid, int cout, float* out, hipStream_t s);
// The other compositions of model_commit (md_op_compose_weights launches them alone): deconv k2s2 [cin, cmid, 2, 2] -> conv 1x1 [cout, cmid]
// as `out` [cin, cout, 2, 2]; two bias-free deconvolutions k2s2 [cin, cmid, 2, 2], [cmid, cout, 2, 2] as `out` [cin, cout, 4, 4]; conv 1x1
// [cmid, cin] -> conv 3x3 [cout, cmid, 3, 3] as `out` [cout, cin, 3, 3] (its bias classes: compose_head_bias(w3, b of the 1x1, b of the 3x3))
int compose_deconv_conv(const float* wd, const float* wo, int cin, int cmid, int cout, float* out, hipStream_t s);
int compose_deconv_pair(const float* wa, const float* wb, int cin, int cmid, int cout, float* out, hipStream_t s);
int compose_c1c3(const float* w1, const float* w3, int cin, int cmid, int cout, float* out, hipStream_t s);
// number of values of w[0..n) that are not exactly representable as an IEEE half (synchronises the stream)
int count_inexact_f16(const float* w, long n, hipStream_t s, unsigned* out);
void fov_scalar_host(float fovx_deg, int H, int W, float* focal_px, float* fovy_rad);
// the known-focal tail on host scalars: f_px -> fovx_deg, fovy_rad (what focal_post computes on the device)
void focal_scalar_host(float f_px, int H, int W, float* fovx_deg, float* fovy_rad);

// ---- Depth-Anything-v3 (md_da3.hip) ----
struct Da3Cfg {
  std::string variant = "metric_large";
  ViTDims vit;
  int image_size = 518, image_width = 0, features = 256, output_dim = 1;  // image_size = rows; image_width 0 = square
  int out_channels[4] = {256, 512, 1024, 1024};
  int hook_ids[4] = {4, 11, 17, 23};
  int precision = MD_PREC_BF16, max_batch = 1;
  float ln_eps = 1e-6f;
  // `small`: dual head + camera decoder + burn_dino backbone extras from block `ext_block_start` on
  bool dual_head = false;
  int ext_block_start = -1, aux_levels = 4, aux_out1_conv_num = 5, aux_output_dim = 7;
  float rope_frequency = 100.f, qk_norm_eps = 1e-5f;
  // `CameraEncoderConfig` (camera.rs:12-37; mod.rs:164-168): only runs under `infer_with_camera`
  bool camera_encoder = false;
  int cam_heads = 16, cam_trunk_depth = 4;
  float cam_ln_eps = 1e-5f;
};
std::vector<ParamSpec> da3_param_specs(const Da3Cfg& cfg, int scheme);
int da3_create(md_device_t dev, const Da3Cfg& cfg, md_model_t* out);
const Da3Cfg& da3_cfg(md_model_t m);
int da3_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, int out_kind,
              hipStream_t stream);
// DepthAnything3Inference (mod.rs:231-239); null = not wanted. aux is [B, aux_output_dim-1, 8ph, 8pw].
struct Da3Outputs {
  float *depth = nullptr, *depth_confidence = nullptr, *aux = nullptr, *aux_confidence = nullptr;
  float *pose_encoding = nullptr, *extrinsics = nullptr, *intrinsics = nullptr;
  // `infer_with_camera` (mod.rs:301-309): known world-to-camera extrinsics [B, views, 3, 4] and intrinsics [B, views, 3, 3], in the
  // memory kind of the input image. Both set + a model with a camera encoder => the encoded token conditions the backbone.
  const float *cam_extrinsics = nullptr, *cam_intrinsics = nullptr;
  int cam_views = 0;
  // multi-view inference (md_da3_infer_views): the B images are B / views scenes of `views` views each, scene-major; the global blocks
  // attend across the views of a scene and views 1.. take the source-view camera token. 1 = every image a scene of its own.
  int views = 1;
  // `infer_from_tokens` (mod.rs:389-469): the head alone on caller-supplied hook tokens. tokens[i] = [B, tokens_per_image, din] fp32
  // in the memory kind `in_kind`; tokens_per_image = P (patch rows only) or P + 1 (a leading cls row is skipped, `patch_token_start`)
  const float* tokens[4] = {nullptr, nullptr, nullptr, nullptr};
  int tokens_per_image = 0;
  // `infer_raw` (mod.rs:364-380): [B, output_dim, H, W] -- the dual head's main logits before the activations, the mono head's
  // `forward_raw` result. When set, `depth` may be NULL and nothing else is produced.
  float* raw_logits = nullptr;
};
int da3_infer_ex(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const Da3Outputs& out, int out_kind,
                 hipStream_t stream);
void da3_destroy_state(md_model_t m);
long da3_shape_builds(md_model_t m);
// The 2-D RoPE tables of a ph x pw patch grid: [max(ph, pw) + 2][16] cos and sin of angle(pos, f) = pos * base^(-2f/32), the angle
// formed in fp32 like the oracle. One function for the model (md_da3.hip) and the stand-alone operators (md_api.cpp).
void da3_rope_tables(int ph, int pw, float base, std::vector<float>* cos_out, std::vector<float>* sin_out);
int da3_infer_direct(md_model_t m, const float* nchw, int B, int H, int W, float* depth, hipStream_t stream);  // device in / out
// da3_infer_ex without the graph layer, device in / out (md_infer_points captures its own graph around it)
int da3_infer_ex_direct(md_model_t m, const float* nchw, int B, int H, int W, const Da3Outputs& out, hipStream_t stream);
// patch size and the current input size (rows, columns; 0 before the first plan) of a Depth-Anything-v3 model
void da3_frame_info(md_model_t m, int* patch, int* cur_h, int* cur_w);  // input sizes whose tables were built so far (0 for Depth Pro models)
int da3_on_commit(md_model_t m);  // re-derives the (interpolated) position table from the weights
int model_load_params_from_container(md_model_t m, const char* path);

}  // namespace md
