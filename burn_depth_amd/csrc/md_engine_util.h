// Helpers shared by the model engines (Depth Pro: md_engine.hip, Depth-Anything-v3: md_da3.hip).
#pragma once

#include <algorithm>
#include <string>

#include "md_engine.h"

namespace md {

inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// elements of a packed weight; `terms` copies of the contraction per row (MD_PREC_F16X2: 2 or 3, PackEntry::terms)
inline size_t pack_elems(const PackEntry& e, int terms = 1) {
  const size_t kpt = (size_t)e.kp * terms;
  switch (e.kind) {
    case PACK_NK: return (size_t)e.d0 * kpt;
    case PACK_CONV3: return (size_t)e.d0 * 9 * kpt;
    case PACK_DECONV: return (size_t)e.k * e.k * e.d1 * kpt;
    case PACK_HEAD_W: return (size_t)4 * e.d0 * 9 * kpt;
    case PACK_HEAD_B: return (size_t)9 * e.d0;
    case PACK_C1C3_W: return (size_t)e.d0 * 9 * kpt;
    case PACK_C1C3_B: return (size_t)9 * e.d0;
    default: return (size_t)e.d0 * e.d1 * e.k * e.k;
  }
}
// allocation size of a pack: split-half models reserve three terms (the form is only known once the weights are committed)
inline size_t pack_bytes(const md_model_s* m, const PackEntry& e) {
  if (e.f32) return pack_elems(e) * 4;
  return pack_elems(e, m->xm == 2 ? 3 : 1) * (m->prec == MD_PREC_F32 ? 4 : 2);
}

inline const float* P32(md_model_s* m, const std::string& name) {
  auto it = m->pindex.find(name);
  return it == m->pindex.end() ? nullptr : m->w32[it->second];
}
inline const void* PK(md_model_s* m, const std::string& name) {
  auto it = m->pack_index.find(name);
  return it == m->pack_index.end() ? nullptr : m->packs[it->second].dst;
}

// ---- create scaffold shared by both models (md_engine.hip) ----
// the zeroed fp32 master arena of `specs`: params, pindex, w32
int alloc_param_arena(md_model_s* m, std::vector<ParamSpec> specs);
// places every pack added so far in one zeroed arena (PackEntry::dst)
int place_packs(md_model_s* m);

// Fills the weight tables at create, once the packed arena is placed. A required name that is not there fails the create with
// MD_ERR_FORMAT (status()); an optional one leaves its field null.
struct Binder {
  md_model_s* m;
  std::string missing;  // the first required name that was not found
  const void* pk(const std::string& n, bool required = true) { return need(PK(m, n), n, required); }
  const float* p32(const std::string& n, bool required = true) { return need(P32(m, n), n, required); }
  // `name`.weight packed (bias: + the fp32 `name`.bias)
  ConvW conv(const std::string& name, bool bias = true) { return {pk(name + ".weight"), bias ? p32(name + ".bias") : nullptr}; }
  // the composed packs: `name`.weight + their nine bias classes `name`.bias
  ConvW composed(const std::string& name, bool required = true) {
    return {pk(name + ".weight", required), (const float*)pk(name + ".bias", required)};
  }
  int status() const {
    if (!missing.empty()) MD_FAIL(MD_ERR_FORMAT, "parameter `%s` is not in the model's inventory", missing.c_str());
    return MD_OK;
  }

 private:
  template <typename T>
  T need(T p, const std::string& n, bool required) {
    if (!p && required && missing.empty()) missing = n;
    return p;
  }
};

// the common tail of the add_pack* helpers: the entry's size, its name and its place in the plan
inline void push_pack(md_model_s* m, const std::string& name, PackEntry e) {
  e.bytes = pack_bytes(m, e);
  m->pack_index[name] = (int)m->packs.size();
  m->packs.push_back(e);
}

// `param` (default: `name` itself) packed under `name`: a second packed form of a parameter has a name of its own (e.g. a
// convolution weight both as a direct-convolution and as an implicit-GEMM operand)
inline void add_pack(md_model_s* m, const std::string& name, int kind, int d0, int d1, int k, bool f32 = false, const std::string& param = "") {
  auto it = m->pindex.find(param.empty() ? name : param);
  if (it == m->pindex.end()) return;
  PackEntry e;
  e.param = it->second; e.kind = kind; e.d0 = d0; e.d1 = d1; e.k = k;
  e.f32 = f32 ? 1 : 0;
  const int contraction = kind == PACK_DECONV ? d0 : d1;
  e.kp = f32 ? contraction : round_up(contraction, m->ke);
  push_pack(m, name, e);
}

// a bias-free deconv k2s2 and the layer behind it, packed as ONE deconvolution on their weight product. k == 2: a 1x1 conv [cout, cout]
// behind it, W'[ci][co][q] = sum_m Wd[ci][m][q] * Wo[co][m] (decoder.rs:124-141 applies out_conv right after deconv); k == 4: a second
// bias-free k2s2 deconvolution (encoder.rs:146-152, nothing between them) = ONE k4s4 deconvolution on the weight product
// W''[ci][co][2 dy1 + dy2][2 dx1 + dx2] = sum_m Wa[ci][m][dy1][dx1] * Wb[m][co][dy2][dx2]
inline void add_pack_product(md_model_s* m, const std::string& name, const std::string& a, const std::string& b, int k, int cin,
                             int cmid, int cout) {
  auto wa = m->pindex.find(a), wb = m->pindex.find(b);
  if (wa == m->pindex.end() || wb == m->pindex.end()) return;
  PackEntry e;
  e.param = wa->second; e.param2 = wb->second;
  if (k == 4) e.param3 = cmid;  // PACK_DECONV with k == 4 and param2: the middle channel count rides here
  e.kind = PACK_DECONV; e.d0 = cin; e.d1 = cout; e.k = k;
  e.kp = round_up(cin, m->ke);
  push_pack(m, name, e);
}

// `first` (+bias) -> `second` (+bias), nothing between them, composed at commit into one 3x3 convolution (`name`.weight, PACK_CONV3
// layout) and nine position-class bias vectors (`name`.bias, f32 [9][cout]). PACK_HEAD_W: the depth head's deconv k2s2 [cin, cmid] ->
// conv 3x3 [cout, cmid] on the deconv's input grid with 4 * cout columns; PACK_C1C3_W: a conv 1x1 [cmid, cin] -> conv 3x3 pad 1
inline void add_pack_fused(md_model_s* m, int kind, const std::string& name, const std::string& first, const std::string& second, int cin,
                           int cmid, int cout) {
  auto w1 = m->pindex.find(first + ".weight"), b1 = m->pindex.find(first + ".bias");
  auto w2 = m->pindex.find(second + ".weight"), b2 = m->pindex.find(second + ".bias");
  if (w1 == m->pindex.end() || b1 == m->pindex.end() || w2 == m->pindex.end() || b2 == m->pindex.end()) return;
  PackEntry e;
  e.param = w1->second; e.param2 = w2->second; e.param3 = b1->second; e.param4 = b2->second;
  e.kind = kind;
  e.d0 = cout; e.d1 = cin; e.k = cmid;
  e.kp = round_up(cin, m->ke);
  push_pack(m, name + ".weight", e);
  e.kind = kind + 1;  // PACK_HEAD_B / PACK_C1C3_B
  e.f32 = 1;
  push_pack(m, name + ".bias", e);
}

// The graph layer of an infer entry: `body` through the model's GraphCache when graphs are on and the call is `eligible`. Timing /
// tap modes and calls with host-side buffers always run eagerly.
template <typename F>
inline int run_with_graph(md_model_s* m, hipStream_t st, const std::vector<uintptr_t>& key, bool eligible, F&& body) {
  if (!m->graph_enabled) return body();
  m->graphs.track_generation(model_root(m)->commit_gen);
  if (!eligible || m->timing_enabled || m->taps_enabled) return body();
  return m->graphs.run(st, key, body);
}

struct Run {
  md_model_s* m;
  hipStream_t st;
  int B;
  int pending = -1;
  void begin(const char* name) {
    if (!m->timing_enabled) return;
    if (!m->timing_filter.empty() && m->timing_filter != name) return;
    TimingEntry t;
    t.name = name;
    (void)hipEventCreate(&t.a);
    (void)hipEventCreate(&t.b);
    (void)hipEventRecord(t.a, st);
    m->timing.push_back(t);
    pending = (int)m->timing.size() - 1;
  }
  void end() {
    if (!m->timing_enabled || pending < 0) return;
    (void)hipEventRecord(m->timing[pending].b, st);
    pending = -1;
  }
  // the tap `name` holding n floats: reallocated at exactly n when the count changes (debug memory, not counted in alloc_count)
  int sized_tap(const char* name, size_t n, Tap** out) {
    Tap& t = m->taps[name];
    if (t.count != n) {
      if (t.dev) (void)hipFree(t.dev);
      t.dev = nullptr;
      t.count = 0;
      MD_HIP(hipMalloc((void**)&t.dev, n * 4));
      t.count = n;
    }
    *out = &t;
    return MD_OK;
  }
  // NHWC T tensor -> NCHW fp32 tap
  int tap_nhwc(const char* name, const void* p, int C, int H, int W, long ld, int coff = 0) {
    if (!m->taps_enabled) return MD_OK;
    Tap* t = nullptr;
    MD_TRY(sized_tap(name, (size_t)B * C * H * W, &t));
    t->dims[0] = B; t->dims[1] = C; t->dims[2] = H; t->dims[3] = W;
    return launch_nhwc_to_nchw(p, B, C, H, W, ld, coff, t->dev, m->prec, st);
  }
  // token rows of an fp32 [B*S, width] tensor -> tap [B, nrows, dst_width] columns [coff, coff + width): rows row0 .. row0+nrows of
  // every sequence (the patch tokens of a hook, depth_anything3/mod.rs:344-347). Call once per column block.
  int tap_token_rows(const char* name, const float* src, int S, int row0, int nrows, int width, int dst_width, int coff) {
    if (!m->taps_enabled) return MD_OK;
    Tap* t = nullptr;
    MD_TRY(sized_tap(name, (size_t)B * nrows * dst_width, &t));
    t->dims[0] = B; t->dims[1] = nrows; t->dims[2] = dst_width; t->dims[3] = 0;
    for (int b = 0; b < B; ++b)
      MD_HIP(hipMemcpy2DAsync(t->dev + ((size_t)b * nrows) * dst_width + coff, (size_t)dst_width * 4, src + ((size_t)b * S + row0) * width,
                              (size_t)width * 4, (size_t)width * 4, (size_t)nrows, hipMemcpyDeviceToDevice, st));
    return MD_OK;
  }
  int tap_f32(const char* name, const float* p, int64_t d0, int64_t d1, int64_t d2, int64_t d3) {
    if (!m->taps_enabled) return MD_OK;
    const size_t n = (size_t)d0 * std::max<int64_t>(d1, 1) * std::max<int64_t>(d2, 1) * std::max<int64_t>(d3, 1);
    Tap* t = nullptr;
    MD_TRY(sized_tap(name, n, &t));
    t->dims[0] = d0; t->dims[1] = d1; t->dims[2] = d2; t->dims[3] = d3;
    MD_HIP(hipMemcpyAsync(t->dev, p, n * 4, hipMemcpyDeviceToDevice, st));
    return MD_OK;
  }
};

inline int cpad(const md_model_s* m, int ch) { return (ch + m->ke - 1) / m->ke * m->ke; }

// ---- split-half operands (MD_PREC_F16X2; every function below is the identity on the one-plane modes) ----
// Callers pass LOGICAL padded channel counts (row widths, K); an activation row is physically [hi | lo] and a weight row
// `terms` copies of its contraction (2: [W | W], 3: [Wh | Wh | Wl]). terms == 0 = the model's plain-weight form
// (md_model_s::wterms); the products composed at commit are never f16-exact and pass 3.
// (a fork reads its ROOT's term count: a re-commit on the root may change it while the fork lives, and the packed rows the
// fork's launches read are the root's)
// What these helpers and the launch-parameter builders below read of a model, and ALL they read: the operand geometry of its
// precision. The engines pass geom_of(model); the stand-alone operator entries (md_api.cpp, OpStage) build one for a precision alone.
struct OperandGeom {
  int ke = 64;      // contraction elements per 128-byte LDS row
  int xm = 1;       // planes per activation element (2: split-half)
  int wterms = 1;   // split-half: MFMA terms of a product with a plain weight (md_model_s::wterms of the ROOT model)
  void* zero_page = nullptr;
};
inline OperandGeom geom_of(const md_model_s* m) { return OperandGeom{m->ke, m->xm, (m->parent ? m->parent : m)->wterms, m->zero_page}; }
inline int split_terms(const OperandGeom& o, int terms) { return o.xm == 1 ? 1 : (terms > 0 ? terms : o.wterms); }
inline int split_terms(const md_model_s* m, int terms) { return split_terms(geom_of(m), terms); }
// dense / indexed A operand of `kp` logical channels per row
inline void split_dense_a(const OperandGeom& o, GemmParams& p, int kp, long lda, int terms) {
  const int t = split_terms(o, terms);
  p.K = kp * t;
  p.lda = lda * o.xm;
  p.a_wrap = t == 3 ? 2 * kp / o.ke : 0;
}
inline void split_dense_a(const md_model_s* m, GemmParams& p, int kp, long lda, int terms) { split_dense_a(geom_of(m), p, kp, lda, terms); }
// 3x3-convolution A operand: NHWC pixels of `cin_p` logical channels
inline void split_conv_a(const OperandGeom& o, GemmParams& p, int cin_p, int terms) {
  const int t = split_terms(o, terms);
  p.cC = cin_p * o.xm;
  p.cCk = o.xm == 1 ? 0 : cin_p * t;
  p.K = 9 * cin_p * t;
  p.a_wrap = t == 3 ? 2 * cin_p / o.ke : 0;
}
inline void split_conv_a(const md_model_s* m, GemmParams& p, int cin_p, int terms) { split_conv_a(geom_of(m), p, cin_p, terms); }
// T-typed output (and residual inputs) with `ldo` logical channels per row
inline void split_out(const OperandGeom& o, GemmParams& p, long ldo, bool t_out) {
  if (!t_out) { p.ldo = ldo; return; }
  p.ldo = ldo * o.xm;
  p.o_plane = o.xm == 2 ? ldo : 0;
}
inline void split_out(const md_model_s* m, GemmParams& p, long ldo, bool t_out) { split_out(geom_of(m), p, ldo, t_out); }

// 1x1 conv / linear over NHWC rows.  A may be gathered through `idx`. `res1` (T-typed rows of ldo): a residual table whose row is
// m % res_mod (the Depth-Anything-v3 stage projection's position table, one per image)
// (the launch parameters apart from the launch: md_op_indexed_gemm launches the very same ones)
inline GemmParams rows_params(const OperandGeom& m, const void* A, long lda, const int* idx, long M, const void* W, int N, int K,
                              const float* bias, void* out, long ldo, int out_f32 = 0, int act = ACT_NONE, int terms = 0,
                              const void* res1 = nullptr, int res_mod = 0) {
  GemmParams p;
  p.N = N; p.ngroups = 1; p.g_rows[0] = (int)M; p.W[0] = W;
  p.A = A; p.a_index = idx;
  split_dense_a(m, p, K, lda, terms);
  p.epi = EPI_STORE; p.act = act; p.out_f32 = out_f32; p.bias[0] = bias; p.out = out;
  split_out(m, p, ldo, !out_f32);
  if (res1) { p.res1 = res1; p.ldr = p.ldo; p.r_plane = p.o_plane; p.res_mod = res_mod; }
  return p;
}
inline int gemm_rows(Run& r, const char* name, const void* A, long lda, const int* idx, long M, const void* W, int N, int K,
              const float* bias, void* out, long ldo, int out_f32 = 0, int act = ACT_NONE, int terms = 0) {
  const GemmParams p = rows_params(geom_of(r.m), A, lda, idx, M, W, N, K, bias, out, ldo, out_f32, act, terms);
  r.begin(name);
  int s = launch_gemm(p, idx ? A_INDEXED : A_DENSE, r.m->prec, TILE_AUTO, r.st);
  r.end();
  return s;
}

// ConvTranspose2d k=2 s=2 as GEMM + pixel shuffle (encoder.rs:61-69, decoder.rs:100-105, mod.rs:81-84)
// (the launch parameters apart from the launch: md_op_deconv2x2 / md_op_conv3x3 / md_op_decoder_gemm launch the very same ones)
inline GemmParams deconv2_params(const OperandGeom& m, int B, const void* A, long lda, const int* idx, int h, int w, const void* W, int Cin_p,
                                 int Cout, const float* bias, void* out, long ldo, int coff, void* out2 = nullptr, int f = 2, int terms = 0) {
  GemmParams p;
  p.N = f * f * Cout; p.ngroups = 1; p.g_rows[0] = B * h * w; p.W[0] = W; p.ps_f = f;
  p.A = A; p.a_index = idx;
  split_dense_a(m, p, Cin_p, lda, terms);
  p.epi = EPI_PIXSHUF; p.bias[0] = bias; p.out = out; p.out2 = out2;
  split_out(m, p, ldo, true);
  p.psH = h; p.psW = w; p.psC = Cout; p.ps_coff = coff;
  return p;
}
inline int deconv2(Run& r, const char* name, const void* A, long lda, const int* idx, int h, int w, const void* W, int Cin_p,
            int Cout, const float* bias, void* out, long ldo, int coff, void* out2 = nullptr, int f = 2, int terms = 0) {
  const GemmParams p = deconv2_params(geom_of(r.m), r.B, A, lda, idx, h, w, W, Cin_p, Cout, bias, out, ldo, coff, out2, f, terms);
  r.begin(name);
  int s = launch_gemm(p, idx ? A_INDEXED : A_DENSE, r.m->prec, TILE_AUTO, r.st);
  r.end();
  return s;
}

// Conv2d 3x3 s1 p1 over NHWC as implicit GEMM (decoder.rs:55-72,167-175; mod.rs:78-87). G > 1: weight set w[g] over images
// [g*B, (g+1)*B) of `in` / `out` (`in_shared`: every group reads images [0, B) of `in`; `res1_shared`: the same for res1)
inline GemmParams conv3_params(const OperandGeom& m, int B, const void* in, int H, int W, int Cin_p, const ConvW* w, int Cout, void* out,
                                long ldo, int act, const void* res1, const void* res2, void* out2, int terms = 0, int G = 1,
                                bool in_shared = false, bool res1_shared = false) {
  GemmParams p;
  const int M = B * H * W;
  p.N = Cout; p.ngroups = G;
  for (int g = 0; g < G; ++g) {
    p.g_rows[g] = M; p.g_row0[g] = g * M; p.g_arow0[g] = in_shared ? 0 : g * M;
    p.W[g] = w[g].w; p.bias[g] = w[g].b;
  }
  p.A = in; p.cH = H; p.cW = W; p.zero_page = m.zero_page;
  split_conv_a(m, p, Cin_p, terms);
  p.epi = EPI_STORE; p.act = act; p.out = out; p.out2 = out2;
  split_out(m, p, ldo, true);
  p.res1 = res1; p.res2 = res2; p.ldr = p.ldo; p.r_plane = (res1 || res2) ? p.o_plane : 0;
  if (res1 && res1_shared && G > 1) p.res_mod = M;
  return p;
}
inline int conv3(Run& r, const char* name, const void* in, int H, int W, int Cin_p, const ConvW* w, int Cout, void* out, long ldo,
                 int act, const void* res1, const void* res2, void* out2, int terms = 0, int G = 1, bool in_shared = false,
                 bool res1_shared = false) {
  const GemmParams p = conv3_params(geom_of(r.m), r.B, in, H, W, Cin_p, w, Cout, out, ldo, act, res1, res2, out2, terms, G, in_shared, res1_shared);
  r.begin(name);
  int s = launch_gemm(p, A_CONV3, r.m->prec, TILE_AUTO, r.st);
  r.end();
  return s;
}

// ResidualBlock / ResidualConvUnit (decoder.rs:74-87, dpt.rs:1248-1252): out = x + conv2(relu(conv1(relu(x)))) [+ extra] on C
// channels (Cp padded), `xr` = relu(x), `t` scratch; u[g] per weight group as in conv3 (`x_shared`: x and xr are shared)
inline int residual_unit(Run& r, const char* name, const ResUnitW* u, int G, int H, int W, int Cp, int C, const void* x,
                         const void* xr, bool x_shared, const void* extra, void* t, void* out, void* out_relu) {
  const ConvW c1[2] = {u[0].c1, u[G - 1].c1}, c2[2] = {u[0].c2, u[G - 1].c2};
  MD_TRY(conv3(r, name, xr, H, W, Cp, c1, C, t, Cp, ACT_RELU, nullptr, nullptr, nullptr, 0, G, x_shared));
  return conv3(r, name, t, H, W, Cp, c2, C, out, Cp, ACT_NONE, x, extra, out_relu, 0, G, false, x_shared);
}

// fp32 attention as three launches: scores = q k^T (batched GEMM) -> row softmax -> P V^T^T (batched GEMM). qk [nseq*S, 2D] (q | k),
// vT [nseq][heads][64][kpad], scores [nseq*heads*S, kpad] fp32 scratch, out [nseq*S, D]. `r` (optional) times the three launches.
int attention_f32(Run* r, hipStream_t st, const void* qk, const void* vT, void* out, float* scores, int nseq, int S, int n_tokens,
                  int heads, int kpad);

// ---- the DINOv2 ViT block (Depth Pro's three encoders, Depth-Anything-v3's backbone) ----
// the packs of the ViT under `prefix`: patch embedding, then qkv | proj | fc1 | fc2 of every block
void vit_add_packs(md_model_s* m, const std::string& prefix, const ViTDims& v);
// the weight tables of the ViT under `prefix` (after the packed arena is placed)
void vit_bind(md_model_s* m, const std::string& prefix, int depth, VitW& w);

// One call's ViT stage as run_vit_block sees it, filled once per call. Row group g is vit[g] on sequences [glo[g], glo[g] + gcnt[g])
// (Depth Pro: its encoders clipped to the window; Depth-Anything-v3: one group over the batch). Buffers are the workspace bases:
// GEMMs address absolute rows, LayerNorms and attention the window's sequences [s_lo, s_lo + WS).
struct VitPlan {
  int G = 1;
  const VitW* vit[3] = {nullptr, nullptr, nullptr};
  int glo[3] = {0, 0, 0}, gcnt[3] = {0, 0, 0};
  int s_lo = 0, WS = 0;
  int views = 1;                            // > 1: global blocks attend across the `views` consecutive sequences of a scene (WS % views == 0)
  int D = 0, heads = 0, SS = 0, NT = 0, kpad = 0;
  float ln_eps = 0.f;
  float* x = nullptr;     // fp32 residual stream; a global block writes `xalt` and the two swap
  float* xalt = nullptr;
  void *xn = nullptr, *qk = nullptr, *vT = nullptr, *ao = nullptr, *hbuf = nullptr;
  float* scores = nullptr;                  // MD_PREC_F32 attention
  int* redo = nullptr;                      // launch_attention's assembly-kernel flags (null: never the assembly kernel)
  int redo_units = 0;
  // LayerNorm fold (md_model_s::ln_fold_opt): folded / neutral (3) statistics, finished by an ln_finish launch (3, 4)
  bool fold = false, neutral = false, finish_launch = false;
  float *ln_stats = nullptr, *ln_ab = nullptr;
  const float* zero_c = nullptr;
  int lin_prec = MD_PREC_BF16;              // operands of the four linear layers (MD_PREC_FP8: e4m3, VitBlockW::w8)
  float a_scale = 0.f, h_scale = 0.f;       // MD_PREC_FP8: static scales of the LayerNorm / attention and of the GELU outputs
  float qk_norm_eps = 0.f;                  // blocks with VitBlockW::qkn_*: RoPE tables of this input size
  const float *rope_cos = nullptr, *rope_sin = nullptr;
  int rope_pw = 0;
  int tok0_block = -1;                      // entering this block, row 0 of every sequence becomes tok0 (+ b * tok0_stride)
  const float* tok0 = nullptr;
  int tok0_stride = 0;
};
// Block i: LayerNorm 1 -> qkv GEMM -> attention -> proj GEMM (+ residual) -> LayerNorm 2 -> fc1 GEMM (GELU) -> fc2 GEMM (+ residual)
int run_vit_block(Run& r, VitPlan& v, int i);


}  // namespace md
