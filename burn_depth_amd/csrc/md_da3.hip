// Depth-Anything-v3 on the same kernel set: `metric_large` (ViT-L/14 + mono DPT head) and `small` (ViT-S/14 with
// the burn_dino extras -- QK-norm, 2-D RoPE, local/global alternation, camera token, concatenated hooks -- + dual
// DPT head with the aux/ray branch + camera decoder; reference: mod.rs:158-216, dpt.rs:153-513, camera.rs:113-199,
// 281-416; the backbone extras are restated from the public model, see oracle/da3_ref.py).
//
// reference: src/model/depth_anything3/mod.rs:288-291,495-624 (infer), dpt.rs:515-731 (mono head),
// dpt.rs:784-932 (UV position embedding), dpt.rs:1194-1301 (fusion blocks), interpolate.rs:7-47.
// The backbone is burn_dino's plain DINOv2 ViT (un-vendored; restated, parity unpinned): hooks are the
// final-LayerNorm'ed outputs of the hook blocks with the cls token dropped.
//
// Layout: tokens [b*SS + token, D] (fp32 residual, T operands), head feature maps NHWC. The mono head is
// 1x1 conv (GEMM over gathered token rows, + UV position table as an epilogue addend) -> k4s4 / k2s2
// ConvTranspose (GEMM + pixel shuffle) or 3x3 stride-2 conv (implicit GEMM with stride) -> 3x3 convs,
// residual units and align-corners-true bilinear resizes in NHWC -> fused tail
// exp(w_out . relu(conv1) + b) written straight to the depth output.
#include <cmath>
#include <cstring>

#include "md_engine.h"
#include "md_engine_util.h"

using namespace md;

struct md_model_s::Da3State {
  Da3Cfg cfg;
  int ih = 0, iw = 0;  // configured input size (rows x columns; any multiples of the patch size)
  int ph = 0, pw = 0, P = 0, NT = 0, SS = 0, kpad = 0, Kp = 0, h3h = 0, h3w = 0;
  VitW vit;
  // workspace
  void *patches = nullptr, *xn = nullptr, *qk = nullptr, *vT = nullptr, *ao = nullptr, *hbuf = nullptr;
  float *xres = nullptr, *lnf = nullptr, *scores = nullptr, *xin = nullptr;
  void* hookn[4] = {0, 0, 0, 0};
  void *sp[4] = {0, 0, 0, 0}, *sr[4] = {0, 0, 0, 0}, *rn[4] = {0, 0, 0, 0}, *rnr[4] = {0, 0, 0, 0};
  void *t = nullptr, *x = nullptr, *xr = nullptr, *y = nullptr, *up = nullptr, *o = nullptr, *c1 = nullptr, *c1r = nullptr;
  GrowBuf<float> depth_stage;  // device home of a host output (grow-only, md::grow)
  // ---- per-shape tables: the reference's `PosEmbedCache` (dpt.rs:784-833: UV tables built once per (C, h, w, W, H) key and
  //      kept) and burn_dino's position-embedding interpolation, keyed by the input size. `infer` takes any H x W that are
  //      multiples of the patch size (mod.rs:509-520); the first call at a new size builds its tables (host work + uploads),
  //      later calls at that size find them here. At most kMaxShapes sizes are kept (least recently used goes first).
  struct ShapeTables {
    void* pos_stage[4] = {0, 0, 0, 0};  // T [P, cp(oc)] = 0.1 * UV embedding
    float* pos_final = nullptr;         // f32 [H*W, F/2]
    float* pos_aux = nullptr;           // f32 [8ph*8pw, F/2] = 2 * 0.1 * UV table (added twice, dpt.rs:428-435)
    float* pos_used = nullptr;          // [NT, D] position embedding interpolated to this grid (null: the native grid)
    float *rope_cos = nullptr, *rope_sin = nullptr;  // [max(ph, pw) + 2][16]
    std::map<int, int*> tok_index;      // per B: [B*P] -> row b*SS + 1 + p
    unsigned long last_use = 0;
  };
  static constexpr int kMaxShapes = 16;
  std::map<std::pair<int, int>, ShapeTables> shapes;
  unsigned long use_clock = 0;
  long table_builds = 0;              // shapes built so far (md_model_query "da3_shape_builds")
  // the CURRENT shape's tables (aliases into `shapes`)
  void* pos_stage[4] = {0, 0, 0, 0};
  float* pos_final = nullptr;
  std::map<int, int*>* tok_index = nullptr;
  float* pos_used = nullptr;
  int native_grid = 0;
  // ---- `small` (dual head) ----
  std::string hp = "head_mono";       // head parameter prefix
  // ---- weight tables behind the backbone, bound at create (da3_bind) ----
  const float* pos_native = nullptr;  // the pos_embed parameter (its native grid)
  const float *head_norm_g = nullptr, *head_norm_b = nullptr;  // the dual head's token norm
  const float* camera_token = nullptr;  // the learned reference-view camera token (dual head)
  ConvW proj[4], resize[4], layer_rn[4];  // projects, resize_layers 0 | 1 | 3 (2 is the identity), layerN_rn (no bias)
  // refinenet1..4 of the main | aux ("_aux") pyramid, group innermost: residual1 (none at level 3) | residual2, out_conv
  ResUnitW res[4][2][2];
  ConvW out_conv[4][2];
  ConvW oc1, oc2_1, oc2_2;              // output_conv1, output_conv2.conv1, output_conv2.conv2 (fp32 weight and bias)
  std::vector<ConvW> aux_neck;          // the last aux level: output_conv1_aux layers, output_conv2_aux reduce | project (fp32)
  ConvW aux_reduce, aux_project;
  CamEncW cam_enc{};                    // camera encoder (checked where it runs), camera decoder
  CamDecW cam_dec{};
  int din = 0;                        // head input width: D (mono) or 2D (concatenated hooks)
  float* xlocal = nullptr;            // [rows, D] fp32: residual stream after the last LOCAL block
  float* rope_cos = nullptr;          // current shape's tables (aliases)
  float* rope_sin = nullptr;
  float *cam_raw = nullptr, *cam_h1 = nullptr, *cam_h2 = nullptr, *pose = nullptr, *extr = nullptr, *intr = nullptr;
  float* view_tok = nullptr;          // [max_batch, D]: the camera token of every sequence of a multi-view call (slot 0 | slot 1 ...)
  float* pos_aux = nullptr;
  float *conf_stage = nullptr, *aux_stage = nullptr;  // device staging when the caller wants host outputs
  // camera encoder (`infer_with_camera`): grow-only scratch = staged inputs [B*V*21] | encoded tokens [B*D] | kernel scratch
  GrowBuf<float> cam_enc_ws;
  // `infer_from_tokens`: caller-supplied hook tokens staged as fp32 rows [max_batch * SS + 64, din] (grow-only, zero-filled on growth)
  GrowBuf<float> tok_stage;
  void *up2 = nullptr, *o2 = nullptr;
  std::vector<float> main_bias, aux_bias;             // output_conv2.conv2.bias, output_conv2_aux.<last>.project.bias
  // ---- MD_PREC_FP8: the four ViT linear layers on e4m3 operands (weights per output channel, static activation scales) ----
  bool fp8 = false;
  char* w8_base = nullptr;                            // one allocation: per block qkv | proj | fc1 | fc2 (e4m3) + their scales (VitBlockW::w8 / s8)
  static constexpr float kActScale = 8.0f / 448.0f;   // LayerNorm output, attention output
  static constexpr float kHidScale = 16.0f / 448.0f;  // GELU output
};

namespace md {

// dpt.rs:835-932 -- the reference's table, including its transposed pixel index (dpt.rs:879)
static void sincos(int dim, float position, float* out) {
  const int half = dim / 2;
  for (int i = 0; i < half; ++i) {
    const float exponent = half > 0 ? (float)i / (float)half : 0.f;
    const float omega = powf(100.0f, -exponent);
    out[i] = sinf(position * omega);
  }
  const int remaining = dim - half;
  for (int i = 0; i < remaining; ++i) {
    const float exponent = remaining > 0 ? (float)i / (float)remaining : 0.f;
    const float omega = powf(100.0f, -exponent);
    out[half + i] = cosf(position * omega);
  }
}

// returns NHWC [h*w][C] scaled by `ratio`
static std::vector<float> build_pos_table_nhwc(int C, int h, int w, int image_w, int image_h, float ratio) {
  const float aspect = (float)image_w / (float)image_h;
  const float diag = sqrtf(aspect * aspect + 1.0f);
  const float span_x = aspect / diag, span_y = 1.0f / diag;
  const float left_x = -span_x * ((float)w - 1.0f) / (float)w, right_x = span_x * ((float)w - 1.0f) / (float)w;
  const float top_y = -span_y * ((float)h - 1.0f) / (float)h, bottom_y = span_y * ((float)h - 1.0f) / (float)h;
  auto lin = [](float a, float b, int n, int i) { return n <= 1 ? a : a + ((b - a) / ((float)n - 1.0f)) * (float)i; };
  const int xc = C / 2, yc = C - xc;
  std::vector<float> ex((size_t)w * xc), ey((size_t)h * yc);
  for (int i = 0; i < w; ++i) sincos(xc, lin(left_x, right_x, w, i), ex.data() + (size_t)i * xc);
  for (int i = 0; i < h; ++i) sincos(yc, lin(top_y, bottom_y, h, i), ey.data() + (size_t)i * yc);
  std::vector<float> t((size_t)h * w * C);
  // reference: chw[c*h*w + (x_idx*height + y_idx)], then viewed as [C, h, w]
  for (int xi = 0; xi < w; ++xi)
    for (int yi = 0; yi < h; ++yi) {
      const size_t pix = (size_t)xi * h + yi;  // flat pixel index inside the [h, w] view
      float* dst = t.data() + pix * C;
      for (int c = 0; c < xc; ++c) dst[c] = ex[(size_t)xi * xc + c] * ratio;
      for (int c = 0; c < yc; ++c) dst[xc + c] = ey[(size_t)yi * yc + c] * ratio;
    }
  return t;
}

// 2-D RoPE tables: angle(pos, f) = pos * base^(-2f/32), f < 16 (fp32 like the oracle); positions 0 .. max(ph, pw) + 1
void da3_rope_tables(int ph, int pw, float base, std::vector<float>* cos_out, std::vector<float>* sin_out) {
  const int npos = std::max(ph, pw) + 2;
  std::vector<float>&rc = *cos_out, &rs = *sin_out;
  rc.assign((size_t)npos * 16, 0.f);
  rs.assign((size_t)npos * 16, 0.f);
  for (int pz = 0; pz < npos; ++pz)
    for (int f = 0; f < 16; ++f) {
      const float inv = 1.0f / powf(base, (float)(2 * f) / 32.0f);
      const float ang = (float)pz * inv;
      rc[(size_t)pz * 16 + f] = cosf(ang);
      rs[(size_t)pz * 16 + f] = sinf(ang);
    }
}

// DINOv2 `interpolate_pos_encoding`: bicubic (A = -0.75, align_corners = False), scale factor
// (grid + 0.1) / native_grid per axis, source index = (dst + 0.5) / scale - 0.5, border-clamped taps.
// burn_dino's version is not visible (parity unpinned); this restates the public DINOv2 code path
// (torch.nn.functional.interpolate with scale_factor, which the oracle calls directly).
static void cubic_coeffs(float t, float w[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
  w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
  w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

static std::vector<float> interpolate_pos_embed(const std::vector<float>& pos, int M, int D, int ph, int pw) {
  std::vector<float> out((size_t)(1 + ph * pw) * D);
  memcpy(out.data(), pos.data(), (size_t)D * 4);  // class token position is kept
  const float sy = 1.0f / (((float)ph + 0.1f) / (float)M), sx = 1.0f / (((float)pw + 0.1f) / (float)M);
  for (int oy = 0; oy < ph; ++oy) {
    const float fy = sy * ((float)oy + 0.5f) - 0.5f;
    const int iy = (int)floorf(fy);
    float wy[4];
    cubic_coeffs(fy - (float)iy, wy);
    for (int ox = 0; ox < pw; ++ox) {
      const float fx = sx * ((float)ox + 0.5f) - 0.5f;
      const int ix = (int)floorf(fx);
      float wx[4];
      cubic_coeffs(fx - (float)ix, wx);
      float* dst = out.data() + (size_t)(1 + oy * pw + ox) * D;
      for (int c = 0; c < D; ++c) dst[c] = 0.f;
      for (int a = 0; a < 4; ++a) {
        const int yy = std::min(std::max(iy - 1 + a, 0), M - 1);
        for (int b = 0; b < 4; ++b) {
          const int xx = std::min(std::max(ix - 1 + b, 0), M - 1);
          const float wgt = wy[a] * wx[b];
          const float* src = pos.data() + (size_t)(1 + yy * M + xx) * D;
          for (int c = 0; c < D; ++c) dst[c] += wgt * src[c];
        }
      }
    }
  }
  return out;
}

static void da3_drop_shapes(md_model_s* m);
static int da3_set_shape(md_model_s* m, int H, int W, bool force);

int da3_on_commit(md_model_t m) {
  md_model_s::Da3State* d = m->da3;
  const int D = d->cfg.vit.D;
  if (d->fp8) {  // e4m3 copies of the ViT linear weights, one scale per output channel
    const int nn[4] = {3 * D, D, 4 * D, D}, kk[4] = {D, D, D, 4 * D};
    for (const VitBlockW& k : d->vit.blk)
      for (int j = 0; j < 4; ++j) {
        if (!k.w32[j]) MD_FAIL(MD_ERR_FORMAT, "missing ViT weight for the fp8 pack");
        MD_TRY(launch_pack_fp8_rows(k.w32[j], nn[j], kk[j], kk[j], k.w8[j], k.s8[j], m->dev->stream));
      }
    MD_HIP(hipStreamSynchronize(m->dev->stream));
  }
  const Da3Cfg& c = d->cfg;
  d->main_bias.assign(c.output_dim, 0.f);
  MD_HIP(hipMemcpy(d->main_bias.data(), d->oc2_2.b, c.output_dim * 4, hipMemcpyDeviceToHost));
  if (c.dual_head) {
    d->aux_bias.assign(c.aux_output_dim, 0.f);
    MD_HIP(hipMemcpy(d->aux_bias.data(), d->aux_project.b, c.aux_output_dim * 4, hipMemcpyDeviceToHost));
  }
  // the interpolated position embeddings were made from the previous weights: drop every cached shape and rebuild the
  // current one from the committed parameters
  da3_drop_shapes(m);
  return da3_set_shape(m, d->ih, d->iw, /*force=*/true);
}

static int da3_plan(md_model_s* m, bool dry, size_t* total_out) {
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const int B = c.max_batch, D = c.vit.D, F = c.features;
  const int esz = m->esz * m->xm;  // bytes per LOGICAL element of a T tensor (MD_PREC_F16X2: two half planes)
  const size_t SS2 = (size_t)d->ih * d->iw;  // pixels of one input image
  const int* oc = c.out_channels;
  size_t total = 0;
  auto take = [&](size_t bytes) -> void* {
    bytes = align_up(bytes + 256, 256);
    total += bytes;
    return dry ? nullptr : m->ws.take(bytes);
  };
#define DA3_TAKE(field, type, bytes)                                          \
  do {                                                                        \
    void* _p = take(bytes);                                                   \
    if (!dry) {                                                               \
      if (!_p) MD_FAIL(MD_ERR_OOM, "workspace arena exhausted at " #field);   \
      d->field = (type)_p;                                                    \
    }                                                                         \
  } while (0)
  const size_t rows = (size_t)B * d->SS + 64;
  const int ph = d->ph, pw = d->pw;
  const size_t P = d->P;
  auto cp = [&](int ch) { return (size_t)round_up(ch, m->ke); };
  DA3_TAKE(xin, float*, (size_t)B * 3 * SS2 * 4);
  DA3_TAKE(patches, void*, (size_t)B * P * d->Kp * esz);
  DA3_TAKE(xres, float*, rows * D * 4);
  DA3_TAKE(lnf, float*, rows * D * 4);
  DA3_TAKE(xn, void*, rows * D * esz);
  DA3_TAKE(qk, void*, rows * 2 * D * esz);
  DA3_TAKE(vT, void*, (size_t)B * c.vit.heads * 64 * d->kpad * esz);
  m->vt_plane = m->xm == 2 ? (size_t)B * c.vit.heads * 64 * d->kpad : 0;
  DA3_TAKE(ao, void*, rows * D * esz);
  DA3_TAKE(hbuf, void*, rows * 4 * D * esz);
  if (m->prec == MD_PREC_F32) DA3_TAKE(scores, float*, (size_t)B * c.vit.heads * d->SS * d->kpad * 4);
  for (int s = 0; s < 4; ++s) DA3_TAKE(hookn[s], void*, rows * d->din * esz);
  if (c.dual_head) {
    DA3_TAKE(xlocal, float*, rows * D * 4);
    DA3_TAKE(cam_raw, float*, (size_t)B * d->din * 4);
    DA3_TAKE(view_tok, float*, (size_t)B * D * 4);
    DA3_TAKE(cam_h1, float*, (size_t)B * d->din * 4);
    DA3_TAKE(cam_h2, float*, (size_t)B * d->din * 4);
    DA3_TAKE(pose, float*, (size_t)B * 9 * 4);
    DA3_TAKE(extr, float*, (size_t)B * 12 * 4);
    DA3_TAKE(intr, float*, (size_t)B * 9 * 4);
    DA3_TAKE(conf_stage, float*, (size_t)B * SS2 * 4);
    DA3_TAKE(aux_stage, float*, (size_t)B * c.aux_output_dim * 64 * ph * pw * 4);
  }
  const size_t px[4] = {(size_t)16 * ph * pw, (size_t)4 * ph * pw, (size_t)ph * pw, (size_t)d->h3h * d->h3w};
  for (int s = 0; s < 4; ++s) {
    DA3_TAKE(sp[s], void*, (size_t)B * P * cp(oc[s]) * esz);
    if (s != 2) DA3_TAKE(sr[s], void*, (size_t)B * px[s] * cp(oc[s]) * esz);
    DA3_TAKE(rn[s], void*, (size_t)B * px[s] * cp(F) * esz);
    DA3_TAKE(rnr[s], void*, (size_t)B * px[s] * cp(F) * esz);
  }
  const size_t big = (size_t)B * 64 * ph * pw * cp(F) * esz;  // 8ph x 8pw
  // the dual head runs its two fusion pyramids in the same launches: every pyramid map holds 2B images (main | aux)
  const size_t pg = c.dual_head ? 2 : 1;
  DA3_TAKE(t, void*, pg * big / 4);
  DA3_TAKE(x, void*, pg * big / 4);
  DA3_TAKE(xr, void*, pg * big / 4);
  DA3_TAKE(y, void*, pg * big / 4);
  DA3_TAKE(up, void*, pg * big);
  DA3_TAKE(o, void*, pg * big);
  if (c.dual_head) {  // ping-pong maps of the aux neck (it runs beside the main tail, which reads `o`)
    DA3_TAKE(up2, void*, big);
    DA3_TAKE(o2, void*, big);
  }
  DA3_TAKE(c1, void*, (size_t)B * 64 * ph * pw * cp(F / 2) * esz);
  DA3_TAKE(c1r, void*, (size_t)B * SS2 * cp(F / 2) * esz);
#undef DA3_TAKE
  if (total_out) *total_out = total + 4096;
  return MD_OK;
}

static void da3_set_geometry(md_model_s* m, int H, int W) {
  md_model_s::Da3State* d = m->da3;
  const ViTDims& v = d->cfg.vit;
  d->ih = H;
  d->iw = W;
  d->ph = H / v.ps;
  d->pw = W / v.ps;
  d->P = d->ph * d->pw;
  d->NT = d->P + 1;
  d->SS = round_up(d->NT, 4);
  d->kpad = round_up(d->NT, 64);
  d->Kp = round_up(3 * v.ps * v.ps, m->ke);
  d->h3h = (d->ph + 2 - 3) / 2 + 1;
  d->h3w = (d->pw + 2 - 3) / 2 + 1;
  m->SS = d->SS;
}

static void da3_free_tables(md_model_s::Da3State::ShapeTables& t) {
  for (int s = 0; s < 4; ++s)
    if (t.pos_stage[s]) (void)hipFree(t.pos_stage[s]);
  if (t.pos_final) (void)hipFree(t.pos_final);
  if (t.pos_aux) (void)hipFree(t.pos_aux);
  if (t.pos_used) (void)hipFree(t.pos_used);
  if (t.rope_cos) (void)hipFree(t.rope_cos);
  if (t.rope_sin) (void)hipFree(t.rope_sin);
  for (auto& kv : t.tok_index) (void)hipFree(kv.second);
  t = md_model_s::Da3State::ShapeTables();
}

static void da3_drop_shapes(md_model_s* m) {
  md_model_s::Da3State* d = m->da3;
  (void)hipDeviceSynchronize();
  for (auto& kv : d->shapes) da3_free_tables(kv.second);
  d->shapes.clear();
  d->tok_index = nullptr;
  m->graphs.clear();  // captured graphs hold workspace / table pointers of the shape they were captured at
}

// UV position tables, interpolated position embedding and RoPE tables of one input size (PosEmbedCache::add /
// build_positional_embedding, dpt.rs:784-932; burn_dino's pos-embed interpolation, restated: interpolate_pos_embed above)
static int da3_build_tables(md_model_s* m, md_model_s::Da3State::ShapeTables& t) {
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const int IH = d->ih, IW = d->iw, F = c.features, D = c.vit.D, M = d->native_grid;
  const int* oc = c.out_channels;
  hipStream_t st = m->dev->stream;
  float* tmp = nullptr;
  size_t tmp_elems = 0;
  for (int s = 0; s < 4; ++s) tmp_elems = std::max(tmp_elems, (size_t)d->P * round_up(oc[s], m->ke));
  MD_HIP(hipMalloc((void**)&tmp, tmp_elems * 4));
  for (int s = 0; s < 4; ++s) {
    std::vector<float> tab = build_pos_table_nhwc(oc[s], d->ph, d->pw, IW, IH, 0.1f);
    const int ld = round_up(oc[s], m->ke);
    std::vector<float> padded((size_t)d->P * ld, 0.f);
    for (int p = 0; p < d->P; ++p) memcpy(&padded[(size_t)p * ld], &tab[(size_t)p * oc[s]], (size_t)oc[s] * 4);
    MD_HIP(hipMalloc(&t.pos_stage[s], padded.size() * m->esz * m->xm + 256));
    MD_HIP(hipMemcpy(tmp, padded.data(), padded.size() * 4, hipMemcpyHostToDevice));
    MD_TRY(launch_f32_to_rows(tmp, (long)padded.size(), t.pos_stage[s], m->prec, st, ld));
    MD_HIP(hipStreamSynchronize(st));
  }
  MD_HIP(hipFree(tmp));
  {
    std::vector<float> tab = build_pos_table_nhwc(F / 2, IH, IW, IW, IH, 0.1f);
    MD_HIP(hipMalloc((void**)&t.pos_final, tab.size() * 4));
    MD_HIP(hipMemcpy(t.pos_final, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  }
  if (c.dual_head) {
    // aux head input = neck + 0.1*UV + 0.1*UV (added twice, dpt.rs:428-435)
    std::vector<float> ta = build_pos_table_nhwc(F / 2, 8 * d->ph, 8 * d->pw, IW, IH, 0.1f);
    for (auto& x : ta) x = x + x;
    MD_HIP(hipMalloc((void**)&t.pos_aux, ta.size() * 4));
    MD_HIP(hipMemcpy(t.pos_aux, ta.data(), ta.size() * 4, hipMemcpyHostToDevice));
    std::vector<float> rc, rs;
    da3_rope_tables(d->ph, d->pw, c.rope_frequency, &rc, &rs);
    MD_HIP(hipMalloc((void**)&t.rope_cos, rc.size() * 4));
    MD_HIP(hipMalloc((void**)&t.rope_sin, rs.size() * 4));
    MD_HIP(hipMemcpy(t.rope_cos, rc.data(), rc.size() * 4, hipMemcpyHostToDevice));
    MD_HIP(hipMemcpy(t.rope_sin, rs.data(), rs.size() * 4, hipMemcpyHostToDevice));
  }
  if (d->ph != M || d->pw != M) {  // position embedding interpolated from the parameter's native grid
    std::vector<float> pos((size_t)(1 + M * M) * D);
    MD_HIP(hipMemcpy(pos.data(), d->pos_native, pos.size() * 4, hipMemcpyDeviceToHost));
    std::vector<float> ip = interpolate_pos_embed(pos, M, D, d->ph, d->pw);
    MD_HIP(hipMalloc((void**)&t.pos_used, ip.size() * 4));
    MD_HIP(hipMemcpy(t.pos_used, ip.data(), ip.size() * 4, hipMemcpyHostToDevice));
  }
  d->table_builds += 1;
  return MD_OK;
}

// Makes H x W the model's current input size: geometry, workspace plan (the arena grows when the new size needs more --
// never per call at a size seen before), and the size's tables from the cache (built on first use). A call at the current
// size returns at once.
static int da3_set_shape(md_model_s* m, int H, int W, bool force) {
  md_model_s::Da3State* d = m->da3;
  const ViTDims& v = d->cfg.vit;
  if (H <= 0 || W <= 0 || H % v.ps != 0 || W % v.ps != 0)  // mod.rs:509-520
    MD_FAIL(MD_ERR_SHAPE, "Input %dx%d must be divisible by patch size %d", H, W, v.ps);
  const auto key = std::make_pair(H, W);
  if (!force && H == d->ih && W == d->iw && d->tok_index) {
    d->shapes[key].last_use = ++d->use_clock;
    return MD_OK;
  }
  if ((long)(H / v.ps) * (W / v.ps) + 1 > 60000) MD_FAIL(MD_ERR_UNSUPPORTED, "input %dx%d: more than 60000 tokens", H, W);
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_HIP(hipDeviceSynchronize());  // nothing may still run on the plan that is about to be replaced
  const int oh = d->ih, ow = d->iw;
  da3_set_geometry(m, H, W);
  size_t need = 0;
  da3_plan(m, true, &need);
  if (need > m->ws.cap) {  // grow-only arena
    if (m->ws.base) (void)hipFree(m->ws.base);
    m->ws.base = nullptr;
    m->ws.cap = 0;
    if (hipMalloc((void**)&m->ws.base, need) != hipSuccess) {
      if (oh > 0) da3_set_geometry(m, oh, ow);
      d->tok_index = nullptr;  // forces a rebuild of the plan on the next call
      MD_FAIL(MD_ERR_OOM, "hipMalloc of %zu bytes for the %dx%d workspace failed (max_batch=%d)", need, H, W, d->cfg.max_batch);
    }
    m->ws.cap = need;
    m->alloc_count += 1;
    m->graphs.clear();
  }
  // padding rows / channels / keys must be finite zeros for every kernel: the buffers move with the plan, so the arena is
  // cleared whenever the plan changes (a few hundred MB at HBM speed, once per change of size)
  MD_HIP(hipMemset(m->ws.base, 0, m->ws.cap));
  m->ws.off = 0;
  MD_TRY(da3_plan(m, false, nullptr));
  auto it = d->shapes.find(key);
  if (it == d->shapes.end()) {
    if ((int)d->shapes.size() >= md_model_s::Da3State::kMaxShapes) {  // evict the least recently used size
      auto lru = d->shapes.begin();
      for (auto j = d->shapes.begin(); j != d->shapes.end(); ++j)
        if (j->second.last_use < lru->second.last_use) lru = j;
      da3_free_tables(lru->second);
      d->shapes.erase(lru);
      m->graphs.clear();
    }
    md_model_s::Da3State::ShapeTables t;
    const int st = da3_build_tables(m, t);
    if (st != MD_OK) {
      da3_free_tables(t);
      d->tok_index = nullptr;
      return st;
    }
    it = d->shapes.emplace(key, t).first;
  }
  md_model_s::Da3State::ShapeTables& t = it->second;
  t.last_use = ++d->use_clock;
  for (int s = 0; s < 4; ++s) d->pos_stage[s] = t.pos_stage[s];
  d->pos_final = t.pos_final;
  d->pos_aux = t.pos_aux;
  d->rope_cos = t.rope_cos;
  d->rope_sin = t.rope_sin;
  d->pos_used = t.pos_used;
  d->tok_index = &t.tok_index;
  d->vit.pos = t.pos_used ? t.pos_used : d->pos_native;
  MD_HIP(hipDeviceSynchronize());
  return MD_OK;
}

// the packs of the DPT head (behind the backbone's, vit_add_packs) ...
static void da3_add_packs(md_model_s* m) {
  const Da3Cfg& cfg = m->da3->cfg;
  const int F = cfg.features;
  const int* oc = cfg.out_channels;
  const std::string& hp = m->da3->hp;
  for (int s = 0; s < 4; ++s) add_pack(m, hp + ".projects." + std::to_string(s) + ".weight", PACK_NK, oc[s], m->da3->din, 1);
  add_pack(m, hp + ".resize_layers.0.conv_t.weight", PACK_DECONV, oc[0], oc[0], 4);
  add_pack(m, hp + ".resize_layers.1.conv_t.weight", PACK_DECONV, oc[1], oc[1], 2);
  add_pack(m, hp + ".resize_layers.3.conv.weight", PACK_CONV3, oc[3], oc[3], 3);
  for (int s = 0; s < 4; ++s) add_pack(m, hp + ".scratch.layer" + std::to_string(s + 1) + "_rn.weight", PACK_CONV3, F, oc[s], 3);
  for (const char* suffix : {"", "_aux"}) {
    if (suffix[0] && !cfg.dual_head) continue;
    for (int i = 1; i <= 4; ++i) {
      const std::string r = hp + ".scratch.refinenet" + std::to_string(i) + suffix;
      for (const char* u : {"residual1", "residual2"}) {
        add_pack(m, r + "." + u + ".conv1.weight", PACK_CONV3, F, F, 3);
        add_pack(m, r + "." + u + ".conv2.weight", PACK_CONV3, F, F, 3);
      }
      add_pack(m, r + ".out_conv.weight", PACK_NK, F, F, 1);
    }
  }
  add_pack(m, hp + ".scratch.output_conv1.weight", PACK_CONV3, F / 2, F, 3);
  add_pack(m, hp + ".scratch.output_conv2.conv1.weight", PACK_CONV3, 32, F / 2, 3);
  if (cfg.dual_head) {  // only the last aux level reaches the outputs (build_aux_logits, dpt.rs:405-440)
    const std::string lv = std::to_string(cfg.aux_levels - 1);
    int cin = F;
    for (int j = 0; j < cfg.aux_out1_conv_num; ++j) {
      const int cout = j % 2 == 0 ? F / 2 : F;
      add_pack(m, hp + ".scratch.output_conv1_aux." + lv + ".layers." + std::to_string(j) + ".weight", PACK_CONV3, cout, cin, 3);
      cin = cout;
    }
    add_pack(m, hp + ".scratch.output_conv2_aux." + lv + ".reduce.weight", PACK_CONV3, 32, F / 2, 3);
  }
}

// ... and the tables of everything behind the backbone (after the packed arena is placed)
static int da3_bind(md_model_s* m) {
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const std::string &hp = d->hp, sc = hp + ".scratch.", bp = "backbone.pretrained";
  Binder bd{m, {}};
  d->pos_native = bd.p32(bp + ".pos_embed");
  d->head_norm_g = bd.p32(hp + ".norm.gamma", c.dual_head);
  d->head_norm_b = bd.p32(hp + ".norm.beta", c.dual_head);
  d->camera_token = bd.p32(bp + ".camera_token", c.dual_head);
  for (int s = 0; s < 4; ++s) {
    d->proj[s] = bd.conv(hp + ".projects." + std::to_string(s));
    d->layer_rn[s] = bd.conv(sc + "layer" + std::to_string(s + 1) + "_rn", false);
  }
  d->resize[0] = bd.conv(hp + ".resize_layers.0.conv_t");
  d->resize[1] = bd.conv(hp + ".resize_layers.1.conv_t");
  d->resize[3] = bd.conv(hp + ".resize_layers.3.conv");
  for (int g = 0; g < (c.dual_head ? 2 : 1); ++g)
    for (int lvl = 0; lvl < 4; ++lvl) {
      const std::string r = sc + "refinenet" + std::to_string(lvl + 1) + (g ? "_aux" : "");
      if (lvl != 3) d->res[lvl][0][g] = {bd.conv(r + ".residual1.conv1"), bd.conv(r + ".residual1.conv2")};
      d->res[lvl][1][g] = {bd.conv(r + ".residual2.conv1"), bd.conv(r + ".residual2.conv2")};
      d->out_conv[lvl][g] = bd.conv(r + ".out_conv");
    }
  d->oc1 = bd.conv(sc + "output_conv1");
  d->oc2_1 = bd.conv(sc + "output_conv2.conv1");
  d->oc2_2 = {bd.p32(sc + "output_conv2.conv2.weight"), bd.p32(sc + "output_conv2.conv2.bias")};
  if (c.dual_head) {
    const std::string lv = std::to_string(c.aux_levels - 1), oh = sc + "output_conv2_aux." + lv;
    for (int j = 0; j < c.aux_out1_conv_num; ++j) d->aux_neck.push_back(bd.conv(sc + "output_conv1_aux." + lv + ".layers." + std::to_string(j)));
    d->aux_reduce = bd.conv(oh + ".reduce");
    d->aux_project = {bd.p32(oh + ".project.weight"), bd.p32(oh + ".project.bias")};
    auto cw = [&](const char* n) { return bd.p32(std::string("camera_decoder.") + n); };
    CamDecW& w = d->cam_dec;
    w.w1 = cw("backbone_1.weight"); w.b1 = cw("backbone_1.bias"); w.w2 = cw("backbone_2.weight"); w.b2 = cw("backbone_2.bias");
    w.wt = cw("fc_t.weight"); w.bt = cw("fc_t.bias"); w.wq = cw("fc_qvec.weight"); w.bq = cw("fc_qvec.bias");
    w.wf = cw("fc_fov.weight"); w.bf = cw("fc_fov.bias");
  }
  if (c.camera_encoder) {  // optional here: da3_camera_encoder reports what is missing when it runs
    auto ce = [&](const std::string& n) { return bd.p32("camera_encoder." + n, false); };
    CamEncW& w = d->cam_enc;
    w.fc1_w = ce("pose_branch.fc1.weight"); w.fc1_b = ce("pose_branch.fc1.bias");
    w.fc2_w = ce("pose_branch.fc2.weight"); w.fc2_b = ce("pose_branch.fc2.bias");
    w.tn_g = ce("token_norm.gamma"); w.tn_b = ce("token_norm.beta");
    w.on_g = ce("trunk_norm.gamma"); w.on_b = ce("trunk_norm.beta");
    w.depth = c.cam_trunk_depth;
    for (int i = 0; i < std::min(w.depth, (int)CamEncW::kMaxDepth); ++i) {
      const std::string bk = "trunk." + std::to_string(i) + ".";
      CamEncW::Blk& k = w.blk[i];
      k.n1g = ce(bk + "norm1.gamma"); k.n1b = ce(bk + "norm1.beta"); k.n2g = ce(bk + "norm2.gamma"); k.n2b = ce(bk + "norm2.beta");
      k.qkv_w = ce(bk + "attn.qkv.weight"); k.qkv_b = ce(bk + "attn.qkv.bias");
      k.proj_w = ce(bk + "attn.proj.weight"); k.proj_b = ce(bk + "attn.proj.bias"); k.ls1 = ce(bk + "ls1.gamma");
      k.fc1_w = ce(bk + "mlp.fc1.weight"); k.fc1_b = ce(bk + "mlp.fc1.bias");
      k.fc2_w = ce(bk + "mlp.fc2.weight"); k.fc2_b = ce(bk + "mlp.fc2.bias"); k.ls2 = ce(bk + "ls2.gamma");
    }
  }
  return bd.status();
}

int da3_create(md_device_t dev, const Da3Cfg& cfg, md_model_t* out) {
  if (!dev || !out) MD_FAIL(MD_ERR_INVALID_ARG, "device/model pointer is null");
  const ViTDims& v = cfg.vit;
  if (v.D != v.heads * 64 || v.D % 64 != 0 || v.D > 1024) MD_FAIL(MD_ERR_UNSUPPORTED, "ViT width %d / heads %d unsupported", v.D, v.heads);
  const int img_h = cfg.image_size, img_w = cfg.image_width > 0 ? cfg.image_width : cfg.image_size;
  if (img_h % v.ps != 0 || img_w % v.ps != 0 || img_h <= 0 || img_w <= 0)  // mod.rs:509-520
    MD_FAIL(MD_ERR_SHAPE, "Input %dx%d must be divisible by patch size %d", img_h, img_w, v.ps);
  if (cfg.features % 64 != 0 || cfg.output_dim != (cfg.dual_head ? 2 : 1))
    MD_FAIL(MD_ERR_UNSUPPORTED, "head features %d / output_dim %d unsupported", cfg.features, cfg.output_dim);
  for (int s = 0; s < 4; ++s)
    if (cfg.out_channels[s] % 4 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "head out_channels must be multiples of 4");
  if (cfg.dual_head && (cfg.ext_block_start < 0 || cfg.ext_block_start >= v.depth))
    MD_FAIL(MD_ERR_INVALID_ARG, "dual head needs the extended backbone (ext_block_start %d)", cfg.ext_block_start);
  MD_HIP(hipSetDevice(dev->ordinal));
  md_model_s* m = new md_model_s();
  m->dev = dev;
  m->kind = 1;
  // MD_PREC_FP8 is bf16 everywhere except the four ViT linear layers (e4m3 operands)
  const bool fp8 = cfg.precision == MD_PREC_FP8;
  if (fp8 && v.D % 128 != 0) MD_FAIL(MD_ERR_UNSUPPORTED, "fp8 operands need a ViT width that is a multiple of 128 (got %d)", v.D);
  m->prec = fp8 ? MD_PREC_BF16 : cfg.precision;
  m->esz = m->prec == MD_PREC_F32 ? 4 : 2;
  m->ke = 128 / m->esz;
  m->xm = m->prec == MD_PREC_F16X2 ? 2 : 1;  // split-half operands: activation rows are [hi | lo]
  m->wterms = m->xm == 2 ? 3 : 1;            // decided by model_commit: 2 when every plain weight is an exact half (an f16 record)
  m->cfg.max_batch = cfg.max_batch;
  m->cfg.precision = m->prec;
  m->da3 = new md_model_s::Da3State();
  md_model_s::Da3State* d = m->da3;
  d->cfg = cfg;
  d->cfg.precision = m->prec;
  d->fp8 = fp8;
  d->hp = cfg.dual_head ? "head_dual" : "head_mono";
  d->din = cfg.dual_head ? 2 * v.D : v.D;
  d->native_grid = v.img / v.ps;  // the pos_embed parameter's grid (37 for ViT-L/14 @ 518)
  da3_set_geometry(m, img_h, img_w);
  m->S = cfg.image_size;
  auto fail = [&](int code) {
    model_destroy(m);
    return code;
  };
  int st = alloc_param_arena(m, da3_param_specs(cfg, MD_INIT_REFERENCE));
  if (st != MD_OK) return fail(st);
  const int D = v.D;
  const std::string bp = "backbone.pretrained";
  vit_add_packs(m, bp, v);
  da3_add_packs(m);
  if ((st = place_packs(m)) != MD_OK) return fail(st);
  VitW& w = d->vit;
  vit_bind(m, bp, v.depth, w);
  for (int i = 0; i < v.depth; ++i)  // the extended backbone alternates local and global blocks from ext_block_start on
    w.blk[i].global = cfg.dual_head && i >= cfg.ext_block_start && i % 2 == 1;
  if ((st = da3_bind(m)) != MD_OK) return fail(st);
  if (fp8) {
    const size_t per_block = (size_t)12 * D * D + (size_t)(3 * D + D + 4 * D + D) * 4 + 8 * 256;
    if (hipMalloc((void**)&d->w8_base, per_block * v.depth) != hipSuccess) {
      set_error("hipMalloc of %zu bytes for the fp8 weights failed", per_block * v.depth);
      return fail(MD_ERR_OOM);
    }
    (void)hipMemset(d->w8_base, 0, per_block * v.depth);
    char* q = d->w8_base;
    const int nn[4] = {3 * D, D, 4 * D, D}, kk[4] = {D, D, D, 4 * D};
    for (VitBlockW& k : w.blk)
      for (int j = 0; j < 4; ++j) {
        k.w8[j] = q;
        q += align_up((size_t)nn[j] * kk[j], 256);
        k.s8[j] = (float*)q;
        q += align_up((size_t)nn[j] * 4, 256);
      }
  }

  if (hipMalloc(&m->zero_page, 4096) != hipSuccess) return fail(MD_ERR_OOM);
  (void)hipMemset(m->zero_page, 0, 4096);
  // workspace for the configured size + its tables (PosEmbedCache, dpt.rs:784-833: built once per shape); other sizes get
  // theirs on their first infer call (da3_set_shape)
  d->ih = 0;
  d->iw = 0;
  if ((st = da3_set_shape(m, img_h, img_w, true)) != MD_OK) return fail(st);
  m->alloc_count = 0;  // count what the infer calls allocate, not the construction
  (void)hipDeviceSynchronize();
  *out = m;
  return MD_OK;
}

void da3_frame_info(md_model_t m, int* patch, int* cur_h, int* cur_w) {
  *patch = m->da3->cfg.vit.ps;
  *cur_h = m->da3->tok_index ? m->da3->ih : 0;
  *cur_w = m->da3->tok_index ? m->da3->iw : 0;
}

const Da3Cfg& da3_cfg(md_model_t m) { return m->da3->cfg; }
long da3_shape_builds(md_model_t m) { return (m && m->da3) ? m->da3->table_builds : 0; }

void da3_destroy_state(md_model_t m) {
  if (m && m->da3 && m->da3->w8_base) (void)hipFree(m->da3->w8_base);
  if (!m || !m->da3) return;
  for (auto& kv : m->da3->shapes) da3_free_tables(kv.second);
  m->da3->shapes.clear();
  delete m->da3;
  m->da3 = nullptr;
}

static int da3_tok_index(md_model_s* m, int B, int** out) {
  md_model_s::Da3State* d = m->da3;
  auto it = d->tok_index->find(B);
  if (it != d->tok_index->end()) {
    *out = it->second;
    return MD_OK;
  }
  std::vector<int> h((size_t)B * d->P);
  token_index_table(B, d->P, d->SS, 0, h.data());
  int* dev = nullptr;
  MD_HIP(hipMalloc((void**)&dev, h.size() * 4));
  MD_HIP(hipMemcpy(dev, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  (*d->tok_index)[B] = dev;
  m->alloc_count += 1;
  *out = dev;
  return MD_OK;
}

static int da3_infer_eager(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const Da3Outputs& outp, int out_kind,
                           hipStream_t stream);

// what a multi-view call (Da3Outputs::views > 1) asks of the model; checked before anything is launched or captured
static int da3_check_views(md_model_t m, int B, const Da3Outputs& outp) {
  const md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  if (outp.views == 1) return MD_OK;
  if (outp.views < 1 || B % outp.views != 0) MD_FAIL(MD_ERR_SHAPE, "%d images in scenes of %d views", B, outp.views);
  if (B > c.max_batch) MD_FAIL(MD_ERR_SHAPE, "%d scenes of %d views exceed max_batch %d", B / outp.views, outp.views, c.max_batch);
  if (!c.dual_head) MD_FAIL(MD_ERR_UNSUPPORTED, "multi-view inference needs the extended backbone's global blocks (the mono head has none)");
  if (outp.tokens[0]) MD_FAIL(MD_ERR_UNSUPPORTED, "multi-view inference runs the backbone; infer_from_tokens has none");
  if (outp.cam_extrinsics || outp.cam_intrinsics)
    MD_FAIL(MD_ERR_UNSUPPORTED, "multi-view inference with caller cameras: the camera encoder yields one token per image, not per view");
  if (m->prec == MD_PREC_F32 || d->fp8) MD_FAIL(MD_ERR_UNSUPPORTED, "multi-view inference runs in the bf16, f16 and f16x2 modes");
  return MD_OK;
}

int da3_infer_ex(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const Da3Outputs& outp, int out_kind,
                 hipStream_t stream) {
  if (!m || m->kind != 1 || !m->da3) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth-Anything-v3 model");
  MD_TRY(da3_check_views(m, B, outp));
  auto body = [&]() { return da3_infer_eager(m, nchw, B, H, W, in_kind, outp, out_kind, stream); };
  if (!m->graph_enabled) return body();
  MD_HIP(hipSetDevice(m->dev->ordinal));
  hipStream_t st = model_stream(m, stream);
  const bool eligible = nchw && !outp.tokens[0] && outp.depth && !outp.raw_logits && in_kind == MD_MEM_DEVICE && out_kind == MD_MEM_DEVICE && m->committed && B > 0 &&
                        B <= m->da3->cfg.max_batch && H == m->da3->ih && W == m->da3->iw;
  const std::vector<uintptr_t> key = {(uintptr_t)st, (uintptr_t)B, (uintptr_t)H, (uintptr_t)W, (uintptr_t)nchw, (uintptr_t)outp.depth,
                                      (uintptr_t)outp.depth_confidence, (uintptr_t)outp.aux, (uintptr_t)outp.aux_confidence,
                                      (uintptr_t)outp.pose_encoding, (uintptr_t)outp.extrinsics, (uintptr_t)outp.intrinsics,
                                      (uintptr_t)outp.cam_extrinsics, (uintptr_t)outp.cam_intrinsics, (uintptr_t)outp.cam_views,
                                      (uintptr_t)outp.views};
  return run_with_graph(m, st, key, eligible, body);
}

// ---- the stages of one call (da3_infer_eager) ----
// what the stages share of one call
struct Da3Call {
  const Da3Outputs& outp;
  int in_kind, out_kind, H, W;
  bool want_aux, want_cam;
  int G;                           // pyramid weight groups: 2 = main | aux in the same launches (want_aux)
  int sh[4], sw[4];                // prepare_stage sizes (rows, columns)
  const float* cam_tok = nullptr;  // the camera encoder's tokens [B, D] (null: the learned reference-view token)
  float* depth_dev = nullptr;      // device home of `depth` (infer_raw: of `raw_logits`)
  const void* c1_map = nullptr;    // output_conv1's result
  const void* aux_cur = nullptr;   // want_aux: the aux neck's first map
};

static int host_out(hipStream_t st, int out_kind, float* dst, const float* src, size_t n) {
  if (out_kind == MD_MEM_HOST && dst) MD_HIP(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToHost, st));
  return MD_OK;
}

// fused tail: out_c[img][pixel] = act_c(w_c . relu(conv3x3(in) + b1) + b_c) for `nch` channels in ONE launch over a
// [B, hh, ww, 64-padded] map (ConvStack / `reduce` + `project`, dpt.rs:481-513,1287-1290)
struct TailCh { const float* w; float b; int act; float* out; long bstride; };
static int tail(Run& r, const char* name, const void* in, int hh, int ww, const ConvW& w1, const TailCh* chs, int nch) {
  if (nch <= 0) return MD_OK;
  md_model_s* m = r.m;
  GemmParams p;
  p.N = 32; p.ngroups = 1; p.g_rows[0] = r.B * hh * ww; p.W[0] = w1.w;
  p.A = in; p.cH = hh; p.cW = ww; p.zero_page = m->zero_page;
  split_conv_a(m, p, cpad(m, m->da3->cfg.features / 2), 0);
  p.epi = EPI_HEAD; p.bias[0] = w1.b; p.head_nch = nch; p.head_plane = hh * ww;
  for (int i = 0; i < nch; ++i) {
    p.head_wc[i] = chs[i].w; p.head_bs[i] = chs[i].b; p.head_acts[i] = chs[i].act; p.head_out[i] = chs[i].out; p.head_bstride[i] = chs[i].bstride;
  }
  r.begin(name);
  int s = launch_gemm(p, A_CONV3, m->prec, TILE_256x32, r.st);
  r.end();
  return s;
}

// `infer_from_tokens` (mod.rs:405-469): no backbone, no camera prediction; the head's token LayerNorm (mono: non-affine,
// dpt.rs:761-766; dual: the affine `norm`, dpt.rs:308) on the caller's hook tokens, patch rows only
static int da3_stage_tokens(Run& r, const Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const Da3Outputs& outp = k.outp;
  const int B = r.B, SS = d->SS, P = d->P, din = d->din;
  if (outp.pose_encoding || outp.extrinsics || outp.intrinsics)
    MD_FAIL(MD_ERR_UNSUPPORTED, "infer_from_tokens has no camera prediction (finalize_inference(head_output, None), mod.rs:468)");
  const int T = outp.tokens_per_image;
  if (T != P && T != P + 1)  // mod.rs:419-424: tokens == expected -> patch_start 0, else patch_token_start = 1
    MD_FAIL(MD_ERR_SHAPE, "%d tokens per image for a %dx%d input: expected %d patch rows (or %d with a leading cls row)", T, k.H, k.W, P, P + 1);
  for (int hk = 0; hk < 4; ++hk)
    if (!outp.tokens[hk]) MD_FAIL(MD_ERR_LEVELS, "Backbone returned fewer hooks (%d) than requested (4)", hk);
  const int start = T == P ? 0 : 1;
  const size_t need = ((size_t)c.max_batch * SS + 64) * din;
  bool grown = false;
  MD_TRY(grow(m, r.st, d->tok_stage, need * 4, &grown));
  if (grown) MD_HIP(hipMemset(d->tok_stage.p, 0, need * 4));
  SeqGroups tg;
  memset(&tg, 0, sizeof(tg));
  tg.ngroups = 1;
  tg.nseq[0] = B;
  tg.a[0] = c.dual_head ? d->head_norm_g : nullptr;
  tg.b[0] = c.dual_head ? d->head_norm_b : nullptr;
  const hipMemcpyKind kind = k.in_kind == MD_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  for (int hk = 0; hk < 4; ++hk) {
    for (int b = 0; b < B; ++b)  // patch rows of image b -> rows b*SS + 1 .. of the staging tensor (the layout the head gathers from)
      MD_HIP(hipMemcpyAsync(d->tok_stage.p + ((size_t)b * SS + 1) * din, outp.tokens[hk] + ((size_t)b * T + start) * din, (size_t)P * din * 4,
                            kind, r.st));
    r.begin("layernorm");
    MD_TRY(launch_layernorm(d->tok_stage.p, d->hookn[hk], (long)B * SS, din, 1e-5f, SS, tg, m->prec, 0, r.st));
    r.end();
    if (m->taps_enabled) MD_TRY(r.tap_token_rows(("backbone_tokens_" + std::to_string(hk)).c_str(), d->tok_stage.p, SS, 1, P, din, din, 0));
  }
  return MD_OK;
}

// camera encoder (`infer_with_camera`, mod.rs:522-527): the known cameras -> one token per image (k.cam_tok)
static int da3_camera_encoder(Run& r, Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const Da3Outputs& outp = k.outp;
  const int B = r.B, V = outp.cam_views, D = c.vit.D;
  if (V < 1 || V > MD_CAM_MAX_VIEWS) MD_FAIL(MD_ERR_SHAPE, "camera inputs with %d views (1..%d supported)", V, MD_CAM_MAX_VIEWS);
  const size_t n_in = (size_t)B * V * 21, n_tok = align_up((size_t)B * D, 64);
  const size_t need = align_up(n_in, 64) + n_tok + camera_encoder_scratch_floats(B, V, D);
  MD_TRY(grow(m, r.st, d->cam_enc_ws, need * 4));
  const float *e_dev = outp.cam_extrinsics, *k_dev = outp.cam_intrinsics;
  if (k.in_kind == MD_MEM_HOST) {
    MD_HIP(hipMemcpyAsync(d->cam_enc_ws.p, outp.cam_extrinsics, (size_t)B * V * 12 * 4, hipMemcpyHostToDevice, r.st));
    MD_HIP(hipMemcpyAsync(d->cam_enc_ws.p + (size_t)B * V * 12, outp.cam_intrinsics, (size_t)B * V * 9 * 4, hipMemcpyHostToDevice, r.st));
    e_dev = d->cam_enc_ws.p; k_dev = d->cam_enc_ws.p + (size_t)B * V * 12;
  }
  float* cam_tok = d->cam_enc_ws.p + align_up(n_in, 64);
  const CamEncW& w = d->cam_enc;
  if (w.depth > CamEncW::kMaxDepth) MD_FAIL(MD_ERR_UNSUPPORTED, "camera encoder trunk of %d blocks", w.depth);
  for (int i = 0; i < w.depth; ++i)
    if (!w.blk[i].qkv_w || !w.blk[i].ls2) MD_FAIL(MD_ERR_FORMAT, "camera encoder block %d is not in the inventory", i);
  if (!w.fc1_w || !w.on_b) MD_FAIL(MD_ERR_FORMAT, "camera encoder is not in the inventory");
  r.begin("camera_encoder");
  MD_TRY(launch_camera_encoder(e_dev, k_dev, B, V, D, c.cam_heads, k.H, k.W, c.cam_ln_eps, c.ln_eps, w, cam_tok + n_tok, cam_tok, r.st));
  r.end();
  MD_TRY(r.tap_f32("camera_token", cam_tok, B, D, 0, 0));  // CameraEncoder::forward's result (camera.rs:89-110)
  k.cam_tok = cam_tok;
  return MD_OK;
}

// the backbone: patchify, patch embedding, the blocks and their hooks (d->hookn)
static int da3_backbone(Run& r, const Da3Call& k, const float* x_dev) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const ViTDims& v = c.vit;
  const int B = r.B, D = v.D, SS = d->SS, NT = d->NT, P = d->P;
  r.begin("patchify");  // + the cls rows (cls + pos[0]) and the zero padding rows of the residual stream, in the same launch
  MD_TRY(launch_patchify(x_dev, B, k.H, k.W, v.ps, d->Kp, d->patches, m->prec, r.st, d->xres, SS, NT, D, d->vit.cls, d->vit.pos));
  r.end();
  SeqGroups sg;
  memset(&sg, 0, sizeof(sg));
  sg.ngroups = 1;
  sg.nseq[0] = B;
  {
    GemmParams p;
    p.N = D; p.ngroups = 1; p.g_rows[0] = B * P; p.W[0] = d->vit.pe_w; p.bias[0] = d->vit.pe_b; p.pos[0] = d->vit.pos;
    p.A = d->patches;
    split_dense_a(m, p, d->Kp, d->Kp, 0);
    p.epi = EPI_PATCH_EMBED; p.out = d->xres; p.ldo = D; p.seq_stride = SS; p.seq_patches = P; p.embed = D;
    r.begin("patch_embed");
    MD_TRY(launch_gemm(p, A_DENSE, m->prec, TILE_AUTO, r.st));
    r.end();
  }
  const long rows = (long)B * SS;
  int hook_slot = 0;
  // The residual stream lives in `vp.x`. A GLOBAL block of the extended backbone needs the state behind the last LOCAL block
  // for its hook (cat(x_local, LayerNorm(x))): its output projection therefore writes x + ls * (...) into the other buffer
  // (GemmParams::resid_src) and the two swap -- the copy of the whole stream that used to precede every global block is gone.
  VitPlan vp;
  vp.vit[0] = &d->vit; vp.gcnt[0] = B; vp.WS = B;
  vp.D = D; vp.heads = v.heads; vp.SS = SS; vp.NT = NT; vp.kpad = d->kpad; vp.ln_eps = c.ln_eps;
  vp.x = d->xres; vp.xalt = d->xlocal; vp.xn = d->xn; vp.qk = d->qk; vp.vT = d->vT; vp.ao = d->ao; vp.hbuf = d->hbuf; vp.scores = d->scores;
  vp.lin_prec = d->fp8 ? MD_PREC_FP8 : m->prec;
  if (d->fp8) { vp.a_scale = md_model_s::Da3State::kActScale; vp.h_scale = md_model_s::Da3State::kHidScale; }
  vp.qk_norm_eps = c.qk_norm_eps; vp.rope_cos = d->rope_cos; vp.rope_sin = d->rope_sin; vp.rope_pw = d->pw;
  // entering block ext_block_start the camera token takes the cls slot -- the encoder's (mod.rs:522-531) or the learned
  // reference-view one
  vp.tok0_block = c.dual_head ? c.ext_block_start : -1;
  vp.tok0 = k.cam_tok ? k.cam_tok : d->camera_token;
  vp.tok0_stride = k.cam_tok ? D : 0;
  if (k.outp.views > 1) {
    // B / views scenes of `views` views: the global blocks attend across a scene, and the learned camera token [1, 2, D] gives slot 0
    // to view 0 of every scene and slot 1 to the other views -- laid out per sequence in view_tok
    vp.views = k.outp.views;
    r.begin("view_tokens");
    MD_TRY(launch_set_token0(d->view_tok, B, 1, D, d->camera_token + D, r.st, 0));
    MD_TRY(launch_set_token0(d->view_tok, B / vp.views, vp.views, D, d->camera_token, r.st, 0));
    r.end();
    vp.tok0 = d->view_tok;
    vp.tok0_stride = D;
  }
  for (int i = 0; i < v.depth; ++i) {
    MD_TRY(run_vit_block(r, vp, i));
    const float* xcur = vp.x;
    const float* xl = d->vit.blk[i].global ? vp.xalt : xcur;  // a local block is its own "last local" state; behind a global block the other buffer holds it
    for (int hk = 0; hk < 4; ++hk) {  // a block may feed several hooks
      if (c.hook_ids[hk] != i) continue;
      const std::string tn = "backbone_tokens_" + std::to_string(hk);  // DepthTrace::backbone_tokens (mod.rs:241-246,344-347)
      if (c.dual_head) {
        // hooks = LayerNorm_head(cat(x after the last local block, LayerNorm_final(x))); the camera feature is
        // token 0 of the raw concat at the last hook
        r.begin("hook_cat_ln");
        MD_TRY(launch_hook_cat_ln(xl, xcur, rows, SS, NT, D, d->vit.norm_g, d->vit.norm_b, c.ln_eps, d->head_norm_g,
                                  d->head_norm_b, 1e-5f, d->hookn[hk], hk == 3 ? d->cam_raw : nullptr, m->prec, r.st));
        r.end();
        if (m->taps_enabled) {  // cat(x_local, LayerNorm_final(x)) patch rows
          sg.a[0] = d->vit.norm_g; sg.b[0] = d->vit.norm_b;
          MD_TRY(launch_layernorm(xcur, d->lnf, rows, D, c.ln_eps, SS, sg, m->prec, 1, r.st));
          MD_TRY(r.tap_token_rows(tn.c_str(), xl, SS, 1, P, D, 2 * D, 0));
          MD_TRY(r.tap_token_rows(tn.c_str(), d->lnf, SS, 1, P, D, 2 * D, D));
        }
      } else {
        // hooks (mod.rs:202-215): final LayerNorm of the block output, then the head's non-affine token
        // norm (apply_token_norm, dpt.rs:761-766: biased variance, eps 1e-5)
        sg.a[0] = d->vit.norm_g; sg.b[0] = d->vit.norm_b;
        r.begin("layernorm");
        MD_TRY(launch_layernorm(xcur, d->lnf, rows, D, c.ln_eps, SS, sg, m->prec, 1, r.st));
        r.end();
        if (m->taps_enabled) MD_TRY(r.tap_token_rows(tn.c_str(), d->lnf, SS, 1, P, D, D, 0));
        sg.a[0] = nullptr; sg.b[0] = nullptr;
        r.begin("layernorm");
        MD_TRY(launch_layernorm(d->lnf, d->hookn[hk], rows, D, 1e-5f, SS, sg, m->prec, 0, r.st));
        r.end();
      }
      ++hook_slot;
    }
  }
  if (hook_slot < 4) MD_FAIL(MD_ERR_LEVELS, "Backbone returned fewer hooks (%d) than requested (4)", hook_slot);  // mod.rs:532-537
  return MD_OK;
}

// DPT head: prepare_stage (dpt.rs:282-317 / 649-689) -> the layerN_rn maps (d->rn, d->rnr)
static int da3_prepare_stages(Run& r, const Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const int B = r.B, P = d->P, ph = d->ph, pw = d->pw, F = c.features, Fp = cpad(m, F);
  const int* oc = c.out_channels;
  int* tok_idx = nullptr;
  MD_TRY(da3_tok_index(m, B, &tok_idx));
  for (int s = 0; s < 4; ++s) {
    const int ocp = cpad(m, oc[s]);
    {  // 1x1 projection over gathered patch tokens + 0.1 * UV position table
      const GemmParams p = rows_params(geom_of(m), d->hookn[s], d->din, tok_idx, (long)B * P, d->proj[s].w, oc[s], d->din, d->proj[s].b,
                                       d->sp[s], ocp, 0, ACT_NONE, 0, d->pos_stage[s], P);
      r.begin("head_proj");
      MD_TRY(launch_gemm(p, A_INDEXED, m->prec, TILE_AUTO, r.st));
      r.end();
    }
    const void* feat = d->sp[s];
    if (s == 0 || s == 1) {  // ConvTranspose k4s4 / k2s2 (+bias)
      MD_TRY(deconv2(r, "head_deconv", d->sp[s], ocp, nullptr, ph, pw, d->resize[s].w, ocp, oc[s], d->resize[s].b, d->sr[s], ocp, 0, nullptr,
                     s == 0 ? 4 : 2));
      feat = d->sr[s];
    } else if (s == 3) {  // Conv2d 3x3 stride 2 pad 1 (+bias)
      GemmParams p;
      p.N = oc[3]; p.ngroups = 1; p.g_rows[0] = B * d->h3h * d->h3w;
      p.W[0] = d->resize[3].w; p.bias[0] = d->resize[3].b;
      p.A = d->sp[3]; p.cH = ph; p.cW = pw; p.cOH = d->h3h; p.cOW = d->h3w; p.cstride = 2; p.zero_page = m->zero_page;
      split_conv_a(m, p, ocp, 0);
      p.epi = EPI_STORE; p.out = d->sr[3];
      split_out(m, p, ocp, true);
      r.begin("head_conv_s2");
      MD_TRY(launch_gemm(p, A_CONV3, m->prec, TILE_AUTO, r.st));
      r.end();
      feat = d->sr[3];
    }
    // layerN_rn: 3x3, no bias -> features (+ relu copy for the residual units)
    MD_TRY(conv3(r, "head_conv3x3", feat, k.sh[s], k.sw[s], ocp, &d->layer_rn[s], F, d->rn[s], Fp, ACT_NONE, nullptr, nullptr, d->rnr[s]));
    if (m->taps_enabled) {  // prepare_stage output and its layerN_rn map (dpt.rs:649-703)
      MD_TRY(r.tap_nhwc(("stage_" + std::to_string(s)).c_str(), feat, oc[s], k.sh[s], k.sw[s], ocp));
      MD_TRY(r.tap_nhwc(("layer" + std::to_string(s + 1) + "_rn").c_str(), d->rn[s], F, k.sh[s], k.sw[s], Fp));
    }
  }
  return MD_OK;
}

// the four FeatureFusionBlocks (dpt.rs:1206-1222) from the coarsest stage up, then output_conv1 (dpt.rs:337-344). Dual head: the main
// fusion pyramid (depth, confidence) and the aux fusion pyramid (rays, confidence) have the same shapes and share their inputs (the
// layerN_rn maps): with the aux outputs wanted they run in the SAME launches as two weight groups -- group 0 = main on images [0, B),
// group 1 = aux on images [B, 2B) of every pyramid map. A 64-feature 3x3 convolution costs ~11 us at 37^2 and ~14 us at 296^2
// (launch floor + nine dependent k-tiles, not throughput), so the second group is nearly free where a second chain of launches was
// not (round 4: 44 -> 22 pyramid launches; the side-stream form overlapped only a third of the aux pyramid,
// profiles/r04_cfg2_branches.txt).
static int da3_pyramid(Run& r, Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const int B = r.B, G = k.G, ph = d->ph, pw = d->pw, F = d->cfg.features, Fp = cpad(m, F), F2p = cpad(m, F / 2);
  const size_t px_bytes = (size_t)Fp * m->esz * m->xm;  // one pixel of an F-channel map
  const int target[4] = {8 * ph, 4 * ph, 2 * ph, ph}, targw[4] = {8 * pw, 4 * pw, 2 * pw, pw};  // output size of refinenet1..4
  const void* top = nullptr;
  for (int lvl = 3; lvl >= 0; --lvl) {
    const void *yx = d->rn[3], *yxr = d->rnr[3];
    if (lvl != 3) {
      MD_TRY(residual_unit(r, "head_conv3x3", d->res[lvl][0], G, k.sh[lvl], k.sw[lvl], Fp, F, d->rn[lvl], d->rnr[lvl], true, top, d->t, d->x, d->xr));
      yx = d->x; yxr = d->xr;
    }
    MD_TRY(residual_unit(r, "head_conv3x3", d->res[lvl][1], G, k.sh[lvl], k.sw[lvl], Fp, F, yx, yxr, lvl == 3, nullptr, d->t, d->y, nullptr));
    r.begin("head_resize");
    MD_TRY(launch_resize_nhwc(d->y, G * B, k.sh[lvl], k.sw[lvl], F, Fp, d->up, target[lvl], targw[lvl], Fp, MD_INTERP_BURN, nullptr, m->prec, r.st));
    r.end();
    {  // out_conv 1x1 (+bias), one weight set per group
      GemmParams p;
      const int M2 = B * target[lvl] * targw[lvl];
      p.N = F; p.ngroups = G;
      for (int g = 0; g < G; ++g) {
        p.g_rows[g] = M2; p.g_row0[g] = g * M2; p.g_arow0[g] = g * M2;
        p.W[g] = d->out_conv[lvl][g].w; p.bias[g] = d->out_conv[lvl][g].b;
      }
      p.A = d->up;
      split_dense_a(m, p, Fp, Fp, 0);
      p.epi = EPI_STORE; p.out = d->o;
      split_out(m, p, Fp, true);
      r.begin("head_out_conv");
      MD_TRY(launch_gemm(p, A_DENSE, m->prec, TILE_AUTO, r.st));
      r.end();
    }
    top = d->o;
    if (m->taps_enabled)  // FeatureFusionBlock outputs (dpt.rs:705-720), main and aux pyramids
      for (int g = 0; g < G; ++g)
        MD_TRY(r.tap_nhwc(("refinenet" + std::to_string(lvl + 1) + (g ? "_aux" : "")).c_str(),
                          (const char*)d->o + (size_t)g * B * target[lvl] * targw[lvl] * px_bytes, F, target[lvl], targw[lvl], Fp));
  }
  // output_conv1 and the first convolution of the aux neck (dpt.rs:1085-1113) are both 3x3 F -> F/2 on the 8ph x 8pw results of their
  // pyramids: one launch, two weight groups, into the (now free) `up` map -- main | aux
  const ConvW c1w[2] = {d->oc1, k.want_aux ? d->aux_neck[0] : ConvW{}};
  void* c1 = k.want_aux ? d->up : d->c1;
  MD_TRY(conv3(r, "head_conv3x3", d->o, 8 * ph, 8 * pw, Fp, c1w, F / 2, c1, F2p, ACT_NONE, nullptr, nullptr, nullptr, 0, G));
  k.c1_map = c1;
  if (k.want_aux) k.aux_cur = (const char*)c1 + (size_t)B * 64 * ph * pw * F2p * m->esz * m->xm;
  return MD_OK;
}

// aux branch (build_aux_logits, dpt.rs:356-441): the last level's 5-conv neck (its first convolution ran in da3_pyramid) -> + 2 x 0.1 x
// UV -> reduce 3x3 -> ReLU -> project 1x1 (7 ch: 6 ray values + confidence)
static int da3_aux_tail(Run& r, const Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const Da3Outputs& outp = k.outp;
  const int B = r.B, F = c.features, F2 = F / 2, F2p = cpad(m, F2), ah = 8 * d->ph, aw = 8 * d->pw;
  const void* cur = k.aux_cur;
  void* pp[2] = {d->up2, d->o2};
  int cin = F2;
  for (int j = 1; j < c.aux_out1_conv_num; ++j) {
    const int cout = j % 2 == 0 ? F / 2 : F;
    MD_TRY(conv3(r, "aux_conv3x3", cur, ah, aw, cpad(m, cin), &d->aux_neck[j], cout, pp[j & 1], cpad(m, cout), ACT_NONE, nullptr, nullptr, nullptr));
    cur = pp[j & 1];
    cin = cout;
  }
  void* hin = cur == d->up2 ? d->o2 : d->up2;
  r.begin("head_resize");
  MD_TRY(launch_resize_nhwc(cur, B, ah, aw, F2, F2p, hin, ah, aw, F2p, MD_INTERP_BURN, d->pos_aux, m->prec, r.st));
  r.end();
  if (m->taps_enabled) {  // DepthTrace::aux_stage_necks (last level) / aux_head_input (mod.rs:241-246)
    MD_TRY(r.tap_nhwc("aux_neck", cur, F2, ah, aw, F2p));
    MD_TRY(r.tap_nhwc("aux_head_input", hin, F2, ah, aw, F2p));
  }
  const size_t plane = (size_t)ah * aw;
  const int K7 = c.aux_output_dim;
  TailCh chs[8];
  int nch = 0;
  for (int ch = 0; ch < K7; ++ch) {  // aux lands as [B, 6, h, w], the confidence as [B, h, w]; host outputs through [B, 7, h, w] staging
    const bool conf = ch == K7 - 1;
    float* user = conf ? outp.aux_confidence : outp.aux;
    if (!user) continue;
    TailCh t;
    t.w = (const float*)d->aux_project.w + 32 * ch; t.b = d->aux_bias[ch]; t.act = conf ? 3 : 2;
    if (k.out_kind == MD_MEM_HOST) { t.out = d->aux_stage + (size_t)ch * plane; t.bstride = (long)K7 * plane; }
    else if (conf) { t.out = user; t.bstride = (long)plane; }
    else { t.out = user + (size_t)ch * plane; t.bstride = (long)(K7 - 1) * plane; }
    chs[nch++] = t;
  }
  MD_TRY(tail(r, "aux_tail_fused", hin, ah, aw, d->aux_reduce, chs, nch));
  if (k.out_kind == MD_MEM_HOST)
    for (int ch = 0; ch < K7; ++ch) {
      const bool conf = ch == K7 - 1;
      float* user = conf ? outp.aux_confidence : outp.aux;
      if (!user) continue;
      for (int b = 0; b < B; ++b)
        MD_TRY(host_out(r.st, k.out_kind, conf ? user + (size_t)b * plane : user + ((size_t)b * (K7 - 1) + ch) * plane,
                        d->aux_stage + ((size_t)b * K7 + ch) * plane, plane));
    }
  return MD_OK;
}

// camera decoder (camera.rs:143-199) on the raw camera feature of the last hook, fp32: pose = (t3 | quat4 | relu(fov2)) rows [B, 9];
// device outputs are written straight into the caller's buffers
static int da3_camera_decoder(Run& r, const Da3Call& k) {
  md_model_s::Da3State* d = r.m->da3;
  const Da3Outputs& outp = k.outp;
  const int B = r.B;
  const bool dev_out = k.out_kind == MD_MEM_DEVICE;
  float* pose = (dev_out && outp.pose_encoding) ? outp.pose_encoding : d->pose;
  float* extr = (dev_out && outp.extrinsics) ? outp.extrinsics : d->extr;
  float* intr = (dev_out && outp.intrinsics) ? outp.intrinsics : d->intr;
  r.begin("camera_decoder");
  MD_TRY(launch_camera_decoder(d->cam_raw, B, d->din, d->cam_dec, k.H, k.W, d->cam_h1, d->cam_h2, pose, outp.extrinsics ? extr : nullptr,
                               outp.intrinsics ? intr : nullptr, r.st));
  r.end();
  if (!dev_out) {
    if (outp.pose_encoding) MD_HIP(hipMemcpyAsync(outp.pose_encoding, pose, (size_t)B * 9 * 4, hipMemcpyDeviceToHost, r.st));
    if (outp.extrinsics) MD_HIP(hipMemcpyAsync(outp.extrinsics, extr, (size_t)B * 12 * 4, hipMemcpyDeviceToHost, r.st));
    if (outp.intrinsics) MD_HIP(hipMemcpyAsync(outp.intrinsics, intr, (size_t)B * 9 * 4, hipMemcpyDeviceToHost, r.st));
  }
  return MD_OK;
}

// main branch: output_conv1 -> resize to the image size (+ UV table) -> output_conv2 + activation
static int da3_main_tail(Run& r, const Da3Call& k) {
  md_model_s* m = r.m;
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const Da3Outputs& outp = k.outp;
  const int B = r.B, ph = d->ph, pw = d->pw, IH = d->ih, IW = d->iw, F2 = c.features / 2, F2p = cpad(m, F2);
  r.begin("head_resize");
  MD_TRY(launch_resize_nhwc(k.c1_map, B, 8 * ph, 8 * pw, F2, F2p, d->c1r, IH, IW, F2p, MD_INTERP_BURN, d->pos_final, m->prec, r.st));
  r.end();
  if (m->taps_enabled) {
    MD_TRY(r.tap_nhwc("output_conv1", k.c1_map, F2, 8 * ph, 8 * pw, F2p));
    MD_TRY(r.tap_nhwc("head_input", d->c1r, F2, IH, IW, F2p));  // resized + UV table: the input of output_conv2
  }
  const float* w2 = (const float*)d->oc2_2.w;
  const size_t out_elems = (size_t)B * IH * IW;
  TailCh chs[8];
  int nch = 0;
  if (outp.raw_logits) {
    // infer_raw (mod.rs:364-380): the dual head hands out `depth_logits` = output_conv2's result as it is (dpt.rs:337-354, 271);
    // the mono head's `forward_raw` has its activation applied (dpt.rs:700)
    if (c.output_dim > 8) MD_FAIL(MD_ERR_UNSUPPORTED, "infer_raw with %d channels", c.output_dim);
    for (int ch = 0; ch < c.output_dim; ++ch)
      chs[nch++] = TailCh{w2 + 32 * ch, d->main_bias[ch], c.dual_head ? 2 : 1, k.depth_dev + (size_t)ch * IH * IW, (long)c.output_dim * IH * IW};
    MD_TRY(tail(r, "head_tail_fused", d->c1r, IH, IW, d->oc2_1, chs, nch));
    MD_TRY(host_out(r.st, k.out_kind, outp.raw_logits, k.depth_dev, out_elems * c.output_dim));
  } else {
    float* cd = nullptr;
    chs[nch++] = TailCh{w2, d->main_bias[0], 1, k.depth_dev, (long)IH * IW};  // depth = exp(ch 0)
    if (c.dual_head && outp.depth_confidence) {  // confidence = exp(last channel) + 1 (select_conf_channel, ExpP1)
      cd = k.out_kind == MD_MEM_HOST ? d->conf_stage : outp.depth_confidence;
      chs[nch++] = TailCh{w2 + 32 * (c.output_dim - 1), d->main_bias[c.output_dim - 1], 3, cd, (long)IH * IW};
    }
    MD_TRY(tail(r, "head_tail_fused", d->c1r, IH, IW, d->oc2_1, chs, nch));
    MD_TRY(host_out(r.st, k.out_kind, outp.depth, k.depth_dev, out_elems));
    if (cd) MD_TRY(host_out(r.st, k.out_kind, outp.depth_confidence, cd, out_elems));
  }
  if (k.out_kind == MD_MEM_HOST) MD_HIP(hipStreamSynchronize(r.st));
  return MD_OK;
}

static int da3_infer_eager(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, const Da3Outputs& outp, int out_kind,
                           hipStream_t stream) {
  if (!m || m->kind != 1 || !m->da3) MD_FAIL(MD_ERR_INVALID_ARG, "not a Depth-Anything-v3 model");
  if (!m->committed) MD_FAIL(MD_ERR_INVALID_ARG, "weights were modified; call md_model_commit_weights first");
  const KsplitScope ksplit(m->batch_invariant ? 0 : 1);  // small long-K launches may split their contraction inside the workgroup (kernels/gemm.h)
  const AttnSmallScope attn_small(m->batch_invariant ? 0 : 1);  // ... and few-workgroup attention launches their keys (kernels/ops.h)
  const bool from_tokens = outp.tokens[0] != nullptr;
  if ((!nchw && !from_tokens) || (!outp.depth && !outp.raw_logits)) MD_FAIL(MD_ERR_INVALID_ARG, "null pointer");
  if (outp.raw_logits && (outp.depth || outp.depth_confidence || outp.aux || outp.aux_confidence || outp.pose_encoding || outp.extrinsics || outp.intrinsics))
    MD_FAIL(MD_ERR_INVALID_ARG, "infer_raw returns the main logits only");
  md_model_s::Da3State* d = m->da3;
  const Da3Cfg& c = d->cfg;
  const ViTDims& v = c.vit;
  if (!c.dual_head && (outp.depth_confidence || outp.aux || outp.aux_confidence || outp.pose_encoding || outp.extrinsics || outp.intrinsics))
    MD_FAIL(MD_ERR_UNSUPPORTED, "the mono head produces depth only (finalize_inference, mod.rs:587-624)");
  if (B <= 0 || H <= 0 || W <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid input shape [%d,3,%d,%d]", B, H, W);
  if (H % v.ps != 0 || W % v.ps != 0)  // depth_anything3/mod.rs:509-520 (assert -> checked precondition)
    MD_FAIL(MD_ERR_SHAPE, "Input %dx%d must be divisible by patch size %d", H, W, v.ps);
  if (B > c.max_batch) MD_FAIL(MD_ERR_SHAPE, "batch %d exceeds max_batch %d", B, c.max_batch);
  MD_TRY(da3_check_views(m, B, outp));
  MD_HIP(hipSetDevice(m->dev->ordinal));
  MD_TRY(da3_set_shape(m, H, W, false));  // any multiple of the patch size (mod.rs:509-520); a no-op at the current size
  hipStream_t st = model_stream(m, stream);
  Run r{m, st, B};
  const bool want_aux = c.dual_head && (outp.aux || outp.aux_confidence);
  const bool want_cam = c.dual_head && !from_tokens && (outp.pose_encoding || outp.extrinsics || outp.intrinsics);
  Da3Call k{outp, in_kind, out_kind, H, W, want_aux, want_cam, want_aux ? 2 : 1,
            {4 * d->ph, 2 * d->ph, d->ph, d->h3h}, {4 * d->pw, 2 * d->pw, d->pw, d->h3w}};
  const float* x_dev = nchw;
  if (in_kind == MD_MEM_HOST && !from_tokens) {
    MD_HIP(hipMemcpyAsync(d->xin, nchw, (size_t)B * 3 * H * W * 4, hipMemcpyHostToDevice, st));
    x_dev = d->xin;
  }
  if (from_tokens) {
    MD_TRY(da3_stage_tokens(r, k));
  } else {
    // a model without a camera encoder ignores the camera inputs (mod.rs:522-527)
    if (c.camera_encoder && c.dual_head && outp.cam_extrinsics && outp.cam_intrinsics) MD_TRY(da3_camera_encoder(r, k));
    MD_TRY(da3_backbone(r, k, x_dev));
  }
  MD_TRY(da3_prepare_stages(r, k));
  k.depth_dev = outp.raw_logits ? outp.raw_logits : outp.depth;
  if (out_kind == MD_MEM_HOST) {
    MD_TRY(grow(m, st, d->depth_stage, (size_t)B * H * W * (outp.raw_logits ? c.output_dim : 1) * 4));
    k.depth_dev = d->depth_stage.p;
  }
  // Everything runs on the caller's stream. Rounds 3-4 ran the aux branch and the camera decoder on side streams (parallel branches of
  // the captured graph): every fork / join cost more than the overlap gave back (config 2, all outputs: 1.97 ms with two side streams,
  // 1.80 on one stream, 1.70 with the aux branch alone on a side stream; with the pyramids grouped 1.74 with a side stream for the aux
  // tail against 1.63 without -- profiles/r04_cfg2_branches.txt).
  MD_TRY(da3_pyramid(r, k));  // both pyramids (two weight groups) when the aux outputs are wanted
  if (want_aux) MD_TRY(da3_aux_tail(r, k));
  if (want_cam) MD_TRY(da3_camera_decoder(r, k));
  return da3_main_tail(r, k);
}

int da3_infer_direct(md_model_t m, const float* nchw, int B, int H, int W, float* depth, hipStream_t stream) {
  Da3Outputs o;
  o.depth = depth;
  return da3_infer_eager(m, nchw, B, H, W, MD_MEM_DEVICE, o, MD_MEM_DEVICE, stream);
}

int da3_infer_ex_direct(md_model_t m, const float* nchw, int B, int H, int W, const Da3Outputs& out, hipStream_t stream) {
  return da3_infer_eager(m, nchw, B, H, W, MD_MEM_DEVICE, out, MD_MEM_DEVICE, stream);
}

int da3_infer(md_model_t m, const float* nchw, int B, int H, int W, int in_kind, float* depth, int out_kind,
              hipStream_t stream) {
  Da3Outputs o;
  o.depth = depth;
  return da3_infer_ex(m, nchw, B, H, W, in_kind, o, out_kind, stream);
}

}  // namespace md
