// md_process_frame: a u8 RGB camera frame in, a displayable depth map out, on the device in one call (the viewer's
// `process_frame`, crates/bevy_burn_depth/src/lib.rs:16-132; the CLI's prepare / save_depth_map, example/inference.rs:79-273).
// prepare (kernels/frame.hip) -> model (model_infer / da3_infer_ex bodies) -> display (kernels/frame.hip); one captured graph
// per replay key when the model replays graphs.
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "md_engine.h"
#include "md_engine_util.h"

namespace md {

namespace {
struct AxisTable {
  int2* win = nullptr;   // device [out_len]
  float* w = nullptr;    // device [out_len * maxc]
  int maxc = 1;
  std::vector<int> left, count;  // host copies (the horizontal pass's byte span)
};
}  // namespace

}  // namespace md

// Tap tables are never freed before the model: a captured graph bakes their addresses. The scratch buffers grow only (md::grow).
struct md_model_s::FrameState {
  std::map<std::pair<int, int>, md::AxisTable> tables;  // (in_len, out_len); out_len 0 = the identity (crop-only) table of in_len
  md::GrowBuf<float> nchw, tmp, depth;
  md::GrowBuf<float2> parts;
  // device homes of outputs the caller wants in host memory
  md::GrowBuf<void> display;
  md::GrowBuf<uint8_t> prepared;
  md::GrowBuf<float> small;  // range [B,2] | focal [B] | fovy [B]
};

namespace md {

void frame_destroy_state(md_model_t m) {
  md_model_s::FrameState* f = m->frame;
  if (!f) return;
  for (auto& kv : f->tables) {
    if (kv.second.win) (void)hipFree(kv.second.win);
    if (kv.second.w) (void)hipFree(kv.second.w);
  }
  delete f;
  m->frame = nullptr;
}

// host tables of one axis: Catmull-Rom (out_len > 0) or the identity of a crop (out_len == 0)
static void build_axis(int in_len, int out_len, std::vector<int>& left, std::vector<int>& count, std::vector<float>& w, int* maxc) {
  const int n = out_len > 0 ? out_len : in_len;
  *maxc = out_len > 0 ? catmull_rom_max_taps(in_len, out_len) : 1;
  left.assign(n, 0);
  count.assign(n, 1);
  w.assign((size_t)n * *maxc, 0.f);
  for (int o = 0; o < n; ++o) {
    if (out_len > 0) {
      catmull_rom_window(in_len, out_len, o, &left[o], &count[o], &w[(size_t)o * *maxc]);
    } else {
      left[o] = o;
      w[(size_t)o * *maxc] = 1.f;
    }
  }
}

static int upload_axis(int in_len, int out_len, AxisTable* t) {
  std::vector<float> w;
  build_axis(in_len, out_len, t->left, t->count, w, &t->maxc);
  const int n = (int)t->left.size();
  std::vector<int2> win(n);
  for (int o = 0; o < n; ++o) win[o] = make_int2(t->left[o], t->count[o]);
  MD_HIP(hipMalloc((void**)&t->win, (size_t)n * sizeof(int2)));
  MD_HIP(hipMalloc((void**)&t->w, w.size() * 4));
  MD_HIP(hipMemcpy(t->win, win.data(), (size_t)n * sizeof(int2), hipMemcpyHostToDevice));
  MD_HIP(hipMemcpy(t->w, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  return MD_OK;
}

static int frame_axis(md_model_s* m, int in_len, int out_len, const AxisTable** out) {
  md_model_s::FrameState* f = m->frame;
  auto it = f->tables.find({in_len, out_len});
  if (it == f->tables.end()) {
    AxisTable t;
    const int s = upload_axis(in_len, out_len, &t);
    if (s != MD_OK) {
      if (t.win) (void)hipFree(t.win);
      if (t.w) (void)hipFree(t.w);
      return s;
    }
    m->alloc_count += 2;
    it = f->tables.emplace(std::make_pair(in_len, out_len), std::move(t)).first;
  }
  *out = &it->second;
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------
// geometry (prepare_depth_anything3_image, src/model/mod.rs:162-210; prepare_input_frame, lib.rs:76-132)
// ------------------------------------------------------------------------------------------------
struct FramePlan {
  int sw = 0, sh = 0;  // resized size (= w, h: no resize)
  bool resize = false;
  int cx = 0, cy = 0, tw = 0, th = 0;  // centre crop = the model input
  int ow = 0, oh = 0;                  // display map
};

static int align_down(int v, int ps) {  // lib.rs:94-114
  const int a = ps * 4;
  if (v < ps) return v;
  if (v >= a) return v - v % a;
  return v - v % ps;
}

static int frame_plan(md_model_s* m, int w, int h, const md_frame_opts& o, FramePlan* p) {
  if (m->kind == 0) {
    if (o.target != 0) MD_FAIL(MD_ERR_INVALID_ARG, "Depth Pro takes the frame at its own size: target must be 0, got %d", o.target);
    p->sw = w; p->sh = h; p->tw = w; p->th = h;
  } else {
    int ps = 14, ch = 0, cw = 0;
    da3_frame_info(m, &ps, &ch, &cw);
    if (o.target < -1) MD_FAIL(MD_ERR_INVALID_ARG, "target %d (> 0, 0 = the model's img_size, -1 = patch-aligned crop)", o.target);
    if (o.target == -1) {
      const int cwd = std::max(align_down(w, ps), 1), cht = std::max(align_down(h, ps), 1);
      p->sw = w; p->sh = h; p->tw = cwd; p->th = cht;
      p->cx = (w - cwd) / 2;
      p->cy = (h - cht) / 2;
    } else {
      const int t = std::max(std::max(o.target == 0 ? m->S : o.target, ps), 1);
      p->tw = p->th = t;
      if (w == t && h == t) {
        p->sw = w; p->sh = h;
      } else {
        const float shortest = (float)std::max(std::min(w, h), 1);
        const float scale = (float)t / shortest;
        p->sw = std::max((int)rintf((float)w * scale), t);
        p->sh = std::max((int)rintf((float)h * scale), t);
        p->resize = true;
        p->cx = (p->sw - t) / 2;
        p->cy = (p->sh - t) / 2;
      }
    }
    if (p->th % ps != 0 || p->tw % ps != 0)  // the model's own check (depth_anything3/mod.rs:509-520)
      MD_FAIL(MD_ERR_SHAPE, "Input %dx%d must be divisible by patch size %d", p->th, p->tw, ps);
  }
  p->ow = o.restore ? w : p->tw;
  p->oh = o.restore ? h : p->th;
  return MD_OK;
}

static int check_opts(const md_frame_opts* o) {
  if (!o) MD_FAIL(MD_ERR_INVALID_ARG, "frame options are null");
  if (o->format != MD_FRAME_U8_GRAY && o->format != MD_FRAME_RGBA_F32) MD_FAIL(MD_ERR_INVALID_ARG, "unknown display format %d", o->format);
  if (o->format == MD_FRAME_U8_GRAY && !o->normalize) MD_FAIL(MD_ERR_INVALID_ARG, "the u8 grey display needs normalize = 1");
  return MD_OK;
}

int frame_geometry(md_model_t m, int w, int h, const md_frame_opts* o, int* th, int* tw, int* oh, int* ow) {
  if (w <= 0 || h <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid frame size %dx%d", w, h);
  MD_TRY(check_opts(o));
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  FramePlan p;
  MD_TRY(frame_plan(m, w, h, *o, &p));
  if (th) *th = p.th;
  if (tw) *tw = p.tw;
  if (oh) *oh = p.oh;
  if (ow) *ow = p.ow;
  return MD_OK;
}

DisplayGeom display_geom(int B, int h, int w, int cx, int cy, int cw, int ch, int ow, int oh) {
  DisplayGeom g;
  g.B = B; g.h = h; g.w = w; g.cx = cx; g.cy = cy; g.cw = cw; g.ch = ch; g.ow = ow; g.oh = oh;
  g.resize = (ow != cw || oh != ch) ? 1 : 0;  // pipeline.resize_depth_field returns the map itself at its own size
  g.sx = ow > 1 ? (float)cw / (float)ow : 0.f;
  g.sy = oh > 1 ? (float)ch / (float)oh : 0.f;
  return g;
}

// ------------------------------------------------------------------------------------------------
// the call
// ------------------------------------------------------------------------------------------------
static int frame_eager(md_model_s* m, const uint8_t* rgb, int B, int w, int h, int in_kind, const md_frame_opts& o, const FramePlan& p,
                       const md_frame_outputs& out, int out_kind, hipStream_t st) {
  if (!m->frame) m->frame = new md_model_s::FrameState();
  md_model_s::FrameState* f = m->frame;
  const bool host_out = out_kind == MD_MEM_HOST;
  const size_t in_bytes = (size_t)B * h * w * 3, tpx = (size_t)B * p.th * p.tw, opx = (size_t)B * p.oh * p.ow;
  const size_t disp_bytes = opx * (o.format == MD_FRAME_U8_GRAY ? 1 : 16);
  // ---- device homes (grow-only, before anything is enqueued) ----
  MD_TRY(grow(m, st, f->nchw, tpx * 3 * 4));
  float* depth = out.depth;
  if (!depth || host_out) {
    MD_TRY(grow(m, st, f->depth, tpx * 4));
    depth = f->depth.p;
  }
  void* display = out.display;
  uint8_t* prepared = out.prepared;
  float *range = out.depth_range, *focal = out.focallength_px, *fovy = out.fovy_rad;
  if (host_out) {
    if (display) {
      MD_TRY(grow(m, st, f->display, disp_bytes));
      display = f->display.p;
    }
    if (prepared) {
      MD_TRY(grow(m, st, f->prepared, tpx * 3));
      prepared = f->prepared.p;
    }
    if (range || focal || fovy) {
      MD_TRY(grow(m, st, f->small, (size_t)B * 4 * 4));
      range = range ? f->small.p : nullptr;
      focal = focal ? f->small.p + 2 * B : nullptr;
      fovy = fovy ? f->small.p + 3 * B : nullptr;
    }
  }
  const DisplayGeom g = display_geom(B, p.th, p.tw, 0, 0, p.tw, p.th, p.ow, p.oh);
  if (o.normalize || range) MD_TRY(grow(m, st, f->parts, (size_t)B * display_parts(g) * sizeof(float2)));
  const AxisTable *av = nullptr, *ah = nullptr;
  int xb0 = 0, nq = 0;
  if (m->kind == 1) {
    MD_TRY(frame_axis(m, h, p.resize ? p.sh : 0, &av));
    MD_TRY(frame_axis(m, w, p.resize ? p.sw : 0, &ah));
    catmull_rom_span(ah->left.data(), ah->count.data(), p.cx, p.tw, &xb0, &nq);
    MD_TRY(grow(m, st, f->tmp, (size_t)B * p.th * nq * 16));
  }
  // ---- the frame on the device ----
  const uint8_t* src = rgb;
  if (in_kind == MD_MEM_HOST) MD_TRY(model_stage_rgb(m, rgb, in_bytes, st, &src));
  Run r{m, st, B};
  // ---- prepare ----
  if (m->kind == 1) {
    r.begin("frame_prepare");
    MD_TRY(launch_resize_catmull_rom(src, B, h, w, CrAxis{av->win, av->w, av->maxc}, p.cy, p.th, CrAxis{ah->win, ah->w, ah->maxc}, p.cx,
                                     p.tw, xb0, nq, f->tmp.p, prepared, f->nchw.p, st));
    r.end();
    MD_TRY(da3_infer_direct(m, f->nchw.p, B, p.th, p.tw, depth, st));
  } else {
    r.begin("frame_prepare");
    for (int b = 0; b < B; ++b)  // rgb_to_input_tensor per frame (what md_infer_from_rgb runs)
      MD_TRY(launch_rgb_to_input(src + (size_t)b * h * w * 3, w, h, f->nchw.p + (size_t)b * 3 * h * w, st));
    if (prepared) MD_HIP(hipMemcpyAsync(prepared, src, in_bytes, hipMemcpyDeviceToDevice, st));
    r.end();
    MD_TRY(model_infer_direct(m, f->nchw.p, B, h, w, depth, focal, fovy, st));
  }
  // ---- display ----
  r.begin("frame_display");
  MD_TRY(launch_depth_display(depth, g, o.normalize, o.format, display, range, f->parts.p, st));
  r.end();
  if (!host_out) return MD_OK;
  auto d2h = [&](void* dst, const void* srcp, size_t bytes) -> int {
    if (dst) MD_HIP(hipMemcpyAsync(dst, srcp, bytes, hipMemcpyDeviceToHost, st));
    return MD_OK;
  };
  MD_TRY(d2h(out.depth, depth, tpx * 4));
  MD_TRY(d2h(out.display, display, disp_bytes));
  MD_TRY(d2h(out.prepared, prepared, tpx * 3));
  MD_TRY(d2h(out.depth_range, range, (size_t)B * 8));
  MD_TRY(d2h(out.focallength_px, focal, (size_t)B * 4));
  MD_TRY(d2h(out.fovy_rad, fovy, (size_t)B * 4));
  MD_HIP(hipStreamSynchronize(st));  // host outputs are complete when the call returns
  return MD_OK;
}

int process_frame(md_model_t m, const uint8_t* rgb, int B, int w, int h, int in_kind, const md_frame_opts* o, const md_frame_outputs* out,
                  int out_kind, hipStream_t stream) {
  if (!rgb) MD_FAIL(MD_ERR_INVALID_ARG, "rgb pointer is null");
  if (w <= 0 || h <= 0) MD_FAIL(MD_ERR_SHAPE, "invalid frame size %dx%d", w, h);
  if (B <= 0) MD_FAIL(MD_ERR_SHAPE, "batch %d: at least one frame", B);
  MD_TRY(check_opts(o));
  if (!out) MD_FAIL(MD_ERR_INVALID_ARG, "frame outputs are null");
  if ((in_kind != MD_MEM_HOST && in_kind != MD_MEM_DEVICE) || (out_kind != MD_MEM_HOST && out_kind != MD_MEM_DEVICE))
    MD_FAIL(MD_ERR_INVALID_ARG, "unknown memory kind");
  if (!m) MD_FAIL(MD_ERR_INVALID_ARG, "model is null");
  if (B > m->cfg.max_batch) MD_FAIL(MD_ERR_SHAPE, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
  if (m->kind == 1 && (out->focallength_px || out->fovy_rad))
    MD_FAIL(MD_ERR_INVALID_ARG, "focal length / fovy are Depth Pro outputs");
  if (!model_root(m)->committed) MD_FAIL(MD_ERR_INVALID_ARG, "weights were modified; call md_model_commit_weights first");
  FramePlan p;
  MD_TRY(frame_plan(m, w, h, *o, &p));
  MD_HIP(hipSetDevice(m->dev->ordinal));
  hipStream_t st = model_stream(m, stream);
  auto body = [&]() { return frame_eager(m, rgb, B, w, h, in_kind, *o, p, *out, out_kind, st); };
  if (!m->graph_enabled) return body();
  // the key: stream, frame size, every option, every pointer and the commit generation (a graph bakes the weights' by-value
  // launch parameters); a Depth-Anything-v3 graph only replays at the model's current input size (its workspace plan)
  const unsigned gen = model_root(m)->commit_gen;
  bool eligible = in_kind == MD_MEM_DEVICE && out_kind == MD_MEM_DEVICE;
  if (m->kind == 1) {
    int ps = 0, ch = 0, cw = 0;
    da3_frame_info(m, &ps, &ch, &cw);
    eligible = eligible && ch == p.th && cw == p.tw;
  }
  const std::vector<uintptr_t> key = {(uintptr_t)0x46524d45u, (uintptr_t)st, (uintptr_t)B, (uintptr_t)w, (uintptr_t)h, (uintptr_t)rgb,
                                      (uintptr_t)(intptr_t)o->target, (uintptr_t)o->restore, (uintptr_t)o->normalize, (uintptr_t)o->format,
                                      (uintptr_t)out->display, (uintptr_t)out->depth, (uintptr_t)out->depth_range, (uintptr_t)out->prepared,
                                      (uintptr_t)out->focallength_px, (uintptr_t)out->fovy_rad, (uintptr_t)gen};
  return run_with_graph(m, st, key, eligible, body);
}

}  // namespace md
