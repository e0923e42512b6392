// CPU-only table of md::gemm256_form (csrc/kernels/gemm.hip): which kernel a 256 x 256 GEMM launch takes. One line per case:
//
//   PREC AMODE SHAPE TILES KT N PERSIST DIRECT DIAG CUS : FAMILY EK FOLD QKV CONV DIAG GRID PTILES STAGGER
//   PREC AMODE SHAPE TILES KT N PERSIST DIRECT DIAG CUS : refused CODE MESSAGE
//
// The parameters are filled the way the engine fills them (run_vit_block, conv3, deconv2, gemm_rows) and as launch_gemm hands
// them to the launcher. tests/test_gemm_form_table.py builds this file with the host compiler (no GPU, no HIP runtime call) and
// compares the output with tests/golden/gemm256_form_table.txt, which was recorded from the launcher as it was BEFORE the choice
// moved into gemm256_form (that launcher reporting its kernel instead of launching it): the table pins the selection, not the code.
//
// Without arguments: the committed table, a few hundred cases -- (a) the engine's launches in every precision, (b) the launches that
// take a tile loop along each axis through the loops' thresholds and switches, (c) the diagnostic path. `--full`: the complete cross
// product of all ten dimensions (1.6 million lines; compared once with the previous launcher, not committed).
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels/gemm.h"

using namespace md;

// the precision entry points gemm.hip dispatches to: not part of this program (launch_gemm is never called)
namespace md {
int launch_gemm_bf16(GemmParams&, int, int, hipStream_t) { return MD_ERR_UNSUPPORTED; }
int launch_gemm_f32(GemmParams&, int, int, hipStream_t) { return MD_ERR_UNSUPPORTED; }
int launch_gemm_f16(GemmParams&, int, int, hipStream_t) { return MD_ERR_UNSUPPORTED; }
int launch_gemm_fp8(GemmParams&, int, int, hipStream_t) { return MD_ERR_UNSUPPORTED; }
int launch_gemm_f16x2(GemmParams&, int, int, hipStream_t) { return MD_ERR_UNSUPPORTED; }
}  // namespace md

static float g_buf[16];  // every pointer of a case points here: gemm256_form looks at null / non-null only

static const int kPrec[] = {MD_PREC_BF16, MD_PREC_F16, MD_PREC_F16X2, MD_PREC_FP8, MD_PREC_F32};
static const char* const kPrecName[] = {"bf16", "f16", "f16x2", "fp8", "f32"};
static const int kAmode[] = {A_DENSE, A_INDEXED, A_CONV3};
static const char* const kAmodeName[] = {"dense", "indexed", "conv3"};
enum Shape {
  S_STORE, S_GELU, S_GELU_LN, S_GELU_LNRAW, S_QKV, S_QKV_LN, S_QKV_LNRAW, S_QKV_QKNORM, S_RESID, S_RESID_LN, S_RESID_SRC, S_PIXSHUF_FAST,
  S_PIXSHUF, S_CONV_LEAN, S_CONV_RES, S_OUT_F32, S_WSCALE, S_BATCH2, S_COUNT
};
static const char* const kShapeName[] = {"store", "gelu", "gelu+ln", "gelu+lnraw", "qkv", "qkv+ln", "qkv+lnraw", "qkv+qknorm", "resid", "resid+ln",
                                         "resid+src", "pixshuf_fast", "pixshuf", "conv_lean", "conv_res", "out_f32", "wscale", "batch2"};
static const int kTiles[] = {1, 767, 768, 1023, 1024, 2047, 2048};
static const int kKT[] = {2, 3, 8, 16, 32, 64};
static const int kPersist[] = {0, 1, 2, 4, 8, 15};
static const int kCus[] = {4, 256, 304};

struct Case {
  int prec, amode, shape, tiles, kt, nz, persist, direct, diag, cus;
};

// the launch as the engine's helpers fill it; returns the tile count the case really has (a multiple of its n-tiles)
static long fill(const Case& c, GemmParams& p) {
  const int prec = kPrec[c.prec];
  const int xm = prec == MD_PREC_F16X2 ? 2 : 1;  // planes per element
  const int ke = prec == MD_PREC_F32 ? 32 : (prec == MD_PREC_FP8 ? 128 : 64);
  const bool qkv = c.shape >= S_QKV && c.shape <= S_QKV_QKNORM;
  const bool gelu = c.shape == S_GELU || c.shape == S_GELU_LN || c.shape == S_GELU_LNRAW || c.shape == S_WSCALE;
  // N: whole 256-column tiles, or 128 columns more (qkv: embed = 256 / 384)
  const int N = qkv ? (c.nz ? 1152 : 768) : gelu ? (c.nz ? 1152 : 1024) : (c.nz ? 384 : 256);
  const int D = qkv ? N / 3 : gelu ? N / 4 : N;
  const int tn = (N + 255) / 256;
  // the tile counts just below a threshold round down to whole rows of n-tiles, the others up
  const bool below = c.tiles == 1 || c.tiles == 767 || c.tiles == 1023 || c.tiles == 2047;
  long tm = below ? c.tiles / tn : (c.tiles + tn - 1) / tn;
  if (tm < 1) tm = 1;
  p.N = N;
  p.K = c.kt * ke;
  p.ngroups = 1;
  p.g_rows[0] = (int)(tm * 256 - 37);  // a partial last m-tile
  p.W[0] = g_buf;
  p.A = g_buf;
  p.lda = p.K;
  p.bias[0] = g_buf;
  p.out = g_buf;
  auto t_out = [&](long ldo) { p.ldo = ldo * xm, p.o_plane = xm == 2 ? ldo : 0; };  // split_out
  if (kAmode[c.amode] == A_INDEXED) p.a_index = (const int*)g_buf;
  if (kAmode[c.amode] == A_CONV3) p.cH = 64, p.cW = 64, p.cC = 64 * xm, p.cCk = xm == 1 ? 0 : 128, p.zero_page = g_buf;
  auto ln_consumer = [&](bool raw) { p.ln_c[0] = g_buf, p.ln_stats = g_buf, p.ln_raw = raw, p.ln_parts = D / 256, p.ln_inv_n = 1.f / D, p.ln_eps = 1e-6f; };
  switch (c.shape) {
    case S_STORE: case S_BATCH2: case S_OUT_F32:  // gemm_rows
      p.epi = EPI_STORE;
      if (c.shape == S_OUT_F32) p.out_f32 = 1, p.ldo = N;
      else t_out(N);
      if (c.shape == S_BATCH2) p.batch = 2, p.batch_inner = 1, p.o_bs[0] = 1 << 20;
      break;
    case S_GELU: case S_GELU_LN: case S_GELU_LNRAW: case S_WSCALE:  // fc1
      p.epi = EPI_STORE, p.act = ACT_GELU;
      t_out(N);
      if (c.shape == S_GELU_LN || c.shape == S_GELU_LNRAW) ln_consumer(c.shape == S_GELU_LNRAW);
      if (c.shape == S_WSCALE) p.wscale[0] = g_buf, p.ascale = 0.5f, p.out_fp8 = prec == MD_PREC_FP8, p.out_inv_scale = 2.f;
      break;
    case S_QKV: case S_QKV_LN: case S_QKV_LNRAW: case S_QKV_QKNORM:
      p.epi = EPI_QKV, p.vT = g_buf, p.seq_stride = 580, p.embed = D, p.heads = D / 64, p.kpad = 640, p.qscale = 0.18f;
      p.v_plane = xm == 2 ? 1 << 20 : 0;
      if (c.shape == S_QKV_LN || c.shape == S_QKV_LNRAW) ln_consumer(c.shape == S_QKV_LNRAW);
      if (c.shape == S_QKV_QKNORM) {
        p.qkn_g[0] = p.qkn_g[1] = p.qkn_b[0] = p.qkn_b[1] = p.rope_cos = p.rope_sin = g_buf;
        p.rope_pw = 37, p.rope_ntok = 577;
      }
      break;
    case S_RESID: case S_RESID_LN: case S_RESID_SRC:  // proj / fc2
      p.epi = EPI_RESID_LS, p.scale[0] = g_buf, p.ldo = D;
      if (c.shape == S_RESID_SRC) p.resid_src = g_buf;
      if (c.shape == S_RESID_LN)
        p.ln_out = g_buf, p.ln_ldo = (long)D * xm, p.ln_plane = xm == 2 ? D : 0, p.ln_stats_out = g_buf, p.ln_parts = D / 256, p.ln_gamma[0] = g_buf;
      break;
    case S_PIXSHUF_FAST: case S_PIXSHUF:  // deconv2
      p.epi = EPI_PIXSHUF, p.ps_f = 2, p.psH = 48, p.psW = 48, p.psC = N / 4;
      t_out(256);
      if (c.shape == S_PIXSHUF) p.out2 = g_buf;
      p.ps_fast = prec != MD_PREC_F32 && !p.out2;  // (launch_gemm's rule for these parameters)
      break;
    case S_CONV_LEAN: case S_CONV_RES:  // conv3: the two convolutions of a residual unit
      p.epi = EPI_STORE;
      t_out(N);
      if (c.shape == S_CONV_LEAN) p.act = ACT_RELU;
      else p.res1 = g_buf, p.out2 = g_buf;
      p.ldr = p.ldo, p.r_plane = p.res1 ? p.o_plane : 0;
      break;
  }
  p.direct_store = c.direct;
  p.persist = c.persist;
  if (c.diag) p.debug_flags = 4;
  return tm * tn;
}

static const char* const kFamilyName[] = {"one_tile", "loop_p", "loop_r"};

static void run(const Case& c) {
  GemmParams p;
  const long blocks = fill(c, p);
  std::string why;
  const Form256 f = gemm256_form(p, kAmode[c.amode], kPrec[c.prec], c.cus, &why);
  printf("%s %s %s %ld %d %d %d %d %d %d : ", kPrecName[c.prec], kAmodeName[c.amode], kShapeName[c.shape], blocks, c.kt, p.N, c.persist, c.direct, c.diag, c.cus);
  if (f.err != MD_OK) printf("refused %d %s\n", f.err, why.c_str());
  else printf("%s %d %d %d %d %d %d %d %d\n", kFamilyName[f.family], f.ek, (int)f.fold, (int)f.qkv, (int)f.conv, (int)f.diag, f.grid, f.ptiles, f.stagger);
}

template <typename F>
static void each_launch(F&& body) {  // precision x A mode x epilogue shape
  for (int pr = 0; pr < 5; ++pr)
    for (int am = 0; am < 3; ++am)
      for (int sh = 0; sh < S_COUNT; ++sh) body(pr, am, sh);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--full")) {
    each_launch([](int pr, int am, int sh) {
      for (int t : kTiles) for (int kt : kKT) for (int nz = 0; nz < 2; ++nz) for (int pm : kPersist) for (int ds = 0; ds < 2; ++ds)
        for (int dg = 0; dg < 2; ++dg) for (int cu : kCus) run({pr, am, sh, t, kt, nz, pm, ds, dg, cu});
    });
    return 0;
  }
  // the launches the engine makes (shape in its own A mode) and some it does not (a GELU behind a gathered / convolution A operand)
  struct Launch { int amode, shape; };  // amode: index into kAmode
  static const Launch kLaunch[] = {{0, S_STORE}, {0, S_GELU}, {0, S_GELU_LN}, {0, S_GELU_LNRAW}, {0, S_QKV}, {0, S_QKV_LN}, {0, S_QKV_LNRAW}, {0, S_QKV_QKNORM},
                                   {0, S_RESID}, {0, S_RESID_LN}, {0, S_RESID_SRC}, {0, S_PIXSHUF_FAST}, {0, S_PIXSHUF}, {0, S_OUT_F32}, {0, S_WSCALE}, {0, S_BATCH2},
                                   {1, S_STORE}, {1, S_GELU}, {1, S_PIXSHUF_FAST}, {2, S_STORE}, {2, S_GELU}, {2, S_CONV_LEAN}, {2, S_CONV_RES}};
  static const Launch kLoop[] = {{0, S_GELU}, {0, S_GELU_LNRAW}, {0, S_QKV}, {0, S_QKV_LNRAW}, {0, S_RESID}, {0, S_RESID_LN}, {2, S_CONV_LEAN}, {2, S_CONV_RES}};
  // (a) every launch in every precision where all tile loops accept what they can take, and with N % 256 != 0
  for (int pr = 0; pr < 5; ++pr)
    for (const Launch& l : kLaunch) for (int nz = 0; nz < 2; ++nz) run({pr, l.amode, l.shape, 2048, 16, nz, 15, 1, 0, 256});
  // (b) the loop launches (bf16; fc1 and the read-modify-write pair in split-half too) through the thresholds: every tile count at 16
  //     k-tiles, every k-tile count at 2048 tiles; every persist mask x direct_store; the other CU counts
  for (int pr : {0, 2})
    for (const Launch& l : kLoop) {
      if (pr == 2 && (l.amode != 0 || l.shape == S_QKV || l.shape == S_QKV_LNRAW)) continue;  // (no split-half QKV / convolution loop)
      for (int t : kTiles) if (t != 2048) run({pr, l.amode, l.shape, t, 16, 0, 15, 1, 0, 256});
      for (int kt : kKT) if (kt != 16) run({pr, l.amode, l.shape, 2048, kt, 0, 15, 1, 0, 256});
      for (int pm : kPersist) for (int ds = 0; ds < 2; ++ds) if (!(pm == 15 && ds == 1)) run({pr, l.amode, l.shape, 2048, 16, 0, pm, ds, 0, 256});
      for (int cu : {4, 304}) run({pr, l.amode, l.shape, 2048, 16, 0, 15, 1, 0, cu});
    }
  // (c) the diagnostic path (stamps / ablation flags): built for dense bf16, refused elsewhere
  for (int pr : {0, 1})
    for (const Launch& l : kLaunch) run({pr, l.amode, l.shape, 2048, 16, 0, 15, 1, 1, 256});
  return 0;
}
