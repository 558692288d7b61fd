// Host-side logic of libcatseg_hip.so under AddressSanitizer + UBSan (the reference has no sanitizer; "the build adds ... an ASan
// build of the C++ host code").  GPU code cannot be sanitised on this pool, and needs no GPU here: everything called below either answers on
// the host (size / plan / capability queries) or must REJECT its arguments before the first HIP call.  Built and run by
// tests/test_host_asan_cpu.py against csrc/Makefile's `asan` target; test infrastructure, not shipped.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "catseg.h"
#include "catseg_debug.h"

static int checks = 0, failed = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    ++checks;                                                               \
    if (!(cond)) { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

// an entry point must refuse its arguments on the host: `code`, and a message that contains `sub`
#define EXPECT_ERR(call, code, sub)                                                                            \
  do {                                                                                                         \
    const int rc__ = (call);                                                                                   \
    ++checks;                                                                                                  \
    if (rc__ != (code) || std::strstr(catseg_last_error(), (sub)) == nullptr) {                                \
      ++failed;                                                                                                \
      std::printf("FAILED %s:%d: %s -> %d \"%s\" (expected %d \"%s\")\n", __FILE__, __LINE__, #call, rc__, catseg_last_error(), (code), (sub)); \
    }                                                                                                          \
  } while (0)

static catseg_conv_desc desc(int B, int H, int W, int Cin, int Cout, int k, int s, int p, int d = 1) {
  catseg_conv_desc c;
  std::memset(&c, 0, sizeof c);
  c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout;
  c.kh = c.kw = k; c.stride = s; c.pad = p; c.dil = d;
  c.Ho = (H + 2 * p - d * (k - 1) - 1) / s + 1;
  c.Wo = (W + 2 * p - d * (k - 1) - 1) / s + 1;
  c.ldx = Cin; c.ldy = (Cout + 3) / 4 * 4;
  return c;
}

// the convolution entry points take descriptors: one call per line below through these (a field not named is NULL / 0)
enum { F32 = CATSEG_OPERANDS_F32, B3 = CATSEG_OPERANDS_BF16X3, B3B = CATSEG_OPERANDS_BF16X3_BLOCKED, H2P = CATSEG_OPERANDS_F16X2,
       H2B = CATSEG_OPERANDS_F16X2_BLOCKED };
static int fwd(int form, const catseg_conv_desc& g, const void* x, const void* x_scale, const void* w, const void* w_scale, const float* bias, float* y,
               int zero_to, float* bn_part = nullptr, size_t bn_part_floats = 0, int* tile_rows = nullptr, int* n_tiles = nullptr,
               const float* residual = nullptr, int ldr = 0, int relu = 0) {
  const catseg_conv_fwd_desc q = {g, form, x, x_scale, w, w_scale, bias, y, zero_to, bn_part, bn_part_floats, tile_rows, n_tiles, residual, ldr, relu};
  return catseg_conv2d_fwd(&q, nullptr);
}
static int dgrad(int form, const catseg_conv_desc& g, const void* dy, const void* dy_scale, const void* w, const void* w_scale, float* dx, int accumulate) {
  const catseg_conv_bwd_data_desc q = {g, form, dy, dy_scale, w, w_scale, dx, accumulate};
  return catseg_conv2d_bwd_data(&q, nullptr);
}
static int wgrad(int form, const catseg_conv_desc& g, const void* x, const void* x_scale, const void* dy, const void* dy_scale, float* dw, void* workspace,
                 size_t workspace_bytes, float* dbias = nullptr) {
  const catseg_conv_bwd_weight_desc q = {g, form, x, x_scale, dy, dy_scale, dw, dbias, workspace, workspace_bytes};
  return catseg_conv2d_bwd_weight(&q, nullptr);
}

int main() {
  EXPECT(catseg_version() >= 3);
  alignas(16) static float buf[64];
  float* p16 = buf;

  // ---- size / capability queries over the shapes of the bench model and a few hostile ones
  const int widths[] = {0, 1, 3, 4, 8, 25, 32, 48, 64, 96, 192, 384, 720, 2048, 1 << 20};
  for (int C : widths) {
    const int sup = catseg_dconv3_supported(C), supw = catseg_dwgrad3_supported(C);
    const int supp = catseg_dconv3_pl_supported(C), supwp = catseg_dwgrad3_pl_supported(C);
    EXPECT((sup == 0 || sup == 1) && (supw == 0 || supw == 1) && (supp == 0 || supp == 1) && (supwp == 0 || supwp == 1));
    if (sup) {
      EXPECT(catseg_dconv3_wimg_bytes(C) >= (size_t)9 * C * C * 2);
      int th = -1, tw = -1;
      const int nt = catseg_dconv3_tiles(C, 8, 136, 240, &th, &tw);
      EXPECT(nt > 0 && th > 0 && tw > 0 && (long long)nt * th * tw >= 8LL * 136 * 240);
      EXPECT(catseg_dconv3_tiles(C, 8, 136, 240, nullptr, nullptr) == nt);
      EXPECT(catseg_dconv3_tiles(C, 1, 1, 1, &th, &tw) >= 1);
    }
    if (supw) EXPECT(catseg_dwgrad3_workspace(8, 136, 240, C) > 0);
    if (supp) EXPECT(catseg_dconv3_pl_rows(C, 8, 136, 240) > 0 && catseg_dconv3_pl_rows(C, 1, 3, 5) > 0);
    if (supwp) EXPECT(catseg_dwgrad3_pl_workspace(8, 68, 120, C) > 0);
    if (C > 0 && C % 8 == 0 && C <= 4096) EXPECT(catseg_planes_bytes(1000, C) == (size_t)1000 * C * 4);
  }
  EXPECT(catseg_split3_elems(10, 13) == 10u * 16u);
  EXPECT(catseg_split3_blocked_elems(10, 17) == 3u * 32u * 10u);
  EXPECT(catseg_split2h_blocked_elems(7, 48) == 2u * 48u * 7u && catseg_split2h_planar_elems(7, 50) == 2u * 7u * 56u);
  EXPECT(catseg_lovasz_workspace(4177920, 25) > (size_t)4177920 * 25 * 16);
  EXPECT(catseg_lovasz_workspace(1, 1) > 0 && catseg_ce_workspace(1) > 0 && catseg_ohem_workspace(1) > 0);
  EXPECT(catseg_ce_workspace(4177920) > 0 && catseg_ohem_workspace(4177920) > 0);
  EXPECT(catseg_bn_workspace(261120, 48) > 0 && catseg_bn_workspace(1, 4) > 0 && catseg_bn_workspace(8LL * 544 * 960, 2048) > 0);
  EXPECT(catseg_softmax_spatial_workspace(8, 32640) > 0);

  // ---- tile planner over every convolution family of the three training configurations (+ degenerate extents)
  struct Shape { int B, H, W, Cin, Cout, k, s, p, d; };
  const Shape shapes[] = {
      {8, 544, 960, 4, 64, 3, 2, 1, 1},    {8, 272, 480, 64, 64, 3, 2, 1, 1},   {8, 136, 240, 64, 256, 1, 1, 0, 1},
      {8, 136, 240, 48, 48, 3, 1, 1, 1},   {8, 136, 240, 48, 96, 3, 2, 1, 1},   {8, 68, 120, 96, 192, 3, 2, 1, 1},
      {8, 17, 30, 384, 48, 1, 1, 0, 1},    {8, 136, 240, 720, 512, 3, 1, 1, 1}, {8, 136, 240, 1024, 512, 1, 1, 0, 1},
      {8, 136, 240, 512, 25, 1, 1, 0, 1},  {8, 68, 120, 2048, 256, 3, 1, 12, 12}, {8, 68, 120, 2048, 256, 3, 1, 36, 36},
      {1, 1, 1, 4, 1, 1, 1, 0, 1},         {1, 3, 5, 8, 7, 3, 1, 1, 1},         {2, 16, 24, 32, 32, 16, 8, 4, 1},
      {8, 25, 1, 512, 256, 1, 1, 0, 1},    {4, 272, 480, 2048, 512, 3, 1, 1, 1}};
  for (const Shape& q : shapes) {
    catseg_conv_desc d = desc(q.B, q.H, q.W, q.Cin, q.Cout, q.k, q.s, q.p, q.d);
    for (int op = 0; op < 3; ++op) {
      int out[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
      const int rc = catseg_debug_plan_conv(&d, op, out);
      if (rc != CATSEG_OK) std::printf("plan_conv(%d x %d x %d x %d -> %d, k%d s%d, op %d): %s\n", q.B, q.H, q.W, q.Cin, q.Cout, q.k, q.s, op, catseg_last_error());
      EXPECT(rc == CATSEG_OK);
      EXPECT(out[0] >= 0);
    }
    EXPECT(catseg_conv2d_bwd_weight_workspace(&d, F32) > 0);
    if (q.Cin % 8 == 0) {       // (0 = this layer is not one the split-precision backward-weight kernels take)
      catseg_conv_desc e = d;
      e.ldx = q.Cin; e.ldy = (q.Cout + 7) / 8 * 8;
      (void)catseg_conv2d_bwd_weight_workspace(&e, B3);
      (void)catseg_conv2d_bwd_weight_workspace(&e, H2P);
    }
  }
  {
    catseg_conv_desc d = desc(1, 8, 8, 8, 8, 3, 1, 1);
    int out[8];
    EXPECT(catseg_debug_plan_conv(&d, 3, out) != CATSEG_OK && catseg_debug_plan_conv(&d, -1, out) != CATSEG_OK);
    EXPECT(catseg_debug_plan_conv(&d, 0, nullptr) != CATSEG_OK);
  }

  // ---- pinned plans: workspace sizes and tile plans of the layers the split-precision paths serve, as literals (recorded from the library
  // before the host launch code of the implicit-GEMM files was consolidated; a mismatch prints the row to paste after a DELIBERATE change)
  {
    struct Pin { Shape s; size_t ws_b3, ws_h2, ws_f32; int plan[3][5]; };
    const Pin pins[] = {
        {{8, 136, 240, 720, 512, 3, 1, 1, 1}, 716636160u, 716636160u, 66879488u, {{2, 2, 0, 1, 0}, {2, 2, 0, 1, 0}, {4, 2, 0, 5, 0}}},
        {{8, 136, 240, 512, 512, 3, 1, 1, 1}, 603979776u, 603979776u, 66584576u, {{2, 2, 0, 1, 0}, {2, 2, 0, 1, 0}, {4, 2, 0, 7, 0}}},
        {{8, 136, 240, 1024, 512, 1, 1, 0, 1}, 67108864u, 67108864u, 67633152u, {{2, 2, 0, 1, 0}, {2, 2, 0, 1, 0}, {4, 2, 0, 32, 0}}},
        {{8, 68, 120, 2048, 512, 1, 1, 0, 1}, 67108864u, 67108864u, 67633152u, {{2, 2, 0, 1, 0}, {2, 2, 0, 1, 0}, {4, 2, 0, 16, 0}}},
        {{8, 68, 120, 512, 2048, 1, 1, 0, 1}, 67108864u, 67108864u, 69206016u, {{2, 2, 0, 1, 0}, {2, 2, 0, 1, 0}, {4, 2, 0, 16, 0}}},
        {{8, 136, 240, 48, 48, 3, 1, 1, 1}, 5308416u, 5308416u, 42350592u, {{2, 1, 1, 1, 0}, {2, 1, 1, 1, 0}, {1, 1, 0, 96, 1}}},
        {{8, 136, 240, 48, 96, 3, 2, 1, 1}, 4976640u, 4976640u, 15857664u, {{2, 2, 1, 1, 0}, {2, 1, 1, 1, 0}, {1, 1, 0, 95, 0}}},
        {{8, 68, 120, 96, 192, 3, 2, 1, 1}, 4644864u, 4644864u, 20766720u, {{1, 1, 0, 1, 0}, {2, 2, 1, 1, 0}, {1, 1, 0, 31, 0}}},
        {{1, 3, 5, 8, 7, 3, 1, 1, 1}, 0u, 0u, 7168u, {{2, 1, 3, 1, 0}, {1, 1, 0, 1, 0}, {1, 1, 0, 1, 0}}},
    };
    for (const Pin& q : pins) {
      const Shape& s = q.s;
      catseg_conv_desc d = desc(s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.s, s.p, s.d);
      const size_t b3 = catseg_conv2d_bwd_weight_workspace(&d, B3), h2 = catseg_conv2d_bwd_weight_workspace(&d, H2P);
      const size_t f32 = catseg_conv2d_bwd_weight_workspace(&d, F32);
      int plan[3][5];
      bool same = b3 == q.ws_b3 && h2 == q.ws_h2 && f32 == q.ws_f32;
      for (int op = 0; op < 3; ++op) {
        EXPECT(catseg_debug_plan_conv(&d, op, plan[op]) == CATSEG_OK);
        same = same && std::memcmp(plan[op], q.plan[op], sizeof plan[op]) == 0;
      }
      EXPECT(same);
      if (!same) {
        std::printf("        {{%d, %d, %d, %d, %d, %d, %d, %d, %d}, %zuu, %zuu, %zuu, {", s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.s, s.p, s.d, b3, h2, f32);
        for (int op = 0; op < 3; ++op)
          std::printf("{%d, %d, %d, %d, %d}%s", plan[op][0], plan[op][1], plan[op][2], plan[op][3], plan[op][4], op < 2 ? ", " : "}},\n");
      }
    }
  }

  // ---- argument validation: every call below must fail ON THE HOST, with a message, before any HIP call (there is no GPU here)
  {
    catseg_conv_desc d = desc(1, 8, 8, 6, 16, 1, 1, 0);        // Cin not a multiple of 4
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);
    EXPECT(std::strstr(catseg_last_error(), "multiple of 4") != nullptr);
    d = desc(1, 8, 8, 8, 16, 3, 1, 1);
    d.Ho = 9;                                                   // inconsistent geometry
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);
    EXPECT(dgrad(F32, d, p16, nullptr, p16, nullptr, p16, 0) != CATSEG_OK);
    d = desc(1, 8, 8, 8, 16, 3, 1, 1);
    d.ldx = 6;                                                  // row stride below the channel count
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);
    d = desc(1, 8, 8, 8, 16, 3, 1, 1);
    EXPECT(fwd(F32, d, p16 + 1, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);      // misaligned pointer
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 64) != CATSEG_OK);         // zero_to beyond the row
    d = desc(INT_MAX / 2, 8, 8, 8, 16, 3, 1, 1);                                            // extents whose products overflow 32 bits
    (void)catseg_conv2d_bwd_weight_workspace(&d, F32);
    int out[8];
    (void)catseg_debug_plan_conv(&d, 0, out);
    d = desc(1, 8, 8, 8, 16, 3, 1, 1);
    d.stride = 0;                                                                           // stride 0: no division by it on the host
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);
    d = desc(1, 8, 8, 8, 16, 3, 1, 1);
    d.groups = 3;                                                                           // channels not divisible by the groups
    EXPECT(fwd(F32, d, p16, nullptr, p16, nullptr, nullptr, p16, 0) != CATSEG_OK);
  }
  // ---- the split-precision convolution entry points (bf16x3: three bf16 planes; f16x2: two fp16 planes): each refuses with its own code and
  // message -- misaligned planes, a channel count its layout cannot hold, a strided backward-data, operands past the index limits, a workspace
  // below what its own query asks for
  {
    void* pl = p16;
    void* off = (char*)p16 + 4;     // 4-byte aligned only
    int tr = -1, ntl = -1;
    const catseg_conv_desc ok = desc(1, 8, 8, 16, 16, 3, 1, 1);
    const catseg_conv_desc c24 = desc(1, 8, 8, 24, 16, 3, 1, 1);       // Cin % 8 == 0, % 16 != 0
    const catseg_conv_desc c12 = desc(1, 8, 8, 12, 16, 3, 1, 1);       // Cin % 8 != 0
    const catseg_conv_desc s2 = desc(1, 8, 8, 16, 16, 3, 2, 1);
    const catseg_conv_desc grp = [&] { catseg_conv_desc g = ok; g.groups = 2; return g; }();
    const catseg_conv_desc huge = desc(64, 1024, 1024, 32, 32, 1, 1, 0);    // 2^31 elements per activation plane
    const catseg_conv_desc big = desc(8, 1024, 1024, 96, 96, 1, 1, 0);      // < 2^31 elements, but the planes of one operand pass 4 GB
    const catseg_conv_desc head = desc(8, 136, 240, 720, 512, 3, 1, 1);     // a layer whose backward-weight plans several splits

    EXPECT_ERR(fwd(B3, ok, off, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL, "conv fwd bf16x3: alignment");
    EXPECT_ERR(fwd(B3, ok, pl, nullptr, pl, nullptr, nullptr, p16, 64), CATSEG_EINVAL, "conv fwd bf16x3: alignment");     // zero_to > ldy
    EXPECT_ERR(fwd(B3, c12, pl, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL, "conv fwd bf16x3: needs Cin % 8 == 0");
    EXPECT_ERR(fwd(B3, grp, pl, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL, "conv fwd bf16x3: needs Cin % 8 == 0");
    EXPECT_ERR(fwd(B3, huge, pl, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL, "conv fwd bf16x3: 32-bit offsets");
    EXPECT_ERR(fwd(B3, ok, pl, nullptr, off, nullptr, nullptr, p16, 0, p16, 64, &tr, &ntl), CATSEG_EINVAL, "conv fwd bf16x3: bad args");
    EXPECT_ERR(fwd(B3, ok, pl, nullptr, pl, nullptr, nullptr, p16, 0, p16, 64, nullptr, &ntl), CATSEG_EINVAL, "conv fwd bf16x3: bad args");
    EXPECT_ERR(fwd(B3, c12, pl, nullptr, pl, nullptr, nullptr, p16, 0, p16, 64, &tr, &ntl), CATSEG_EINVAL, "conv fwd bf16x3: needs Cin % 8 == 0");
    EXPECT_ERR(fwd(B3, huge, pl, nullptr, pl, nullptr, nullptr, p16, 0, p16, 64, &tr, &ntl), CATSEG_EINVAL, "conv fwd bf16x3: 32-bit offsets");
    EXPECT(tr == -1 && ntl == -1);                                          // a refused call leaves the tile contract untouched
    EXPECT_ERR(fwd(B3B, c24, pl, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL,
               "conv fwd bf16x3 blocked: needs Cin % 16 == 0");
    EXPECT_ERR(fwd(B3B, ok, off, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL,
               "conv fwd bf16x3 blocked: alignment");
    EXPECT_ERR(fwd(B3B, ok, pl, nullptr, pl, nullptr, nullptr, p16, 0, p16, 64, nullptr, nullptr), CATSEG_EINVAL,
               "conv fwd bf16x3 blocked: tile_rows / n_tiles");
    EXPECT_ERR(fwd(B3B, big, pl, nullptr, pl, nullptr, nullptr, p16, 0), CATSEG_EINVAL,
               "bf16x3 blocked planes: an operand's three planes must stay below 4 GB");
    EXPECT_ERR(fwd(B3B, big, pl, nullptr, pl, nullptr, nullptr, p16, 0, p16, 0, &tr, &ntl), CATSEG_EINVAL,
               "bf16x3 blocked planes: an operand's three planes must stay below 4 GB");
    EXPECT(tr == 0 && ntl == 0);                                            // (the partials did not fit: claimed nothing, then refused by the launcher)
    EXPECT_ERR(fwd(B3B, c24, pl, nullptr, pl, nullptr, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 1), CATSEG_EINVAL,
               "conv fwd fused bf16x3: needs Cin % 16 == 0");
    EXPECT_ERR(fwd(B3B, ok, pl, nullptr, pl, nullptr, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, p16, 8, 1), CATSEG_EINVAL, "conv fwd fused bf16x3: bad args");
    EXPECT_ERR(fwd(B3B, ok, pl, nullptr, pl, nullptr, nullptr, (float*)off, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 1), CATSEG_EINVAL,
               "conv fwd fused bf16x3: bad args");
    EXPECT_ERR(fwd(B3B, big, pl, nullptr, pl, nullptr, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 1), CATSEG_EINVAL,
               "bf16x3 blocked planes: an operand's three planes must stay below 4 GB");
    EXPECT_ERR(dgrad(B3, s2, pl, nullptr, pl, nullptr, p16, 0), CATSEG_EINVAL, "conv bwd_data bf16x3: stride 1");
    EXPECT_ERR(dgrad(B3, ok, pl, nullptr, off, nullptr, p16, 0), CATSEG_EINVAL, "conv bwd_data bf16x3: alignment");
    EXPECT_ERR(dgrad(B3, huge, pl, nullptr, pl, nullptr, p16, 0), CATSEG_EINVAL, "conv bwd_data bf16x3: 32-bit offsets");
    EXPECT_ERR(dgrad(B3B, s2, pl, nullptr, pl, nullptr, p16, 0), CATSEG_EINVAL, "conv bwd_data bf16x3 blocked: stride 1");
    EXPECT_ERR(dgrad(B3B, ok, off, nullptr, pl, nullptr, p16, 1), CATSEG_EINVAL, "conv bwd_data bf16x3 blocked: alignment");
    EXPECT_ERR(dgrad(B3B, big, pl, nullptr, pl, nullptr, p16, 0), CATSEG_EINVAL,
               "bf16x3 blocked planes: an operand's three planes must stay below 4 GB");
    EXPECT_ERR(wgrad(B3, c12, pl, nullptr, pl, nullptr, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight bf16x3: dense, Cin % 8 == 0");
    EXPECT_ERR(wgrad(B3, ok, off, nullptr, pl, nullptr, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight bf16x3: alignment");
    EXPECT_ERR(wgrad(B3, huge, pl, nullptr, pl, nullptr, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight bf16x3: 32-bit offsets");
    char msg[96];
    std::snprintf(msg, sizeof msg, "conv bwd_weight bf16x3: workspace 256 < %zu", catseg_conv2d_bwd_weight_workspace(&head, B3));
    EXPECT(catseg_conv2d_bwd_weight_workspace(&head, B3) > 256);
    EXPECT_ERR(wgrad(B3, head, pl, nullptr, pl, nullptr, p16, p16, 256), CATSEG_EWORKSPACE, msg);
    std::snprintf(msg, sizeof msg, "conv bwd_weight bf16x3: workspace %zu < %zu", (size_t)1 << 40, catseg_conv2d_bwd_weight_workspace(&head, B3));
    EXPECT_ERR(wgrad(B3, head, pl, nullptr, pl, nullptr, p16, nullptr, (size_t)1 << 40), CATSEG_EWORKSPACE, msg);   // null workspace

    const void* sc = p16;           // {amax bits, exponent}: never read on the host
    EXPECT_ERR(fwd(H2B, c24, pl, sc, pl, sc, nullptr, p16, 0), CATSEG_EINVAL,
               "conv fwd f16x2: needs Cin % 16 == 0");
    EXPECT_ERR(fwd(H2B, ok, off, sc, pl, sc, nullptr, p16, 0), CATSEG_EINVAL,
               "conv fwd f16x2: alignment");
    EXPECT_ERR(fwd(H2B, ok, pl, nullptr, pl, sc, nullptr, p16, 0), CATSEG_EINVAL,
               "conv fwd f16x2: alignment");
    EXPECT_ERR(fwd(H2B, ok, pl, sc, pl, sc, nullptr, p16, 0, p16, 64, &tr, nullptr), CATSEG_EINVAL,
               "conv fwd f16x2: tile_rows / n_tiles");
    tr = ntl = -1;
    EXPECT_ERR(fwd(H2B, huge, pl, sc, pl, sc, nullptr, p16, 0, p16, (size_t)1 << 40, &tr, &ntl), CATSEG_EINVAL,
               "f16x2 blocked planes: an operand's two planes must stay below 4 GB");
    EXPECT(tr == 256 && ntl == 64 * 1024 * 1024 / 256);                     // (claimed for 256-row tiles, then refused by the launcher)
    EXPECT_ERR(fwd(H2B, c24, pl, sc, pl, sc, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 1), CATSEG_EINVAL,
               "conv fwd fused f16x2: needs Cin % 16 == 0");
    EXPECT_ERR(fwd(H2B, ok, pl, sc, pl, sc, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, p16, 8, 0), CATSEG_EINVAL, "conv fwd fused f16x2: bad args");
    EXPECT_ERR(fwd(H2B, ok, pl, sc, pl, nullptr, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 1), CATSEG_EINVAL,
               "conv fwd fused f16x2: bad args");
    EXPECT_ERR(fwd(H2B, huge, pl, sc, pl, sc, nullptr, p16, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, 0), CATSEG_EINVAL,
               "f16x2 blocked planes: an operand's two planes must stay below 4 GB");
    EXPECT_ERR(dgrad(H2B, s2, pl, sc, pl, sc, p16, 0), CATSEG_EINVAL, "conv bwd_data f16x2: stride 1");
    EXPECT_ERR(dgrad(H2B, ok, pl, sc, off, sc, p16, 0), CATSEG_EINVAL, "conv bwd_data f16x2: alignment");
    EXPECT_ERR(dgrad(H2B, huge, pl, sc, pl, sc, p16, 1), CATSEG_EINVAL,
               "f16x2 blocked planes: an operand's two planes must stay below 4 GB");
    std::snprintf(msg, sizeof msg, "conv bwd_weight f16x2: workspace 256 < %zu", catseg_conv2d_bwd_weight_workspace(&head, H2P));
    for (int blocked = 0; blocked < 2; ++blocked) {
      const int h2 = blocked ? H2B : H2P;
      EXPECT_ERR(wgrad(h2, c12, pl, sc, pl, sc, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight f16x2: dense, Cin % 8 == 0");
      EXPECT_ERR(wgrad(h2, ok, pl, sc, off, sc, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight f16x2: alignment");
      EXPECT_ERR(wgrad(h2, ok, pl, sc, pl, nullptr, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight f16x2: alignment");
      EXPECT_ERR(wgrad(h2, huge, pl, sc, pl, sc, p16, nullptr, 0), CATSEG_EINVAL, "conv bwd_weight f16x2: an operand's two planes must stay below 4 GB");
      EXPECT_ERR(wgrad(h2, head, pl, sc, pl, sc, p16, p16, 256), CATSEG_EWORKSPACE, msg);
    }
  }
  EXPECT(catseg_lovasz_softmax(p16, (const int64_t*)p16, 100, 200, 1.0f, p16, nullptr, 0, p16, (size_t)1 << 30, nullptr) != CATSEG_OK);   // K > 64
  EXPECT(catseg_lovasz_softmax(p16, (const int64_t*)p16, 100, 8, 1.0f, p16, nullptr, 0, p16, 16, nullptr) != CATSEG_OK);                  // workspace too small
  EXPECT(catseg_maxpool2x2_fwd(p16, 6, p16, 8, (uint8_t*)p16, 1, 4, 4, 8, nullptr) != CATSEG_OK);        // row stride not 16-byte granular
  EXPECT(catseg_maxpool2x2_fwd(p16, 8, p16, 8, (uint8_t*)p16, 1, 1, 4, 8, nullptr) != CATSEG_OK);        // no output row
  EXPECT(catseg_maxpool2x2_bwd(p16, 8, nullptr, p16, 8, 1, 4, 4, 8, nullptr) != CATSEG_OK);
  EXPECT(catseg_bias_rows(p16, p16, 4, 10, 8, nullptr) != CATSEG_OK);                                    // ld < C
  EXPECT(catseg_bias_grad(p16, 8, 10, 8, p16, p16, 16, nullptr) != CATSEG_OK);                           // workspace too small
  EXPECT(catseg_axpy2d(p16, 6, p16, 8, 4, 6, 1.0f, 0, nullptr) != CATSEG_OK);
  EXPECT(catseg_dwgrad3(8, 16, 16, 50, p16, 50, p16, 50, p16, p16, 1 << 20, nullptr) != CATSEG_OK);       // unsupported width
  EXPECT(catseg_planes_from_f32(p16, 6, 10, 6, p16, p16, 1, nullptr) != CATSEG_OK);                      // C not a multiple of 8
  EXPECT(catseg_dconv3_pl(1, 8, 8, 50, p16, p16, p16, p16, nullptr, p16, 50, 0, nullptr, 0, nullptr, nullptr, nullptr) != CATSEG_OK);
  EXPECT(std::strlen(catseg_last_error()) > 0);

  // ---- debug knobs: out-of-range values are refused or clamped, defaults restored
  (void)catseg_debug_set_tile(99, 99);
  (void)catseg_debug_set_tile(0, 0);
  (void)catseg_debug_set_splits(-5);
  (void)catseg_debug_set_splits(0);
  (void)catseg_debug_set_dconv3_blocks(-1);
  (void)catseg_debug_set_dconv3_blocks(0);
  (void)catseg_debug_set_dwgrad3_blocks(1 << 30);
  (void)catseg_debug_set_dwgrad3_blocks(0);
  (void)catseg_debug_set_dconv3_pl_slots(-3);
  (void)catseg_debug_set_dconv3_pl_slots(512);
  (void)catseg_debug_set_b3_tile(7);
  (void)catseg_debug_set_b3_tile(0);
  for (const Shape& q : shapes) {     // the planner again after the knobs went through their extremes
    catseg_conv_desc d = desc(q.B, q.H, q.W, q.Cin, q.Cout, q.k, q.s, q.p, q.d);
    int out[8];
    EXPECT(catseg_debug_plan_conv(&d, 2, out) == CATSEG_OK);
  }
  std::printf("%s %d checks, %d failed\n", failed ? "FAILED" : "ok", checks, failed);
  return failed ? 1 : 0;
}
