// What PointRend's point kernels share (csrc/pointrend.hip: the eval-mode gather at cell centres; csrc/pointrend_train.hip: the train-mode
// kernels at arbitrary coordinates): point_sample's 2 p - 1, F.grid_sample's four bilinear taps with ZERO padding, and the sweep of one
// point's channels by one wave.  Every kernel that includes this file places a point's taps and forms their weights with the same
// instructions, so the same point gets the same bits in all of them.  Those instructions are NOT one rounding per operation: hipcc
// contracts a * b + c by default and __fmul_rn / __fadd_rn / __fsub_rn are plain operators to it, so (g + 1) (size / 2) - 0.5 is one
// v_fmamk (2 p - 1 as well, where fusing changes nothing: 2 p is exact).  The eval-mode gather has had these bits since it was written and
// keeps them; against torch's two roundings a tap position differs by at most one ulp, which the tests' fp64 bars cover.  Where a result
// is an integer that is compared exactly (pixel index, nearest label: csrc/pointrend_train.hip) the expressions switch contraction off.
#pragma once
#include "common.h"

constexpr int PR_MAXSRC = 5;
constexpr int PR_MAXDST = 4;

struct PrGather {                 // by value in the kernel arguments: nothing to upload, capturable
  const float* src[PR_MAXSRC];
  int ld[PR_MAXSRC], H[PR_MAXSRC], W[PR_MAXSRC], C[PR_MAXSRC], off[PR_MAXSRC];     // off: first column of the source's block in the point row
  int vec[PR_MAXSRC];             // the source's pixels are 16-byte aligned and hold C rounded up to 4 readable floats: 16-byte loads
  int nsrc;
  float* extra[PR_MAXDST];        // further destinations of the LAST source's block (the coarse logits)
  int extra_ld[PR_MAXDST], extra_off[PR_MAXDST];
  int nextra;
};

// point_sample: the grid coordinate 2 p - 1 of a point coordinate p in [0, 1]
__device__ __forceinline__ float pr_grid(float p) { return __fsub_rn(__fmul_rn(2.f, p), 1.f); }

// grid_sample, align_corners = False: ((g + 1) * size - 1) / 2 = (g + 1) * (size / 2) - 0.5
__device__ __forceinline__ float pr_unnormalize(float g, int size) { return __fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), 0.5f * (float)size), 0.5f); }

struct PrTaps {                   // the four taps of one point in one H x W map: nw, ne, sw, se
  int x0, y0;                     // the nw tap; ne = (x0 + 1, y0), sw = (x0, y0 + 1), se = (x0 + 1, y0 + 1)
  float w[4];
  bool ok[4];                     // the tap lies inside the map (zero padding: a tap outside contributes nothing)
};

__device__ __forceinline__ PrTaps pr_taps(float gx, float gy, int Hs, int Ws) {
  PrTaps t;
  const float ix = pr_unnormalize(gx, Ws), iy = pr_unnormalize(gy, Hs);
  const float fx = floorf(ix), fy = floorf(iy);
  t.x0 = (int)fx;
  t.y0 = (int)fy;
  const int x1 = t.x0 + 1, y1 = t.y0 + 1;
  const float tx1 = ix - fx, ty1 = iy - fy, tx0 = (fx + 1.f) - ix, ty0 = (fy + 1.f) - iy;
  t.w[0] = tx0 * ty0;
  t.w[1] = tx1 * ty0;
  t.w[2] = tx0 * ty1;
  t.w[3] = tx1 * ty1;
  const bool vx0 = t.x0 >= 0 && t.x0 < Ws, vx1 = x1 >= 0 && x1 < Ws, vy0 = t.y0 >= 0 && t.y0 < Hs, vy1 = y1 >= 0 && y1 < Hs;
  t.ok[0] = vy0 && vx0;
  t.ok[1] = vy0 && vx1;
  t.ok[2] = vy1 && vx0;
  t.ok[3] = vy1 && vx1;
  return t;
}

// One wave writes row p of the point matrix: the blocks of all sources of image b sampled at the grid coordinate (gx, gy).
__device__ __forceinline__ void pr_gather_point(const PrGather& g, int b, long long p, float gx, float gy, float* __restrict__ out, int ldo, int lane) {
  float* orow = out + p * ldo;
  for (int s = 0; s < g.nsrc; ++s) {
    const int Hs = g.H[s], Ws = g.W[s], C = g.C[s], ld = g.ld[s];
    const PrTaps t = pr_taps(gx, gy, Hs, Ws);
    const float wnw = t.w[0], wne = t.w[1], wsw = t.w[2], wse = t.w[3];
    const float* base = g.src[s] + (long long)b * Hs * Ws * ld;
    const float* pnw = base + ((long long)t.y0 * Ws + t.x0) * ld;
    const float* pne = pnw + ld;
    const float* psw = pnw + (long long)Ws * ld;
    const float* pse = psw + ld;
    const bool last = s == g.nsrc - 1;
    const int Cq = (C + 3) & ~3;
    if (!g.vec[s]) {                                  // dense K-class logits (ld = K, K % 4 != 0): one channel per lane
      for (int c = lane; c < Cq; c += 64) {
        float v = 0.f;                                // pad columns of the block: zero
        if (c < C) {
          const float a = t.ok[0] ? pnw[c] : 0.f, bq = t.ok[1] ? pne[c] : 0.f;      // zero padding: a tap outside the map is 0
          const float cq = t.ok[2] ? psw[c] : 0.f, dq = t.ok[3] ? pse[c] : 0.f;
          v = a * wnw + bq * wne + cq * wsw + dq * wse;
        }
        orow[g.off[s] + c] = v;
        if (last)
          for (int q = 0; q < g.nextra; ++q) g.extra[q][p * g.extra_ld[q] + g.extra_off[q] + c] = v;
      }
      continue;
    }
    for (int c = lane * 4; c < Cq; c += 256) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const f32x4 a = t.ok[0] ? *(const f32x4*)(pnw + c) : z;       // zero padding: a tap outside the map is 0
      const f32x4 bq = t.ok[1] ? *(const f32x4*)(pne + c) : z;
      const f32x4 cq = t.ok[2] ? *(const f32x4*)(psw + c) : z;
      const f32x4 dq = t.ok[3] ? *(const f32x4*)(pse + c) : z;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (c + e < C) ? (a[e] * wnw + bq[e] * wne + cq[e] * wsw + dq[e] * wse) : 0.f;      // pad columns of the block: zero
      *(f32x4*)(orow + g.off[s] + c) = v;
      if (last)
        for (int q = 0; q < g.nextra; ++q) *(f32x4*)(g.extra[q] + p * g.extra_ld[q] + g.extra_off[q] + c) = v;
    }
  }
}
