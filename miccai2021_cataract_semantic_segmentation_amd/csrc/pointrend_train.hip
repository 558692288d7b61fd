// PointRend's train-mode forward and backward (reference: models/PointRend.py:43-73, utils/pointrend_utils.py:65-116,
// managers/EncDec_Manager.py:158-177), the parts that are not a convolution, a resize or a loss:
//   catseg_pointrend_draw              [N, M, 2] uniforms in [0, 1) with Philox4x32-10 from 16 bytes of DEVICE state; the same launch advances the
//                                      draw counter (as catseg_dropout2d_mask does), so a captured step draws the next points at every replay
//   catseg_pointrend_point_uncertainty per candidate point the bilinear zero-padded sample of the K coarse logits and second-largest - largest
//                                      of the K sampled values; the [N, K, M] samples are never written
//   catseg_pointrend_compose           coords = the selected candidates, then the random rest; per point its pixel of the full-size map (the
//                                      reference's fp32 arithmetic, round half to even) and its label (grid_sample, mode = 'nearest', zeros)
//   catseg_pointrend_gather_bwd        dX [N P, cols] -> the gradients of up to five NHWC sources, WITHOUT floating-point atomics: per (image,
//                                      source) the 4 P tap pixels are staged in LDS, one wave takes a tap; a tap whose pixel occurs at a lower
//                                      tap number leaves, the first tap of a pixel (its leader) collects the pixel's taps by ballot in
//                                      ascending tap order and sweeps the channels with 16-byte accesses.  Every pixel's sum is formed by one
//                                      wave in one fixed order: two launches give the same bits.
//   catseg_pointrend_scatter_last      seg[b, pix[b, p], :] = rows[b, p, :] where the HIGHEST p of a pixel writes (scatter_ on the CPU: the last
//                                      point wins); an O(P^2) comparison in LDS, no race
//   catseg_pointrend_scatter_bwd       d_rows[b, p, :] (+)= dseg[b, pix[b, p], :] for EVERY p (duplicates included), then dseg = 0 at every
//                                      scattered pixel (the interpolate output receives no gradient there)
// (the gather at coordinates itself is catseg_pointrend_gather_at, csrc/pointrend.hip: it shares the eval-mode gather's sweep)
// Nothing here synchronises with the host, allocates or touches host memory.
#include "philox.h"
#include "pointrend_taps.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- draw
// ONE block (the state is read by every thread in front of the barrier and advanced by thread 0 behind it).  Float i of the output takes word
// i & 3 of philox4x32_10(counter = (i >> 2, draw, PHILOX_STREAM_POINTS, layer | rank << 16), key = (seed lo, seed hi)); u = (word >> 8) 2^-24.
constexpr int kDrawThreads = 256;
__global__ __launch_bounds__(kDrawThreads) void pr_draw_kernel(unsigned* __restrict__ state, const float* __restrict__ fixed, int total,
                                                               float* __restrict__ out) {
  if (fixed != nullptr) {                             // the test knob: the given coordinates, the state does not move
    for (int i = threadIdx.x; i < total; i += kDrawThreads) out[i] = fixed[i];
    return;
  }
  const unsigned s0 = state[0], s1 = state[1], s2 = state[2], draw = state[3];
  __syncthreads();
  if (threadIdx.x == 0) state[3] = draw + 1u;
  const int groups = (total + 3) >> 2;
  for (int q = threadIdx.x; q < groups; q += kDrawThreads) {
    const ph_u32x4 r = philox4x32_10(ph_u32x4{(unsigned)q, draw, PHILOX_STREAM_POINTS, s2}, s0, s1);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < total) out[4 * q + e] = (float)(r[e] >> 8) * 0x1p-24f;
  }
}

// ---------------------------------------------------------------------------------------------------------------- candidate uncertainty
// One thread per candidate: its four taps are four rows of K consecutive floats.
__global__ __launch_bounds__(256) void pr_point_uncertainty_kernel(const float* __restrict__ coarse, int ld, int H, int W, int K,
                                                                   const float* __restrict__ coords, int M, long long total,
                                                                   float* __restrict__ unc) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / M);
  const PrTaps t = pr_taps(pr_grid(coords[2 * i]), pr_grid(coords[2 * i + 1]), H, W);
  const float* pnw = coarse + (((long long)b * H + t.y0) * W + t.x0) * ld;
  const float* pne = pnw + ld;
  const float* psw = pnw + (long long)W * ld;
  const float* pse = psw + ld;
  float m1 = -INFINITY, m2 = -INFINITY;               // largest and second-largest (torch.topk(k = 2): equal values count twice)
  for (int c = 0; c < K; ++c) {                       // the K real columns only: pad columns never take part
    const float a = t.ok[0] ? pnw[c] : 0.f, bq = t.ok[1] ? pne[c] : 0.f, cq = t.ok[2] ? psw[c] : 0.f, dq = t.ok[3] ? pse[c] : 0.f;
    const float v = a * t.w[0] + bq * t.w[1] + cq * t.w[2] + dq * t.w[3];
    if (v > m1) {
      m2 = m1;
      m1 = v;
    } else if (v > m2) {
      m2 = v;
    }
  }
  unc[i] = m2 - m1;
}

// ---------------------------------------------------------------------------------------------------------------- compose
// One thread per point.  models/PointRend.py:56-57: round(y (h - 1)) w + round(x (w - 1)), every operation an fp32 tensor operation
// (torch.round rounds half to even, as rintf does), then .long().  The label: F.grid_sample(mode = 'nearest', align_corners = False, zeros).
// Both results are integers that the tests compare exactly, so the products and sums in front of the roundings must round one by one:
// hipcc contracts a * b + c by default, and __fmul_rn / __fadd_rn are plain operators to it, hence the pragma.
__device__ __forceinline__ float pr_pixel_index(float x, float y, int h, int w) {
#pragma clang fp contract(off)
  const float ry = rintf(y * (float)(h - 1)), rx = rintf(x * (float)(w - 1));
  const float rows = ry * (float)w;
  return rows + rx;
}

__device__ __forceinline__ float pr_nearest(float p, int size) {      // the tap of grid_sample(mode = 'nearest') at point coordinate p
#pragma clang fp contract(off)
  const float g = 2.f * p - 1.f;                      // (exact bar the subtraction's rounding, fused or not)
  const float up = g + 1.f;
  const float scaled = up * (0.5f * (float)size);
  return rintf(scaled - 0.5f);
}

__global__ __launch_bounds__(256) void pr_compose_kernel(const float* __restrict__ cand, int M, const int* __restrict__ sel, int kb,
                                                         const float* __restrict__ rest, int P, long long total, int h, int w,
                                                         const long long* __restrict__ lbl, int Hl, int Wl, float* __restrict__ coords,
                                                         int* __restrict__ pix, long long* __restrict__ labels) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / P), p = (int)(i - (long long)b * P);
  const float* src;
  if (p < kb) {
    int j = sel[(long long)b * kb + p];
    j = j < 0 ? 0 : (j >= M ? M - 1 : j);             // (the selection's indices lie in [0, M); a corrupt one stays inside the table)
    src = cand + ((long long)b * M + j) * 2;
  } else {
    src = rest + ((long long)b * (P - kb) + (p - kb)) * 2;
  }
  const float x = src[0], y = src[1];
  coords[2 * i] = x;
  coords[2 * i + 1] = y;
  const float fpix = pr_pixel_index(x, y, h, w);
  const long long hw = (long long)h * w;
  pix[i] = (fpix >= 0.f && fpix < (float)hw) ? (int)fpix : -1;      // (-1: a point outside [0, 1]^2 scatters nothing)
  if (labels != nullptr) {
    const float lx = pr_nearest(x, Wl), ly = pr_nearest(y, Hl);
    long long v = 0;                                  // a tap outside the map yields 0.0: class 0
    if (lx >= 0.f && lx < (float)Wl && ly >= 0.f && ly < (float)Hl) v = lbl[((long long)b * Hl + (int)ly) * Wl + (int)lx];
    labels[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather backward
struct PrScatterAdd {             // by value in the kernel arguments
  float* dst[PR_MAXSRC];
  int ld[PR_MAXSRC], H[PR_MAXSRC], W[PR_MAXSRC], C[PR_MAXSRC], off[PR_MAXSRC], acc[PR_MAXSRC];
  int nsrc;
};

__global__ __launch_bounds__(256) void pr_zero_rows_kernel(float* __restrict__ p, long long quads) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) *(f32x4*)(p + 4 * i) = z;
}

constexpr int GB_WAVES = 4;                           // waves per block
constexpr int GB_TAPS = 16;                           // taps per wave
constexpr int GB_CHUNKS = 8;                          // 16-byte channel groups a lane keeps in registers: 8 x 64 x 4 = 2048 channels per sweep
constexpr int GB_SCAN = 256;                          // staged pixels a wave compares per scan step: four per lane, one 16-byte LDS read

// grid (tap groups, N, sources).  Every block stages the pixel of each of the image's T = 4 P taps in this source (-1: outside the map);
// its waves then take GB_TAPS taps each.  Tap number t = 4 p + corner (nw, ne, sw, se); lane l of a scan step holds taps j0 + 4 l .. + 3.
__global__ __launch_bounds__(64 * GB_WAVES) void pr_gather_bwd_kernel(PrScatterAdd g, const float* __restrict__ coords, int P,
                                                                      const float* __restrict__ dX, int ldx) {
  extern __shared__ int4 pr_tap_pix4[];               // [T rounded up to GB_SCAN] ints
  int* pr_tap_pix = (int*)pr_tap_pix4;
  const int b = blockIdx.y, s = blockIdx.z;
  const int Hs = g.H[s], Ws = g.W[s], C = g.C[s], ld = g.ld[s];
  const int T = 4 * P, Tq = (T + GB_SCAN - 1) / GB_SCAN * GB_SCAN;
  const float* xy = coords + (long long)b * P * 2;
  for (int t = threadIdx.x; t < Tq; t += blockDim.x) {
    int px = -1;
    if (t < T) {
      const int p = t >> 2, corner = t & 3;
      const PrTaps tp = pr_taps(pr_grid(xy[2 * p]), pr_grid(xy[2 * p + 1]), Hs, Ws);
      const int x = tp.x0 + (corner & 1), y = tp.y0 + (corner >> 1);
      if (x >= 0 && x < Ws && y >= 0 && y < Hs) px = y * Ws + x;
    }
    pr_tap_pix[t] = px;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Cq = (C + 3) & ~3;
  const bool acc = g.acc[s] != 0;
  const float* dXb = dX + (long long)b * P * ldx + g.off[s];
  const int t0 = (blockIdx.x * GB_WAVES + wave) * GB_TAPS;
  for (int t = t0; t < t0 + GB_TAPS && t < T; ++t) {  // (t is the same in every lane of a wave)
    const int mine = pr_tap_pix[t];
    if (mine < 0) continue;                           // a tap outside the map is dropped
    float* drow = g.dst[s] + ((long long)b * Hs * Ws + mine) * ld;
    for (int cg = 0; cg < Cq; cg += GB_CHUNKS * 256) {
      f32x4 sum[GB_CHUNKS];
#pragma unroll
      for (int q = 0; q < GB_CHUNKS; ++q) sum[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      bool leader = true;
      for (int j0 = 0; j0 < Tq; j0 += GB_SCAN) {
        const int4 v = pr_tap_pix4[(j0 >> 2) + lane];
        const int bits = (v.x == mine ? 1 : 0) | (v.y == mine ? 2 : 0) | (v.z == mine ? 4 : 0) | (v.w == mine ? 8 : 0);
        unsigned long long m = __ballot(bits != 0);
        if (m == 0ull) continue;
        const int l0 = __ffsll((long long)m) - 1;
        if (j0 + 4 * l0 + (__ffs(__shfl(bits, l0, 64)) - 1) < t) {      // the pixel occurs at a lower tap number: that tap's wave forms the sum
          leader = false;
          break;
        }
        while (m) {                                   // the pixel's taps of this step, ascending: lane by lane, within a lane bit by bit
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          int lb = __shfl(bits, l, 64);
          while (lb) {
            const int j = j0 + 4 * l + (__ffs(lb) - 1);
            lb &= lb - 1;
            const int p = j >> 2, corner = j & 3;
            const PrTaps tp = pr_taps(pr_grid(xy[2 * p]), pr_grid(xy[2 * p + 1]), Hs, Ws);
            const float wt = corner == 0 ? tp.w[0] : corner == 1 ? tp.w[1] : corner == 2 ? tp.w[2] : tp.w[3];
            const float* xr = dXb + (long long)p * ldx;
#pragma unroll
            for (int q = 0; q < GB_CHUNKS; ++q) {
              const int c = cg + q * 256 + lane * 4;
              if (c < Cq) {
                const f32x4 x4 = *(const f32x4*)(xr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[q][e] += wt * x4[e];
              }
            }
          }
        }
      }
      if (!leader) break;
#pragma unroll
      for (int q = 0; q < GB_CHUNKS; ++q) {
        const int c = cg + q * 256 + lane * 4;
        if (c < Cq) {
          f32x4 v = sum[q];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (c + e >= C) v[e] = 0.f;               // the pad columns of the point matrix carry no gradient
          if (acc) v += *(const f32x4*)(drow + c);
          *(f32x4*)(drow + c) = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- scatter, its backward
// grid (point groups of 64, N): the image's P pixels in LDS; a wave takes SL_POINTS points in turn and compares the pixels of the LATER
// points with its point's, 64 per step; a point with a later point on its pixel does not write.
constexpr int SL_POINTS = 16;
__global__ __launch_bounds__(256) void pr_scatter_last_kernel(const float* __restrict__ rows, int ldr, const int* __restrict__ pix, int P, long long hw,
                                                              float* __restrict__ seg, int lds, int K) {
  extern __shared__ int pr_pix[];
  const int b = blockIdx.y;
  const int* pb = pix + (long long)b * P;
  for (int i = threadIdx.x; i < P; i += 256) pr_pix[i] = pb[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p0 = (blockIdx.x * 4 + wave) * SL_POINTS;
  for (int p = p0; p < p0 + SL_POINTS && p < P; ++p) {          // (p is the same in every lane of a wave)
    const int mine = pr_pix[p];
    if (mine < 0 || mine >= hw) continue;             // (a pixel outside the map writes nothing)
    bool later = false;
    for (int j0 = p + 1; j0 < P && !later; j0 += 64) {
      const int j = j0 + lane;
      later = __ballot(j < P && pr_pix[j] == mine) != 0ull;
    }
    if (later) continue;
    const float* r = rows + ((long long)b * P + p) * ldr;
    float* d = seg + ((long long)b * hw + mine) * lds;
    for (int c = lane; c < K; c += 64) d[c] = r[c];
  }
}

__global__ __launch_bounds__(256) void pr_scatter_bwd_read_kernel(const float* __restrict__ dseg, int lds, const int* __restrict__ pix, int P,
                                                                  long long npts, long long hw, float* __restrict__ drows, int ldr, int K, int acc) {
  const long long total = npts * K;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long p = i / K;
    const int c = (int)(i - p * K);
    const long long b = p / P;
    const long long px = pix[p];
    const float g = (px >= 0 && px < hw) ? dseg[(b * hw + px) * lds + c] : 0.f;
    float* d = drows + p * ldr + c;
    *d = acc ? *d + g : g;
  }
}

__global__ __launch_bounds__(256) void pr_scatter_bwd_zero_kernel(float* __restrict__ dseg, int lds, const int* __restrict__ pix, int P, long long npts,
                                                                  long long hw, int K) {
  const long long total = npts * K;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long p = i / K;
    const int c = (int)(i - p * K);
    const long long b = p / P;
    const long long px = pix[p];
    if (px >= 0 && px < hw) dseg[(b * hw + px) * lds + c] = 0.f;      // (duplicates store the same zero)
  }
}

}  // namespace

extern "C" int catseg_pointrend_draw(void* state, const float* fixed, int N, int M, float* out, catseg_stream_t stream) {
  CS_REQUIRE(N >= 1 && M >= 1 && (long long)N * M < (1ll << 29), "pointrend draw: N, M >= 1 and fewer than 2^29 points");
  CS_REQUIRE(out && (state || fixed), "pointrend draw: the output and either the state or fixed coordinates are required");
  CS_REQUIRE(fixed || (((uintptr_t)state) & 15) == 0, "pointrend draw: the state is 16 bytes of device memory, 16-byte aligned");
  hipLaunchKernelGGL(pr_draw_kernel, dim3(1), dim3(kDrawThreads), 0, (hipStream_t)stream, (unsigned*)state, fixed, N * M * 2, out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_point_uncertainty(const float* coarse, int ld, int N, int H, int W, int K, const float* coords, int M,
                                                  float* uncertainty, catseg_stream_t stream) {
  CS_REQUIRE(coarse && coords && uncertainty && N > 0 && H > 0 && W > 0 && M > 0, "pointrend point uncertainty: bad args");
  CS_REQUIRE(K >= 2, "pointrend point uncertainty: the difference of the two largest logits needs K >= 2 classes (got %d)", K);
  CS_REQUIRE(ld >= K, "pointrend point uncertainty: ld (%d) < K (%d)", ld, K);
  CS_REQUIRE((long long)N * H * W * ld < (1ll << 40) && (long long)N * M < (1ll << 31), "pointrend point uncertainty: too large");
  const long long total = (long long)N * M;
  hipLaunchKernelGGL(pr_point_uncertainty_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coarse, ld, H, W, K, coords, M,
                     total, uncertainty);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_compose(const float* cand, int M, const int* sel, int kb, const float* rest, int N, int P, int h, int w,
                                        const long long* lbl, int Hl, int Wl, float* coords, int* pix, long long* labels, catseg_stream_t stream) {
  CS_REQUIRE(N > 0 && P > 0 && kb >= 0 && kb <= P && (long long)N * P < (1ll << 31), "pointrend compose: N, P > 0 and 0 <= selected <= P (N %d, P %d, selected %d)", N, P, kb);
  CS_REQUIRE(kb == 0 || (cand && sel && M >= kb), "pointrend compose: %d selected points need the candidates, the selection and M >= %d (got %d)", kb, kb, M);
  CS_REQUIRE(kb == P || rest, "pointrend compose: the %d random points are missing", P - kb);
  CS_REQUIRE(h > 0 && w > 0 && (long long)h * w < (1ll << 24), "pointrend compose: the pixel index is formed in fp32 as the reference forms it: h w < 2^24 (got %d x %d)", h, w);
  CS_REQUIRE(coords && pix, "pointrend compose: coords and pix are required");
  CS_REQUIRE((labels == nullptr) == (lbl == nullptr) && (lbl == nullptr || (Hl > 0 && Wl > 0)), "pointrend compose: labels need a label map (and the other way round)");
  const long long total = (long long)N * P;
  hipLaunchKernelGGL(pr_compose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cand, M, sel, kb, rest, P, total, h, w, lbl,
                     Hl, Wl, coords, pix, labels);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_gather_bwd(const catseg_pointrend_gather_bwd_desc* d, catseg_stream_t stream) {
  CS_REQUIRE(d, "pointrend gather backward: null descriptor");
  CS_REQUIRE(d->n_sources >= 1 && d->n_sources <= PR_MAXSRC, "pointrend gather backward: 1 to %d sources (got %d)", PR_MAXSRC, d->n_sources);
  CS_REQUIRE(d->N > 0 && d->N <= 65535 && d->P > 0, "pointrend gather backward: 1 <= N <= 65535, P >= 1 (N %d, P %d)", d->N, d->P);
  const size_t lds = (size_t)((4 * (long long)d->P + GB_SCAN - 1) / GB_SCAN * GB_SCAN) * 4;
  CS_REQUIRE(lds <= CS_LDS_QUICK, "pointrend gather backward: the taps of an image are staged in LDS: P <= %d (got %d)", (int)(CS_LDS_QUICK / 16), d->P);
  CS_REQUIRE(d->coords && d->dx && cs_aligned16(d->dx) && d->ld_dx % 4 == 0, "pointrend gather backward: coords and a 16-byte aligned dX with ld %% 4 == 0 are required");
  PrScatterAdd g = {};
  int col = 0;
  for (int s = 0; s < d->n_sources; ++s) {
    const int Cq = (d->C[s] + 3) & ~3;
    CS_REQUIRE(d->dst[s] != nullptr, "pointrend gather backward: destination %d is NULL", s);
    CS_REQUIRE(d->H[s] > 0 && d->W[s] > 0 && d->C[s] > 0 && (long long)d->H[s] * d->W[s] < (1ll << 31), "pointrend gather backward: destination %d needs H, W, C > 0", s);
    CS_REQUIRE(cs_aligned16(d->dst[s]) && d->ld[s] % 4 == 0 && d->ld[s] >= Cq,
               "pointrend gather backward: destination %d: 16-byte aligned pixels of ld %% 4 == 0 floats that hold C rounded up to 4 (C %d, ld %d)", s, d->C[s], d->ld[s]);
    CS_REQUIRE((long long)d->N * d->H[s] * d->W[s] * d->ld[s] < (1ll << 40), "pointrend gather backward: destination %d too large", s);
    g.dst[s] = d->dst[s]; g.ld[s] = d->ld[s]; g.H[s] = d->H[s]; g.W[s] = d->W[s]; g.C[s] = d->C[s]; g.off[s] = col; g.acc[s] = d->accumulate[s] ? 1 : 0;
    col += Cq;
  }
  CS_REQUIRE(d->ld_dx >= col, "pointrend gather backward: dX has ld %d, the blocks need %d columns", d->ld_dx, col);
  g.nsrc = d->n_sources;
  hipStream_t st = (hipStream_t)stream;
  for (int s = 0; s < d->n_sources; ++s)
    if (!g.acc[s]) {                                  // written, not accumulated: the pixels no tap touches are zero
      const long long quads = (long long)d->N * d->H[s] * d->W[s] * d->ld[s] / 4;
      hipLaunchKernelGGL(pr_zero_rows_kernel, dim3(cs_grid_256(quads, 16384)), dim3(256), 0, st, g.dst[s], quads);
    }
  const int T = 4 * d->P, per_block = GB_WAVES * GB_TAPS;
  hipLaunchKernelGGL(pr_gather_bwd_kernel, dim3((unsigned)((T + per_block - 1) / per_block), (unsigned)d->N, (unsigned)d->n_sources), dim3(64 * GB_WAVES), lds, st,
                     g, d->coords, d->P, d->dx, d->ld_dx);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_scatter_last(const float* rows, int ld_rows, const int* pix, int N, int P, long long hw, float* seg, int ld_seg, int K,
                                             catseg_stream_t stream) {
  CS_REQUIRE(rows && pix && seg && N > 0 && N <= 65535 && P > 0 && hw > 0 && hw < (1ll << 31) && K > 0 && ld_rows >= K && ld_seg >= K,
             "pointrend scatter (last point wins): bad args");
  const size_t lds = (size_t)P * 4;
  CS_REQUIRE(lds <= CS_LDS_QUICK, "pointrend scatter (last point wins): the pixels of an image are staged in LDS: P <= %d (got %d)", (int)(CS_LDS_QUICK / 4), P);
  hipLaunchKernelGGL(pr_scatter_last_kernel, dim3((unsigned)((P + 4 * SL_POINTS - 1) / (4 * SL_POINTS)), (unsigned)N), dim3(256), lds, (hipStream_t)stream, rows, ld_rows, pix, P, hw, seg,
                     ld_seg, K);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_scatter_bwd(float* dseg, int ld_seg, const int* pix, int N, int P, long long hw, float* drows, int ld_rows, int K,
                                            int accumulate, catseg_stream_t stream) {
  CS_REQUIRE(dseg && pix && drows && N > 0 && P > 0 && hw > 0 && hw < (1ll << 31) && K > 0 && ld_rows >= K && ld_seg >= K,
             "pointrend scatter backward: bad args");
  const long long npts = (long long)N * P, total = npts * K;
  hipStream_t st = (hipStream_t)stream;
  // two launches: every point has read its pixel's gradient before any pixel is cleared (duplicates read the same pixel)
  hipLaunchKernelGGL(pr_scatter_bwd_read_kernel, dim3(cs_grid_256(total, 16384)), dim3(256), 0, st, (const float*)dseg, ld_seg, pix, P, npts, hw, drows, ld_rows,
                     K, accumulate ? 1 : 0);
  hipLaunchKernelGGL(pr_scatter_bwd_zero_kernel, dim3(cs_grid_256(total, 16384)), dim3(256), 0, st, dseg, ld_seg, pix, P, npts, hw, K);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
