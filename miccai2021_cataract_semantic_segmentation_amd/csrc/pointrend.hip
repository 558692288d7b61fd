// PointRend's eval-mode refinement (reference: models/PointRend.py:74-90, utils/pointrend_utils.py:25-46,119-148,220-232), the parts that are
// not a convolution:
//   catseg_pointrend_uncertainty second-largest - largest logit per pixel, from the K real columns of the rows the resize launch stored,
//                                256 rows per block staged through LDS
//                                (catseg_bilinear_fwd itself writes the 2x logits: which of its kernels a shape takes, and how the compiler
//                                contracted that kernel's lerp, decides the last bit of a logit, so no second kernel can promise its bits)
//   catseg_pointrend_topk        per image the k most uncertain of h w pixels.  A radix select on the 64-bit key (order-preserving bits of u,
//                                complemented pixel index): all keys differ, so among equal uncertainties the LOWER pixel index wins
//                                (-0.0 == +0.0), whatever the launch order.  Four histogram passes over the 32 value bits fix the k-th VALUE
//                                and how many of its equals are taken; a count pass and an ordered emit pass write the indices ascending.  No
//                                host synchronisation, no allocation, no atomics on the output: capturable, the same list on every launch.
//   catseg_pointrend_gather      per (image, point): the cell centre in [0, 1]^2 as the reference forms it in fp32, F.grid_sample's bilinear taps
//                                with ZERO padding (a tap at -1 or at the map's size contributes nothing: points in the outer half cell of a
//                                coarse map are attenuated, not clamped) from up to five NHWC maps, written as one row of the point matrix; the
//                                last source's block (the coarse logits) also goes to the buffers that later layers concatenate it to
//   catseg_pointrend_scatter     seg[b, idx[b, p], 0:K] = rows[b, p, 0:K]
// One wave sweeps a point's channels with 16-byte loads (NHWC: a pixel's channels are contiguous).
#include "lerp.h"
#include "pointrend_taps.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_ITEMS = 8;                           // candidates per thread and block
constexpr int TK_CHUNK = TK_THREADS * TK_ITEMS;       // candidates per block
constexpr int TK_PASSES = 4;                          // 8 bits of the value per pass

// ---------------------------------------------------------------------------------------------------------------- uncertainty
// A block takes 256 consecutive pixels: their rows are one contiguous span of 256 ldy floats, read with consecutive lanes on consecutive
// floats (a lane walking its own row would touch a new cache line per load: rows are 100 bytes apart at K = 25) and staged through LDS with
// an odd row stride, so that lane t walking row t meets no bank conflict.  STAGED = false: rows too wide for LDS, read from global memory.
template <bool STAGED>
__global__ __launch_bounds__(256) void pr_uncertainty_kernel(const float* __restrict__ y, int ldy, float* __restrict__ unc, long long pixels, int K,
                                                             int LS) {
  extern __shared__ float pr_rows[];
  const long long p0 = (long long)blockIdx.x * 256;
  const int np = (int)min((long long)256, pixels - p0);
  const float* r = y + (p0 + threadIdx.x) * ldy;
  if (STAGED) {
    const float* g = y + p0 * ldy;
    const int n = np * ldy;
    for (int i = threadIdx.x; i < n; i += 256) {
      const int row = i / ldy, c = i - row * ldy;
      if (c < K) pr_rows[row * LS + c] = g[i];        // the K real columns only: pad columns never take part
    }
    __syncthreads();
    r = pr_rows + threadIdx.x * LS;
  }
  if ((int)threadIdx.x < np) {
    float m1 = -INFINITY, m2 = -INFINITY;             // largest and second-largest (torch.topk(k = 2): equal values count twice)
    for (int c = 0; c < K; ++c) {
      const float v = r[c];
      if (v > m1) {
        m2 = m1;
        m1 = v;
      } else if (v > m2) {
        m2 = v;
      }
    }
    unc[p0 + threadIdx.x] = m2 - m1;
  }
}

// ---------------------------------------------------------------------------------------------------------------- top-k
__global__ __launch_bounds__(256) void pr_zero_kernel(unsigned* __restrict__ p, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

// order-preserving bits of an uncertainty: a > b  <=>  key(a) > key(b); -0.0 is +0.0
__device__ __forceinline__ unsigned pr_key(float u) {
  unsigned b = __float_as_uint(u);
  if (u == 0.f) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// What the histograms of the first `npass` passes decide: the leading 8 npass bits of the k-th largest key (`prefix`) and how many keys are
// still to be taken among those that share them (`krem` >= 1).  Every block of a launch recomputes it from the histograms its predecessors
// completed (256 threads, a suffix sum of 256 bins per pass): there is no launch in between.  Called by all TK_THREADS threads.
__device__ __forceinline__ void pr_resolve(const unsigned* __restrict__ hist, int npass, unsigned k, unsigned& prefix, unsigned& krem) {
  __shared__ unsigned s_sum[TK_THREADS];
  __shared__ unsigned s_out[2];
  const int t = threadIdx.x;
  prefix = 0u;
  krem = k;
  for (int q = 0; q < npass; ++q) {
    const unsigned h = hist[q * 256 + t];
    s_sum[t] = h;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {               // inclusive suffix sum: s_sum[t] = sum of bins >= t
      const unsigned add = (t + o < 256) ? s_sum[t + o] : 0u;
      __syncthreads();
      s_sum[t] += add;
      __syncthreads();
    }
    const unsigned above = s_sum[t] - h;              // keys in larger bins
    if (above < krem && s_sum[t] >= krem) {           // exactly one bin holds the krem-th largest
      s_out[0] = (unsigned)t;
      s_out[1] = krem - above;
    }
    __syncthreads();
    prefix = (prefix << 8) | s_out[0];
    krem = s_out[1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(TK_THREADS) void pr_topk_hist_kernel(const float* __restrict__ unc, long long n, unsigned k, int pass,
                                                                  unsigned* __restrict__ ws, size_t ws_words_per_image) {
  __shared__ unsigned s_hist[256];
  unsigned* hist = ws + (size_t)blockIdx.y * ws_words_per_image;
  const float* u = unc + (long long)blockIdx.y * n;
  unsigned prefix, krem;
  pr_resolve(hist, pass, k, prefix, krem);
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const long long i0 = (long long)blockIdx.x * TK_CHUNK;
#pragma unroll
  for (int j = 0; j < TK_ITEMS; ++j) {
    const long long i = i0 + j * TK_THREADS + threadIdx.x;
    if (i < n) {
      const unsigned key = pr_key(u[i]);
      if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  const unsigned c = s_hist[threadIdx.x];
  if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);          // integer sums: the order of arrival does not change them
}

// per block: how many of its candidates lie above the k-th value, and how many equal it
__global__ __launch_bounds__(TK_THREADS) void pr_topk_count_kernel(const float* __restrict__ unc, long long n, unsigned k, unsigned* __restrict__ ws,
                                                                   size_t ws_words_per_image) {
  __shared__ unsigned s_cnt[2];
  unsigned* hist = ws + (size_t)blockIdx.y * ws_words_per_image;
  unsigned* counts = hist + TK_PASSES * 256;
  const float* u = unc + (long long)blockIdx.y * n;
  unsigned kth, krem;
  pr_resolve(hist, TK_PASSES, k, kth, krem);
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  unsigned gt = 0u, eq = 0u;
  const long long i0 = (long long)blockIdx.x * TK_CHUNK;
#pragma unroll
  for (int j = 0; j < TK_ITEMS; ++j) {
    const long long i = i0 + j * TK_THREADS + threadIdx.x;
    if (i < n) {
      const unsigned key = pr_key(u[i]);
      gt += key > kth ? 1u : 0u;
      eq += key == kth ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    gt += (unsigned)__shfl_xor((int)gt, o, 64);
    eq += (unsigned)__shfl_xor((int)eq, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_cnt[0], gt);
    atomicAdd(&s_cnt[1], eq);
  }
  __syncthreads();
  if (threadIdx.x < 2) counts[2 * blockIdx.x + threadIdx.x] = s_cnt[threadIdx.x];
}

// the selected pixels in ascending order: a candidate above the k-th value is taken, one equal to it if fewer than `krem` equals precede it
__global__ __launch_bounds__(TK_THREADS) void pr_topk_emit_kernel(const float* __restrict__ unc, long long n, unsigned k, const unsigned* __restrict__ ws,
                                                                  size_t ws_words_per_image, int* __restrict__ idx) {
  __shared__ unsigned s_red[2][TK_THREADS / 64];
  __shared__ unsigned s_wave[2][TK_THREADS / 64];
  const unsigned* hist = ws + (size_t)blockIdx.y * ws_words_per_image;
  const unsigned* counts = hist + TK_PASSES * 256;
  const float* u = unc + (long long)blockIdx.y * n;
  int* out = idx + (long long)blockIdx.y * k;
  unsigned kth, krem;
  pr_resolve(hist, TK_PASSES, k, kth, krem);
  // candidates of the blocks in front of this one
  unsigned gt0 = 0u, eq0 = 0u;
  for (int bq = threadIdx.x; bq < (int)blockIdx.x; bq += TK_THREADS) {
    gt0 += counts[2 * bq];
    eq0 += counts[2 * bq + 1];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    gt0 += (unsigned)__shfl_xor((int)gt0, o, 64);
    eq0 += (unsigned)__shfl_xor((int)eq0, o, 64);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    s_red[0][wave] = gt0;
    s_red[1][wave] = eq0;
  }
  __syncthreads();
  gt0 = eq0 = 0u;
#pragma unroll
  for (int q = 0; q < TK_THREADS / 64; ++q) {
    gt0 += s_red[0][q];
    eq0 += s_red[1][q];
  }
  const long long i0 = (long long)blockIdx.x * TK_CHUNK;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;      // the lanes in front of this one
  for (int j = 0; j < TK_ITEMS; ++j) {                                        // (in index order: tile j holds indices i0 + 256 j ...)
    const long long i = i0 + j * TK_THREADS + threadIdx.x;
    bool gt = false, eq = false;
    if (i < n) {
      const unsigned key = pr_key(u[i]);
      gt = key > kth;
      eq = key == kth;
    }
    const unsigned long long mg = __ballot(gt), me = __ballot(eq);
    __syncthreads();                                  // (s_wave of the previous tile has been read)
    if (lane == 0) {
      s_wave[0][wave] = (unsigned)__popcll(mg);
      s_wave[1][wave] = (unsigned)__popcll(me);
    }
    __syncthreads();
    unsigned g_before = gt0 + (unsigned)__popcll(mg & below), e_before = eq0 + (unsigned)__popcll(me & below);
    unsigned g_tile = 0u, e_tile = 0u;
#pragma unroll
    for (int q = 0; q < TK_THREADS / 64; ++q) {
      if (q < wave) {
        g_before += s_wave[0][q];
        e_before += s_wave[1][q];
      }
      g_tile += s_wave[0][q];
      e_tile += s_wave[1][q];
    }
    if (gt || (eq && e_before < krem)) {
      const unsigned pos = g_before + (e_before < krem ? e_before : krem);
      if (pos < k) out[pos] = (int)i;                 // (always true: above + taken equals = k; the bound keeps a NaN-ridden input inside the list)
    }
    gt0 += g_tile;
    eq0 += e_tile;
  }
}

// ---------------------------------------------------------------------------------------------------------------- point gather
// (PrGather, the taps and the sweep of a point's channels: pointrend_taps.h, shared with the train-mode kernels)
__global__ __launch_bounds__(256) void pr_gather_kernel(PrGather g, const int* __restrict__ idx, int k, long long npts, int h, int w, float hstep,
                                                        float hhalf, float wstep, float whalf, float* __restrict__ out, int ldo) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);       // one wave per point
  if (p >= npts) return;
  const int b = (int)(p / k);
  const int pix = idx[p];
  const int row = pix / w, col = pix - row * w;
  // utils/pointrend_utils.py:146-147: step / 2 + index * step, every operation rounded to fp32; then point_sample's 2 p - 1
  const float px = __fadd_rn(whalf, __fmul_rn((float)col, wstep)), py = __fadd_rn(hhalf, __fmul_rn((float)row, hstep));
  pr_gather_point(g, b, p, pr_grid(px), pr_grid(py), out, ldo, lane);
}

// the train-mode form: the point's (x, y) in [0, 1]^2 is read, not derived from a cell index
__global__ __launch_bounds__(256) void pr_gather_at_kernel(PrGather g, const float* __restrict__ coords, int k, long long npts, float* __restrict__ out,
                                                           int ldo) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);       // one wave per point
  if (p >= npts) return;
  pr_gather_point(g, (int)(p / k), p, pr_grid(coords[2 * p]), pr_grid(coords[2 * p + 1]), out, ldo, lane);
}

// ---------------------------------------------------------------------------------------------------------------- scatter
__global__ __launch_bounds__(256) void pr_scatter_kernel(const float* __restrict__ rows, int ldr, const int* __restrict__ idx, int k, long long npts,
                                                         long long hw, float* __restrict__ seg, int lds, int K) {
  const long long total = npts * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long p = i / K;
    const int c = (int)(i - p * K);
    const long long b = p / k;
    const long long pix = idx[p];
    if (pix >= 0 && pix < hw) seg[(b * hw + pix) * lds + c] = rows[p * ldr + c];       // (an index outside the map writes nothing)
  }
}

size_t topk_words_per_image(long long n) {
  const long long blocks = (n + TK_CHUNK - 1) / TK_CHUNK;
  return (size_t)(TK_PASSES * 256 + 2 * blocks + 63) / 64 * 64;
}

}  // namespace

extern "C" int catseg_pointrend_uncertainty(const float* y, int ldy, float* uncertainty, long long pixels, int K, catseg_stream_t stream) {
  CS_REQUIRE(y && uncertainty && pixels > 0, "pointrend uncertainty: bad args");
  CS_REQUIRE(K >= 2, "pointrend uncertainty: the difference of the two largest logits needs K >= 2 classes (got %d)", K);
  CS_REQUIRE(ldy >= K, "pointrend uncertainty: ldy (%d) < K (%d)", ldy, K);
  CS_REQUIRE(pixels < (1ll << 31) * 256 && (long long)ldy * 256 < (1ll << 31), "pointrend uncertainty: too many pixels or rows too wide");
  const unsigned blocks = (unsigned)((pixels + 255) / 256);
  const int LS = K | 1;
  const size_t lds = (size_t)256 * LS * 4;
  if (lds <= CS_LDS_QUICK)
    hipLaunchKernelGGL(pr_uncertainty_kernel<true>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, y, ldy, uncertainty, pixels, K, LS);
  else
    hipLaunchKernelGGL(pr_uncertainty_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, y, ldy, uncertainty, pixels, K, LS);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" size_t catseg_pointrend_topk_workspace(int N, long long n) {
  if (N <= 0 || n <= 0) return 0;
  return (size_t)N * topk_words_per_image(n) * 4;
}

extern "C" int catseg_pointrend_topk(const float* uncertainty, int N, long long n, int k, int* idx, void* workspace, size_t workspace_bytes,
                                     catseg_stream_t stream) {
  CS_REQUIRE(uncertainty && idx && N > 0 && N <= 65535 && n > 0 && n < (1ll << 31), "pointrend topk: bad args");
  CS_REQUIRE(k >= 1 && k <= n, "pointrend topk: 1 <= k <= candidates per image (got k = %d, %lld candidates); the caller clamps k", k, n);
  const size_t need = catseg_pointrend_topk_workspace(N, n);
  if (!workspace || workspace_bytes < need || !cs_aligned16(workspace)) {
    catseg_set_error("pointrend topk: workspace too small or misaligned (%zu bytes needed, catseg_pointrend_topk_workspace)", need);
    return CATSEG_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t words = topk_words_per_image(n);
  // the histograms and block counts start from zero: cleared by a kernel of this file, in stream order in front of the first pass
  const size_t nwords = need / 4;
  hipLaunchKernelGGL(pr_zero_kernel, dim3(cs_grid_256((long long)nwords, 1024)), dim3(256), 0, st, (unsigned*)workspace, nwords);
  const dim3 grid((unsigned)((n + TK_CHUNK - 1) / TK_CHUNK), (unsigned)N);
  unsigned* ws = (unsigned*)workspace;
  for (int pass = 0; pass < TK_PASSES; ++pass)
    hipLaunchKernelGGL(pr_topk_hist_kernel, grid, dim3(TK_THREADS), 0, st, uncertainty, n, (unsigned)k, pass, ws, words);
  hipLaunchKernelGGL(pr_topk_count_kernel, grid, dim3(TK_THREADS), 0, st, uncertainty, n, (unsigned)k, ws, words);
  hipLaunchKernelGGL(pr_topk_emit_kernel, grid, dim3(TK_THREADS), 0, st, uncertainty, n, (unsigned)k, (const unsigned*)ws, words, idx);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

namespace {
// validates everything but the points of a gather descriptor and fills the kernel's argument
int gather_args(const catseg_pointrend_gather_desc* d, PrGather& g) {
  CS_REQUIRE(d->n_sources >= 1 && d->n_sources <= PR_MAXSRC, "pointrend gather: 1 to %d sources (got %d)", PR_MAXSRC, d->n_sources);
  CS_REQUIRE(d->n_extra >= 0 && d->n_extra <= PR_MAXDST, "pointrend gather: at most %d further destinations of the last block (got %d)", PR_MAXDST, d->n_extra);
  CS_REQUIRE(d->out && cs_aligned16(d->out) && d->ld_out % 4 == 0, "pointrend gather: a 16-byte aligned point matrix with ld %% 4 == 0 is required");
  int col = 0;
  for (int s = 0; s < d->n_sources; ++s) {
    const int Cq = (d->C[s] + 3) & ~3;
    CS_REQUIRE(d->src[s] != nullptr, "pointrend gather: source %d is NULL", s);
    CS_REQUIRE(d->H[s] > 0 && d->W[s] > 0 && d->C[s] > 0 && d->ld[s] >= d->C[s], "pointrend gather: source %d needs H, W, C > 0 and ld >= C (C %d, ld %d)", s, d->C[s], d->ld[s]);
    g.vec[s] = (cs_aligned16(d->src[s]) && d->ld[s] % 4 == 0 && d->ld[s] >= Cq) ? 1 : 0;
    CS_REQUIRE((long long)d->N * d->H[s] * d->W[s] * d->ld[s] < (1ll << 40), "pointrend gather: source %d too large", s);
    g.src[s] = d->src[s]; g.ld[s] = d->ld[s]; g.H[s] = d->H[s]; g.W[s] = d->W[s]; g.C[s] = d->C[s]; g.off[s] = col;
    col += Cq;
  }
  CS_REQUIRE(d->ld_out >= col, "pointrend gather: the point matrix has ld %d, the blocks need %d columns", d->ld_out, col);
  const int Cl = (d->C[d->n_sources - 1] + 3) & ~3;
  for (int q = 0; q < d->n_extra; ++q) {
    CS_REQUIRE(d->extra[q] && cs_aligned16(d->extra[q]) && d->extra_ld[q] % 4 == 0 && d->extra_off[q] % 4 == 0 && d->extra_off[q] >= 0 &&
                   d->extra_off[q] + Cl <= d->extra_ld[q],
               "pointrend gather: further destination %d: 16-byte aligned, ld and offset multiples of 4, offset + block <= ld", q);
    g.extra[q] = d->extra[q]; g.extra_ld[q] = d->extra_ld[q]; g.extra_off[q] = d->extra_off[q];
  }
  g.nsrc = d->n_sources;
  g.nextra = d->n_extra;
  return CATSEG_OK;
}
}  // namespace

extern "C" int catseg_pointrend_gather(const catseg_pointrend_gather_desc* d, catseg_stream_t stream) {
  CS_REQUIRE(d, "pointrend gather: null descriptor");
  CS_REQUIRE(d->n_sources >= 1 && d->n_sources <= PR_MAXSRC, "pointrend gather: 1 to %d sources (got %d)", PR_MAXSRC, d->n_sources);
  CS_REQUIRE(d->N > 0 && d->k > 0 && d->h > 0 && d->w > 0 && (long long)d->h * d->w < (1ll << 31) && d->k <= (long long)d->h * d->w,
             "pointrend gather: bad point grid (N %d, k %d, grid %d x %d)", d->N, d->k, d->h, d->w);
  CS_REQUIRE(d->idx, "pointrend gather: idx is required");
  PrGather g = {};
  if (const int rc = gather_args(d, g)) return rc;
  const long long npts = (long long)d->N * d->k;
  // 1 / float(h) is a Python float (double) in the reference; multiplied into / added to an fp32 tensor it is rounded to fp32 first
  const double hs = 1.0 / (double)d->h, wsd = 1.0 / (double)d->w;
  hipLaunchKernelGGL(pr_gather_kernel, dim3((unsigned)((npts + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, d->idx, d->k, npts, d->h, d->w, (float)hs,
                     (float)(hs / 2.0), (float)wsd, (float)(wsd / 2.0), d->out, d->ld_out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_gather_at(const catseg_pointrend_gather_desc* d, const float* coords, catseg_stream_t stream) {
  CS_REQUIRE(d && coords, "pointrend gather at coordinates: the descriptor and the coordinates [N, k, 2] are required");
  CS_REQUIRE(d->N > 0 && d->k > 0 && (long long)d->N * d->k < (1ll << 31), "pointrend gather at coordinates: N, k > 0 (N %d, k %d)", d->N, d->k);
  PrGather g = {};
  if (const int rc = gather_args(d, g)) return rc;
  const long long npts = (long long)d->N * d->k;
  hipLaunchKernelGGL(pr_gather_at_kernel, dim3((unsigned)((npts + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, coords, d->k, npts, d->out, d->ld_out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_pointrend_scatter(const float* rows, int ld_rows, const int* idx, int N, int k, long long hw, float* seg, int ld_seg, int K,
                                        catseg_stream_t stream) {
  CS_REQUIRE(rows && idx && seg && N > 0 && k > 0 && hw > 0 && hw < (1ll << 31) && k <= hw && K > 0 && ld_rows >= K && ld_seg >= K,
             "pointrend scatter: bad args");
  const long long total = (long long)N * k * K;
  hipLaunchKernelGGL(pr_scatter_kernel, dim3(cs_grid_256(total, 16384)), dim3(256), 0, (hipStream_t)stream, rows, ld_rows, idx, k, (long long)N * k, hw, seg,
                     ld_seg, K);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
