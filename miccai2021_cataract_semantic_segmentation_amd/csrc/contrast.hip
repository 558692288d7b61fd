// The dense contrastive loss over a fixed set of anchor slots (include/ext/catseg_contrast.h; losses.DenseContrastiveLoss).
//
// ct_count_kernel / ct_scan_kernel / ct_select_kernel   the anchors: per 256-pixel chunk the class counts of the low-resolution labels (an
//   integer histogram in LDS; the full-size int64 map is read at the sampled positions only), per class an exclusive scan over the chunks,
//   per slot a binary search over the scanned counts and a select inside the chunk by ballot and popcount.  One wave per slot.
// ct_gather_kernel     one wave per slot: the feature row of its pixel, normalised as F.normalize does (a division per element).
// ct_rows_kernel       one 256-thread block per row of S = Z Z^T: the row in registers, a max pass, then D_i, the positive sum and count;
//                      writes ell_i and overwrites the row with G_i (zeros where the next product's pad contract needs them).
// ct_finalize_kernel   the fp64 sum of ell, one wave, contiguous segments summed in lane order.
// ct_fill0_kernel / ct_scatter_kernel   the gradient of the feature map: zeros, then per filled slot the adjoint of the normalisation.
// Integer atomics (the LDS histogram) only: every floating-point sum is formed by one thread, wave or block in a fixed order.
#include "common.h"
#include "ext/catseg_contrast.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = CATSEG_CONTRAST_CHUNK;
constexpr int kFillCap = 4096;
static_assert(kChunk == kThreads && kChunk % 64 == 0, "a chunk is one block of the count kernel and whole waves of the select");

inline int r4(int n) { return (n + 3) & ~3; }

// ---------------------------------------------------------------------------------------------------------------- anchors
__device__ __forceinline__ int ct_low_label(const long long* __restrict__ labels, int H, int W, int h, int w, long long q, int K) {
  const int j = (int)(q % w);
  const long long r = q / w;
  const int i = (int)(r % h);
  const long long b = r / h;
  const int y = (int)(((long long)i * H) / h), x = (int)(((long long)j * W) / w);
  const long long l = labels[(b * H + y) * W + x];
  return (l >= 0 && l < K) ? (int)l : -1;
}

// workspace (ints): [0] the draw number this pick uses, [4, 4 + K) the classes' counts, [4 + r4(K), ...) cnt[c][chunk]
__global__ __launch_bounds__(kThreads) void ct_count_kernel(const long long* __restrict__ labels, int H, int W, int h, int w, long long N, int K,
                                                            int nchunks, unsigned* __restrict__ state, int* __restrict__ ws_draw,
                                                            int* __restrict__ cnt) {
  extern __shared__ int ct_hist[];
  for (int c = threadIdx.x; c < K; c += kThreads) ct_hist[c] = 0;
  __syncthreads();
  const long long q = (long long)blockIdx.x * kChunk + threadIdx.x;
  const int l = q < N ? ct_low_label(labels, H, W, h, w, q, K) : -1;
  if (l >= 0) atomicAdd(&ct_hist[l], 1);
  __syncthreads();
  for (int c = threadIdx.x; c < K; c += kThreads) cnt[(long long)c * nchunks + blockIdx.x] = ct_hist[c];
  if (state != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {     // the select reads the draw number from the workspace: no race
    const unsigned draw = state[3];
    ws_draw[0] = (int)draw;
    state[3] = draw + 1u;
  }
}

// one block per class: cnt[c][0 .. nchunks) -> its exclusive scan in place, tot[c] = the class's count
__global__ __launch_bounds__(kThreads) void ct_scan_kernel(int* __restrict__ cnt, int nchunks, int* __restrict__ tot) {
  __shared__ int part[kThreads];
  int* row = cnt + (long long)blockIdx.x * nchunks;
  const int len = (nchunks + kThreads - 1) / kThreads;
  const int lo = min((int)threadIdx.x * len, nchunks), hi = min(lo + len, nchunks);
  int s = 0;
  for (int k = lo; k < hi; ++k) s += row[k];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
    tot[blockIdx.x] = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int k = lo; k < hi; ++k) {
    const int v = row[k];
    row[k] = run;
    run += v;
  }
}

__global__ __launch_bounds__(kThreads) void ct_select_kernel(const long long* __restrict__ labels, int H, int W, int h, int w, long long N, int K,
                                                             int M, int nchunks, const unsigned* __restrict__ state,
                                                             const int* __restrict__ fixed_u, int eval, const int* __restrict__ ws_draw,
                                                             const int* __restrict__ tot, const int* __restrict__ cnt,
                                                             int* __restrict__ idx, int* __restrict__ label, int* __restrict__ n_pos) {
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    int s = 0;
    for (int c = lane; c < K; c += 64) {
      const int n = min(tot[c], M);
      if (n >= 2) s += n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) n_pos[0] = s;
  }
  const int A = K * M;
  const int a = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);      // one wave per slot: everything below is uniform in the wave
  if (a >= A) return;
  const int c = a / M, m = a - c * M;
  const int n = tot[c];
  long long rank;
  if (n <= M) {
    if (m >= n) {
      if (lane == 0) {
        idx[a] = -1;
        label[a] = -1;
      }
      return;
    }
    rank = m;
  } else {
    unsigned u24;
    if (fixed_u != nullptr) {
      u24 = (unsigned)fixed_u[a] & 0xFFFFFFu;
    } else if (eval) {
      u24 = 1u << 23;
    } else {
      const ph_u32x4 r = philox4x32_10(ph_u32x4{(unsigned)a >> 2, (unsigned)ws_draw[0], PHILOX_STREAM_ANCHORS, state[2]}, state[0], state[1]);
      u24 = r[a & 3] >> 8;
    }
    const long long b0 = ((long long)m * n) / M, b1 = ((long long)(m + 1) * n) / M;
    rank = b0 + (((long long)u24 * (b1 - b0)) >> 24);
  }
  const int* row = cnt + (long long)c * nchunks;
  int lo = 0, hi = nchunks - 1;
  while (lo < hi) {                     // the last chunk whose scanned count is <= rank: it holds the pixel of that rank
    const int mid = (lo + hi + 1) >> 1;
    if (row[mid] <= rank) lo = mid; else hi = mid - 1;
  }
  int r = (int)(rank - row[lo]);
  const long long base = (long long)lo * kChunk;
  bool found = false;
  for (int sub = 0; sub < kChunk / 64 && !found; ++sub) {
    const long long q = base + sub * 64 + lane;
    const bool mine = q < N && ct_low_label(labels, H, W, h, w, q, K) == c;
    const unsigned long long mask = __ballot(mine);
    const int cm = __popcll(mask);
    if (r < cm) {
      if (mine && __popcll(mask & ((1ull << lane) - 1ull)) == r) {
        idx[a] = (int)q;
        label[a] = c;
      }
      found = true;
    } else {
      r -= cm;
    }
  }
  if (!found && lane == 0) {            // (cannot happen with consistent counts; a slot is never left unwritten)
    idx[a] = -1;
    label[a] = -1;
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather + normalise
template <bool VEC>
__global__ __launch_bounds__(kThreads) void ct_gather_kernel(const float* __restrict__ feat, int ld, long long n_pix, int d, int dp,
                                                             const int* __restrict__ idx, int A, float eps, float* __restrict__ Z,
                                                             float* __restrict__ inv_norm) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (a >= A) return;
  float* zr = Z + (long long)a * dp;
  const long long q = idx[a];
  if (q < 0 || q >= n_pix) {
    for (int k = lane; k < dp; k += 64) zr[k] = 0.f;
    if (lane == 0) inv_norm[a] = 0.f;
    return;
  }
  const float* f = feat + q * ld;
  float ss = 0.f;
  if (VEC) {
    for (int k = lane * 4; k < d; k += 256) {
      const f32x4 v = *(const f32x4*)(f + k);
      ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
  } else {
    for (int k = lane; k < d; k += 64) ss += f[k] * f[k];
  }
  ss = wave_sum(ss);
  const float norm = sqrtf(ss);
  const bool clamped = norm < eps;
  const float den = clamped ? eps : norm;
  if (VEC) {                            // (d % 4 == 0: there are no pad columns)
    for (int k = lane * 4; k < d; k += 256) {
      f32x4 v = *(const f32x4*)(f + k);
      v[0] /= den; v[1] /= den; v[2] /= den; v[3] /= den;
      *(f32x4*)(zr + k) = v;
    }
  } else {
    for (int k = lane; k < dp; k += 64) zr[k] = k < d ? f[k] / den : 0.f;
  }
  if (lane == 0) inv_norm[a] = clamped ? -(1.f / den) : 1.f / den;
}

// ---------------------------------------------------------------------------------------------------------------- loss rows
__device__ __forceinline__ float ct_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float ct_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ void ct_zero_row(float* __restrict__ row, int A4) {
  for (int j = threadIdx.x; j < A4; j += kThreads) row[j] = 0.f;
}

template <int NPT>
__global__ __launch_bounds__(kThreads) void ct_rows_kernel(float* __restrict__ S, int lds, int A, const int* __restrict__ label,
                                                           const float* __restrict__ Wt, int K, float inv_tau, const int* __restrict__ n_pos,
                                                           float* __restrict__ ell) {
  extern __shared__ float ct_wrow[];
  __shared__ float red[4];
  const int i = blockIdx.x;
  const int A4 = (A + 3) & ~3;
  float* row = S + (long long)i * lds;
  const int yi = label[i];
  if (yi < 0 || yi >= K) {              // an empty slot (uniform in the block)
    ct_zero_row(row, A4);
    if (threadIdx.x == 0) ell[i] = 0.f;
    return;
  }
  for (int c = threadIdx.x; c < K; c += kThreads) ct_wrow[c] = Wt[(long long)yi * K + c];
  __syncthreads();
  float s[NPT], e[NPT];                 // e: first the pair's weight (0 = no pair), then w exp(s - max)
  bool pos[NPT];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = threadIdx.x + kThreads * k;
    const int yj = j < A ? label[j] : -1;
    const bool ok = yj >= 0 && yj < K && j != i;
    pos[k] = ok && yj == yi;
    e[k] = ok ? (pos[k] ? 1.f : ct_wrow[yj]) : 0.f;
    s[k] = ok ? row[j] * inv_tau : -INFINITY;
    mx = fmaxf(mx, s[k]);
  }
  mx = ct_block_max(mx, red);
  if (mx == -INFINITY) {                // no other filled slot
    ct_zero_row(row, A4);
    if (threadIdx.x == 0) ell[i] = 0.f;
    return;
  }
  float D = 0.f, ps = 0.f, pc = 0.f;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const bool ok = s[k] != -INFINITY;
    e[k] = ok ? e[k] * expf(s[k] - mx) : 0.f;
    D += e[k];
    ps += pos[k] ? s[k] : 0.f;
    pc += pos[k] ? 1.f : 0.f;
  }
  D = ct_block_sum(D, red);
  ps = ct_block_sum(ps, red);
  pc = ct_block_sum(pc, red);
  if (pc == 0.f) {                      // no positive: the row takes no part
    ct_zero_row(row, A4);
    if (threadIdx.x == 0) ell[i] = 0.f;
    return;
  }
  if (threadIdx.x == 0) ell[i] = (mx + logf(D)) - ps / pc;
  const int np = n_pos[0];
  const float invn = 1.f / (float)(np > 1 ? np : 1);
  const float ipc = 1.f / pc;
#pragma unroll
  for (int k = 0; k < NPT; ++k) {
    const int j = threadIdx.x + kThreads * k;
    if (j < A4) {
      const bool ok = s[k] != -INFINITY;
      row[j] = ok ? (e[k] / D - (pos[k] ? ipc : 0.f)) * invn : 0.f;
    }
  }
}

__global__ __launch_bounds__(64) void ct_finalize_kernel(const float* __restrict__ ell, int A, const int* __restrict__ n_pos,
                                                         float* __restrict__ loss) {
  __shared__ double part[64];
  const int len = (A + 63) / 64;
  const int lo = min((int)threadIdx.x * len, A), hi = min(lo + len, A);
  double s = 0.0;
  for (int k = lo; k < hi; ++k) s += (double)ell[k];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 64; ++k) t += part[k];
    const int np = n_pos[0];
    loss[0] = (float)(t / (double)(np > 1 ? np : 1));
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(kThreads) void ct_fill0_kernel(float* __restrict__ p, long long n4, long long n) {
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreads) {
    const long long e = i * 4;
    if (e + 3 < n) {
      *(f32x4*)(p + e) = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (long long j = e; j < n; ++j) p[j] = 0.f;
    }
  }
}

__global__ __launch_bounds__(kThreads) void ct_scatter_kernel(const float* __restrict__ dZ, const float* __restrict__ Z, int ldz,
                                                              const float* __restrict__ inv_norm, const int* __restrict__ idx, int A, int d,
                                                              const float* __restrict__ g, float inv_tau, float* __restrict__ dfeat,
                                                              long long n_pix) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (a >= A) return;
  const long long q = idx[a];
  if (q < 0 || q >= n_pix) return;
  const float inv = inv_norm[a];
  const float sc = g[0] * inv_tau;
  const float* dz = dZ + (long long)a * ldz;
  const float* z = Z + (long long)a * ldz;
  float* out = dfeat + q * d;
  if (inv < 0.f) {                      // the norm was clamped to eps: it carries no gradient
    for (int k = lane; k < d; k += 64) out[k] = (dz[k] * sc) * -inv;
    return;
  }
  float dot = 0.f;
  for (int k = lane; k < d; k += 64) dot += (dz[k] * sc) * z[k];
  dot = wave_sum(dot);
  for (int k = lane; k < d; k += 64) out[k] = (dz[k] * sc - dot * z[k]) * inv;
}

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
inline unsigned wave_blocks(int A) { return (unsigned)((A + kThreads / 64 - 1) / (kThreads / 64)); }

}  // namespace

#define PICK_REQUIRE(cond, ...) CS_REQUIRE(cond, "catseg_contrast_pick: " __VA_ARGS__)
#define GATHER_REQUIRE(cond, ...) CS_REQUIRE(cond, "catseg_contrast_gather: " __VA_ARGS__)
#define ROWS_REQUIRE(cond, ...) CS_REQUIRE(cond, "catseg_contrast_rows: " __VA_ARGS__)
#define FIN_REQUIRE(cond, ...) CS_REQUIRE(cond, "catseg_contrast_finalize: " __VA_ARGS__)
#define SCAT_REQUIRE(cond, ...) CS_REQUIRE(cond, "catseg_contrast_scatter_bwd: " __VA_ARGS__)

extern "C" size_t catseg_contrast_pick_workspace(int B, int h, int w, int K) {
  if (B <= 0 || h <= 0 || w <= 0 || K <= 0) return 0;
  const long long N = (long long)B * h * w;
  const long long nchunks = (N + kChunk - 1) / kChunk;
  return (size_t)(4 + r4(K) + (long long)K * nchunks) * sizeof(int);
}

extern "C" int catseg_contrast_pick(const long long* labels, int B, int H, int W, int h, int w, int K, int M, void* state, const int* fixed_u,
                                    int eval, int* idx, int* label, int* n_pos, void* workspace, size_t workspace_bytes,
                                    catseg_stream_t stream) {
  PICK_REQUIRE(B > 0 && H > 0 && W > 0 && h > 0 && w > 0 && K > 0 && M > 0, "every dimension must be positive");
  PICK_REQUIRE((long long)K * M <= CATSEG_CONTRAST_MAX_ANCHORS, "K M = %lld slots exceed %d", (long long)K * M, CATSEG_CONTRAST_MAX_ANCHORS);
  PICK_REQUIRE(h <= H && w <= W, "the feature map (%d x %d) must not exceed the label map (%d x %d)", h, w, H, W);
  const long long N = (long long)B * h * w;
  PICK_REQUIRE(N < (1ll << 31), "B h w must stay below 2^31");
  PICK_REQUIRE(labels && (((uintptr_t)labels) & 7) == 0, "labels are required, 8-byte aligned");
  PICK_REQUIRE(idx && label && n_pos && aligned4(idx) && aligned4(label) && aligned4(n_pos), "idx, label and n_pos are required, 4-byte aligned");
  PICK_REQUIRE(aligned4(fixed_u), "fixed_u must be 4-byte aligned");
  const bool draws = fixed_u == nullptr && !eval;
  PICK_REQUIRE(!draws || (state && (((uintptr_t)state) & 15) == 0), "a draw needs the 16 bytes of device state, 16-byte aligned");
  const size_t need = catseg_contrast_pick_workspace(B, h, w, K);
  PICK_REQUIRE(workspace && aligned4(workspace) && workspace_bytes >= need, "the workspace needs %zu bytes, 4-byte aligned (got %zu)", need,
               workspace_bytes);
  const int nchunks = (int)((N + kChunk - 1) / kChunk);
  int* ws = (int*)workspace;
  int* tot = ws + 4;
  int* cnt = ws + 4 + r4(K);
  hipStream_t st = (hipStream_t)stream;
  unsigned* moving = draws ? (unsigned*)state : nullptr;
  hipLaunchKernelGGL(ct_count_kernel, dim3((unsigned)nchunks), dim3(kThreads), (size_t)K * sizeof(int), st, labels, H, W, h, w, N, K, nchunks, moving,
                     ws, cnt);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(ct_scan_kernel, dim3((unsigned)K), dim3(kThreads), 0, st, cnt, nchunks, tot);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(ct_select_kernel, dim3(wave_blocks(K * M)), dim3(kThreads), 0, st, labels, H, W, h, w, N, K, M, nchunks, (const unsigned*)moving,
                     fixed_u, eval, (const int*)ws, (const int*)tot, (const int*)cnt, idx, label, n_pos);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_contrast_gather(const float* feat, int ld, long long n_pix, int d, const int* idx, int A, float eps, float* Z,
                                      float* inv_norm, catseg_stream_t stream) {
  GATHER_REQUIRE(n_pix > 0 && d > 0 && A > 0 && A <= CATSEG_CONTRAST_MAX_ANCHORS, "n_pix, d > 0 and 0 < A <= %d", CATSEG_CONTRAST_MAX_ANCHORS);
  GATHER_REQUIRE(ld >= d, "ld (%d) < d (%d)", ld, d);
  GATHER_REQUIRE(eps > 0.f, "eps must be positive");
  GATHER_REQUIRE(feat && idx && inv_norm && aligned4(feat) && aligned4(idx) && aligned4(inv_norm), "feat, idx and inv_norm are required, 4-byte aligned");
  GATHER_REQUIRE(Z && cs_aligned16(Z), "Z is required, 16-byte aligned");
  const int dp = r4(d);
  hipStream_t st = (hipStream_t)stream;
  if (d % 4 == 0 && ld % 4 == 0 && cs_aligned16(feat))
    hipLaunchKernelGGL(ct_gather_kernel<true>, dim3(wave_blocks(A)), dim3(kThreads), 0, st, feat, ld, n_pix, d, dp, idx, A, eps, Z, inv_norm);
  else
    hipLaunchKernelGGL(ct_gather_kernel<false>, dim3(wave_blocks(A)), dim3(kThreads), 0, st, feat, ld, n_pix, d, dp, idx, A, eps, Z, inv_norm);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_contrast_rows(float* S, int lds, int A, const int* label, const float* Wt, int K, float inv_tau, const int* n_pos,
                                    float* ell, catseg_stream_t stream) {
  ROWS_REQUIRE(A > 0 && A <= CATSEG_CONTRAST_MAX_ANCHORS && K > 0 && K <= CATSEG_CONTRAST_MAX_ANCHORS, "0 < A, K <= %d", CATSEG_CONTRAST_MAX_ANCHORS);
  ROWS_REQUIRE(lds >= r4(A), "lds (%d) < r4(A) (%d)", lds, r4(A));
  ROWS_REQUIRE(inv_tau > 0.f, "inv_tau must be positive");
  ROWS_REQUIRE(S && cs_aligned16(S), "S is required, 16-byte aligned");
  ROWS_REQUIRE(label && Wt && n_pos && ell && aligned4(label) && aligned4(Wt) && aligned4(n_pos) && aligned4(ell),
               "label, Wt, n_pos and ell are required, 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds_bytes = (size_t)K * sizeof(float);
  if (A <= 2 * kThreads)
    hipLaunchKernelGGL(ct_rows_kernel<2>, dim3((unsigned)A), dim3(kThreads), lds_bytes, st, S, lds, A, label, Wt, K, inv_tau, n_pos, ell);
  else if (A <= 8 * kThreads)
    hipLaunchKernelGGL(ct_rows_kernel<8>, dim3((unsigned)A), dim3(kThreads), lds_bytes, st, S, lds, A, label, Wt, K, inv_tau, n_pos, ell);
  else
    hipLaunchKernelGGL(ct_rows_kernel<32>, dim3((unsigned)A), dim3(kThreads), lds_bytes, st, S, lds, A, label, Wt, K, inv_tau, n_pos, ell);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_contrast_finalize(const float* ell, int A, const int* n_pos, float* loss, catseg_stream_t stream) {
  FIN_REQUIRE(A > 0 && A <= CATSEG_CONTRAST_MAX_ANCHORS, "0 < A <= %d", CATSEG_CONTRAST_MAX_ANCHORS);
  FIN_REQUIRE(ell && n_pos && loss && aligned4(ell) && aligned4(n_pos) && aligned4(loss), "ell, n_pos and loss are required, 4-byte aligned");
  hipLaunchKernelGGL(ct_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ell, A, n_pos, loss);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_contrast_scatter_bwd(const float* dZ, const float* Z, int ldz, const float* inv_norm, const int* idx, int A, int d,
                                           const float* g, float inv_tau, float* dfeat, long long n_pix, catseg_stream_t stream) {
  SCAT_REQUIRE(n_pix > 0 && d > 0 && A > 0 && A <= CATSEG_CONTRAST_MAX_ANCHORS, "n_pix, d > 0 and 0 < A <= %d", CATSEG_CONTRAST_MAX_ANCHORS);
  SCAT_REQUIRE(n_pix * d < (1ll << 40), "the gradient is too large");
  SCAT_REQUIRE(ldz >= r4(d), "ldz (%d) < r4(d) (%d)", ldz, r4(d));
  SCAT_REQUIRE(inv_tau > 0.f, "inv_tau must be positive");
  SCAT_REQUIRE(dZ && Z && cs_aligned16(dZ) && cs_aligned16(Z), "dZ and Z are required, 16-byte aligned");
  SCAT_REQUIRE(inv_norm && idx && g && aligned4(inv_norm) && aligned4(idx) && aligned4(g), "inv_norm, idx and g are required, 4-byte aligned");
  SCAT_REQUIRE(dfeat && cs_aligned16(dfeat), "dfeat is required, 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long n = n_pix * d, n4 = (n + 3) / 4;
  hipLaunchKernelGGL(ct_fill0_kernel, dim3(cs_grid_256(n4, kFillCap)), dim3(kThreads), 0, st, dfeat, n4, n);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(ct_scatter_kernel, dim3(wave_blocks(A)), dim3(kThreads), 0, st, dZ, Z, ldz, inv_norm, idx, A, d, g, inv_tau, dfeat, n_pix);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
