// SoftIoU, GenDiceLoss (losses/SoftIoU.py, losses/GenDiceLoss.py of the reference) and FocalLoss (losses/FocalLoss.py) on gfx950:
// a softmax over K <= 64 classes per pixel, a few per-class sums and a closed-form gradient -- one streaming pass forward, one backward.
//
// Overlap losses (logits [P][K], labels int64 [P]; label classes: 0 <= y < K one-hot column y; y == ignore (>= 0) a zero one-hot row whose
// probabilities still enter the sums over all pixels; any other label is INVALID: the pixel is dropped and counted):
//   ov_stats     : grid-stride over 256-pixel tiles, per class c in registers: S_c = sum_p p_pc, I_c = sum_{y_p = c} p_pc, n_c = #{y_p = c};
//                  fp32 within a tile, fp64 across tiles; one fp64 slab row per block (no float atomics: bitwise reproducible)
//   ov_finalize  : one block sums the slab in a fixed order (fp64) and forms the loss and the coefficients of
//                  d loss / d p_pc = alpha_c [y_p = c] + beta_c   (written to a buffer owned by the call)
//   ov_bwd       : dz_pk = up * p_pk * (g_pk - sum_c p_pc g_pc), g_pc = alpha_c [y_p = c] + beta_c, up = autograd's upstream scalar (device)
// Focal loss: focal_fwd (per-pixel terms, block partials) + focal_finalize (fp64, mean over all P pixels), focal_bwd (one pass, upstream
// scalar from device memory).  Invalid labels (outside [0, K)) contribute zero loss and zero gradient and stay in the mean's denominator.
#include "common.h"
#include "rows.h"

namespace {

constexpr int PIX = 256;
constexpr int MAXK = 64;
constexpr int OV_BLOCKS = 1536;  // grid of the statistics pass: 6 blocks per CU (the LDS bound at K = 25), ~11 tiles per block at the bench shape

struct ClassVec {
  float v[MAXK];
};

// >= 0: class with a one-hot column; -1: the ignore label (zero one-hot row); -2: invalid (dropped, counted)
__device__ __forceinline__ int classify(int64_t lab, int K, long long ignore) {
  if (lab >= 0 && lab < K) return (int)lab;
  if (ignore >= 0 && lab == ignore) return -1;
  return -2;
}

// softmax of one LDS row in place: row[c] = p_c
__device__ __forceinline__ void softmax_row(float* row, int K) {
  float m = row[0];
  for (int c = 1; c < K; ++c) m = fmaxf(m, row[c]);
  float s = 0.f;
  for (int c = 0; c < K; ++c) { const float e = expf(row[c] - m); row[c] = e; s += e; }
  const float inv = 1.f / s;
  for (int c = 0; c < K; ++c) row[c] *= inv;
}

// ---- overlap statistics ------------------------------------------------------------------------------------------------------------------
// slab, column-major [SL][nblk] (SL = 3K + 1 doubles per block): rows [0, K) S_c, [K, 2K) I_c, [2K, 3K) n_c, [3K] invalid labels
__global__ __launch_bounds__(PIX) void ov_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long long P, int K,
                                                       long long ignore, double* __restrict__ slab) {
  extern __shared__ float sh[];
  __shared__ int lab_s[PIX];
  __shared__ int inval_s;
  const int KS = K | 1;
  const int t = threadIdx.x;
  const int R = PIX / K;                  // row groups of the column pass: thread (c, g) = (t % K, t / K), t < R * K
  const int c = t % K, g = t / K;
  const bool col = t < R * K;
  double accS = 0.0, accI = 0.0;
  int accN = 0, inval = 0;
  if (t == 0) inval_s = 0;
  const long long ntiles = (P + PIX - 1) / PIX;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long p0 = tile * PIX;
    const int np = (int)min((long long)PIX, P - p0);
    stage_rows(logits, p0, np, K, KS, sh);
    int cls = -2;
    if (t < np) {
      cls = classify(labels[p0 + t], K, ignore);
      inval += cls == -2;
      lab_s[t] = cls;
    }
    __syncthreads();
    if (t < np) {
      float* row = sh + t * KS;
      if (cls == -2) {
        for (int k = 0; k < K; ++k) row[k] = 0.f;
      } else {
        softmax_row(row, K);
      }
    }
    __syncthreads();
    if (col) {
      float s = 0.f, in = 0.f;
      int n = 0;
      for (int r = g; r < np; r += R) {
        const float v = sh[r * KS + c];
        const bool hit = lab_s[r] == c;
        s += v;
        in += hit ? v : 0.f;
        n += hit;
      }
      accS += s;
      accI += in;
      accN += n;
    }
    __syncthreads();
  }
  // block reduction over the row groups, fixed order (the LDS tile is free now)
  double* rS = reinterpret_cast<double*>(sh);
  double* rI = rS + PIX;
  int* rN = reinterpret_cast<int*>(rI + PIX);
  rS[t] = accS;
  rI[t] = accI;
  rN[t] = accN;
  if (inval) atomicAdd(&inval_s, inval);  // integer: order-independent
  __syncthreads();
  const size_t nblk = gridDim.x;
  double* out = slab + blockIdx.x;
  if (t < K) {
    double s = 0.0, in = 0.0;
    long long n = 0;
    for (int q = 0; q < R; ++q) { s += rS[q * K + t]; in += rI[q * K + t]; n += rN[q * K + t]; }
    out[t * nblk] = s;
    out[(K + t) * nblk] = in;
    out[(2 * K + t) * nblk] = (double)n;
  }
  if (t == 0) out[3 * K * nblk] = (double)inval_s;
}

// one block per slab row: the OV_BLOCKS / 256 loads of a thread unconditional (clamped index + select) and in flight together, then a
// fixed-order reduction (wave butterfly, then the four waves in order): deterministic
__global__ __launch_bounds__(256) void ov_colsum_kernel(const double* __restrict__ slab, int nblk, double* __restrict__ tot) {
  constexpr int PER = OV_BLOCKS / 256;
  const double* col = slab + (size_t)blockIdx.x * nblk;
  const int t = threadIdx.x;
  double v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) v[u] = col[min(u * 256 + t, nblk - 1)];
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < PER; ++u) s += u * 256 + t < nblk ? v[u] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ double w[4];
  if ((t & 63) == 0) w[t >> 6] = s;
  __syncthreads();
  if (t == 0) tot[blockIdx.x] = ((w[0] + w[1]) + w[2]) + w[3];
}

// kind 0 = SoftIoU, 1 = GenDice; weight_mode (GenDice) 0 = none, 1 = 'auto' (1 / n_c^2, 1 where n_c = 0), 2 = the list w
__global__ __launch_bounds__(256) void ov_finalize_kernel(const double* __restrict__ colsum, int K, int kind, int naive, int weight_mode,
                                                          ClassVec w, float* __restrict__ loss_out, float* __restrict__ coef,
                                                          long long* __restrict__ invalid_out) {
  __shared__ double tot[3 * MAXK + 1];
  const int t = threadIdx.x;
  if (t < 3 * K + 1) tot[t] = colsum[t];
  __syncthreads();
  if (t != 0) return;
  // pass 1: fractions and the kept set (the reference's frac[union / divisor != 0]; naive: every class, nan where 0 / 0)
  double sum = 0.0;
  int kept = 0;
  for (int c = 0; c < K; ++c) {
    const double S = tot[c], I = tot[K + c], n = tot[2 * K + c];
    double num, den;
    if (kind == 0) {
      num = I;
      den = S + n - I;
    } else {
      const double wc = weight_mode == 0 ? 1.0 : weight_mode == 1 ? (n == 0.0 ? 1.0 : 1.0 / (n * n)) : (double)w.v[c];
      num = wc * I;
      den = wc * (S + n);
    }
    if (naive || den != 0.0) { sum += num / den; ++kept; }
  }
  const double mean = sum / (double)kept;  // no class kept: 0 / 0 = nan, as torch.mean of an empty tensor
  loss_out[0] = (float)(kind == 0 ? -mean : 1.0 - 2.0 * mean);
  invalid_out[0] = (long long)tot[3 * K];
  // pass 2: d loss / d p_pc = alpha_c [y_p = c] + beta_c
  const double dmean = (kind == 0 ? -1.0 : -2.0) / (double)kept;  // d loss / d frac_c for a kept class
  for (int c = 0; c < K; ++c) {
    const double S = tot[c], I = tot[K + c], n = tot[2 * K + c];
    double a = 0.0, b = 0.0;
    if (kind == 0) {
      const double U = S + n - I;  // d I / d p = [y = c], d U / d p = 1 - [y = c]
      if (naive || U != 0.0) {
        const double dI = dmean / U, dU = -dmean * I / (U * U);
        a = dI - dU;
        b = dU;
      }
    } else {
      const double wc = weight_mode == 0 ? 1.0 : weight_mode == 1 ? (n == 0.0 ? 1.0 : 1.0 / (n * n)) : (double)w.v[c];
      const double den = wc * (S + n);  // d dividend / d p = w [y = c], d divisor / d p = w
      if (naive || den != 0.0) {
        a = dmean * wc / den;
        b = -dmean * (wc * I) * wc / (den * den);
      }
    }
    coef[c] = (float)a;
    coef[MAXK + c] = (float)b;
  }
}

__global__ __launch_bounds__(PIX) void ov_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long long P, int K,
                                                     long long ignore, const float* __restrict__ coef, const float* __restrict__ upstream,
                                                     float* __restrict__ dlogits) {
  extern __shared__ float sh[];
  __shared__ float al[MAXK], be[MAXK];
  const int KS = K | 1;
  const long long p0 = (long long)blockIdx.x * PIX;
  const int np = (int)min((long long)PIX, P - p0);
  const int t = threadIdx.x;
  if (t < K) { al[t] = coef[t]; be[t] = coef[MAXK + t]; }
  stage_rows(logits, p0, np, K, KS, sh);
  __syncthreads();
  if (t < np) {
    float* row = sh + t * KS;
    const int cls = classify(labels[p0 + t], K, ignore);
    if (cls == -2) {
      for (int k = 0; k < K; ++k) row[k] = 0.f;
    } else {
      const float up = upstream ? upstream[0] : 1.f;
      softmax_row(row, K);
      float dot = 0.f;
      for (int k = 0; k < K; ++k) dot += row[k] * be[k];
      if (cls >= 0) dot += row[cls] * al[cls];
      for (int k = 0; k < K; ++k) {
        const float gk = be[k] + (k == cls ? al[k] : 0.f);
        row[k] = up * (row[k] * (gk - dot));
      }
    }
  }
  __syncthreads();
  unstage_rows(dlogits, p0, np, K, KS, sh, false);
}

// ---- focal loss --------------------------------------------------------------------------------------------------------------------------
// per pixel: l = log p_y (unweighted), pt = exp(l), term = -a_y (1 - pt)^gamma l;
// d term / d l = -a_y (1 - pt)^gamma + a_y gamma (1 - pt)^(gamma - 1) pt l  (the second term is absent for gamma = 0, as torch's pow backward)
__device__ __forceinline__ float focal_term(const float* row, int K, int y, float gamma, float a) {
  float m = row[0];
  for (int c = 1; c < K; ++c) m = fmaxf(m, row[c]);
  float s = 0.f;
  for (int c = 0; c < K; ++c) s += expf(row[c] - m);
  const float l = (row[y] - m) - logf(s);
  return -(powf(1.f - expf(l), gamma) * (l * a));
}
__device__ __forceinline__ float focal_dterm(float l, float gamma, float a) {
  const float pt = expf(l);
  const float base = 1.f - pt;
  return -a * powf(base, gamma) + (gamma != 0.f ? a * gamma * powf(base, gamma - 1.f) * pt * l : 0.f);
}

__global__ __launch_bounds__(PIX) void focal_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long long P, int K,
                                                        float gamma, int has_alpha, ClassVec alpha, float* __restrict__ part) {
  extern __shared__ float sh[];
  const int KS = K | 1;
  const long long p0 = (long long)blockIdx.x * PIX;
  const int np = (int)min((long long)PIX, P - p0);
  stage_rows(logits, p0, np, K, KS, sh);
  __syncthreads();
  const int t = threadIdx.x;
  float l = 0.f, bad = 0.f;
  if (t < np) {
    const int64_t lab = labels[p0 + t];
    if (lab >= 0 && lab < K) {
      l = focal_term(sh + t * KS, K, (int)lab, gamma, has_alpha ? alpha.v[(int)lab] : 1.f);
    } else {
      bad = 1.f;
    }
  }
  l = wave_sum(l);
  bad = wave_sum(bad);
  __shared__ float r[8];
  if ((t & 63) == 0) { r[t >> 6] = l; r[4 + (t >> 6)] = bad; }
  __syncthreads();
  if (t == 0) {
    part[2 * blockIdx.x] = r[0] + r[1] + r[2] + r[3];
    part[2 * blockIdx.x + 1] = r[4] + r[5] + r[6] + r[7];
  }
}

__global__ __launch_bounds__(1024) void focal_finalize_kernel(const float* __restrict__ part, long long nb, long long P, float* __restrict__ loss_out,
                                                              long long* __restrict__ invalid_out) {
  __shared__ double s1[1024], s2[1024];
  const long long t = threadIdx.x;
  double a = 0, b = 0;
  for (long long base = 0; base < nb; base += 8 * 1024) {   // eight pairs in flight per thread (clamped index + select, no predicated loads)
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const float2*>(part)[min(base + u * 1024 + t, nb - 1)];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (base + u * 1024 + t < nb) { a += v[u].x; b += v[u].y; }
  }
  s1[t] = a; s2[t] = b;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o) { s1[threadIdx.x] += s1[threadIdx.x + o]; s2[threadIdx.x] += s2[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_out[0] = (float)(s1[0] / (double)P);
    invalid_out[0] = (long long)s2[0];
  }
}

__global__ __launch_bounds__(PIX) void focal_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, long long P, int K,
                                                        float gamma, int has_alpha, ClassVec alpha, float inv_p, const float* __restrict__ upstream,
                                                        float* __restrict__ dlogits) {
  extern __shared__ float sh[];
  const int KS = K | 1;
  const long long p0 = (long long)blockIdx.x * PIX;
  const int np = (int)min((long long)PIX, P - p0);
  stage_rows(logits, p0, np, K, KS, sh);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < np) {
    float* row = sh + t * KS;
    const int64_t lab = labels[p0 + t];
    if (lab >= 0 && lab < K) {
      const int y = (int)lab;
      float m = row[0];
      for (int c = 1; c < K; ++c) m = fmaxf(m, row[c]);
      const float zy = row[y] - m;
      float s = 0.f;
      for (int c = 0; c < K; ++c) { const float e = expf(row[c] - m); row[c] = e; s += e; }
      const float d = focal_dterm(zy - logf(s), gamma, has_alpha ? alpha.v[y] : 1.f);
      const float w = d * inv_p * (upstream ? upstream[0] : 1.f);
      const float inv = 1.f / s;
      for (int c = 0; c < K; ++c) row[c] = ((c == y ? 1.f : 0.f) - row[c] * inv) * w;
    } else {
      for (int c = 0; c < K; ++c) row[c] = 0.f;
    }
  }
  __syncthreads();
  unstage_rows(dlogits, p0, np, K, KS, sh, false);
}

size_t cs_max_sz(size_t a, size_t b) { return a > b ? a : b; }

int ov_blocks(long long P) {
  const long long ntiles = (P + PIX - 1) / PIX;
  return (int)(ntiles < OV_BLOCKS ? ntiles : OV_BLOCKS);
}

}  // namespace

extern "C" size_t catseg_overlap_workspace(long long P, int K) {
  if (P <= 0 || K <= 0 || K > MAXK) return 0;
  return cs_align_up((size_t)(ov_blocks(P) + 1) * (3 * K + 1) * 8, 256);  // the slab, then its row sums
}

extern "C" int catseg_overlap_fwd(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index, int kind, int naive,
                                  int weight_mode, const float* weights, float* loss_out, float* coef, long long* invalid_out,
                                  void* workspace, size_t workspace_bytes, catseg_stream_t stream) {
  CS_REQUIRE(P > 0 && P < (1ll << 31), "overlap: need 0 < P < 2^31");
  CS_REQUIRE(K > 0 && K <= MAXK, "overlap: need 0 < K <= %d", MAXK);
  CS_REQUIRE(kind == 0 || kind == 1, "overlap: kind must be 0 (SoftIoU) or 1 (GenDice)");
  CS_REQUIRE(weight_mode >= 0 && weight_mode <= 2 && (weight_mode != 2 || weights) && (kind == 1 || weight_mode == 0),
             "overlap: weight_mode must be 0, 1 or 2 (GenDice only; 2 needs the weights)");
  CS_REQUIRE(logits && labels && loss_out && coef && invalid_out, "overlap: null pointer");
  if (workspace_bytes < catseg_overlap_workspace(P, K) || !workspace) {
    catseg_set_error("overlap: workspace too small");
    return CATSEG_EWORKSPACE;
  }
  ClassVec w = {};
  if (weight_mode == 2)
    for (int c = 0; c < K; ++c) w.v[c] = weights[c];
  hipStream_t st = (hipStream_t)stream;
  const int nblk = ov_blocks(P);
  const size_t shb = cs_max_sz((size_t)PIX * (K | 1) * 4, (size_t)PIX * 20);  // (the tile, then the block reduction: 2 doubles + 1 int per thread)
  hipLaunchKernelGGL(ov_stats_kernel, dim3(nblk), dim3(PIX), shb, st, logits, labels, P, K, ignore_index, (double*)workspace);
  double* colsum = (double*)workspace + (size_t)nblk * (3 * K + 1);
  hipLaunchKernelGGL(ov_colsum_kernel, dim3(3 * K + 1), dim3(256), 0, st, (const double*)workspace, nblk, colsum);
  hipLaunchKernelGGL(ov_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)colsum, K, kind, naive, weight_mode, w, loss_out, coef,
                     invalid_out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_overlap_bwd(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index, const float* coef,
                                  const float* upstream, float* dlogits, catseg_stream_t stream) {
  CS_REQUIRE(P > 0 && P < (1ll << 31), "overlap bwd: need 0 < P < 2^31");
  CS_REQUIRE(K > 0 && K <= MAXK, "overlap bwd: need 0 < K <= %d", MAXK);
  CS_REQUIRE(logits && labels && coef && dlogits, "overlap bwd: null pointer");
  const long long nb = (P + PIX - 1) / PIX;
  const size_t shb = (size_t)PIX * (K | 1) * 4;
  hipLaunchKernelGGL(ov_bwd_kernel, dim3((unsigned)nb), dim3(PIX), shb, (hipStream_t)stream, logits, labels, P, K, ignore_index, coef, upstream,
                     dlogits);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" size_t catseg_focal_workspace(long long P) {
  if (P <= 0) return 0;
  return cs_align_up((size_t)((P + PIX - 1) / PIX) * 8, 256);
}

extern "C" int catseg_focal_fwd(const float* logits, const int64_t* labels, long long P, int K, float gamma, const float* alpha, float* loss_out,
                                long long* invalid_out, void* workspace, size_t workspace_bytes, catseg_stream_t stream) {
  CS_REQUIRE(P > 0 && P < (1ll << 31), "focal: need 0 < P < 2^31");
  CS_REQUIRE(K > 0 && K <= MAXK, "focal: need 0 < K <= %d", MAXK);
  CS_REQUIRE(logits && labels && loss_out && invalid_out, "focal: null pointer");
  if (workspace_bytes < catseg_focal_workspace(P) || !workspace) {
    catseg_set_error("focal: workspace too small");
    return CATSEG_EWORKSPACE;
  }
  ClassVec a = {};
  if (alpha)
    for (int c = 0; c < K; ++c) a.v[c] = alpha[c];
  hipStream_t st = (hipStream_t)stream;
  const long long nb = (P + PIX - 1) / PIX;
  const size_t shb = (size_t)PIX * (K | 1) * 4;
  hipLaunchKernelGGL(focal_fwd_kernel, dim3((unsigned)nb), dim3(PIX), shb, st, logits, labels, P, K, gamma, alpha ? 1 : 0, a, (float*)workspace);
  hipLaunchKernelGGL(focal_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)workspace, nb, P, loss_out, invalid_out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_focal_bwd(const float* logits, const int64_t* labels, long long P, int K, float gamma, const float* alpha,
                                const float* upstream, float* dlogits, catseg_stream_t stream) {
  CS_REQUIRE(P > 0 && P < (1ll << 31), "focal bwd: need 0 < P < 2^31");
  CS_REQUIRE(K > 0 && K <= MAXK, "focal bwd: need 0 < K <= %d", MAXK);
  CS_REQUIRE(logits && labels && dlogits, "focal bwd: null pointer");
  ClassVec a = {};
  if (alpha)
    for (int c = 0; c < K; ++c) a.v[c] = alpha[c];
  const long long nb = (P + PIX - 1) / PIX;
  const size_t shb = (size_t)PIX * (K | 1) * 4;
  hipLaunchKernelGGL(focal_bwd_kernel, dim3((unsigned)nb), dim3(PIX), shb, (hipStream_t)stream, logits, labels, P, K, gamma, alpha ? 1 : 0, a,
                     (float)(1.0 / (double)P), upstream, dlogits);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
