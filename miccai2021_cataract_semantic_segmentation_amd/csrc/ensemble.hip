// Bagging ensemble at inference (reference: models/Ensemble.py:57-74 -- per member nn.Softmax2d, torch.stack, torch.mean over the members;
// managers/BaseManager.py:671-674 takes the argmax of the result) as ONE streaming launch: M reads of the members' NHWC logits, one write of
// the merged probabilities and / or the label map.  The torch formulation is ~13 passes over a P x K tensor for three members.
//   catseg_ensemble_merge:      per pixel and member p_m = softmax(logits_m[pixel, 0:K]); mean or element-wise max over the members; argmax
//   catseg_nchw3_to_nhwc4_norm: torchvision Normalize of the NCHW frame written straight into the stem's NHWC-4 layout (UPerNet members)
// Rows of K (or ld) floats go through LDS (rows.h: 16-byte global accesses, odd LDS row stride = no bank conflict when lane t walks row t);
// a lane owns one pixel and keeps its K merged values in registers.
#include "rows.h"

namespace {

constexpr int PIX = 256;          // pixels per block
constexpr int MAXK = 64;
constexpr int MAXM = 8;
constexpr int MAXLD = MAXK + 4;   // widest row (floats) that is staged through LDS; wider member rows are read straight from global memory

struct MergeSrc {                 // passed BY VALUE in the kernel arguments: no device-side pointer table, nothing to upload, capturable
  const float* p[MAXM];
  int ld[MAXM];
};

// one member's row -> softmax -> folded into the lane's merged values
template <int KMAX>
__device__ __forceinline__ void merge_row(const float* row, int K, int mode, float (&acc)[KMAX]) {
  float v[KMAX];
  float mx = row[0];
#pragma unroll
  for (int c = 0; c < KMAX; ++c)
    if (c < K) {
      v[c] = row[c];
      mx = fmaxf(mx, v[c]);
    }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < KMAX; ++c)
    if (c < K) {
      v[c] = expf(v[c] - mx);                        // nn.Softmax2d: the row maximum subtracted
      s += v[c];
    }
#pragma unroll
  for (int c = 0; c < KMAX; ++c)
    if (c < K) {
      const float p = __fdiv_rn(v[c], s);
      acc[c] = mode ? fmaxf(acc[c], p) : __fadd_rn(acc[c], p);      // mean: summed in member order, as torch.mean(torch.stack(...), 0)
    }
}

// KMAX = K rounded up to the template's bucket: the per-pixel arrays are indexed by unrolled constants only (registers, no scratch)
template <int KMAX>
__global__ __launch_bounds__(PIX) void ensemble_merge_kernel(MergeSrc src, int M, long long P, int K, int LS, int mode,
                                                             float* __restrict__ probs, int ldp, int64_t* __restrict__ labels) {
  extern __shared__ float sh[];
  const long long p0 = (long long)blockIdx.x * PIX;
  const int np = (int)min((long long)PIX, P - p0);
  const int t = threadIdx.x;
  float acc[KMAX];
#pragma unroll
  for (int c = 0; c < KMAX; ++c) acc[c] = 0.f;      // 0 + p = p exactly; max(0, p) = p: the first member needs no special case
  bool dirty = false;                                // the LDS image is still being read by some lane
  for (int m = 0; m < M; ++m) {
    const float* __restrict__ g = src.p[m];
    const int ld = src.ld[m];
    const bool staged = ld <= MAXLD;                 // (uniform over the block)
    if (staged) {
      if (dirty) __syncthreads();
      stage_rows(g, p0, np, ld, LS, sh);             // whole rows, pad columns included: one contiguous 16-byte-aligned span per block
      __syncthreads();
      dirty = true;
    }
    if (t < np) {
      if (staged) merge_row<KMAX>(sh + t * LS, K, mode, acc);      // (two call sites: the LDS one compiles to ds_read, not to flat loads)
      else merge_row<KMAX>(g + (p0 + t) * (long long)ld, K, mode, acc);
    }
  }
  if (t < np) {
    if (mode == 0) {
      const float fm = (float)M;
#pragma unroll
      for (int c = 0; c < KMAX; ++c)
        if (c < K) acc[c] = __fdiv_rn(acc[c], fm);
    }
    if (labels) {                                    // the FIRST maximal class (torch.argmax), from the very values that are stored
      int best = 0;
      float bv = acc[0];
#pragma unroll
      for (int c = 1; c < KMAX; ++c)
        if (c < K && acc[c] > bv) {
          bv = acc[c];
          best = c;
        }
      labels[p0 + t] = (int64_t)best;
    }
  }
  if (probs) {
    if (dirty) __syncthreads();
    if (t < np) {
      float* row = sh + t * LS;
#pragma unroll
      for (int c = 0; c < KMAX; ++c)
        if (c < K) row[c] = acc[c];
      for (int c = K; c < ldp; ++c) row[c] = 0.f;    // pad columns are written zero
    }
    __syncthreads();
    unstage_rows(probs, p0, np, ldp, LS, sh, false);
  }
}

struct Norm3 {
  float mean[3], stdv[3];
};

__global__ __launch_bounds__(256) void nchw3_to_nhwc4_norm_kernel(const float* __restrict__ x, float* __restrict__ y, int B, long long HW,
                                                                  Norm3 n) {
  const long long total = (long long)B * HW;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / HW, p = i - b * HW;
    const float* s = x + b * 3 * HW + p;
    // Normalize: tensor.sub_(mean).div_(std) -- two roundings, a true division, no contraction
    f32x4 v = {__fdiv_rn(__fsub_rn(s[0], n.mean[0]), n.stdv[0]), __fdiv_rn(__fsub_rn(s[HW], n.mean[1]), n.stdv[1]),
               __fdiv_rn(__fsub_rn(s[2 * HW], n.mean[2]), n.stdv[2]), 0.f};
    *(f32x4*)(y + i * 4) = v;
  }
}

template <int KMAX>
int merge_launch(const MergeSrc& src, int M, long long P, int K, int LS, int mode, float* probs, int ldp, int64_t* labels, hipStream_t st) {
  const size_t shb = (size_t)PIX * LS * 4;
  CS_LDS_RESERVE(ensemble_merge_kernel<KMAX>, shb, "ensemble merge");
  hipLaunchKernelGGL(ensemble_merge_kernel<KMAX>, dim3((unsigned)((P + PIX - 1) / PIX)), dim3(PIX), shb, st, src, M, P, K, LS, mode, probs, ldp,
                     labels);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

}  // namespace

extern "C" int catseg_ensemble_merge(const float* const* logits, const int* ld, int M, long long P, int K, int mode, float* probs,
                                     int ld_probs, int64_t* labels, catseg_stream_t stream) {
  CS_REQUIRE(M >= 1 && M <= MAXM, "ensemble merge: 1 <= M <= %d members (got %d)", MAXM, M);
  CS_REQUIRE(K >= 1 && K <= MAXK, "ensemble merge: 1 <= K <= %d classes (got %d)", MAXK, K);
  CS_REQUIRE(P > 0 && P < (1ll << 31) * PIX, "ensemble merge: bad pixel count");
  CS_REQUIRE(mode == 0 || mode == 1, "ensemble merge: mode 0 (mean) or 1 (max)");
  CS_REQUIRE(logits && ld, "ensemble merge: null member table");
  CS_REQUIRE(probs || labels, "ensemble merge: both outputs are NULL");
  CS_REQUIRE(!probs || (ld_probs >= K && ld_probs <= MAXLD), "ensemble merge: K <= ld_probs <= %d (got %d)", MAXLD, ld_probs);
  MergeSrc src;
  int widest = probs ? ld_probs : 1;
  for (int m = 0; m < MAXM; ++m) {
    src.p[m] = nullptr;
    src.ld[m] = 0;
  }
  for (int m = 0; m < M; ++m) {
    CS_REQUIRE(logits[m] != nullptr, "ensemble merge: member %d is NULL", m);
    CS_REQUIRE(ld[m] >= K, "ensemble merge: member %d has ld %d < K = %d", m, ld[m], K);
    src.p[m] = logits[m];
    src.ld[m] = ld[m];
    if (ld[m] <= MAXLD && ld[m] > widest) widest = ld[m];
  }
  const int LS = widest | 1;
  hipStream_t st = (hipStream_t)stream;
  if (K <= 8) return merge_launch<8>(src, M, P, K, LS, mode, probs, ld_probs, labels, st);
  if (K <= 16) return merge_launch<16>(src, M, P, K, LS, mode, probs, ld_probs, labels, st);
  if (K <= 32) return merge_launch<32>(src, M, P, K, LS, mode, probs, ld_probs, labels, st);
  return merge_launch<64>(src, M, P, K, LS, mode, probs, ld_probs, labels, st);
}

extern "C" int catseg_nchw3_to_nhwc4_norm(const float* x, float* y, int B, int H, int W, const float* mean, const float* stdv,
                                          catseg_stream_t stream) {
  CS_REQUIRE(B > 0 && H > 0 && W > 0 && x && y && mean && stdv, "nchw3_to_nhwc4_norm: bad args");
  CS_REQUIRE(cs_aligned16(y), "nchw3_to_nhwc4_norm: the NHWC-4 output must be 16-byte aligned");
  Norm3 n;
  for (int c = 0; c < 3; ++c) {
    CS_REQUIRE(stdv[c] != 0.f, "nchw3_to_nhwc4_norm: std[%d] is zero", c);
    n.mean[c] = mean[c];
    n.stdv[c] = stdv[c];
  }
  const long long HW = (long long)H * W, total = (long long)B * HW;
  long long blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(nchw3_to_nhwc4_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, B, HW, n);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
