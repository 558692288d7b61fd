// Label census and per-batch IoU average (include/catseg_census.h): what the class-aware train loaders start from and feed on.
//
// label_census_kernel   grid (chunks of a frame, frames), 256 threads.  A frame is H * W bytes at any address: the bytes in front of its
//   first 16-byte boundary and behind its last one (at most 15 each) are counted bytewise by the frame's block 0, the 16-byte vectors
//   between are dealt to the blocks in runs of kVecPerBlock and read once, one vector per lane and iteration.  Label maps are large
//   uniform regions, so counting is run-length first:
//     wave run   all 64 lanes hold sixteen times the same byte: 1024 pixels go to a (value, run) pair in registers, which lane 0 hands
//                to the wave's LDS histogram when the value changes -- one LDS atomic per run of a wave, not per pixel;
//     lane runs  otherwise every lane walks its 16 bytes and hands over each run (one atomic per run; sixteen at worst).
//   Four per-wave histograms of nbins + 1 32-bit counters (a block sees fewer than 2^31 pixels); at the end the block adds each non-empty
//   bin once to counts[b][bin] with a 64-bit integer atomic.  The label table is applied when a run is handed over, through a 256-entry
//   LDS table that also folds every value >= nbins into the "other" bin.
// iou_ema_kernel        one block: thread c owns class c (integer row / column sums of cm_running - cm_prev, one fp32 conversion each,
//   fp32 arithmetic in the reference's order, contraction off), then the block copies cm_running over cm_prev.
#include "common.h"
#include "catseg_census.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256, kWaves = 4, kMaxBins = 257;
constexpr long long kVecPerBlock = 1024;      // 16 KB of labels per block: 32 blocks for a 540 x 960 frame

__global__ __launch_bounds__(256) void label_census_kernel(const uint8_t* __restrict__ lbl, const uint8_t* __restrict__ lut, long long n,
                                                           int nbins, u64* __restrict__ counts) {
  __shared__ unsigned hist[kWaves][kMaxBins];
  __shared__ unsigned short bin_of[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  for (int i = tid; i < kWaves * kMaxBins; i += kThreads) (&hist[0][0])[i] = 0u;
  {
    const unsigned v = lut ? (unsigned)lut[tid] : (unsigned)tid;
    bin_of[tid] = (unsigned short)(v < (unsigned)nbins ? v : (unsigned)nbins);
  }
  __syncthreads();
  const uint8_t* frame = lbl + (long long)b * n;
  long long head = (long long)((16u - (unsigned)((uintptr_t)frame & 15u)) & 15u);
  if (head > n) head = n;
  const long long nv = (n - head) >> 4, tail = n - head - (nv << 4);
  unsigned* h = hist[wave];
  if (blockIdx.x == 0) {
    if (tid < head) atomicAdd(&h[bin_of[frame[tid]]], 1u);
    if (tid < tail) atomicAdd(&h[bin_of[frame[head + (nv << 4) + tid]]], 1u);
  }
  const uint4* vec = (const uint4*)(frame + head);
  const long long v0 = (long long)blockIdx.x * kVecPerBlock;
  const long long v1 = v0 + kVecPerBlock < nv ? v0 + kVecPerBlock : nv;
  unsigned cur = 0u, run = 0u;                 // the wave's open run (the same in every lane)
  for (long long base = v0 + wave * 64; base < v1; base += kThreads) {      // (bounds uniform over the wave: all lanes reach __all)
    const long long i = base + lane;
    const bool valid = i < v1;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (valid) q = vec[i];
    const unsigned first = q.x & 255u;
    const bool flat = valid && q.x == first * 0x01010101u && q.y == q.x && q.z == q.x && q.w == q.x;
    const unsigned lead = (unsigned)__builtin_amdgcn_readfirstlane((int)first);
    if (__all(flat && first == lead)) {
      if (lead != cur) {
        if (run != 0u && lane == 0) atomicAdd(&h[bin_of[cur]], run);
        cur = lead;
        run = 0u;
      }
      run += 1024u;
    } else if (valid) {
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
      unsigned pv = first, pr = 0u;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const unsigned v = (w[k >> 2] >> ((k & 3) * 8)) & 255u;
        if (v == pv) {
          ++pr;
        } else {
          atomicAdd(&h[bin_of[pv]], pr);
          pv = v;
          pr = 1u;
        }
      }
      atomicAdd(&h[bin_of[pv]], pr);
    }
  }
  if (run != 0u && lane == 0) atomicAdd(&h[bin_of[cur]], run);
  __syncthreads();
  u64* row = counts + (long long)b * (nbins + 1);
  for (int bin = tid; bin <= nbins; bin += kThreads) {
    const u64 s = (u64)hist[0][bin] + hist[1][bin] + hist[2][bin] + hist[3][bin];
    if (s != 0ull) atomicAdd(&row[bin], s);
  }
}

__global__ __launch_bounds__(256) void iou_ema_kernel(const int32_t* __restrict__ cm, int32_t* __restrict__ prev, int K, float w_old,
                                                      float w_new, float* __restrict__ values, float* __restrict__ iou_batch) {
  const int c = threadIdx.x;
  if (c < K) {
    long long r = 0, s = 0;
    for (int i = 0; i < K; ++i) {
      r += (long long)cm[i * K + c] - prev[i * K + c];      // sum over dim 0: the reference's row_sum
      s += (long long)cm[c * K + i] - prev[c * K + i];      // sum over dim 1: its col_sum
    }
    const long long d = (long long)cm[c * K + c] - prev[c * K + c];
    const float df = (float)d, rf = (float)r, sf = (float)s;
    const float den = (rf + sf) - df;
    float iou = df / den;                      // correctly rounded (hipcc's default for fp32 division)
    if (iou != iou) iou = 0.0f;
    const float keep = w_old * values[c];
    const float gain = w_new * iou;
    values[c] = keep + gain;
    if (iou_batch) iou_batch[c] = iou;
  }
  __syncthreads();                             // every difference is taken before cm_prev moves
  for (int i = threadIdx.x; i < K * K; i += kThreads) prev[i] = cm[i];
}

}  // namespace

#define CENSUS_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_label_census_u8: " msg)
#define EMA_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_iou_ema: " msg)

extern "C" int catseg_label_census_u8(const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, int nbins, int64_t* counts, int accumulate,
                                      catseg_stream_t stream) {
  CENSUS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "bad dims (B in 1..65535, H, W > 0)");
  const long long n = (long long)H * (long long)W;
  CENSUS_REQUIRE(n < (1ll << 31), "a frame is limited to 2^31 - 1 pixels (the sub-counters are 32 bits wide)");
  CENSUS_REQUIRE(nbins >= 1 && nbins <= 256, "nbins must be in 1..256");
  CENSUS_REQUIRE(lbl != nullptr, "the label map is NULL");
  CENSUS_REQUIRE(counts != nullptr, "counts is NULL");
  CENSUS_REQUIRE((((uintptr_t)counts) & 7) == 0, "counts must be 8-byte aligned");
  if (!accumulate) {
    if (hipMemsetAsync(counts, 0, (size_t)B * (size_t)(nbins + 1) * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) {
      (void)hipGetLastError();
      catseg_set_error("catseg_label_census_u8: cannot clear counts");
      return CATSEG_EHIP;
    }
  }
  const long long chunks = ((n >> 4) + kVecPerBlock - 1) / kVecPerBlock;
  hipLaunchKernelGGL(label_census_kernel, dim3((unsigned)(chunks > 0 ? chunks : 1), (unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, lbl, lut,
                     n, nbins, (u64*)counts);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_iou_ema(const int32_t* cm_running, int32_t* cm_prev, int K, float w_old, float w_new, float* iou_values, float* iou_batch,
                              catseg_stream_t stream) {
  EMA_REQUIRE(K >= 1 && K <= 256, "K must be in 1..256");
  EMA_REQUIRE(cm_running != nullptr && cm_prev != nullptr && iou_values != nullptr, "cm_running, cm_prev and iou_values are required");
  EMA_REQUIRE(cm_running != cm_prev, "cm_prev must not be the running matrix");
  EMA_REQUIRE(((((uintptr_t)cm_running) | ((uintptr_t)cm_prev) | ((uintptr_t)iou_values) | ((uintptr_t)iou_batch)) & 3) == 0,
              "operands must be 4-byte aligned");
  hipLaunchKernelGGL(iou_ema_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, cm_running, cm_prev, K, w_old, w_new, iou_values, iou_batch);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
