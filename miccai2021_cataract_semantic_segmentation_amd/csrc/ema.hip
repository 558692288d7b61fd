// The running average of the weights (include/catseg_ema.h): EMA / SWA update of a shadow of the flat parameter buffer, the
// in-place exchange of the two, and the same two operations over a table of small buffers (BatchNorm running statistics).
//
// ema_update_kernel / ema_swap_kernel   streaming, the shape of adam_ex_kernel (csrc/optim.hip): a capped grid of 256-thread blocks
//   strides over the 16-byte vectors; an iteration issues both loads before the first use.  The weight arrives by value or from device
//   memory (one 4-byte load per thread, uniform).  The last n % 4 elements go one by one.
// ema_table_kernel   one block per table entry, 4-byte accesses (the live buffers promise no more than that alignment).
#include "common.h"
#include "catseg_ema.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kGridCap = 8192;                 // blocks of the two streaming kernels (the cap of the optimiser update kernels)

struct EmaEntry { float* live; long long shadow_off; int n; int pad; };
static_assert(sizeof(EmaEntry) == CATSEG_EMA_ENTRY_BYTES, "catseg_ema_entry is 24 bytes");

// torch.lerp's two-sided form.  Contraction is off in this file and the one fused multiply-add per side is spelled out (what torch's CPU
// kernel does: fmadd(w, d, avg) / fmadd(w - 1, d, p)), so that the bits do not depend on what the compiler chooses to fuse.
__device__ __forceinline__ float lerp1(float avg, float p, float w, float rest, bool small) {
  const float d = p - avg;
  return small ? __builtin_fmaf(w, d, avg) : __builtin_fmaf(-d, rest, p);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ avg, long long n4, long long n,
                                                         float w, const float* __restrict__ w_dev) {
  if (w_dev) w = w_dev[0];
  const bool small = w < 0.5f;
  const float rest = 1.f - w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    if (e + 3 < n) {
      const f32x4 pp = *(const f32x4*)(p + e);
      f32x4 aa = *(f32x4*)(avg + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) aa[k] = lerp1(aa[k], pp[k], w, rest, small);
      *(f32x4*)(avg + e) = aa;
    } else {
      for (long long j = e; j < n; ++j) avg[j] = lerp1(avg[j], p[j], w, rest, small);
    }
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ a, float* __restrict__ b, long long n4, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    if (e + 3 < n) {
      const f32x4 aa = *(f32x4*)(a + e);
      const f32x4 bb = *(f32x4*)(b + e);
      *(f32x4*)(a + e) = bb;
      *(f32x4*)(b + e) = aa;
    } else {
      for (long long j = e; j < n; ++j) {
        const float x = a[j], y = b[j];
        a[j] = y;
        b[j] = x;
      }
    }
  }
}

template <bool SWAP>
__global__ __launch_bounds__(256) void ema_table_kernel(const EmaEntry* __restrict__ entries, float* __restrict__ shadow, float w,
                                                        const float* __restrict__ w_dev) {
  const EmaEntry ent = entries[blockIdx.x];
  float* __restrict__ live = ent.live;
  float* __restrict__ sh = shadow + ent.shadow_off;
  if (!SWAP && w_dev) w = w_dev[0];
  const bool small = w < 0.5f;
  const float rest = 1.f - w;
  for (int i = threadIdx.x; i < ent.n; i += kThreads) {
    const float x = live[i], s = sh[i];
    if (SWAP) {
      live[i] = s;
      sh[i] = x;
    } else {
      sh[i] = lerp1(s, x, w, rest, small);
    }
  }
}

inline bool weight_ok(float w) { return w >= 0.f && w <= 1.f; }      // (false for NaN)

}  // namespace

#define UPD_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_ema_update: " msg)
#define SWAP_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_ema_swap: " msg)
#define TAB_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_ema_table: " msg)

extern "C" int catseg_ema_grid_cap(void) { return kGridCap; }

extern "C" int catseg_ema_update(const float* p, float* avg, long long n, float w_host, const float* w_dev, catseg_stream_t stream) {
  UPD_REQUIRE(n > 0, "n must be positive");
  UPD_REQUIRE(p && avg, "p and avg are required");
  UPD_REQUIRE(cs_aligned16(p) && cs_aligned16(avg), "buffers must be 16-byte aligned");
  UPD_REQUIRE((((uintptr_t)w_dev) & 3) == 0, "w_dev must be 4-byte aligned");
  UPD_REQUIRE(w_dev || weight_ok(w_host), "the weight must be in [0, 1]");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(ema_update_kernel, dim3(cs_grid_256(n4, kGridCap)), dim3(kThreads), 0, (hipStream_t)stream, p, avg, n4, n, w_host, w_dev);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_ema_swap(float* a, float* b, long long n, catseg_stream_t stream) {
  SWAP_REQUIRE(n > 0, "n must be positive");
  SWAP_REQUIRE(a && b, "a and b are required");
  SWAP_REQUIRE(cs_aligned16(a) && cs_aligned16(b), "buffers must be 16-byte aligned");
  const long long n4 = (n + 3) / 4;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(cs_grid_256(n4, kGridCap)), dim3(kThreads), 0, (hipStream_t)stream, a, b, n4, n);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_ema_table(const void* entries, int count, float* shadow, int mode, float w_host, const float* w_dev,
                                catseg_stream_t stream) {
  TAB_REQUIRE(count > 0, "count must be positive");
  TAB_REQUIRE(entries && (((uintptr_t)entries) & 7) == 0, "the table is required and must be 8-byte aligned");
  TAB_REQUIRE(shadow && (((uintptr_t)shadow) & 3) == 0, "the shadow is required and must be 4-byte aligned");
  TAB_REQUIRE(mode == CATSEG_EMA_LERP || mode == CATSEG_EMA_SWAP, "unknown mode");
  TAB_REQUIRE((((uintptr_t)w_dev) & 3) == 0, "w_dev must be 4-byte aligned");
  TAB_REQUIRE(mode == CATSEG_EMA_SWAP || w_dev || weight_ok(w_host), "the weight must be in [0, 1]");
  const EmaEntry* tab = (const EmaEntry*)entries;
  hipStream_t st = (hipStream_t)stream;
  if (mode == CATSEG_EMA_SWAP)
    hipLaunchKernelGGL(ema_table_kernel<true>, dim3((unsigned)count), dim3(kThreads), 0, st, tab, shadow, w_host, w_dev);
  else
    hipLaunchKernelGGL(ema_table_kernel<false>, dim3((unsigned)count), dim3(kThreads), 0, st, tab, shadow, w_host, w_dev);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
