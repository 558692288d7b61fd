// Fused optimiser updates on the flat parameter buffer (include/catseg_optim.h): Adam / AdamW with weight decay and amsgrad,
// momentum SGD, parameter groups through a per-chunk group map, and the global gradient norm behind clipping.
//
// adam_ex_kernel / sgd_kernel   streaming: a capped grid of 256-thread blocks strides over the 16-byte vectors; an iteration issues every
//   load it needs (g, p, the state buffers, the chunk's group byte) before the first use, and writes p and the state back.  The 20 step
//   scalars arrive either by value (kernel argument) or from a device row; both are copied to LDS once per block, where the group's
//   {lr, wd} pair is looked up per vector.  A vector of 4 floats lies inside one 64-float chunk, so one group byte serves it.
//   adam_ex_kernel keeps the expression order of adam_kernel (csrc/lovasz.hip) and spells out the fused multiply-adds the compiler
//   formed there: with no option it writes the same bits.
// grad_sq_kernel / grad_norm_final_kernel   block b sums the squares of vectors [b * slice, (b + 1) * slice) in fp64: a thread walks its
//   vectors in order into one accumulator, the 64 lanes of a wave combine in a fixed butterfly, thread 0 adds the four wave sums in order.
//   The second launch stages the partials in LDS and thread 0 adds them in index order.
#include "common.h"
#include "catseg_optim.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kGridCap = 8192;                 // blocks of the update kernels (adam_kernel's cap; with 2048 the option-free launch measured 386 us against 363 us on 73 M floats)
constexpr int kNormMaxBlocks = 1024;           // partials of the norm (8 KB of LDS in the second launch)
constexpr long long kNormMinVecPerBlock = 2048;

struct HyperRow { float f[CATSEG_OPTIM_HYPER_FLOATS]; };

__device__ __forceinline__ void stage_hyper(float* sh, const HyperRow& hv, const float* __restrict__ hyper) {
  if (threadIdx.x < CATSEG_OPTIM_HYPER_FLOATS) sh[threadIdx.x] = hyper ? hyper[threadIdx.x] : hv.f[threadIdx.x];
  __syncthreads();
}

// One element of the Adam update.  Contraction is off in this file and every fused multiply-add is spelled out, so that the bits do not
// depend on what the compiler chooses to fuse.  FUSED = true is what it made of adam_kernel's vector path (csrc/lovasz.hip):
// m = fma(m, b1, g (1 - b1)), v = fma(v, b2, (g g) (1 - b2)), p = fma(-(lr / bc1), q, p); FUSED = false leaves the two moment sums unfused.
template <int WD, bool AMS, bool CLIP, bool FUSED>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float* vx, float lr, float wd, float step_size, float bc2s,
                                         float gscale, float cl, float b1, float b2, float eps) {
  g = g * gscale;
  if (CLIP) g = g * cl;
  if (WD == CATSEG_WD_COUPLED) g = __builtin_fmaf(wd, p, g);
  if (WD == CATSEG_WD_DECOUPLED) p = p * __builtin_fmaf(-lr, wd, 1.f);
  const float tm = g * (1.f - b1), tv = (g * g) * (1.f - b2);
  m = FUSED ? __builtin_fmaf(m, b1, tm) : m * b1 + tm;
  v = FUSED ? __builtin_fmaf(v, b2, tv) : v * b2 + tv;
  float d = v;
  if (AMS) {
    d = fmaxf(*vx, v);
    *vx = d;
  }
  p = __builtin_fmaf(-step_size, m / (sqrtf(d) / bc2s + eps), p);
}

template <int WD, bool AMS, bool CLIP>
__global__ __launch_bounds__(256) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ vmax, long long n4, long long n,
                                                      const uint8_t* __restrict__ map, const HyperRow hv, const float* __restrict__ hyper,
                                                      float b1, float b2, float eps, const float* __restrict__ clip) {
  __shared__ float sh[CATSEG_OPTIM_HYPER_FLOATS];
  stage_hyper(sh, hv, hyper);
  const float bc1 = sh[0], bc2s = sh[1], gscale = sh[2];
  const float cl = CLIP ? clip[1] : 1.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    const int gid = map ? (int)map[e >> 6] : 0;
    if (e + 3 < n) {
      const f32x4 gg = *(const f32x4*)(g + e);
      f32x4 mm = *(f32x4*)(m + e);
      f32x4 vv = *(f32x4*)(v + e);
      f32x4 pp = *(f32x4*)(p + e);
      f32x4 vx = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (AMS) vx = *(f32x4*)(vmax + e);
      const float lr = sh[4 + 2 * gid], wd = WD != CATSEG_WD_NONE ? sh[5 + 2 * gid] : 0.f;
      const float step_size = lr / bc1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pk = pp[k], mk = mm[k], vk = vv[k], xk = vx[k];
        adam_one<WD, AMS, CLIP, true>(pk, gg[k], mk, vk, &xk, lr, wd, step_size, bc2s, gscale, cl, b1, b2, eps);
        pp[k] = pk; mm[k] = mk; vv[k] = vk; vx[k] = xk;
      }
      *(f32x4*)(m + e) = mm; *(f32x4*)(v + e) = vv; *(f32x4*)(p + e) = pp;
      if (AMS) *(f32x4*)(vmax + e) = vx;
    } else {
      // the last 1..3 elements of a buffer whose length is no multiple of 4 (never a FlatParams buffer).  adam_kernel's remainder loop,
      // as compiled, runs pairs with the fused sums and an odd last element with the unfused ones; spelled out here for the same bits.
      const float lr = sh[4 + 2 * gid], wd = WD != CATSEG_WD_NONE ? sh[5 + 2 * gid] : 0.f;
      const float step_size = lr / bc1;
      const long long paired = e + ((n - e) & ~1ll);
      for (long long j = e; j < n; ++j) {
        float pj = p[j], mj = m[j], vj = v[j], xj = AMS ? vmax[j] : 0.f;
        if (j < paired)
          adam_one<WD, AMS, CLIP, true>(pj, g[j], mj, vj, &xj, lr, wd, step_size, bc2s, gscale, cl, b1, b2, eps);
        else
          adam_one<WD, AMS, CLIP, false>(pj, g[j], mj, vj, &xj, lr, wd, step_size, bc2s, gscale, cl, b1, b2, eps);
        p[j] = pj; m[j] = mj; v[j] = vj;
        if (AMS) vmax[j] = xj;
      }
    }
  }
}

template <bool MOM, bool CLIP>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n4,
                                                  long long n, const uint8_t* __restrict__ map, const HyperRow hv,
                                                  const float* __restrict__ hyper, float mu, int nesterov, int use_wd,
                                                  const float* __restrict__ clip) {
  __shared__ float sh[CATSEG_OPTIM_HYPER_FLOATS];
  stage_hyper(sh, hv, hyper);
  const float gscale = sh[2], keep = 1.f - sh[3];
  const float cl = CLIP ? clip[1] : 1.f;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 4;
    const int gid = map ? (int)map[e >> 6] : 0;
    if (e + 3 < n) {
      f32x4 gg = *(const f32x4*)(g + e);
      f32x4 pp = *(f32x4*)(p + e);
      f32x4 bb;
      if (MOM) bb = *(f32x4*)(buf + e);
      const float lr = sh[4 + 2 * gid], wd = use_wd ? sh[5 + 2 * gid] : 0.f;
      gg = gg * gscale;
      if (CLIP) gg = gg * cl;
      if (use_wd) gg = gg + pp * wd;
      f32x4 u = gg;
      if (MOM) {
        bb = bb * mu + gg * keep;
        *(f32x4*)(buf + e) = bb;
        u = nesterov ? gg + bb * mu : bb;
      }
      pp = pp - u * lr;
      *(f32x4*)(p + e) = pp;
    } else {
      const float lr = sh[4 + 2 * gid], wd = use_wd ? sh[5 + 2 * gid] : 0.f;
      for (long long j = e; j < n; ++j) {
        float gg = g[j] * gscale;
        const float pp = p[j];
        if (CLIP) gg = gg * cl;
        if (use_wd) gg = gg + pp * wd;
        float u = gg;
        if (MOM) {
          const float bb = buf[j] * mu + gg * keep;
          buf[j] = bb;
          u = nesterov ? gg + bb * mu : bb;
        }
        p[j] = pp - u * lr;
      }
    }
  }
}

__device__ __forceinline__ double sq4(const f32x4 q, double acc) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double d = (double)q[k];
    acc += d * d;
  }
  return acc;
}

__global__ __launch_bounds__(256) void grad_sq_kernel(const float* __restrict__ g, long long n4, long long n, long long slice,
                                                      double* __restrict__ partial) {
  __shared__ double wsum[kThreads / 64];
  const long long v0 = (long long)blockIdx.x * slice;
  const long long v1 = v0 + slice < n4 ? v0 + slice : n4;
  const long long nfull = n >> 2;               // vectors that lie wholly inside [0, n)
  double acc = 0.0;
  for (long long i = v0 + threadIdx.x; i < v1; i += 4 * kThreads) {
    f32x4 q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {               // four loads in flight before the first use
      const long long j = i + (long long)k * kThreads;
      q[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (j < v1) {
        if (j < nfull) {
          q[k] = *(const f32x4*)(g + j * 4);
        } else {                                // the one partial vector at the end of the buffer
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (j * 4 + c < n) q[k][c] = g[j * 4 + c];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = sq4(q[k], acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partial, int nb, float gscale,
                                                              const float* __restrict__ hyper, float max_norm, float* __restrict__ out) {
  __shared__ double sh[kNormMaxBlocks];
  for (int i = threadIdx.x; i < nb; i += kThreads) sh[i] = partial[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    if (hyper) gscale = hyper[2];
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += sh[i];
    const float norm = (float)(sqrt(s) * fabs((double)gscale));
    out[0] = norm;
    out[1] = fminf(1.f, max_norm / (norm + 1e-6f));
  }
}

inline long long norm_blocks(long long n) {
  const long long n4 = (n + 3) / 4;
  long long nb = (n4 + kNormMinVecPerBlock - 1) / kNormMinVecPerBlock;
  return nb < 1 ? 1 : (nb > kNormMaxBlocks ? kNormMaxBlocks : nb);
}

inline bool load_row(const float* hyper_host, HyperRow* hv) {
  for (int k = 0; k < CATSEG_OPTIM_HYPER_FLOATS; ++k) hv->f[k] = hyper_host ? hyper_host[k] : 0.f;
  return true;
}

template <int WD, bool AMS>
void launch_adam(bool clip_on, dim3 grid, hipStream_t st, float* p, const float* g, float* m, float* v, float* vmax, long long n4, long long n,
                 const uint8_t* map, const HyperRow& hv, const float* hyper, float b1, float b2, float eps, const float* clip) {
  if (clip_on)
    hipLaunchKernelGGL((adam_ex_kernel<WD, AMS, true>), grid, dim3(kThreads), 0, st, p, g, m, v, vmax, n4, n, map, hv, hyper, b1, b2, eps, clip);
  else
    hipLaunchKernelGGL((adam_ex_kernel<WD, AMS, false>), grid, dim3(kThreads), 0, st, p, g, m, v, vmax, n4, n, map, hv, hyper, b1, b2, eps, clip);
}

}  // namespace

#define ADAM_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_adam_step_ex: " msg)
#define SGD_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_sgd_step: " msg)
#define NORM_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_grad_norm: " msg)

extern "C" int catseg_optim_grid_cap(void) { return kGridCap; }

extern "C" void catseg_optim_hyper(int step, float beta1, float beta2, float grad_scale, float dampening, int G, const float* lr, const float* wd,
                                   float* row) {
  const int s = step < 1 ? 1 : step;
  row[0] = (float)(1.0 - pow((double)beta1, s));
  row[1] = (float)sqrt(1.0 - pow((double)beta2, s));
  row[2] = grad_scale;
  row[3] = s <= 1 ? 0.f : dampening;
  for (int k = 0; k < CATSEG_OPTIM_MAX_GROUPS; ++k) {
    const bool on = k < G && lr && wd;
    row[4 + 2 * k] = on ? lr[k] : 0.f;
    row[5 + 2 * k] = on ? wd[k] : 0.f;
  }
}

extern "C" int catseg_adam_step_ex(float* p, const float* g, float* m, float* v, float* vmax, long long n, const uint8_t* group_of_chunk, int G,
                                   const float* hyper_host, const float* hyper_dev, float beta1, float beta2, float eps, int wd_mode,
                                   const float* clip, catseg_stream_t stream) {
  ADAM_REQUIRE(n > 0, "n must be positive");
  ADAM_REQUIRE(p && g && m && v, "p, g, m and v are required");
  ADAM_REQUIRE(cs_aligned16(p) && cs_aligned16(g) && cs_aligned16(m) && cs_aligned16(v) && cs_aligned16(vmax), "buffers must be 16-byte aligned");
  ADAM_REQUIRE(G >= 1 && G <= CATSEG_OPTIM_MAX_GROUPS, "G must be in 1..8");
  ADAM_REQUIRE((hyper_host != nullptr) != (hyper_dev != nullptr), "exactly one of hyper_host and hyper_dev");
  ADAM_REQUIRE(wd_mode >= CATSEG_WD_NONE && wd_mode <= CATSEG_WD_DECOUPLED, "unknown wd_mode");
  ADAM_REQUIRE((((uintptr_t)clip) & 3) == 0 && (((uintptr_t)hyper_dev) & 3) == 0, "clip and hyper_dev must be 4-byte aligned");
  HyperRow hv;
  load_row(hyper_host, &hv);
  const long long n4 = (n + 3) / 4;
  const dim3 grid(cs_grid_256(n4, kGridCap));
  hipStream_t st = (hipStream_t)stream;
  const bool c = clip != nullptr;
#define ADAM_GO(WD, AMS) launch_adam<WD, AMS>(c, grid, st, p, g, m, v, vmax, n4, n, group_of_chunk, hv, hyper_dev, beta1, beta2, eps, clip)
  if (vmax) {
    if (wd_mode == CATSEG_WD_NONE) ADAM_GO(CATSEG_WD_NONE, true);
    else if (wd_mode == CATSEG_WD_COUPLED) ADAM_GO(CATSEG_WD_COUPLED, true);
    else ADAM_GO(CATSEG_WD_DECOUPLED, true);
  } else {
    if (wd_mode == CATSEG_WD_NONE) ADAM_GO(CATSEG_WD_NONE, false);
    else if (wd_mode == CATSEG_WD_COUPLED) ADAM_GO(CATSEG_WD_COUPLED, false);
    else ADAM_GO(CATSEG_WD_DECOUPLED, false);
  }
#undef ADAM_GO
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_sgd_step(float* p, const float* g, float* buf, long long n, const uint8_t* group_of_chunk, int G, const float* hyper_host,
                               const float* hyper_dev, float momentum, int nesterov, int use_wd, const float* clip, catseg_stream_t stream) {
  SGD_REQUIRE(n > 0, "n must be positive");
  SGD_REQUIRE(p && g, "p and g are required");
  SGD_REQUIRE(cs_aligned16(p) && cs_aligned16(g) && cs_aligned16(buf), "buffers must be 16-byte aligned");
  SGD_REQUIRE(G >= 1 && G <= CATSEG_OPTIM_MAX_GROUPS, "G must be in 1..8");
  SGD_REQUIRE((hyper_host != nullptr) != (hyper_dev != nullptr), "exactly one of hyper_host and hyper_dev");
  SGD_REQUIRE(!nesterov || buf, "nesterov needs the momentum buffer");
  SGD_REQUIRE((((uintptr_t)clip) & 3) == 0 && (((uintptr_t)hyper_dev) & 3) == 0, "clip and hyper_dev must be 4-byte aligned");
  HyperRow hv;
  load_row(hyper_host, &hv);
  const long long n4 = (n + 3) / 4;
  const dim3 grid(cs_grid_256(n4, kGridCap));
  hipStream_t st = (hipStream_t)stream;
#define SGD_GO(MOM, CLIP)                                                                                                             \
  hipLaunchKernelGGL((sgd_kernel<MOM, CLIP>), grid, dim3(kThreads), 0, st, p, g, buf, n4, n, group_of_chunk, hv, hyper_dev, momentum, \
                     nesterov ? 1 : 0, use_wd ? 1 : 0, clip)
  if (buf) {
    if (clip) SGD_GO(true, true); else SGD_GO(true, false);
  } else {
    if (clip) SGD_GO(false, true); else SGD_GO(false, false);
  }
#undef SGD_GO
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" size_t catseg_grad_norm_workspace(long long n) { return n > 0 ? (size_t)norm_blocks(n) * sizeof(double) : 0; }

extern "C" int catseg_grad_norm(const float* g, long long n, float grad_scale, const float* hyper_dev, float max_norm, void* workspace,
                                size_t workspace_bytes, float* out, catseg_stream_t stream) {
  NORM_REQUIRE(n > 0, "n must be positive");
  NORM_REQUIRE(g && cs_aligned16(g), "g is required and must be 16-byte aligned");
  NORM_REQUIRE(workspace != nullptr, "the workspace is NULL");
  NORM_REQUIRE((((uintptr_t)workspace) & 7) == 0, "the workspace must be 8-byte aligned");
  NORM_REQUIRE(workspace_bytes >= catseg_grad_norm_workspace(n), "the workspace is smaller than catseg_grad_norm_workspace(n)");
  NORM_REQUIRE(out && (((uintptr_t)out) & 7) == 0, "out is required and must be 8-byte aligned");
  NORM_REQUIRE((((uintptr_t)hyper_dev) & 3) == 0, "hyper_dev must be 4-byte aligned");
  NORM_REQUIRE(max_norm >= 0.f, "max_norm must not be negative or NaN");
  const long long n4 = (n + 3) / 4, nb = norm_blocks(n), slice = (n4 + nb - 1) / nb;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_sq_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, g, n4, n, slice, (double*)workspace);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)workspace, (int)nb, grad_scale, hyper_dev, max_norm, out);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
