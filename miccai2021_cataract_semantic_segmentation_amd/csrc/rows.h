// Pixel-row staging shared by the per-pixel loss kernels (lovasz.hip, overlap.hip): logits [P][K] <-> LDS rows of stride KS (odd).
#pragma once
#include "common.h"

namespace {

// ---- stage a block of PIX pixels x K logits into LDS, row stride KS (odd).  The block's span starts at p0 * K floats with
// p0 a multiple of PIX, so it is 16-byte aligned whenever the tensor is: 16-byte global accesses (a scalar dword per lane
// moves ~1/4 of the bytes per request), one integer division per four elements instead of one each.
__device__ __forceinline__ void stage_rows(const float* __restrict__ logits, long long p0, int np, int K, int KS, float* sh) {
  const int n = np * K;
  const float* src = logits + p0 * K;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    const int n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    // Eight 16-byte loads per thread IN FLIGHT, then their LDS stores (a load -> LDS store loop waits for every load in turn -- the compiler
    // cannot move a global load over an LDS store through a generic pointer: 256 x 25 floats were 7 dependent HBM round trips per block and
    // the per-pixel kernels ran at ~2 TB/s)
    for (int base = 0; base < n4; base += 8 * blockDim.x) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i4 = base + u * blockDim.x + threadIdx.x;
        v[u] = i4 < n4 ? s4[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i4 = base + u * blockDim.x + threadIdx.x;
        if (i4 < n4) {
          const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
          int r = (4 * i4) / K, c = 4 * i4 - r * K;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            sh[r * KS + c] = e[q];
            if (++c == K) { c = 0; ++r; }
          }
        }
      }
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += blockDim.x) {
    const int r = i / K, c = i - r * K;
    sh[r * KS + c] = src[i];
  }
}
// the reverse: rows of the LDS image to global (acc: added to what is there)
__device__ __forceinline__ void unstage_rows(float* __restrict__ out, long long p0, int np, int K, int KS, const float* sh, bool acc) {
  const int n = np * K;
  float* dst = out + p0 * K;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const int n4 = n >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i4 = threadIdx.x; i4 < n4; i4 += blockDim.x) {
      float e[4];
      int r = (4 * i4) / K, c = 4 * i4 - r * K;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        e[u] = sh[r * KS + c];
        if (++c == K) { c = 0; ++r; }
      }
      float4 v = make_float4(e[0], e[1], e[2], e[3]);
      if (acc) {
        const float4 o = d4[i4];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      d4[i4] = v;
    }
    done = n4 << 2;
  }
  for (int i = done + threadIdx.x; i < n; i += blockDim.x) {
    const int r = i / K, c = i - r * K;
    const float v = sh[r * KS + c];
    dst[i] = acc ? dst[i] + v : v;
  }
}

}  // namespace
