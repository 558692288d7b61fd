// Split reductions of the backward-weight kernels: every split of the pixel range writes its partial dw into a slab of the workspace, a
// second launch adds the slabs in a fixed order (deterministic).  The two reducers, and the split planning the bf16x3 and f16x2
// implicit-GEMM backward-weight share.  Kernels and helpers have internal linkage: one copy per translation unit that uses them -- the
// reducers and their launchers are templates (of nothing) for that alone: a plain __global__ function is emitted into the code object of every
// file that includes this header, an instantiation only where it is launched.
#pragma once
#include "common.h"

namespace {

// out[i] = sum_s slab[s][i], one chain per float4 (few slabs of a large tensor)
template <int = 0>
__global__ void cs_reduce_slabs_kernel(const float* __restrict__ slabs, float* __restrict__ out, long long n4, int splits, long long stride4) {
  const f32x4* s = (const f32x4*)slabs;
  f32x4* o = (f32x4*)out;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    f32x4 a = s[i];
    for (int k = 1; k < splits; ++k) a += s[i + k * stride4];
    o[i] = a;
  }
}
// n4 float4 per slab, slabs back to back; at most max_blocks blocks
template <int = 0>
void cs_launch_reduce_slabs(const float* slabs, float* out, long long n4, int splits, int max_blocks, hipStream_t st) {
  hipLaunchKernelGGL(cs_reduce_slabs_kernel<>, dim3(cs_grid_256(n4, max_blocks)), dim3(256), 0, st, slabs, out, n4, splits, n4);
}

// the same for many slabs of a small tensor (the direct 3 x 3 backward-weight kernels): 64 float4 columns (1 KB contiguous per slab row) x 4
// slab lanes per block, each lane adds every 4th slab with four independent load chains, fixed-order combine over the lanes
template <int = 0>
__global__ __launch_bounds__(256) void cs_reduce_slabs4_kernel(const float* __restrict__ slabs, float* __restrict__ dw, long long n4, int splits,
                                                               long long slab_stride4) {
  __shared__ f32x4 sh[4][64];
  const int c = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const long long col = (long long)blockIdx.x * 64 + c;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  if (col < n4) {
    const f32x4* p = (const f32x4*)slabs + col;
    int k = sl;
    for (; k + 12 < splits; k += 16) {
      s0 += p[(long long)k * slab_stride4];
      s1 += p[(long long)(k + 4) * slab_stride4];
      s2 += p[(long long)(k + 8) * slab_stride4];
      s3 += p[(long long)(k + 12) * slab_stride4];
    }
    for (; k < splits; k += 4) s0 += p[(long long)k * slab_stride4];
  }
  sh[sl][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && col < n4) ((f32x4*)dw)[col] = (sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c]);
}
template <int = 0>
void cs_launch_reduce_slabs4(const float* slabs, float* dw, long long n4, int splits, hipStream_t st) {
  hipLaunchKernelGGL(cs_reduce_slabs4_kernel<>, dim3((unsigned)((n4 + 63) / 64)), dim3(256), 0, st, slabs, dw, n4, splits, n4);
}

// ---- the 256 x 256-tile split-precision backward-weight GEMM  dw[Cout][taps * Cin] = sum over the P = B Ho Wo output pixels ----------------
// splits of the pixel range for `tiles` output tiles: the count that fills the 256 CUs best
inline int cs_wgrad_splits(int tiles, long long P) {
  int best = 1;
  double best_fill = 0.0;
  for (int sp = 1; sp <= 64; ++sp) {
    if (P / sp < 2048 && sp > 1) break;                 // at least 128 K-steps per block
    const double rounds = (double)tiles * sp / 256.0;
    const double fill = rounds / (double)(long long)(rounds + 0.999999);
    if (fill > best_fill + 0.01) { best_fill = fill; best = sp; }
  }
  return best;
}

struct CsWgradPlan {
  long long P;
  int N, tilesM, tilesN, splits;   // splits: as planned (the launch may need fewer once the rows per split are rounded up to 16)
  size_t workspace_bytes;          // the slabs; 0 when one split writes dw itself
};
inline CsWgradPlan cs_wgrad_plan(const catseg_conv_desc* d) {
  CsWgradPlan pl;
  pl.P = (long long)d->B * d->Ho * d->Wo;
  pl.N = d->kh * d->kw * d->Cin;
  pl.tilesM = (d->Cout + 255) / 256; pl.tilesN = (pl.N + 255) / 256;
  pl.splits = cs_wgrad_splits(pl.tilesM * pl.tilesN, pl.P);
  pl.workspace_bytes = pl.splits > 1 ? cs_align_up((size_t)pl.splits * d->Cout * pl.N * 4, 256) : 0;
  return pl;
}
// the fields B3TArgs and H2TArgs carry under the same names (operand planes, scales and layout flags stay with their file); returns the
// number of slabs the launch writes: 1 = straight into dw, otherwise into `workspace`, to be reduced
template <class Args>
int cs_wgrad_fill(Args& a, const catseg_conv_desc* d, const CsWgradPlan& pl, float* dw, void* workspace) {
  a.P = (int)pl.P;
  a.M = d->Cout; a.Cin = d->Cin; a.taps = d->kh * d->kw; a.N = pl.N;
  a.ldo = (d->Cout + 7) & ~7; a.ldx = d->Cin;
  cs_fill_geometry(a, d);
  const int img = d->Ho * d->Wo;
  a.step_b = 16 / img; a.step_qy = (16 % img) / d->Wo; a.step_rx = (16 % img) % d->Wo;
  a.tilesM = pl.tilesM; a.tilesN = pl.tilesN;
  a.rows_per_split = (int)(((pl.P + pl.splits - 1) / pl.splits + 15) / 16 * 16);
  const int sp = (a.P + a.rows_per_split - 1) / a.rows_per_split;
  a.ldc = a.N; a.c_split_stride = (long long)a.M * a.N;
  a.C = sp > 1 ? (float*)workspace : dw;
  return sp;
}

}  // namespace
