// The source index and the two taps of one output position of a bilinear resize (ATen's arithmetic in fp32), shared by the resize kernels
// (csrc/pointwise.hip) and the skip-junction kernel (csrc/unet.hip): one definition, so that both evaluate the same expression.
#pragma once
#include "common.h"

// ATen's area_pixel_compute_source_index in fp32
__device__ __forceinline__ float src_index(float scale, int dst, bool align) {
  if (align) return scale * dst;
  const float s = scale * (dst + 0.5f) - 0.5f;
  return s < 0.f ? 0.f : s;
}
// (no contraction of scale * dst with the subtraction below: where `align` is a compile-time constant the compiler would otherwise form one fma
//  and the weights would differ in the last bit from those of the kernels that take `align` as an argument)
__device__ __forceinline__ void lerp_setup(float scale, int dst, bool align, int in_size, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  const float s = src_index(scale, dst, align);
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = s - i0;
  l0 = 1.f - l1;
}
__host__ __device__ inline float resize_scale(int in, int out, bool align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}
