// Philox4x32-10, the generator of every device-side draw (csrc/dropout.hip: the Dropout2d masks; csrc/pointrend_train.hip: PointRend's training
// points; csrc/contrast.hip: the anchors of the dense contrastive loss).  A draw is philox4x32_10(counter, key = (seed lo, seed hi)) with counter = (group of four elements, draw number, STREAM,
// layer | rank << 16): the STREAM word keeps the consumers apart (PHILOX_STREAM_DROPOUT, PHILOX_STREAM_POINTS, PHILOX_STREAM_ANCHORS), so that two of them seeded
// alike never share a block of random bits.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned ph_u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned PHILOX_STREAM_DROPOUT = 0u, PHILOX_STREAM_POINTS = 1u, PHILOX_STREAM_ANCHORS = 2u;

__device__ __forceinline__ ph_u32x4 philox4x32_10(ph_u32x4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c = ph_u32x4{hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
