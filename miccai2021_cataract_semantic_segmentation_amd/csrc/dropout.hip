// nn.Dropout2d of the OCRNet heads (reference: models/OCR.py:87 interm_prediction_head[3], :311-316 conv_bn_dropout[3]): one keep decision per
// (image, channel), the kept channels scaled by 1 / (1 - p).
//   catseg_dropout2d_mask        draws the [B][C] multipliers (and their packed bits) with Philox4x32-10 from 16 bytes of DEVICE state and
//                                advances the draw counter in the same launch: no host value enters a draw, so a captured step replays the
//                                launch and gets the next mask
//   catseg_dropout2d_mask_fixed  the same two tables from a given 0 / 1 table (tests inject a mask)
//   catseg_dropout2d_apply       out[row][c] = x[row][c] * mult[row / HW][c] over NHWC rows, 16-byte accesses -- forward and backward of the
//                                routes that do not run the fused head kernels (csrc/headfuse.h applies the bits in registers)
// The draw: element i = n C + c takes word i & 3 of philox4x32_10(counter = (i >> 2, draw, 0, layer | rank << 16), key = (seed lo, seed hi)),
// u = (word >> 8) 2^-24, kept iff u >= p.
#include "common.h"
#include "philox.h"

namespace {

typedef ph_u32x4 dr_u32x4;

// ONE block.  A thread owns spans of 32 consecutive elements (= one word of `bits` where C % 32 == 0: n C + c is then linear in the words).
// fixed == nullptr: a draw; every thread reads the state in front of the barrier, thread 0 stores the advanced counter behind it.
constexpr int kMaskThreads = 256;
__global__ __launch_bounds__(kMaskThreads) void dropout2d_mask_kernel(unsigned* __restrict__ state, const float* __restrict__ fixed, float p,
                                                                      float keep, int total, float* __restrict__ mult,
                                                                      unsigned* __restrict__ bits) {
  unsigned s0 = 0, s1 = 0, s2 = 0, draw = 0;
  if (fixed == nullptr) {
    s0 = state[0];
    s1 = state[1];
    s2 = state[2];
    draw = state[3];
    __syncthreads();
    if (threadIdx.x == 0) state[3] = draw + 1u;
  }
  const int spans = (total + 31) >> 5;
  for (int w = threadIdx.x; w < spans; w += kMaskThreads) {
    unsigned word = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i0 = 32 * w + 4 * q;
      if (i0 >= total) break;
      dr_u32x4 r = {0u, 0u, 0u, 0u};
      if (fixed == nullptr) r = philox4x32_10(dr_u32x4{(unsigned)(i0 >> 2), draw, PHILOX_STREAM_DROPOUT, s2}, s0, s1);
      f32x4 m;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bool kept;
        if (fixed == nullptr) kept = (float)(r[e] >> 8) * 0x1p-24f >= p;
        else kept = i0 + e < total && fixed[i0 + e] != 0.f;
        m[e] = kept ? keep : 0.f;
        word |= (kept && keep != 0.f ? 1u : 0u) << (4 * q + e);
      }
      if (i0 + 4 <= total) *(f32x4*)(mult + i0) = m;
      else
        for (int e = 0; i0 + e < total; ++e) mult[i0 + e] = m[e];
    }
    if (bits != nullptr) bits[w] = word;
  }
}

__global__ __launch_bounds__(256) void dropout2d_apply_kernel(const float* x, int ldx, const float* __restrict__ mult, unsigned quads,
                                                              unsigned c4, unsigned hw, float* out, int ldo) {      // (out may be x)
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < quads; i += gridDim.x * 256u) {
    const unsigned row = i / c4, q = i - row * c4, n = row / hw;
    const f32x4 v = *(const f32x4*)(x + (long long)row * ldx + 4 * q);
    const f32x4 m = *(const f32x4*)(mult + ((long long)n * c4 + q) * 4);
    *(f32x4*)(out + (long long)row * ldo + 4 * q) = v * m;
  }
}

int mask_launch(unsigned* state, const float* fixed, float p, int B, int C, float* mult, unsigned* bits, catseg_stream_t stream) {
  CS_REQUIRE(B >= 1 && C >= 1 && (long long)B * C < (1ll << 30), "dropout2d mask: B, C >= 1 and fewer than 2^30 elements");
  CS_REQUIRE(p >= 0.f && p <= 1.f, "dropout2d mask: p must lie in [0, 1]");
  CS_REQUIRE(mult && cs_aligned16(mult) && (state || fixed), "dropout2d mask: pointers / alignment");
  CS_REQUIRE(bits == nullptr || C % 32 == 0, "dropout2d mask: the packed bits need C to be a multiple of 32");
  const float keep = p < 1.f ? 1.f / (1.f - p) : 0.f;      // (p == 1: everything dropped, no division)
  hipLaunchKernelGGL(dropout2d_mask_kernel, dim3(1), dim3(kMaskThreads), 0, (hipStream_t)stream, state, fixed, p, keep, B * C, mult, bits);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

}  // namespace

extern "C" int catseg_dropout2d_mask(void* state, float p, int B, int C, float* mult, unsigned* bits, catseg_stream_t stream) {
  CS_REQUIRE(state && (((uintptr_t)state) & 15) == 0, "dropout2d mask: the state is 16 bytes of device memory, 16-byte aligned");
  return mask_launch((unsigned*)state, nullptr, p, B, C, mult, bits, stream);
}

extern "C" int catseg_dropout2d_mask_fixed(const float* keep01, float p, int B, int C, float* mult, unsigned* bits, catseg_stream_t stream) {
  CS_REQUIRE(keep01, "dropout2d mask: the 0 / 1 table is missing");
  return mask_launch(nullptr, keep01, p, B, C, mult, bits, stream);
}

extern "C" int catseg_dropout2d_apply(const float* x, int ldx, const float* mult, long long rows, int C, long long hw, float* out, int ldo,
                                      catseg_stream_t stream) {
  CS_REQUIRE(rows > 0 && hw > 0 && rows % hw == 0 && C >= 4 && C % 4 == 0 && ldx >= C && ldo >= C && ldx % 4 == 0 && ldo % 4 == 0,
             "dropout2d apply: rows a multiple of H W, C and both row strides multiples of 4");
  CS_REQUIRE(rows * (C / 4) < (1ll << 31) && hw < (1ll << 31), "dropout2d apply: fewer than 2^31 groups of four channels");
  CS_REQUIRE(x && mult && out && cs_aligned16(x) && cs_aligned16(mult) && cs_aligned16(out), "dropout2d apply: pointers / alignment");
  const long long quads = rows * (C / 4);
  hipLaunchKernelGGL(dropout2d_apply_kernel, dim3(cs_grid_256(quads, 8192)), dim3(256), 0, (hipStream_t)stream, x, ldx, mult, (unsigned)quads,
                     (unsigned)(C / 4), (unsigned)hw, out, ldo);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
