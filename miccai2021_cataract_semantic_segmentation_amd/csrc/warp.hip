// Geometric augmentation fused into the ingest (reference: AffineNP with crop_to_fit=False, CropNP, PadNP after FlipNP and remap_mask;
// utils/transforms.py:23-61, 254-303, wired at utils/utils.py:356-401):
//   the reference warps [image | ones | K-channel one-hot] as float64 onto a 2H x 2W canvas (cv2.warpPerspective, bilinear, constant border 0),
//   rounds the colours, takes the argmax of the one-hot channels and then crops a window out of the canvas.
// Here: one thread per output pixel OF THE WINDOW, one gather of up to four source pixels; the one-hot never exists.
//   coordinates: fp64, X = rint(((m00 x + m01 y) + m02) * 32), every operation rounded on its own (no FMA), 5 fractional bits as OpenCV's
//                fixed-point remap (INTER_BITS = 5); the bilinear weights are integers over 1024, so everything after X, Y is exact:
//   colour:      N = sum p * w <= 255 * 1024, result = N / 1024 rounded half to even (np.round);
//   label:       the weights of the in-frame neighbours summed per remapped label; largest sum wins, ties to the smaller id, none -> 0 (np.argmax).
// Every source read is guarded by a bounds test in the flipped frame's coordinates: whatever the matrix / origin hold, the worst case is zeros.
// HBM-bound: <= 4 x 4 B read (neighbours share cache lines), 12 (+16) (+3) + 8 B written per pixel; ~10 fp64 operations beside it.
#include "common.h"
#include "catseg_ingest_tables.h"
#include "warp_label.h"

namespace {

__device__ __forceinline__ int reflect(int r, int n) {  // np.pad(mode='reflect'): no edge repeat
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  r = r % period;
  if (r < 0) r += period;
  return r < n ? r : period - r;
}

__global__ __launch_bounds__(256) void ingest_warp_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lbl, int B, int H, int W,
                                                          const uint8_t* __restrict__ luts, int T,
                                                          const int32_t* __restrict__ table_of_frame, const int32_t* __restrict__ flips,
                                                          const double* __restrict__ minv, int Hc, int Wc, const int32_t* __restrict__ origin,
                                                          int Ww, int pad_top, int Ho, const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, float* __restrict__ x_nchw, float* __restrict__ x_nhwc4,
                                                          uint8_t* __restrict__ x_u8, int64_t* __restrict__ labels) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // row-major over the window: a wave's pixels gather neighbouring source pixels
  const long long n = (long long)B * Ho * Ww;
  if (i >= n) return;
  const int c = (int)(i % Ww);
  const long long t = i / Ww;
  const int r = (int)(t % Ho), b = (int)(t / Ho);
  const int f = flips ? flips[b] : 0;
  // canvas pixel of this output pixel (padding: only with a window as tall as the canvas, so the reflected row is a canvas row)
  const long long cy = (long long)reflect(r - pad_top, Hc) + (origin ? origin[2 * b] : 0);
  const long long cx = (long long)c + (origin ? origin[2 * b + 1] : 0);
  int wt[4];
  long long src[4];
  warp_taps(minv ? minv + (long long)b * 6 : nullptr, b, f, cy, cx, H, W, Hc, Wc, wt, src);   // csrc/warp_label.h, shared with cropfreq.hip
  if (img) {
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (wt[k] > 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)img[src[k] * 3 + ch] * wt[k];
      }
    float v[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int q = acc[ch] >> 10, rem = acc[ch] & 1023;
      const int u = q + ((rem > 512 || (rem == 512 && (q & 1))) ? 1 : 0);   // np.round: half to even
      if (x_u8) x_u8[i * 3 + ch] = (uint8_t)u;
      float p = __fdiv_rn((float)u, 255.0f);  // ToTensor: correctly rounded division, as torch's .div(255)
      if (mean) {
        p = __fsub_rn(p, mean[ch]);           // Normalize: sub_ then div_, two roundings, no contraction
        p = __fdiv_rn(p, stdv[ch]);
      }
      v[ch] = p;
    }
    if (x_nchw) {
      const long long plane = (long long)Ho * Ww;
      float* o = x_nchw + (long long)b * 3 * plane + (long long)r * Ww + c;
      o[0] = v[0]; o[plane] = v[1]; o[2 * plane] = v[2];
    }
    if (x_nhwc4) *reinterpret_cast<float4*>(x_nhwc4 + i * 4) = make_float4(v[0], v[1], v[2], 0.f);
  }
  if (lbl) labels[i] = (int64_t)warp_label(lbl, label_table_row(luts, T, table_of_frame, b), wt, src);   // (the index is clamped into [0, T))
}

#define WARP_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_ingest_warp_u8: " msg)

// the one launch behind both entry points (luts: [T][256], table_of_frame: [B] or null = row 0)
int warp_launch(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T, const int32_t* table_of_frame,
                const int32_t* flips, const double* minv, int Hc, int Wc, const int32_t* origin, int Hw, int Ww, int pad_top, int pad_bottom,
                const float* mean, const float* stdv, float* x_nchw, float* x_nhwc4, uint8_t* x_u8, int64_t* labels, catseg_stream_t stream) {
  WARP_REQUIRE(B > 0 && H > 0 && W > 0 && Hc > 0 && Wc > 0 && Hw > 0 && Ww > 0 && pad_top >= 0 && pad_bottom >= 0, "bad dims");
  WARP_REQUIRE(H <= 16384 && W <= 16384 && Hc <= 16384 && Wc <= 16384, "frame and canvas are limited to 16384 x 16384");
  WARP_REQUIRE(Hw <= Hc && Ww <= Wc, "the window must fit into the canvas");
  WARP_REQUIRE(minv != nullptr || (Hc == H && Wc == W), "without a matrix the canvas is the frame");
  WARP_REQUIRE(pad_top < Hc && pad_bottom < Hc, "reflect padding must be smaller than the canvas (np.pad 'reflect')");
  WARP_REQUIRE((pad_top == 0 && pad_bottom == 0) || Hw == Hc, "padding needs a window as tall as the canvas (PadNP runs only without a crop)");
  WARP_REQUIRE((img == nullptr) == (x_nchw == nullptr && x_nhwc4 == nullptr && x_u8 == nullptr), "image input and image outputs go together");
  WARP_REQUIRE((lbl == nullptr) == (labels == nullptr), "label input and label output go together");
  WARP_REQUIRE(img != nullptr || lbl != nullptr, "nothing to do");
  WARP_REQUIRE((mean == nullptr) == (stdv == nullptr), "mean and std go together");
  WARP_REQUIRE(x_nhwc4 == nullptr || cs_aligned16(x_nhwc4), "NHWC-4 output must be 16-byte aligned");
  WARP_REQUIRE((((uintptr_t)minv) & 7) == 0, "the matrices must be 8-byte aligned");
  const int Ho = Hw + pad_top + pad_bottom;
  const long long n = (long long)B * Ho * Ww;
  WARP_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "too many output pixels for one launch");
  hipLaunchKernelGGL(ingest_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, lbl, B, H, W, luts, T,
                     table_of_frame, flips, minv, Hc, Wc, origin, Ww, pad_top, Ho, mean, stdv, x_nchw, x_nhwc4, x_u8, labels);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

}  // namespace

extern "C" int catseg_ingest_warp_u8(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, const int32_t* flips,
                                     const double* minv, int Hc, int Wc, const int32_t* origin, int Hw, int Ww, int pad_top, int pad_bottom,
                                     const float* mean, const float* stdv, float* x_nchw, float* x_nhwc4, uint8_t* x_u8, int64_t* labels,
                                     catseg_stream_t stream) {
  return warp_launch(img, lbl, B, H, W, lut, 1, nullptr, flips, minv, Hc, Wc, origin, Hw, Ww, pad_top, pad_bottom, mean, stdv, x_nchw, x_nhwc4,
                     x_u8, labels, stream);
}

extern "C" int catseg_ingest_warp_u8_tables(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T,
                                            const int32_t* table_of_frame, const int32_t* flips, const double* minv, int Hc, int Wc,
                                            const int32_t* origin, int Hw, int Ww, int pad_top, int pad_bottom, const float* mean,
                                            const float* stdv, float* x_nchw, float* x_nhwc4, uint8_t* x_u8, int64_t* labels,
                                            catseg_stream_t stream) {
  WARP_REQUIRE(T >= 1 && (luts != nullptr || table_of_frame == nullptr), "a table index needs T >= 1 tables");
  WARP_REQUIRE((((uintptr_t)table_of_frame) & 3) == 0, "the table index must be 4-byte aligned");
  return warp_launch(img, lbl, B, H, W, luts, T, table_of_frame, flips, minv, Hc, Wc, origin, Hw, Ww, pad_top, pad_bottom, mean, stdv, x_nchw,
                     x_nhwc4, x_u8, labels, stream);
}
