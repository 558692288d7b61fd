// The per-pixel source gather and the label rule of the geometric augmentation, shared by the ingest's warp (csrc/warp.hip) and the
// frequency-weighted crop pick (csrc/cropfreq.hip), so that the labels the pick weighs are the labels the warp writes:
//   coordinates: fp64, X = rint(((m00 x + m01 y) + m02) * 32), every operation rounded on its own (no FMA), 5 fractional bits as OpenCV's
//                fixed-point remap (INTER_BITS = 5); the bilinear weights are integers over 1024;
//   label:       the weights of the in-frame neighbours summed per remapped label; largest sum wins, ties to the smaller id, none -> 0 (np.argmax).
// Every source index warp_taps hands out has passed a bounds test in the flipped frame's coordinates, and a tap is read only where its weight
// is positive: whatever the matrix holds, the worst case is "no neighbour".
#pragma once
#include <stdint.h>

// fixed-point source coordinate of canvas pixel (x, y) for one row (a, b, c) of the inverse matrix
__device__ __forceinline__ int warp_coord(double a, double b, double c, double x, double y) {
#pragma clang fp contract(off)          // mul, mul, add, add, mul as five roundings: __dmul_rn / __dadd_rn alone still came out as v_fmac_f64
  const double p = a * x;
  const double q = b * y;
  const double s = p + q;
  const double t = s + c;
  double v = rint(t * 32.0);            // round half to even
  if (!(v >= -2147483648.0)) v = -2147483648.0;   // (NaN lands here too: far outside every frame)
  if (v > 2147483647.0) v = 2147483647.0;
  return (int)v;
}

// the up to four source pixels of canvas pixel (cx, cy) of frame b: wt[k] > 0 and src[k] = pixel index into the [B][H][W] input (un-flipped:
// f bit 0 = horizontal, bit 1 = vertical flip) where neighbour k lies inside the frame, wt[k] = 0 otherwise.  m: the frame's six matrix
// entries, or null = the canvas is the frame.
__device__ __forceinline__ void warp_taps(const double* __restrict__ m, int b, int f, long long cy, long long cx, int H, int W, int Hc, int Wc,
                                          int (&wt)[4], long long (&src)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { wt[k] = 0; src[k] = 0; }
  if (cy >= 0 && cy < Hc && cx >= 0 && cx < Wc) {          // (an origin outside the canvas: zeros)
    int X, Y;
    if (m) {
      const double xd = (double)(int)cx, yd = (double)(int)cy;
      X = warp_coord(m[0], m[1], m[2], xd, yd);
      Y = warp_coord(m[3], m[4], m[5], xd, yd);
    } else {
      X = (int)cx * 32;
      Y = (int)cy * 32;
    }
    const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;    // |sx|, |sy| <= 2^26: sx + 1 cannot overflow
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int yy = sy + (k >> 1), xx = sx + (k & 1);
      const int w = ((k & 1) ? fx : 32 - fx) * ((k >> 1) ? fy : 32 - fy);
      if (w > 0 && yy >= 0 && yy < H && xx >= 0 && xx < W) {         // the guard of the reads
        wt[k] = w;
        src[k] = ((long long)b * H + ((f & 2) ? H - 1 - yy : yy)) * W + ((f & 1) ? W - 1 - xx : xx);   // un-flip, as ingest_kernel
      }
    }
  }
}

// row `t` of T 256-entry label tables, t clamped into [0, T): whatever a per-frame table index holds, the row read is one of the T given
__device__ __forceinline__ const uint8_t* label_table_row(const uint8_t* __restrict__ luts, int T, const int32_t* __restrict__ table_of_frame,
                                                          int b) {
  if (!luts || !table_of_frame) return luts;          // null index: row 0 for every frame
  int t = table_of_frame[b];
  t = t < 0 ? 0 : (t >= T ? T - 1 : t);
  return luts + (long long)t * 256;
}

// the label of a canvas pixel from its taps: remap (lut = the frame's table row, may be null) precedes the warp
__device__ __forceinline__ int warp_label(const uint8_t* __restrict__ lbl, const uint8_t* __restrict__ lut, const int (&wt)[4],
                                          const long long (&src)[4]) {
  int lab[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lab[k] = 0;
    if (wt[k] > 0) lab[k] = lut ? lut[lbl[src[k]]] : lbl[src[k]];
  }
  int best = 0, bestw = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (wt[j] > 0) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += (lab[k] == lab[j]) ? wt[k] : 0;   // (wt = 0 where nothing was read)
      if (s > bestw || (s == bestw && lab[j] < best)) { best = lab[j]; bestw = s; }
    }
  return best;
}
