// Frequency-weighted crop pick (reference: CropNP with crop_mode 'freq', utils/transforms.py:282-293): the window's corner is the index of a
// region pixel drawn with probability ~ 1 / (frequency of its class), random.choices = bisect of u * total in the running sum of the weights.
// Here the weights are integers (wq = w * 2^s, exact for float32 w), so the running sum does not depend on the order of its additions:
//   row pass   one block per (region row, frame): every lane evaluates the label of its canvas pixels with the warp's own gather and label
//              rule (csrc/warp_label.h), looks wq up in a 256-entry table staged in LDS and the block reduces in 64 bits -> rowsum[b][r];
//   pick pass  one block per frame: total = sum of the row sums, T = (m * total) >> 53 from the 128-bit product (m = floor(u 2^53)), a block
//              scan of the row sums finds the row whose inclusive sum first exceeds T, a block scan of that row's weights (labels evaluated
//              again: one row) finds the column.  The first i with cum_i > T is the one pixel with cum_{i-1} <= T < cum_i: exactly one lane
//              sees that, no reduction of candidates is needed.
// No atomics, no ordering between blocks, integer sums: two launches give the same bits.  Reads: the label bytes under the region once (+ one
// row per frame), through the guards of warp_taps; the tables by an 8-bit index.  8 B written per region row, 8 (+16) B per frame.
#include "common.h"
#include "catseg_cropfreq.h"
#include "catseg_ingest_tables.h"
#include "warp_label.h"

namespace {

typedef unsigned long long u64;

struct RegionArgs {
  const uint8_t* lbl; const uint8_t* luts; const int32_t* table_of_frame; const int32_t* flips; const double* minv;
  int T, H, W, Hc, Wc, margin, rh, rw;      // luts: [T][256]; table_of_frame: [B] or null = row 0 for every frame
};

// integer weight of region pixel (r, c) of frame b; tab: the 256 weights in LDS
__device__ __forceinline__ u64 pixel_weight(const RegionArgs& a, const u64* tab, int b, int f, int r, int c) {
  int wt[4];
  long long src[4];
  warp_taps(a.minv ? a.minv + (long long)b * 6 : nullptr, b, f, (long long)a.margin + r, (long long)a.margin + c, a.H, a.W, a.Hc, a.Wc, wt, src);
  return tab[warp_label(a.lbl, label_table_row(a.luts, a.T, a.table_of_frame, b), wt, src) & 255];   // (the index is clamped into [0, T))
}

// inclusive scan of v over the 256 threads of the block (thread order), *block_total = the sum; sm: 4 words of LDS, free again on return
__device__ __forceinline__ u64 block_scan(u64 v, u64* sm, u64* block_total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) sm[wave] = v;
  __syncthreads();
  u64 before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const u64 s = sm[w];
    if (w < wave) before += s;
    all += s;
  }
  __syncthreads();
  *block_total = all;
  return v + before;
}

__global__ __launch_bounds__(256) void crop_freq_rows_kernel(RegionArgs a, const u64* __restrict__ wq, u64* __restrict__ rowsum) {
  __shared__ u64 tab[256];
  __shared__ u64 sm[4];
  const int r = blockIdx.x, b = blockIdx.y;
  tab[threadIdx.x] = wq[threadIdx.x];
  __syncthreads();
  const int f = a.flips ? a.flips[b] : 0;
  u64 s = 0;
  for (int c = threadIdx.x; c < a.rw; c += 256) s += pixel_weight(a, tab, b, f, r, c);   // a wave's pixels gather neighbouring source pixels
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) rowsum[(long long)b * a.rh + r] = sm[0] + sm[1] + sm[2] + sm[3];
}

__global__ __launch_bounds__(256) void crop_freq_pick_kernel(RegionArgs a, const u64* __restrict__ wq, const u64* __restrict__ m53,
                                                             const u64* __restrict__ rowsum, int32_t* __restrict__ origin,
                                                             u64* __restrict__ total, int64_t* __restrict__ flat) {
  __shared__ u64 tab[256];
  __shared__ u64 sm[4];
  __shared__ u64 row_before;
  __shared__ int row_sel, col_sel;
  const int b = blockIdx.x, tid = threadIdx.x;
  tab[tid] = wq[tid];
  if (tid == 0) { row_sel = -1; col_sel = -1; row_before = 0; }
  const u64* rs = rowsum + (long long)b * a.rh;
  u64 part = 0;
  for (int r = tid; r < a.rh; r += 256) part += rs[r];
  u64 tot;
  block_scan(part, sm, &tot);                        // (its barriers also publish tab and the selections' initial values)
  const u64 m = m53[b];
  const u64 hi = __umul64hi(m, tot), lo = m * tot;   // m < 2^53, tot < 2^62: hi < 2^51, T < tot.  An m of 2^53 or more: no pixel exceeds T -> the cap
  const u64 T = ((m >> 53) || (hi >> 53)) ? ~0ULL : ((hi << 11) | (lo >> 53));
  u64 carry = 0;
  for (int base = 0; base < a.rh; base += 256) {     // (uniform bounds: every thread reaches the barriers of block_scan)
    const int r = base + tid;
    const u64 v = r < a.rh ? rs[r] : 0;
    u64 chunk;
    const u64 p = carry + block_scan(v, sm, &chunk);
    if (r < a.rh && p > T && p - v <= T) { row_sel = r; row_before = p - v; }   // one row at most: the sums do not decrease
    carry += chunk;
  }
  __syncthreads();
  int R = row_sel, Cc = a.rw - 1;
  if (R < 0) {
    R = a.rh - 1;                                    // random.choices' hi = n - 1: nothing exceeds T (total = 0), the last pixel
  } else {
    const u64 Tc = T - row_before;                   // < the row's sum
    const int f = a.flips ? a.flips[b] : 0;
    carry = 0;
    for (int base = 0; base < a.rw; base += 256) {
      const int c = base + tid;
      const u64 v = c < a.rw ? pixel_weight(a, tab, b, f, R, c) : 0;
      u64 chunk;
      const u64 p = carry + block_scan(v, sm, &chunk);
      if (c < a.rw && p > Tc && p - v <= Tc) col_sel = c;
      carry += chunk;
    }
    __syncthreads();
    if (col_sel >= 0) Cc = col_sel;
  }
  if (tid == 0) {
    origin[2 * b] = R;
    origin[2 * b + 1] = Cc;
    if (total) total[b] = tot;
    if (flat) flat[b] = (int64_t)R * a.rw + Cc;
  }
}

// margin, region rows and columns of a px window on an Hc x Wc canvas (the reference slices the columns with the height: [margin, Hc - margin),
// clipped at Wc by numpy)
bool region_of(int Hc, int Wc, int px, int* margin, int* rh, int* rw) {
  if (Hc <= 0 || Wc <= 0 || px < 1 || px > Hc || px > Wc) return false;
  *margin = px / 2;
  *rh = Hc - 2 * *margin;
  *rw = (Hc - *margin < Wc ? Hc - *margin : Wc) - *margin;
  return true;
}

#define PICK_REQUIRE(cond, msg) CS_REQUIRE(cond, "catseg_crop_freq_pick: " msg)

// the two launches behind both entry points
int pick_launch(const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T, const int32_t* table_of_frame, const int32_t* flips,
                const double* minv, int Hc, int Wc, int px, const uint64_t* wq, const uint64_t* m53, int32_t* origin, uint64_t* total,
                int64_t* flat, void* workspace, size_t workspace_bytes, catseg_stream_t stream) {
  PICK_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && Hc > 0 && Wc > 0, "bad dims");
  PICK_REQUIRE(H <= 16384 && W <= 16384 && Hc <= 16384 && Wc <= 16384, "frame and canvas are limited to 16384 x 16384");
  int margin = 0, rh = 0, rw = 0;
  PICK_REQUIRE(region_of(Hc, Wc, px, &margin, &rh, &rw), "px outside the canvas (1 <= px <= min(Hc, Wc))");
  PICK_REQUIRE(rh > 0 && rw > 0, "empty region: the window is as tall as the canvas, nothing is left to pick from");
  PICK_REQUIRE(lbl != nullptr, "the label map is NULL");
  PICK_REQUIRE(wq != nullptr, "the weight table is NULL");
  PICK_REQUIRE(m53 != nullptr && origin != nullptr, "m53 and origin are required");
  PICK_REQUIRE(minv != nullptr || (Hc == H && Wc == W), "without a matrix the canvas is the frame");
  PICK_REQUIRE(((((uintptr_t)minv) | ((uintptr_t)wq) | ((uintptr_t)m53) | ((uintptr_t)total) | ((uintptr_t)flat)) & 7) == 0 &&
                   (((uintptr_t)origin) & 3) == 0, "alignment (8 bytes: minv, wq, m53, total, flat; 4: origin)");
  const size_t need = (size_t)B * (size_t)rh * sizeof(u64);
  if (workspace == nullptr || (((uintptr_t)workspace) & 7) != 0 || workspace_bytes < need) {
    catseg_set_error("catseg_crop_freq_pick: workspace too small (%zu bytes, 8-byte aligned, needed; %zu given)", need,
                     workspace ? workspace_bytes : (size_t)0);
    return CATSEG_EWORKSPACE;
  }
  RegionArgs a{lbl, luts, table_of_frame, flips, minv, T, H, W, Hc, Wc, margin, rh, rw};
  u64* rowsum = (u64*)workspace;
  hipLaunchKernelGGL(crop_freq_rows_kernel, dim3((unsigned)rh, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a, (const u64*)wq, rowsum);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(crop_freq_pick_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a, (const u64*)wq, (const u64*)m53,
                     (const u64*)rowsum, origin, (u64*)total, flat);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

}  // namespace

extern "C" size_t catseg_crop_freq_workspace(int B, int Hc, int Wc, int px) {
  int margin, rh, rw;
  if (B <= 0 || !region_of(Hc, Wc, px, &margin, &rh, &rw) || rh <= 0 || rw <= 0) return 0;
  return (size_t)B * (size_t)rh * sizeof(u64);
}

extern "C" int catseg_crop_freq_pick(const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, const int32_t* flips, const double* minv, int Hc,
                                     int Wc, int px, const uint64_t* wq, const uint64_t* m53, int32_t* origin, uint64_t* total, int64_t* flat,
                                     void* workspace, size_t workspace_bytes, catseg_stream_t stream) {
  return pick_launch(lbl, B, H, W, lut, 1, nullptr, flips, minv, Hc, Wc, px, wq, m53, origin, total, flat, workspace, workspace_bytes, stream);
}

extern "C" int catseg_crop_freq_pick_tables(const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T, const int32_t* table_of_frame,
                                            const int32_t* flips, const double* minv, int Hc, int Wc, int px, const uint64_t* wq,
                                            const uint64_t* m53, int32_t* origin, uint64_t* total, int64_t* flat, void* workspace,
                                            size_t workspace_bytes, catseg_stream_t stream) {
  PICK_REQUIRE(T >= 1 && (luts != nullptr || table_of_frame == nullptr), "a table index needs T >= 1 tables");
  PICK_REQUIRE((((uintptr_t)table_of_frame) & 3) == 0, "the table index must be 4-byte aligned");
  return pick_launch(lbl, B, H, W, luts, T, table_of_frame, flips, minv, Hc, Wc, px, wq, m53, origin, total, flat, workspace, workspace_bytes,
                     stream);
}
