// Network output -> label maps and coloured uint8 frames, the last stage of video inference (reference: managers/BaseManager.py:690-741 --
// argmax(Softmax2d(out)), mask_to_colormap(from_network=True), np.round(frame * 255), np.concatenate; utils/utils.py:50-142,202-211;
// utils/torch_utils.py:7-21 clipped_argmax) as ONE streaming launch over the NHWC logits: the reference's sequence is a softmax, an argmax,
// a where, a loop over the colour table on the host, a concatenation and a rounding pass.
//   catseg_egress_u8: per pixel the FIRST maximal class (optionally clipped to an ignore id by its softmax score), then any of
//                     labels int64, labels uint8 (through the network id -> dataset id table) and a canvas of up to three panels
//                     frame | target | prediction, 3 bytes per pixel (rows = NULL: no prediction, the other panels alone).
// A block takes 256 consecutive output pixels of ONE image (the cropped rows lie between the images: they are never read).  Rows of ld <= 68
// floats go through LDS (rows.h: 16-byte global loads, odd LDS row stride); lane t picks the class of pixel t and leaves its id in LDS.
// The byte outputs are then written by lanes that own FOUR consecutive pixels of one output row each: 12 canvas bytes = three dwords,
// 4 label bytes = one dword; wave w of the block writes panel w.  Where W is not a multiple of 4 (canvas rows are n_panels * W * 3 bytes:
// unaligned rows, groups that straddle a panel edge) a lane owns one pixel and writes bytes.
#include "rows.h"

namespace {

constexpr int PIX = 256;          // pixels per block
constexpr int MAXK = 64;
constexpr int MAXLD = MAXK + 4;   // widest row (floats) staged through LDS; wider rows (views into a concat buffer) are read per lane

enum { OUT_FRAME = 0, OUT_TARGET = 1, OUT_PRED = 2, OUT_LABELS = 3 };

struct EgressArgs {
  const float* rows;
  int ld, LS, K, probs;
  int H, W, Ho, crop_top;
  float threshold;
  int ignore_value;
  const uint8_t* lut;
  const uint8_t* palette;
  const float* frame;
  int nhwc4, norm, bgr;
  float mean[3], stdv[3];
  const int64_t* target;
  int64_t* labels_i64;
  uint8_t* labels_u8;
  uint8_t* canvas;
  int n_panels;       // panels of the canvas
  int n_outs;         // byte outputs of the launch: the panels + labels_u8
  unsigned kinds;     // 4 bits per byte output: OUT_*; for a panel its index on the canvas is its position in this list
  int vec;            // W % 4 == 0 and every byte pointer aligned: the dword path
};

// the FIRST maximal value of the row (torch.argmax; the rule of catseg_confusion_matrix and catseg_ensemble_merge); with need_score the
// value clipped_argmax compares with its threshold: the maximum itself for probabilities, 1 / sum_k exp(x_k - max) for logits
// (= the maximal entry of nn.Softmax2d: exp(0) / sum)
__device__ __forceinline__ int pick_class(const float* row, int K, bool need_score, bool probs, float& score) {
  int best = 0;
  float bv = row[0];
#pragma unroll 4
  for (int c = 1; c < K; ++c) {
    const float v = row[c];
    if (v > bv) {
      bv = v;
      best = c;
    }
  }
  score = bv;
  if (need_score && !probs) {
    float s = 0.f;
#pragma unroll 4
    for (int c = 0; c < K; ++c) s += expf(row[c] - bv);
    score = __fdiv_rn(1.f, s);
  }
  return best;
}

// np.round(x * 255).astype(uint8) (ties to even), clamped; un_normalise (utils/utils.py:453) first: a rounded multiply, then a rounded
// add -- a contraction to one FMA would move the .5 cases
__device__ __forceinline__ unsigned frame_byte(float x, int norm, float sd, float mn) {
  if (norm) x = __fadd_rn(__fmul_rn(x, sd), mn);
  const float v = fminf(fmaxf(rintf(__fmul_rn(x, 255.f)), 0.f), 255.f);
  return (unsigned)(int)v;
}

__device__ __forceinline__ float sel3(int c, float v0, float v1, float v2) { return c == 0 ? v0 : c == 1 ? v1 : v2; }   // (no indexed kernel argument)

// network id -> the palette entry of its dataset id; ids outside the tables are left black (mask_to_colormap leaves unmapped ids 0)
__device__ __forceinline__ void id_colour(long long id, const uint8_t* s_lut, const uint8_t* s_pal, unsigned (&c)[3]) {
  if (id < 0 || id > 255) {
    c[0] = c[1] = c[2] = 0;
    return;
  }
  const int d = s_lut[id] * 3;
  c[0] = s_pal[d];
  c[1] = s_pal[d + 1];
  c[2] = s_pal[d + 2];
}

__global__ __launch_bounds__(PIX) void egress_kernel(EgressArgs a) {
  extern __shared__ float sh[];
  int* ids = reinterpret_cast<int*>(sh + PIX * a.LS);
  uint8_t* s_lut = reinterpret_cast<uint8_t*>(ids + PIX);
  uint8_t* s_pal = s_lut + 256;
  const int t = threadIdx.x;
  const long long b = blockIdx.y;
  const int HWo = a.Ho * a.W, HWi = a.H * a.W;
  const int q0 = blockIdx.x * PIX;                                   // first output pixel of the block, within its image
  const int np = min(PIX, HWo - q0);
  const int pin0 = a.crop_top * a.W + q0;                            // the same pixel within the uncropped image
  const long long p0 = b * HWi + pin0;

  s_lut[t] = a.lut ? a.lut[t] : (uint8_t)t;
  if (a.palette)
    for (int i = t; i < 768; i += PIX) s_pal[i] = a.palette[i];
  const bool staged = a.rows && a.ld <= MAXLD;
  if (staged) stage_rows(a.rows, p0, np, a.ld, a.LS, sh);           // whole rows, pad columns included; never a cropped row
  __syncthreads();

  if (a.rows && t < np) {
    const bool need_score = a.threshold > 0.f;
    float score;
    int id = staged ? pick_class(sh + t * a.LS, a.K, need_score, a.probs, score)      // (two call sites: ds_read here, global loads there)
                    : pick_class(a.rows + (p0 + t) * (long long)a.ld, a.K, need_score, a.probs, score);
    if (need_score && score < a.threshold) id = a.ignore_value;
    ids[t] = id;
    if (a.labels_i64) a.labels_i64[b * HWo + q0 + t] = (int64_t)id;
  }
  if (a.n_outs == 0) return;
  __syncthreads();

  if (a.vec) {
    // item = (byte output, group of four pixels): np is a multiple of 4 here, and with q0 and W multiples of 4 a group lies in one row
    const int ngroups = np >> 2;
    for (int item = t; item < a.n_outs * 64; item += PIX) {
      const int slot = item >> 6, g = item & 63;
      if (g >= ngroups) continue;
      const int kind = (a.kinds >> (4 * slot)) & 15;
      const int q = q0 + 4 * g;
      if (kind == OUT_LABELS) {
        unsigned w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) w |= (unsigned)s_lut[ids[4 * g + i] & 255] << (8 * i);
        *reinterpret_cast<unsigned*>(a.labels_u8 + b * HWo + q) = w;
        continue;
      }
      unsigned px[4][3];
      if (kind == OUT_FRAME) {
        if (a.nhwc4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float4 v = *reinterpret_cast<const float4*>(a.frame + (p0 + 4 * g + i) * 4);
            const float e[3] = {v.x, v.y, v.z};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              const int c = a.bgr ? 2 - j : j;
              px[i][j] = frame_byte(sel3(c, e[0], e[1], e[2]), a.norm, sel3(c, a.stdv[0], a.stdv[1], a.stdv[2]), sel3(c, a.mean[0], a.mean[1], a.mean[2]));
            }
          }
        } else {
          float e[3][4];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float4 v = *reinterpret_cast<const float4*>(a.frame + (b * 3 + c) * HWi + pin0 + 4 * g);
            e[c][0] = v.x; e[c][1] = v.y; e[c][2] = v.z; e[c][3] = v.w;
          }
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int c = a.bgr ? 2 - j : j;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              px[i][j] = frame_byte(sel3(c, e[0][i], e[1][i], e[2][i]), a.norm, sel3(c, a.stdv[0], a.stdv[1], a.stdv[2]), sel3(c, a.mean[0], a.mean[1], a.mean[2]));
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          id_colour(kind == OUT_TARGET ? (long long)a.target[p0 + 4 * g + i] : (long long)ids[4 * g + i], s_lut, s_pal, px[i]);
      }
      const int y = q / a.W, x = q - y * a.W;
      unsigned* dst = reinterpret_cast<unsigned*>(a.canvas + (((b * a.Ho + y) * a.n_panels + slot) * a.W + x) * 3);
      dst[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
      dst[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
      dst[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
    }
  } else {
    // a lane owns one pixel of one byte output
    for (int item = t; item < a.n_outs * PIX; item += PIX) {
      const int slot = item >> 8, i = item & (PIX - 1);
      if (i >= np) continue;
      const int kind = (a.kinds >> (4 * slot)) & 15;
      const int q = q0 + i;
      if (kind == OUT_LABELS) {
        a.labels_u8[b * HWo + q] = s_lut[ids[i] & 255];
        continue;
      }
      unsigned px[3];
      if (kind == OUT_FRAME) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int c = a.bgr ? 2 - j : j;
          const float v = a.nhwc4 ? a.frame[(p0 + i) * 4 + c] : a.frame[(b * 3 + c) * HWi + pin0 + i];
          px[j] = frame_byte(v, a.norm, sel3(c, a.stdv[0], a.stdv[1], a.stdv[2]), sel3(c, a.mean[0], a.mean[1], a.mean[2]));
        }
      } else {
        id_colour(kind == OUT_TARGET ? (long long)a.target[p0 + i] : (long long)ids[i], s_lut, s_pal, px);
      }
      const int y = q / a.W, x = q - y * a.W;
      uint8_t* dst = a.canvas + (((b * a.Ho + y) * a.n_panels + slot) * a.W + x) * 3;
      dst[0] = (uint8_t)px[0];
      dst[1] = (uint8_t)px[1];
      dst[2] = (uint8_t)px[2];
    }
  }
}

}  // namespace

extern "C" int catseg_egress_u8(const float* rows, int ld, int B, int H, int W, int K, int values_are_probs, int crop_top, int crop_bottom,
                                float threshold, int ignore_value, const uint8_t* lut, const uint8_t* palette, const float* frame,
                                int frame_nhwc4, const float* mean, const float* stdv, int bgr, const int64_t* target,
                                int64_t* labels_i64, uint8_t* labels_u8, uint8_t* canvas, catseg_stream_t stream) {
  CS_REQUIRE(!rows || (K >= 1 && K <= MAXK), "egress: 1 <= K <= %d classes (got %d)", MAXK, K);
  CS_REQUIRE(!rows || ld >= K, "egress: ld %d < K = %d", ld, K);
  CS_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 29), "egress: bad batch / frame size");
  CS_REQUIRE(crop_top >= 0 && crop_bottom >= 0 && crop_top + crop_bottom < H, "egress: crop (%d, %d) leaves no row of %d", crop_top,
             crop_bottom, H);
  CS_REQUIRE(labels_i64 || labels_u8 || canvas, "egress: all outputs are NULL");
  CS_REQUIRE(!canvas || palette, "egress: a canvas needs a palette");
  CS_REQUIRE(threshold < 1.f, "egress: threshold %g must be below 1", (double)threshold);   // (a NaN fails this too)
  CS_REQUIRE(!(threshold > 0.f) || (ignore_value >= 0 && ignore_value <= 255), "egress: ignore_value %d outside [0, 255]", ignore_value);
  CS_REQUIRE(rows || (!labels_i64 && !labels_u8 && (frame || target)), "egress: without rows there is no prediction: only frame / target panels");
  CS_REQUIRE(canvas || (!frame && !target), "egress: frame / target panels need a canvas");
  CS_REQUIRE((mean == nullptr) == (stdv == nullptr) && (!mean || frame), "egress: mean and std come together, with a frame");
  EgressArgs a;
  a.rows = rows;
  a.ld = ld;
  a.LS = rows && ld <= MAXLD ? (ld | 1) : 1;
  a.K = K;
  a.probs = values_are_probs ? 1 : 0;
  a.H = H;
  a.W = W;
  a.Ho = H - crop_top - crop_bottom;
  a.crop_top = crop_top;
  a.threshold = threshold;
  a.ignore_value = ignore_value;
  a.lut = lut;
  a.palette = palette;
  a.frame = frame;
  a.nhwc4 = frame_nhwc4 ? 1 : 0;
  a.norm = mean ? 1 : 0;
  a.bgr = bgr ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = mean ? mean[c] : 0.f;
    a.stdv[c] = stdv ? stdv[c] : 1.f;
  }
  a.target = target;
  a.labels_i64 = labels_i64;
  a.labels_u8 = labels_u8;
  a.canvas = canvas;
  a.n_outs = 0;
  a.kinds = 0;
  if (canvas) {                                    // the panels that are present, in the fixed order frame | target | prediction
    if (frame) a.kinds |= (unsigned)OUT_FRAME << (4 * a.n_outs++);
    if (target) a.kinds |= (unsigned)OUT_TARGET << (4 * a.n_outs++);
    if (rows) a.kinds |= (unsigned)OUT_PRED << (4 * a.n_outs++);
  }
  a.n_panels = a.n_outs;
  if (labels_u8) a.kinds |= (unsigned)OUT_LABELS << (4 * a.n_outs++);
  const auto al = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; };
  a.vec = W % 4 == 0 && al(canvas, 4) && al(labels_u8, 4) && al(frame, 16);
  const size_t shb = (size_t)PIX * a.LS * 4 + PIX * 4 + 1024;
  CS_LDS_RESERVE(egress_kernel, shb, "egress");
  const unsigned blocks = (unsigned)(((long long)a.Ho * W + PIX - 1) / PIX);
  hipLaunchKernelGGL(egress_kernel, dim3(blocks, (unsigned)B), dim3(PIX), shb, (hipStream_t)stream, a);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
