// Streaming kernels of the BatchNorm-free conv + bias + ReLU networks (models/UNet.py of the reference: double_conv, MaxPool2d(2), 2x bilinear
// Upsample(align_corners=True), torch.cat([up, skip], 1)).  The split-precision direct / pointwise / gather convolution kernels take a layer
// only when its input (backward: its output gradient) carries an amax record, and without BatchNorm none of the record producers
// (bn_apply, add_n_act, bn_backward) runs.  These kernels leave the records in the passes the skip junction needs anyway:
//   amax_record        read-only max|x| of a tensor that no other pass touches (the first convolution's output of a double_conv)
//   maxpool2x2_fwd_rec the 2x2 max-pool of csrc/pool.hip + the record of its input and of its output
//   upcat2x_fwd        cat = [resize2x(x), skip] in one launch + the record of everything written
//   relu_bwd_rec       g = dz * (z > 0) + the record of g; junction form: dz = a channel slice of the concatenation's gradient + the pooled
//                      gradient routed through the pool's argmax bytes (no temporary, no accumulating pass)
// All NHWC fp32, C % 4 == 0, 16-byte accesses, grid-strided; a record is filled as add_n_act_kernel fills its own (common.h: block
// reduction of the |v| bits, one atomicMax per block into a slot) from the very values that were written, so it bounds them exactly.
#include "lerp.h"

namespace {

constexpr long long UN_MAX_BLOCKS = 8192;      // 32 blocks of 256 threads per CU: the kernels stride over the rest

__device__ __forceinline__ f32x4 un_ld4(const float* p) { return *(const f32x4*)p; }

__global__ __launch_bounds__(256) void amax_record_kernel(const float* __restrict__ x, int ld, long long rows, int C, unsigned* __restrict__ rec) {
  const int cpt = C >> 2;
  unsigned m = 0;
  CS_QUAD_LOOP(rows, cpt, r, c) m = max(m, cs_abs_bits4(un_ld4(x + r * ld + c)));
  cs_amax_commit(m, rec);
}

// maxpool2_fwd_kernel (csrc/pool.hip: same scan order, same `v > best || isnan(v)` rule, same idx bytes).  Every input element is read by
// exactly one thread: the thread of the last window of a row / column also reads the odd row / column that max_pool2d's floor leaves out,
// for the input's record alone.
__global__ __launch_bounds__(256) void maxpool2_fwd_rec_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy,
                                                               unsigned char* __restrict__ idx, int B, int H, int W, int C, int Ho, int Wo,
                                                               unsigned* __restrict__ xrec, unsigned* __restrict__ yrec) {
  const int cpt = C >> 2;
  const long long total = (long long)B * Ho * Wo * cpt;
  unsigned mx = 0, my = 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long p = t / cpt;
    const int c = (int)(t - p * cpt) * 4;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho), b = (int)(p / ((long long)Wo * Ho));
    const int ny = 2 + (((H & 1) && oy == Ho - 1) ? 1 : 0), nx = 2 + (((W & 1) && ox == Wo - 1) ? 1 : 0);
    f32x4 best = {0.f, 0.f, 0.f, 0.f};
    unsigned char bi[4] = {0, 0, 0, 0};
    for (int iy = 0; iy < ny; ++iy)
      for (int ix = 0; ix < nx; ++ix) {
        const f32x4 v = un_ld4(x + (((long long)b * H + 2 * oy + iy) * W + 2 * ox + ix) * ldx + c);
        mx = max(mx, cs_abs_bits4(v));
        if (iy > 1 || ix > 1) continue;
        const int k = (iy << 1) | ix;
        if (k == 0) { best = v; continue; }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (v[j] > best[j] || v[j] != v[j]) { best[j] = v[j]; bi[j] = (unsigned char)k; }
      }
    *(f32x4*)(y + p * ldy + c) = best;
    *(uchar4*)(idx + p * C + c) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
    my = max(my, cs_abs_bits4(best));
  }
  if (xrec) cs_amax_commit(mx, xrec);
  if (yrec) {
    __syncthreads();      // (cs_amax_commit's staging words are shared by both reductions)
    cs_amax_commit(my, yrec);
  }
}

// cat[b, oy, ox, 0 .. Cx) = bilinear_fwd_kernel<2>'s expression on x (align_corners, Ho = 2 h, Wo = 2 w); cat[b, oy, ox, Cx .. Cx + Cs) = skip.
// A block walks whole output rows (the row's two taps and weights once per row).
__global__ __launch_bounds__(256) void upcat2x_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ skip, int lds,
                                                          float* __restrict__ cat, int ldc, int B, int H, int W, int Cx, int Cs, float sh, float sw,
                                                          unsigned* __restrict__ rec) {
  const int Ho = 2 * H, Wo = 2 * W, qx = Cx >> 2, q = (Cx + Cs) >> 2, n = Wo * q;
  unsigned m = 0;
  for (long long row = blockIdx.x; row < (long long)B * Ho; row += gridDim.x) {
    const int b = (int)(row / Ho), oy = (int)(row - (long long)b * Ho);
    int y0, y1;
    float ly0, ly1;
    lerp_setup(sh, oy, true, H, y0, y1, ly0, ly1);
    const float* r0 = x + ((long long)b * H + y0) * W * ldx;
    const float* r1 = x + ((long long)b * H + y1) * W * ldx;
    const float* s = skip + row * Wo * lds;
    float* o = cat + row * Wo * ldc;
    for (int u = threadIdx.x; u < n; u += blockDim.x) {
      const int ox = u / q, j = u - ox * q;
      f32x4 v;
      if (j < qx) {
        const int c = j * 4;
        int x0, x1;
        float lx0, lx1;
        lerp_setup(sw, ox, true, W, x0, x1, lx0, lx1);
        const f32x4 a0 = un_ld4(r0 + x0 * ldx + c), a1 = un_ld4(r0 + x1 * ldx + c), b0 = un_ld4(r1 + x0 * ldx + c), b1 = un_ld4(r1 + x1 * ldx + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ly0 * (lx0 * a0[e] + lx1 * a1[e]) + ly1 * (lx0 * b0[e] + lx1 * b1[e]);
      } else {
        v = un_ld4(s + (long long)ox * lds + (j - qx) * 4);
      }
      *(f32x4*)(o + (long long)ox * ldc + j * 4) = v;
      m = max(m, cs_abs_bits4(v));
    }
  }
  if (rec) cs_amax_commit(m, rec);
}

// g = dz * (z > 0): relu_bwd_kernel (csrc/pointwise.hip) + the record of g
__global__ __launch_bounds__(256) void relu_bwd_rec_kernel(const float* __restrict__ dz, int lddz, const float* __restrict__ z, int ldz,
                                                           float* __restrict__ g, int ldg, long long rows, int C, unsigned* __restrict__ rec) {
  const int cpt = C >> 2;
  unsigned m = 0;
  CS_QUAD_LOOP(rows, cpt, r, c) {
    f32x4 d = un_ld4(dz + r * lddz + c);
    const f32x4 zz = un_ld4(z + r * ldz + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = zz[k] > 0.f ? d[k] : 0.f;
    *(f32x4*)(g + r * ldg + c) = d;
    m = max(m, cs_abs_bits4(d));
  }
  if (rec) cs_amax_commit(m, rec);
}

// junction: dz = dcat slice + maxpool2_bwd_kernel's routing of dpool (csrc/pool.hip: the pooled gradient goes to the window position idx names,
// 0 everywhere else and outside the pooled area), one fp32 addition per element
__global__ __launch_bounds__(256) void relu_bwd_junction_kernel(const float* __restrict__ dcat, int lddc, const float* __restrict__ dpool, int lddp,
                                                                const unsigned char* __restrict__ idx, const float* __restrict__ z, int ldz,
                                                                float* __restrict__ g, int ldg, int B, int H, int W, int C, int Ho, int Wo,
                                                                unsigned* __restrict__ rec) {
  const int cpt = C >> 2;
  const long long total = (long long)B * H * W * cpt;
  unsigned m = 0;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long p = t / cpt;
    const int c = (int)(t - p * cpt) * 4;
    const int xx = (int)(p % W), yy = (int)((p / W) % H), b = (int)(p / ((long long)W * H));
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    const int oy = yy >> 1, ox = xx >> 1;
    if (oy < Ho && ox < Wo) {
      const long long qq = ((long long)b * Ho + oy) * Wo + ox;
      const f32x4 d = un_ld4(dpool + qq * lddp + c);
      const uchar4 i4 = *(const uchar4*)(idx + qq * C + c);
      const int k = ((yy & 1) << 1) | (xx & 1);
      r[0] = i4.x == k ? d[0] : 0.f; r[1] = i4.y == k ? d[1] : 0.f; r[2] = i4.z == k ? d[2] : 0.f; r[3] = i4.w == k ? d[3] : 0.f;
    }
    f32x4 d = un_ld4(dcat + p * lddc + c) + r;
    const f32x4 zz = un_ld4(z + p * ldz + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = zz[k] > 0.f ? d[k] : 0.f;
    *(f32x4*)(g + p * ldg + c) = d;
    m = max(m, cs_abs_bits4(d));
  }
  if (rec) cs_amax_commit(m, rec);
}

inline bool un_row_ok(const void* p, int ld, int C) { return p && ld >= C && ld % 4 == 0 && cs_aligned16(p); }

}  // namespace

extern "C" int catseg_amax_record(const float* x, int ld, long long rows, int C, void* record, catseg_stream_t stream) {
  CS_REQUIRE(rows > 0 && C > 0 && C % 4 == 0 && un_row_ok(x, ld, C) && record, "amax_record: bad args (C and ld multiples of 4, x 16-byte aligned, a record)");
  hipLaunchKernelGGL(amax_record_kernel, dim3(cs_grid_256(rows * (C / 4), UN_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, ld, rows, C,
                     (unsigned*)record);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_maxpool2x2_fwd_rec(const float* x, int ldx, float* y, int ldy, uint8_t* idx, int B, int H, int W, int C, void* x_record,
                                         void* y_record, catseg_stream_t stream) {
  const int Ho = H / 2, Wo = W / 2;
  CS_REQUIRE(B > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && un_row_ok(x, ldx, C) && un_row_ok(y, ldy, C) && idx,
             "maxpool2x2 fwd rec: bad args (C and ld multiples of 4, 16-byte aligned tensors)");
  hipLaunchKernelGGL(maxpool2_fwd_rec_kernel, dim3(cs_grid_256((long long)B * Ho * Wo * (C / 4), UN_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream,
                     x, ldx, y, ldy, idx, B, H, W, C, Ho, Wo, (unsigned*)x_record, (unsigned*)y_record);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_upcat2x_fwd(const float* x, int ldx, const float* skip, int lds, float* cat, int ldc, int B, int h, int w, int Cx, int Cs,
                                  void* record, catseg_stream_t stream) {
  CS_REQUIRE(B > 0 && h > 0 && w > 0 && Cx > 0 && Cs > 0 && Cx % 4 == 0 && Cs % 4 == 0 && un_row_ok(x, ldx, Cx) && un_row_ok(skip, lds, Cs) &&
                 un_row_ok(cat, ldc, Cx + Cs) && (long long)2 * w * ((Cx + Cs) / 4) < (1ll << 31),
             "upcat2x fwd: bad args (Cx, Cs and ld multiples of 4, 16-byte aligned tensors)");
  const long long rows = (long long)B * 2 * h;
  hipLaunchKernelGGL(upcat2x_fwd_kernel, dim3((unsigned)(rows < UN_MAX_BLOCKS ? rows : UN_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, ldx, skip,
                     lds, cat, ldc, B, h, w, Cx, Cs, resize_scale(h, 2 * h, true), resize_scale(w, 2 * w, true), (unsigned*)record);
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}

extern "C" int catseg_relu_bwd_rec(const float* dz, int lddz, const float* dpool, int lddp, const uint8_t* idx, const float* z, int ldz, float* g,
                                   int ldg, int B, int H, int W, int C, void* record, catseg_stream_t stream) {
  CS_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && un_row_ok(dz, lddz, C) && un_row_ok(z, ldz, C) && un_row_ok(g, ldg, C),
             "relu_bwd rec: bad args (C and ld multiples of 4, 16-byte aligned tensors)");
  CS_REQUIRE((dpool == nullptr) == (idx == nullptr), "relu_bwd rec: the junction form takes dpool and idx together");
  const long long rows = (long long)B * H * W;
  const unsigned grid = cs_grid_256(rows * (C / 4), UN_MAX_BLOCKS);
  if (dpool) {
    CS_REQUIRE(H / 2 > 0 && W / 2 > 0 && un_row_ok(dpool, lddp, C), "relu_bwd rec: bad dpool (ld a multiple of 4, 16-byte aligned, a pooled map)");
    hipLaunchKernelGGL(relu_bwd_junction_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dz, lddz, dpool, lddp, idx, z, ldz, g, ldg, B, H, W, C,
                       H / 2, W / 2, (unsigned*)record);
  } else {
    hipLaunchKernelGGL(relu_bwd_rec_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dz, lddz, z, ldz, g, ldg, rows, C, (unsigned*)record);
  }
  CS_LAUNCH_CHECK();
  return CATSEG_OK;
}
