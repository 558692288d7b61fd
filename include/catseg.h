/*
 * catseg.h — C ABI of libcatseg_hip.so: the MI355X (gfx950) hot path of the
 * cataract-segmentation trainer.
 *
 * The reference (RViMLab/MICCAI2021_Cataract_semantic_segmentation) is 100 % Python and
 * has no FFI: its hot path is the list of ATen ops dispatched from models/*.py and
 * losses/*.py.  Each entry point below replaces one such ATen call site (cited as
 * file:line relative to the reference tree).  The boundary is plain C: raw device
 * pointers, explicit sizes / strides, a hipStream_t passed as void*, int status.
 *
 * Conventions
 *  - activations are NHWC fp32: pixel p = (b*H + y)*W + x, element (p, c) at base[p*ld + c],
 *    ld >= C and ld % 4 == 0, base 16-byte aligned ("ld" lets a tensor live inside a
 *    wider concat buffer without a copy);
 *  - conv weights are OHWI fp32 (a torch [O,I,kh,kw] tensor in channels_last memory format);
 *  - every function is asynchronous on `stream`, never allocates, never synchronises;
 *  - return value: 0 = ok, otherwise a CATSEG_E* code; catseg_last_error() gives a message.
 */
#ifndef CATSEG_H
#define CATSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CATSEG_OK 0
#define CATSEG_EINVAL 1   /* bad argument (shape / alignment)  */
#define CATSEG_EHIP 2     /* a HIP runtime call failed          */
#define CATSEG_EWORKSPACE 3

typedef void* catseg_stream_t; /* hipStream_t */

const char* catseg_last_error(void);
int catseg_version(void);   /* 3: catseg_conv2d_* take a descriptor (2: catseg_bn_apply / catseg_bn_backward do, catseg_add_n_act takes its records) */

/* ---- convolution as implicit GEMM on v_mfma_f32_32x32x2_f32 ------------------------------
 * replaces F.conv2d behind nn.Conv2d at models/OCR.py:72-97,200-235,308-313 and
 * models/DeepLabv3Plus.py:92-105,145-156, models/HRNetv2.py:23-33 etc. and every
 * torchvision ResNet conv (models/OCR.py:58-61). */
typedef struct {
  int B, H, W, Cin;        /* input  NHWC dims                                   */
  int Ho, Wo, Cout;        /* output NHWC dims                                   */
  int kh, kw, stride, pad, dil;
  int ldx, ldy;            /* floats per pixel of x / y buffers                  */
  int stem4;               /* 1: 7x7/2 stem on a 4-channel-padded image, weights packed [O][kh][8][4] */
  int groups;              /* 0 or 1 = dense; g > 1 = grouped (forward only: ResNeXt inference, models/ResNeXt.py:46-60);
                              weights [Cout][kh][kw][Cin/g], Cin/g a multiple of 4 */
} catseg_conv_desc;

/* ---- the four convolution entry points: one per direction + the backward-weight workspace query.  `operands` says how BOTH GEMM operands
 * of a call are stored; the descriptors are flat, a field left NULL / 0 is "not used".
 *
 *  CATSEG_OPERANDS_  activation (x / dy) and weight operand                                         directions and extras accepted
 *  F32               NHWC fp32 activations; OHWI fp32 weights (forward and backward-data read the   all three; groups, stem4, any stride, residual / relu,
 *                    same tensor)                                                                   dbias
 *  BF16X3            catseg_split3 [3][rows][roundup(C, 8)]; weights: catseg_split3 of the          all three; Cin % 8 == 0; no residual / relu
 *                    [Cout][kh kw Cin] view (forward), catseg_split3_weight_t (backward-data)
 *  BF16X3_BLOCKED    catseg_split3_blocked [3][ceil(C/16)][rows][16]; catseg_split3_weight_blocked  forward (Cin % 16 == 0; residual / relu), backward-data
 *                    (forward), catseg_split3_weight_t_blocked (backward-data)
 *  F16X2             catseg_split2h planar [2][rows][roundup(C, 8)] + both 8-byte scale records     backward-weight; Cin % 8 == 0
 *  F16X2_BLOCKED     catseg_split2h blocked [2][ceil(C/16)][rows][16] + both scale records;         all three (forward: Cin % 16 == 0, residual / relu;
 *                    catseg_split2h_weight_blocked (forward), _weight_t_blocked (backward-data)     backward-weight: Cin % 8 == 0)
 *
 *  geo.ldx / geo.ldy.  F32: floats per pixel of the x (dx) and y (dy) buffers.  Plane operands: a plane has its own pitch (above), so only
 *  the fp32 side of a call is a row stride -- forward: ldx = Cin, ldy = row stride of y; backward-data: ldx = row stride of dx,
 *  ldy = roundup(Cout, 8); backward-weight: ldx = Cin, ldy = roundup(Cout, 8).
 *
 *  Plane operands: dense only (groups <= 1, no stem4); at most 32 taps in forward / backward-data; backward-data for stride 1 only; planes
 *  16-byte aligned; no dbias (catseg_bias_grad computes it); a scale record per operand with f16x2, none with any other form.  residual /
 *  relu (the inference epilogue) exclude zero_to and bn_part.  Anything else returns CATSEG_EINVAL before any launch, with a message that
 *  starts with the function's name. */
#define CATSEG_OPERANDS_F32 0
#define CATSEG_OPERANDS_BF16X3 1
#define CATSEG_OPERANDS_BF16X3_BLOCKED 2
#define CATSEG_OPERANDS_F16X2 3
#define CATSEG_OPERANDS_F16X2_BLOCKED 4
/* y[p, o] = act(sum_{ky,kx,c} x[pix(p,ky,kx), c] * w[o,ky,kx,c] (+ bias[o]) (+ residual[p, o])), act = relu if relu != 0; columns
 * [Cout, zero_to) of y are written as zeros (zero_to <= ldy, 0 = none).
 * bn_part != NULL: the training forward of conv -> BatchNorm (models/OCR.py:72-76 etc.): the epilogue also writes per-(M-tile, channel)
 * BatchNorm partials [n_tiles][3][Cout] (K, s1, s2) for catseg_bn_finalize -- no separate statistics pass over y.  tile_rows / n_tiles are
 * then required and always written; *tile_rows == 0: this layer's tile form has no fused statistics (or bn_part_floats is too small for
 * them), use catseg_bn_train_stats.
 * residual / relu: inference, with catseg_fold_bn this is Conv2d + eval-mode BatchNorm2d + residual add + ReLU of a ResNet / UPerNet block
 * in one kernel. */
typedef struct {
  catseg_conv_desc geo; int operands;
  const void* x; const void* x_scale;
  const void* w; const void* w_scale;
  const float* bias;
  float* y; int zero_to;
  float* bn_part; size_t bn_part_floats; int* tile_rows; int* n_tiles;
  const float* residual; int ldr; int relu;
} catseg_conv_fwd_desc;
int catseg_conv2d_fwd(const catseg_conv_fwd_desc* d, catseg_stream_t stream);
/* dx[q, c] (+)= sum_{ky,kx,o} dy[opix(q,ky,kx), o] * w[o,ky,kx,c]  (autograd of the above; w: see the table) */
typedef struct {
  catseg_conv_desc geo; int operands;
  const void* dy; const void* dy_scale;
  const void* w; const void* w_scale;
  float* dx; int accumulate;
} catseg_conv_bwd_data_desc;
int catseg_conv2d_bwd_data(const catseg_conv_bwd_data_desc* d, catseg_stream_t stream);
/* dw[o,ky,kx,c] = sum_p dy[p, o] * x[pix(p,ky,kx), c]; dbias[o] = sum_p dy[p,o] (may be NULL).
 * workspace: catseg_conv2d_bwd_weight_workspace() bytes (split-reduction slabs); too small: CATSEG_EWORKSPACE. */
typedef struct {
  catseg_conv_desc geo; int operands;
  const void* x; const void* x_scale;
  const void* dy; const void* dy_scale;
  float* dw; float* dbias;
  void* workspace; size_t workspace_bytes;
} catseg_conv_bwd_weight_desc;
size_t catseg_conv2d_bwd_weight_workspace(const catseg_conv_desc* geo, int operands);
int catseg_conv2d_bwd_weight(const catseg_conv_bwd_weight_desc* d, catseg_stream_t stream);
/* Operand contract of the F32 convolutions: catseg_conv2d_fwd / _bwd_data / _bwd_weight with
 * CATSEG_OPERANDS_F32.  r4(n) = n rounded up to 4; a "pixel" is a row of ldx / ldy floats.
 * tests/test_conv_exact_gpu.py holds the kernels, on every tile form, to the sentences about what
 * is read, what is written and what keeps its bits; the preconditions of the first paragraph
 * (checked on the host before a launch) and the state of the workspace are not part of that test.
 *
 * All directions.  x / dx, y / dy, w / dw 16-byte aligned; ldx, ldy multiples of 4, ldx >= Cin,
 *   ldy >= Cout; Cin (grouped: Cin / groups) a multiple of 4; every tensor below 2^31 floats.
 *   Anything else returns CATSEG_EINVAL before a launch.
 *   The tensors may be channel slices of wider buffers (concatenation views): of the B H W pixels
 *   of x / dx and the B Ho Wo pixels of y / dy only the columns named below are touched; no float
 *   in front of the first pixel, behind the last, in front of or behind w, dw, bias or dbias is
 *   read or written.  A tap that falls outside the image contributes zero: it reads a zero page,
 *   not a neighbouring row, pixel or image.
 * w   [Cout][kh][kw][Cin / groups], dense.  Forward and backward-data read exactly these floats:
 *     nothing has to be zero, no row >= Cout is read.
 * stem4.  x is the dense 4-channel image (ldx == 4) with a FINITE fourth channel
 *     (catseg_nchw3_to_nhwc4 writes 0); w / dw are the packed [Cout][kh][8][4] image of
 *     catseg_stem_pack_weight: entries [..][7][.] and [..][.][3] of w are zero, the same entries
 *     of dw are written with values that catseg_stem_unpack_grad drops.
 *
 * forward
 *   x         exactly the columns [0, Cin) of the pixels a tap reaches are read; columns
 *             [Cin, ldx) are never read, whatever they hold.
 *   bias      [0, Cout) when not NULL.
 *   residual  columns [0, Cout) of the B Ho Wo pixels of ldr floats; the rest of a pixel is never
 *             read.
 *   y         columns [0, Cout) of every pixel are written (previous contents are not read, NaNs
 *             are overwritten): act((sum + bias) + residual); columns [Cout, zero_to) are written
 *             as +0; columns [max(Cout, zero_to), ldy) keep their bits.  zero_to <= Cout writes
 *             no zeros.  Grouped: zero_to == 0 and residual == NULL (CATSEG_EINVAL otherwise).
 *             There is no accumulating forward.
 * backward-data
 *   dy        columns [0, r4(Cout)) of the pixels a tap reaches are read, and the pad columns
 *             [Cout, r4(Cout)) MUST BE ZERO -- they are multiplied by zeros that stand in for w's
 *             rows >= Cout, so an Inf / NaN there would reach every column of the dx pixels the
 *             tap feeds (catseg_conv2d_fwd(zero_to) and catseg_bilinear_bwd(zero_to) write these
 *             zeros); columns [r4(Cout), ldy) are never read.  Grouped: Cout / groups is a
 *             multiple of 4, there are no pad columns.
 *   dx        columns [0, Cin) of EVERY pixel are written or added to; columns [Cin, ldx) keep
 *             their bits.  accumulate == 0: previous contents are not read, and a pixel no tap
 *             reaches (a parity class of a strided convolution without a tap) is written as +0.
 *             accumulate != 0: dx = dx + sum, the sum formed first; a pixel no tap reaches keeps
 *             its value.
 * backward-weight
 *   x         exactly the columns [0, Cin) of the pixels a tap reaches.
 *   dy        the B Ho Wo pixels only (the last K-step of 16 rows is filled with zeros, not with
 *             rows behind the tensor).  Columns [0, r4(Cout)) are read; the pad columns
 *             [Cout, r4(Cout)) may hold anything (they meet only accumulators that are not
 *             stored).  With dbias != NULL, ldy == 32 and Cout <= 32 all 32 columns are read, and
 *             [Cout, 32) may hold anything as well.  Other columns are never read.
 *   dw        all of [Cout][kh][kw][Cin / groups] is written (previous contents are not read),
 *             with or without a K split, through the implicit GEMM or the direct 48 / 96-channel
 *             kernel; dbias [0, Cout) when not NULL.  Nothing else is written: the partial sums of
 *             a split live in the workspace, whose contents are undefined afterwards.
 *
 * The summation order depends on the tile form, the split count and the kernel (and is fixed for a
 * given shape and plan): results are deterministic, and bit-identical across forms only where the
 * sums are exact. */
/* w'[o,:] = w[o,:] * gamma[o]/sqrt(rv[o]+eps), b'[o] = beta[o] + (b[o] - rm[o]) * gamma[o]/sqrt(rv[o]+eps);
 * per_out = floats per output channel of w (kh*kw*Cin, or 7*32 for the packed stem) */
int catseg_fold_bn(const float* w, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                   const float* running_var, float eps, int O, int per_out, float* w_folded, float* bias_folded,
                   catseg_stream_t stream);

/* ---- batched GEMM for the OCR gather / object attention (torch.matmul at
 * models/OCR.py:167,266,274).  C[z] (M x N, ldc) = op(A[z]) * op(B[z]):
 *   layout "NT": A is M x K (lda), B is N x K (ldb)      (K contiguous in both)
 *   layout "NN": A is M x K (lda), B is K x N (ldb)
 *   layout "TN": A is K x M (lda), B is K x N (ldb)      (reduction over rows) */
#define CATSEG_GEMM_NT 0
#define CATSEG_GEMM_NN 1
#define CATSEG_GEMM_TN 2
/* second stage of a K-split reduction: out[b][i] (+)= sum_s slabs[b][s][i] in a fixed order (slabs [batch][splits][n], n % 4 == 0).  The
 * OCR head's reductions over all N = H * W pixels into a K x C result (models/OCR.py:158-170 spatial gather, the value / key gradients of
 * :266-274) run as catseg_gemm_batched over batch * splits row chunks followed by this sum */
int catseg_sum_slabs(const float* slabs, float* out, long long n, int splits, int batch, int accumulate, catseg_stream_t stream);
/* Operand contract of catseg_gemm_batched (tests/test_gemm_gpu.py holds the kernel to every sentence; r4(n) = n rounded up to 4).
 * All layouts: A, Bm and C 16-byte aligned; lda, ldb, strideA, strideB multiples of 4 (ldc, strideC: any); 0 <= zero_to <= ldc; batch item
 *   z of an operand starts z * stride floats behind its pointer, and the strides may exceed the dense item (slices of wider buffers).
 *   Anything else returns CATSEG_EINVAL before a launch.  No row outside an item's logical rows, no float between or behind the batch
 *   items, is ever read or written.
 * NT  K % 4 == 0, K <= lda, ldb.  Exactly the columns [0, K) of A's M rows and of B's N rows are read: nothing has to be zero, columns
 *     [K, ld) are never read.
 * NN  r4(K) <= lda, r4(N) <= ldb.  A: columns [0, r4(K)) of its M rows are read, and the pad columns [K, r4(K)) MUST BE ZERO -- they are
 *     multiplied by zeros that stand in for B's rows >= K, so an Inf / NaN there would reach every column of that row of C (the softmax
 *     kernels that produce these operands write the zeros); columns [r4(K), lda) are never read.  B: rows [0, K) only -- rows >= K are
 *     never read, whatever they hold; of those rows columns [0, r4(N)) are read, the pad columns [N, r4(N)) may hold anything (they
 *     meet only accumulators that are not stored); columns [r4(N), ldb) are never read.
 * TN  r4(M) <= lda, r4(N) <= ldb.  Exactly the K rows of A and of B are read (the last K-step of 16 is filled with zeros, not with rows
 *     >= K); of those rows columns [0, r4(M)) of A and [0, r4(N)) of B are read, the pad columns [M, r4(M)) / [N, r4(N)) may hold
 *     anything (not stored), the columns behind them are never read.
 * C   Rows [0, M) of every batch item: columns [0, N) are written (accumulate == 0: previous contents are not read, NaNs are overwritten)
 *     or added to (accumulate != 0: C = C + A B, the product summed first); columns [N, zero_to) are written as +0 in BOTH modes;
 *     columns [max(N, zero_to), ldc) and everything between and behind the batch items keep their bits.  zero_to <= N writes no zeros.
 * The summation order over K depends on the tile the planner picks (and is fixed for a given shape): results are deterministic, and
 * bit-identical across tiles only where the sums are exact. */
int catseg_gemm_batched(int layout, int batch, int M, int N, int K, const float* A, int lda,
                        long long strideA, const float* Bm, int ldb, long long strideB, float* C,
                        int ldc, long long strideC, int zero_to, int accumulate,
                        catseg_stream_t stream);

/* ---- split-precision convolution on the bf16 matrix cores (csrc/igemm_bf16x3.hip): every fp32 operand is split exactly into
 * three bf16 planes (catseg_split3), six bf16 MFMA partial products per block reproduce the fp32 product to ~2^-23;
 * 2.7x the fp32-matrix peak.  Same F.conv2d call sites as catseg_conv2d_fwd / _bwd_data; results agree with the fp32 kernels
 * to ~1e-6 relative (not bit-identical). */
size_t catseg_split3_elems(long long rows, int C);   /* 16-bit elements per plane: rows * roundup(C, 8) */
int catseg_split3(const float* x, int ld, long long rows, int C, void* planes, catseg_stream_t stream);
int catseg_split3_weight_t(const float* w, int O, int taps, int Cin, void* planes, catseg_stream_t stream);
/* BLOCKED operand planes for the large layers (>= 193 output columns): activations [3][ceil(C/16)][rows][16], weights
 * [3][K/16][N][16] -- the 256 rows of one K-step form one contiguous run, so that every LDS-DMA instruction of the 256 x 256
 * kernel reads whole cache lines (the [rows][C] planes above gave each lane pair its own line and bounded that kernel by the
 * vector L1's line rate).  catseg_split3_blocked writes, from ONE pass over x, the blocked planes and -- if planar_planes is not
 * null -- the catseg_split3 layout as well (the backward-weight kernel keeps reading that one). */
size_t catseg_split3_blocked_elems(long long rows, int C);   /* 16-bit elements of ALL three planes: 3 * roundup(C, 16) * rows */
int catseg_split3_blocked(const float* x, long long rows, int C, int ld, void* blocked_planes, void* planar_planes,
                          catseg_stream_t stream);
int catseg_split3_weight_blocked(const float* w, int O, int taps, int Cin, void* planes, catseg_stream_t stream);    /* Cin % 16 == 0 */
int catseg_split3_weight_t_blocked(const float* w, int O, int taps, int Cin, void* planes, catseg_stream_t stream);  /* [taps*roundup(O,16)/16][Cin][16] */
/* dbias[o] = sum_p dy[p, o] (the bias-gradient part of catseg_conv2d_bwd_weight on its own); workspace >= 256 * C floats */
int catseg_bias_grad(const float* dy, int ld, long long rows, int C, float* dbias, void* workspace, size_t workspace_bytes,
                     catseg_stream_t stream);

/* ---- two-plane fp16 split precision (csrc/igemm_f16x2.hip): the same F.conv2d call sites as the bf16x3 blocked entry points above
 * (the OCR / auxiliary head convolutions 3x3 720 -> 512 and the 1x1 1024 -> 512 of models/OCR.py:88-104, UPerNet's fusion layers), half
 * the matrix work.  Every operand tensor is scaled by 2^e, e = 14 - floor(log2(max|x|)), and split into h = fp16(x 2^e),
 * l = fp16(x 2^e - h) (22 significant bits); the kernel accumulates hh + hl + lh in fp32 and scales the result by 2^-(e_x + e_w).
 *   `scale`: 8 bytes of DEVICE memory per operand, {uint32 bits of max|x|, int32 e}, written by the split call (two launches: amax,
 *   split) and read by the convolution -- no host round trip. */
size_t catseg_split2h_blocked_elems(long long rows, int C);   /* [2][ceil(C/16)][rows][16]: forward / backward-data operand */
size_t catseg_split2h_planar_elems(long long rows, int C);    /* [2][rows][roundup(C, 8)]: backward-weight operand */
int catseg_split2h(const float* x, long long rows, int C, int ld, void* blocked_planes, void* planar_planes, void* scale,
                   catseg_stream_t stream);                   /* either layout may be NULL; one pass over x for both */
/* catseg_split2h without the pass over x that finds max|x|: the maximum over up to four amax records the producers of x (or of its channel
 * slices) left (null = unused); a record may be an upper bound */
int catseg_split2h_bound(const float* x, long long rows, int C, int ld, void* blocked_planes, void* planar_planes, void* scale,
                         const void* rec0, const void* rec1, const void* rec2, const void* rec3, catseg_stream_t stream);
int catseg_split2h_weight_blocked(const float* w, int O, int taps, int Cin, void* planes, void* scale, catseg_stream_t stream);
/* blocked planes of the channel concatenation of up to four bilinearly resized tensors (F.interpolate(..., mode='bilinear', align_corners=False)
 * + torch.cat: the HRNet head input, models/HRNetv2.py:505-508) WITHOUT the fp32 concatenation: xs[i] NHWC [B][Hs[i]][Ws[i]][Cs[i]] (row stride
 * lds[i], Cs[i] % 16 == 0; a source of the output's size is copied), records[i] its amax record; planes [2][sum Cs / 16][B Ho Wo][16]. */
int catseg_concat_bilinear_split2h(int nsrc, const float* const* xs, const int* lds, const int* Hs, const int* Ws, const int* Cs,
                                   const void* const* records, int B, int Ho, int Wo, void* blocked_planes, void* scale, catseg_stream_t stream);
int catseg_split2h_weight_t_blocked(const float* w, int O, int taps, int Cin, void* planes, void* scale, catseg_stream_t stream);
/* (one blocked plane set per tensor serves all three directions of a layer: the backward of F.conv2d at models/OCR.py:72-89, 326-333) */

/* ---- the first stem convolution of HRNet: nn.Conv2d(3, 64, 3, stride 2, padding 1) on the image (models/HRNetv2.py:281-283), exact fp32, HBM-bound
 * direct kernels (csrc/stem3.hip).  x is addressed through element strides (sb, sc, sy, sx) for (batch, channel, row, column): NCHW or NHWC-4,
 * no repack pass.  w / dw: OHWI [64][3][3][3].  y / dy: NHWC rows of ldy floats.
 *   catseg_stem3_fwd: y = F.conv2d(x, w, bias, 2, 1); bn_part != NULL: catseg_stem3_partial_rows(B, H, W) rows [row][3][64] of BatchNorm
 *                     partials (K, sum(v - K), sum((v - K)^2)) with pixel counts in bn_counts, for catseg_bn_finalize_counts.
 *   catseg_stem3_bwd_weight: dw = the weight gradient of the same call (autograd of F.conv2d); workspace catseg_stem3_wgrad_workspace(). */
int catseg_stem3_supported(int H, int W, int Cout);
int catseg_stem3_partial_rows(int B, int H, int W);
size_t catseg_stem3_wgrad_workspace(void);
int catseg_stem3_fwd(const float* x, long long sb, long long sc, long long sy, long long sx, int B, int H, int W, const float* w, const float* bias,
                     float* y, int ldy, float* bn_part, int* bn_counts, catseg_stream_t stream);
int catseg_stem3_bwd_weight(const float* x, long long sb, long long sc, long long sy, long long sx, int B, int H, int W, const float* dy, int lddy,
                            float* dw, void* workspace, size_t workspace_bytes, catseg_stream_t stream);

/* ---- the first convolution of the torchvision ResNet stem: nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False) on the image (the resnet50 / resnet101
 * backbones built at models/OCR.py:58-61 and models/DeepLabv3Plus.py:32-38 of the reference; torchvision's `conv1`), training forward as a direct
 * kernel whose 147 products per output are accumulated in fp64 and rounded once (csrc/stem7.hip).  Arguments as catseg_stem3_fwd; w: OHWI [64][7][7][3].
 *   catseg_stem7_fwd: y = F.conv2d(x, w, bias, 2, 3); bn_part != NULL: catseg_stem7_partial_rows(B, H, W) rows of BatchNorm partials + pixel counts. */
int catseg_stem7_supported(int H, int W, int Cout);
int catseg_stem7_partial_rows(int B, int H, int W);
int catseg_stem7_fwd(const float* x, long long sb, long long sc, long long sy, long long sx, int B, int H, int W, const float* w, const float* bias,
                     float* y, int ldy, float* bn_part, int* bn_counts, catseg_stream_t stream);

/* ---- direct 3x3 / stride 1 / pad 1 convolution in split precision (csrc/dconv3_b3.hip) for the HRNet trunk: the BasicBlock
 * convolutions conv3x3(planes, planes) at models/HRNetv2.py:22-25,41-44 (Cin = Cout = C in {48, 96}; catseg_dconv3_supported).
 * Same F.conv2d call sites and same arithmetic as catseg_conv2d_fwd on bf16x3 operands (three exact bf16 planes per fp32 operand, six bf16
 * MFMA products, fp32 accumulation), but the activation is read as fp32 and split inside the kernel: a block loads the halo
 * tile of its pixel tile once and forms all nine taps from it.
 *   catseg_dconv3_prep: OHWI fp32 weights [C][3][3][C] -> the kernel's pre-split weight image (catseg_dconv3_wimg_bytes bytes);
 *                       backward_data != 0: the transposed, tap-mirrored bank, with which the same kernel run on dy computes dx.
 *   catseg_dconv3:      y[p, o] (+)= sum_{ky,kx,c} x[pix(p,ky,kx), c] * w[o,ky,kx,c] (+ bias[o]).  bn_part != NULL: BatchNorm partials
 *                       [n_tiles][3][C] (tile mean, s1, s2) + bn_counts[n_tiles] (valid pixels of each tile; n_tiles =
 *                       catseg_dconv3_tiles) for catseg_bn_finalize_counts. */
int catseg_dconv3_supported(int C);
size_t catseg_dconv3_wimg_bytes(int C);
int catseg_dconv3_tiles(int C, int B, int H, int W, int* tile_h, int* tile_w);
int catseg_dconv3_prep(const float* w, int C, int backward_data, void* wimg, catseg_stream_t stream);
/* the weight images of ALL direct-kernel layers of a network in one launch (the parameters live in one flat buffer): `entries` is a
 * DEVICE array of n records {int64 weight offset in floats from `flat`; int64 image offset in bytes from wimg_base; int32 C; int32 KC;
 * int32 NT; int32 backward_data} with KC / NT from catseg_dconv3_layout(C) */
int catseg_dconv3_layout(int C, int* kc, int* nt);
int catseg_dconv3_prep_batch(const float* flat, int n, const void* entries, void* wimg_base, catseg_stream_t stream);
int catseg_dconv3(int B, int H, int W, int C, const float* x, int ldx, const void* wimg, const float* bias, float* y, int ldy,
                  int accumulate, float* bn_part, size_t bn_part_floats, int* bn_counts, catseg_stream_t stream);
/* backward-data of a BasicBlock's SECOND convolution fused with the first pass of the backward of the relu(bn1(q)) that produced
 * its input (models/HRNetv2.py:36-47: out = relu(bn1(conv1(x))); conv2(out)): g = (dy (*) w^T) where relu(bn1(q)) > 0 (the mask is
 * recomputed from q, stats = [mean(C), invstd(C)], gamma, beta with the forward's exact expression), and part[n_tiles][2][C] = per
 * tile sum of g and of g * xhat -- what the first pass of catseg_bn_backward computes from (dz, q).  catseg_bn_backward given these partials finishes. */
int catseg_dconv3_bnbwd(int B, int H, int W, int C, const float* dy, int lddy, const void* wimg_bwd, float* g, int ldg, const float* q,
                        int ldq, const float* stats, const float* gamma, const float* beta, float* part, size_t part_floats,
                        catseg_stream_t stream);
/* The same direct kernels on TWO fp16 planes and THREE products (csrc/dconv3_f16x2.hip = dconv3_b3.hip compiled with DC_H2; the
 * arithmetic of catseg_conv2d_fwd on f16x2 operands).  The activation is split inside the kernel, so its power-of-two prescale comes from a
 * DEVICE amax record of CATSEG_AMAX_RECORD_BYTES = 2048 bytes (16 uint32 slots 128 bytes apart; max over the slots = bits of max|x|
 * over the whole tensor) that the PRODUCER of x accumulated (catseg_bn_apply, catseg_add_n_act, catseg_bn_backward given a record:
 * one fire-and-forget atomicMax per block into slot blockIdx % 16; the caller zeroes the record before the producer runs).  A record value above the true maximum is safe, one below it overflows fp16.
 *   catseg_dconv3_f16x2_prep_batch: as catseg_dconv3_prep_batch (same entry records) + `records`, n x 8 bytes: per weight image
 *                                   {bits of max|w|, exponent}, computed on the device (memset + amax launch + image launch). */
#define CATSEG_AMAX_RECORD_BYTES 2048
size_t catseg_dconv3_f16x2_wimg_bytes(int C);
int catseg_dconv3_f16x2_prep_batch(const float* flat, int n, const void* entries, void* wimg_base, void* records, catseg_stream_t stream);
int catseg_dconv3_f16x2(int B, int H, int W, int C, const float* x, int ldx, const void* x_record, const void* wimg, const void* w_record,
                        const float* bias, float* y, int ldy, int accumulate, float* bn_part, size_t bn_part_floats, int* bn_counts,
                        catseg_stream_t stream);
int catseg_dconv3_bnbwd_f16x2(int B, int H, int W, int C, const float* dy, int lddy, const void* dy_record, const void* wimg_bwd,
                              const void* w_record, float* g, int ldg, const float* q, int ldq, const float* stats, const float* gamma,
                              const float* beta, float* part, size_t part_floats, catseg_stream_t stream);
/* backward-weight on two fp16 planes (csrc/dwgrad3_f16x2.hip = dwgrad3_b3.hip compiled with DW_H2): both operands' amax records;
 * workspace = catseg_dwgrad3_workspace */
int catseg_dwgrad3_f16x2(int B, int H, int W, int C, const float* x, int ldx, const void* x_record, const float* dy, int ldy,
                         const void* dy_record, float* dw, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* backward-weight of the same layers (csrc/dwgrad3_b3.hip): dw[o,ky,kx,c] = sum_p dy[p, o] * x[pix(p,ky,kx), c], C in {48, 96, 192, 384};
 * x and dy are read as fp32 and split inside the kernel, fragments by transposed LDS reads, per-block partial sums in
 * `workspace` (catseg_dwgrad3_workspace bytes) added in a fixed order */
int catseg_dwgrad3_supported(int C);
size_t catseg_dwgrad3_workspace(int B, int H, int W, int C);
int catseg_dwgrad3(int B, int H, int W, int C, const float* x, int ldx, const float* dy, int ldy, float* dw, void* workspace,
                   size_t workspace_bytes, catseg_stream_t stream);

/* ---- FCN-8s pieces (models/FCN.py:7-61 of the reference): F.max_pool2d(x, 2) with its argmax (idx: uint8 [B, H/2, W/2, C]) and backward
 * (models/FCN.py:44-53); catseg_bias_rows: out[r][0..C) = bias -- the rows nn.ConvTranspose2d's bias initialises before the transposed
 * convolution (= catseg_conv2d_bwd_data with the same weight tensor, models/FCN.py:35-38) accumulates into them */
int catseg_maxpool2x2_fwd(const float* x, int ldx, float* y, int ldy, uint8_t* idx, int B, int H, int W, int C, catseg_stream_t stream);
int catseg_maxpool2x2_bwd(const float* dy, int lddy, const uint8_t* idx, float* dx, int lddx, int B, int H, int W, int C, catseg_stream_t stream);
int catseg_bias_rows(const float* bias, float* out, int ld, long long rows, int C, catseg_stream_t stream);

/* ---- UNet pieces (models/UNet.py:6-63 of the reference: conv + bias + ReLU without BatchNorm, MaxPool2d(2), 2x bilinear Upsample with
 * align_corners=True, torch.cat([up, skip], 1)); csrc/unet.hip.  The passes a skip junction needs anyway also leave the amax records
 * (CATSEG_AMAX_RECORD_BYTES, zeroed by the caller; max|.| of exactly what was written is folded into the slots) that let the layers reach
 * the split-precision direct / pointwise / gather kernels.  NHWC fp32, every C and ld a multiple of 4, 16-byte aligned tensors; anything
 * else returns CATSEG_EINVAL and launches nothing.  Pad columns (ld > C) are never read.
 *   catseg_amax_record         record <- max|x| over [rows][0 .. C): a read-only pass
 *   catseg_maxpool2x2_fwd_rec  y, idx exactly as catseg_maxpool2x2_fwd; x_record <- max|x| over the whole input (an odd last row / column
 *                              included), y_record <- max|y|; either record may be NULL
 *   catseg_upcat2x_fwd         cat[B, 2h, 2w, 0 .. Cx) = catseg_bilinear_fwd(x [B, h, w, Cx], align_corners = 1) bit for bit,
 *                              cat[B, 2h, 2w, Cx .. Cx + Cs) = skip [B, 2h, 2w, Cs]; record (may be NULL) <- max|cat|
 *   catseg_relu_bwd_rec        g = d * (z > 0) on [B, H, W, C], record (may be NULL) <- max|g|.  dpool == idx == NULL: d = dz.  Junction
 *                              form (z fed a 2x2 max-pool AND a concatenation): d = dz + catseg_maxpool2x2_bwd(dpool [B, H/2, W/2, C], idx),
 *                              dz being the channel slice of the concatenation's gradient (pointer to its first column, lddz its ld) */
int catseg_amax_record(const float* x, int ld, long long rows, int C, void* record, catseg_stream_t stream);
int catseg_maxpool2x2_fwd_rec(const float* x, int ldx, float* y, int ldy, uint8_t* idx, int B, int H, int W, int C, void* x_record,
                              void* y_record, catseg_stream_t stream);
int catseg_upcat2x_fwd(const float* x, int ldx, const float* skip, int lds, float* cat, int ldc, int B, int h, int w, int Cx, int Cs,
                       void* record, catseg_stream_t stream);
int catseg_relu_bwd_rec(const float* dz, int lddz, const float* dpool, int lddp, const uint8_t* idx, const float* z, int ldz, float* g,
                        int ldg, int B, int H, int W, int C, void* record, catseg_stream_t stream);

/* ---- fp16 x 2 OPERAND PLANES written by the producer of a tensor, and the direct 3x3 kernels that stream them (round 4;
 * csrc/planes.h, csrc/dconv3_pl.hip).  Replaces, for the same reference layers as catseg_dconv3_f16x2 (conv3x3(planes, planes) of
 * models/HRNetv2.py:22-65), the in-kernel fp32 -> 2 x fp16 split: planes = [plane h / l][C / 8 channel groups][pixel][8] fp16,
 * catseg_planes_bytes(rows, C) bytes, written with the exponent e that the tensor's amax record holds in word 1 (xs = x * 2^e).
 *   catseg_planes_from_f32:  standalone producer (tests; tensors whose producing kernel writes no planes).  compute_amax != 0: the record
 *                            is zeroed and max|x| taken here; else its 16 amax slots are taken as they are (a larger value is safe).
 *   catseg_dconv3_pl:        catseg_dconv3_f16x2 on planes.  BatchNorm partials PER WAVE: catseg_dconv3_pl_rows(C, B, H, W) rows of
 *                            [3][C] floats + one int32 count per row, for catseg_bn_finalize_counts.  out_record (may be NULL): max|y| is
 *                            folded into its amax slots (the BatchNorm that follows derives the exponent of ITS output planes from it).
 *   catseg_dconv3_pl_bnbwd:  catseg_dconv3_bnbwd_f16x2 on planes of dy; part = [rows][2][C]; max|g| to out_record. */
int catseg_dconv3_pl_supported(int C);
int catseg_dconv3_pl_rows(int C, int B, int H, int W);
size_t catseg_planes_bytes(long long rows, int C);
int catseg_planes_from_f32(const float* x, int ld, long long rows, int C, void* record, void* planes, int compute_amax, catseg_stream_t stream);
int catseg_dconv3_pl(int B, int H, int W, int C, const void* planes, const void* planes_record, const void* wimg, const void* w_record,
                     const float* bias, float* y, int ldy, int accumulate, float* bn_part, size_t bn_part_floats, int* bn_counts,
                     void* out_record, catseg_stream_t stream);
int catseg_dconv3_pl_bnbwd(int B, int H, int W, int C, const void* dy_planes, const void* dy_record, const void* wimg_bwd, const void* w_record,
                           float* g, int ldg, const float* q, int ldq, const float* stats, const float* gamma, const float* beta, float* part,
                           size_t part_floats, void* out_record, catseg_stream_t stream);

/* PRODUCERS of planes: the kernels that write a trunk activation / gradient write its planes in the same pass (csrc/norm.hip,
 * csrc/pointwise.hip).  The exponent is fixed BEFORE the pass from a bound of max| |:
 *   catseg_bn_finalize_counts_bound: catseg_bn_finalize_counts, and z_record[2] = max_c |scale_c| (max|y| + |mean_c|) + |beta_c| (max|y| from
 *                                    y_record, the record catseg_dconv3_pl's epilogue filled)                  [nn.BatchNorm2d training forward]
 *   catseg_bn_apply with z_planes:   planes of z (+ z itself when z != NULL); exponent from the record's bound + max|residual|
 *   catseg_add_n_act with out_planes: out and its planes; exponent from the sum of the terms' max| |                  [HRNet fuse sum]
 *   catseg_bn_backward with dy_planes: dy as planes ONLY; bound |gamma invstd| (max|g| + |mean g| + max|xhat| |mean g xhat|) per
 *                                    channel                                                                  [autograd of BatchNorm2d] */
int catseg_bn_finalize_counts_bound(const float* partials, int n_blocks, const int* counts, long long rows, int C, const float* gamma,
                                    const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* stats_out,
                                    float* scale, const void* y_record, void* z_record, catseg_stream_t stream);
/* The K-class classifier of a segmentation head fused with the BatchNorm + ReLU in front of it (csrc/headfuse.h; replaces nn.BatchNorm2d + ReLU +
 * the 1 x 1 nn.Conv2d of models/OCR.py:72-74 (interm_prediction_head[1..4]) and :97 with conv_bn_dropout[1..2], and their autograd): the
 * normalised activation z and its gradient exist in registers only.
 *   catseg_head_fwd       logits[rows][ldl] = relu((y - mean) * scale + beta) Wh^T + bh, columns [K, zero_to) zeroed; Wh [K][C], K <= 32,
 *                         C % 32 == 0, C <= 512; mean / scale as catseg_bn_finalize left them
 *   catseg_head_backward  from dl [rows][lddl] (lddl >= 32): dy as the blocked planes + scale record of catseg_bn_backward's dy_h2_planes (same three zeroed
 *                         amax records), dgamma / dbeta of the BatchNorm, dbias (may be null) = column sums of dy, dwh [K][C] and dbh [K]
 *                         (may be null) of the classifier -- all WRITTEN; C % 64 == 0; workspace = catseg_head_backward_workspace bytes;
 *                         every reduction in a fixed order (deterministic) */
int catseg_head_fwd(const float* y, int ldy, const float* mean, const float* scale, const float* beta, const float* wh, const float* bh, int K,
                    long long rows, int C, float* logits, int ldl, int zero_to, catseg_stream_t stream);
size_t catseg_head_backward_workspace(long long rows, int C);
int catseg_head_backward(const float* dl, int lddl, const float* y, int ldy, const float* stats, const float* gamma, const float* beta,
                         const float* wh, int K, long long rows, int C, void* dy_planes, void* dy_scale, float* dgamma, float* dbeta, float* dbias,
                         float* dwh, float* dbh, void* g_record, void* y_record, void* dy_record, void* workspace, size_t workspace_bytes,
                         catseg_stream_t stream);

/* nn.Dropout2d of the OCRNet heads (csrc/dropout.hip; models/OCR.py:87 interm_prediction_head[3] and :311-316 conv_bn_dropout[3] of the reference):
 * one keep decision per (image, channel), kept channels scaled by 1 / (1 - p).
 *   catseg_dropout2d_mask        ONE launch draws mult [B][C] (0 or 1 / (1 - p); p == 1: all zeros) and, where bits is given (C % 32 == 0), the
 *                                packed keep bits [B][C / 32], and advances the draw counter.  state: 16 bytes of device memory {seed lo, seed hi,
 *                                layer | rank << 16, draw counter}.  Element i = n C + c takes word i & 3 of philox4x32_10(counter = (i >> 2, draw,
 *                                0, layer | rank << 16), key = (seed lo, seed hi)); u = (word >> 8) 2^-24; kept iff u >= p.  No host value enters
 *                                a draw: a captured launch draws the next mask at every replay.
 *   catseg_dropout2d_mask_fixed  the same two tables from a given 0 / 1 table keep01 [B][C]; no state
 *   catseg_dropout2d_apply       out[row][c] = x[row][c] * mult[row / hw][c], rows = B hw NHWC pixels; C and both row strides multiples of 4;
 *                                out may be x.  Forward and backward of the routes that do not run the fused head kernels.
 *   catseg_head_fwd_drop / catseg_head_backward_drop   catseg_head_fwd / catseg_head_backward with the dropout between the ReLU and the
 *                                classifier: z_d = m z feeds the logits and dWh, g = relu' m (dl Wh) everything else; bits / keep as
 *                                catseg_dropout2d_mask wrote them (keep = 1 / (1 - p) >= 1), hw = H W of an image, C % 64 == 0 */
int catseg_dropout2d_mask(void* state, float p, int B, int C, float* mult, unsigned* bits, catseg_stream_t stream);
int catseg_dropout2d_mask_fixed(const float* keep01, float p, int B, int C, float* mult, unsigned* bits, catseg_stream_t stream);
int catseg_dropout2d_apply(const float* x, int ldx, const float* mult, long long rows, int C, long long hw, float* out, int ldo,
                           catseg_stream_t stream);
int catseg_head_fwd_drop(const float* y, int ldy, const float* mean, const float* scale, const float* beta, const float* wh, const float* bh, int K,
                         long long rows, int C, float* logits, int ldl, int zero_to, const unsigned* bits, long long hw, float keep,
                         catseg_stream_t stream);
int catseg_head_backward_drop(const float* dl, int lddl, const float* y, int ldy, const float* stats, const float* gamma, const float* beta,
                              const float* wh, int K, long long rows, int C, void* dy_planes, void* dy_scale, float* dgamma, float* dbeta,
                              float* dbias, float* dwh, float* dbh, void* g_record, void* y_record, void* dy_record, void* workspace,
                              size_t workspace_bytes, const unsigned* bits, long long hw, float keep, catseg_stream_t stream);

/* catseg_dwgrad3_f16x2 on producer-written planes of BOTH operands (csrc/dwgrad3_pl.hip): dw[o][ky][kx][c] = sum_px dy[px][o] x[px + tap][c]
 * for the trunk widths 48 / 96 / 192 / 384 (autograd of F.conv2d, models/HRNetv2.py:22-65); workspace = catseg_dwgrad3_pl_workspace bytes
 * (slabs of partial sums, added in a fixed order: deterministic) */
int catseg_dwgrad3_pl_supported(int C);
size_t catseg_dwgrad3_pl_workspace(int B, int H, int W, int C);
int catseg_dwgrad3_pl(int B, int H, int W, int C, const void* x_planes, const void* x_record, const void* dy_planes, const void* dy_record,
                      float* dw, void* workspace, size_t workspace_bytes, catseg_stream_t stream);

/* (tuning / measurement hooks live in catseg_debug.h: they are process-global and not part of the product surface) */

/* ---- BatchNorm (+ReLU, +residual) — nn.BatchNorm2d/ReLU at e.g. models/OCR.py:74-75,
 * torchvision Bottleneck, models/DeepLabv3Plus.py:98-104.  rows = B*H*W pixels. */
/* batch statistics + running-stat update.  stats_out = [mean(C), invstd(C)] (biased variance),
 *   scale = gamma*invstd.  running_mean/var may be NULL (no update; unbiased variance, momentum
 *   as nn.BatchNorm2d).  workspace >= catseg_bn_workspace(rows, C). */
size_t catseg_bn_workspace(long long rows, int C);
int catseg_bn_train_stats(const float* y, long long rows, int C, int ldy, const float* gamma, float eps,
                          float momentum, float* running_mean, float* running_var, float* stats_out,
                          float* scale, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* merge of [n_blocks][3][C] partials (per row block: K, sum(y - K), sum((y - K)^2)) into the batch statistics: the second half
 * of catseg_bn_train_stats, fed by the convolution epilogues above */
int catseg_bn_finalize(const float* partials, int n_blocks, long long rows_per_block, long long rows, int C, const float* gamma,
                       float eps, float momentum, float* running_mean, float* running_var, float* stats_out, float* scale,
                       catseg_stream_t stream);
/* the same merge for blocks with individual row counts (2-D pixel tiles with ragged edges: catseg_dconv3) */
int catseg_bn_finalize_counts(const float* partials, int n_blocks, const int* counts, long long rows, int C, const float* gamma,
                              float eps, float momentum, float* running_mean, float* running_var, float* stats_out, float* scale,
                              catseg_stream_t stream);
/* eval mode: scale = gamma / sqrt(running_var + eps) (use with mean = running_mean) */
int catseg_bn_eval_scale(int C, const float* gamma, const float* running_var, float eps, float* scale,
                         catseg_stream_t stream);
/* z = act((y - mean) * scale + beta (+ residual)),  act = relu if relu != 0.  The optional fields that are non-NULL say what is written:
 *   z_planes == NULL   z (required); record (may be NULL): a zeroed amax record, max|z| is folded into it
 *   z_planes != NULL   the fp16 x 2 planes of z (catseg_planes_bytes(rows, C); C % 8 == 0), and z itself only when z != NULL.  record
 *                      (required) is the record catseg_bn_finalize_counts_bound left the bound in: the exponent comes from it (+ max|residual|
 *                      from residual_record, required with a residual), max|z| is folded into its amax slots
 *   mask != NULL       also the ReLU mask of z as BITS (catseg_bn_mask_bytes(rows, C) = rows C / 8 bytes: bit (e & 7) of byte e >> 3 for the
 *                      flat element index e = r C + c); needs relu and C % 8 == 0.  For z = relu(bn(y) + residual) of a residual block
 *                      (models/HRNetv2.py:36-106, torchvision's BasicBlock / Bottleneck), whose backward then reads 1 bit per element, not z */
typedef struct {
  const float* y; int ldy;
  const float* mean; const float* scale; const float* beta;
  const float* residual; int ldr;      /* may be NULL */
  const void* residual_record;
  float* z; int ldz;
  void* z_planes;
  long long rows; int C;
  int relu;
  void* record;
  void* mask;
} catseg_bn_apply_desc;
size_t catseg_bn_mask_bytes(long long rows, int C);
int catseg_bn_apply(const catseg_bn_apply_desc* d, catseg_stream_t stream);

/* backward of the fused op.  g = dz * (ReLU mask if relu).  Produces dgamma, dbeta (either may be NULL), the gradient of y in ONE of three
 * forms and, when dres != NULL, the residual-branch gradient (dres (+)= g if dres_accumulate).
 *   ReLU mask (relu != 0)  from z; or from the bits in mask (as catseg_bn_apply wrote them; C % 8 == 0; z is then not read and must be NULL);
 *                          or, with neither and no residual branch, recomputed from y, gamma, beta and the saved statistics with the
 *                          forward's exact expression (one tensor read less in both passes)
 *   partials != NULL       dz is already masked and [n_blocks][2][C] per-block sums of g and g * xhat exist (catseg_dconv3_bnbwd and its
 *                          kin): the first pass is skipped.  Not with relu, z, mask, dres or the h2 output; workspace >= 2 C floats
 *                          (rounded up to 256 bytes), catseg_bn_workspace(rows, C) otherwise
 *   dy                     fp32 [rows][lddy]; dy_record (may be NULL): a zeroed amax record, max|dy| is folded into it; g_record and
 *                          y_record must be NULL
 *   dy_planes              the fp16 x 2 planes of catseg_planes_bytes(rows, C) ONLY (C % 8 == 0).  g_record: a zeroed amax record that
 *                          receives max|g| (with partials: the one their producer filled); y_record: max|y| of the forward pass;
 *                          dy_record: zeroed, receives the bound the exponent comes from, and the exponent
 *   dy_h2_planes           ONLY the blocked fp16 x 2 planes of catseg_split2h (catseg_split2h_blocked_elems(rows, C) halves) with
 *                          dy_h2_scale, their 8-byte record {bits of the bound, e} -- for a layer whose backward-weight / backward-data run
 *                          catseg_conv2d_bwd_weight / catseg_conv2d_bwd_data on CATSEG_OPERANDS_F16X2_BLOCKED (the BatchNorm behind the head
 *                          convolutions, models/OCR.py:72-89, 326-333).  dbias (may be NULL) = column sums of dy (gradient of a convolution
 *                          bias in front of the BatchNorm).  No residual branch, no mask; C % 64 == 0; the planes below 4 GB; g_record /
 *                          y_record / dy_record: three zeroed amax records, they receive max|g|, max|y| and the bound;
 *                          workspace >= catseg_bn_backward_h2_workspace(rows, C) */
typedef struct {
  const float* dz; int lddz;
  const float* y; int ldy;
  const float* stats;                  /* [mean(C), invstd(C)] */
  const float* gamma;
  long long rows; int C;
  int relu; const float* z; int ldz; const float* beta; const void* mask;
  const float* partials; int n_blocks;
  float* dres; int lddres; int dres_accumulate;
  void* g_record; void* y_record; void* dy_record;
  float* dgamma; float* dbeta;
  void* workspace; size_t workspace_bytes;
  float* dy; int lddy;
  void* dy_planes;
  void* dy_h2_planes; void* dy_h2_scale; float* dbias;
  int frozen;                          /* != 0: the statistics are constants of the layer, not functions of y (below) */
  const float* running_mean; const float* running_var; float eps;
  const float* scale;                  /* [C], the row catseg_bn_eval_scale wrote for the forward pass */
} catseg_bn_backward_desc;
size_t catseg_bn_backward_h2_workspace(long long rows, int C);
int catseg_bn_backward(const catseg_bn_backward_desc* d, catseg_stream_t stream);
/* frozen != 0: backward of z = act((y - running_mean) * scale + beta (+ residual)) with scale = gamma / sqrt(running_var + eps) -- a BatchNorm
 * that keeps its running statistics while its gamma / beta train (nn.BatchNorm2d.eval() inside a training model):
 *   g = dz * (ReLU mask if relu);  dy = g * scale[c];  dres (+)= g;  dbeta[c] = sum_rows g;
 *   dgamma[c] = invstd[c] * sum_rows g * (y - running_mean[c]),  invstd = 1 / sqrt(running_var + eps) in fp32
 * dy does not depend on the column sums: ONE streaming pass reads dz and the mask source (y only when dgamma is wanted or the mask is
 * recomputed from it), writes dy and dres and leaves [row blocks][2][C] partial sums in the workspace; a small launch adds them in block
 * order (no float atomics: two calls on the same input give the same bits).  With dgamma and dbeta both NULL nothing is summed and the
 * second launch does not happen.  The three ReLU mask sources are those above; the recomputed one evaluates the forward's expression on
 * (y, running_mean, scale, beta) and equals the mask catseg_bn_apply produced bit for bit.
 * Output: dy (fp32) only, dy_record as above.  stats, partials, dy_planes, dy_h2_planes, dy_h2_scale and dbias must be NULL, gamma is not read;
 * running_mean, running_var and scale are required.  With frozen == 0 the four fields behind it must be NULL / 0.
 * workspace >= catseg_bn_workspace(rows, C) suffices. */

/* ---- layout / pointwise helpers ---------------------------------------------------------- */
/* img.float() NCHW (B,3,H,W) -> NHWC with 4 channels (4th = 0) : managers/OCRNet_Manager.py:86 */
int catseg_nchw3_to_nhwc4(const float* x, float* y, int B, int H, int W, catseg_stream_t stream);
/* the same with torchvision.transforms.Normalize folded in (models/Ensemble.py:63-65 normalises the frame for its UPerNet members only):
 * y[b][h][w][c] = (x[b][c][h][w] - mean[c]) / stdv[c] for c < 3 -- a subtraction and a TRUE division, two roundings, bit-identical to
 * tensor.sub_(mean).div_(std) -- and 0 for c = 3.  mean, stdv: HOST float[3] (stdv[c] != 0).  y 16-byte aligned. */
int catseg_nchw3_to_nhwc4_norm(const float* x, float* y, int B, int H, int W, const float* mean, const float* stdv,
                               catseg_stream_t stream);
/* OIHW-logical/OHWI-physical 7x7x3 stem weight -> packed [O][7][8][4] and back (gradient) */
int catseg_stem_pack_weight(const float* w_ohwi, float* packed, int O, catseg_stream_t stream);
int catseg_stem_unpack_grad(const float* packed_grad, float* dw_ohwi, int O, catseg_stream_t stream);
/* dst[p, c] (+)= alpha * src[p, c] */
int catseg_axpy2d(const float* src, int lds, float* dst, int ldd, long long rows, int C, float alpha,
                  int accumulate, catseg_stream_t stream);
/* out = act(in_0 + ... + in_{n-1}), n <= 4 (HRNet fuse sum, models/HRNetv2.py:237-261).  term_records and out_planes both NULL: out_record
 * (may be NULL) is a zeroed amax record, max|out| is folded into it.  Both given (C % 8 == 0, out_record required): the fp16 x 2 planes of out
 * are written too, with the exponent from the SUM of the terms' max| | (term_records[i] = the amax record of in[i]).  g = dz * (z > 0) */
int catseg_add_n_act(const float* const* in, const int* ld, const void* const* term_records, int n, float* out, int ldo, void* out_planes,
                     long long rows, int C, int relu, void* out_record, catseg_stream_t stream);
int catseg_relu_bwd(const float* dz, int lddz, const float* z, int ldz, float* g, int ldg, long long rows, int C,
                    catseg_stream_t stream);
/* conv weight [O][taps][cin] -> zero-padded [O][taps][cpad] (unpad = 0) or back (unpad = 1): lets a
 * 3-channel 3x3 stem (models/HRNetv2.py:311) run on the 4-channel NHWC image */
int catseg_weight_pad_cin(const float* w, float* out, int O, int taps, int cin, int cpad, int unpad,
                          catseg_stream_t stream);
/* x[i] *= s[0], s on the device (applies an upstream loss gradient without a host sync) */
int catseg_scale_by_device_scalar(float* x, long long n, const float* s, catseg_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) of the torchvision stem; idx = window position of the max (uint8) */
int catseg_maxpool3x3s2_fwd(const float* x, int ldx, float* y, int ldy, uint8_t* idx, int B, int H, int W,
                            int C, int Ho, int Wo, catseg_stream_t stream);
int catseg_maxpool3x3s2_bwd(const float* dy, int lddy, const uint8_t* idx, float* dx, int lddx, int B,
                            int H, int W, int C, int Ho, int Wo, catseg_stream_t stream);
/* F.interpolate(mode='bilinear') — models/OCR.py:128-131, DeepLabv3Plus.py:68,123,163,
 * HRNetv2.py:253-256,504-512.  NHWC, C channels, input ld ldx, output ld ldy. */
int catseg_bilinear_fwd(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, int Ho,
                        int Wo, int align_corners, int accumulate, catseg_stream_t stream);
/* dx[., c] = sum of dy contributions (deterministic gather form); columns [C, zero_to) of dx zeroed.
 * workspace >= B*H*Wo*C*4 bytes. */
int catseg_bilinear_bwd(const float* dy, int lddy, float* dx, int lddx, int B, int H, int W, int C,
                        int Ho, int Wo, int align_corners, int zero_to, int accumulate, void* workspace,
                        size_t workspace_bytes, catseg_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) (ASPP image pooling, DeepLabv3Plus.py:121) and its backward */
int catseg_global_avgpool_fwd(const float* x, int ldx, float* y, int B, int HW, int C,
                              catseg_stream_t stream);
int catseg_global_avgpool_bwd(const float* dy, float* dx, int lddx, int B, int HW, int C, int accumulate,
                              catseg_stream_t stream);

/* nn.AdaptiveAvgPool2d(S) (UPerNet pyramid pooling, models/UPerNet.py:25-33); y is [B][S][S][C] compact */
int catseg_adaptive_avgpool_fwd(const float* x, int ldx, float* y, int B, int H, int W, int C, int S,
                                catseg_stream_t stream);
int catseg_adaptive_avgpool_bwd(const float* dy, float* dx, int lddx, int B, int H, int W, int C, int S,
                                int accumulate, catseg_stream_t stream);

/* ---- softmax ------------------------------------------------------------------------------ */
/* F.softmax(probs.view(B,K,N), dim=2) at models/OCR.py:165, on NHWC logits [B][N][ld]:
 * per (b, k) over the N pixels, K <= 64 (one block column per 32 classes).  Columns [K, ld) of the output are zeroed.
 * _bwd: dx (+)= y * (dy - sum_n dy y) in columns [0, K); columns [K, ld) of dx are WRITTEN ZERO, also when accumulate != 0
 * (the pad columns of a class-logit buffer stay zero whatever was there). */
size_t catseg_softmax_spatial_workspace(int B, int N);
int catseg_softmax_spatial_fwd(const float* x, float* y, int B, int N, int K, int ld, void* workspace,
                               size_t workspace_bytes, catseg_stream_t stream);
int catseg_softmax_spatial_bwd(const float* y, const float* dy, float* dx, int B, int N, int K, int ld,
                               int accumulate, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* F.softmax(scale * sim, dim=-1) at models/OCR.py:270-271: per row over K (<= 64) columns */
int catseg_softmax_rows_fwd(const float* x, float* y, long long rows, int K, int ld, float scale,
                            catseg_stream_t stream);
int catseg_softmax_rows_bwd(const float* y, const float* dy, float* dx, long long rows, int K, int ld,
                            float scale, catseg_stream_t stream);

/* ---- losses ------------------------------------------------------------------------------- */
/* The per-pixel kernels of this section and catseg_confusion_matrix stage 256 pixel rows of K | 1 floats in LDS: with S = 1024 * (K | 1)
 * bytes, Lovasz forward and cross entropy ask for S (+ up to 1 KB static), OHEM for S + 8 KB, Lovasz backward for 2 S + 1 KB, the
 * confusion matrix for S + 4 K^2.  That passes the 64 KB a block gets by default from K = 32 (Lovasz backward), K = 54 (confusion
 * matrix), K = 56 (OHEM), K = 64 (Lovasz forward, cross entropy).  Every entry point accepts 1 <= K <= 64: beyond 64 KB it opts in
 * (hipFuncSetAttribute) up to the device's opt-in maximum, which catseg_lds_limits reports (an MI355X reports 163840 bytes, by default and after opting in: every K <= 64 is served,
 * Lovasz backward at K = 64 with 131 KB = one block per CU).  On a device whose maximum is smaller the call returns CATSEG_EINVAL with a
 * message BEFORE launching anything: outputs and workspace are untouched. */
int catseg_lds_limits(int* per_block, int* per_block_optin); /* bytes of LDS per block: by default / after opting in */
/* LovaszSoftmax.forward (losses/LovaszSoftmax.py:19-61, per_image=False, classes 'present',
 * nothing ignored) fused with its autograd backward.  logits [P][K] (ld = K, compact),
 * labels int64 [P].  loss_out[0] = loss; dlogits (may be NULL) = weight * dloss/dlogits. */
size_t catseg_lovasz_workspace(long long P, int K);
int catseg_lovasz_softmax(const float* logits, const int64_t* labels, long long P, int K, float weight,
                          float* loss_out, float* dlogits, int accumulate_dlogits, void* workspace,
                          size_t workspace_bytes, catseg_stream_t stream);
/* the same pipeline in two calls around autograd (losses/LovaszSoftmax.py:19-32 + its backward): _fwd leaves d loss / d prob and the class
   counts in `workspace` (catseg_lovasz_workspace bytes, kept untouched by the caller together with `logits`) when want_grad != 0; _bwd writes
   (d loss / d logit) * upstream, upstream = a DEVICE scalar (autograd's grad_output; null = 1): no separate scaling pass over the gradient */
int catseg_lovasz_softmax_fwd(const float* logits, const int64_t* labels, long long P, int K, float weight, float* loss_out,
                              int want_grad, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
int catseg_lovasz_softmax_bwd(const float* logits, long long P, int K, float weight, const float* upstream, float* dlogits,
                              int accumulate_dlogits, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* nn.CrossEntropyLoss(ignore_index) (losses/LossWrapper.py:17-24) fused with backward.  A label outside [0, K) is IGNORED whether or not it
 * equals ignore_index (torch raises on such a label; here it contributes neither to the sum nor to the count, and its gradient row is 0).
 * No valid pixel at all: loss = NaN (0 / 0, as torch), dlogits all zero. */
size_t catseg_ce_workspace(long long P);
int catseg_cross_entropy(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index,
                         float weight, float* loss_out, float* dlogits, void* workspace,
                         size_t workspace_bytes, catseg_stream_t stream);
/* OhemCrossEntropy.forward (losses/OhemCrossEntropy.py:22-39) fused with backward: mean CE over the non-ignored
 * pixels whose target-class probability is < max(thresh, k-th smallest probability), k = min(min_kept, n - 1).
 * The k-th order statistic is found by a 3-pass radix select on device (no sort, no host sync). */
size_t catseg_ohem_workspace(long long P);
int catseg_ohem_cross_entropy(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index,
                              float thresh, long long min_kept, float weight, float* loss_out, float* dlogits,
                              void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* SoftIoU.forward / GenDiceLoss.forward (losses/SoftIoU.py, losses/GenDiceLoss.py) in two calls around autograd.  Labels 0 <= y < K have
 * one-hot column y; y == ignore_index (>= 0; -1 = none) is a zero one-hot row whose probabilities still enter the sums; any other label
 * is invalid: the pixel is dropped and counted in invalid_out[0] (int64, device).  kind 0 = SoftIoU, 1 = GenDice; naive != 0: the mean
 * over all K classes (nan where 0 / 0), else over the classes whose union / weighted divisor is non-zero.  weight_mode (GenDice):
 * 0 none, 1 'auto' (1 / n_c^2, 1 where n_c = 0), 2 = weights (HOST array of K floats).  _fwd writes loss_out[0] and coef (device,
 * 128 floats, owned by the caller until _bwd): d loss / d p_pc = coef[c] [y_p = c] + coef[64 + c].  _bwd writes
 * dlogits = (d loss / d logits) * upstream[0] (a DEVICE scalar; null = 1). */
size_t catseg_overlap_workspace(long long P, int K);
int catseg_overlap_fwd(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index, int kind, int naive,
                       int weight_mode, const float* weights, float* loss_out, float* coef, long long* invalid_out,
                       void* workspace, size_t workspace_bytes, catseg_stream_t stream);
int catseg_overlap_bwd(const float* logits, const int64_t* labels, long long P, int K, long long ignore_index, const float* coef,
                       const float* upstream, float* dlogits, catseg_stream_t stream);
/* FocalLoss.forward (losses/FocalLoss.py): mean over all P pixels of -alpha_y (1 - p_y)^gamma log p_y, p_y from the unweighted
 * log-softmax; alpha = HOST array of K floats or null.  Labels outside [0, K) add zero loss and zero gradient (and stay in the
 * denominator); their number goes to invalid_out[0] (int64, device).  _bwd: dlogits = (d loss / d logits) * upstream[0] (device; null = 1). */
size_t catseg_focal_workspace(long long P);
int catseg_focal_fwd(const float* logits, const int64_t* labels, long long P, int K, float gamma, const float* alpha, float* loss_out,
                     long long* invalid_out, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
int catseg_focal_bwd(const float* logits, const int64_t* labels, long long P, int K, float gamma, const float* alpha,
                     const float* upstream, float* dlogits, catseg_stream_t stream);

/* ---- input side -------------------------------------------------------------- */
/* Dataset_from_df.__getitem__ + its deterministic transforms (datasets/Dataset_from_df.py:31-69;
 * remap_mask utils/utils.py:23-47; FlipNP / PadNP utils/transforms.py:222-240, 8-20; ToTensor / Normalize
 * utils/utils.py:440-447) for a whole batch on device.
 *   img u8 [B][H][W][3] RGB, lbl u8 [B][H][W] raw ids; lut u8[256] (NULL = identity);
 *   flips int32 [B] (NULL = none): bit 0 = horizontal, bit 1 = vertical, applied before the padding;
 *   rows are reflect-padded (np.pad 'reflect') by pad_top / pad_bottom; x = u8 / 255, then (x - mean) / std if given.
 *   Outputs: x_nchw f32 [B][3][H'][W] and / or x_nhwc4 f32 [B][H'][W][4] (4th channel 0: the stem layout),
 *   labels int64 [B][H'][W], H' = H + pad_top + pad_bottom.  Either side (image / label) may be NULL. */
int catseg_ingest_u8(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, const int32_t* flips,
                     int pad_top, int pad_bottom, const float* mean, const float* stdv, float* x_nchw, float* x_nhwc4,
                     int64_t* labels, catseg_stream_t stream);

/* The same with the geometric augmentations of the reference's `transforms` list fused in (csrc/warp.hip): after remap and flip,
 * AffineNP(crop_to_fit=False) warps the frame onto an Hc x Wc canvas (the reference: 2H x 2W; utils/transforms.py:38-61), CropNP keeps an
 * Hw x Ww window of the canvas at a per-image origin (:270-303), PadNP reflect-pads the rows when nothing was cropped (utils/utils.py:394-401).
 * Only the window's pixels are computed: one gather of up to four source pixels each.
 *   minv: DEVICE double [B][6], rows 0 and 1 of the inverse of the frame -> canvas matrix (NULL = identity, then the canvas is the frame);
 *   source coordinates in 1/32 pixel: X = rint(((m00 x + m01 y) + m02) * 32) in fp64 without contraction, clamped to int32; bilinear weights
 *   are integers over 1024, neighbours outside the frame count as 0 (constant border); colour = the weighted sum rounded half to even;
 *   label = the remapped label with the largest summed weight, ties to the smaller id, 0 where no neighbour is inside the frame;
 *   origin: DEVICE int32 [B][2] = (row, column) of the window in the canvas (NULL = (0, 0)); window pixels outside the canvas are zeros;
 *   pad_top / pad_bottom reflect the canvas rows and need Hw == Hc.  No source read is unguarded, whatever minv / origin hold.
 *   Outputs (any combination): x_nchw f32 [B][3][H'][Ww], x_nhwc4 f32 [B][H'][Ww][4], x_u8 u8 [B][H'][Ww][3] (the warped frame before
 *   ToTensor: the input of the blur / colour jitter kernels below), labels int64 [B][H'][Ww]; H' = Hw + pad_top + pad_bottom. */
int catseg_ingest_warp_u8(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, const int32_t* flips,
                          const double* minv, int Hc, int Wc, const int32_t* origin, int Hw, int Ww, int pad_top, int pad_bottom,
                          const float* mean, const float* stdv, float* x_nchw, float* x_nhwc4, uint8_t* x_u8, int64_t* labels,
                          catseg_stream_t stream);

/* PIL-based training augmentations on uint8 NHWC batches [B][H][W][3], bit-exact with Pillow (csrc/augment.hip; reference call
 * sites utils/utils.py:412-417, utils/transforms.py:242-251):
 *   catseg_aug_pad_flip_u8: FlipNP (bit 0 horizontal, bit 1 vertical) + PadNP reflect rows, uint8 -> uint8 (what precedes ToPILImage);
 *   catseg_aug_box_blur: ONE extended box-blur pass along axis (0 = H, 1 = W) with per-image (radius, ww, fw) of BoxBlur.c
 *     (radius[b] < 0: copy); ImageFilter.GaussianBlur(r) = 3 passes along W, then 3 along H, box radius from r (host side);
 *   catseg_aug_color_op: ONE operation of torchvision ColorJitter per image, in place: op[b] = 0 brightness, 1 contrast,
 *     2 saturation (factor[b] = the enhance factor), 3 hue (factor[b] = the integer H shift 0..255), < 0 none; workspace >= 8 B bytes.
 *     The workspace size selects the pipeline (op[] is device memory; the host cannot see which codes a call carries):
 *       workspace_bytes <  CATSEG_AUG_WS_LUT(B) = roundup(8 B, 256) + 3072 B: the two ColorJitter launches; codes >= 4 are not served;
 *       workspace_bytes >= CATSEG_AUG_WS_LUT(B): the extended pipeline (a 16-byte aligned workspace, H W < 2^31).  Codes 0 ... 3 give
 *         the same bits, and 4 = ImageOps.autocontrast (cutoff 0), 5 = ImageOps.equalize, both per band (factor unused),
 *         6 = ImageOps.posterize (factor[b] = bits, 1 ... 8), 7 = ImageOps.solarize (factor[b] = the threshold); codes < 0 or > 8
 *         leave the image unchanged.  Layout: [B] 64-bit luma sums, at roundup(8 B, 256) [B][3][256] 32-bit histogram counters;
 *       workspace_bytes >= CATSEG_AUG_WS_FULL(B, H, W) = CATSEG_AUG_WS_LUT(B) + 3 B H W: also 8 = ImageEnhance.Sharpness (factor[b] =
 *         the enhance factor), which reads the neighbours from a copy of the frame at CATSEG_AUG_WS_LUT(B); below that size an
 *         image with code 8 stays unchanged.  No byte at or behind workspace_bytes is written. */
#define CATSEG_AUG_WS_LUT(B) ((((size_t)(B) * 8 + 255) / 256 * 256) + (size_t)(B) * 3072)
#define CATSEG_AUG_WS_FULL(B, H, W) (CATSEG_AUG_WS_LUT(B) + (size_t)(B) * (size_t)(H) * (size_t)(W) * 3)
int catseg_aug_pad_flip_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, int C, const int32_t* flips, int pad_top,
                           int pad_bottom, catseg_stream_t stream);
int catseg_aug_box_blur(const uint8_t* in, uint8_t* out, int B, int H, int W, int axis, const int32_t* radius, const uint32_t* ww,
                        const uint32_t* fw, catseg_stream_t stream);
int catseg_aug_color_op(uint8_t* img, int B, int H, int W, const int32_t* op, const float* factor, void* workspace,
                        size_t workspace_bytes, catseg_stream_t stream);

/* Test-time augmentation plumbing (managers/BaseManager.py:652-660 wraps the model in ttach
 * HorizontalFlip x Scale(0.75, 1, 1.5, 1.75, 2), merge 'mean'; ttach is an un-vendored dependency: its Scale is
 * F.interpolate(mode='nearest', size=(int(h*s), int(w*s)))).  NHWC nearest resize:
 *   dst[b][y][x][:] (+)= src[b][sy][sx][:], sy = min(floor(y * (float)Hi / Ho), Hi - 1), sx likewise;
 *   flip 1: the source is flipped horizontally first (image augmentation), flip 2: the result is flipped
 *   (mask de-augmentation); accumulate: add into dst; divide_by != 0: the stored value is divided by it
 *   (the 'mean' merge on the last accumulation). */
int catseg_resize_nearest(const float* src, int lds, float* dst, int ldd, int B, int Hi, int Wi, int Ho, int Wo, int C, int flip,
                          int accumulate, float divide_by, catseg_stream_t stream);

/* ---- ensemble merge (models/Ensemble.py:57-74: nn.Softmax2d per member, torch.stack, torch.mean; BaseManager.py:671-674: argmax) ---- */
/* One launch for M members' NHWC logits [P][ld[m]] (ld[m] >= K; rows up to 68 floats are staged through LDS with 16-byte loads, wider ones --
 * views into a concat buffer -- are read per lane).  logits, ld: HOST arrays of M device pointers / leading dimensions; the kernel receives
 * them by value (no device-side table, no copy: the launch can be captured).  1 <= M <= 8, 1 <= K <= 64.
 *   p_m = softmax(logits_m[pixel][0:K]) with the row maximum subtracted, fp32;
 *   mode 0 (mean): (p_0 + p_1 + ... + p_{M-1}) / M, summed in member order, a true division; mode 1 (max): element-wise maximum;
 *   probs (may be NULL): merged values [P][ld_probs], K <= ld_probs <= 68, columns [K, ld_probs) WRITTEN ZERO;
 *   labels (may be NULL): int64 [P], the FIRST maximal merged class (torch.argmax, the rule of catseg_confusion_matrix), taken from the very
 *   fp32 values stored in probs: labels == argmax(probs) bit for bit.
 * HBM traffic (M + 1) P K 4 bytes + 8 P.  LDS: 1024 * (widest staged row | 1) bytes, opt-in beyond 64 KB as the loss kernels do.
 * CATSEG_EINVAL before anything is launched: M or K out of range, a NULL member, ld[m] < K, bad ld_probs, both outputs NULL. */
int catseg_ensemble_merge(const float* const* logits, const int* ld, int M, long long P, int K, int mode, float* probs, int ld_probs,
                          int64_t* labels, catseg_stream_t stream);

/* ---- egress: network output -> label maps and coloured uint8 frames (managers/BaseManager.py:690-741 demo_infer; utils/utils.py:50-142,
 * 202-211 mask_from_network / mask_to_colormap / to_comb_image; utils/torch_utils.py:7-21 clipped_argmax) ---- */
/* One launch per batch, every argument by value (no device-side pointer table: the launch can be captured).
 *   rows: fp32 NHWC [B][H][W] pixels of ld >= K floats (out.permute(0, 2, 3, 1) of any model's output); 1 <= K <= 64.  Rows of up to 68
 *     floats are staged through LDS with 16-byte loads, wider ones (views into a concat buffer) are read per lane; columns [K, ld) are
 *     never taken for classes.
 *   The predicted class is the FIRST maximal value of the row (torch.argmax; the rule of catseg_confusion_matrix and
 *     catseg_ensemble_merge).
 *   values_are_probs 0: rows are logits, the score of a pixel is 1 / sum_k exp(x_k - max) in fp32 (the maximum of nn.Softmax2d);
 *     1: rows are probabilities (catseg_ensemble_merge's output), the score is the maximum itself.
 *   threshold > 0: a pixel whose score is < threshold takes network id ignore_value (in [0, 255]) instead (clipped_argmax);
 *     threshold <= 0: no score, no exp is evaluated.
 *   crop_top, crop_bottom: rows of every image left out of the outputs (the inverse of PadNP(ver=(2, 2))): H' = H - crop_top - crop_bottom;
 *     cropped rows are never read, in rows, frame or target.
 *   lut: DEVICE uint8[256] network id -> dataset id (mask_from_network: the ignore id -> 255 for experiments 2 and 3); NULL = identity.
 *   palette: DEVICE uint8[256][3], the colour of each dataset id ALREADY in the output channel order; unmapped ids 0.
 *   frame (may be NULL): fp32 image [B][3][H][W], or [B][H][W][4] with frame_nhwc4 != 0; mean / stdv (HOST float[3], both or neither):
 *     x * std + mean first (un_normalise, utils/utils.py:453: a rounded multiply, then a rounded add).  The byte is rintf(x * 255.f), ties
 *     to even (np.round), clamped to [0, 255]; bgr != 0 reverses the channel order.
 *   rows may be NULL when only the frame / target panels are wanted (mask_to_colormap of a label map): no prediction panel, no labels.
 *   target (may be NULL): int64 [B][H][W] network-id ground truth, coloured through the same lut and palette (ids outside [0, 255]: black).
 * Outputs (each may be NULL, not all):
 *   labels_i64 [B][H'][W]: network ids after clipping, before lut (what argmax / clipped_argmax return);
 *   labels_u8  [B][H'][W]: dataset ids, after lut;
 *   canvas uint8 [B][H'][n_panels * W][3]: the panels that are present in the fixed order frame | target | prediction
 *     (all three, RGB = to_comb_image; frame + prediction, BGR = the demo; prediction only, BGR = 'miccai_demo').
 * With W % 4 == 0 (and 4-byte aligned byte outputs, a 16-byte aligned frame) a lane owns four consecutive pixels of one output row and
 * stores 12 canvas bytes as three dwords, 4 label bytes as one; otherwise (unaligned canvas rows) bytes.  HBM traffic B H' W (4 ld + the
 * output bytes) + the panels' inputs.  LDS: 1024 * (ld | 1) + 2048 bytes.
 * CATSEG_EINVAL before anything is launched: K out of range, ld < K, crop_top + crop_bottom >= H, all outputs NULL, a canvas without a
 * palette, threshold >= 1, ignore_value outside [0, 255] with a threshold, frame / target without a canvas, mean without std. */
int catseg_egress_u8(const float* rows, int ld, int B, int H, int W, int K, int values_are_probs, int crop_top, int crop_bottom,
                     float threshold, int ignore_value, const uint8_t* lut, const uint8_t* palette, const float* frame, int frame_nhwc4,
                     const float* mean, const float* stdv, int bgr, const int64_t* target, int64_t* labels_i64, uint8_t* labels_u8,
                     uint8_t* canvas, catseg_stream_t stream);

/* ---- metrics / optimiser ------------------------------------------------------------------ */
/* t_get_confusion_matrix (utils/torch_utils.py:221-241): cm[pred*K + gt] += 1 (int32, K x K),
 * labels outside [0, K) (>= K or negative) are dropped; pred = the FIRST maximal logit of the row (torch.argmax); cm is accumulated
 * into (zero it first for a fresh matrix). */
int catseg_confusion_matrix(const float* logits, const int64_t* labels, long long P, int K, int32_t* cm,
                            catseg_stream_t stream);
/* torch.optim.Adam(lr) step over a flat parameter buffer (managers/BaseManager.py:441): g' = grad_scale * g, m = beta1 m + (1 - beta1) g',
 * v = beta2 v + (1 - beta2) g'^2, p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  lr, beta1, beta2, eps are the
 * float values passed (1 - beta is formed from the float: exact), the bias corrections are formed in double.  p, g, m, v 16-byte aligned
 * (CATSEG_EINVAL otherwise, nothing written); any n >= 1. */
int catseg_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                     float beta2, float eps, int step, float grad_scale, catseg_stream_t stream);
/* the same step with its step-dependent scalars in DEVICE memory -- hyper = {lr, 1 - beta1^step, sqrt(1 - beta2^step), grad_scale}, the
   values catseg_adam_hyper (host, no GPU call) computes exactly as catseg_adam_step does -- so that a launch captured in a hipGraph
   (the whole training step of managers/OCRNet_Manager.py:80-90 replayed as one graph) follows the learning-rate schedule and the bias
   correction of torch.optim.Adam from step to step; bit-identical to catseg_adam_step for equal values */
void catseg_adam_hyper(float lr, float beta1, float beta2, int step, float grad_scale, float* hyper4);
int catseg_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, const float* hyper, float beta1,
                         float beta2, float eps, catseg_stream_t stream);

/* ---- pointwise (1 x 1, stride 1) convolutions in split precision with the split in registers (csrc/pconv1.hip) ----
   Replaces the ATen 1 x 1 conv2d calls (forward, and their autograd backward) of the stage-1 bottlenecks (models/HRNetv2.py:68-106), of the
   object-attention block (models/OCR.py:186-235: f_pixel / f_up) and of the HRNet fuse layers (models/HRNetv2.py:237-261) -- layers too
   small for the blocked-plane kernels above, HBM-bound GEMMs with K = 64 ... 512 -- and, since round 6, of the 1 x 1 layers of torchvision's
   ResNet bottlenecks up to 2048 output columns (models/OCR.py:58-61: 64 <-> 256, 128 <-> 512, 256 <-> 1024 at stride 8; catseg_pconv1_supported:
   32 <= N <= 2048, 32 <= K <= 8160, K % 8 == 0).  The activation operand is the fp32 NHWC tensor itself
   plus the amax record its producer left (CATSEG_AMAX_RECORD_BYTES); the weight operand is a pre-split image.
   catseg_pconv1_prep_batch: entries = DEVICE array of n 64-byte records {int64 weight offset (floats, relative to flat), int64 image offset
   (bytes, relative to wimg_base), int32 O, I, kh, kw, transposed, ky0, kys, nky, kx0, kxs, nkx, pad} (a 1 x 1 layer: kh = kw = nky = nkx =
   kys = kxs = 1, ky0 = kx0 = 0); records = n x {uint32 bits of max|w|, int32 exponent} (DEVICE).
   catseg_pconv1: y[M][N] (+)= x[M][K] . B^T (+ bias); B = image of (N, K) = the layer's [O][I] weights (forward: N = O, K = I) or, with
   transposed != 0 at preparation, their transpose (backward-data: N = I, K = O).  bn_part as in catseg_conv2d_fwd.
   catseg_pconv1_wgrad: dw[Cout][Cin] = dy^T . x over P pixels (slabs + fixed-order sum: deterministic). */
int catseg_pconv1_supported(int N, int K);
size_t catseg_pconv1_wimg_bytes(int N, int K);
int catseg_pconv1_prep_batch(const float* flat, int n, const void* entries, void* wimg_base, void* records, catseg_stream_t stream);
int catseg_pconv1(long long M, int N, int K, const float* x, int ldx, const void* x_rec, const void* wimg, const void* w_rec,
                  const float* bias, float* y, int ldy, int accumulate, float* bn_part, size_t bn_part_floats, int* tile_rows,
                  int* n_tiles, catseg_stream_t stream);
int catseg_pconv1_wgrad_supported(int Cout, int Cin);
size_t catseg_pconv1_wgrad_workspace(long long P, int Cout, int Cin);
int catseg_pconv1_wgrad(long long P, int Cout, int Cin, const float* dy, int lddy, const void* dy_rec, const float* x, int ldx,
                        const void* x_rec, float* dw, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
/* The same kernels as "gather" launches for dense convolutions with kh x kw taps, stride 1 / 2, padding, dilation (stride 1) whose input
   carries an amax record: the 3 x 3 / stride 2 layers of the HRNet fuse chains and transitions (models/HRNetv2.py:176-198,237-261: ATen
   conv2d + its autograd backward), the 256 -> 48 transition, the stem's second convolution.  Weight images through
   catseg_pconv1_prep_batch with the 64-byte entries catseg_gconv_entries fills (host memory; 1 entry forward, stride^2 entries -- one
   per input-pixel parity class, catseg_gconv_class_bytes apart -- backward-data).  Results as the fp32 kernels' to split-precision accuracy. */
int catseg_gconv_supported(const catseg_conv_desc* d);
size_t catseg_gconv_class_bytes(const catseg_conv_desc* d);
size_t catseg_gconv_wimg_bytes(const catseg_conv_desc* d, int backward_data);
int catseg_gconv_entries(const catseg_conv_desc* d, int backward_data, long long w_off, long long img_off, void* entries_out);
int catseg_gconv_fwd(const catseg_conv_desc* d, const float* x, const void* x_rec, const void* wimg, const void* w_rec,
                     const float* bias, float* y, float* bn_part, size_t bn_part_floats, int* tile_rows, int* n_tiles,
                     catseg_stream_t stream);
int catseg_gconv_bwd_data(const catseg_conv_desc* d, const float* dy, const void* dy_rec, const void* wimg_classes, const void* w_rec,
                          float* dx, int accumulate, catseg_stream_t stream);
int catseg_gconv_wgrad_supported(const catseg_conv_desc* d);
size_t catseg_gconv_wgrad_workspace(const catseg_conv_desc* d);
int catseg_gconv_bwd_weight(const catseg_conv_desc* d, const float* dy, const void* dy_rec, const float* x, const void* x_rec,
                            float* dw, void* workspace, size_t workspace_bytes, catseg_stream_t stream);

/* ---- PointRend, eval-mode refinement (models/PointRend.py:74-90 of the reference: F.interpolate x 2, calculate_uncertainty, torch.topk,
 * five point_sample = F.grid_sample calls, torch.cat, scatter_; csrc/pointrend.hip).  The point head's layers are 1 x 1 convolutions over
 * the N k points and run through catseg_conv2d_fwd; the upsampling is the catseg_bilinear_fwd launch.  Nothing here synchronises with the host or allocates: a
 * refinement step can be captured in a hipGraph.
 *   uncertainty: uncertainty[p] = second-largest - largest of y[p ldy + 0 .. K) (<= 0; equal logits give 0), p < pixels: the rows the resize
 *               launch (catseg_bilinear_fwd, align_corners = 0, x 2) stored.  Columns K .. ldy are never read.  K >= 2 (one class has no
 *               second logit: CATSEG_EINVAL), ldy >= K.
 *   topk:       idx [N, k] (int32, ascending) = the k largest of uncertainty [N, n] per image; among equal values the LOWER index is
 *               taken, -0.0 equals +0.0; deterministic.  1 <= k <= n < 2^31 (k = n selects everything), N <= 65535; workspace of
 *               the size the workspace query returns, 16-byte aligned (CATSEG_EWORKSPACE otherwise).
 *   gather:     per image b and point p: the centre of cell idx[b, p] of the h x w grid, x = (1/w)/2 + (idx % w) (1/w), y likewise, every
 *               operation rounded to fp32 as utils/pointrend_utils.py:146-147 does; from every source s (NHWC [N, H_s, W_s, C_s], pixel
 *               stride ld_s) F.grid_sample(bilinear, align_corners = False, ZERO padding) at 2 (x, y) - 1; out[b k + p] = the sources'
 *               blocks side by side, each C_s rounded up to 4 columns wide, the pad columns zero.  The LAST source's block is also
 *               written to extra[q] + (b k + p) extra_ld[q] + extra_off[q], q < n_extra (the coarse logits that every layer of the
 *               point head concatenates to its input).  ld_s >= C_s; a source whose pixels are 16-byte aligned rows of at least C_s rounded
 *               up to 4 floats is read with 16-byte loads, any other (dense K-class logits) one channel per lane; out and extra 16-byte aligned.
 *   scatter:    seg[b, idx[b, p], 0:K] = rows[b k + p, 0:K] (seg: [N, hw] pixels of ld_seg floats). */
typedef struct {
  const float* src[5]; int ld[5], H[5], W[5], C[5];
  int n_sources;                 /* 1 .. 5 */
  const int* idx;                /* [N, k] pixel indices of the h x w grid */
  int N, k, h, w;
  float* out; int ld_out;        /* [N k] rows */
  float* extra[4]; int extra_ld[4], extra_off[4];
  int n_extra;                   /* 0 .. 4 */
} catseg_pointrend_gather_desc;
int catseg_pointrend_uncertainty(const float* y, int ldy, float* uncertainty, long long pixels, int K, catseg_stream_t stream);
size_t catseg_pointrend_topk_workspace(int N, long long n);
int catseg_pointrend_topk(const float* uncertainty, int N, long long n, int k, int* idx, void* workspace, size_t workspace_bytes,
                          catseg_stream_t stream);
int catseg_pointrend_gather(const catseg_pointrend_gather_desc* d, catseg_stream_t stream);
int catseg_pointrend_scatter(const float* rows, int ld_rows, const int* idx, int N, int k, long long hw, float* seg, int ld_seg, int K,
                             catseg_stream_t stream);

/* ---- PointRend, train-mode forward and backward (models/PointRend.py:43-73, utils/pointrend_utils.py:65-116 and
 * managers/EncDec_Manager.py:158-177 of the reference; csrc/pointrend_train.hip, catseg_pointrend_gather_at in csrc/pointrend.hip).  Points are
 * (x, y) pairs in [0, 1]^2, [N, P, 2] fp32.  No entry point synchronises with the host, allocates or touches host memory: all are capturable.
 *   draw:        out [N, M, 2] uniforms in [0, 1).  state: 16 bytes of device memory {seed lo, seed hi, layer | rank << 16, draw counter},
 *                16-byte aligned.  Float i takes word i & 3 of philox4x32_10(counter = (i >> 2, draw, 1, layer | rank << 16), key = (seed lo,
 *                seed hi)) -- counter word 2 is 1 where catseg_dropout2d_mask has 0 -- u = (word >> 8) 2^-24; the launch advances the draw
 *                counter by one.  fixed != NULL (a test knob): out = fixed, the state is neither read nor written.
 *   point_uncertainty: uncertainty[b, m] = second-largest - largest over the K real columns of F.grid_sample(coarse, 2 coords - 1; bilinear,
 *                align_corners = False, ZERO padding); coarse NHWC [N, H, W] pixels of ld floats.  K >= 2.  No [N, K, M] intermediate.
 *   gather_at:   catseg_pointrend_gather with the point read from coords [N, k, 2] instead of derived from a cell index (idx, h, w of the
 *                descriptor are not read); the same sweep, the same bits for the same point.
 *   compose:     coords [N, P, 2] = cand[b, sel[b, 0 .. kb)] (sel: int32 indices into the M candidates of image b, as catseg_pointrend_topk
 *                writes them), then rest [N, P - kb, 2]; pix [N, P] (int32) = round(y (h - 1)) w + round(x (w - 1)), every operation rounded
 *                to fp32, round half to even (models/PointRend.py:56-57; h w < 2^24; a result outside [0, h w) is stored as -1);
 *                labels [N, P] (int64) = F.grid_sample(lbl [N, Hl, Wl] int64, mode = 'nearest', zero padding): a tap outside the map gives 0,
 *                every stored value (the ignore class too) passes through.  lbl and labels may both be NULL.
 *   gather_bwd:  the adjoint of gather_at: dst_s[b, tap pixel, 0:C_s] (+)= weight * dx[b P + p, block s] over the four bilinear taps of every
 *                point; a tap outside the map is dropped.  accumulate[s] == 0: the WHOLE destination [N, H_s, W_s] x ld_s floats is zeroed
 *                first, so pixels no tap touches are 0; != 0: they keep their values.  No floating-point atomics: a pixel's sum is formed by
 *                one wave over its taps in ascending tap number 4 p + corner (nw, ne, sw, se); two launches give the same bits.
 *                Destinations: 16-byte aligned, ld_s % 4 == 0, ld_s >= C_s rounded up to 4 (the pad columns receive 0).  P <= 3584.
 *   scatter_last: seg[b, pix[b, p], 0:K] = rows[b P + p, 0:K]; among the points of one pixel the HIGHEST p writes (torch's scatter_ on
 *                the CPU); pix outside [0, hw) writes nothing.  P <= 14336.
 *   scatter_bwd: drows[b P + p, 0:K] (+)= dseg[b, pix[b, p], 0:K] for EVERY p (each duplicate receives its pixel's gradient), then
 *                dseg[b, pix[b, p], 0:K] = 0 (the tensor the points were scattered into receives no gradient there). */
typedef struct {
  float* dst[5]; int ld[5], H[5], W[5], C[5], accumulate[5];
  int n_sources;                 /* 1 .. 5 */
  const float* coords;           /* [N, P, 2] */
  int N, P;
  const float* dx; int ld_dx;    /* [N P] rows: the sources' blocks side by side, each C_s rounded up to 4 columns wide */
} catseg_pointrend_gather_bwd_desc;
int catseg_pointrend_draw(void* state, const float* fixed, int N, int M, float* out, catseg_stream_t stream);
int catseg_pointrend_point_uncertainty(const float* coarse, int ld, int N, int H, int W, int K, const float* coords, int M, float* uncertainty,
                                       catseg_stream_t stream);
int catseg_pointrend_gather_at(const catseg_pointrend_gather_desc* d, const float* coords, catseg_stream_t stream);
int catseg_pointrend_compose(const float* cand, int M, const int* sel, int kb, const float* rest, int N, int P, int h, int w, const long long* lbl,
                             int Hl, int Wl, float* coords, int* pix, long long* labels, catseg_stream_t stream);
int catseg_pointrend_gather_bwd(const catseg_pointrend_gather_bwd_desc* d, catseg_stream_t stream);
int catseg_pointrend_scatter_last(const float* rows, int ld_rows, const int* pix, int N, int P, long long hw, float* seg, int ld_seg, int K,
                                  catseg_stream_t stream);
int catseg_pointrend_scatter_bwd(float* dseg, int ld_seg, const int* pix, int N, int P, long long hw, float* drows, int ld_rows, int K, int accumulate,
                                 catseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_H */
