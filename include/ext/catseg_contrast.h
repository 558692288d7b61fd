/*
 * libcatseg_hip.so -- feature header: the dense contrastive loss over a fixed set of anchor slots (losses.DenseContrastiveLoss),
 * csrc/contrast.hip.  The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok,
 * catseg_last_error() gives the message, which starts with the function's name).  Every launch can be captured into a hipGraph.  No
 * floating-point atomics: two launches on the same inputs write the same bits.  r4(n) = n rounded up to a multiple of 4.
 *
 * The anchor set: A = K * M slots, slot a = c * M + m belongs to class c.  The low-resolution label of pixel q = (b h + i) w + j of the
 * [B, h, w] feature map is labels[b, (i H) / h, (j W) / w] (F.interpolate(mode = 'nearest')); a pixel is valid when 0 <= label < K.  The
 * pixels of class c are ranked in ascending q, n_c is their count.  n_c <= M: slot m < n_c takes rank m, the other slots are empty
 * (idx = -1, label = -1).  n_c > M: with b_m = (m n_c) / M the slot takes rank b_m + ((u24 (b_{m+1} - b_m)) >> 24), 64-bit integers.
 * u24: the top 24 bits of word a & 3 of philox4x32_10(counter = (a >> 2, draw, 2 = the anchors' stream, layer | rank << 16), key = seed)
 * with {seed lo, seed hi, layer | rank << 16, draw} the 16 bytes of `state`; the launch advances the draw counter by one.  With fixed_u
 * (A ints, the low 24 bits are used) or eval != 0 (u24 = 2^23) the state is neither read nor written and may be NULL.
 *
 * catseg_contrast_pick_workspace -- bytes of workspace for catseg_contrast_pick.
 * catseg_contrast_pick -- labels: DEVICE int64 [B, H, W].  Outputs, all DEVICE int32: idx [A] (the pixel q of the slot or -1), label [A]
 *   (c or -1), n_pos [1] = sum over classes of [min(n_c, M) >= 2] min(n_c, M), the number of anchors that have a positive.  Three launches:
 *   per chunk of 256 pixels the class counts (block 0 also moves the draw counter), per class an exclusive scan over the chunks, per
 *   slot a binary search over the scanned counts and an in-chunk select by ballot and popcount.
 * catseg_contrast_gather -- feat: DEVICE float rows of pitch ld >= d, row q = pixel q.  Z [A, r4(d)]: z_a = f_a / max(|f_a|, eps), zeros in
 *   empty rows and in the pad columns.  inv_norm [A]: 1 / |f_a|; -(1 / eps) for a row shorter than eps (the sign tells the adjoint that
 *   the norm was clamped); 0 for an empty slot.  16-byte accesses where d, ld are multiples of 4 and feat is 16-byte aligned.
 * catseg_contrast_rows -- S: DEVICE float [A, lds], lds >= r4(A), row i holds z_i . z_j in columns [0, A); s_ij = S_ij inv_tau.  Pairs are
 *   i != j with both slots filled, P(i) the same-label j, w_ij = 1 for the same label, else Wt[y_i K + y_j] (Wt: DEVICE float [K, K]).
 *   ell[i] = -(1 / |P(i)|) sum_P s_ip + log sum_{j != i} w_ij exp(s_ij) for a row with a positive, else 0.  The row of S is overwritten with
 *   G_ij = (w_ij exp(s_ij) / D_i - [j in P(i)] / |P(i)|) / max(n_pos, 1) for rows with a positive; the diagonal, empty rows and columns,
 *   rows without a positive and the pad columns [A, r4(A)) are written as +0.  One 256-thread block per row, the row in registers
 *   (A <= 8192).  K floats of dynamic LDS hold the row Wt[y_i, :].
 * catseg_contrast_finalize -- loss[0] = (float)(sum_i ell[i] / max(n_pos, 1)), the sum in fp64 in a fixed order.
 * catseg_contrast_scatter_bwd -- dfeat: DEVICE float [n_pix, d] dense; every element is written: zero, but for the pixel idx[a] of a filled
 *   slot, which receives (v - (v . z_a) z_a) |inv_norm[a]| with v = dZ[a, :] g[0] inv_tau (inv_norm[a] < 0: v |inv_norm[a]|, the clamped
 *   norm carries no gradient).  dZ, Z: [A, ldz], ldz >= r4(d).  g: DEVICE float [1], the upstream gradient.  The indices of the filled
 *   slots are distinct (catseg_contrast_pick gives distinct ranks); an index outside [0, n_pix) is skipped.
 *
 * CATSEG_EINVAL before anything is launched: a NULL or misaligned pointer (4 bytes; state, Z, dZ, S: 16 bytes), a dimension <= 0,
 * K M > 8192, h > H or w > W (the nearest rule samples, it does not enlarge), B h w >= 2^31, ld < d, lds < r4(A), ldz < r4(d), a
 * workspace that is too small, eps <= 0, inv_tau <= 0.
 */
#ifndef CATSEG_CONTRAST_H
#define CATSEG_CONTRAST_H

#include "catseg.h"

#define CATSEG_CONTRAST_MAX_ANCHORS 8192
#define CATSEG_CONTRAST_CHUNK 256

#ifdef __cplusplus
extern "C" {
#endif

size_t catseg_contrast_pick_workspace(int B, int h, int w, int K);
int catseg_contrast_pick(const long long* labels, int B, int H, int W, int h, int w, int K, int M, void* state, const int* fixed_u,
                         int eval, int* idx, int* label, int* n_pos, void* workspace, size_t workspace_bytes, catseg_stream_t stream);
int catseg_contrast_gather(const float* feat, int ld, long long n_pix, int d, const int* idx, int A, float eps, float* Z, float* inv_norm,
                           catseg_stream_t stream);
int catseg_contrast_rows(float* S, int lds, int A, const int* label, const float* Wt, int K, float inv_tau, const int* n_pos, float* ell,
                         catseg_stream_t stream);
int catseg_contrast_finalize(const float* ell, int A, const int* n_pos, float* loss, catseg_stream_t stream);
int catseg_contrast_scatter_bwd(const float* dZ, const float* Z, int ldz, const float* inv_norm, const int* idx, int A, int d,
                                const float* g, float inv_tau, float* dfeat, long long n_pix, catseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
