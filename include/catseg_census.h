/*
 * libcatseg_hip.so -- feature header: the label census and the per-batch IoU average behind the class-aware train loaders
 * (adaptive batching, oversampling, weighted random; managers/BaseManager.py:198-229, 286-405 of the reference), csrc/census.hip.
 * The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok, catseg_last_error() gives
 * the message, which starts with the function's name).  Both launches can be captured into a hipGraph.
 *
 * catseg_label_census_u8 -- per-frame class pixel counts of raw uint8 label maps (what utils/data_class_analysis.py:get_class_numbers
 * of the reference computes offline with 36 np.sum(label == i) passes per frame):
 *   lbl:     DEVICE uint8 [B][H][W], frames H * W bytes apart; neither the base pointer nor a frame start needs any alignment;
 *   lut:     DEVICE uint8 [256] applied to every label before it is counted, or NULL = identity;
 *   nbins:   1..256; counts: DEVICE int64 [B][nbins + 1], 8-byte aligned;
 *   counts[b][v] = the pixels of frame b whose (table-mapped) value is v < nbins; counts[b][nbins] = every other pixel (the reference's
 *   "Unknown class found"), so that a row gains exactly H * W per launch;
 *   accumulate = 0 overwrites (a memset node in front of the kernel), accumulate = 1 adds in 64 bits to what is there.
 * Integers only: the result does not depend on the order of the additions, two launches give the same bits.  The label bytes are
 * read once, in 16-byte loads between the first and the last 16-byte boundary of each frame and bytewise outside; every sub-counter
 * (a wave's run in registers, the per-wave LDS histograms) is 32 bits wide and H * W < 2^31, so none can wrap; a block adds each
 * non-empty bin once to `counts` with a 64-bit integer atomic.  No workspace.
 * CATSEG_EINVAL before anything is launched: bad dims (B in 1..65535, H, W > 0, H * W < 2^31), nbins outside 1..256, a NULL lbl or
 * counts, counts not 8-byte aligned.
 *
 * catseg_iou_ema -- the per-class IoU of the batch that was added to a running confusion matrix since the last call, and its
 * exponential average (managers/OCRNet_Manager.py:108-117 of the reference), one block:
 *   cm_running: DEVICE int32 [K][K] (rows = prediction, columns = ground truth), cm_prev: DEVICE int32 [K][K], 1 <= K <= 256;
 *   batch = cm_running - cm_prev; then cm_prev = cm_running;
 *   per class c: d = batch[c][c], r = sum_i batch[i][c], s = sum_j batch[c][j] as INTEGERS, each converted to fp32 once;
 *   iou = d / fl(fl(r + s) - d), correctly rounded, 0/0 -> 0 (the reference's iou[iou != iou] = 0);
 *   iou_values[c] = fl(fl(w_old * iou_values[c]) + fl(w_new * iou)), no fused multiply-add; iou_batch[c] = iou unless NULL.
 * The host passes w_old = float32(1 - a), w_new = float32(a): what numpy evaluates for (1 - a) * values_f32 + a * iou_f32.
 * WHILE A BATCH HOLDS FEWER THAN 2^24 PIXELS every integer above is exact in fp32 and the launch reproduces the reference's
 * t_get_mean_iou(confusion_matrix, experiment, calculate_mean=False) and its update bit for bit; past that the reference itself sums
 * rounded fp32 values in an order of torch's choosing and only the integers here stay exact.
 * CATSEG_EINVAL: K outside 1..256, a NULL cm_running / cm_prev / iou_values, operands not 4-byte aligned, cm_prev == cm_running.
 */
#ifndef CATSEG_CENSUS_H
#define CATSEG_CENSUS_H

#include "catseg.h"

#ifdef __cplusplus
extern "C" {
#endif

int catseg_label_census_u8(const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, int nbins, int64_t* counts, int accumulate,
                           catseg_stream_t stream);
int catseg_iou_ema(const int32_t* cm_running, int32_t* cm_prev, int K, float w_old, float w_new, float* iou_values, float* iou_batch,
                   catseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
