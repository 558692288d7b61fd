/*
 * libcatseg_hip.so -- feature header: the frequency-weighted crop pick (CropNP with crop_mode 'freq', utils/transforms.py:282-293 of the
 * reference), csrc/cropfreq.hip.  The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok,
 * catseg_last_error() gives the message, which starts with the function's name).
 *
 * The reference draws the crop's upper-left corner from the pixels of a region of the (warped) label map with probability proportional to
 * 1 / (frequency of the pixel's class): random.choices over float64 weights.  Here the same pick is evaluated in integers, so that it does
 * not depend on the order of summation and runs in parallel:
 *   labels:  of the canvas pixels, exactly as catseg_ingest_warp_u8 computes them from lbl, lut, flips and minv (csrc/warp_label.h);
 *   region:  margin = px / 2; canvas rows [margin, Hc - margin), canvas columns [margin, min(Hc - margin, Wc)) (the reference slices the
 *            columns with the HEIGHT; numpy clips at the width), n = rows * columns pixels scanned row-major;
 *   wq:      DEVICE uint64 [256], the integer weight of every label value (entries past the last class: 0);
 *            max(wq) * n must stay below 2^62 (the caller's check: the sums are 64-bit);
 *   m53:     DEVICE uint64 [B], per frame m = floor(u * 2^53) of a uniform u in [0, 1);
 *   T = (m * total) >> 53 from the 128-bit product, total = the sum of wq[label] over the region;
 *   pick = the first pixel i whose inclusive running sum exceeds T, n - 1 if there is none (total = 0, or m >= 2^53);
 *   origin:  DEVICE int32 [B][2] = (i / columns, i % columns): the pixel's index IN THE REGION is the window's upper-left corner in the
 *            canvas, as the reference has it.  It can be handed to catseg_ingest_warp_u8 as it is; with Wc < Hc - margin the px-wide
 *            window may reach past the canvas' right edge, where that launch writes zeros (the reference returns a narrower array there).
 *   total (may be NULL): DEVICE uint64 [B]; flat (may be NULL): DEVICE int64 [B] = i.
 * Two launches: a row pass (one block per frame and region row; B * rows * 8 bytes of row sums into `workspace`) and a pick pass (one
 * block per frame).  No atomics, no ordering between blocks: the same inputs give the same bits.  No read is unguarded, whatever minv,
 * lut, flips or m53 hold.  HBM traffic: the labels under the region once (up to four source bytes per pixel, neighbours share cache
 * lines), plus one region row per frame a second time.
 * CATSEG_EINVAL before anything is launched: bad dims, px outside the canvas, an empty region, a NULL label map / table / m53 / origin,
 * a canvas that is not the frame without a matrix, misaligned 8-byte operands.  CATSEG_EWORKSPACE: workspace NULL, misaligned or smaller
 * than catseg_crop_freq_workspace() (0 for arguments the pick would refuse).
 */
#ifndef CATSEG_CROPFREQ_H
#define CATSEG_CROPFREQ_H

#include "catseg.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t catseg_crop_freq_workspace(int B, int Hc, int Wc, int px);
int catseg_crop_freq_pick(const uint8_t* lbl, int B, int H, int W, const uint8_t* lut, const int32_t* flips, const double* minv, int Hc,
                          int Wc, int px, const uint64_t* wq, const uint64_t* m53, int32_t* origin, uint64_t* total, int64_t* flat,
                          void* workspace, size_t workspace_bytes, catseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
