/*
 * libcatseg_hip.so -- feature header: per-frame label tables for the ingest launches (csrc/ingest.hip, csrc/warp.hip, csrc/cropfreq.hip).
 * The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok, catseg_last_error() gives the
 * message).
 *
 * A semi-supervised batch holds labelled frames (raw CaDIS ids, to be remapped to network ids) beside pseudo-labelled frames (network ids
 * already: DatasetFromDF(labels_remaped=True), datasets/Dataset_from_df.py:49-53 of the reference).  One launch serves both:
 *   luts:            DEVICE uint8 [T][256], T >= 1 label tables (may be NULL without an index: labels pass through);
 *   table_of_frame:  DEVICE int32 [B], the table row of every frame, or NULL = row 0 for every frame.  The kernels clamp the index into
 *                    [0, T): whatever it holds, no read is unguarded.
 * Every other argument is the one of the entry point without `_tables` (catseg.h: catseg_ingest_u8, catseg_ingest_warp_u8;
 * catseg_cropfreq.h: catseg_crop_freq_pick), and so are the results: those entry points are these with T = 1 and a NULL index.
 * CATSEG_EINVAL before anything is launched, beside the refusals of the plain entry points: T < 1, an index without tables, a misaligned
 * index.
 */
#ifndef CATSEG_INGEST_TABLES_H
#define CATSEG_INGEST_TABLES_H

#include "catseg.h"

#ifdef __cplusplus
extern "C" {
#endif

int catseg_ingest_u8_tables(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T,
                            const int32_t* table_of_frame, const int32_t* flips, int pad_top, int pad_bottom, const float* mean,
                            const float* stdv, float* x_nchw, float* x_nhwc4, int64_t* labels, catseg_stream_t stream);
int catseg_ingest_warp_u8_tables(const uint8_t* img, const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T,
                                 const int32_t* table_of_frame, const int32_t* flips, const double* minv, int Hc, int Wc,
                                 const int32_t* origin, int Hw, int Ww, int pad_top, int pad_bottom, const float* mean, const float* stdv,
                                 float* x_nchw, float* x_nhwc4, uint8_t* x_u8, int64_t* labels, catseg_stream_t stream);
int catseg_crop_freq_pick_tables(const uint8_t* lbl, int B, int H, int W, const uint8_t* luts, int T, const int32_t* table_of_frame,
                                 const int32_t* flips, const double* minv, int Hc, int Wc, int px, const uint64_t* wq, const uint64_t* m53,
                                 int32_t* origin, uint64_t* total, int64_t* flat, void* workspace, size_t workspace_bytes,
                                 catseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
