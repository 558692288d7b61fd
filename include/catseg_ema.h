/*
 * libcatseg_hip.so -- feature header: the running average of the weights (EMA / SWA; optim.WeightAverage), csrc/ema.hip.
 * The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok, catseg_last_error() gives
 * the message, which starts with the function's name).  Every launch can be captured into a hipGraph.
 *
 * The weight w -- passed by value (w_host, in [0, 1]), or read by the kernel from DEVICE memory w_dev[0] when w_dev != NULL (w_host is
 * then ignored and a value in device memory is not checked), so that a captured launch replays with what was uploaded in front of
 * the replay.  Both forms run the same kernel on the same value and write the same bits.
 *
 * lerp(avg, p, w) is torch.lerp's two-sided form, the product and the sum of each side one fused multiply-add (as torch's CPU kernel
 * forms them; spelled out, so the compiler's choice does not decide the bits):
 *   w < 0.5:   avg + w * (p - avg)        = fma(w, p - avg, avg)
 *   otherwise: p - (p - avg) * (1 - w)    = fma(-(p - avg), 1 - w, p)
 * so that w = 1 writes p itself (p - (p - avg) * 0): the first update of an average is a copy without a branch that a graph replay
 * would freeze.  An element with p = avg = 0 (the padding of engine.FlatParams) stays exactly 0 for every w.
 *
 * catseg_ema_update -- avg[i] = lerp(avg[i], p[i], w), i < n.  p, avg: DEVICE float [n], 16-byte aligned, not overlapping.  A capped
 *   grid of 256-thread blocks strides over the 16-byte vectors; the last n % 4 elements are read and written one by one.  12 bytes of
 *   HBM traffic per element.
 * catseg_ema_swap -- exchanges a[i] and b[i], i < n.  Same buffers, same access pattern; 16 bytes per element.
 * catseg_ema_table -- one launch over a DEVICE table of `count` entries (8-byte aligned, 24 bytes each):
 *     struct catseg_ema_entry { float* live; long long shadow_off; int n; int pad; };
 *   entry e stands for the n floats at `live` (DEVICE, 4-byte aligned: a separately allocated buffer or a view into one) and the n
 *   floats shadow[shadow_off .. shadow_off + n).  mode CATSEG_EMA_LERP: shadow = lerp(shadow, live, w); mode CATSEG_EMA_SWAP: the two
 *   are exchanged (w is not read).  One 256-thread block per entry, 4-byte accesses: the entries are the running means and variances
 *   of BatchNorm modules, a few to 2048 floats each.  The entries' contents are device memory and are not checked.
 *
 * CATSEG_EINVAL before anything is launched: n <= 0; a NULL or misaligned (16 bytes) p / avg / a / b; w_host outside [0, 1] or NaN
 * when w_dev is NULL (catseg_ema_table: in mode CATSEG_EMA_LERP); a misaligned (4 bytes) w_dev; count <= 0; an unknown mode; a NULL
 * or misaligned table (8 bytes) or shadow (4 bytes).
 */
#ifndef CATSEG_EMA_H
#define CATSEG_EMA_H

#include "catseg.h"

#define CATSEG_EMA_LERP 0
#define CATSEG_EMA_SWAP 1
#define CATSEG_EMA_ENTRY_BYTES 24

#ifdef __cplusplus
extern "C" {
#endif

int catseg_ema_update(const float* p, float* avg, long long n, float w_host, const float* w_dev, catseg_stream_t stream);
int catseg_ema_swap(float* a, float* b, long long n, catseg_stream_t stream);
int catseg_ema_table(const void* entries, int count, float* shadow, int mode, float w_host, const float* w_dev, catseg_stream_t stream);
/* the grid cap of catseg_ema_update / catseg_ema_swap in blocks of 256 threads x 4 elements (tests size a case past one sweep with it) */
int catseg_ema_grid_cap(void);

#ifdef __cplusplus
}
#endif
#endif
