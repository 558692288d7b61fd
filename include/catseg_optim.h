/*
 * libcatseg_hip.so -- feature header: the fused optimiser updates on the flat parameter buffer (Adam / AdamW with weight decay and
 * amsgrad, momentum SGD, parameter groups, clipping by the global gradient norm; optim.py), csrc/optim.hip.
 * The conventions of catseg.h hold (asynchronous on `stream`, never allocates, never synchronises, 0 = ok, catseg_last_error() gives
 * the message, which starts with the function's name).  Every launch can be captured into a hipGraph.
 *
 * Buffers p, g, m, v, vmax, buf: DEVICE float [n], 16-byte aligned, laid out as engine.FlatParams lays the parameters out: every
 * parameter starts on a 64-float boundary and the gap behind it is zero, so that a 64-float chunk belongs to one parameter.
 *
 * Group map -- group_of_chunk: DEVICE uint8 [ceil(n / 64)], entry c names the parameter group (0 .. G-1, 1 <= G <= 8) of the elements
 * 64 c .. 64 c + 63; NULL = group 0 everywhere.  The update kernels read 16 bytes (4 elements) per access, which never straddles a
 * chunk.  An entry >= G is not detected (the map is device memory); it selects a row entry that catseg_optim_hyper zeroed (lr = wd = 0).
 *
 * Step scalars -- a row of CATSEG_OPTIM_HYPER_FLOATS (20) floats that catseg_optim_hyper fills on the HOST:
 *   row[0] = 1 - beta1^step, row[1] = sqrt(1 - beta2^step), both formed in double and rounded once (step >= 1);
 *   row[2] = the gradient scale (1/world of dist.GradSync);
 *   row[3] = the effective dampening of SGD: 0 while step <= 1, `dampening` afterwards;
 *   row[4 + 2 k] = lr of group k, row[5 + 2 k] = weight decay of group k, k < G; 0 for G <= k < 8.
 * The launches take the row either from HOST memory (hyper_host: read during the call and passed to the kernel by value) or from DEVICE
 * memory (hyper_dev: read by the kernel, so that a captured launch replays with the values uploaded in front of the replay); exactly
 * one of the two is non-NULL.  Both forms run the same kernel on the same 20 values and write the same bits.
 *
 * Clip pointer -- clip: DEVICE float [2] as catseg_grad_norm writes it, or NULL.  The update kernels read clip[1]; NULL means 1.
 *
 * catseg_adam_step_ex -- per element, with g' = (g * grad_scale) * clip and the group's lr, wd:
 *   wd_mode CATSEG_WD_COUPLED (torch.optim.Adam):    g' += wd * p;
 *   wd_mode CATSEG_WD_DECOUPLED (torch.optim.AdamW): p *= 1 - lr * wd before the update;
 *   wd_mode CATSEG_WD_NONE: the weight-decay entries of the row are not read;
 *   m = m * beta1 + g' * (1 - beta1); v = v * beta2 + g' * g' * (1 - beta2);
 *   vmax != NULL (amsgrad): vmax = max(vmax, v), and vmax takes v's place below;
 *   p -= (lr / row[0]) * (m / (sqrt(v) / row[1] + eps)).
 * With G = 1, CATSEG_WD_NONE, no map, vmax = NULL and clip = NULL it writes the bits of catseg_adam_step / catseg_adam_step_dev
 * (catseg.h) for the same lr, step and gradient scale.  A padding element (p = g = 0, state 0) stays exactly 0 under every option.
 *
 * catseg_sgd_step -- torch.optim.SGD's order, per element with g' = (g * grad_scale) * clip:
 *   g' += wd * p (coupled, when use_wd != 0);
 *   buf != NULL: buf = momentum * buf + (1 - row[3]) * g'; u = nesterov ? g' + momentum * buf : buf;    buf == NULL: u = g';
 *   p -= lr * u.
 * The momentum buffer starts at zero; row[3] = 0 on the first step gives torch's "buf = g'" there (momentum * 0 + g') without a branch
 * that a graph replay would freeze.  nesterov needs buf.
 *
 * catseg_grad_norm -- the global L2 norm of g * grad_scale and the clip factor, two launches, deterministic:
 *   1. catseg_grad_norm_workspace(n) / 8 blocks (a function of n alone, at most 1024); block b sums the squares of a fixed slice of g in
 *      fp64 (the square of an fp32 value is exact there, nothing overflows) in a fixed order and writes workspace[b];
 *   2. one block adds the partials in index order, s, and writes out[0] = (float)(sqrt(s) * |grad_scale|) and
 *      out[1] = min(1, max_norm / (out[0] + 1e-6f)) in fp32 (torch.nn.utils.clip_grad_norm_'s factor).
 *   No float atomics, no completion counter: two launches over the same gradients give the same bits.
 *   grad_scale is passed by value, or read from hyper_dev[2] when hyper_dev != NULL (a DEVICE row as above).
 *   workspace: DEVICE, 8-byte aligned, at least catseg_grad_norm_workspace(n) bytes; out: DEVICE float [2], 8-byte aligned.
 *
 * CATSEG_EINVAL before anything is launched: n <= 0; a NULL or misaligned p / g / m / v (a misaligned vmax / buf); G outside 1..8;
 * neither or both of hyper_host / hyper_dev; an unknown wd_mode; nesterov without buf; a NULL or misaligned workspace or out; a
 * workspace smaller than the query; max_norm that is negative or NaN.
 */
#ifndef CATSEG_OPTIM_H
#define CATSEG_OPTIM_H

#include "catseg.h"

#define CATSEG_OPTIM_HYPER_FLOATS 20
#define CATSEG_OPTIM_MAX_GROUPS 8
#define CATSEG_WD_NONE 0
#define CATSEG_WD_COUPLED 1
#define CATSEG_WD_DECOUPLED 2

#ifdef __cplusplus
extern "C" {
#endif

void catseg_optim_hyper(int step, float beta1, float beta2, float grad_scale, float dampening, int G, const float* lr, const float* wd,
                        float* row);
int catseg_adam_step_ex(float* p, const float* g, float* m, float* v, float* vmax, long long n, const uint8_t* group_of_chunk, int G,
                        const float* hyper_host, const float* hyper_dev, float beta1, float beta2, float eps, int wd_mode,
                        const float* clip, catseg_stream_t stream);
int catseg_sgd_step(float* p, const float* g, float* buf, long long n, const uint8_t* group_of_chunk, int G, const float* hyper_host,
                    const float* hyper_dev, float momentum, int nesterov, int use_wd, const float* clip, catseg_stream_t stream);
size_t catseg_grad_norm_workspace(long long n);
int catseg_grad_norm(const float* g, long long n, float grad_scale, const float* hyper_dev, float max_norm, void* workspace,
                     size_t workspace_bytes, float* out, catseg_stream_t stream);
/* the grid cap of the two update kernels in blocks of 256 threads x 4 elements (tests size a case past one sweep with it) */
int catseg_optim_grid_cap(void);

#ifdef __cplusplus
}
#endif
#endif
