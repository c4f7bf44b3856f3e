/*
 * beso_scale.h -- C ABI of libbeso_scale.so: the scalings of MinMaxScaler (reference beso/networks/scaler/scaler_class.py:169-338,
 * the scaler of the block-push workspace) as single launches on the MI355X (gfx950).
 *
 *     beso_scale_rows_mixed     up to four tensors, each z-scored or min-max scaled per feature, in ONE launch
 *                               (a training batch: state and goal z-scored, the action min-max scaled)
 *     beso_rollout_end_minmax   the tail of a vectorised rollout step for this scaler: newest action, clip, remember,
 *                               min-max un-scale (beso_rollout_end of include/beso_hip.h is the z-score one)
 *
 * Conventions are those of include/beso_select.h: plain C, device pointers owned by the caller, contiguous fp32 (lengths:
 * int32, clip bounds: float64), work is enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library
 * allocates nothing, never synchronises and keeps no state beside the calling thread's last message.  Return value: a status
 * of include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2, BESO_ERR_BAD_ARG = -3, BESO_ERR_HIP = -6); beso_scale_last_error
 * names what a non-zero status refused.  Everything is checked before anything is enqueued.  Every element of an output is
 * written and nothing outside its extent is.  No atomics, no workspace.
 *
 * Arithmetic: every operation below is its own correctly rounded IEEE fp32 operation, in the order written -- nothing is
 * contracted into an fma, the division is the correctly rounded one -- so the results are, bit for bit, those of the torch
 * expressions of the reference evaluated one elementwise operation at a time.  A zero range divides by zero and gives the
 * inf / NaN the reference gives.
 */
#ifndef BESO_SCALE_H
#define BESO_SCALE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

enum {
    BESO_SCALE_ZSCORE = 0, /* out = (x - p0[c]) / p1[c]:                    p0 = mean, p1 = std + 1e-12 */
    BESO_SCALE_MINMAX = 1  /* out = ((x - p0[c]) / p1[c]) * p2[c] + p3[c]:  p0 = min, p1 = max - min, p2 = new_max - new_min,
                              p3 = new_min */
};
#define BESO_SCALE_MAX_ITEMS 4 /* tensors per beso_scale_rows_mixed launch */

/* What the calling thread's last non-zero status of this library refused ("" before the first). */
const char* beso_scale_last_error(void);

/* dst[k][r, c] from src[k][r, c] for the n tensors k = 0 ... n-1, tensor k being [rows[k], cols[k]] and scaled as kind[k]
 * says, with the per-feature rows p0[k] ... p3[k] of cols[k] floats each (ZSCORE reads p0 and p1 only; its p2[k] / p3[k] may
 * be NULL, and so may the tables p2 / p3 themselves when no tensor is MINMAX):
 *     ZSCORE   d = x - p0[c];  out = d / p1[c]
 *     MINMAX   a = x - p0[c];  b = a / p1[c];  m = b * p2[c];  out = m + p3[c]
 * src, dst, kind, p0 ... p3, rows and cols are HOST arrays of n entries whose pointer entries are device pointers.  ONE launch,
 * grid-stride over the rows[k] cols[k] elements of all tensors (64-bit counts).  1 <= n <= BESO_SCALE_MAX_ITEMS, rows[k] >= 0
 * (a tensor without rows is skipped), cols[k] >= 1.  dst[k] may be src[k]; no other overlap. */
int beso_scale_rows_mixed(const float* const* src, float* const* dst, const int* kind, const float* const* p0,
                          const float* const* p1, const float* const* p2, const float* const* p3, const long long* rows,
                          const int* cols, int n, void* stream);

/* One thread per (environment n, action component c), with t = lengths[n] read as the nearest of 1 ... window:
 *     v       = x0[n, t - 1, c]                                   x0 [n_envs, window, act_dim], the sampler's result
 *     clipped = float(min(max(double(v), lo[c]), hi[c]))          lo / hi [act_dim] float64: MinMaxScaler.clip_action's
 *                                                                 1.1 y_bounds rows (a NaN passes through)
 *     act_ctx[n, t - 1, c] = clipped                              act_ctx [n_envs, window, act_dim]
 *     a = clipped - new_lo[c];  b = a / span[c];  m = b * range[c];  pred[n, c] = m + lo_y[c]
 * -- MinMaxScaler.inverse_scale_output with new_lo = new_min_y, span = new_max_y - new_min_y, range = y_max - y_min,
 * lo_y = y_min, [act_dim] fp32 each.  All four NULL (scale_data off): pred[n, c] = clipped; some of them NULL is an error.
 * window, act_dim >= 1; n_envs >= 0, where 0 enqueues nothing; n_envs window act_dim within int range. */
int beso_rollout_end_minmax(const float* x0, const int32_t* lengths, const double* lo, const double* hi, const float* new_lo,
                            const float* span, const float* range, const float* lo_y, float* act_ctx, float* pred, int n_envs,
                            int window, int act_dim, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_SCALE_H */
