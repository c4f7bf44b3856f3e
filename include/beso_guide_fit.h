/*
 * beso_guide_fit.h -- C ABI of libbeso_guidefit.so: training the guide of classifier-guided sampling (include/beso_guide.h) as a
 * classifier of the NOISED action and its noise level, on the MI355X (gfx950).
 *
 * The guide is the MLPNetwork of include/beso_mlp.h with out_dim == 1.  A noise-aware guide reads one more input column behind
 * [state | a | goal]: c_noise[b] = log(sigma[b]) / 4, the value GCDenoiser feeds its network.  The caller computes c_noise (one
 * value per sample); this library only places it.
 *
 * One fit step is five enqueues: beso_guide_fit_rows (here), beso_mlp_fwd with a keep buffer, beso_guide_fit_loss (here),
 * beso_mlp_bwd with dy = dq, and the optimizer step.  beso_guide_apply_sigma is beso_guide_apply over rows with the c_noise
 * column, for sampling with such a guide.
 *
 * Conventions are those of include/beso_mlp.h: plain C, device pointers owned by the caller, contiguous fp32, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state.  Return value: a status of include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2,
 * BESO_ERR_BAD_ARG = -3, BESO_ERR_HIP = -6).  Everything is checked before anything is enqueued.  Outputs may hold anything on
 * entry; every element of every output is written and nothing outside its extent is.  No atomics anywhere: equal inputs give
 * equal bits.
 */
#ifndef BESO_GUIDE_FIT_H
#define BESO_GUIDE_FIT_H

#include <stddef.h>
#include <stdint.h>

#include "beso_mlp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* beso_guide_fit_loss: the per-row loss l(q, y) */
enum {
    BESO_GUIDE_FIT_MSE = 0,   /* (q - y)^2                                                                                */
    BESO_GUIDE_FIT_BCE = 1    /* q a logit, y in [0, 1]: max(q, 0) - q y + log1p(exp(-|q|))                                */
};

/* rows [M = B T, in_dim], in_dim = obs_dim + act_dim (+ obs_dim with a goal) (+ 1 with c_noise), at most 512.  Row (b, t) is
 *     [ state[b, t, :] | action[b, t, :] + sigma[b] * noise[b, t, :] | goal[gb, goal_steps - 1, :] | c_noise[b] ]
 * ONE launch, one thread per element of `rows`, plain vector stores.  The noised action is a multiplication, then an addition,
 * each rounded to fp32 on its own (never a fused multiply-add): `action + sigma[:, None, None] * noise` in fp32 torch ops gives
 * the same bits.
 *   state         [B, state_steps, obs_dim], state_steps >= T: row (b, t) reads step t
 *   action        [B, T, act_dim]
 *   goal          NULL, or [goal_rows, goal_steps, obs_dim] with goal_rows == B or 1 (gb = b or 0): only step goal_steps - 1 is
 *                 read (pass goal_steps = goal_rows = 0 with NULL)
 *   sigma, noise  [B] and [B, T, act_dim]; both NULL: the rows hold the clean action
 *   c_noise       NULL, or [B]: the last column
 * BESO_ERR_BAD_SHAPE also for more than 2^31 - 1 rows, or 2^39 elements and more.                                         */
int beso_guide_fit_rows(const float* state, const float* action, const float* goal, const float* sigma, const float* noise,
                        const float* c_noise, int B, int T, int state_steps, int goal_steps, int goal_rows, int obs_dim,
                        int act_dim, float* rows, void* stream);

/* The weighted mean loss of q [M] against target [M], each row's loss, and the gradient beso_mlp_bwd takes as dy:
 *     S = sum_m w_m (M, as an fp32 value, when weight == NULL: every w_m = 1)
 *     loss [1] = (sum_m w_m l_m) / S        per_row [M] = l_m        dq [M] = (w_m * dl_m/dq) / S
 * with dl/dq = 2 (q - y) for BESO_GUIDE_FIT_MSE and sigmoid(q) - y for BESO_GUIDE_FIT_BCE.  S == 0 gives loss = 0 and dq = 0
 * (no NaN from the division).  ONE launch of ONE 256-thread workgroup that passes over the rows twice.
 *
 * The order of every rounding is part of the contract.  All arithmetic is fp32; no product is fused into an addition.
 *   pass 1   lane j (0 ... 255) visits the rows m = j, j + 256, j + 512, ... in ascending order.  For each it forms l_m --
 *            BESO_GUIDE_FIT_MSE: d = q - y, l = d * d -- writes per_row[m] and adds w_m to its sum s_j and (w_m * l_m) to its
 *            sum n_j, both starting from 0 (without weights: s_j is not formed and l_m is added as it is)
 *   between  S = ((s_0 + s_1) + s_2) + ... + s_255, lane order, starting from s_0; N likewise from the n_j; loss = N / S
 *   pass 2   dq[m] = (w_m * g_m) / S with g_m = 2 * d for BESO_GUIDE_FIT_MSE (without weights: g_m / S)
 * BESO_GUIDE_FIT_BCE follows the same order with l and g evaluated by expf and log1pf: its bits are the device library's.
 *   weight   NULL, or [M]                                                                                                 */
int beso_guide_fit_loss(const float* q, const float* target, const float* weight, long long M, int kind, float* loss,
                        float* per_row, float* dq, void* stream);

/* beso_guide_supported (include/beso_guide.h) for rows that end in the c_noise column: dims->in_dim == obs_dim + act_dim
 * (+ obs_dim with use_goal) + 1, and the LDS rule taken at that in_dim. */
int beso_guide_supported_sigma(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal);

/* beso_guide_apply (include/beso_guide.h: arguments, limits, arithmetic, ONE launch) over rows
 * [state | a | goal | c_noise[b]]: the same kernel with the row assembly reading a fourth source.  The column's input gradient,
 * like the state and goal columns', is not part of `out`.
 *   c_noise  [B] on the device: log(sigma) / 4 as the caller computed it                                                  */
int beso_guide_apply_sigma(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                           const float* goal, const float* pred, const float* sigma, const float* c_noise, int B, int T,
                           int state_steps, int goal_steps, int goal_rows, int obs_dim, int act_dim, float lam, float* out,
                           void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_GUIDE_FIT_H */
