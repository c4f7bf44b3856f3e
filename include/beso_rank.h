/*
 * beso_rank.h -- C ABI of libbeso_rank.so: value-ranked best-of-K action selection for rollout inference on the MI355X
 * (gfx950).  "Sample K actions from the diffusion policy, execute argmax_k q": behind one sampler call on N K rows
 * (include/beso_select.h: beso_candidates_expand in front of it) stands ONE launch that scores every candidate with a learned
 * scalar function q = MLP([state | action | goal]) -- the MLPNetwork of include/beso_mlp.h with out_dim == 1, over the rows of
 * include/beso_guide.h -- and writes the best candidate's window.  Forward only: no gradient, no change to the sampler.
 *
 * Conventions are those of include/beso_select.h: plain C, device pointers owned by the caller, contiguous fp32 (lengths and
 * index: int32), work is enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates
 * nothing, never synchronises and keeps no state beside the calling thread's last message.  Return value: a status of
 * include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2, BESO_ERR_BAD_ARG = -3, BESO_ERR_UNSUPPORTED = -5, BESO_ERR_HIP = -6);
 * beso_rank_last_error names what a non-zero status refused.  Everything is checked before anything is enqueued.  Output
 * buffers may hold anything on entry; every element of them is written and nothing outside their extent is.  No atomics, no
 * keep buffer, no workspace, plain vector stores, every sum in a fixed order: the same inputs give the same bits.
 *
 * Arithmetic: fp32 throughout.  Every product of a layer runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), which is a
 * k-ordered chain of fused multiply-adds.  A row's dot product with a weight row w over `width` inputs (zeros behind `width` up
 * to the next multiple of 16) is ONE such chain that starts at 0 and takes the products in the order
 *     for k0 = 0, 16, 32, ...:  for j = 0 ... 3:  for g = 0 ... 3:   acc = fma(x[k0 + 4 g + j], w[k0 + 4 g + j], acc)
 * then z = acc + bias, then the activation in fp32 (include/beso_mlp.h's; a NaN pre-activation stays NaN through every one of
 * them, ReLU included, as in torch).  The order is a function of the layer's width alone: a candidate's score does not depend
 * on N, on the environment's index, on K or on where among its siblings the candidate stands.
 *
 * lengths [N] is the rollout's live tensor behind beso_rollout_begin (include/beso_hip.h), in 1 ... W; a value outside that
 * range is read as the nearest end of it, so that it cannot index out of a window.
 */
#ifndef BESO_RANK_H
#define BESO_RANK_H

#include <stddef.h>
#include <stdint.h>

#include "beso_mlp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define BESO_RANK_MAX_K 256  /* candidates per environment beso_rank_candidates takes (BESO_SELECT_MAX_K) */
#define BESO_RANK_MAX_ACT 64 /* action components it takes (BESO_SELECT_MAX_ACT) */

/* What the calling thread's last non-zero status of this library refused ("" before the first). */
const char* beso_rank_last_error(void);

/* BESO_OK when beso_rank_candidates serves a network of `dims` over rows [obs_dim | act_dim (| obs_dim with use_goal)], else
 * the status beso_rank_candidates would return for it (beso_rank_last_error names the reason).  Reads `dims` only; touches no
 * device.  Supported: what beso_mlp_fwd supports (in_dim in 1 ... 512; hidden_dim a multiple of 16 up to 512; n_hidden in
 * 1 ... 4; a known activation) with out_dim == 1, in_dim == obs_dim + act_dim (+ obs_dim with use_goal), obs_dim >= 1 and
 * 1 <= act_dim <= BESO_RANK_MAX_ACT (else BESO_ERR_UNSUPPORTED). */
int beso_rank_supported(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal);

/* x0 [N, W, act_dim], index [N], scores [N, K] from the sampler's result x0_k [N K, W, act_dim].  ONE launch, a workgroup of
 * 256 threads per environment.  With t = clamp(lengths[n], 1, W) the input row of candidate k is
 *     [state[n, t - 1, :] | x0_k[n K + k, t - 1, :] | goal[n or 0, goal_steps - 1, :]]
 * (the column order of MLPGuide.forward; the goal part only with a goal).  The workgroup carries its K rows forward through
 * the network in tiles of 16 rows -- two [16][round16(max(in_dim, hidden_dim)) + 4] LDS tiles, the weights streamed from memory
 * as the MFMA's other operand -- keeps the K scalars q in LDS, and writes
 *     scores[n, k] = q_k
 *     index[n]     = argmax_k q_k: the lowest k among equal scores.  A NaN score compares as "not greater" than any score, and
 *                    any other score as greater than a NaN: a candidate with a NaN score is chosen only when every score is
 *                    NaN, and then index[n] = 0.  index[n] is in 0 ... K-1 whatever the scores are.
 *     x0[n]        = x0_k[n K + index[n]]: the whole window, bit for bit (its earlier slots are the shared previous actions as
 *                    the sampler returned them for that row).
 *   params       host array of n_params = 2 (n_hidden + 1) DEVICE pointers, as beso_mlp_fwd takes them
 *   state        [N, W, obs_dim] (what beso_rollout_begin wrote: the un-expanded windows)
 *   goal         NULL (dims->in_dim == obs_dim + act_dim; pass goal_steps = goal_rows = 0), or [goal_rows, goal_steps, obs_dim]
 *                with goal_rows == N or 1 (one goal shared by all environments): only step goal_steps - 1 is read
 * 1 <= K <= BESO_RANK_MAX_K and 1 <= act_dim <= BESO_RANK_MAX_ACT, else BESO_ERR_UNSUPPORTED; a network outside
 * beso_rank_supported, N, W < 1 or N K / W act_dim beyond the int range: BESO_ERR_BAD_SHAPE; a NULL or misaligned pointer, a
 * wrong n_params, an unknown activation: BESO_ERR_BAD_ARG.  x0 must not overlap x0_k. */
int beso_rank_candidates(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                         const float* goal, int goal_steps, int goal_rows, const float* x0_k, const int32_t* lengths, int N,
                         int W, int obs_dim, int act_dim, int K, float* x0, int32_t* index, float* scores, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_RANK_H */
