/*
 * beso_select.h -- C ABI of libbeso_select.so: best-of-K action selection for rollout inference on the MI355X (gfx950).
 *
 * A diffusion policy is multimodal: K x_T draws per environment give K action candidates, and the rollout acts on their mean
 * or on the candidate in the densest mode.  Around one sampler call on N K rows stand two launches:
 *     beso_candidates_expand   N windows -> N K sampler rows, a fresh x_T in each row's newest slot
 *     beso_candidates_select   N K sampled windows -> N chosen ones
 *
 * Conventions are those of include/beso_guide.h: plain C, device pointers owned by the caller, contiguous fp32 (lengths and
 * index: int32), work is enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates
 * nothing, never synchronises and keeps no state beside the calling thread's last message.  Return value: a status of
 * include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2, BESO_ERR_BAD_ARG = -3, BESO_ERR_UNSUPPORTED = -5, BESO_ERR_HIP = -6);
 * beso_candidates_last_error names what a non-zero status refused.  Everything is checked before anything is enqueued.  Output
 * buffers may hold anything on entry; every element of them is written and nothing outside their extent is.  No atomics, no
 * workspace, every sum in a fixed order: the same inputs give the same bits.
 *
 * lengths [N] is the rollout's live tensor behind beso_rollout_begin (include/beso_hip.h), in 1 ... W; a value outside that
 * range is read as the nearest end of it, so that it cannot index out of a window.
 */
#ifndef BESO_SELECT_H
#define BESO_SELECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

enum {
    BESO_SELECT_MEAN = 0, /* the sample mean of the K newest-slot actions */
    BESO_SELECT_KDE = 1   /* the candidate of the highest diagonal Gaussian kernel density among its K siblings */
};
#define BESO_SELECT_MAX_K 256  /* candidates per environment beso_candidates_select takes */
#define BESO_SELECT_MAX_ACT 64 /* action components it takes: K act floats live in LDS */

/* What the calling thread's last non-zero status of this library refused ("" before the first). */
const char* beso_candidates_last_error(void);

/* state_k [N K, W, obs_dim] and x_k [N K, W, act_dim]: row n K + k is a copy of environment n's state [N, W, obs_dim] /
 * x [N, W, act_dim] (what beso_rollout_begin wrote), and slot lengths[n] - 1 of x_k is then noise[n, k, :] * sigma_max
 * (noise [N, K, act_dim]: the product beso_rollout_begin forms for the newest slot).  ONE launch, a workgroup per output row;
 * 16-byte loads and stores where W obs_dim (W act_dim) is a multiple of 4 and the buffers are 16-byte aligned, one float at
 * a time otherwise.  N, K, W, obs_dim, act_dim >= 1; N K and the floats of one row within int range. */
int beso_candidates_expand(const float* state, const float* x, const int32_t* lengths, const float* noise, float sigma_max,
                           int N, int W, int obs_dim, int act_dim, int K, float* state_k, float* x_k, void* stream);

/* x0 [N, W, act_dim], index [N], scores [N, K] from the sampler's result x0_k [N K, W, act_dim].  The candidates of
 * environment n are c[k, :] = x0_k[n K + k, lengths[n] - 1, :]; ONE launch, a workgroup per environment holds them in LDS.
 *
 * BESO_SELECT_MEAN: a[d] = (((c[0, d] + c[1, d]) + c[2, d]) + ... + c[K-1, d]) / float(K), one running fp32 sum in that
 *   order -- the order is part of the contract.  x0[n] is row n K's window with its newest slot replaced by a;
 *   index[n] = -1; scores[n, :] = 0.  `bandwidth` is not read.
 *
 * BESO_SELECT_KDE: with mu_d / sd_d the population mean / standard deviation of component d over the K candidates,
 *   h_d = bandwidth                                                        when bandwidth > 0, else (Scott's rule, diagonal)
 *   h_d = max(sd_d, 1e-6 max(1, |mu_d|)) K^(-1 / (act_dim + 4));
 *   s_k = log sum_j exp(-1/2 sum_d ((c[k, d] - c[j, d]) / h_d)^2), j = 0 ... K-1 in that order, j = k included: its term is
 *   the sum's largest, exp(0), so no shift is needed and s_k >= 0;
 *   index[n] = argmax_k s_k, the lowest k among equal scores; scores[n, :] = s; x0[n] is the whole window of row
 *   n K + index[n] (its earlier slots are the shared previous actions as the sampler returned them for that row).
 *   Differences, quotients, squares, exp and log are fp32; mu_d, sd_d and the sum over j are accumulated in fp64.
 *   K = 1 gives index 0 and s_0 = 0; K identical candidates give s_k = log K and index 0.
 *   Non-finite candidates: the arithmetic runs through (no loop depends on a value), a NaN score compares as "not greater"
 *   and as "not equal", and index[n] is in 0 ... K-1 whatever the scores are.
 *
 * 1 <= K <= BESO_SELECT_MAX_K and 1 <= act_dim <= BESO_SELECT_MAX_ACT, else BESO_ERR_UNSUPPORTED; N, W >= 1 and a known
 * mode, else BESO_ERR_BAD_SHAPE / BESO_ERR_BAD_ARG.  x0 must not overlap x0_k. */
int beso_candidates_select(const float* x0_k, const int32_t* lengths, int mode, float bandwidth, int N, int W, int act_dim,
                           int K, float* x0, int32_t* index, float* scores, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_SELECT_H */
