/*
 * beso_guide.h -- C ABI of libbeso_guide.so: the sampling-time hot path of classifier-guided sampling (the reference's
 * k_diffusion/classifier_free_sampler.py::ClassifierGuidedSampleModel, lines 56-90) with an MLP guide, on the MI355X (gfx950).
 *
 * Behind every denoiser evaluation of a guided sampler stands
 *     out[b, t, :] = pred[b, t, :] + lam * sigma[b]^2 * d/da sum(q),    q = MLP([state[b, t, :] | a[b, t, :] | goal[gb, G-1, :]])
 * taken at a = pred: q the scalar output (out_dim == 1) of the MLPNetwork of include/beso_mlp.h, the goal part present only
 * with a goal, gb = b or 0 (one goal row shared by all samples).  beso_guide_apply is that line as ONE launch.
 *
 * Conventions are those of include/beso_mlp.h: plain C, device pointers owned by the caller, contiguous fp32, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state.  Return value: a status of include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2,
 * BESO_ERR_BAD_ARG = -3, BESO_ERR_HIP = -6).  Everything is checked before anything is enqueued.  `out` may hold anything on
 * entry; every element of it is written and nothing outside its extent is.
 *
 * Arithmetic: fp32 throughout.  Every product of the GEMMs runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) with fp32
 * accumulation in a fixed order; no keep buffer, no workspace, no weight gradients, no atomics: the same inputs give the same
 * bits, and a row (b, t) of `out` depends on that row's inputs alone.
 *
 * Supported: what include/beso_mlp.h supports (in_dim in 1 ... 512; hidden_dim a multiple of 16 up to 512; n_hidden in
 * 1 ... 4) with out_dim == 1, in_dim == obs_dim + act_dim (+ obs_dim with a goal), and n_hidden + 2 tiles of
 * 16 x (round16(max(in_dim, hidden_dim)) + 4) floats within the 160 KiB of LDS a workgroup may have on gfx950 -- at
 * hidden_dim = 512 that is n_hidden <= 2; n_hidden = 4 goes up to a width of 416.  Anything else is BESO_ERR_BAD_SHAPE (an
 * unknown activation: BESO_ERR_BAD_ARG).
 */
#ifndef BESO_GUIDE_H
#define BESO_GUIDE_H

#include <stddef.h>
#include <stdint.h>

#include "beso_mlp.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* BESO_OK when beso_guide_apply serves a guide network of `dims` over rows [obs_dim | act_dim (| obs_dim with use_goal)],
 * else the status beso_guide_apply would return for it.  Reads `dims` only; touches no device. */
int beso_guide_supported(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal);

/* out [B, T, act_dim] = pred + lam * sigma^2 * d/da sum(MLP([state | a | goal])) at a = pred.  ONE launch: a workgroup of 256
 * threads owns 16 of the M = B T rows.  It assembles their input rows from the three sources in LDS, carries them forward
 * through the hidden layers keeping every pre-activation tile in LDS (the last Linear's value q is not needed: only its weight
 * row is, as the chain's seed dq = 1 times W_last), runs the data-gradient chain backward through the same tiles, and for the
 * action columns of the input gradient alone writes the line above.
 *   params       host array of n_params = 2 (n_hidden + 1) DEVICE pointers, as beso_mlp_fwd takes them
 *   state        [B, state_steps, obs_dim], state_steps >= T: row (b, t) reads step t
 *   goal         NULL (dims->in_dim == obs_dim + act_dim), or [goal_rows, goal_steps, obs_dim] with goal_rows == B or 1: only
 *                step goal_steps - 1 is read (pass goal_steps = goal_rows = 0 with NULL)
 *   pred, out    [B, T, act_dim]; they may be the same buffer (any other overlap is not supported)
 *   sigma        [B] on the device
 *   lam          the guidance scale, a host value                                                                       */
int beso_guide_apply(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                     const float* goal, const float* pred, const float* sigma, int B, int T, int state_steps, int goal_steps,
                     int goal_rows, int obs_dim, int act_dim, float lam, float* out, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_GUIDE_H */
