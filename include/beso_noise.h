/*
 * beso_noise.h -- C ABI of libbeso_noise.so: keyed standard-normal draws for rollout inference on the MI355X (gfx950).
 *
 * A rollout over N environments draws an x_T per environment step, K of them with best-of-K selection, and one tensor per
 * sampler step with an ancestral sampler.  Drawn from one generator over all rows, what environment 7 receives depends on N,
 * on its row and on every draw made before.  Here a value is a pure function of
 *     key       uint64   the environment's seed
 *     episode   uint32   the environment's episode counter         step   uint32   its step counter inside the episode
 *     purpose   BESO_NOISE_*  which draw of the step               s      the slab: candidate k, or sampler step i
 *     e         the element inside the environment's slice of the slab
 * and of nothing else: not of N, of the environment's row, of the launch geometry or of any other call.
 *
 * THE GENERATOR is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), stated
 * in full so that it can be restated anywhere.  All arithmetic is on uint32 and wraps.
 *     counter c = (c0, c1, c2, c3) = (e / 4, s, step, (episode << 4) | purpose)       key (k0, k1) = (key & 0xffffffff, key >> 32)
 *     ten rounds; before every round but the first:  k0 += 0x9E3779B9, k1 += 0xBB67AE85
 *     one round:  p0 = 0xD2511F53 * c0 (64-bit product), p1 = 0xCD9E8D57 * c2 (64-bit product)
 *                 c = (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0))
 *     the words w0 ... w3 are c after the tenth round.  (counter 0, key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.)
 * Episodes at or above 2^28 share their counter word with lower ones: (episode << 4) drops the top four bits.
 *
 * THE NORMALS are two Box-Muller pairs in fp32, every operation rounded on its own (no contraction):
 *     u(w) = float((w >> 8) + 1) * 2^-24       in (0, 1]: exact, and the logarithm's argument is never 0
 *     v(w) = float(w >> 8) * 2^-24             in [0, 1): exact
 *     r01 = sqrtf(-2.0f * logf(u(w0))),  t01 = 6.2831855f * v(w1):   z0 = r01 * cosf(t01),  z1 = r01 * sinf(t01)
 *     r23 = sqrtf(-2.0f * logf(u(w2))),  t23 = 6.2831855f * v(w3):   z2 = r23 * cosf(t23),  z3 = r23 * sinf(t23)
 * (6.2831855f is 2 pi rounded to fp32, 0x40C90FDB.)  Element e takes z[e % 4] of the block e / 4, times `scale` (one fp32
 * multiply); beso_noise_words gives w[e % 4] itself.  |z| <= sqrt(48 ln 2) = 5.77.  logf / cosf / sinf are the device
 * library's: they agree with a float64 evaluation of the same expression from the same words to a few fp32 ulps of the
 * result's scale, not to the bit.
 *
 * Conventions are those of include/beso_select.h: plain C, device pointers owned by the caller, contiguous arrays, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state beside the calling thread's last message.  Return value: a status of include/beso_hip.h
 * (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2, BESO_ERR_BAD_ARG = -3, BESO_ERR_HIP = -6); beso_noise_last_error names what a non-zero
 * status refused.  Everything is checked before anything is enqueued.  Output buffers may hold anything on entry; every
 * element of them is written and nothing outside their extent is.  One launch per call, a thread per four elements (one
 * Philox block), plain loads and stores: no atomics, no LDS, no workspace.
 */
#ifndef BESO_NOISE_H
#define BESO_NOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

enum {
    BESO_NOISE_XT = 0,        /* the x_T draw of an environment step: slab 0, e in [act_dim] */
    BESO_NOISE_CANDIDATE = 1, /* the x_T draw of candidate k of best-of-K selection: slab k, e in [act_dim] */
    BESO_NOISE_STEP = 2       /* the noise of step i of an ancestral sampler: slab i, e in the environment's sampler rows */
};
#define BESO_NOISE_MAX_PURPOSE 15 /* the purpose shares a counter word with the episode: four bits */

/* What the calling thread's last non-zero status of this library refused ("" before the first). */
const char* beso_noise_last_error(void);

/* out [S][N][E] uint32: out[s][n][e] = word e % 4 of the block (key keys[n]; counter (e / 4, s, steps[n], (episodes[n] << 4) |
 * purpose)).  keys [N] uint64, episodes / steps [N] uint32.  For audit and for bit-exact tests of the generator.
 * N, S, E >= 1 and S N E within int range, 0 <= purpose <= BESO_NOISE_MAX_PURPOSE; pointers 4-byte (keys: 8-byte) aligned. */
int beso_noise_words(const uint64_t* keys, const uint32_t* episodes, const uint32_t* steps, int N, int purpose, int S, int E,
                     uint32_t* out, void* stream);

/* out [S][N][E] fp32: the normal of the same block and position, times `scale` (finite).  Otherwise as beso_noise_words. */
int beso_noise_normal(const uint64_t* keys, const uint32_t* episodes, const uint32_t* steps, int N, int purpose, int S, int E,
                      float scale, float* out, void* stream);

/* One environment step's draws, one launch in front of beso_rollout_begin (include/beso_hip.h).
 *
 * The counters advance first: with reset [N] uint8 (may be NULL: no environment resets) set for environment n,
 * episode = episodes_in[n] + 1 and step = 0; otherwise episode = episodes_in[n] and step = steps_in[n] + 1.  The advanced
 * counters are written to episodes_out / steps_out [N] and are the ones every draw of the call uses.  The out pair must not
 * overlap the in pair (BESO_ERR_BAD_ARG where the pointers are equal): every thread of the launch reads an environment's
 * counters and one writes them, so the caller alternates between two pairs of arrays from step to step.  `reset` is the
 * rollout's own flag array, read only.  (An environment that is to start at episode 0, step 0 is handed episode 0xffffffff
 * with its reset flag set.)
 *
 * With the advanced counters:
 *   x_t   [N][act_dim]          purpose BESO_NOISE_XT, slab 0: the `noise` of beso_rollout_begin
 *   cand  [N][K][act_dim]       purpose BESO_NOISE_CANDIDATE, slab k: the `noise` of beso_candidates_expand (include/
 *                               beso_select.h); NULL with K = 0
 *   step_noise [n_steps][N][step_elems]   purpose BESO_NOISE_STEP, slab i, e in [step_elems]: the `noise` of
 *                               beso_sample_ancestral / beso_sample_solver with step_elems = rows window act_dim, `rows` the
 *                               sampler rows per environment (1, or K with candidates: row k of the environment is
 *                               e / (window act_dim) = k, so candidate 0's step noise is the K = 1 rollout's); NULL with
 *                               n_steps = 0
 * all unscaled standard normals.  N, act_dim >= 1; K, n_steps >= 0; step_elems >= 1 where n_steps > 0; every array within int
 * range. */
int beso_noise_rollout(const uint64_t* keys, const uint8_t* reset, const uint32_t* episodes_in, const uint32_t* steps_in,
                       uint32_t* episodes_out, uint32_t* steps_out, int N, int act_dim, int K, int n_steps, int step_elems,
                       float* x_t, float* cand, float* step_noise, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_NOISE_H */
