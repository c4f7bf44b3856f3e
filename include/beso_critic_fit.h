/*
 * beso_critic_fit.h -- C ABI of libbeso_critic.so: training the critic behind value-ranked action selection
 * (include/beso_rank.h) by Implicit Q-Learning (Kostrikov et al. 2021) on the MI355X (gfx950).  Q(s, a, g) and V(s, g) are two
 * MLPNetworks of include/beso_mlp.h with out_dim == 1; V is fitted to a target copy of Q by an expectile regression, Q to
 * r + gamma (1 - done) V(s') by a squared error.  No action outside the data set is ever evaluated.
 *
 * One critic step is ten enqueues: beso_critic_rows (here), beso_mlp_fwd of Q with a keep buffer, beso_mlp_fwd of Q on the
 * target parameters, beso_mlp_fwd of V on the 2 M rows [V rows ; V' rows] with a keep buffer, beso_critic_loss (here),
 * beso_mlp_bwd of Q with dy = dq, beso_mlp_bwd of V with dy = [dv ; M zeros], and the two optimizer steps (Q's also moves the
 * target: beso_adam_step's ema argument).
 *
 * Conventions are those of include/beso_mlp.h: plain C, device pointers owned by the caller, contiguous fp32, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state beside the calling thread's last message.  Return value: a status of include/beso_hip.h
 * (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2, BESO_ERR_BAD_ARG = -3, BESO_ERR_HIP = -6); beso_critic_last_error names the argument a
 * non-zero status refused.  Everything is checked before anything is enqueued.  Outputs may hold anything on entry; every
 * element of every output is written and nothing outside its extent is.  No atomics anywhere: equal inputs give equal bits.
 */
#ifndef BESO_CRITIC_FIT_H
#define BESO_CRITIC_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* What the calling thread's last non-zero status of this library refused ("" before the first). */
const char* beso_critic_last_error(void);

/* The three row blocks of a step, M = B T rows each, straight from their sources.  With gw = obs_dim when goal != NULL, else 0:
 *     q_rows [M, obs_dim + act_dim + gw]   row (b, t) = [ state[b, t, :] | action[b, t, :] | goal[gb, goal_steps - 1, :] ]
 *     v_rows [2 M, obs_dim + gw]           row (b, t) = [ state[b, t, :] | goal[gb, goal_steps - 1, :] ]
 *                                  row M + (b, t) = [ s'[b, t, :]     | goal[gb, goal_steps - 1, :] ]
 * with s'[b, t] = next_state[b, t] when next_state != NULL, else state[b, t + 1].  The next-state rows stand directly behind the
 * V rows, so that one beso_mlp_fwd call on 2 M rows evaluates V(s) and V(s').  ONE launch, one thread per output element, plain
 * vector stores; every output float is a copy of an input float (no arithmetic).  Row widths are at most 512.
 *   state        [B, state_steps, obs_dim]; state_steps >= T + 1 when next_state == NULL, >= T otherwise
 *   next_state   NULL, or [B, T, obs_dim]
 *   action       [B, T, act_dim]
 *   goal         NULL, or [goal_rows, goal_steps, obs_dim] with goal_rows == B or 1 (gb = b or 0): only step goal_steps - 1 is
 *                read (pass goal_steps = goal_rows = 0 with NULL)
 * BESO_ERR_BAD_SHAPE also for more than 2^31 - 1 rows, or more than (2^31 - 1) 256 output elements (the launch's grid limit);
 * q_rows and v_rows must not overlap each other or an input.                                                              */
int beso_critic_rows(const float* state, const float* next_state, const float* action, const float* goal, int B, int T,
                     int state_steps, int goal_steps, int goal_rows, int obs_dim, int act_dim, float* q_rows, float* v_rows,
                     void* stream);

/* The two coupled losses of one IQL step over M rows, and their two gradients.  Per row m, with tau = expectile:
 *     u = q_target - v         e = (u < 0) ? 1 - tau : tau        l_v = e (u u)        (expectile regression of V onto Q_target)
 *     y = reward + gamma (1 - done) v_next       d = q - y        l_q = d d            (TD regression of Q onto r + gamma V(s'))
 *     S = sum_m w_m (M, as an fp32 value, when weight == NULL: every w_m = 1)
 *     loss_v [1] = (sum_m w_m l_v,m) / S      per_row_v [M] = l_v,m      dv [M] = (w_m * dl_v/dv) / S,  dl_v/dv = -2 e u
 *     loss_q [1] = (sum_m w_m l_q,m) / S      per_row_q [M] = l_q,m      dq [M] = (w_m * dl_q/dq) / S,  dl_q/dq =  2 d
 *     adv [M] = u                                                                      (the advantage Q_target(s, a) - V(s))
 * q_target and v_next are constants of both losses: no gradient is formed for them, dv holds nothing of L_Q and dq nothing of
 * L_V.  S == 0 gives loss_v = loss_q = 0 and dv = dq = 0 (no NaN from the division).  u == 0 and u == -0 take e = tau.  A NaN in
 * q, reward, done or v_next reaches loss_q, per_row_q[m] and dq[m] of its own row; one in v, loss_v, per_row_v[m], dv[m] and
 * adv[m] of its own row; one in q_target those of L_V likewise; no other row's gradient sees it.  (A NaN weight reaches S and so
 * everything.)  ONE launch of ONE 256-thread workgroup that passes over the rows twice.
 *
 * The order of every rounding is part of the contract.  All arithmetic is fp32; no product is fused into an addition.
 *   constants  om = 1 - tau (one fp32 subtraction)
 *   pass 1   lane j (0 ... 255) visits the rows m = j, j + 256, j + 512, ... in ascending order.  For each it forms
 *                u = q_target - v;  e = u < 0 ? om : tau;  uu = u * u;  l_v = e * uu
 *                nd = 1 - done;  gn = gamma * nd;  p = gn * v_next;  y = reward + p;  d = q - y;  l_q = d * d
 *            writes per_row_v[m] = l_v, per_row_q[m] = l_q, adv[m] = u, and adds w_m to its sum s_j, (w_m * l_v) to its sum a_j and
 *            (w_m * l_q) to its sum b_j, all three starting from 0 (without weights: s_j is not formed and l_v, l_q are added as
 *            they are)
 *   between  S = ((s_0 + s_1) + s_2) + ... + s_255, lane order, starting from s_0; A likewise from the a_j and B from the b_j;
 *            loss_v = A / S, loss_q = B / S
 *   pass 2   u, e and d are formed again as in pass 1;  eu = e * u;  g_v = -2 * eu;  g_q = 2 * d;
 *            dv[m] = (w_m * g_v) / S,  dq[m] = (w_m * g_q) / S  (without weights: g_v / S and g_q / S)
 *   q, q_target, v, v_next, reward, done   [M]; done holds 0 or 1 as floats
 *   weight   NULL, or [M]
 * No output may overlap an input or another output.
 * BESO_ERR_BAD_SHAPE: M < 1 or M > 2^31 - 1.  BESO_ERR_BAD_ARG: a NULL (other than weight) or misaligned pointer, gamma outside
 * [0, 1], expectile outside (0, 1) -- a NaN is outside.                                                                      */
int beso_critic_loss(const float* q, const float* q_target, const float* v, const float* v_next, const float* reward,
                     const float* done, const float* weight, long long M, float gamma, float expectile, float* loss_q,
                     float* loss_v, float* per_row_q, float* per_row_v, float* dq, float* dv, float* adv, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_CRITIC_FIT_H */
