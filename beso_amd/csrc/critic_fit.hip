// Training the critic behind value-ranked action selection by Implicit Q-Learning (include/beso_critic_fit.h): libbeso_critic.so.
// Two kernels of its own around the network launches of libbeso_mlp.so:
//   critic_rows_kernel   one thread per output element of the three row blocks: Q rows [state | action | goal], V rows
//                        [state | goal] and, directly behind them, V' rows [next state | goal] -- copies, no arithmetic
//   critic_loss_kernel   ONE workgroup, two passes over the M rows: the per-row expectile and TD losses, the advantage and the
//                        lane sums, then dv = w dl_v/dv / S and dq = w dl_q/dq / S
// The loss kernel is fp32 with every product and sum rounded on its own (fp contraction off): the header states the order.
#include "side_host.h"
#include "../../include/beso_critic_fit.h"

namespace beso_critic {

using beso::launch_plain;
using namespace beso_side;

constexpr int kThreads = 256;
constexpr int kMaxDim = 512;
constexpr long long kMaxElements = 0x7fffffffLL * kThreads;   // one thread per output element: the grid's x dimension ends at 2^31 - 1

struct Rows {
    const float *state, *next_state, *action, *goal;
    float *q_rows, *v_rows;
    int T, state_steps, obs, adim, gw;         // gw: obs with a goal, else 0
    long long goal_stride, goal_off;           // floats between two samples' goals (0: one shared goal) and to step G - 1
    long long M, q_total, total;               // rows of a block; M (obs + adim + gw); q_total + 2 M (obs + gw)
};

__global__ __launch_bounds__(kThreads) void critic_rows_kernel(Rows rw) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= rw.total) return;
    const bool is_q = e < rw.q_total;
    const long long i = is_q ? e : e - rw.q_total;                   // element of q_rows, or of v_rows [2 M, obs + gw]
    const int width = rw.obs + (is_q ? rw.adim : 0) + rw.gw;
    const long long r = i / width;
    const int c = (int)(i - r * width);
    const bool next = !is_q && r >= rw.M;
    const long long m = next ? r - rw.M : r;                         // (b, t)
    const long long b = m / rw.T;
    const int t = (int)(m - b * rw.T);
    const int gc = c - rw.obs - (is_q ? rw.adim : 0);                // the goal column, when >= 0
    float v;
    if (c < rw.obs) {
        if (!next) v = rw.state[((size_t)b * rw.state_steps + t) * rw.obs + c];
        else if (rw.next_state) v = rw.next_state[(size_t)m * rw.obs + c];
        else v = rw.state[((size_t)b * rw.state_steps + t + 1) * rw.obs + c];
    } else if (gc < 0) {
        v = rw.action[(size_t)m * rw.adim + (c - rw.obs)];
    } else {
        v = rw.goal[(size_t)b * rw.goal_stride + rw.goal_off + gc];
    }
    (is_q ? rw.q_rows : rw.v_rows)[i] = v;
}

struct Loss {
    const float *q, *q_target, *v, *v_next, *reward, *done, *weight;
    float *loss_q, *loss_v, *per_row_q, *per_row_v, *dq, *dv, *adv;
    long long M;
    float gamma, expectile;
};

// u = q_target - v, its expectile weight e, and d = q - y of row m
__device__ __forceinline__ void row_terms(const Loss& a, long long m, float om, float& u, float& e, float& d) {
#pragma clang fp contract(off)
    u = a.q_target[m] - a.v[m];
    e = u < 0.f ? om : a.expectile;
    const float nd = 1.0f - a.done[m];
    const float gn = a.gamma * nd;
    const float p = gn * a.v_next[m];
    const float y = a.reward[m] + p;
    d = a.q[m] - y;
}

__global__ __launch_bounds__(kThreads) void critic_loss_kernel(Loss a) {
#pragma clang fp contract(off)
    __shared__ float lane_s[kThreads], lane_a[kThreads], lane_b[kThreads];
    __shared__ float total_s;
    const int j = threadIdx.x;
    const float om = 1.0f - a.expectile;
    float s = 0.f, sa = 0.f, sb = 0.f;
    for (long long m = j; m < a.M; m += kThreads) {
        float u, e, d;
        row_terms(a, m, om, u, e, d);
        const float uu = u * u;
        const float lv = e * uu;
        const float lq = d * d;
        a.per_row_v[m] = lv;
        a.per_row_q[m] = lq;
        a.adv[m] = u;
        if (a.weight) {
            const float w = a.weight[m];
            const float wv = w * lv;
            const float wq = w * lq;
            s = s + w;
            sa = sa + wv;
            sb = sb + wq;
        } else {
            sa = sa + lv;
            sb = sb + lq;
        }
    }
    lane_s[j] = s;
    lane_a[j] = sa;
    lane_b[j] = sb;
    __syncthreads();
    if (j == 0) {
        float S = lane_s[0], A = lane_a[0], B = lane_b[0];
        for (int i = 1; i < kThreads; ++i) {
            S = S + lane_s[i];
            A = A + lane_a[i];
            B = B + lane_b[i];
        }
        if (!a.weight) S = (float)a.M;
        total_s = S;
        a.loss_v[0] = S == 0.f ? 0.f : A / S;
        a.loss_q[0] = S == 0.f ? 0.f : B / S;
    }
    __syncthreads();
    const float S = total_s;
    for (long long m = j; m < a.M; m += kThreads) {
        float u, e, d;
        row_terms(a, m, om, u, e, d);
        const float eu = e * u;
        float gv = -2.0f * eu;
        float gq = 2.0f * d;
        if (a.weight) {
            const float w = a.weight[m];
            gv = w * gv;
            gq = w * gq;
        }
        a.dv[m] = S == 0.f ? 0.f : gv / S;
        a.dq[m] = S == 0.f ? 0.f : gq / S;
    }
}

}  // namespace beso_critic

// ------------------------------------------------------------------------------------------------------------ host
using namespace beso_critic;

extern "C" const char* beso_critic_last_error(void) { return g_error; }

extern "C" int beso_critic_rows(const float* state, const float* next_state, const float* action, const float* goal, int B, int T,
                                int state_steps, int goal_steps, int goal_rows, int obs_dim, int act_dim, float* q_rows,
                                float* v_rows, void* stream) {
    const char* fn = "beso_critic_rows";
    if (obs_dim < 1 || obs_dim > kMaxDim) return refuse(BESO_ERR_BAD_SHAPE, "%s: obs_dim = %d, supported: 1 ... %d", fn, obs_dim, kMaxDim);
    if (act_dim < 1 || act_dim > kMaxDim) return refuse(BESO_ERR_BAD_SHAPE, "%s: act_dim = %d, supported: 1 ... %d", fn, act_dim, kMaxDim);
    const int gw = goal ? obs_dim : 0;
    const int qw = obs_dim + act_dim + gw, vw = obs_dim + gw;
    if (qw > kMaxDim)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: obs_dim + act_dim%s = %d floats per Q row, supported: up to %d", fn, goal ? " + obs_dim" : "", qw, kMaxDim);
    if (B < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: B = %d must be at least 1", fn, B);
    if (T < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: T = %d must be at least 1", fn, T);
    const int need = next_state ? T : T + 1;
    if (state_steps < need || (long long)T + 1 > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: state_steps = %d, but %s needs at least T%s = %d", fn, state_steps,
                      next_state ? "a step with next_state" : "next_state == NULL (s' = state[:, t + 1])", next_state ? "" : " + 1", need);
    const long long M = (long long)B * T;
    const long long total = M * qw + 2 * M * vw;
    if (M > 0x7fffffffLL || total > kMaxElements)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: B T = %lld rows (at most 2^31 - 1) with %lld output elements (at most (2^31 - 1) 256)", fn, M, total);
    if (!GoalRows::valid(goal, goal_steps, goal_rows, B))
        return refuse(BESO_ERR_BAD_SHAPE, "%s: goal_steps = %d, goal_rows = %d: a goal is [B = %d or 1, goal_steps >= 1, obs_dim], and both are 0 without one",
                      fn, goal_steps, goal_rows, B);
    const Named ptrs[] = {{"state", state, false}, {"next_state", next_state, true}, {"action", action, false}, {"goal", goal, true},
                          {"q_rows", q_rows, false}, {"v_rows", v_rows, false}};
    if (const int st = check_pointers(fn, ptrs)) return st;

    Rows rw{};
    rw.state = state;
    rw.next_state = next_state;
    rw.action = action;
    rw.goal = goal;
    rw.q_rows = q_rows;
    rw.v_rows = v_rows;
    rw.T = T;
    rw.state_steps = state_steps;
    rw.obs = obs_dim;
    rw.adim = act_dim;
    rw.gw = gw;
    const GoalRows g(goal, goal_steps, goal_rows, B, obs_dim);
    rw.goal_stride = g.stride;
    rw.goal_off = g.off;
    rw.M = M;
    rw.q_total = M * qw;
    rw.total = total;
    const hipError_t e = launch_plain<critic_rows_kernel>(dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads),
                                                          (hipStream_t)stream, rw);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}

extern "C" int beso_critic_loss(const float* q, const float* q_target, const float* v, const float* v_next, const float* reward,
                                const float* done, const float* weight, long long M, float gamma, float expectile, float* loss_q,
                                float* loss_v, float* per_row_q, float* per_row_v, float* dq, float* dv, float* adv, void* stream) {
    const char* fn = "beso_critic_loss";
    if (M < 1 || M > 0x7fffffffLL) return refuse(BESO_ERR_BAD_SHAPE, "%s: M = %lld rows, supported: 1 ... 2^31 - 1", fn, M);
    if (!(gamma >= 0.f && gamma <= 1.f)) return refuse(BESO_ERR_BAD_ARG, "%s: gamma = %g must lie in [0, 1]", fn, (double)gamma);
    if (!(expectile > 0.f && expectile < 1.f))
        return refuse(BESO_ERR_BAD_ARG, "%s: expectile = %g must lie in (0, 1)", fn, (double)expectile);
    const Named ptrs[] = {{"q", q, false}, {"q_target", q_target, false}, {"v", v, false}, {"v_next", v_next, false},
                          {"reward", reward, false}, {"done", done, false}, {"weight", weight, true}, {"loss_q", loss_q, false},
                          {"loss_v", loss_v, false}, {"per_row_q", per_row_q, false}, {"per_row_v", per_row_v, false},
                          {"dq", dq, false}, {"dv", dv, false}, {"adv", adv, false}};
    if (const int st = check_pointers(fn, ptrs)) return st;

    Loss a{};
    a.q = q;
    a.q_target = q_target;
    a.v = v;
    a.v_next = v_next;
    a.reward = reward;
    a.done = done;
    a.weight = weight;
    a.loss_q = loss_q;
    a.loss_v = loss_v;
    a.per_row_q = per_row_q;
    a.per_row_v = per_row_v;
    a.dq = dq;
    a.dv = dv;
    a.adv = adv;
    a.M = M;
    a.gamma = gamma;
    a.expectile = expectile;
    const hipError_t e = launch_plain<critic_loss_kernel>(dim3(1), dim3(kThreads), (hipStream_t)stream, a);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}
