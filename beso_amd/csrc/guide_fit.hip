// Training the guide of classifier-guided sampling (include/beso_guide_fit.h): libbeso_guidefit.so.  Two kernels of its own around
// the network launches of libbeso_mlp.so, and the guide gradient of guide_tile.h over rows with the noise-level column:
//   fit_rows_kernel   one thread per element of rows [M, in_dim]: [state | action + sigma noise | goal | c_noise]
//   fit_loss_kernel   ONE workgroup, two passes over q [M]: per-row loss and the lane sums, then dq = w dl/dq / S
// Both are fp32 with every product and sum rounded on its own (fp contraction off): the header states the order.
#include "guide_tile.h"
#include "../../include/beso_guide_fit.h"

namespace beso_guide_fit {

using beso::launch_plain;
using beso::to_status;
using namespace beso_side;

constexpr int kThreads = 256;
constexpr int kMaxDim = 512;

struct Rows {
    const float *state, *action, *goal, *sigma, *noise, *c_noise;
    float* rows;
    int T, state_steps, obs, adim, in_dim;
    long long goal_stride, goal_off;           // floats between two samples' goals (0: one shared goal) and to step G - 1
    long long total;                           // M in_dim
};

__global__ __launch_bounds__(kThreads) void fit_rows_kernel(Rows rw) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= rw.total) return;
    const long long m = e / rw.in_dim;
    const int c = (int)(e - m * rw.in_dim);
    const long long b = m / rw.T;
    const int t = (int)(m - b * rw.T);
    float v;
    if (c < rw.obs) {
        v = rw.state[((size_t)b * rw.state_steps + t) * rw.obs + c];
    } else if (c < rw.obs + rw.adim) {
        const size_t i = (size_t)m * rw.adim + (c - rw.obs);
        v = rw.action[i];
        if (rw.noise) {
            const float p = rw.sigma[b] * rw.noise[i];
            v = v + p;
        }
    } else if (rw.c_noise && c == rw.in_dim - 1) {
        v = rw.c_noise[b];
    } else {
        v = rw.goal[(size_t)b * rw.goal_stride + rw.goal_off + (c - rw.obs - rw.adim)];
    }
    rw.rows[e] = v;
}

// l and g = dl/dq of one row
__device__ __forceinline__ void row_loss(int kind, float q, float y, float& l, float& g) {
#pragma clang fp contract(off)
    if (kind == BESO_GUIDE_FIT_MSE) {
        const float d = q - y;
        l = d * d;
        g = 2.0f * d;
    } else {
        const float e = expf(-fabsf(q));                              // in (0, 1]: no overflow at either end
        l = fmaxf(q, 0.f) - q * y + log1pf(e);
        g = (q >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e)) - y;      // sigmoid(q) - y
    }
}

__global__ __launch_bounds__(kThreads) void fit_loss_kernel(const float* __restrict__ q, const float* __restrict__ target,
                                                            const float* __restrict__ weight, long long M, int kind,
                                                            float* __restrict__ loss, float* __restrict__ per_row,
                                                            float* __restrict__ dq) {
#pragma clang fp contract(off)
    __shared__ float lane_s[kThreads], lane_n[kThreads];
    __shared__ float total_s;
    const int j = threadIdx.x;
    float s = 0.f, n = 0.f;
    for (long long m = j; m < M; m += kThreads) {
        float l, g;
        row_loss(kind, q[m], target[m], l, g);
        per_row[m] = l;
        if (weight) {
            const float w = weight[m];
            const float wl = w * l;
            s = s + w;
            n = n + wl;
        } else {
            n = n + l;
        }
    }
    lane_s[j] = s;
    lane_n[j] = n;
    __syncthreads();
    if (j == 0) {
        float S = lane_s[0], N = lane_n[0];
        for (int i = 1; i < kThreads; ++i) {
            S = S + lane_s[i];
            N = N + lane_n[i];
        }
        if (!weight) S = (float)M;
        total_s = S;
        loss[0] = S == 0.f ? 0.f : N / S;
    }
    __syncthreads();
    const float S = total_s;
    for (long long m = j; m < M; m += kThreads) {
        float l, g;
        row_loss(kind, q[m], target[m], l, g);
        if (weight) g = weight[m] * g;
        dq[m] = S == 0.f ? 0.f : g / S;
    }
}

}  // namespace beso_guide_fit

using namespace beso_guide_fit;

extern "C" int beso_guide_fit_rows(const float* state, const float* action, const float* goal, const float* sigma,
                                   const float* noise, const float* c_noise, int B, int T, int state_steps, int goal_steps,
                                   int goal_rows, int obs_dim, int act_dim, float* rows, void* stream) {
    if (obs_dim < 1 || act_dim < 1 || obs_dim > kMaxDim || act_dim > kMaxDim) return BESO_ERR_BAD_SHAPE;
    const int in_dim = obs_dim + act_dim + (goal ? obs_dim : 0) + (c_noise ? 1 : 0);
    if (in_dim > kMaxDim) return BESO_ERR_BAD_SHAPE;
    if (B < 1 || T < 1 || state_steps < T) return BESO_ERR_BAD_SHAPE;
    const long long M = (long long)B * T;
    if (M > 0x7fffffffLL || M * in_dim >= (1LL << 39)) return BESO_ERR_BAD_SHAPE;
    if (!GoalRows::valid(goal, goal_steps, goal_rows, B)) return BESO_ERR_BAD_SHAPE;
    if (!state || !action || !rows || (sigma == nullptr) != (noise == nullptr)) return BESO_ERR_BAD_ARG;
    if (misaligned(state, 4) || misaligned(action, 4) || misaligned(goal, 4) || misaligned(sigma, 4) || misaligned(noise, 4) ||
        misaligned(c_noise, 4) || misaligned(rows, 4))
        return BESO_ERR_BAD_ARG;

    Rows rw{};
    rw.state = state;
    rw.action = action;
    rw.goal = goal;
    rw.sigma = sigma;
    rw.noise = noise;
    rw.c_noise = c_noise;
    rw.rows = rows;
    rw.T = T;
    rw.state_steps = state_steps;
    rw.obs = obs_dim;
    rw.adim = act_dim;
    rw.in_dim = in_dim;
    const GoalRows g(goal, goal_steps, goal_rows, B, obs_dim);
    rw.goal_stride = g.stride;
    rw.goal_off = g.off;
    rw.total = M * in_dim;
    return to_status(launch_plain<fit_rows_kernel>(dim3((unsigned)((rw.total + kThreads - 1) / kThreads)), dim3(kThreads),
                                                   (hipStream_t)stream, rw));
}

extern "C" int beso_guide_fit_loss(const float* q, const float* target, const float* weight, long long M, int kind, float* loss,
                                   float* per_row, float* dq, void* stream) {
    if (M < 1 || M > 0x7fffffffLL) return BESO_ERR_BAD_SHAPE;
    if (kind != BESO_GUIDE_FIT_MSE && kind != BESO_GUIDE_FIT_BCE) return BESO_ERR_BAD_ARG;
    if (!q || !target || !loss || !per_row || !dq) return BESO_ERR_BAD_ARG;
    if (misaligned(q, 4) || misaligned(target, 4) || misaligned(weight, 4) || misaligned(loss, 4) || misaligned(per_row, 4) || misaligned(dq, 4))
        return BESO_ERR_BAD_ARG;
    return to_status(launch_plain<fit_loss_kernel>(dim3(1), dim3(kThreads), (hipStream_t)stream, q, target, weight, M, kind, loss,
                                                   per_row, dq));
}

extern "C" int beso_guide_supported_sigma(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal) {
    return beso_guide::check_guide(dims, obs_dim, act_dim, use_goal, 1);
}

extern "C" int beso_guide_apply_sigma(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                                      const float* goal, const float* pred, const float* sigma, const float* c_noise, int B, int T,
                                      int state_steps, int goal_steps, int goal_rows, int obs_dim, int act_dim, float lam,
                                      float* out, void* stream) {
    return beso_guide::guide_apply<true>(params, n_params, dims, state, goal, pred, sigma, c_noise, B, T, state_steps, goal_steps,
                                         goal_rows, obs_dim, act_dim, lam, out, stream);
}
