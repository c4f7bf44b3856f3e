// The guide-gradient kernel and its host call, shared by guide.hip (libbeso_guide.so: rows [state | pred | goal]) and
// guide_fit.hip (libbeso_guidefit.so: the same rows with the noise-level column c_noise behind them).  One kernel template, fp32 on
// v_mfma_f32_16x16x4_f32 through the tile GEMMs of mlp_tile.h:
//   guide_apply_kernel<SIGMA>  a workgroup assembles 16 rows [state | pred | goal (| c_noise)] in LDS, carries them forward through
//                              the hidden layers (every pre-activation tile stays in LDS), runs the data-gradient chain of sum(q)
//                              backward and writes out = pred + lam sigma^2 dq/da for the action columns
// Nothing leaves the workgroup but `out`: no keep buffer, no workspace, no weight gradient.  SIGMA = false reads three sources and
// is, instruction for instruction, the kernel guide.hip held before the column existed.
#pragma once
#include "mlp_tile.h"
#include "side_host.h"

namespace beso_guide {

using namespace beso_mlp;
using beso_side::GoalRows;
using beso_side::misaligned;

constexpr int kMaxLinear = 5;                  // n_hidden <= 4
constexpr size_t kMaxLds = 160 * 1024;         // what one workgroup may declare on gfx950

struct Guide {
    const float* w[kMaxLinear];
    const float* b[kMaxLinear];
    const float *state, *goal, *pred, *sigma;  // pred and out may be the same buffer: neither is __restrict__
    float* out;
    int n_hidden, in_dim, hidden, act;
    int T, state_steps, obs, adim;
    long long goal_stride, goal_off;           // floats between two samples' goals (0: one shared goal) and to step G - 1
    float lam;
};

// c_noise [B]: the last input column of SIGMA rows; not read without SIGMA
template <bool SIGMA>
__global__ __launch_bounds__(kThreads) void guide_apply_kernel(Guide gd, long long M, int pitch, const float* c_noise) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* cur = lds;
    float* nxt = lds + kRows * pitch;
    float* Z = lds + 2 * kRows * pitch;                               // Z + l * kRows * pitch: z_l, hidden layer l's pre-activation
    const long long m0 = (long long)blockIdx.x * kRows;
    const int H = gd.hidden, I = gd.in_dim, L = gd.n_hidden, act = gd.act;
    const int obs = gd.obs, adim = gd.adim;

    // the input rows, column by column from their three (SIGMA: four) sources; rows >= M and columns [I, round16(I)) are 0
    const int wp = round16(I);
    for (int i = threadIdx.x; i < kRows * wp; i += kThreads) {
        const int r = i / wp, c = i - r * wp;
        const long long m = m0 + r;
        float v = 0.f;
        if (m < M && c < I) {
            const long long b = m / gd.T;
            const int t = (int)(m - b * gd.T);
            if (c < obs) v = gd.state[((size_t)b * gd.state_steps + t) * obs + c];
            else if (c < obs + adim) v = gd.pred[(size_t)m * adim + (c - obs)];
            else if (SIGMA && c == I - 1) v = c_noise[b];
            else v = gd.goal[(size_t)b * gd.goal_stride + gd.goal_off + (c - obs - adim)];
        }
        cur[r * pitch + c] = v;
    }
    __syncthreads();

    // forward: z_l = a_{l-1} W_l^T + b_l kept, a_l = act(z_l) for the next layer.  The last Linear is not evaluated: d sum(q)
    // needs its weight row, not q.
    for (int l = 0; l < L; ++l) {
        const int K = l == 0 ? I : H;
        const float* bias = gd.b[l];
        float* z = Z + l * kRows * pitch;
        const bool feed = l + 1 < L;
        tile_xwt(cur, pitch, gd.w[l], H, K, [&](int r, int n, float v) {
            const float zz = v + bias[n];
            z[r * pitch + n] = zz;
            if (feed) nxt[r * pitch + n] = act_fwd(act, zz);
        });
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }

    // the seed dq = 1 through the last Linear [1, H]: dz_{L-1} = W_last * act'(z_{L-1})
    {
        const float* wl = gd.w[L];
        const float* z = Z + (L - 1) * kRows * pitch;
        for (int i = threadIdx.x; i < kRows * H; i += kThreads) {
            const int r = i / H, k = i - r * H;
            cur[r * pitch + k] = wl[k] * act_bwd(act, z[r * pitch + k]);
        }
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {                                // dz_{l-1} = (dz_l W_l) * act'(z_{l-1})
        const float* z = Z + (l - 1) * kRows * pitch;
        tile_xw(cur, pitch, gd.w[l], H, H, [&](int r, int k, float v) { nxt[r * pitch + k] = v * act_bwd(act, z[r * pitch + k]); });
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }

    // dx = dz_0 W_0 for the action columns only (the state, goal and c_noise columns' gradient is never formed), and the guided
    // prediction.  A thread reads pred[e] before it writes out[e], and no other thread touches element e: pred == out is safe.
    const float lam = gd.lam;
    tile_xw(cur, pitch, gd.w[0], H, I, obs, adim, [&](int r, int c, float v) {
        const long long m = m0 + r;
        if (m < M) {
            const float s = gd.sigma[m / gd.T];
            const size_t e = (size_t)m * adim + c;
            gd.out[e] = gd.pred[e] + (lam * v) * (s * s);
        }
    });
}

// ------------------------------------------------------------------------------------------------------------ host
static int pitch_of(const beso_mlp_dims* d) { return tile_pitch(std::max(d->in_dim, d->hidden_dim)); }

static size_t lds_bytes(const beso_mlp_dims* d) {
    return (size_t)(d->n_hidden + 2) * kRows * pitch_of(d) * sizeof(float);
}

// `sigma_col`: the rows end in the c_noise column, which d->in_dim counts
static int check_guide(const beso_mlp_dims* d, int obs, int adim, int use_goal, int sigma_col) {
    if (!d) return BESO_ERR_BAD_ARG;
    if (d->out_dim != 1 || d->n_hidden < 1 || d->n_hidden > kMaxLinear - 1) return BESO_ERR_BAD_SHAPE;
    if (obs < 1 || adim < 1 || obs > kMaxDim || adim > kMaxDim) return BESO_ERR_BAD_SHAPE;
    if (d->in_dim != obs + adim + (use_goal ? obs : 0) + (sigma_col ? 1 : 0)) return BESO_ERR_BAD_SHAPE;
    const int st = check_common(d->in_dim, d->hidden_dim, 1, d->activation, 1);       // M is the apply call's to check
    // the LDS ceiling is a shape error, and like every shape error it ranks above a bad activation
    if (st == BESO_ERR_BAD_SHAPE || lds_bytes(d) > kMaxLds) return BESO_ERR_BAD_SHAPE;
    return st;
}

// beso_guide_apply (SIGMA = false, c_noise unused) and beso_guide_apply_sigma: every check, then the one launch
template <bool SIGMA>
static int guide_apply(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state, const float* goal,
                       const float* pred, const float* sigma, const float* c_noise, int B, int T, int state_steps, int goal_steps,
                       int goal_rows, int obs_dim, int act_dim, float lam, float* out, void* stream) {
    int st = check_guide(dims, obs_dim, act_dim, goal != nullptr, SIGMA);
    if (st != BESO_OK) return st;
    if (B < 1 || T < 1 || state_steps < T) return BESO_ERR_BAD_SHAPE;
    const long long M = (long long)B * T;
    if (M > 0x7fffffffLL) return BESO_ERR_BAD_SHAPE;
    if (!GoalRows::valid(goal, goal_steps, goal_rows, B)) return BESO_ERR_BAD_SHAPE;
    if (check_params(params, n_params, 2 * (dims->n_hidden + 1)) != BESO_OK) return BESO_ERR_BAD_ARG;
    if (!state || !pred || !sigma || !out || misaligned(state, 4) || misaligned(goal, 4) || misaligned(pred, 4) ||
        misaligned(sigma, 4) || misaligned(out, 4))
        return BESO_ERR_BAD_ARG;
    if (SIGMA && (!c_noise || misaligned(c_noise, 4))) return BESO_ERR_BAD_ARG;

    Guide gd{};
    for (int l = 0; l <= dims->n_hidden; ++l) {
        gd.w[l] = params[2 * l];
        gd.b[l] = params[2 * l + 1];
    }
    gd.state = state;
    gd.goal = goal;
    gd.pred = pred;
    gd.sigma = sigma;
    gd.out = out;
    gd.n_hidden = dims->n_hidden;
    gd.in_dim = dims->in_dim;
    gd.hidden = dims->hidden_dim;
    gd.act = dims->activation;
    gd.T = T;
    gd.state_steps = state_steps;
    gd.obs = obs_dim;
    gd.adim = act_dim;
    const GoalRows g(goal, goal_steps, goal_rows, B, obs_dim);
    gd.goal_stride = g.stride;
    gd.goal_off = g.off;
    gd.lam = lam;

    return to_status(launch_lds_attr<guide_apply_kernel<SIGMA>>(kMaxLds, dim3(tile_grid(M)), dim3(kThreads), lds_bytes(dims),
                                                                (hipStream_t)stream, gd, M, pitch_of(dims), c_noise));
}

}  // namespace beso_guide
