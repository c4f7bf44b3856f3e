// Value-ranked best-of-K action selection for rollout inference (include/beso_rank.h): libbeso_rank.so.  One kernel behind the
// sampler call on N K rows:
//   rank_candidates_kernel   a workgroup per environment assembles its K rows [state | candidate action | goal] 16 at a time in
//                            LDS (the row layout of guide_tile.h), carries each tile forward through the MLPNetwork with the two
//                            LDS tiles of mlp_fwd_kernel (encoder.hip), keeps the K scalars q in LDS, takes their argmax and
//                            writes the chosen window (the write-back of candidates_select_kernel, select.hip)
// fp32 on v_mfma_f32_16x16x4_f32 through tile_xwt of mlp_tile.h.  Forward only: no keep buffer, no workspace, no atomics.
#include "mlp_tile.h"
#include "side_host.h"
#include "../../include/beso_rank.h"

namespace beso_rank {

using namespace beso_mlp;
using namespace beso_side;

constexpr int kMaxLinear = 5;      // n_hidden <= 4

struct Rank {
    const float* w[kMaxLinear];
    const float* b[kMaxLinear];
    const float *state, *goal, *x0_k;
    const int* lengths;
    float *x0, *scores;
    int* index;
    int n_hidden, in_dim, hidden, act;
    int W, obs, adim, K;
    long long goal_stride, goal_off;           // floats between two environments' goals (0: one shared goal) and to step G - 1
};

__device__ __forceinline__ int clamp_len(int len, int W) { return len < 1 ? 1 : (len > W ? W : len); }

// act_fwd, with a NaN pre-activation kept (act_fwd's ReLU is `z > 0 ? z : 0`, which turns a NaN into 0: a candidate with a NaN
// action would then score like a finite one)
__device__ __forceinline__ float act_keep_nan(int act, float z) { return z != z ? z : act_fwd(act, z); }

// Does candidate (s, k) take the place of (best, at)?  A NaN loses to every other score; among equal scores, and among NaNs, the
// lower k wins.  `at` == 0x7fffffff with a NaN `best` is a lane without a candidate: it loses to every candidate.
__device__ __forceinline__ bool takes(float s, int k, float best, int at) {
    const bool sn = s != s, bn = best != best;
    if (sn != bn) return bn;
    if (sn) return k < at;
    return s > best || (s == best && k < at);
}

// LDS: two tiles [16][pitch], the scores [K], the chosen index
__host__ __device__ inline size_t rank_lds_floats(int pitch, int K) { return 2 * (size_t)kRows * pitch + K + 4; }

__global__ __launch_bounds__(kThreads) void rank_candidates_kernel(Rank rk, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sc = lds + 2 * kRows * pitch;
    int* chosen = reinterpret_cast<int*>(sc + rk.K);
    const int n = blockIdx.x, tid = threadIdx.x;
    const int H = rk.hidden, I = rk.in_dim, L = rk.n_hidden, act = rk.act;
    const int obs = rk.obs, adim = rk.adim, K = rk.K;
    const int n_act = rk.W * adim;
    const int slot = clamp_len(rk.lengths[n], rk.W) - 1;
    const float* rows = rk.x0_k + (size_t)n * K * n_act;              // environment n's K sampled windows
    const float* st = rk.state + ((size_t)n * rk.W + slot) * obs;
    const float* gl = rk.goal ? rk.goal + (size_t)n * rk.goal_stride + rk.goal_off : nullptr;
    const int wp = round16(I);

    for (int m0 = 0; m0 < K; m0 += kRows) {
        float* cur = lds;
        float* nxt = lds + kRows * pitch;
        // the input rows, column by column from their three sources; rows >= K and columns [I, round16(I)) are 0
        for (int i = tid; i < kRows * wp; i += kThreads) {
            const int r = i / wp, c = i - r * wp;
            const int k = m0 + r;
            float v = 0.f;
            if (k < K && c < I) {
                if (c < obs) v = st[c];
                else if (c < obs + adim) v = rows[(size_t)k * n_act + slot * adim + (c - obs)];
                else v = gl[c - obs - adim];
            }
            cur[r * pitch + c] = v;
        }
        __syncthreads();
        for (int l = 0; l < L; ++l) {
            const float* bias = rk.b[l];
            tile_xwt(cur, pitch, rk.w[l], H, l == 0 ? I : H, [&](int r, int c, float v) { nxt[r * pitch + c] = act_keep_nan(act, v + bias[c]); });
            __syncthreads();
            float* t = cur;
            cur = nxt;
            nxt = t;
        }
        const float* bias = rk.b[L];
        tile_xwt(cur, pitch, rk.w[L], 1, H, [&](int r, int c, float v) {
            if (m0 + r < K) sc[m0 + r] = v + bias[0];
        });
        __syncthreads();                                              // the next tile's rows go where this one's were read
    }

    for (int k = tid; k < K; k += kThreads) rk.scores[(size_t)n * K + k] = sc[k];

    // argmax, the lowest k among equal scores: every lane of the first wave scans k = lane, lane + 64, ... upward, then the
    // lanes meet in a butterfly (`takes` is a strict total order on (score, k): every lane ends with the same pair)
    if (tid < beso::kWave) {
        float best = __builtin_nanf("");
        int at = 0x7fffffff;                                          // (a lane without a candidate: K < 64)
        for (int k = tid; k < K; k += beso::kWave) {
            const float s = sc[k];
            if (takes(s, k, best, at)) {
                best = s;
                at = k;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, beso::kWave);
            const int oa = __shfl_xor(at, o, beso::kWave);
            if (takes(ob, oa, best, at)) {
                best = ob;
                at = oa;
            }
        }
        if (tid == 0) {
            at = at < 0 ? 0 : (at >= K ? K - 1 : at);                 // (lane 0 owns candidate 0: `at` is in range already)
            *chosen = at;
            rk.index[n] = at;
        }
    }
    __syncthreads();
    const float* win = rows + (size_t)(*chosen) * n_act;
    float* out = rk.x0 + (size_t)n * n_act;
    for (int e = tid; e < n_act; e += kThreads) out[e] = win[e];
}

// ------------------------------------------------------------------------------------------------------------ host
static int pitch_of(const beso_mlp_dims* d) { return tile_pitch(std::max(d->in_dim, d->hidden_dim)); }

constexpr size_t kLdsMax = 2 * kTileBytes + (BESO_RANK_MAX_K + 4) * sizeof(float);

// the network and its row layout: what beso_rank_supported answers, for `fn`'s message
static int check_network(const char* fn, const beso_mlp_dims* d, int obs, int adim, int use_goal) {
    if (!d) return refuse(BESO_ERR_BAD_ARG, "%s: dims is NULL", fn);
    if (adim < 1 || adim > BESO_RANK_MAX_ACT)
        return refuse(BESO_ERR_UNSUPPORTED, "%s: act_dim = %d, supported: 1 ... %d", fn, adim, BESO_RANK_MAX_ACT);
    if (obs < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: obs_dim = %d must be at least 1", fn, obs);
    if (d->out_dim != 1)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: out_dim = %d: the network must give one scalar q per row (out_dim == 1)", fn, d->out_dim);
    if (d->n_hidden < 1 || d->n_hidden > kMaxLinear - 1)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: n_hidden = %d, supported: 1 ... %d", fn, d->n_hidden, kMaxLinear - 1);
    const long long want = (long long)obs + adim + (use_goal ? obs : 0);
    if (d->in_dim != want)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: in_dim = %d, but obs_dim + act_dim%s = %lld", fn, d->in_dim, use_goal ? " + obs_dim" : "", want);
    const int st = check_common(d->in_dim, d->hidden_dim, 1, d->activation, 1);
    if (st == BESO_ERR_BAD_SHAPE)
        return refuse(st, "%s: in_dim = %d (1 ... %d) or hidden_dim = %d (a multiple of 16 up to %d) is outside what beso_mlp_fwd supports", fn,
                      d->in_dim, kMaxDim, d->hidden_dim, kMaxDim);
    if (st != BESO_OK) return refuse(st, "%s: activation = %d is not a BESO_MLP_ACT_* value", fn, d->activation);
    return BESO_OK;
}

}  // namespace beso_rank

using namespace beso_rank;

extern "C" const char* beso_rank_last_error(void) { return g_error; }

extern "C" int beso_rank_supported(const beso_mlp_dims* dims, int obs_dim, int act_dim, int use_goal) {
    return check_network("beso_rank_supported", dims, obs_dim, act_dim, use_goal);
}

extern "C" int beso_rank_candidates(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* state,
                                    const float* goal, int goal_steps, int goal_rows, const float* x0_k, const int32_t* lengths,
                                    int N, int W, int obs_dim, int act_dim, int K, float* x0, int32_t* index, float* scores,
                                    void* stream) {
    const char* fn = "beso_rank_candidates";
    if (K < 1 || K > BESO_RANK_MAX_K)
        return refuse(BESO_ERR_UNSUPPORTED, "%s: K = %d candidates per environment, supported: 1 ... %d", fn, K, BESO_RANK_MAX_K);
    const int st = check_network(fn, dims, obs_dim, act_dim, goal != nullptr);
    if (st != BESO_OK) return st;
    if (N < 1 || W < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: N = %d and W = %d must be at least 1", fn, N, W);
    if ((long long)W * act_dim > 0x7fffffffLL || (long long)W * obs_dim > 0x7fffffffLL || (long long)N * K > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: W act_dim = %lld / W obs_dim = %lld floats per row or N K = %lld rows exceed the int range", fn,
                      (long long)W * act_dim, (long long)W * obs_dim, (long long)N * K);
    if (!GoalRows::valid(goal, goal_steps, goal_rows, N))
        return refuse(BESO_ERR_BAD_SHAPE, "%s: goal_steps = %d, goal_rows = %d: a goal is [N = %d or 1, goal_steps >= 1, obs_dim], and both are 0 without one",
                      fn, goal_steps, goal_rows, N);
    if (check_params(params, n_params, 2 * (dims->n_hidden + 1)) != BESO_OK)
        return refuse(BESO_ERR_BAD_ARG, "%s: params must be %d non-NULL 4-byte aligned device pointers, n_params = %d", fn,
                      2 * (dims->n_hidden + 1), n_params);
    if (!state || !x0_k || !lengths || !x0 || !index || !scores) return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer", fn);
    if (misaligned(state, 4) || misaligned(goal, 4) || misaligned(x0_k, 4) || misaligned(lengths, 4) || misaligned(x0, 4) || misaligned(index, 4) ||
        misaligned(scores, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: a pointer that is not 4-byte aligned", fn);

    Rank rk{};
    for (int l = 0; l <= dims->n_hidden; ++l) {
        rk.w[l] = params[2 * l];
        rk.b[l] = params[2 * l + 1];
    }
    rk.state = state;
    rk.goal = goal;
    rk.x0_k = x0_k;
    rk.lengths = (const int*)lengths;
    rk.x0 = x0;
    rk.scores = scores;
    rk.index = (int*)index;
    rk.n_hidden = dims->n_hidden;
    rk.in_dim = dims->in_dim;
    rk.hidden = dims->hidden_dim;
    rk.act = dims->activation;
    rk.W = W;
    rk.obs = obs_dim;
    rk.adim = act_dim;
    rk.K = K;
    const GoalRows g(goal, goal_steps, goal_rows, N, obs_dim);
    rk.goal_stride = g.stride;
    rk.goal_off = g.off;

    const int pitch = pitch_of(dims);
    const hipError_t e = launch_lds_attr<rank_candidates_kernel>(kLdsMax, dim3((unsigned)N), dim3(kThreads),
                                                                 rank_lds_floats(pitch, K) * sizeof(float), (hipStream_t)stream, rk, pitch);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}
