// Best-of-K action selection for rollout inference (include/beso_select.h): libbeso_select.so.  Two kernels around one sampler
// call on N K rows:
//   candidates_expand_kernel   a workgroup per output row n K + k copies environment n's state / x window and puts
//                              noise[n, k, :] * sigma_max into the newest slot of x
//   candidates_select_kernel   a workgroup per environment holds its K newest-slot actions in LDS, forms their mean or their
//                              kernel-density scores and argmax, and writes the chosen window
// Copy work and a K x K x act loop: no MFMA, no atomics, no workspace, every sum sequential in a fixed order.
#include "side_host.h"
#include "../../include/beso_select.h"

#include <cmath>

namespace beso_select {

using namespace beso_side;

using beso::f32x4;

constexpr int kThreads = 256;

// ------------------------------------------------------------------------------------------------------------ expand
// One window of one output row: dst[e] = src[e], except dst[e] = nz[e - lo] * smax for e in [lo, hi) (lo == hi: a plain copy).
// VEC: n is a multiple of 4 and both pointers are 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void copy_window(const float* __restrict__ src, float* __restrict__ dst, int n, int lo, int hi,
                                            const float* __restrict__ nz, float smax) {
    if (VEC) {
        for (int q = threadIdx.x; q < n / 4; q += kThreads) {
            f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int e = 4 * q + c;
                if (e >= lo && e < hi) v[c] = nz[e - lo] * smax;
            }
            reinterpret_cast<f32x4*>(dst)[q] = v;
        }
    } else {
        for (int e = threadIdx.x; e < n; e += kThreads) dst[e] = e >= lo && e < hi ? nz[e - lo] * smax : src[e];
    }
}

__device__ __forceinline__ int clamp_len(int len, int W) { return len < 1 ? 1 : (len > W ? W : len); }

template <bool VEC_S, bool VEC_X>
__global__ __launch_bounds__(kThreads) void candidates_expand_kernel(
    const float* __restrict__ state, const float* __restrict__ x, const int* __restrict__ lengths,
    const float* __restrict__ noise, float sigma_max, int W, int obs, int act, int K, float* __restrict__ state_k,
    float* __restrict__ x_k) {
    const int row = blockIdx.x;                         // n K + k
    const int n = row / K;
    const int n_obs = W * obs, n_act = W * act;
    const int slot = clamp_len(lengths[n], W) - 1;
    copy_window<VEC_S>(state + (size_t)n * n_obs, state_k + (size_t)row * n_obs, n_obs, 0, 0, nullptr, 0.f);
    copy_window<VEC_X>(x + (size_t)n * n_act, x_k + (size_t)row * n_act, n_act, slot * act, (slot + 1) * act,
                       noise + (size_t)row * act, sigma_max);
}

// ------------------------------------------------------------------------------------------------------------ select
// LDS: the candidates [K][pitch] (pitch odd: thread k walking its own row beside thread k + 1 meets no bank twice), h [act],
// the scores [K] and the chosen index.
__host__ __device__ inline int cand_pitch(int act) { return act | 1; }
__host__ __device__ inline size_t select_lds_floats(int K, int act) { return (size_t)K * cand_pitch(act) + act + K + 4; }

__global__ __launch_bounds__(kThreads) void candidates_select_kernel(
    const float* __restrict__ x0_k, const int* __restrict__ lengths, int mode, float bandwidth, double scott, int W, int act,
    int K, float* __restrict__ x0, int* __restrict__ index, float* __restrict__ scores) {
#pragma clang fp contract(off)          // the sums below are stated operation by operation (include/beso_select.h)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int pitch = cand_pitch(act);
    float* cand = lds;
    float* h = cand + (size_t)K * pitch;                // KDE: the bandwidths; mean: the mean action
    float* sc = h + act;
    int* chosen = reinterpret_cast<int*>(sc + K);
    const int n = blockIdx.x, tid = threadIdx.x;
    const int n_act = W * act;
    const int slot = clamp_len(lengths[n], W) - 1;
    const float* rows = x0_k + (size_t)n * K * n_act;   // environment n's K sampled windows

    for (int i = tid; i < K * act; i += kThreads) {
        const int k = i / act, d = i - k * act;
        cand[k * pitch + d] = rows[(size_t)k * n_act + slot * act + d];
    }
    __syncthreads();

    // per component: the mean action as ONE running fp32 sum over k = 0 ... K-1 (the contract of BESO_SELECT_MEAN), or the
    // bandwidth -- for Scott's rule from the population deviation, whose two sums run in fp64 (2 K additions per component;
    // the scores inherit every error of h)
    if (tid < act) {
        if (mode == BESO_SELECT_MEAN) {
            float sum = cand[tid];
            for (int k = 1; k < K; ++k) sum = sum + cand[k * pitch + tid];
            h[tid] = sum / (float)K;
        } else if (bandwidth > 0.f) {
            h[tid] = bandwidth;
        } else {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum += (double)cand[k * pitch + tid];
            const double mu = sum / K;
            double ss = 0.0;
            for (int k = 0; k < K; ++k) {
                const double dv = (double)cand[k * pitch + tid] - mu;
                ss += dv * dv;
            }
            const double sd = sqrt(ss / K);
            const double floor_ = 1e-6 * fmax(1.0, fabs(mu));
            h[tid] = (float)((sd > floor_ ? sd : floor_) * scott);      // (a NaN deviation takes the floor: the scores decide nothing then)
        }
    }
    __syncthreads();

    float* out = x0 + (size_t)n * n_act;
    if (mode == BESO_SELECT_MEAN) {
        for (int e = tid; e < n_act; e += kThreads) {
            const int j = e / act;
            out[e] = j == slot ? h[e - j * act] : rows[e];
        }
        for (int k = tid; k < K; k += kThreads) scores[(size_t)n * K + k] = 0.f;
        if (tid == 0) index[n] = -1;
        return;
    }

    // s_k = log sum_j exp(-q_kj / 2): thread k owns candidate k, j runs in order (the reads of row j are broadcasts)
    for (int k = tid; k < K; k += kThreads) {
        const float* ck = cand + k * pitch;
        double sum = 0.0;                               // (K terms in (0, 1]: fp64 keeps the sum's error out of the score)
        for (int j = 0; j < K; ++j) {
            const float* cj = cand + j * pitch;
            float q = 0.f;
            for (int d = 0; d < act; ++d) {
                const float z = (ck[d] - cj[d]) / h[d];
                q = q + z * z;
            }
            sum += (double)expf(-0.5f * q);
        }
        const float s = logf((float)sum);
        sc[k] = s;
        scores[(size_t)n * K + k] = s;
    }
    __syncthreads();

    // argmax, the lowest k among equal scores: every lane of the first wave scans k = lane, lane + 64, ... upward, then the
    // lanes meet in a butterfly.  "Greater" and "equal" are both false against a NaN, so a NaN is never taken over another
    // lane's value and never given up either; whatever lane 0 ends with is the index of a candidate.
    if (tid < beso::kWave) {
        float best = -INFINITY;
        int at = 0x7fffffff;                            // (a lane without a candidate: K < 64)
        if (tid < K) {
            best = sc[tid];
            at = tid;
            for (int k = tid + beso::kWave; k < K; k += beso::kWave) {
                const float s = sc[k];
                if (s > best) {
                    best = s;
                    at = k;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, beso::kWave);
            const int oa = __shfl_xor(at, o, beso::kWave);
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        if (tid == 0) {
            at = at < 0 ? 0 : (at >= K ? K - 1 : at);   // (lane 0 owns candidate 0: `at` is in range already)
            *chosen = at;
            index[n] = at;
        }
    }
    __syncthreads();
    const float* win = rows + (size_t)(*chosen) * n_act;
    for (int e = tid; e < n_act; e += kThreads) out[e] = win[e];
}

// ------------------------------------------------------------------------------------------------------------ host
static bool aligned16(const void* p) { return !misaligned(p, 16); }

}  // namespace beso_select

using namespace beso_select;

extern "C" const char* beso_candidates_last_error(void) { return g_error; }

extern "C" int beso_candidates_expand(const float* state, const float* x, const int32_t* lengths, const float* noise,
                                      float sigma_max, int N, int W, int obs_dim, int act_dim, int K, float* state_k,
                                      float* x_k, void* stream) {
    const char* fn = "beso_candidates_expand";
    if (N < 1 || W < 1 || obs_dim < 1 || act_dim < 1 || K < 1)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: N = %d, W = %d, obs_dim = %d, act_dim = %d, K = %d must all be at least 1", fn, N, W,
                      obs_dim, act_dim, K);
    if ((long long)N * K > 0x7fffffffLL || (long long)W * obs_dim > 0x7fffffffLL || (long long)W * act_dim > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: N K = %lld rows or W obs_dim = %lld / W act_dim = %lld floats per row exceed the int range",
                      fn, (long long)N * K, (long long)W * obs_dim, (long long)W * act_dim);
    if (!state || !x || !lengths || !noise || !state_k || !x_k) return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer", fn);
    if (misaligned(state, 4) || misaligned(x, 4) || misaligned(lengths, 4) || misaligned(noise, 4) || misaligned(state_k, 4) || misaligned(x_k, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: a pointer that is not 4-byte aligned", fn);
    const bool vs = (W * obs_dim) % 4 == 0 && aligned16(state) && aligned16(state_k);
    const bool vx = (W * act_dim) % 4 == 0 && aligned16(x) && aligned16(x_k);
    const dim3 grid((unsigned)(N * K)), block(kThreads);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
#define BESO_EXPAND(VS, VX) \
    beso::launch_plain<candidates_expand_kernel<VS, VX>>(grid, block, s, state, x, (const int*)lengths, noise, sigma_max, W, obs_dim, act_dim, K, state_k, x_k)
    if (vs && vx) e = BESO_EXPAND(true, true);
    else if (vs) e = BESO_EXPAND(true, false);
    else if (vx) e = BESO_EXPAND(false, true);
    else e = BESO_EXPAND(false, false);
#undef BESO_EXPAND
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}

extern "C" int beso_candidates_select(const float* x0_k, const int32_t* lengths, int mode, float bandwidth, int N, int W,
                                      int act_dim, int K, float* x0, int32_t* index, float* scores, void* stream) {
    const char* fn = "beso_candidates_select";
    if (K < 1 || K > BESO_SELECT_MAX_K)
        return refuse(BESO_ERR_UNSUPPORTED, "%s: K = %d candidates per environment, supported: 1 ... %d", fn, K, BESO_SELECT_MAX_K);
    if (act_dim < 1 || act_dim > BESO_SELECT_MAX_ACT)
        return refuse(BESO_ERR_UNSUPPORTED, "%s: act_dim = %d, supported: 1 ... %d (the candidates live in LDS)", fn, act_dim,
                      BESO_SELECT_MAX_ACT);
    if (N < 1 || W < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: N = %d and W = %d must be at least 1", fn, N, W);
    if ((long long)W * act_dim > 0x7fffffffLL || (long long)N * K > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: W act_dim = %lld floats per row or N K = %lld rows exceed the int range", fn,
                      (long long)W * act_dim, (long long)N * K);
    if (mode != BESO_SELECT_MEAN && mode != BESO_SELECT_KDE)
        return refuse(BESO_ERR_BAD_ARG, "%s: mode %d is neither BESO_SELECT_MEAN nor BESO_SELECT_KDE", fn, mode);
    if (mode == BESO_SELECT_KDE && std::isnan(bandwidth)) return refuse(BESO_ERR_BAD_ARG, "%s: the bandwidth is NaN", fn);
    if (!x0_k || !lengths || !x0 || !index || !scores) return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer", fn);
    if (misaligned(x0_k, 4) || misaligned(lengths, 4) || misaligned(x0, 4) || misaligned(index, 4) || misaligned(scores, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: a pointer that is not 4-byte aligned", fn);
    const double scott = std::pow((double)K, -1.0 / (double)(act_dim + 4));
    const size_t lds = select_lds_floats(K, act_dim) * sizeof(float);
    const size_t lds_max = select_lds_floats(BESO_SELECT_MAX_K, BESO_SELECT_MAX_ACT) * sizeof(float);
    const hipError_t e = beso::launch_lds_attr<candidates_select_kernel>(
        lds_max, dim3((unsigned)N), dim3(kThreads), lds, (hipStream_t)stream, x0_k, (const int*)lengths, mode, bandwidth, scott, W,
        act_dim, K, x0, (int*)index, scores);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}
