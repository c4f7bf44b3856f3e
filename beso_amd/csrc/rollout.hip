// Vectorised rollout: the window bookkeeping of BesoAgent.predict (reference agents/diffusion_agents/beso_agent.py:296-388)
// for N environments whose episodes start and end independently, on contexts that live in HBM.
//
//   lengths [N] int32                 observations in environment n's window (0 ... W)
//   obs_ctx [N][W][obs]               the scaled observations: the reference's deque(maxlen = W)
//   act_ctx [N][W][act]               the clipped actions in the scaled domain, slot j beside observation slot j: the
//                                     reference's deque(maxlen = W - 1) (slot t - 1 is the action the step is about to draw)
//
// rollout_begin_kernel (one workgroup per environment) appends the step's observation and writes the sampler's inputs as FULL
// W-slot windows, the unused slots behind the t valid ones zero: attention is causal and positions belong to slots, so the
// tokens of slots < t never see the padding.  rollout_end_kernel (one thread per action component) takes the
// newest action out of the sampler's result, clips it, remembers it and un-scales it.  Copy work of a few KiB per call.
#include "common.h"

namespace beso {
namespace {

constexpr int kRolloutThreads = 128;

// The full-window case moves every slot down by one IN PLACE.  The workgroup walks its environment's elements (the obs
// context, then the action context) in chunks of blockDim.x in rising order; every thread loads its element's new value, the
// workgroup meets at a barrier, and then the values are stored.  A store of chunk c goes to an index below (c + 1) blockDim.x
// of its array and every later load comes from an index above that (the source of element e is e + one row), so nothing
// is read after the same launch has overwritten it.
__global__ __launch_bounds__(kRolloutThreads) void rollout_begin_kernel(
    const float* __restrict__ obs_in, const unsigned char* __restrict__ reset, const float* __restrict__ noise,
    const float* __restrict__ mean, const float* __restrict__ den, float sigma_max, int* __restrict__ lengths,
    float* obs_ctx, float* act_ctx, float* __restrict__ state_out, float* __restrict__ x_out, int W, int obs, int act) {
    const int n = blockIdx.x;
    int len = lengths[n];
    if (reset && reset[n]) len = 0;
    len = len < 0 ? 0 : (len > W ? W : len);            // (a length the caller never wrote must not index out of the window)
    const bool shift = len == W;                        // deque(maxlen): the oldest slot leaves
    const int t = shift ? W : len + 1;                  // observations in the window after the append
    const int n_obs = W * obs, n_act = W * act;
    float* oc = obs_ctx + (size_t)n * n_obs;
    float* ac = act_ctx + (size_t)n * n_act;
    float* so = state_out + (size_t)n * n_obs;
    float* xo = x_out + (size_t)n * n_act;
    for (int base = 0; base < n_obs + n_act; base += kRolloutThreads) {
        const int i = base + (int)threadIdx.x;
        float v = 0.f;
        bool keep = false;                              // the value also goes back into the context
        if (i < n_obs) {
            const int j = i / obs, c = i - j * obs;
            if (j == t - 1) {
                const float raw = obs_in[(size_t)n * obs + c];
                if (mean) {                             // Scaler.scale_input: a subtraction and a correctly rounded division
                    const float d = raw - mean[c];
                    v = d / den[c];
                } else {
                    v = raw;
                }
                keep = true;
            } else if (j < t - 1) {
                v = oc[shift ? i + obs : i];
                keep = shift;
            }
        } else if (i < n_obs + n_act) {
            const int e = i - n_obs;
            const int j = e / act, c = e - j * act;
            if (j == t - 1) {
                v = noise[(size_t)n * act + c] * sigma_max;       // torch.randn(...) * self.sigma_max
            } else if (j < t - 1) {
                v = ac[shift ? e + act : e];
                keep = shift;
            }
        }
        __syncthreads();
        if (i < n_obs) {
            so[i] = v;
            if (keep) oc[i] = v;
        } else if (i < n_obs + n_act) {
            xo[i - n_obs] = v;
            if (keep) ac[i - n_obs] = v;
        }
    }
    __syncthreads();                                    // (every thread has read lengths[n])
    if (threadIdx.x == 0) lengths[n] = t;
}

__global__ __launch_bounds__(256) void rollout_end_kernel(
    const float* __restrict__ x0, const int* __restrict__ lengths, const double* __restrict__ lo, const double* __restrict__ hi,
    const float* __restrict__ den_y, const float* __restrict__ mean_y, float* __restrict__ act_ctx, float* __restrict__ pred,
    int n_envs, int W, int act) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_envs * act) return;
    const int n = i / act, c = i - n * act;
    int t = lengths[n];
    t = t < 1 ? 1 : (t > W ? W : t);
    const size_t at = ((size_t)n * W + (t - 1)) * act + c;
    // Scaler.clip_action: torch.clamp of the fp32 action against float64 bounds promotes to float64; the result is rounded
    // to fp32.  (NaN compares false twice and passes through, as clamp propagates it.)
    double v = (double)x0[at];
    if (v < lo[c]) v = lo[c];
    if (v > hi[c]) v = hi[c];
    const float clipped = (float)v;
    act_ctx[at] = clipped;
    float p = clipped;
    if (den_y) {
#pragma clang fp contract(off)          // Scaler.inverse_scale_output: y * den + mean as two rounded operations
        const float m = clipped * den_y[c];
        p = m + mean_y[c];
    }
    pred[i] = p;
}

}  // namespace

hipError_t launch_rollout_begin(const float* obs_in, const unsigned char* reset, const float* noise, const float* mean,
                                const float* den, float sigma_max, int* lengths, float* obs_ctx, float* act_ctx,
                                float* state_out, float* x_out, int n_envs, int W, int obs, int act, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(rollout_begin_kernel, dim3(n_envs), dim3(kRolloutThreads), 0, s, obs_in, reset, noise, mean, den,
                       sigma_max, lengths, obs_ctx, act_ctx, state_out, x_out, W, obs, act);
    return hipGetLastError();
}

hipError_t launch_rollout_end(const float* x0, const int* lengths, const double* lo, const double* hi, const float* den_y,
                              const float* mean_y, float* act_ctx, float* pred, int n_envs, int W, int act, hipStream_t s) {
    (void)hipGetLastError();
    const int total = n_envs * act;
    hipLaunchKernelGGL(rollout_end_kernel, dim3((total + 255) / 256), dim3(256), 0, s, x0, lengths, lo, hi, den_y, mean_y,
                       act_ctx, pred, n_envs, W, act);
    return hipGetLastError();
}

}  // namespace beso
