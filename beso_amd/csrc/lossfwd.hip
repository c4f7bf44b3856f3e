// The gradient-free score-matching objective (reference k_diffusion/score_wrappers.py:45-79 under torch.no_grad()): the
// held-out loss of the eval-mode network, per sample and as a scalar, on the INFERENCE path.  beso_loss_fwd (api.hip) enqueues
//
//   loss_prep_kernel   scaled = (action + noise * sigma) * c_in                              elementwise over [B, t, act]
//   the forward        pred = F(state, scaled, goal, sigma): beso_score_fwd's kernels, whatever plan the library picks
//   loss_rows_kernel   per_sample[b] = mean over the scored elements of (pred - target)^2    one wave per sample
//   loss_mean_kernel   loss = sum_b per_sample[b] / B                                        ONE workgroup
//
// F(c_in * noised) is compared with the target, the reference's operation order: forming (D - action) / c_out from the
// preconditioned output would subtract two numbers that agree to several digits at sigma ~ sigma_min and divide by c_out ~ 1e-3.
// The target is not stored: loss_rows_kernel recomputes noised and target from action, noise and sigma with the expressions of
// prep_kernel (train_rows.h), every product, quotient and sum rounded on its own as torch rounds them.  Both reductions run in a
// fixed order and there is no atomic: two runs give equal bits wherever the forward does, and per_sample[b] depends on sample
// b's values only.
#include "common.h"

namespace beso {
namespace {

constexpr int kLossPrepThreads = 256;
constexpr int kLossRowWaves = 4;              // samples (waves) per workgroup of loss_rows_kernel
constexpr int kLossMeanThreads = 256;

__global__ __launch_bounds__(kLossPrepThreads) void loss_prep_kernel(
    const float* __restrict__ action, const float* __restrict__ noise, const float* __restrict__ sigma,
    float* __restrict__ scaled, int per_sample, size_t n, float sigma_data) {
#pragma clang fp contract(off)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float sg = sigma[i / per_sample];
        const float sd2 = sigma_data * sigma_data, den = sg * sg + sd2;
        const float c_in = 1.0f / sqrtf(den);
        const float p = noise[i] * sg;
        const float nz = action[i] + p;
        scaled[i] = nz * c_in;
    }
}

// One wave per sample.  Lane l walks elements first + l, first + l + 64, ... of the sample's scored range -- all t * act
// values, or the last row's act values with last_only -- and the wave's partial sums meet in wave_sum_dpp's fixed order.
__global__ __launch_bounds__(kLossRowWaves * kWave) void loss_rows_kernel(
    const float* __restrict__ pred, const float* __restrict__ action, const float* __restrict__ noise,
    const float* __restrict__ sigma, float* __restrict__ per_sample, int batch, int per, int first, float sigma_data) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * kLossRowWaves + (int)(threadIdx.x >> 6);       // (uniform in the wave)
    if (b >= batch) return;
    const float sg = sigma[b];
    const float sd2 = sigma_data * sigma_data, den = sg * sg + sd2;
    const float c_skip = sd2 / den, c_out = sg * sigma_data / sqrtf(den);
    const size_t base = (size_t)b * per;
    float acc = 0.f;
    for (int e = first + lane; e < per; e += kWave) {
        const float a = action[base + e];
        const float p = noise[base + e] * sg;
        const float nz = a + p;
        const float q = c_skip * nz;
        const float target = (a - q) / c_out;
        const float diff = pred[base + e] - target;
        const float sq = diff * diff;
        acc = acc + sq;
    }
    const float total = wave_sum_dpp(acc);
    if (lane == 0) per_sample[b] = total / (float)(per - first);
}

// ONE workgroup: thread i adds per_sample[i], per_sample[i + 256], ... in rising order, then a fixed tree through LDS.
__global__ __launch_bounds__(kLossMeanThreads) void loss_mean_kernel(const float* __restrict__ per_sample, float* __restrict__ loss,
                                                                     int batch) {
#pragma clang fp contract(off)
    __shared__ float part[kLossMeanThreads];
    float acc = 0.f;
    for (int i = threadIdx.x; i < batch; i += kLossMeanThreads) acc = acc + per_sample[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = kLossMeanThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = part[0] / (float)batch;
}

}  // namespace

hipError_t launch_loss_prep(const float* action, const float* noise, const float* sigma, float* scaled, int batch, int t, int act,
                            float sigma_data, hipStream_t s) {
    const size_t n = (size_t)batch * t * act;
    const size_t blocks = (n + kLossPrepThreads - 1) / kLossPrepThreads;
    (void)hipGetLastError();
    hipLaunchKernelGGL(loss_prep_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kLossPrepThreads), 0, s, action, noise,
                       sigma, scaled, t * act, n, sigma_data);
    return hipGetLastError();
}

hipError_t launch_loss_reduce(const float* pred, const float* action, const float* noise, const float* sigma, float* per_sample,
                              float* loss, int batch, int t, int act, int last_only, float sigma_data, hipStream_t s) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(loss_rows_kernel, dim3((batch + kLossRowWaves - 1) / kLossRowWaves), dim3(kLossRowWaves * kWave), 0, s, pred,
                       action, noise, sigma, per_sample, batch, t * act, last_only ? (t - 1) * act : 0, sigma_data);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !loss) return e;
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(kLossMeanThreads), 0, s, per_sample, loss, batch);
    return hipGetLastError();
}

}  // namespace beso
