// K11 + K12: one optimizer step over ALL parameter tensors in one launch, optionally followed by the EMA
// update on the freshly written parameter (beso_agent.py:236-244 -> torch.optim.AdamW / Adam,
// configs/agents/beso_kitchen.yaml:9-12, beso_block_push.yaml:9-11; ema.py:45-53).
//
// HBM bound: per element it reads p, g, m, v (+ema) and writes p, m, v (+ema) = 28 (36) bytes; the
// 9.4 M-parameter kitchen model is 0.34 GB per step, ~70 us at 5 TB/s, against one launch per tensor and
// per operation (several hundred launches) for the eager optimizer.  The arithmetic follows torch's
// single-tensor Adam(W) (amsgrad = False, maximize = False) operation by operation in fp32:
//     AdamW:  p *= 1 - lr*wd                      Adam:  g += wd*p
//     m = m + (g - m)*(1 - beta1)                 (Tensor.lerp_)
//     v = v*beta2 + (1 - beta2)*g*g               (mul_ + addcmul_)
//     denom = sqrt(v)/sqrt(1 - beta2^t) + eps;  p -= (lr/(1 - beta1^t)) * (m/denom)
//     ema -= (1 - decay)*(ema - p)                (the reference's EMA, on the updated p)
//
// Gradient clipping and the non-finite guard (beso_grad_sumsq + beso_adam_step_clipped): the global L2 norm of the
// gradient is reduced ON THE DEVICE over the same chunk table (grad_sumsq_kernel -> grad_sumsq_finish_kernel ->
// stats[0]) and consumed by the step launch with no host in between -- train_step returns before the backward has run,
// so a host-side isfinite / clip_grad_norm_ would bring the per-step synchronisation back.  The clipped step is a
// second kernel (adam_ema_clipped_kernel): adam_ema_kernel itself is what it was.
//     double stats[4] = { sumsq, norm (fp32 value), clip coefficient applied (0: step skipped), skipped steps so far }
#include "common.h"

namespace beso {

struct OptimChunk {          // == beso_optim_chunk (include/beso_hip.h)
    float* p;
    const float* g;
    unsigned long long off;  // element offset of the chunk in the flat state buffers (m, v, ema)
    unsigned int n;          // elements in the chunk
    unsigned int pad;
};
// chunks hold at most 4096 elements (beso_amd/optim.py); any count works

__global__ __launch_bounds__(256) void adam_ema_kernel(const OptimChunk* __restrict__ chunks, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, float lr,
                                                       float beta1, float beta2, float eps, float wd, int decoupled,
                                                       float step_size, float rsqrt_bc2_inv, float ema_decay) {
    const OptimChunk c = chunks[blockIdx.x];
    for (unsigned i = threadIdx.x; i < c.n; i += 256) {
        float p = c.p[i], g = c.g[i];
        float mi = m[c.off + i], vi = v[c.off + i];
        if (decoupled) p = p * (1.0f - lr * wd);
        else g = fmaf(wd, p, g);                       // grad.add(param, alpha=wd); wd = 0 leaves g untouched
        mi = mi + (g - mi) * (1.0f - beta1);
        vi = vi * beta2;
        vi = fmaf((1.0f - beta2) * g, g, vi);          // addcmul_(g, g, value = 1 - beta2)
        const float denom = sqrtf(vi) / rsqrt_bc2_inv + eps;
        p = p - step_size * (mi / denom);
        c.p[i] = p;
        m[c.off + i] = mi;
        v[c.off + i] = vi;
        if (ema) {
            const float s = ema[c.off + i];
            ema[c.off + i] = s - (1.0f - ema_decay) * (s - p);
        }
    }
}

// sum over the block's 256 threads in a fixed order: lanes (shuffle tree), then the four waves through LDS; the result
// is valid in thread 0
__device__ __forceinline__ double block_sum_256(double x, double* red) {
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per chunk row: partial[row] = sum g^2 of the row.  The square of an fp32 value is exact in double; the
// additions run in a fixed order (thread-strided, lanes, waves): no atomics, nothing depends on the launch order.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const OptimChunk* __restrict__ chunks, double* __restrict__ partial) {
    __shared__ double red[4];
    const OptimChunk c = chunks[blockIdx.x];
    double acc = 0.0;
    for (unsigned i = threadIdx.x; i < c.n; i += 256) {
        const double g = (double)c.g[i];
        acc += g * g;
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// one workgroup: stats[0] = sum of partial[0 .. n) in a fixed order (n = 0 writes 0)
__global__ __launch_bounds__(256) void grad_sumsq_finish_kernel(const double* __restrict__ partial, int n,
                                                                double* __restrict__ stats) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) stats[0] = acc;
}

// adam_ema_kernel with the gradient scaled in registers by clip_grad_norm_'s coefficient, min(1, max_norm / (norm + 1e-6)),
// of the global norm sqrt(stats[0]) -- the gradient buffer itself is left as it is -- and, with skip_nonfinite, a return
// before the first store when that norm is not finite (p, m, v and ema keep their bits).  Every workgroup reads stats[0],
// which no workgroup of this launch writes; thread 0 of workgroup 0 records the norm, the coefficient and the skip count.
__global__ __launch_bounds__(256) void adam_ema_clipped_kernel(const OptimChunk* __restrict__ chunks, float* __restrict__ m,
                                                               float* __restrict__ v, float* __restrict__ ema, float lr,
                                                               float beta1, float beta2, float eps, float wd, int decoupled,
                                                               float step_size, float rsqrt_bc2_inv, float ema_decay,
                                                               double* __restrict__ stats, float max_norm, int skip_nonfinite) {
    const double sumsq = stats[0];
    const float norm = (float)sqrt(sumsq);
    const bool skip = skip_nonfinite && !isfinite(sumsq);
    const float coef = skip ? 0.0f : fminf(1.0f, max_norm / (norm + 1e-6f));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[1] = (double)norm;
        stats[2] = (double)coef;
        if (skip) stats[3] = stats[3] + 1.0;
    }
    if (skip) return;
    const OptimChunk c = chunks[blockIdx.x];
    for (unsigned i = threadIdx.x; i < c.n; i += 256) {
        float p = c.p[i], g = __fmul_rn(c.g[i], coef);  // one rounded multiply, never contracted into what follows
        float mi = m[c.off + i], vi = v[c.off + i];
        if (decoupled) p = p * (1.0f - lr * wd);
        else g = fmaf(wd, p, g);
        mi = mi + (g - mi) * (1.0f - beta1);
        vi = vi * beta2;
        vi = fmaf((1.0f - beta2) * g, g, vi);
        const float denom = sqrtf(vi) / rsqrt_bc2_inv + eps;
        p = p - step_size * (mi / denom);
        c.p[i] = p;
        m[c.off + i] = mi;
        v[c.off + i] = vi;
        if (ema) {
            const float s = ema[c.off + i];
            ema[c.off + i] = s - (1.0f - ema_decay) * (s - p);
        }
    }
}

hipError_t launch_adam_ema(const void* chunks, int n_chunks, float* m, float* v, float* ema, float lr, float beta1,
                           float beta2, float eps, float wd, int decoupled, int step, float ema_decay, hipStream_t s) {
    (void)hipGetLastError();
    // bias corrections in double on the host, as Python floats in torch
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_ema_kernel, dim3(n_chunks), dim3(256), 0, s, (const OptimChunk*)chunks, m, v, ema, lr, beta1,
                       beta2, eps, wd, decoupled, step_size, sqrt_bc2, ema_decay);
    return hipGetLastError();
}

hipError_t launch_grad_sumsq(const void* chunks, int n_chunks, double* partial, double* stats, hipStream_t s) {
    (void)hipGetLastError();
    if (n_chunks > 0)
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_chunks), dim3(256), 0, s, (const OptimChunk*)chunks, partial);
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, n_chunks, stats);
    return hipGetLastError();
}

hipError_t launch_adam_ema_clipped(const void* chunks, int n_chunks, float* m, float* v, float* ema, float lr, float beta1,
                                   float beta2, float eps, float wd, int decoupled, int step, float ema_decay, double* stats,
                                   float max_norm, int skip_nonfinite, hipStream_t s) {
    (void)hipGetLastError();
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float step_size = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
    hipLaunchKernelGGL(adam_ema_clipped_kernel, dim3(n_chunks), dim3(256), 0, s, (const OptimChunk*)chunks, m, v, ema, lr,
                       beta1, beta2, eps, wd, decoupled, step_size, sqrt_bc2, ema_decay, stats, max_norm, skip_nonfinite);
    return hipGetLastError();
}

}  // namespace beso
