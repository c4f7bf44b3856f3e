// The trainable MLP observation / goal encoder (include/beso_mlp.h; reference networks/mlps/mlps.py:11-73): libbeso_mlp.so.
// Three kernels, all fp32 on v_mfma_f32_16x16x4_f32 (the exact-fp32 MFMA of gemm.hip's parity mode):
//   mlp_fwd_kernel     a workgroup carries 16 rows through every layer; activations in LDS, weights streamed from memory
//   mlp_bwd_kernel     the data-gradient chain of the same 16 rows in reverse layer order
//   wgrad_kernel<0>    dW / db partial sums per (layer, 16 input columns, row range); reduce_kernel adds them in order
// The tile GEMMs, the activations, the MFMA operand layout, those two kernels and the host's checks and launches: mlp_tile.h
// (shared with resmlp.hip and guide.hip).
#include "mlp_tile.h"

namespace beso_mlp {

constexpr int kMaxLinear = 5;      // n_hidden <= 4

struct Net {
    const float* w[kMaxLinear];
    const float* b[kMaxLinear];
    int n_linear, in_dim, hidden, out_dim, act;
};

__global__ __launch_bounds__(kThreads) void mlp_fwd_kernel(Net net, const float* __restrict__ x, long long M,
                                                           float* __restrict__ y, float* __restrict__ keep, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* cur = lds;
    float* nxt = lds + kRows * pitch;
    const long long m0 = (long long)blockIdx.x * kRows;
    const int H = net.hidden;
    load_tile(cur, pitch, x, net.in_dim, m0, M);
    if (keep) keep_x(keep, x, net.in_dim, m0, M);
    __syncthreads();
    float* keep_z = keep ? keep + (size_t)M * net.in_dim : nullptr;
    for (int l = 0; l < net.n_linear; ++l) {
        const int K = l == 0 ? net.in_dim : H;
        const float* bias = net.b[l];
        if (l + 1 < net.n_linear) {
            float* kz = keep_z ? keep_z + (size_t)l * (size_t)M * H : nullptr;
            const int act = net.act;
            tile_xwt(cur, pitch, net.w[l], H, K, [&](int r, int n, float v) {
                const float z = v + bias[n];
                if (kz && m0 + r < M) kz[(size_t)(m0 + r) * H + n] = z;
                nxt[r * pitch + n] = act_fwd(act, z);
            });
            __syncthreads();
            float* t = cur;
            cur = nxt;
            nxt = t;
        } else {
            const int O = net.out_dim;
            tile_xwt(cur, pitch, net.w[l], O, K, [&](int r, int n, float v) {
                if (m0 + r < M) y[(size_t)(m0 + r) * O + n] = v + bias[n];
            });
        }
    }
}

// dz [n_hidden][M, hidden] (workspace) and, with dx != NULL, dx [M, in]
__global__ __launch_bounds__(kThreads) void mlp_bwd_kernel(Net net, const float* __restrict__ keep,
                                                           const float* __restrict__ dy, long long M,
                                                           float* __restrict__ dz, float* __restrict__ dx, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* cur = lds;
    float* nxt = lds + kRows * pitch;
    const long long m0 = (long long)blockIdx.x * kRows;
    const int H = net.hidden, act = net.act;
    const float* keep_z = keep + (size_t)M * net.in_dim;
    load_tile(cur, pitch, dy, net.out_dim, m0, M);
    __syncthreads();
    for (int l = net.n_linear - 1; l >= 1; --l) {                     // dz_{l-1} = (dz_l W_l) * act'(z_{l-1})
        const int N = l == net.n_linear - 1 ? net.out_dim : H;
        const float* z = keep_z + (size_t)(l - 1) * (size_t)M * H;
        float* out = dz + (size_t)(l - 1) * (size_t)M * H;
        tile_xw(cur, pitch, net.w[l], N, H, [&](int r, int k, float v) {
            float d = 0.f;
            if (m0 + r < M) {
                d = v * act_bwd(act, z[(size_t)(m0 + r) * H + k]);
                out[(size_t)(m0 + r) * H + k] = d;
            }
            nxt[r * pitch + k] = d;
        });
        __syncthreads();
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    if (dx) {
        const int I = net.in_dim;
        tile_xw(cur, pitch, net.w[0], H, I, [&](int r, int k, float v) {
            if (m0 + r < M) dx[(size_t)(m0 + r) * I + k] = v;
        });
    }
}

// ------------------------------------------------------------------------------------------------------------ host
constexpr size_t kLdsMax = 2 * kTileBytes;        // the two tile kernels' LDS, two [16][pitch] buffers, at the widest: 66048

static int check_dims(const beso_mlp_dims* d, long long M) {
    if (!d) return BESO_ERR_BAD_ARG;
    if (d->n_hidden < 1 || d->n_hidden > kMaxLinear - 1) return BESO_ERR_BAD_SHAPE;
    return check_common(d->in_dim, d->hidden_dim, d->out_dim, d->activation, M);
}

static long long param_count(const beso_mlp_dims* d) {
    const long long H = d->hidden_dim;
    return (long long)d->in_dim * H + H + (long long)(d->n_hidden - 1) * (H * H + H) + (long long)d->out_dim * H + d->out_dim;
}

static size_t dz_bytes(const beso_mlp_dims* d, long long M) {
    return align256((size_t)d->n_hidden * (size_t)M * (size_t)d->hidden_dim * sizeof(float));
}

static int fill_net(Net* net, const float* const* params, int n_params, const beso_mlp_dims* d) {
    if (check_params(params, n_params, 2 * (d->n_hidden + 1)) != BESO_OK) return BESO_ERR_BAD_ARG;
    net->n_linear = d->n_hidden + 1;
    for (int l = 0; l < net->n_linear; ++l) {
        net->w[l] = params[2 * l];
        net->b[l] = params[2 * l + 1];
    }
    net->in_dim = d->in_dim;
    net->hidden = d->hidden_dim;
    net->out_dim = d->out_dim;
    net->act = d->activation;
    return BESO_OK;
}

static int pitch_of(const beso_mlp_dims* d) { return tile_pitch(std::max({d->in_dim, d->hidden_dim, d->out_dim})); }

}  // namespace beso_mlp

using namespace beso_mlp;

extern "C" size_t beso_mlp_workspace_bytes(const beso_mlp_dims* dims, long long M, int training) {
    if (check_dims(dims, M) != BESO_OK || !training) return 0;
    return dz_bytes(dims, M) + slab_bytes(M, param_count(dims));
}

extern "C" int beso_mlp_fwd(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* x,
                            long long M, float* y, float* keep, void* stream) {
    int st = check_dims(dims, M);
    if (st != BESO_OK) return st;
    Net net;
    if ((st = fill_net(&net, params, n_params, dims)) != BESO_OK) return st;
    if (!x || !y || ((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)keep & 3)) return BESO_ERR_BAD_ARG;
    const int pitch = pitch_of(dims);
    return to_status(launch_lds_attr<mlp_fwd_kernel>(kLdsMax, dim3(tile_grid(M)), dim3(kThreads), 2 * (size_t)kRows * pitch * sizeof(float),
                                                     (hipStream_t)stream, net, x, M, y, keep, pitch));
}

extern "C" int beso_mlp_bwd(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* keep,
                            const float* dy, long long M, float* dx, float* grads_flat, void* workspace,
                            size_t workspace_bytes, int flags, void* stream) {
    int st = check_dims(dims, M);
    if (st != BESO_OK) return st;
    Net net;
    if ((st = fill_net(&net, params, n_params, dims)) != BESO_OK) return st;
    if (!keep || !dy || !grads_flat || ((uintptr_t)keep & 3) || ((uintptr_t)dy & 3) || ((uintptr_t)dx & 3) ||
        ((uintptr_t)grads_flat & 3) || (flags & ~BESO_MLP_ACCUMULATE))
        return BESO_ERR_BAD_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < beso_mlp_workspace_bytes(dims, M, 1))
        return BESO_ERR_WORKSPACE;

    float* dz = (float*)workspace;
    float* slab = (float*)((char*)workspace + dz_bytes(dims, M));
    const int H = dims->hidden_dim, nl = net.n_linear;
    const float* keep_z = keep + (size_t)M * dims->in_dim;
    WgPlan plan(M, param_count(dims), dims->activation);
    for (int l = 0; l < nl; ++l)                                      // layer l's input: x, else act(z_{l-1}) applied on load
        plan.add(l == nl - 1 ? dy : dz + (size_t)l * (size_t)M * H, l == 0 ? keep : keep_z + (size_t)(l - 1) * (size_t)M * H,
                 l == nl - 1 ? dims->out_dim : H, l == 0 ? dims->in_dim : H, l > 0);

    const int pitch = pitch_of(dims);
    return launch_bwd<mlp_bwd_kernel, 0>(kLdsMax, 2 * (size_t)kRows * pitch * sizeof(float), (hipStream_t)stream, plan, slab,
                                         grads_flat, flags & BESO_MLP_ACCUMULATE, net, keep, dy, M, dz, dx, pitch);
}
