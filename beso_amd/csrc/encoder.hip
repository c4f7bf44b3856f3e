// The trainable MLP observation / goal encoder (include/beso_mlp.h; reference networks/mlps/mlps.py:11-73): libbeso_mlp.so.
// Three kernels, all fp32 on v_mfma_f32_16x16x4_f32 (the exact-fp32 MFMA of gemm.hip's parity mode):
//   mlp_fwd_kernel     a workgroup carries 16 rows through every layer; activations in LDS, weights streamed from memory
//   mlp_bwd_kernel     the data-gradient chain of the same 16 rows in reverse layer order
//   mlp_wgrad_kernel   dW / db partial sums per (layer, 16 input columns, row range); mlp_reduce_kernel adds them in order
// The tile GEMMs, the activations and the MFMA operand layout: mlp_tile.h (shared with resmlp.hip).
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
    if (keep) {                                                       // keep[0 : M in] = x
        for (int i = threadIdx.x; i < kRows * net.in_dim; i += kThreads) {
            const int r = i / net.in_dim, c = i - r * net.in_dim;
            if (m0 + r < M) keep[(size_t)(m0 + r) * net.in_dim + c] = x[(size_t)(m0 + r) * net.in_dim + c];
        }
    }
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

// What one layer's weight gradient reads and where its partial sums go.
struct WgLayer {
    const float* dz;      // [M, N]: dz_l (dy for the last layer)
    const float* a;       // [M, K]: x for layer 0, else z_{l-1} (the activation is applied on the fly)
    int N, K, apply_act;
    int block0;           // first workgroup of the layer: ceil((K + 1) / 16) column tiles x n_splits row ranges
    long long w_off, b_off;   // offsets into one slab row (= into grads_flat)
};
struct WgPlan {
    WgLayer layer[kMaxLinear];
    int n_linear, n_splits, act;
    long long rows_per_split, M, P;
};

// slab[split][w_off + n K + k] = sum over the split's rows of dz[m][n] a[m][k];  column k == K is the bias (a = 1).
__global__ __launch_bounds__(kThreads) void mlp_wgrad_kernel(WgPlan plan, float* __restrict__ slab) {
    int li = 0;
    while (li + 1 < plan.n_linear && (int)blockIdx.x >= plan.layer[li + 1].block0) ++li;
    const WgLayer L = plan.layer[li];
    const int local = blockIdx.x - L.block0;
    const int split = local % plan.n_splits, ktile = local / plan.n_splits;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const long long r0 = (long long)split * plan.rows_per_split;
    const long long r1 = r0 + plan.rows_per_split < plan.M ? r0 + plan.rows_per_split : plan.M;
    const int k = ktile * 16 + lr;
    const int n_tiles = (L.N + 15) / 16;

    f32x4 acc[kWgTiles];
#pragma unroll
    for (int i = 0; i < kWgTiles; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long long m0 = r0; m0 < r1; m0 += 16) {
        f32x4 b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long m = m0 + 4 * g + j;
            float v = 0.f;
            if (m < r1) {
                if (k < L.K) {
                    v = L.a[(size_t)m * L.K + k];
                    if (L.apply_act) v = act_fwd(plan.act, v);
                } else if (k == L.K) {
                    v = 1.f;
                }
            }
            b[j] = v;
        }
#pragma unroll
        for (int i = 0; i < kWgTiles; ++i) {
            const int tile = wid + kWaves * i;
            if (tile < n_tiles) {
                const int n = tile * 16 + lr;
                f32x4 a;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const long long m = m0 + 4 * g + j;
                    a[j] = (m < r1 && n < L.N) ? L.dz[(size_t)m * L.N + n] : 0.f;
                }
                acc[i] = mfma4(acc[i], a, b);
            }
        }
    }
    float* out = slab + (size_t)split * (size_t)plan.P;
#pragma unroll
    for (int i = 0; i < kWgTiles; ++i) {
        const int tile = wid + kWaves * i;
        if (tile < n_tiles) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = tile * 16 + 4 * g + r;
                if (n < L.N) {
                    if (k < L.K) out[L.w_off + (size_t)n * L.K + k] = acc[i][r];
                    else if (k == L.K) out[L.b_off + n] = acc[i][r];
                }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void mlp_reduce_kernel(const float* __restrict__ slab, float* __restrict__ grads,
                                                              long long P, int n_splits, int accumulate) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P) return;
    float s = slab[e];
    for (int i = 1; i < n_splits; ++i) s += slab[(size_t)i * (size_t)P + e];
    grads[e] = accumulate ? grads[e] + s : s;
}

// ------------------------------------------------------------------------------------------------------------ host
static int check_dims(const beso_mlp_dims* d, long long M) {
    if (!d) return BESO_ERR_BAD_ARG;
    if (d->in_dim < 1 || d->in_dim > kMaxDim || d->out_dim < 1 || d->out_dim > kMaxDim) return BESO_ERR_BAD_SHAPE;
    if (d->hidden_dim < 16 || d->hidden_dim > kMaxDim || d->hidden_dim % 16) return BESO_ERR_BAD_SHAPE;
    if (d->n_hidden < 1 || d->n_hidden > kMaxLinear - 1) return BESO_ERR_BAD_SHAPE;
    if (M < 1 || M > 0x7fffffffLL) return BESO_ERR_BAD_SHAPE;
    if (d->activation < BESO_MLP_ACT_RELU || d->activation > BESO_MLP_ACT_SIGMOID) return BESO_ERR_BAD_ARG;
    return BESO_OK;
}

static long long param_count(const beso_mlp_dims* d) {
    const long long H = d->hidden_dim;
    return (long long)d->in_dim * H + H + (long long)(d->n_hidden - 1) * (H * H + H) + (long long)d->out_dim * H + d->out_dim;
}

static size_t dz_bytes(const beso_mlp_dims* d, long long M) {
    return align256((size_t)d->n_hidden * (size_t)M * (size_t)d->hidden_dim * sizeof(float));
}

static int fill_net(Net* net, const float* const* params, int n_params, const beso_mlp_dims* d) {
    if (!params || n_params != 2 * (d->n_hidden + 1)) return BESO_ERR_BAD_ARG;
    for (int i = 0; i < n_params; ++i)
        if (!params[i] || ((uintptr_t)params[i] & 3)) return BESO_ERR_BAD_ARG;
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

// LDS of the two tile kernels: two [16][pitch] buffers
static int tile_pitch(const beso_mlp_dims* d) {
    int w = d->in_dim > d->out_dim ? d->in_dim : d->out_dim;
    if (d->hidden_dim > w) w = d->hidden_dim;
    return round16(w) + kLdsPad;
}

}  // namespace beso_mlp

using namespace beso_mlp;

extern "C" size_t beso_mlp_workspace_bytes(const beso_mlp_dims* dims, long long M, int training) {
    if (check_dims(dims, M) != BESO_OK || !training) return 0;
    const long long R = rows_per_split(M), S = (M + R - 1) / R;
    return dz_bytes(dims, M) + align256((size_t)S * (size_t)param_count(dims) * sizeof(float));
}

extern "C" int beso_mlp_fwd(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* x,
                            long long M, float* y, float* keep, void* stream) {
    int st = check_dims(dims, M);
    if (st != BESO_OK) return st;
    Net net;
    if ((st = fill_net(&net, params, n_params, dims)) != BESO_OK) return st;
    if (!x || !y || ((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)keep & 3)) return BESO_ERR_BAD_ARG;
    const int pitch = tile_pitch(dims);
    const size_t lds = 2 * (size_t)kRows * pitch * sizeof(float);
    (void)hipGetLastError();
    if (allow_lds(mlp_fwd_kernel, lds) != hipSuccess) return BESO_ERR_HIP;
    const unsigned grid = (unsigned)((M + kRows - 1) / kRows);
    hipLaunchKernelGGL(mlp_fwd_kernel, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream, net, x, M, y, keep, pitch);
    return hipGetLastError() == hipSuccess ? BESO_OK : BESO_ERR_HIP;
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

    WgPlan plan;
    plan.n_linear = nl;
    plan.act = dims->activation;
    plan.M = M;
    plan.P = param_count(dims);
    plan.rows_per_split = rows_per_split(M);
    plan.n_splits = (int)((M + plan.rows_per_split - 1) / plan.rows_per_split);
    long long off = 0;
    int blocks = 0;
    for (int l = 0; l < nl; ++l) {
        WgLayer& L = plan.layer[l];
        L.N = l == nl - 1 ? dims->out_dim : H;
        L.K = l == 0 ? dims->in_dim : H;
        L.dz = l == nl - 1 ? dy : dz + (size_t)l * (size_t)M * H;
        L.a = l == 0 ? keep : keep_z + (size_t)(l - 1) * (size_t)M * H;
        L.apply_act = l > 0;
        L.block0 = blocks;
        L.w_off = off;
        L.b_off = off + (long long)L.N * L.K;
        off = L.b_off + L.N;
        blocks += (L.K + 1 + 15) / 16 * plan.n_splits;
    }

    const int pitch = tile_pitch(dims);
    const size_t lds = 2 * (size_t)kRows * pitch * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    if (allow_lds(mlp_bwd_kernel, lds) != hipSuccess) return BESO_ERR_HIP;
    const unsigned grid = (unsigned)((M + kRows - 1) / kRows);
    hipLaunchKernelGGL(mlp_bwd_kernel, dim3(grid), dim3(kThreads), lds, s, net, keep, dy, M, dz, dx, pitch);
    if (hipGetLastError() != hipSuccess) return BESO_ERR_HIP;
    hipLaunchKernelGGL(mlp_wgrad_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, plan, slab);
    if (hipGetLastError() != hipSuccess) return BESO_ERR_HIP;
    hipLaunchKernelGGL(mlp_reduce_kernel, dim3((unsigned)((plan.P + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       (const float*)slab, grads_flat, plan.P, plan.n_splits, flags & BESO_MLP_ACCUMULATE);
    return hipGetLastError() == hipSuccess ? BESO_OK : BESO_ERR_HIP;
}
