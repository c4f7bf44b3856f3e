// The residual MLP encoder (include/beso_resmlp.h; reference networks/mlps/mlps.py:76-133 over res_layers.py): libbeso_resmlp.so.
// fp32 on v_mfma_f32_16x16x4_f32 through the tile GEMMs of mlp_tile.h (operand layout there).  Two kernels of its own:
//   resmlp_fwd_kernel     a workgroup carries 16 rows through every layer: the residual stream and two ping-pong tiles in LDS
//   resmlp_bwd_kernel     the data-gradient chain of the same 16 rows in reverse order, LayerNorm backward at both uses
// and mlp_tile.h's wgrad_kernel<kWgChunk> (dW / db, and dgamma / dbeta as bias-only "layers", summed in chunks) and reduce_kernel.
// The element-wise passes between the GEMMs give a row to 16 lanes (thread t: row t >> 4, columns (t & 15) + 16 i), so a
// LayerNorm statistic is a fixed-order sum per lane and a four-step butterfly over those 16 lanes.
#include "mlp_tile.h"
#include "../../include/beso_resmlp.h"

namespace beso_resmlp {

using namespace beso_mlp;

constexpr int kMaxBlocks = 4;
static_assert(2 + 4 * kMaxBlocks <= kMaxWgLayers, "two outer Linears; per block l1, l2, gamma, beta");
constexpr float kLnEps = 1e-6f;
constexpr size_t kLdsMax = 3 * kTileBytes;            // the two tile kernels' LDS, three [16][pitch] buffers, at the widest: 99072
constexpr int kWgChunk = 2;                           // 16-row steps of the weight gradient summed before they join the total

struct Net {
    const float *w0, *b0, *wl, *bl;
    const float *w1[kMaxBlocks], *b1[kMaxBlocks], *w2[kMaxBlocks], *b2[kMaxBlocks];
    const float *gamma[kMaxBlocks], *beta[kMaxBlocks];                // NULL without a norm
    int n_blocks, in_dim, hidden, out_dim, act;
};

// the sum over the 16 lanes of a row; every lane gets the same bits (each step adds a pair in both lanes)
__device__ __forceinline__ float row_sum16(float v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 16);
    return v;
}

__device__ __forceinline__ void row_stats(const float* row, int H, int l16, float& mean, float& rstd) {
    float s = 0.f;
    for (int c = l16; c < H; c += 16) s += row[c];
    mean = row_sum16(s) / (float)H;
    float q = 0.f;
    for (int c = l16; c < H; c += 16) {
        const float d = row[c] - mean;
        q += d * d;
    }
    rstd = 1.0f / sqrtf(row_sum16(q) / (float)H + kLnEps);
}

// dst[r][c] = act(norm(src[r][c])) for c < H; gamma == NULL: norm is the identity
__device__ __forceinline__ void norm_act(float* dst, const float* src, int pitch, int H, int act,
                                         const float* __restrict__ gamma, const float* __restrict__ beta) {
    const int r = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const float* row = src + r * pitch;
    float* out = dst + r * pitch;
    float mean = 0.f, rstd = 1.f;
    if (gamma) row_stats(row, H, l16, mean, rstd);
    for (int c = l16; c < H; c += 16) {
        float n = row[c];
        if (gamma) n = (n - mean) * rstd * gamma[c] + beta[c];
        out[c] = act_fwd(act, n);
    }
}

// The backward of a = act(norm(z)) on the tile.  d: dL/da on entry, dL/dz on return; z: the pre-norm values.
//   a_out [M, H]   a itself, the input of the Linear behind it (for the weight gradient)
//   dz_out [M, H]  or NULL: dL/dz;   stream or NULL: the LDS tile dL/dz is added to (the residual add)
//   gp, bp [M, H]  (with a norm) dn * xhat and dn, dn the gradient of the normalizer's output: written, or with `second` --
//                  the block's other use of the same normalizer, which the SAME thread wrote earlier -- added to
__device__ __forceinline__ void norm_act_bwd(float* d, const float* z, int pitch, int H, int act,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, float* a_out,
                                             float* dz_out, float* stream, float* gp, float* bp, bool second, long long m0,
                                             long long M) {
    const int r = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const bool live = m0 + r < M;
    const size_t g = (size_t)(m0 + r) * H;
    float* drow = d + r * pitch;
    const float* zrow = z + r * pitch;
    float* srow = stream ? stream + r * pitch : nullptr;
    if (!gamma) {
        for (int c = l16; c < H; c += 16) {
            const float zz = zrow[c];
            const float v = drow[c] * act_bwd(act, zz);
            drow[c] = v;
            if (live) {
                a_out[g + c] = act_fwd(act, zz);
                if (dz_out) dz_out[g + c] = v;
            }
            if (srow) srow[c] += v;
        }
        return;
    }
    float mean, rstd;
    row_stats(zrow, H, l16, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
    for (int c = l16; c < H; c += 16) {
        const float xh = (zrow[c] - mean) * rstd;
        const float n = xh * gamma[c] + beta[c];
        const float dn = drow[c] * act_bwd(act, n);
        if (live) {
            a_out[g + c] = act_fwd(act, n);
            const float p = dn * xh;
            gp[g + c] = second ? gp[g + c] + p : p;
            bp[g + c] = second ? bp[g + c] + dn : dn;
        }
        const float dxh = dn * gamma[c];
        drow[c] = dxh;
        s1 += dxh;
        s2 += dxh * xh;
    }
    s1 = row_sum16(s1) / (float)H;
    s2 = row_sum16(s2) / (float)H;
    for (int c = l16; c < H; c += 16) {
        const float xh = (zrow[c] - mean) * rstd;
        const float v = rstd * (drow[c] - s1 - xh * s2);
        drow[c] = v;
        if (live && dz_out) dz_out[g + c] = v;
        if (srow) srow[c] += v;
    }
}

// rows [m0, m0 + 16) below M of the LDS tile -> dst [M, H]
__device__ __forceinline__ void store_tile(float* __restrict__ dst, const float* lds, int pitch, int H, long long m0,
                                           long long M) {
    for (int i = threadIdx.x; i < kRows * H; i += kThreads) {
        const int r = i / H, c = i - r * H;
        if (m0 + r < M) dst[(size_t)(m0 + r) * H + c] = lds[r * pitch + c];
    }
}

__global__ __launch_bounds__(kThreads) void resmlp_fwd_kernel(Net net, const float* __restrict__ x, long long M,
                                                              float* __restrict__ y, float* __restrict__ keep, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* S = lds;                                                   // the residual stream u
    float* T1 = lds + kRows * pitch;
    float* T2 = lds + 2 * kRows * pitch;
    const long long m0 = (long long)blockIdx.x * kRows;
    const int H = net.hidden, B = net.n_blocks, act = net.act;
    load_tile(T1, pitch, x, net.in_dim, m0, M);
    if (keep) keep_x(keep, x, net.in_dim, m0, M);
    __syncthreads();
    const size_t MH = (size_t)M * H;
    float* keep_u = keep ? keep + (size_t)M * net.in_dim : nullptr;   // u_0 .. u_B
    float* keep_v = keep ? keep_u + (size_t)(B + 1) * MH : nullptr;   // v_0 .. v_{B-1}
    {
        const float* bias = net.b0;
        tile_xwt(T1, pitch, net.w0, H, net.in_dim, [&](int r, int n, float v) {
            const float u = v + bias[n];
            S[r * pitch + n] = u;
            if (keep_u && m0 + r < M) keep_u[(size_t)(m0 + r) * H + n] = u;
        });
    }
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        norm_act(T1, S, pitch, H, act, net.gamma[b], net.beta[b]);
        __syncthreads();
        {
            const float* bias = net.b1[b];
            float* kv = keep_v ? keep_v + (size_t)b * MH : nullptr;
            tile_xwt(T1, pitch, net.w1[b], H, H, [&](int r, int n, float v) {
                const float z = v + bias[n];
                T2[r * pitch + n] = z;
                if (kv && m0 + r < M) kv[(size_t)(m0 + r) * H + n] = z;
            });
        }
        __syncthreads();
        norm_act(T1, T2, pitch, H, act, net.gamma[b], net.beta[b]);
        __syncthreads();
        {
            const float* bias = net.b2[b];
            float* ku = keep_u ? keep_u + (size_t)(b + 1) * MH : nullptr;
            tile_xwt(T1, pitch, net.w2[b], H, H, [&](int r, int n, float v) {   // S is no operand here: each element has one owner
                const float u = (v + bias[n]) + S[r * pitch + n];
                S[r * pitch + n] = u;
                if (ku && m0 + r < M) ku[(size_t)(m0 + r) * H + n] = u;
            });
        }
        __syncthreads();
    }
    const int O = net.out_dim;
    const float* bias = net.bl;
    tile_xwt(S, pitch, net.wl, O, H, [&](int r, int n, float v) {
        if (m0 + r < M) y[(size_t)(m0 + r) * O + n] = v + bias[n];
    });
}

// Fills the workspace arrays of include/beso_resmlp.h (`ws`: dU_0; per block dV, dU_next, A1, A2; then per block GP, BP) and,
// with dx != NULL, dx [M, in].
__global__ __launch_bounds__(kThreads) void resmlp_bwd_kernel(Net net, const float* __restrict__ keep,
                                                              const float* __restrict__ dy, long long M, float* ws,
                                                              float* __restrict__ dx, int pitch) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* S = lds;                                                   // the gradient of the residual stream
    float* T1 = lds + kRows * pitch;
    float* T2 = lds + 2 * kRows * pitch;
    const long long m0 = (long long)blockIdx.x * kRows;
    const int H = net.hidden, B = net.n_blocks, act = net.act;
    const size_t MH = (size_t)M * H;
    const float* keep_u = keep + (size_t)M * net.in_dim;
    const float* keep_v = keep_u + (size_t)(B + 1) * MH;
    float* norm_ws = ws + (size_t)(1 + 4 * B) * MH;
    load_tile(T1, pitch, dy, net.out_dim, m0, M);
    __syncthreads();
    tile_xw(T1, pitch, net.wl, net.out_dim, H, [&](int r, int k, float v) { S[r * pitch + k] = v; });
    __syncthreads();
    for (int b = B - 1; b >= 0; --b) {
        float* blk = ws + (size_t)(1 + 4 * b) * MH;                   // dV_b, dU_{b+1}, A1_b, A2_b
        float* gp = norm_ws + (size_t)(2 * b) * MH;
        float* bp = gp + MH;
        const float *gamma = net.gamma[b], *beta = net.beta[b];
        store_tile(blk + MH, S, pitch, H, m0, M);                     // dU_{b+1}: the output gradient of l2_b
        load_tile(T2, pitch, keep_v + (size_t)b * MH, H, m0, M);
        tile_xw(S, pitch, net.w2[b], H, H, [&](int r, int k, float v) { T1[r * pitch + k] = v; });
        __syncthreads();
        norm_act_bwd(T1, T2, pitch, H, act, gamma, beta, blk + 3 * MH, blk, nullptr, gp, bp, false, m0, M);
        __syncthreads();
        tile_xw(T1, pitch, net.w1[b], H, H, [&](int r, int k, float v) { T2[r * pitch + k] = v; });
        __syncthreads();
        load_tile(T1, pitch, keep_u + (size_t)b * MH, H, m0, M);
        __syncthreads();
        norm_act_bwd(T2, T1, pitch, H, act, gamma, beta, blk + 2 * MH, nullptr, S, gp, bp, true, m0, M);
        __syncthreads();
    }
    store_tile(ws, S, pitch, H, m0, M);                               // dU_0: the output gradient of the first Linear
    if (dx) {
        const int I = net.in_dim;
        tile_xw(S, pitch, net.w0, H, I, [&](int r, int k, float v) {
            if (m0 + r < M) dx[(size_t)(m0 + r) * I + k] = v;
        });
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static int check_dims(const beso_resmlp_dims* d, long long M) {
    if (!d) return BESO_ERR_BAD_ARG;
    if (d->n_blocks < 1 || d->n_blocks > kMaxBlocks) return BESO_ERR_BAD_SHAPE;
    const int st = check_common(d->in_dim, d->hidden_dim, d->out_dim, d->activation, M);
    if (st != BESO_OK) return st;
    return d->norm == BESO_RESMLP_NORM_NONE || d->norm == BESO_RESMLP_NORM_LAYER ? BESO_OK : BESO_ERR_BAD_ARG;
}

static long long param_count(const beso_resmlp_dims* d) {
    const long long H = d->hidden_dim;
    const long long block = 2 * (H * H + H) + (d->norm ? 2 * H : 0);
    return (long long)d->in_dim * H + H + d->n_blocks * block + (long long)d->out_dim * H + d->out_dim;
}

// the [M, hidden] arrays the chain writes in front of the slab
static size_t chain_bytes(const beso_resmlp_dims* d, long long M) {
    const size_t arrays = 1 + (size_t)d->n_blocks * (d->norm ? 6 : 4);
    return align256(arrays * (size_t)M * (size_t)d->hidden_dim * sizeof(float));
}

static int fill_net(Net* net, const float* const* params, int n_params, const beso_resmlp_dims* d) {
    const int per_block = d->norm ? 6 : 4;
    if (check_params(params, n_params, 4 + per_block * d->n_blocks) != BESO_OK) return BESO_ERR_BAD_ARG;
    *net = Net{};
    net->w0 = params[0];
    net->b0 = params[1];
    for (int b = 0; b < d->n_blocks; ++b) {
        const float* const* p = params + 2 + per_block * b;
        net->w1[b] = p[0];
        net->b1[b] = p[1];
        net->w2[b] = p[2];
        net->b2[b] = p[3];
        if (d->norm) {
            net->gamma[b] = p[4];
            net->beta[b] = p[5];
        }
    }
    net->wl = params[n_params - 2];
    net->bl = params[n_params - 1];
    net->n_blocks = d->n_blocks;
    net->in_dim = d->in_dim;
    net->hidden = d->hidden_dim;
    net->out_dim = d->out_dim;
    net->act = d->activation;
    return BESO_OK;
}

static int pitch_of(const beso_resmlp_dims* d) { return tile_pitch(std::max({d->in_dim, d->hidden_dim, d->out_dim})); }

}  // namespace beso_resmlp

using namespace beso_resmlp;

extern "C" size_t beso_resmlp_workspace_bytes(const beso_resmlp_dims* dims, long long M, int training) {
    if (check_dims(dims, M) != BESO_OK || !training) return 0;
    return chain_bytes(dims, M) + slab_bytes(M, param_count(dims));
}

extern "C" int beso_resmlp_fwd(const float* const* params, int n_params, const beso_resmlp_dims* dims, const float* x,
                               long long M, float* y, float* keep, void* stream) {
    int st = check_dims(dims, M);
    if (st != BESO_OK) return st;
    Net net;
    if ((st = fill_net(&net, params, n_params, dims)) != BESO_OK) return st;
    if (!x || !y || ((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)keep & 3)) return BESO_ERR_BAD_ARG;
    const int pitch = pitch_of(dims);
    return to_status(launch_lds_attr<resmlp_fwd_kernel>(kLdsMax, dim3(tile_grid(M)), dim3(kThreads), 3 * (size_t)kRows * pitch * sizeof(float),
                                                        (hipStream_t)stream, net, x, M, y, keep, pitch));
}

extern "C" int beso_resmlp_bwd(const float* const* params, int n_params, const beso_resmlp_dims* dims, const float* keep,
                               const float* dy, long long M, float* dx, float* grads_flat, void* workspace,
                               size_t workspace_bytes, int flags, void* stream) {
    int st = check_dims(dims, M);
    if (st != BESO_OK) return st;
    Net net;
    if ((st = fill_net(&net, params, n_params, dims)) != BESO_OK) return st;
    if (!keep || !dy || !grads_flat || ((uintptr_t)keep & 3) || ((uintptr_t)dy & 3) || ((uintptr_t)dx & 3) ||
        ((uintptr_t)grads_flat & 3) || (flags & ~BESO_MLP_ACCUMULATE))
        return BESO_ERR_BAD_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < beso_resmlp_workspace_bytes(dims, M, 1))
        return BESO_ERR_WORKSPACE;

    float* ws = (float*)workspace;
    float* slab = (float*)((char*)workspace + chain_bytes(dims, M));
    const int H = dims->hidden_dim, B = dims->n_blocks;
    const size_t MH = (size_t)M * H;
    const float* keep_u = keep + (size_t)M * dims->in_dim;
    const float* norm_ws = ws + (size_t)(1 + 4 * B) * MH;

    WgPlan plan(M, param_count(dims), dims->activation);              // apply_act 0: every input is stored as it entered its GEMM
    plan.add(ws, keep, H, dims->in_dim, 0);
    for (int b = 0; b < B; ++b) {
        const float* blk = ws + (size_t)(1 + 4 * b) * MH;
        plan.add(blk, blk + 2 * MH, H, H, 0);                         // l1: dV_b, A1_b
        plan.add(blk + MH, blk + 3 * MH, H, H, 0);                    // l2: dU_{b+1}, A2_b
        if (dims->norm) {                                             // gamma, beta: two bias-only layers, back to back
            const float* gp = norm_ws + (size_t)(2 * b) * MH;
            plan.add(gp, nullptr, H, 0, 0);
            plan.add(gp + MH, nullptr, H, 0, 0);
        }
    }
    plan.add(dy, keep_u + (size_t)B * MH, dims->out_dim, H, 0);

    const int pitch = pitch_of(dims);
    return launch_bwd<resmlp_bwd_kernel, kWgChunk>(kLdsMax, 3 * (size_t)kRows * pitch * sizeof(float), (hipStream_t)stream, plan, slab,
                                                   grads_flat, flags & BESO_MLP_ACCUMULATE, net, keep, dy, M, ws, dx, pitch);
}
