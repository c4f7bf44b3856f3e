// What the three tile-MLP units (encoder.hip: libbeso_mlp.so; resmlp.hip: libbeso_resmlp.so; guide.hip: libbeso_guide.so) share:
// the 16-row tile GEMMs on v_mfma_f32_16x16x4_f32, the activations, the weight-gradient and reduce kernels with their plan and
// row-range rule, and the host's argument checks and launches.  Each unit keeps its own forward and backward chain kernels.
// MFMA operand layout (as gemm.hip): A lane -> (row = lane & 15, k = lane >> 4), B lane -> (k = lane >> 4, col = lane & 15),
// C lane -> (col = lane & 15, rows 4 (lane >> 4) + r).  A 16-wide k group is fed as four MFMAs; MFMA j takes
// k = k0 + 4 (lane >> 4) + j from BOTH operands, so a lane reads four consecutive k of its row.
#pragma once
#include <algorithm>
#include "common.h"               // launch_lds_attr / launch_plain / to_status: only templates and inline code, nothing to link
#include "../../include/beso_mlp.h"

namespace beso_mlp {

using beso::f32x4;
using beso::launch_lds_attr;
using beso::launch_plain;
using beso::to_status;

constexpr int kRows = 16;          // rows of x per workgroup (one MFMA tile)
constexpr int kThreads = 256;      // four waves: a layer's 16-column output tiles are dealt round-robin to them
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 512;
constexpr int kLdsPad = 4;         // row pitch = width + 4 floats: 16 rows of a float4 column hit 64 distinct banks
constexpr int kWgTiles = kMaxDim / 16 / kWaves;   // output-row tiles of dW one wave of a weight-gradient kernel owns: 8
constexpr int kMaxWgLayers = 18;   // the residual network's: two outer Linears; per block (<= 4) l1, l2, gamma, beta
constexpr size_t kTileBytes = (size_t)kRows * (kMaxDim + kLdsPad) * sizeof(float);   // one LDS tile at the widest: 33024

__host__ __device__ inline int round16(int v) { return (v + 15) & ~15; }

__device__ __forceinline__ float act_fwd(int act, float z) {
    if (act == BESO_MLP_ACT_RELU) return z > 0.f ? z : 0.f;
    if (act == BESO_MLP_ACT_SIGMOID) return 1.0f / (1.0f + expf(-z));
    return z * tanhf(log1pf(expf(z)));                                // Mish
}
__device__ __forceinline__ float act_bwd(int act, float z) {
    if (act == BESO_MLP_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    const float s = 1.0f / (1.0f + expf(-z));
    if (act == BESO_MLP_ACT_SIGMOID) return s * (1.0f - s);
    const float t = tanhf(log1pf(expf(z)));                           // Mish: tanh(sp) + z sigmoid(z) (1 - tanh(sp)^2)
    return t + z * s * (1.0f - t * t);
}

__device__ __forceinline__ f32x4 mfma4(f32x4 acc, const f32x4& a, const f32x4& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
    return acc;
}

// rows [m0, m0 + 16) of src [M, width] -> lds [16][pitch]; rows >= M and columns [width, round16(width)) become 0
__device__ __forceinline__ void load_tile(float* lds, int pitch, const float* __restrict__ src, int width, long long m0,
                                          long long M) {
    const int wp = round16(width);
    for (int i = threadIdx.x; i < kRows * wp; i += kThreads) {
        const int r = i / wp, c = i - r * wp;
        const long long m = m0 + r;
        lds[r * pitch + c] = (m < M && c < width) ? src[(size_t)m * width + c] : 0.f;
    }
}

// keep[0 : M width] = x for the tile's rows below M (a forward that keeps for the backward: the backward takes no x)
__device__ __forceinline__ void keep_x(float* __restrict__ keep, const float* __restrict__ x, int width, long long m0, long long M) {
    for (int i = threadIdx.x; i < kRows * width; i += kThreads) {
        const int r = i / width, c = i - r * width;
        if (m0 + r < M) keep[(size_t)(m0 + r) * width + c] = x[(size_t)(m0 + r) * width + c];
    }
}

// One layer of the forward on the tile: out[16, N] = in[16, K] W[N, K]^T, handed to `epi(row, n, value)` for n < N.
// `in` is zero beyond K up to round16(K).  Wave w takes the output tiles w, w + 4, ...
template <typename Epi>
__device__ __forceinline__ void tile_xwt(const float* in, int pitch, const float* __restrict__ W, int N, int K, Epi epi) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const int Kp = round16(K);
    const bool vec = (K & 3) == 0 && ((uintptr_t)W & 15) == 0;
    for (int n0 = wid * 16; n0 < N; n0 += kWaves * 16) {
        const int n = n0 + lr;
        const float* wrow = W + (size_t)(n < N ? n : N - 1) * K;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Kp; k0 += 16) {
            const int k = k0 + 4 * g;
            const f32x4 a = *(const f32x4*)(in + lr * pitch + k);
            f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (n < N) {
                if (vec && k + 3 < K) {
                    b = *(const f32x4*)(wrow + k);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = (k + j < K) ? wrow[k + j] : 0.f;
                }
            }
            acc = mfma4(acc, a, b);
        }
        if (n < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(4 * g + r, n, acc[r]);
        }
    }
}

// One layer of the backward chain on the tile: out[16, n_cols] = in[16, N] W[N, ldw] for the columns [k_lo, k_lo + n_cols) of W,
// handed to `epi(row, column - k_lo, value)`.  `in` is zero beyond N up to round16(N).
template <typename Epi>
__device__ __forceinline__ void tile_xw(const float* in, int pitch, const float* __restrict__ W, int N, int ldw, int k_lo,
                                        int n_cols, Epi epi) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const int Np = round16(N);
    for (int k0 = wid * 16; k0 < n_cols; k0 += kWaves * 16) {
        const int k = k0 + lr;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int n0 = 0; n0 < Np; n0 += 16) {
            const int n = n0 + 4 * g;
            const f32x4 a = *(const f32x4*)(in + lr * pitch + n);
            f32x4 b;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = (k < n_cols && n + j < N) ? W[(size_t)(n + j) * ldw + k_lo + k] : 0.f;
            acc = mfma4(acc, a, b);
        }
        if (k < n_cols) {
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(4 * g + r, k, acc[r]);
        }
    }
}
// ... for all of W [N, K]
template <typename Epi>
__device__ __forceinline__ void tile_xw(const float* in, int pitch, const float* __restrict__ W, int N, int K, Epi epi) {
    tile_xw(in, pitch, W, N, K, 0, K, epi);
}

// What one "layer" of the weight gradient reads and where its partial sums go.  K == 0: only the bias column (the residual
// network's dgamma, dbeta).
struct WgLayer {
    const float* dz;      // [M, N]: the layer's output gradient
    const float* a;       // [M, K]: the layer's input -- as it entered the GEMM, or (apply_act) its pre-activation
    int N, K, apply_act;
    int block0;           // first workgroup of the layer: ceil((K + 1) / 16) column tiles x n_splits row ranges
    long long w_off, b_off;   // offsets into one slab row (= into grads_flat)
};
struct WgPlan {
    WgLayer layer[kMaxWgLayers];
    int n_layers, n_splits, act;
    int blocks;           // workgroups of the launch
    long long rows_per_split, M, P;

    // rows per row range of the slabs: at most 64 ranges, and a function of M alone
    static long long rows_per_range(long long M) {
        const long long r = 16 * ((M + 1023) / 1024);
        return r > 256 ? r : 256;
    }
    WgPlan(long long M_, long long P_, int act_) : n_layers(0), act(act_), blocks(0), M(M_), P(P_) {
        rows_per_split = rows_per_range(M);
        n_splits = (int)((M + rows_per_split - 1) / rows_per_split);
    }
    // the next parameter pair (weight [N, K], bias [N]), in grads_flat's order
    void add(const float* dz, const float* a, int N, int K, int apply_act) {
        const long long off = n_layers ? layer[n_layers - 1].b_off + layer[n_layers - 1].N : 0;
        layer[n_layers++] = WgLayer{dz, a, N, K, apply_act, blocks, off, off + (long long)N * K};
        blocks += (K + 1 + 15) / 16 * n_splits;
    }
};

// slab[split][w_off + n K + k] = sum over the split's rows of dz[m][n] a[m][k];  column k == K is the bias (a = 1).
// CHUNK == 0: the 16-row steps accumulate straight into `acc`.  CHUNK > 0: blocked summation -- `acc` takes CHUNK steps, then
// joins `total`, so that the rounding error of a 256-row range grows like that of a 32-term sum.  Either order is a function of
// (dims, M) alone.
template <int CHUNK>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(WgPlan plan, float* __restrict__ slab) {
    int li = 0;
    while (li + 1 < plan.n_layers && (int)blockIdx.x >= plan.layer[li + 1].block0) ++li;
    const WgLayer L = plan.layer[li];
    const int local = blockIdx.x - L.block0;
    const int split = local % plan.n_splits, ktile = local / plan.n_splits;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const long long r0 = (long long)split * plan.rows_per_split;
    const long long r1 = r0 + plan.rows_per_split < plan.M ? r0 + plan.rows_per_split : plan.M;
    const int k = ktile * 16 + lr;
    const int n_tiles = (L.N + 15) / 16;

    f32x4 acc[kWgTiles], total[kWgTiles];
#pragma unroll
    for (int i = 0; i < kWgTiles; ++i) acc[i] = total[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    int in_chunk = 0;
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
        if (CHUNK > 0 && ++in_chunk == CHUNK) {
            in_chunk = 0;
#pragma unroll
            for (int i = 0; i < kWgTiles; ++i) {
                total[i] += acc[i];
                acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    if (CHUNK > 0) {
#pragma unroll
        for (int i = 0; i < kWgTiles; ++i) total[i] += acc[i];         // the last, partial chunk (zeros if there is none)
    }
    const f32x4* sum = CHUNK > 0 ? total : acc;
    float* out = slab + (size_t)split * (size_t)plan.P;
#pragma unroll
    for (int i = 0; i < kWgTiles; ++i) {
        const int tile = wid + kWaves * i;
        if (tile < n_tiles) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = tile * 16 + 4 * g + r;
                if (n < L.N) {
                    if (k < L.K) out[L.w_off + (size_t)n * L.K + k] = sum[i][r];
                    else if (k == L.K) out[L.b_off + n] = sum[i][r];
                }
            }
        }
    }
}

// grads (+)= the slabs in row-range order, one thread per parameter element.  (A template, as wgrad_kernel is, so that a unit
// that never launches it -- guide.hip -- carries no copy.)
template <typename T>
__global__ __launch_bounds__(kThreads) void reduce_kernel(const T* __restrict__ slab, T* __restrict__ grads, long long P, int n_splits,
                                                          int accumulate) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= P) return;
    T s = slab[e];
    for (int i = 1; i < n_splits; ++i) s += slab[(size_t)i * (size_t)P + e];
    grads[e] = accumulate ? grads[e] + s : s;
}

// ------------------------------------------------------------------------------------------------------------ host
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// bytes of the weight-gradient slabs behind a unit's chain arrays in the workspace
static size_t slab_bytes(long long M, long long P) {
    const long long R = WgPlan::rows_per_range(M);
    return align256((size_t)((M + R - 1) / R) * (size_t)P * sizeof(float));
}

// The ranges every unit shares.  Every shape error ranks above a bad activation: a unit runs its own shape checks first.
static int check_common(int in_dim, int hidden, int out_dim, int activation, long long M) {
    if (in_dim < 1 || in_dim > kMaxDim || out_dim < 1 || out_dim > kMaxDim) return BESO_ERR_BAD_SHAPE;
    if (hidden < 16 || hidden > kMaxDim || hidden % 16) return BESO_ERR_BAD_SHAPE;
    if (M < 1 || M > 0x7fffffffLL) return BESO_ERR_BAD_SHAPE;
    if (activation < BESO_MLP_ACT_RELU || activation > BESO_MLP_ACT_SIGMOID) return BESO_ERR_BAD_ARG;
    return BESO_OK;
}

static int check_params(const float* const* params, int n_params, int expected) {
    if (!params || n_params != expected) return BESO_ERR_BAD_ARG;
    for (int i = 0; i < n_params; ++i)
        if (!params[i] || ((uintptr_t)params[i] & 3)) return BESO_ERR_BAD_ARG;
    return BESO_OK;
}

// row pitch of the LDS tiles of a network whose widest layer is `widest`
static int tile_pitch(int widest) { return round16(widest) + kLdsPad; }

static unsigned tile_grid(long long M) { return (unsigned)((M + kRows - 1) / kRows); }

// The backward's three launches: the unit's chain kernel (dynamic LDS `lds`, the attribute at its ceiling `lds_max`), the
// weight-gradient partial sums, their reduce.
template <auto Chain, int CHUNK, typename... Args>
static int launch_bwd(size_t lds_max, size_t lds, hipStream_t s, const WgPlan& plan, float* slab, float* grads, int accumulate,
                      const Args&... chain_args) {
    if (launch_lds_attr<Chain>(lds_max, dim3(tile_grid(plan.M)), dim3(kThreads), lds, s, chain_args...) != hipSuccess) return BESO_ERR_HIP;
    if (launch_plain<wgrad_kernel<CHUNK>>(dim3((unsigned)plan.blocks), dim3(kThreads), s, plan, slab) != hipSuccess) return BESO_ERR_HIP;
    return to_status(launch_plain<reduce_kernel<float>>(dim3((unsigned)((plan.P + kThreads - 1) / kThreads)), dim3(kThreads), s,
                                                        (const float*)slab, grads, plan.P, plan.n_splits, accumulate));
}

}  // namespace beso_mlp
