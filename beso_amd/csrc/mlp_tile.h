// What the two encoder units (encoder.hip: libbeso_mlp.so; resmlp.hip: libbeso_resmlp.so) share: the 16-row tile GEMMs on
// v_mfma_f32_16x16x4_f32, the activations, and the row-range rule of the weight-gradient slabs.
// MFMA operand layout (as gemm.hip): A lane -> (row = lane & 15, k = lane >> 4), B lane -> (k = lane >> 4, col = lane & 15),
// C lane -> (col = lane & 15, rows 4 (lane >> 4) + r).  A 16-wide k group is fed as four MFMAs; MFMA j takes
// k = k0 + 4 (lane >> 4) + j from BOTH operands, so a lane reads four consecutive k of its row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/beso_hip.h"
#include "../../include/beso_mlp.h"

namespace beso_mlp {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int kRows = 16;          // rows of x per workgroup (one MFMA tile)
constexpr int kThreads = 256;      // four waves: a layer's 16-column output tiles are dealt round-robin to them
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 512;
constexpr int kLdsPad = 4;         // row pitch = width + 4 floats: 16 rows of a float4 column hit 64 distinct banks
constexpr int kWgTiles = kMaxDim / 16 / kWaves;   // output-row tiles of dW one wave of a weight-gradient kernel owns: 8

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

// One layer of the backward chain on the tile: out[16, K] = in[16, N] W[N, K], handed to `epi(row, k, value)` for k < K.
// `in` is zero beyond N up to round16(N).
template <typename Epi>
__device__ __forceinline__ void tile_xw(const float* in, int pitch, const float* __restrict__ W, int N, int K, Epi epi) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    const int Np = round16(N);
    for (int k0 = wid * 16; k0 < K; k0 += kWaves * 16) {
        const int k = k0 + lr;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int n0 = 0; n0 < Np; n0 += 16) {
            const int n = n0 + 4 * g;
            const f32x4 a = *(const f32x4*)(in + lr * pitch + n);
            f32x4 b;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = (k < K && n + j < N) ? W[(size_t)(n + j) * K + k] : 0.f;
            acc = mfma4(acc, a, b);
        }
        if (k < K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(4 * g + r, k, acc[r]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
// rows per row range of the weight-gradient slabs: at most 64 ranges, and a function of M alone
static long long rows_per_split(long long M) {
    const long long r = 16 * ((M + 1023) / 1024);
    return r > 256 ? r : 256;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

template <typename K> static hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace beso_mlp
