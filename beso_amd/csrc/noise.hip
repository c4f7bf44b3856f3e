// Keyed standard-normal draws for rollout inference (include/beso_noise.h): libbeso_noise.so.  One kernel:
//   keyed_noise_kernel   a thread per Philox4x32-10 block (four elements) of up to three output arrays; the rollout form also
//                        advances the per-environment counters, from one pair of arrays into another
// A value depends on (key, episode, step, purpose, slab, element) only: no thread reads what another wrote.  Plain loads and
// stores, no MFMA, no LDS, no atomics, no workspace.  The launch is bound by its round trip, not by its arithmetic.
#include "side_host.h"
#include "../../include/beso_noise.h"

#include <cmath>

namespace beso_noise {

using namespace beso_side;

using beso::f32x4;
using beso::u32x4;

constexpr int kThreads = 256;
constexpr int kMaxSegments = 3;

// One output array: out[s * stride_s + n * stride_n + e], s < S, n < N, e < E.  Its blocks are the global block indices
// [first, first + S N quads), slab-major, then environment, then block of the row.
struct Segment {
    void* out;
    unsigned long long first;
    long long stride_s, stride_n;
    int purpose, E, quads;
    int vec;                      // E % 4 == 0, both strides % 4 == 0 and `out` 16-byte aligned: one 16-byte store per block
};
struct Table {
    Segment seg[kMaxSegments];
    unsigned long long total;     // blocks of all segments
    int n_seg, N;
};

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return u32x4{c0, c1, c2, c3};
}

// Two words -> one Box-Muller pair, operation by operation as include/beso_noise.h states it.
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& za, float& zb) {
#pragma clang fp contract(off)
    const float u = (float)((wa >> 8) + 1u) * 0x1p-24f;
    const float v = (float)(wb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u));
    const float t = 6.2831855f * v;
    za = r * cosf(t);
    zb = r * sinf(t);
}

template <bool WORDS, bool ADVANCE>
__global__ __launch_bounds__(kThreads) void keyed_noise_kernel(
    const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ reset, const uint32_t* __restrict__ episodes_in,
    const uint32_t* __restrict__ steps_in, uint32_t* __restrict__ episodes_out, uint32_t* __restrict__ steps_out, float scale,
    Table t) {
#pragma clang fp contract(off)
    const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= t.total) return;
    int k = 0;
#pragma unroll
    for (int j = 1; j < kMaxSegments; ++j) k += (j < t.n_seg && i >= t.seg[j].first) ? 1 : 0;
    const Segment sg = t.seg[k];
    const unsigned long long local = i - sg.first;
    const int q = (int)(local % (unsigned)sg.quads);
    const unsigned long long row = local / (unsigned)sg.quads;
    const int n = (int)(row % (unsigned)t.N);
    const int s = (int)(row / (unsigned)t.N);

    uint32_t episode = episodes_in[n], step = steps_in[n];
    if (ADVANCE) {
        if (reset != nullptr && reset[n]) {
            episode += 1u;
            step = 0u;
        } else {
            step += 1u;
        }
        // segment 0 is x_t, one slab: its first block of environment n is the one writer of n's advanced counters (into
        // arrays no thread of the launch reads)
        if (k == 0 && q == 0) {
            episodes_out[n] = episode;
            steps_out[n] = step;
        }
    }
    const unsigned long long key = keys[n];
    const u32x4 w = philox4x32_10((uint32_t)q, (uint32_t)s, step, (episode << 4) | (uint32_t)sg.purpose, (uint32_t)key,
                                  (uint32_t)(key >> 32));
    const size_t at = (size_t)((long long)s * sg.stride_s + (long long)n * sg.stride_n) + 4 * (size_t)q;
    const int left = sg.E - 4 * q;                       // elements of the row from this block on: 1 ... 4 are written
    if (WORDS) {
        uint32_t* out = reinterpret_cast<uint32_t*>(sg.out) + at;
        if (sg.vec) {
            *reinterpret_cast<u32x4*>(out) = w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < left) out[c] = w[c];
        }
    } else {
        f32x4 z;
        float za, zb;
        box_muller(w[0], w[1], za, zb);
        z[0] = za * scale;
        z[1] = zb * scale;
        box_muller(w[2], w[3], za, zb);
        z[2] = za * scale;
        z[3] = zb * scale;
        float* out = reinterpret_cast<float*>(sg.out) + at;
        if (sg.vec) {
            *reinterpret_cast<f32x4*>(out) = z;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < left) out[c] = z[c];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

// Appends out[S][N][E] with the given strides (in elements) to the table.
static void add_segment(Table& t, void* out, int purpose, int S, int E, long long stride_s, long long stride_n) {
    Segment& sg = t.seg[t.n_seg++];
    sg.out = out;
    sg.first = t.total;
    sg.stride_s = stride_s;
    sg.stride_n = stride_n;
    sg.purpose = purpose;
    sg.E = E;
    sg.quads = (E + 3) / 4;
    sg.vec = E % 4 == 0 && stride_s % 4 == 0 && stride_n % 4 == 0 && !misaligned(out, 16);
    t.total += (unsigned long long)S * (unsigned long long)t.N * (unsigned long long)sg.quads;
}

template <bool WORDS, bool ADVANCE>
static int launch(const char* fn, const Table& t, const uint64_t* keys, const uint8_t* reset, const uint32_t* episodes_in,
                  const uint32_t* steps_in, uint32_t* episodes_out, uint32_t* steps_out, float scale, void* stream) {
    const dim3 grid((unsigned)((t.total + kThreads - 1) / kThreads)), block(kThreads);
    const hipError_t e = beso::launch_plain<keyed_noise_kernel<WORDS, ADVANCE>>(
        grid, block, (hipStream_t)stream, (const unsigned long long*)keys, reset, episodes_in, steps_in, episodes_out, steps_out,
        scale, t);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}

// The checks beso_noise_words and beso_noise_normal share.
static int check_plain(const char* fn, const uint64_t* keys, const uint32_t* episodes, const uint32_t* steps, int N, int purpose,
                       int S, int E, const void* out) {
    if (N < 1 || S < 1 || E < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: N = %d, S = %d, E = %d must all be at least 1", fn, N, S, E);
    if ((long long)S * N * E > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: S N E = %lld elements exceed the int range", fn, (long long)S * N * E);
    if (purpose < 0 || purpose > BESO_NOISE_MAX_PURPOSE)
        return refuse(BESO_ERR_BAD_ARG, "%s: purpose = %d, supported: 0 ... %d", fn, purpose, BESO_NOISE_MAX_PURPOSE);
    if (!keys || !episodes || !steps || !out) return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer", fn);
    if (misaligned(keys, 8) || misaligned(episodes, 4) || misaligned(steps, 4) || misaligned(out, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: a pointer that is not aligned to its element (keys: 8 bytes, else 4)", fn);
    return BESO_OK;
}

}  // namespace beso_noise

using namespace beso_noise;

extern "C" const char* beso_noise_last_error(void) { return g_error; }

extern "C" int beso_noise_words(const uint64_t* keys, const uint32_t* episodes, const uint32_t* steps, int N, int purpose, int S,
                                int E, uint32_t* out, void* stream) {
    const char* fn = "beso_noise_words";
    if (const int st = check_plain(fn, keys, episodes, steps, N, purpose, S, E, out)) return st;
    Table t = {};
    t.N = N;
    add_segment(t, out, purpose, S, E, (long long)N * E, E);
    return launch<true, false>(fn, t, keys, nullptr, episodes, steps, nullptr, nullptr, 1.0f, stream);
}

extern "C" int beso_noise_normal(const uint64_t* keys, const uint32_t* episodes, const uint32_t* steps, int N, int purpose, int S,
                                 int E, float scale, float* out, void* stream) {
    const char* fn = "beso_noise_normal";
    if (const int st = check_plain(fn, keys, episodes, steps, N, purpose, S, E, out)) return st;
    if (!std::isfinite(scale)) return refuse(BESO_ERR_BAD_ARG, "%s: the scale is not finite", fn);
    Table t = {};
    t.N = N;
    add_segment(t, out, purpose, S, E, (long long)N * E, E);
    return launch<false, false>(fn, t, keys, nullptr, episodes, steps, nullptr, nullptr, scale, stream);
}

extern "C" int beso_noise_rollout(const uint64_t* keys, const uint8_t* reset, const uint32_t* episodes_in, const uint32_t* steps_in,
                                  uint32_t* episodes_out, uint32_t* steps_out, int N, int act_dim, int K, int n_steps,
                                  int step_elems, float* x_t, float* cand, float* step_noise, void* stream) {
    const char* fn = "beso_noise_rollout";
    if (N < 1 || act_dim < 1) return refuse(BESO_ERR_BAD_SHAPE, "%s: N = %d and act_dim = %d must be at least 1", fn, N, act_dim);
    if (K < 0 || n_steps < 0) return refuse(BESO_ERR_BAD_SHAPE, "%s: K = %d and n_steps = %d must not be negative", fn, K, n_steps);
    if (n_steps > 0 && step_elems < 1)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: step_elems = %d must be at least 1 with n_steps = %d", fn, step_elems, n_steps);
    const long long n_cand = (long long)N * (K > 0 ? K : 1) * act_dim;
    const long long n_step = n_steps > 0 ? (long long)n_steps * N * step_elems : 0;
    if (n_cand > 0x7fffffffLL || n_step > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: N K act_dim = %lld or n_steps N step_elems = %lld elements exceed the int range", fn,
                      n_cand, n_step);
    if (!keys || !episodes_in || !steps_in || !episodes_out || !steps_out || !x_t)
        return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer", fn);
    if ((K > 0) != (cand != nullptr)) return refuse(BESO_ERR_BAD_ARG, "%s: cand goes with K > 0 and is NULL with K = 0 (K = %d)", fn, K);
    if ((n_steps > 0) != (step_noise != nullptr))
        return refuse(BESO_ERR_BAD_ARG, "%s: step_noise goes with n_steps > 0 and is NULL with n_steps = 0 (n_steps = %d)", fn, n_steps);
    if (misaligned(keys, 8) || misaligned(episodes_in, 4) || misaligned(steps_in, 4) || misaligned(episodes_out, 4) ||
        misaligned(steps_out, 4) || misaligned(x_t, 4) || misaligned(cand, 4) || misaligned(step_noise, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: a pointer that is not aligned to its element (keys: 8 bytes, else 4)", fn);
    const size_t cb = (size_t)N * sizeof(uint32_t);
    if (overlap(episodes_out, episodes_in, cb) || overlap(episodes_out, steps_in, cb) || overlap(steps_out, episodes_in, cb) ||
        overlap(steps_out, steps_in, cb) || overlap(episodes_out, steps_out, cb))
        return refuse(BESO_ERR_BAD_ARG, "%s: the counters written overlap the counters read (or each other): alternate between two pairs", fn);
    Table t = {};
    t.N = N;
    add_segment(t, x_t, BESO_NOISE_XT, 1, act_dim, 0, act_dim);
    if (K > 0) add_segment(t, cand, BESO_NOISE_CANDIDATE, K, act_dim, act_dim, (long long)K * act_dim);
    if (n_steps > 0) add_segment(t, step_noise, BESO_NOISE_STEP, n_steps, step_elems, (long long)N * step_elems, step_elems);
    return launch<false, true>(fn, t, keys, reset, episodes_in, steps_in, episodes_out, steps_out, 1.0f, stream);
}
