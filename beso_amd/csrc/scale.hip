// The scalings of MinMaxScaler (include/beso_scale.h): libbeso_scale.so.  Two kernels:
//   scale_rows_mixed_kernel     up to four tensors, each z-scored or min-max scaled per feature, grid-stride over all elements
//   rollout_end_minmax_kernel   a thread per (environment, action component): newest action, clip, remember, min-max un-scale
// Copy work of a few KiB with two to four arithmetic operations per element, each stated on its own so that the bits are those of
// the reference's torch expressions: no MFMA, no LDS, no atomics, no workspace.
#include "side_host.h"
#include "../../include/beso_scale.h"

namespace beso_scale {

using namespace beso_side;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

// ------------------------------------------------------------------------------------------------------------ scale_rows_mixed
// Tensor k owns the global element indices [first[k], first[k + 1]); first[n] ... first[kMax] are the total.
struct MixedTable {
    const float* src[BESO_SCALE_MAX_ITEMS];
    float* dst[BESO_SCALE_MAX_ITEMS];
    const float* p0[BESO_SCALE_MAX_ITEMS];
    const float* p1[BESO_SCALE_MAX_ITEMS];
    const float* p2[BESO_SCALE_MAX_ITEMS];
    const float* p3[BESO_SCALE_MAX_ITEMS];
    unsigned long long first[BESO_SCALE_MAX_ITEMS + 1];
    int cols[BESO_SCALE_MAX_ITEMS];
    int kind[BESO_SCALE_MAX_ITEMS];
    int n;
};

__global__ __launch_bounds__(kThreads) void scale_rows_mixed_kernel(MixedTable t) {
#pragma clang fp contract(off)          // every operation is rounded on its own (include/beso_scale.h)
    const unsigned long long total = t.first[t.n];
    for (unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * kThreads) {
        int k = 0;
#pragma unroll
        for (int j = 1; j < BESO_SCALE_MAX_ITEMS; ++j) k += (j < t.n && i >= t.first[j]) ? 1 : 0;
        const unsigned long long e = i - t.first[k];
        const int c = (int)(e % (unsigned long long)t.cols[k]);
        const float x = t.src[k][e];
        float out;
        if (t.kind[k] == BESO_SCALE_ZSCORE) {
            const float d = x - t.p0[k][c];
            out = d / t.p1[k][c];
        } else {
            const float a = x - t.p0[k][c];
            const float b = a / t.p1[k][c];
            const float m = b * t.p2[k][c];
            out = m + t.p3[k][c];
        }
        t.dst[k][e] = out;
    }
}

// ------------------------------------------------------------------------------------------------------------ rollout_end_minmax
__global__ __launch_bounds__(kThreads) void rollout_end_minmax_kernel(
    const float* __restrict__ x0, const int* __restrict__ lengths, const double* __restrict__ lo, const double* __restrict__ hi,
    const float* __restrict__ new_lo, const float* __restrict__ span, const float* __restrict__ range,
    const float* __restrict__ lo_y, float* __restrict__ act_ctx, float* __restrict__ pred, int n_envs, int W, int act) {
#pragma clang fp contract(off)          // MinMaxScaler.inverse_scale_output: four rounded operations
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_envs * act) return;
    const int n = i / act, c = i - n * act;
    int t = lengths[n];
    t = t < 1 ? 1 : (t > W ? W : t);                    // (a length the caller never wrote must not index out of the window)
    const size_t at = ((size_t)n * W + (t - 1)) * act + c;
    // MinMaxScaler.clip_action: torch.clamp of the fp32 action against float64 bounds promotes to float64; the result is rounded
    // to fp32.  (NaN compares false twice and passes through, as clamp propagates it.)
    double v = (double)x0[at];
    if (v < lo[c]) v = lo[c];
    if (v > hi[c]) v = hi[c];
    const float clipped = (float)v;
    act_ctx[at] = clipped;
    float p = clipped;
    if (span) {
        const float a = clipped - new_lo[c];
        const float b = a / span[c];
        const float m = b * range[c];
        p = m + lo_y[c];
    }
    pred[i] = p;
}

// ------------------------------------------------------------------------------------------------------------ host

}  // namespace beso_scale

using namespace beso_scale;

extern "C" const char* beso_scale_last_error(void) { return g_error; }

extern "C" int beso_scale_rows_mixed(const float* const* src, float* const* dst, const int* kind, const float* const* p0,
                                     const float* const* p1, const float* const* p2, const float* const* p3,
                                     const long long* rows, const int* cols, int n, void* stream) {
    const char* fn = "beso_scale_rows_mixed";
    if (n < 1 || n > BESO_SCALE_MAX_ITEMS)
        return refuse(BESO_ERR_BAD_ARG, "%s: n = %d tensors, supported: 1 ... %d", fn, n, BESO_SCALE_MAX_ITEMS);
    if (!src || !dst || !kind || !p0 || !p1 || !rows || !cols)
        return refuse(BESO_ERR_BAD_ARG, "%s: a NULL table (src, dst, kind, p0, p1, rows and cols are required)", fn);
    MixedTable t;
    t.n = n;
    unsigned long long cur = 0;
    for (int k = 0; k < BESO_SCALE_MAX_ITEMS; ++k) {
        t.first[k] = cur;
        t.src[k] = nullptr; t.dst[k] = nullptr; t.p0[k] = t.p1[k] = t.p2[k] = t.p3[k] = nullptr;
        t.cols[k] = 1; t.kind[k] = BESO_SCALE_ZSCORE;
        if (k >= n) continue;
        if (kind[k] != BESO_SCALE_ZSCORE && kind[k] != BESO_SCALE_MINMAX)
            return refuse(BESO_ERR_BAD_ARG, "%s: kind[%d] = %d is neither BESO_SCALE_ZSCORE nor BESO_SCALE_MINMAX", fn, k, kind[k]);
        if (rows[k] < 0 || cols[k] < 1)
            return refuse(BESO_ERR_BAD_SHAPE, "%s: tensor %d is [%lld, %d]: rows must be at least 0 and cols at least 1", fn, k,
                          rows[k], cols[k]);
        if ((unsigned long long)rows[k] > (1ull << 60) / (unsigned long long)cols[k])
            return refuse(BESO_ERR_BAD_SHAPE, "%s: tensor %d is [%lld, %d]: more than 2^60 elements", fn, k, rows[k], cols[k]);
        const bool mm = kind[k] == BESO_SCALE_MINMAX;
        if (mm && (!p2 || !p3)) return refuse(BESO_ERR_BAD_ARG, "%s: tensor %d is BESO_SCALE_MINMAX and the p2 / p3 table is NULL", fn, k);
        if (!src[k] || !dst[k] || !p0[k] || !p1[k] || (mm && (!p2[k] || !p3[k])))
            return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer among src / dst / p0 / p1%s of tensor %d", fn, mm ? " / p2 / p3" : "", k);
        if (misaligned(src[k], 4) || misaligned(dst[k], 4) || misaligned(p0[k], 4) || misaligned(p1[k], 4) ||
            (mm && (misaligned(p2[k], 4) || misaligned(p3[k], 4))))
            return refuse(BESO_ERR_BAD_ARG, "%s: a pointer of tensor %d that is not 4-byte aligned", fn, k);
        t.src[k] = src[k]; t.dst[k] = dst[k]; t.p0[k] = p0[k]; t.p1[k] = p1[k];
        t.p2[k] = mm ? p2[k] : nullptr; t.p3[k] = mm ? p3[k] : nullptr;
        t.cols[k] = cols[k]; t.kind[k] = kind[k];
        cur += (unsigned long long)rows[k] * (unsigned long long)cols[k];
    }
    t.first[BESO_SCALE_MAX_ITEMS] = cur;
    if (cur == 0) return BESO_OK;
    unsigned long long grid = (cur + kThreads - 1) / kThreads;
    if (grid > kMaxBlocks) grid = kMaxBlocks;
    const hipError_t e = beso::launch_plain<scale_rows_mixed_kernel>(dim3((unsigned)grid), dim3(kThreads), (hipStream_t)stream, t);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}

extern "C" int beso_rollout_end_minmax(const float* x0, const int32_t* lengths, const double* lo, const double* hi,
                                       const float* new_lo, const float* span, const float* range, const float* lo_y,
                                       float* act_ctx, float* pred, int n_envs, int window, int act_dim, void* stream) {
    const char* fn = "beso_rollout_end_minmax";
    if (act_dim < 1 || window < 1 || n_envs < 0)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: act_dim = %d and window = %d must be at least 1, n_envs = %d at least 0", fn, act_dim,
                      window, n_envs);
    if ((long long)n_envs * window * act_dim > 0x7fffffffLL)
        return refuse(BESO_ERR_BAD_SHAPE, "%s: n_envs window act_dim = %lld exceeds the int range", fn,
                      (long long)n_envs * window * act_dim);
    if (!x0 || !lengths || !lo || !hi || !act_ctx || !pred)
        return refuse(BESO_ERR_BAD_ARG, "%s: a NULL pointer among x0, lengths, lo, hi, act_ctx and pred", fn);
    const int n_stats = (new_lo != nullptr) + (span != nullptr) + (range != nullptr) + (lo_y != nullptr);
    if (n_stats != 0 && n_stats != 4)
        return refuse(BESO_ERR_BAD_ARG, "%s: new_lo, span, range and lo_y must be given together or all be NULL (%d of 4 given)", fn,
                      n_stats);
    if (misaligned(x0, 4) || misaligned(lengths, 4) || misaligned(act_ctx, 4) || misaligned(pred, 4) || misaligned(new_lo, 4) ||
        misaligned(span, 4) || misaligned(range, 4) || misaligned(lo_y, 4))
        return refuse(BESO_ERR_BAD_ARG, "%s: an fp32 / int32 pointer that is not 4-byte aligned", fn);
    if (misaligned(lo, 8) || misaligned(hi, 8)) return refuse(BESO_ERR_BAD_ARG, "%s: lo / hi are float64 and must be 8-byte aligned", fn);
    if (n_envs == 0) return BESO_OK;
    const int total = n_envs * act_dim;
    const hipError_t e = beso::launch_plain<rollout_end_minmax_kernel>(
        dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), (hipStream_t)stream, x0, (const int*)lengths, lo, hi,
        new_lo, span, range, lo_y, act_ctx, pred, n_envs, window, act_dim);
    if (e != hipSuccess) return refuse(BESO_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    return BESO_OK;
}
