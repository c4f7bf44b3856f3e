// The attention of the training step (train.hip), forward with dropout on the probabilities and backward.  Included by
// train.hip INSIDE its `namespace beso { namespace { ... } }`: everything here keeps the internal linkage it had as part of
// that file.
// Provides: the generic pair attn_fwd_kernel / attn_bwd_kernel (AttnLds, attn_carve, attn_lds_bytes, attn_load_scores); the
//   short-sequence attn_small_kernel (dot_rows, row16_allreduce); the matrix-pipe backward attn_mfma_bwd_kernel (row_chunk16,
//   pack4_bf16, cross_rows_allreduce).
// Needs: common.h only (included by the unit in front of its namespace).  Sees neither train_gemm.h nor train_rows.h nor the host.
#pragma once

// ---------------------------------------------------------------------------------------------
// attention of one (sample, head) per wave, forward (training: dropout on the probabilities, score_gpts.py:69-76)
// and backward.  q/k/v rows of the head in LDS as fp32; T x T scores in LDS.  qkv row layout [q | k | v].
// ---------------------------------------------------------------------------------------------
struct AttnLds { float *q, *k, *v, *dy, *P, *dP; int ldh, ldt; };
__device__ __forceinline__ AttnLds attn_carve(float* base, int T, int hd, bool bwd) {
    AttnLds a;
    a.ldh = hd + 1; a.ldt = T + 1;
    a.q = base; a.k = a.q + T * a.ldh; a.v = a.k + T * a.ldh;
    a.dy = a.v + T * a.ldh;
    a.P = a.dy + (bwd ? T * a.ldh : 0);
    a.dP = a.P + T * a.ldt;
    return a;
}
size_t attn_lds_bytes(int T, int hd, bool bwd) {
    return sizeof(float) * ((size_t)(bwd ? 4 : 3) * T * (hd + 1) + (size_t)(bwd ? 2 : 1) * T * (T + 1));
}

// P (pre-dropout probabilities) for all rows; lanes stride over rows
template <typename E>
__device__ __forceinline__ void attn_load_scores(const E* __restrict__ qkv, const AttnLds& a, int b, int h, int T,
                                                 int D, int hd, float scale, int lane) {
    const size_t ldq = (size_t)3 * D;
    // four elements per lane in flight (12 loads issued before the first is used; clamped index, no branch)
    const int n_el = T * hd;
    for (int u0 = lane; u0 < n_el; u0 += 256) {
        E qv[4], kv[4], vv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = min(u0 + 64 * j, n_el - 1), r = u / hd, d = u - r * hd;
            const E* src = qkv + ((size_t)b * T + r) * ldq + (size_t)h * hd + d;
            qv[j] = src[0]; kv[j] = src[D]; vv[j] = src[2 * D];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = u0 + 64 * j;
            if (u < n_el) {
                const int r = u / hd, d = u - r * hd;
                a.q[r * a.ldh + d] = Act<E>::to(qv[j]);
                a.k[r * a.ldh + d] = Act<E>::to(kv[j]);
                a.v[r * a.ldh + d] = Act<E>::to(vv[j]);
            }
        }
    }
    __syncthreads();
    for (int u = lane; u < T * T; u += 64) {
        const int i = u / T, j = u % T;
        float s = -INFINITY;
        if (j <= i) {
            s = 0.f;
            for (int d = 0; d < hd; ++d) s = fmaf(a.q[i * a.ldh + d], a.k[j * a.ldh + d], s);
            s *= scale;
        }
        a.P[i * a.ldt + j] = s;
    }
    __syncthreads();
    for (int i = lane; i < T; i += 64) {
        float m = -INFINITY;
        for (int j = 0; j <= i; ++j) m = fmaxf(m, a.P[i * a.ldt + j]);
        float l = 0.f;
        for (int j = 0; j <= i; ++j) { const float e = expf(a.P[i * a.ldt + j] - m); a.P[i * a.ldt + j] = e; l += e; }
        const float inv = 1.0f / l;
        for (int j = 0; j < T; ++j) a.P[i * a.ldt + j] = j <= i ? a.P[i * a.ldt + j] * inv : 0.f;
    }
    __syncthreads();
}

template <typename E>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const E* __restrict__ qkv, E* __restrict__ y, int T, int D, int H,
                                                      int hd, float scale, float p, float inv_keep, uint32_t seed,
                                                      uint32_t site) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int pair = blockIdx.x, b = pair / H, h = pair % H, lane = threadIdx.x;
    const AttnLds a = attn_carve(smem_f, T, hd, false);
    attn_load_scores<E>(qkv, a, b, h, T, D, hd, scale, lane);
    if (p > 0.f) {
        for (int u = lane; u < T * T; u += 64) {
            const int i = u / T, j = u % T;
            a.P[i * a.ldt + j] *= drop_scale(seed, site, (size_t)pair * T * T + u, p, inv_keep);
        }
        __syncthreads();
    }
    for (int u = lane; u < T * hd; u += 64) {
        const int i = u / hd, d = u % hd;
        float o = 0.f;
        for (int j = 0; j <= i; ++j) o = fmaf(a.P[i * a.ldt + j], a.v[j * a.ldh + d], o);
        y[((size_t)b * T + i) * D + (size_t)h * hd + d] = Act<E>::from(o);
    }
}

template <typename E>
__global__ __launch_bounds__(64) void attn_bwd_kernel(const E* __restrict__ qkv, const E* __restrict__ dy,
                                                      E* __restrict__ dqkv, int T, int D, int H, int hd, float scale,
                                                      float p, float inv_keep, uint32_t seed, uint32_t site) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int pair = blockIdx.x, b = pair / H, h = pair % H, lane = threadIdx.x;
    const AttnLds a = attn_carve(smem_f, T, hd, true);
    attn_load_scores<E>(qkv, a, b, h, T, D, hd, scale, lane);
    for (int u0 = lane; u0 < T * hd; u0 += 256) {
        E gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = min(u0 + 64 * j, T * hd - 1), r = u / hd, d = u - r * hd;
            gv[j] = dy[((size_t)b * T + r) * D + (size_t)h * hd + d];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int u = u0 + 64 * j;
            if (u < T * hd) { const int r = u / hd, d = u - r * hd; a.dy[r * a.ldh + d] = Act<E>::to(gv[j]); }
        }
    }
    __syncthreads();
    // dP[i][j] = keep-scale * sum_d dy[i][d] v[j][d]   (gradient w.r.t. the pre-dropout probability)
    for (int u = lane; u < T * T; u += 64) {
        const int i = u / T, j = u % T;
        float g = 0.f;
        if (j <= i) {
            for (int d = 0; d < hd; ++d) g = fmaf(a.dy[i * a.ldh + d], a.v[j * a.ldh + d], g);
            if (p > 0.f) g *= drop_scale(seed, site, (size_t)pair * T * T + u, p, inv_keep);
        }
        a.dP[i * a.ldt + j] = g;
    }
    __syncthreads();
    const size_t ldq = (size_t)3 * D;
    // dv[j][d] = sum_{i>=j} Pd[i][j] dy[i][d]  (Pd = P * keep-scale) -- before dP is turned into dS
    for (int u = lane; u < T * hd; u += 64) {
        const int j = u / hd, d = u % hd;
        float g = 0.f;
        for (int i = j; i < T; ++i) {
            float pd = a.P[i * a.ldt + j];
            if (p > 0.f) pd *= drop_scale(seed, site, (size_t)pair * T * T + (size_t)i * T + j, p, inv_keep);
            g = fmaf(pd, a.dy[i * a.ldh + d], g);
        }
        dqkv[((size_t)b * T + j) * ldq + 2 * (size_t)D + (size_t)h * hd + d] = Act<E>::from(g);
    }
    __syncthreads();
    // dS[i][j] = P[i][j] * (dP[i][j] - sum_j' dP[i][j'] P[i][j'])
    for (int i = lane; i < T; i += 64) {
        float dot = 0.f;
        for (int j = 0; j <= i; ++j) dot = fmaf(a.dP[i * a.ldt + j], a.P[i * a.ldt + j], dot);
        for (int j = 0; j < T; ++j)
            a.dP[i * a.ldt + j] = j <= i ? a.P[i * a.ldt + j] * (a.dP[i * a.ldt + j] - dot) * scale : 0.f;
    }
    __syncthreads();
    for (int u = lane; u < T * hd; u += 64) {
        const int r = u / hd, d = u % hd;
        float gq = 0.f, gk = 0.f;
        for (int j = 0; j <= r; ++j) gq = fmaf(a.dP[r * a.ldt + j], a.k[j * a.ldh + d], gq);
        for (int i = r; i < T; ++i) gk = fmaf(a.dP[i * a.ldt + r], a.q[i * a.ldh + d], gk);
        E* dst = dqkv + ((size_t)b * T + r) * ldq + (size_t)h * hd + d;
        dst[0] = Act<E>::from(gq);
        dst[D] = Act<E>::from(gk);
    }
}

// ---------------------------------------------------------------------------------------------
// Short sequences (T <= 16, hd <= 64, hd % 4 == 0: kitchen T = 11 / hd = 60, block-push T = 12 / hd = 20): the
// same attention, forward or backward, with lane d holding column d of q / k / v (/ dy) in registers.  All global
// loads are issued before the first use; the T x T parts run on a (4 rows x 16 columns) lane grid with float4
// dot products from LDS (row stride 68 floats: conflict-free b128 reads), the d-parallel parts read the T x T
// matrices as broadcasts.
// ---------------------------------------------------------------------------------------------
constexpr int kTP = 16, kLdh = 68, kLdt = 20;

__device__ __forceinline__ float dot_rows(const float* a, const float* b, int hd) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < hd; d += 4) acc += *(const f32x4*)(a + d) * *(const f32x4*)(b + d);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// all-reduce over the 16 lanes of a DPP row (lanes 16 r .. 16 r + 15): every lane receives the row's sum / maximum
template <bool IS_MAX>
__device__ __forceinline__ float row16_allreduce(float v) {
    auto dpp = [](float x, auto CTRL) {
        return __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), decltype(CTRL)::value, 0xf, 0xf, false));
    };
    auto op = [](float a, float b) { return IS_MAX ? fmaxf(a, b) : a + b; };
    v = op(v, dpp(v, std::integral_constant<int, 0xB1>{}));       // quad_perm [1,0,3,2]
    v = op(v, dpp(v, std::integral_constant<int, 0x4E>{}));       // quad_perm [2,3,0,1]
    v = op(v, dpp(v, std::integral_constant<int, 0x124>{}));      // row_ror:4
    v = op(v, dpp(v, std::integral_constant<int, 0x128>{}));      // row_ror:8
    return v;
}

template <typename E, bool BWD, int TT>          // TT = T rounded up to a multiple of 4 (8, 12 or 16)
__global__ __launch_bounds__(64) void attn_small_kernel(const E* __restrict__ qkv, const E* __restrict__ dy,
                                                        E* __restrict__ out, int T, int D, int H, int hd, float scale,
                                                        float p, float inv_keep, uint32_t seed, uint32_t site) {
    // q | k rows for the scores; the backward then re-uses the two buffers for dy | v (round 4: 15 -> 9.4 KiB per wave, i.e.
    // 16 instead of 10 waves per CU -- the kernel is a latency chain per (sample, head), so waves in flight are its rate)
    __shared__ __attribute__((aligned(16))) float sq[TT][kLdh], sk[TT][kLdh];
    __shared__ __attribute__((aligned(16))) float sP[TT][kLdt], sdP[BWD ? TT : 1][kLdt];
    const int pair = blockIdx.x, b = pair / H, h = pair % H, lane = threadIdx.x;
    const size_t ldq = (size_t)3 * D;
    const bool act = lane < hd;
    float qr[TT], kr[TT], vr[TT], gr[TT];
    {
        // branch-free: out-of-range rows / lanes read a clamped address and are zeroed afterwards (a load inside a
        // divergent branch is waited for before the next one is issued: 48 serial round trips)
        const int lc = act ? lane : 0;
        const E* base = qkv + (size_t)b * T * ldq + (size_t)h * hd + lc;
        const E* gbase = dy + (size_t)b * T * D + (size_t)h * hd + lc;
        E qe[TT], ke[TT], ve[TT], ge[TT];
#pragma unroll
        for (int r = 0; r < TT; ++r) {
            const int rc = r < T ? r : 0;
            qe[r] = base[rc * ldq];
            ke[r] = base[rc * ldq + D];
            ve[r] = base[rc * ldq + 2 * D];
            if (BWD) ge[r] = gbase[(size_t)rc * D];
        }
#pragma unroll
        for (int r = 0; r < TT; ++r) {
            const bool ok = act && r < T;
            qr[r] = ok ? Act<E>::to(qe[r]) : 0.f;
            kr[r] = ok ? Act<E>::to(ke[r]) : 0.f;
            vr[r] = ok ? Act<E>::to(ve[r]) : 0.f;
            gr[r] = (BWD && ok) ? Act<E>::to(ge[r]) : 0.f;
        }
    }
#pragma unroll
    for (int r = 0; r < TT; ++r) { sq[r][lane] = qr[r]; sk[r][lane] = kr[r]; }
    __syncthreads();
    // scores on the 4 x 16 lane grid: lane (il, j) holds S[4 ib + il][j] for ib = 0 .. TT/4 - 1
    const int il = lane >> 4, j = lane & 15;
    float sc[TT / 4], dpd[TT / 4];
#pragma unroll
    for (int ib = 0; ib < TT / 4; ++ib) {
        const int i = ib * 4 + il;
        const bool in = i < T && j <= i;
        sc[ib] = in ? dot_rows(sq[i], sk[j < TT ? j : 0], hd) * scale : -INFINITY;
    }
    if (BWD) {
        __syncthreads();                              // every score is read: dy | v take the buffers' place
#pragma unroll
        for (int r = 0; r < TT; ++r) { sq[r][lane] = gr[r]; sk[r][lane] = vr[r]; }
        __syncthreads();
#pragma unroll
        for (int ib = 0; ib < TT / 4; ++ib) {
            const int i = ib * 4 + il;
            dpd[ib] = (i < T && j <= i) ? dot_rows(sq[i], sk[j < TT ? j : 0], hd) : 0.f;      // dPd = dy v^T
        }
    }
    // row softmax IN the lane grid (a row's 16 columns are the 16 lanes of a DPP row): max, exp, sum, the dropout keep-scale
    // of the lane's own element and -- backward -- dS, all lanes busy (round 3: T lanes, each a serial loop over its row)
#pragma unroll
    for (int ib = 0; ib < TT / 4; ++ib) {
        const int i = ib * 4 + il;
        const bool in = i < T && j <= i;
        const float m = row16_allreduce<true>(sc[ib]);
        const float e = in ? expf(sc[ib] - m) : 0.f;
        const float l = row16_allreduce<false>(e);
        const float pr = in ? e * (1.0f / l) : 0.f;
        const float ks = (p > 0.f && in) ? drop_scale(seed, site, (size_t)pair * T * T + (size_t)i * T + j, p, inv_keep) : 1.f;
        if (BWD) {
            const float dot = row16_allreduce<false>(dpd[ib] * ks * pr);
            if (i < TT && j < kLdt) sdP[i][j] = pr * (dpd[ib] * ks - dot) * scale;       // dS
        }
        if (i < TT && j < kLdt) sP[i][j] = pr * ks;                                       // Pd
    }
    __syncthreads();
    if (!act) return;
    // the d-parallel products walk the lower triangle only: row i needs columns 0 .. i (in groups of four)
    if (!BWD) {
        E* o = out + (size_t)b * T * D + (size_t)h * hd + lane;
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            if (i < T) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c <= (i | 3) && c < TT; c += 4) {
                    const f32x4 pv = *(const f32x4*)&sP[i][c];
                    acc = fmaf(pv[0], vr[c], acc); acc = fmaf(pv[1], vr[c + 1], acc);
                    acc = fmaf(pv[2], vr[c + 2], acc); acc = fmaf(pv[3], vr[c + 3], acc);
                }
                o[(size_t)i * D] = Act<E>::from(acc);
            }
        }
    } else {
        // dq[i] = sum_j dS[i][j] k[j];  dk[j] = sum_i dS[i][j] q[i];  dv[j] = sum_i Pd[i][j] dy[i]
        float dq[TT], dk[TT], dv[TT];
#pragma unroll
        for (int r = 0; r < TT; ++r) { dq[r] = 0.f; dk[r] = 0.f; dv[r] = 0.f; }
#pragma unroll
        for (int i = 0; i < TT; ++i) {
            if (i < T) {
#pragma unroll
                for (int c = 0; c <= (i | 3) && c < TT; c += 4) {
                    const f32x4 ds = *(const f32x4*)&sdP[i][c], pd = *(const f32x4*)&sP[i][c];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        dq[i] = fmaf(ds[e], kr[c + e], dq[i]);
                        dk[c + e] = fmaf(ds[e], qr[i], dk[c + e]);
                        dv[c + e] = fmaf(pd[e], gr[i], dv[c + e]);
                    }
                }
            }
        }
        E* o = out + (size_t)b * T * ldq + (size_t)h * hd + lane;
#pragma unroll
        for (int r = 0; r < TT; ++r) {
            if (r < T) {
                o[r * ldq] = Act<E>::from(dq[r]);
                o[r * ldq + D] = Act<E>::from(dk[r]);
                o[r * ldq + 2 * D] = Act<E>::from(dv[r]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The same backward on the matrix pipe (bf16 operands, T <= 16, hd <= 64, hd % 4 == 0; round 4).  The VALU kernel above is a
// latency chain of ~29 k cycles per (sample, head): hundreds of dependent LDS round trips for 72 kFLOP.  Here a wave's products
// are 20 MFMAs and everything between them stays in registers:
//   S^T = K Q^T and S = Q K^T, dPd^T = V dY^T and dPd = dY V^T      8 x v_mfma_f32_16x16x32_bf16: both operands of every one are
//        row chunks (lane (x, g): columns 32 kk + 8 g .. + 7 of row x), loaded from global in fragment order, used as A or B
//   the two layouts of the T x T matrices -- "T": lane (i, g) holds keys j = 4 g + r; "N": lane (j, g) holds queries i = 4 g + r
//        -- are what the second stage needs as B operands as they stand (k index 4 g + r), so softmax, dropout and dS are
//        evaluated in both (T: reductions over r and across the four lane rows; N: over the 16 lanes of a DPP row)
//   dq^T = K^T dS^T, dk^T = Q^T dS, dv^T = dY^T Pd                  12 x v_mfma_f32_16x16x16_bf16: A = the transposed operand from a
//        row-major LDS copy (ds_read_b64_tr_b16), D: lane (token, g) holds dims 16 dt + 4 g .. + 3 = one 8-byte store
// Same dropout mask as attn_small_kernel (hash of (pair T + i) T + j).  Four (sample, head) pairs per workgroup, no barriers.
// ---------------------------------------------------------------------------------------------
constexpr int kAmLd = 72;                          // halfwords per LDS row: 64 dims + pad (144 B: the transpose reads spread over banks)

__device__ __forceinline__ u32x4 row_chunk16(const uint16_t* __restrict__ base, size_t ld, int x, int c0, int T, int hd) {
    // ONE 16-byte request per chunk (a head's rows are 8-byte aligned when hd is not a multiple of 8: global memory takes the
    // unaligned dwordx4).  A chunk that straddles the end of the head (hd = 60: columns 56 .. 63) is fetched as the head's last
    // eight columns and shifted down, so nothing behind the head -- or the tensor -- is read.  hd >= 8 (the launch site sends
    // hd = 4 to attn_small_kernel: min(c0, hd - 8) would start in front of the row), a multiple of 4.
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
    const uint16_t* p = base + (size_t)min(x, T - 1) * ld;
    const int cl = min(c0, hd - 8);
    const u32x4_a8 v = *(const u32x4_a8*)(p + cl);
    // (selects, not branches: a branch between the loads makes each of them wait for the one before)
    const bool shifted = cl != c0, half = c0 - cl == 4;               // (c0 - cl is 0, 4 or >= 8)
    const bool lo_on = x < T && c0 < hd, hi_on = x < T && c0 + 4 < hd;
    const uint32_t l0 = shifted ? (half ? v[2] : 0u) : v[0], l1 = shifted ? (half ? v[3] : 0u) : v[1];
    const uint32_t h0 = shifted ? 0u : v[2], h1 = shifted ? 0u : v[3];
    return u32x4{lo_on ? l0 : 0u, lo_on ? l1 : 0u, hi_on ? h0 : 0u, hi_on ? h1 : 0u};
}
__device__ __forceinline__ uint2 pack4_bf16(float a, float b, float c, float d) {
    typedef __attribute__((ext_vector_type(2))) float f2_t;
    typedef __attribute__((ext_vector_type(2))) __bf16 b2_t;
    const f2_t v0 = {a, b}, v1 = {c, d};                 // v_cvt_pk_bf16_f32 (RNE)
    return make_uint2(__builtin_bit_cast(uint32_t, __builtin_convertvector(v0, b2_t)),
                      __builtin_bit_cast(uint32_t, __builtin_convertvector(v1, b2_t)));
}
// sum / maximum over the four lane rows (lanes x, x + 16, x + 32, x + 48), in every lane
template <bool IS_MAX>
__device__ __forceinline__ float cross_rows_allreduce(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
    const u32x2_t a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float r = IS_MAX ? fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])) : __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const u32x2_t b = __builtin_amdgcn_permlane32_swap(__float_as_uint(r), __float_as_uint(r), false, false);
    return IS_MAX ? fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1])) : __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

__global__ __launch_bounds__(256) void attn_mfma_bwd_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dy,
                                                            uint16_t* __restrict__ dqkv, int n_pairs, int T, int D, int H, int hd,
                                                            float scale, float p, float inv_keep, uint32_t seed, uint32_t site) {
    __shared__ __attribute__((aligned(16))) uint16_t sm[4][3][16][kAmLd];       // per wave: q, k, dy row-major
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, x = lane & 15, g = lane >> 4;
    const int pair = blockIdx.x * 4 + wid;
    if (pair >= n_pairs) return;                     // (wave-uniform; the kernel has no workgroup barrier)
    const int b = pair / H, h = pair % H;
    const size_t ldq = (size_t)3 * D;
    const uint16_t* qb = qkv + (size_t)b * T * ldq + (size_t)h * hd;
    const uint16_t* gb = dy + (size_t)b * T * D + (size_t)h * hd;
    const int nkk = hd > 32 ? 2 : 1;
    u32x4 qf[2], kf[2], vf[2], gf[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int c0 = 32 * kk + 8 * g;
        qf[kk] = row_chunk16(qb, ldq, x, c0, T, hd);
        kf[kk] = row_chunk16(qb + D, ldq, x, c0, T, hd);
        vf[kk] = row_chunk16(qb + 2 * D, ldq, x, c0, T, hd);
        gf[kk] = row_chunk16(gb, (size_t)D, x, c0, T, hd);
    }
    uint16_t (*sq)[kAmLd] = sm[wid][0], (*sk)[kAmLd] = sm[wid][1], (*sg)[kAmLd] = sm[wid][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        *(u32x4*)&sq[x][32 * kk + 8 * g] = qf[kk];
        *(u32x4*)&sk[x][32 * kk + 8 * g] = kf[kk];
        *(u32x4*)&sg[x][32 * kk + 8 * g] = gf[kk];
    }
    auto mma32 = [](const u32x4& a, const u32x4& bb, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bb), c, 0, 0, 0);
    };
    f32x4 sT = {0.f, 0.f, 0.f, 0.f}, sN = sT, pT = sT, pN = sT;
    for (int kk = 0; kk < nkk; ++kk) {
        sT = mma32(kf[kk], qf[kk], sT);              // [j][i]: lane (i, g) holds j = 4 g + r
        sN = mma32(qf[kk], kf[kk], sN);              // [i][j]: lane (j, g) holds i = 4 g + r
        pT = mma32(vf[kk], gf[kk], pT);              // dPd, the same two layouts
        pN = mma32(gf[kk], vf[kk], pN);
    }
    // softmax, dropout keep-scales, dS -- layout T: query i = x, keys j = 4 g + r
    float dsT[4], dsN[4], pdN[4];
    {
        float e[4], ks[4], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) { e[r] = (4 * g + r <= x) ? sT[r] * scale : -INFINITY; mx = fmaxf(mx, e[r]); }
        mx = cross_rows_allreduce<true>(mx);
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { e[r] = expf(e[r] - mx); sum += e[r]; }
        sum = cross_rows_allreduce<false>(sum);
        const float inv = 1.0f / sum;
        float dot = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 4 * g + r;
            ks[r] = (p > 0.f && x < T && j <= x) ? drop_scale(seed, site, drop_idx_attn((size_t)pair, T, x, j), p, inv_keep) : 1.f;
            e[r] *= inv;
            dot = fmaf(pT[r] * ks[r], e[r], dot);
        }
        dot = cross_rows_allreduce<false>(dot);
#pragma unroll
        for (int r = 0; r < 4; ++r) dsT[r] = e[r] * (pT[r] * ks[r] - dot) * scale;
    }
    // layout N: key j = x, queries i = 4 g + r (a query's keys are the 16 lanes of this DPP row)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 4 * g + r;
        const bool in = x <= i;
        const float ev = in ? sN[r] * scale : -INFINITY;
        const float mx = row16_allreduce<true>(ev);
        const float ex = expf(ev - mx);
        const float pr = ex * (1.0f / row16_allreduce<false>(ex));
        const float ks = (p > 0.f && i < T && in) ? drop_scale(seed, site, drop_idx_attn((size_t)pair, T, i, x), p, inv_keep) : 1.f;
        const float dot = row16_allreduce<false>(pN[r] * ks * pr);
        dsN[r] = pr * (pN[r] * ks - dot) * scale;
        pdN[r] = pr * ks;
    }
    const uint2 bdsT = pack4_bf16(dsT[0], dsT[1], dsT[2], dsT[3]);
    const uint2 bdsN = pack4_bf16(dsN[0], dsN[1], dsN[2], dsN[3]);
    const uint2 bpdN = pack4_bf16(pdN[0], pdN[1], pdN[2], pdN[3]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                // the wave's LDS copies are written (LDS serves a wave's accesses in order)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
    auto tr = [&](uint16_t (*m)[kAmLd], int dt) {   // lane (x, g): m[4 g + r][16 dt + x], r = 0 .. 3
        return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(&m[4 * g + (x >> 2)][16 * dt + 4 * (x & 3)]));
    };
    auto mma16b = [](const s16x4& a, const uint2& bb, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(s16x4, bb), c, 0, 0, 0);
    };
    uint16_t* ob = dqkv + ((size_t)b * T + x) * ldq + (size_t)h * hd;      // row x of this pair's dq | dk | dv
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // The results leave as 16-BYTE pieces (round 6): a lane holds dims 16 dt + 4 g .. + 3 of its row = 8 bytes; the lane groups g, g + 1
    // of the dim tiles dt, dt + 1 exchange halves (two v_permlane16_swap per tensor), after which an even group holds 8 consecutive
    // dims of tile dt and an odd group 8 of tile dt + 1 -- six requests per lane where there were twelve (a head's rows are 8-byte
    // aligned when hd is not a multiple of 8: global memory takes the unaligned dwordx4).  A piece that straddles the end of the head
    // (hd = 60: dims 56 .. 63) goes out as its first 8 bytes.
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
    auto put16 = [&](uint16_t* dst, int dt, uint2 a, uint2 bq) {            // a: tile dt, bq: tile dt + 1 (this lane's four dims of each)
        const u32x2_t sx = __builtin_amdgcn_permlane16_swap(a.x, bq.x, false, false);
        const u32x2_t sy = __builtin_amdgcn_permlane16_swap(a.y, bq.y, false, false);
        const int f = 16 * (dt + (g & 1)) + 4 * (g & ~1);                  // first of the lane's eight dims
        if (x < T && f + 8 <= hd) *(u32x4_a8*)(dst + f) = u32x4_a8{sx[0], sy[0], sx[1], sy[1]};
        else if (x < T && f < hd) *(uint2*)(dst + f) = make_uint2(sx[0], sy[0]);
    };
#pragma unroll
    for (int dt = 0; dt < 4; dt += 2) {
        if (16 * dt >= hd) break;                    // (wave-uniform)
        uint2 pq[2], pk[2], pv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            pq[u] = pk[u] = pv[u] = make_uint2(0u, 0u);
            if (16 * (dt + u) < hd) {                // (wave-uniform)
                const f32x4 dq = mma16b(tr(sk, dt + u), bdsT, zero);     // [d][i]: lane (i, g) holds d = 16 (dt + u) + 4 g + r
                const f32x4 dk = mma16b(tr(sq, dt + u), bdsN, zero);     // [d][j]
                const f32x4 dv = mma16b(tr(sg, dt + u), bpdN, zero);
                pq[u] = pack4_bf16(dq[0], dq[1], dq[2], dq[3]);
                pk[u] = pack4_bf16(dk[0], dk[1], dk[2], dk[3]);
                pv[u] = pack4_bf16(dv[0], dv[1], dv[2], dv[3]);
            }
        }
        put16(ob, dt, pq[0], pq[1]);
        put16(ob + D, dt, pk[0], pk[1]);
        put16(ob + 2 * D, dt, pv[0], pv[1]);
    }
}
