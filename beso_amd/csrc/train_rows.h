// The row and elementwise kernels of the training step (train.hip).  Included by train.hip INSIDE its
// `namespace beso { namespace { ... } }`: everything here keeps the internal linkage it had as part of that file.
// Provides, in this order: the goal and dropout masks (goal_keep, goal_mask_kernel, dropout_mask_kernel); pack_table_kernel
//   (PackSeg / PackTable); prep_kernel; the embedding (train_embed_kernel, train_feat_kernel, wcat_pack_kernel,
//   scatter_emb_kernel); LayerNorm forward, backward and the reduction of its partials (LnRedCall / LnRedTable); the column sums
//   (colsum_kernel, colsum_part_kernel, part_reduce_kernel); the compact action rows (gather_rows_kernel, scatter_rows2_kernel);
//   the loss kernels; the input VJP (vjp_seed_kernel, vjp_input_kernel, input_grad_kernel).
// Needs: common.h (included by the unit in front of its namespace) and train_gemm.h, for Vec4 alone.  Sees neither train_attn.h
// nor the host.
#pragma once

// (the dropout sites and element counters: common.h, drop_site_* / drop_idx_*)

// mask_cond (score_gpts.py:360-371): cond * (1 - bernoulli(p)), elementwise over [B, G, obs], NO rescaling of the kept
// elements.  keep(b, g, c) = 1 iff the hash-uniform of element ((b*G + g)*obs + c) is >= p.
__device__ __forceinline__ float goal_keep(uint32_t seed, size_t idx, float p) { return drop_scale(seed, kGoalSite, idx, p, 1.0f); }

__global__ void goal_mask_kernel(float* __restrict__ mask, size_t n, float p, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        mask[i] = p > 0.f ? goal_keep(seed, i, p) : 1.f;
}

// The keep-scales of one dropout site as the step applies them (beso_dropout_mask), in the reference's layout: n elements of
// [B, H, T, T] (rows_D = 0: attention, the counter IS the linear index) or of [B T, D] (rows_D = D, D % 4 == 0: a chunk of
// four lies in one token row).  skip_sigma: the embedding site, whose sigma-token rows carry no dropout; compact: the last
// layer's proj / MLP sites, whose counters run over the compact action rows -- the rows that layer does not evaluate get 1.
// Grid-stride over 16-byte chunks; the last chunk of an attention mask may be partial (n % 4 != 0) and is stored by element.
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* __restrict__ scale, size_t n, int rows_D, int T, int t, int G,
                                                           int skip_sigma, int compact, float p, float inv_keep, uint32_t seed,
                                                           uint32_t site) {
    const size_t chunks = (n + 3) / 4;
    for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (size_t)gridDim.x * blockDim.x) {
        const size_t i = 4 * c;
        size_t idx = i;
        bool drawn = p > 0.f;
        if (rows_D > 0) {
            const size_t row = i / (size_t)rows_D;
            const int f = (int)(i - row * (size_t)rows_D), tok = (int)(row % (size_t)T);
            if (skip_sigma && tok == 0) drawn = false;
            if (compact) {
                const long long ar = drop_action_row((long long)(row / (size_t)T), tok, t, G);
                if (ar < 0) drawn = false;
                idx = drop_idx_row((size_t)(ar < 0 ? 0 : ar), rows_D, f);
            } else idx = drop_idx_row(row, rows_D, f);
        }
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = drawn ? drop_scale(seed, site, idx + j, p, inv_keep) : 1.f;
        if (i + 4 <= n) *(f32x4*)(scale + i) = v;
        else for (int j = 0; i + j < n; ++j) scale[i + j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------
// operand-typed copies of one layer's weights (and the fused q|k|v bias) in one launch
// ---------------------------------------------------------------------------------------------
struct PackSeg { const float* src; void* dst; uint32_t first; uint32_t f32; };      // first: index of the segment's first float4 in the launch
constexpr int kPackSegs = 64;                          // 9 per layer: seven layers per launch (24 B each in the kernel argument)
struct PackTable { PackSeg seg[kPackSegs]; int n; };

template <typename E>
__global__ void pack_table_kernel(PackTable t, uint32_t total4) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += gridDim.x * blockDim.x) {
        int lo = 0, hi = t.n - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.seg[mid].first <= i) lo = mid; else hi = mid - 1; }
        const PackSeg& g = t.seg[lo];
        const uint32_t k = i - g.first;
        const f32x4 v = *(const f32x4*)(g.src + 4 * (size_t)k);
        if (g.f32) *(f32x4*)((float*)g.dst + 4 * (size_t)k) = v;
        else Vec4<E>::store((E*)g.dst + 4 * (size_t)k, v);
    }
}

// ---------------------------------------------------------------------------------------------
// prep: noised = a + n*sigma; target = (a - c_skip*noised)/c_out            (score_wrappers.py:64-69)
// ---------------------------------------------------------------------------------------------
// ... and the step's two small initialisations (launches of their own before): the loss accumulator, and the head bias padded
// to the ap columns of the head GEMM.
__global__ void prep_kernel(const float* __restrict__ action, const float* __restrict__ noise,
                            const float* __restrict__ sigma, float* __restrict__ noised, float* __restrict__ target,
                            int per_sample, size_t n, float sigma_data, float* __restrict__ loss, float* __restrict__ b_head,
                            const float* __restrict__ head_bias, int act, int ap) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *loss = 0.f;
        for (int c = threadIdx.x; c < ap; c += blockDim.x) b_head[c] = c < act ? head_bias[c] : 0.f;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float sg = sigma[i / per_sample];
        const float sd2 = sigma_data * sigma_data, den = sg * sg + sd2;
        const float c_skip = sd2 / den, c_out = sg * sigma_data / sqrtf(den);
        const float a = action[i], nz = a + noise[i] * sg;
        noised[i] = nz;
        target[i] = (a - c_skip * nz) / c_out;
    }
}

// ---------------------------------------------------------------------------------------------
// embed (training): x0 row (same arithmetic as embed_kernel of elementwise.hip) + the row of the feature
// matrix Xemb[M][Ke] whose transpose-product with dx0 yields every embedding gradient at once:
//   columns [0,obs) state/goal features | [obs,obs+act) c_in * noised action | obs+act: log(sigma)/4 |
//   +1,+2,+3: one-hot of the token kind (tok_emb.bias, action_emb.bias, sigma_emb.bias) |
//   then seq_size one-hot columns of the position row used (pos_emb).
// ---------------------------------------------------------------------------------------------
template <typename E>
__global__ void train_embed_kernel(const float* __restrict__ state, const float* __restrict__ action,
                                   const float* __restrict__ goal, const float* __restrict__ sigma,
                                   const float* __restrict__ pos, const float* __restrict__ tok_w,
                                   const float* __restrict__ tok_b, const float* __restrict__ sig_w,
                                   const float* __restrict__ sig_b, const float* __restrict__ act_w,
                                   const float* __restrict__ act_b, float* __restrict__ x, E* __restrict__ xemb,
                                   int t, int T, int G, int D, int obs, int act, int Ke, float sigma_data, float p_drop,
                                   float p_goal, uint32_t seed) {
    extern __shared__ float in_vec[];
    const int row = blockIdx.x, b = row / T, j = row % T;
    const float sg = sigma[b];
    int kind, len = 0, posrow = -1;
    const float* src = nullptr;
    float scale = 1.f;
    if (j == 0) {
        kind = 0;
    } else if (j <= G) {
        kind = 1; len = obs; posrow = j - 1; src = goal + ((size_t)b * G + (j - 1)) * obs;
    } else {
        const int idx = j - G - 1, i = idx >> 1;
        posrow = G + i;
        if ((idx & 1) == 0) { kind = 1; len = obs; src = state + ((size_t)b * t + i) * obs; }
        else {
            kind = 2; len = act; src = action + ((size_t)b * t + i) * act;
            scale = 1.0f / sqrtf(sg * sg + sigma_data * sigma_data);                      // c_in
        }
    }
    // training-mode goal masking (mask_cond, score_gpts.py:298-299) happens here: the goal tokens' inputs are zeroed
    // elementwise; the feature matrix xemb (operand of the embedding weight gradients) takes the masked values
    const bool goal_tok = j >= 1 && j <= G && p_goal > 0.f;
    for (int c = threadIdx.x; c < len; c += blockDim.x)
        in_vec[c] = src[c] * scale * (goal_tok ? goal_keep(seed, ((size_t)b * G + (j - 1)) * obs + c, p_goal) : 1.f);
    __syncthreads();
    const float lsg = logf(sg) / 4.0f;
    for (int c = threadIdx.x; c < Ke; c += blockDim.x) {
        float v = 0.f;
        if (c < obs) v = kind == 1 ? in_vec[c] : 0.f;
        else if (c < obs + act) v = kind == 2 ? in_vec[c - obs] : 0.f;
        else if (c == obs + act) v = kind == 0 ? lsg : 0.f;
        else if (c == obs + act + 1) v = kind == 1 ? 1.f : 0.f;
        else if (c == obs + act + 2) v = kind == 2 ? 1.f : 0.f;
        else if (c == obs + act + 3) v = kind == 0 ? 1.f : 0.f;
        else v = (c - (obs + act + 4)) == posrow ? 1.f : 0.f;
        xemb[(size_t)row * Ke + c] = Act<E>::from(v);
    }
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float v;
        if (kind == 0) {
            v = sig_w[d] * lsg + sig_b[d];
        } else {
            const float* w = (kind == 1 ? tok_w : act_w) + (size_t)d * len;
            float acc = 0.f;
            for (int c = 0; c < len; ++c) acc = fmaf(in_vec[c], w[c], acc);
            v = acc + (kind == 1 ? tok_b[d] : act_b[d]) + pos[(size_t)posrow * D + d];
            // self.drop(tok_emb(..) + pos) / self.drop(action_emb(..) + pos): score_gpts.py:321-325 (the sigma token has none)
            if (p_drop > 0.f) v *= drop_scale(seed, kEmbedSite, drop_idx_row((size_t)row, D, d), p_drop, 1.0f / (1.0f - p_drop));
        }
        x[(size_t)row * D + d] = v;
    }
}

// The embedding as ONE GEMM (round 4): x0[M][D] = Xemb[M][Ke] Wcat[D][Ke]^T with the feature matrix below (the operand of the
// embedding weight gradients since round 1) and Wcat = [tok_emb.W | action_emb.W | sigma_emb.W | tok_emb.b | action_emb.b |
// sigma_emb.b | pos_emb^T] -- on the exact-fp32 MFMA (both operands fp32: fp32 products, fp32 accumulation), so the rows
// equal train_embed_kernel's to summation order.  One block per token row with a strided read of every weight took 48 us per
// 1024 kitchen samples; the feature kernel + the GEMM take 6 + 9.  (Embedding dropout keeps the old kernel: its mask is an
// elementwise epilogue this GEMM does not have.)
template <typename E>
__global__ __launch_bounds__(256) void train_feat_kernel(const float* __restrict__ state, const float* __restrict__ action,
                                                         const float* __restrict__ goal, const float* __restrict__ sigma,
                                                         E* __restrict__ xemb, float* __restrict__ xemb32, int M, int t, int T, int G,
                                                         int obs, int act, int Ke, float sigma_data, float p_goal, uint32_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)M * Ke; i += (size_t)gridDim.x * blockDim.x) {
        const int row = (int)(i / Ke), c = (int)(i % Ke), b = row / T, j = row % T;
        int kind, posrow = -1;
        const float* src = nullptr;
        if (j == 0) kind = 0;
        else if (j <= G) { kind = 1; posrow = j - 1; src = goal + ((size_t)b * G + (j - 1)) * obs; }
        else {
            const int idx = j - G - 1, k = idx >> 1;
            posrow = G + k;
            if ((idx & 1) == 0) { kind = 1; src = state + ((size_t)b * t + k) * obs; }
            else { kind = 2; src = action + ((size_t)b * t + k) * act; }
        }
        float v = 0.f;
        if (c < obs) {
            if (kind == 1) {
                v = src[c];
                if (j <= G && p_goal > 0.f) v *= goal_keep(seed, ((size_t)b * G + (j - 1)) * obs + c, p_goal);     // mask_cond
            }
        } else if (c < obs + act) {
            if (kind == 2) { const float sg = sigma[b]; v = src[c - obs] * (1.0f / sqrtf(sg * sg + sigma_data * sigma_data)); }     // c_in
        } else if (c == obs + act) v = kind == 0 ? logf(sigma[b]) / 4.0f : 0.f;
        else if (c == obs + act + 1) v = kind == 1 ? 1.f : 0.f;
        else if (c == obs + act + 2) v = kind == 2 ? 1.f : 0.f;
        else if (c == obs + act + 3) v = kind == 0 ? 1.f : 0.f;
        else v = (c - (obs + act + 4)) == posrow ? 1.f : 0.f;
        xemb[i] = Act<E>::from(v);
        if ((const void*)xemb32 != (const void*)xemb) xemb32[i] = v;
    }
}

__global__ void wcat_pack_kernel(const float* __restrict__ pos, const float* __restrict__ tok_w, const float* __restrict__ tok_b,
                                 const float* __restrict__ sig_w, const float* __restrict__ sig_b, const float* __restrict__ act_w,
                                 const float* __restrict__ act_b, float* __restrict__ wcat, int D, int obs, int act, int seq_size,
                                 int Ke) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D * Ke; i += gridDim.x * blockDim.x) {
        const int d = i / Ke, c = i % Ke;
        float v = 0.f;
        if (c < obs) v = tok_w[(size_t)d * obs + c];
        else if (c < obs + act) v = act_w[(size_t)d * act + (c - obs)];
        else if (c == obs + act) v = sig_w[d];
        else if (c == obs + act + 1) v = tok_b[d];
        else if (c == obs + act + 2) v = act_b[d];
        else if (c == obs + act + 3) v = sig_b[d];
        else if (c - (obs + act + 4) < seq_size) v = pos[(size_t)(c - (obs + act + 4)) * D + d];
        wcat[i] = v;
    }
}

// dWcat[Ke][D] -> the individual embedding gradients (accumulated: the flat buffer was zeroed)
__global__ void scatter_emb_kernel(const float* __restrict__ dw, float* __restrict__ g_pos, float* __restrict__ g_tokw,
                                   float* __restrict__ g_tokb, float* __restrict__ g_sigw, float* __restrict__ g_sigb,
                                   float* __restrict__ g_actw, float* __restrict__ g_actb, int D, int obs, int act,
                                   int seq_size) {
    const int n = (obs + act + 4 + seq_size) * D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int c = i / D, d = i % D;
        const float v = dw[i];
        if (c < obs) g_tokw[(size_t)d * obs + c] += v;
        else if (c < obs + act) g_actw[(size_t)d * act + (c - obs)] += v;
        else if (c == obs + act) g_sigw[d] += v;
        else if (c == obs + act + 1) g_tokb[d] += v;
        else if (c == obs + act + 2) g_actb[d] += v;
        else if (c == obs + act + 3) g_sigb[d] += v;
        else g_pos[(size_t)(c - (obs + act + 4)) * D + d] += v;
    }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm forward with saved statistics; one wave per row, the row in registers as float4 per lane
// (D % 4 == 0, D <= 1024).
// ---------------------------------------------------------------------------------------------
// NV = float4 slots per lane = ceil(D / 256): 1, 2 or 4

template <typename E, int kLnVec>
__global__ void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                              E* __restrict__ out, float* __restrict__ stats, int rows, int D) {
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    f32x4 v[kLnVec];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        const int c = (lane + i * 64) * 4;
        v[i] = c < D ? *(const f32x4*)(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        const int c = (lane + i * 64) * 4;
        if (c < D) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; sq = fmaf(d, d, sq); }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + 1e-5f);
    if (lane == 0) { stats[2 * (size_t)row] = mean; stats[2 * (size_t)row + 1] = rstd; }
    E* o = out + (size_t)row * D;
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        const int c = (lane + i * 64) * 4;
        if (c < D) {
            const f32x4 wv = *(const f32x4*)(w + c), bv = *(const f32x4*)(b + c);
            Vec4<E>::store(o + c, (v[i] - mean) * rstd * wv + bv);
        }
    }
}

// LayerNorm backward + residual gradient:  dres <- dres + dLN(dxn)  (dres_in == nullptr: no incoming residual
// gradient), operand-typed copy dxb = dres * keep-scale(site) for the linear layer that consumes it, that layer's
// bias gradient (column sums of dxb; dbias may be nullptr) and the affine gradients -- register partials per
// wave -> LDS -> one atomic per block and feature.
template <typename E, int kLnVec>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dxn, const float* __restrict__ x,
                                                     const float* __restrict__ stats, const float* __restrict__ gamma,
                                                     const float* dres_in, float* dres_out, E* __restrict__ dxb,
                                                     float* __restrict__ part, int rows, int D, int rows_per_wave, float p,
                                                     float inv_keep, uint32_t seed, uint32_t site, int skip_mod) {
    __shared__ f32x4 red[3][4][64 * kLnVec];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + wid;
    f32x4 gw[kLnVec], ag[kLnVec], ab[kLnVec], ac[kLnVec];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        const int c = (lane + i * 64) * 4;
        gw[i] = c < D ? *(const f32x4*)(gamma + c) : zero;
        ag[i] = zero; ab[i] = zero; ac[i] = zero;
    }
    const int r_begin = wave * rows_per_wave, r_end = min(rows, r_begin + rows_per_wave);
    // TWO rows per iteration: the kernel is bound by the latency chain load -> two wave reductions -> store of a row, not by
    // bytes (bf16 instead of fp32 for dxn changed nothing); with two rows in flight the four reductions interleave
    constexpr int U = kLnVec == 4 ? 1 : 2;         // (D > 512: the second row would not fit the registers of three waves per SIMD)
    for (int row0 = r_begin; row0 < r_end; row0 += U) {
        f32x4 xh[U][kLnVec], dy[U][kLnVec], go[U][kLnVec], xv[U][kLnVec];
        float mean[U], rstd[U], s1[U], s2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = min(row0 + u, r_end - 1);        // (a surplus second row re-reads the first; nothing of it is stored)
            mean[u] = stats[2 * (size_t)row]; rstd[u] = stats[2 * (size_t)row + 1];
#pragma unroll
            for (int i = 0; i < kLnVec; ++i) {
                const int c = (lane + i * 64) * 4;
                go[u][i] = c < D ? *(const f32x4*)(dxn + (size_t)row * D + c) : zero;
                xv[u][i] = c < D ? *(const f32x4*)(x + (size_t)row * D + c) : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = row0 + u < r_end;
            s1[u] = 0.f; s2[u] = 0.f;
#pragma unroll
            for (int i = 0; i < kLnVec; ++i) {
                const int c = (lane + i * 64) * 4;
                xh[u][i] = c < D ? (xv[u][i] - mean[u]) * rstd[u] : zero;
                dy[u][i] = go[u][i] * gw[i];
                const f32x4 t = dy[u][i] * xh[u][i];
                s1[u] += (dy[u][i][0] + dy[u][i][1]) + (dy[u][i][2] + dy[u][i][3]);
                s2[u] += (t[0] + t[1]) + (t[2] + t[3]);
                if (live) { ag[i] += go[u][i] * xh[u][i]; ab[i] += go[u][i]; }
            }
        }
        float c1[U], c2[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { c1[u] = s1[u]; c2[u] = s2[u]; }
#pragma unroll
        for (int u = 0; u < U; ++u) { c1[u] = wave_sum_dpp(c1[u]); c2[u] = wave_sum_dpp(c2[u]); }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = row0 + u;
            if (row >= r_end) break;
            const float m1 = c1[u] / (float)D, m2 = c2[u] / (float)D;
#pragma unroll
            for (int i = 0; i < kLnVec; ++i) {
                const int c = (lane + i * 64) * 4;
                if (c < D) {
                    const size_t idx = (size_t)row * D + c;
                    f32x4 tot = (dy[u][i] - m1 - xh[u][i] * m2) * rstd[u];
                    if (dres_in) tot += *(const f32x4*)(dres_in + idx);
                    *(f32x4*)(dres_out + idx) = tot;
                    f32x4 op = tot;
                    if (p > 0.f && !(skip_mod > 0 && row % skip_mod == 0)) {      // (the sigma token's embedding has no dropout)
#pragma unroll
                        for (int j = 0; j < 4; ++j) op[j] *= drop_scale(seed, site, idx + j, p, inv_keep);
                    }
                    Vec4<E>::store(dxb + idx, op);
                    ac[i] += op;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        red[0][wid][lane + i * 64] = ag[i]; red[1][wid][lane + i * 64] = ab[i]; red[2][wid][lane + i * 64] = ac[i];
    }
    __syncthreads();
    // block partials [3][D] -> part[blockIdx.x]; ln_reduce_kernel sums them for all LayerNorms of the step at once
    // (fp32 atomics from every block were the larger half of this kernel's time)
    const float* r0 = (const float*)red[0], *r1 = (const float*)red[1], *r2 = (const float*)red[2];
    constexpr int WS = 64 * kLnVec * 4;          // floats per wave slab
    float* o = part + (size_t)blockIdx.x * 3 * D;
    for (int c = threadIdx.x; c < D; c += 256) {
        o[c] = r0[c] + r0[WS + c] + r0[2 * WS + c] + r0[3 * WS + c];
        o[D + c] = r1[c] + r1[WS + c] + r1[2 * WS + c] + r1[3 * WS + c];
        o[2 * D + c] = r2[c] + r2[WS + c] + r2[2 * WS + c] + r2[3 * WS + c];
    }
}

// sums the block partials of every LayerNorm backward of the step: call z -> gamma / beta gradient and the bias
// gradient of the linear layer that consumed its output (assigned: each destination has exactly one source)
struct LnRedCall { float* dgamma; float* dbeta; float* dbias; };
struct LnRedTable { LnRedCall c[2 * kMaxLayers + 1]; int nb[2 * kMaxLayers + 1]; };    // nb: block partials call z wrote (<= nblk, the slab stride)
__global__ __launch_bounds__(256) void ln_reduce_kernel(const float* __restrict__ part, LnRedTable t, int nblk, int D,
                                                        int call0) {
    // thread (cx, ry): four consecutive columns (one 16-byte load: 16 lanes = 256 contiguous bytes of a slab row), block partials
    // ry, ry + 16, ... with EIGHT loads in flight.  Round 5's form -- one column per thread, four row groups, four loads in
    // flight -- was nblk / 16 dependent HBM round trips per thread: 375 us at 8192 samples (1878 partials per LayerNorm, 105 MB
    // of slabs) where the bytes cost ~25 us.  The sum order is fixed (row groups in order, then the 16 groups in order):
    // deterministic.  D is a multiple of 4 (the training step requires a multiple of 8).
    __shared__ f32x4 red[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4, which = blockIdx.y, call = blockIdx.z + call0;
    const int c = blockIdx.x * 64 + 4 * cx;
    const float* src = part + ((size_t)call * nblk * 3 + which) * D + c;
    nblk = t.nb[call];
    const size_t rs = (size_t)3 * D;
    f32x4 a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < D) {
        int b = ry;
        for (; b + 112 < nblk; b += 128) {
            // (the eight loads first, into registers of their own: written as a[u] += load the compiler issued them one at a
            //  time -- load, s_waitcnt vmcnt(0), add -- i.e. nblk / 16 dependent round trips again: 326 us at 8192 samples)
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load((const f32x4*)(src + (size_t)(b + 16 * u) * rs));
            __builtin_amdgcn_sched_barrier(0);          // (nor may the scheduler fold the adds back between the loads)
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += v[u];
        }
        for (; b < nblk; b += 16) a[0] += *(const f32x4*)(src + (size_t)b * rs);
    }
    red[ry][cx] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (ry == 0 && c < D) {
        const LnRedCall k = t.c[call];
        float* dst = which == 0 ? k.dgamma : (which == 1 ? k.dbeta : k.dbias);
        if (dst) {
            f32x4 v = red[0][cx];
#pragma unroll
            for (int r = 1; r < 16; ++r) v += red[r][cx];
            *(f32x4*)(dst + c) = v;
        }
    }
}

// column sums (bias gradients): out_j[n - j*seg] += sum_m a[m][n] for n in segment j (q | k | v share one pass).
// Thread (cx, ry): 16-byte chunk cx of the row, rows ry, ry+4, ...; a wave reads 1 KB of a row at a time.
template <typename E>
__global__ __launch_bounds__(256) void colsum_kernel(const E* __restrict__ a, int ld, int rows, int cols, float* out0,
                                                     float* out1, float* out2, int seg, int rows_per_block) {
    constexpr int EPC = 16 / (int)sizeof(E);
    __shared__ float red[4][64][EPC];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + cx) * EPC;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    float acc[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) acc[j] = 0.f;
    if (c < cols) {
        for (int r = r0 + ry; r < r1; r += 4) {
            const u32x4 u = *(const u32x4*)(a + (size_t)r * ld + c);
            if (sizeof(E) == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[2 * j] += __uint_as_float(u[j] << 16);
                    acc[2 * j + 1] += __uint_as_float(u[j] & 0xffff0000u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += __uint_as_float(u[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EPC; ++j) red[ry][cx][j] = acc[j];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * EPC; i += 256) {
        const int n = blockIdx.x * 64 * EPC + i;
        if (n < cols) {
            const int x = i / EPC, j = i % EPC;
            const float v = red[0][x][j] + red[1][x][j] + red[2][x][j] + red[3][x][j];
            const int sj = n / seg;
            float* o = sj == 0 ? out0 : (sj == 1 ? out1 : out2);
            unsafeAtomicAdd(o + (n - sj * seg), v);
        }
    }
}
// BESO_TRAIN_DETERMINISTIC: the same sums of the same row block in the same order (a kernel of its own, so that colsum_kernel's
// instructions stay what they were), stored into row blockIdx.y of the slab part[gridDim.y][cols] instead of added to the output
template <typename E>
__global__ __launch_bounds__(256) void colsum_part_kernel(const E* __restrict__ a, int ld, int rows, int cols,
                                                          float* __restrict__ part, int rows_per_block) {
    constexpr int EPC = 16 / (int)sizeof(E);
    __shared__ float red[4][64][EPC];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + cx) * EPC;
    const int r0 = blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    float acc[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) acc[j] = 0.f;
    if (c < cols) {
        for (int r = r0 + ry; r < r1; r += 4) {
            const u32x4 u = *(const u32x4*)(a + (size_t)r * ld + c);
            if (sizeof(E) == 2) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[2 * j] += __uint_as_float(u[j] << 16);
                    acc[2 * j + 1] += __uint_as_float(u[j] & 0xffff0000u);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += __uint_as_float(u[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EPC; ++j) red[ry][cx][j] = acc[j];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * EPC; i += 256) {
        const int n = blockIdx.x * 64 * EPC + i;
        if (n < cols) {
            const int x = i / EPC, j = i % EPC;
            part[(size_t)blockIdx.y * cols + n] = red[0][x][j] + red[1][x][j] + red[2][x][j] + red[3][x][j];
        }
    }
}

// out[c] = part[0][c] + part[1][c] + ... + part[nparts - 1][c] over a slab of `nparts` rows of `cols` floats: the second stage of
// the deterministic column sums (colsum_part_kernel, the kColPart epilogues).  Thread (cx, ry): column cx of the block's 64, slab
// rows ry, ry + 4, ... with eight loads in flight; then the four row groups in order.  The order of the additions depends on
// (nparts, cols) only.  `out` is assigned, not accumulated.
__global__ __launch_bounds__(256) void part_reduce_kernel(const float* __restrict__ part, int nparts, int cols, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6, c = blockIdx.x * 64 + cx;
    float a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = 0.f;
    if (c < cols) {
        int b = ry;
        for (; b + 28 < nparts; b += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(b + 4 * u) * cols + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += v[u];
        }
        for (; b < nparts; b += 4) a[0] += part[(size_t)b * cols + c];
    }
    red[ry][cx] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    if (ry == 0 && c < cols) out[c] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

// ---------------------------------------------------------------------------------------------
// The last layer's out-projection, MLP, ln_f and head only matter on the action-token rows (nothing else reaches the
// loss: score_gpts.py:341-353), so they run on a COMPACT copy of those rows: compact row c = b*t + i <-> token row
// b*T + G + 2 + 2i.  gather: full -> compact; scatter: compact -> full with zeros on every other row (the gradient
// that enters the attention of the last layer).  Four elements per thread (D % 8 == 0).
// ---------------------------------------------------------------------------------------------
template <typename V>     // V: float or the operand type
__global__ void gather_rows_kernel(const V* __restrict__ src, V* __restrict__ dst, int n_compact, int t, int T, int G, int D) {
    const int d4 = D / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_compact * d4; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i / d4), k = (int)(i % d4), b = c / t, j = c % t;
        const size_t m = (size_t)b * T + G + 2 + 2 * j;
        Vec4<V>::store(dst + (size_t)c * D + 4 * k, Vec4<V>::load(src + m * D + 4 * k));
    }
}

// both scatters of the last layer's backward in one launch (round 6: two dependent launches of ~7 us on the step's chain)
template <typename E>
__global__ void scatter_rows2_kernel(const E* __restrict__ src_e, E* __restrict__ dst_e, const float* __restrict__ src_f,
                                     float* __restrict__ dst_f, int M, int t, int T, int G, int D) {
    const int d4 = D / 4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)M * d4; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / d4), k = (int)(i % d4), b = m / T, idx = m % T - 1 - G;
        f32x4 ve = {0.f, 0.f, 0.f, 0.f}, vf = ve;
        if (idx >= 0 && (idx & 1)) {
            const size_t so = ((size_t)b * t + (idx >> 1)) * D + 4 * k;
            ve = Vec4<E>::load(src_e + so);
            vf = Vec4<float>::load(src_f + so);
        }
        Vec4<E>::store(dst_e + (size_t)m * D + 4 * k, ve);
        Vec4<float>::store(dst_f + (size_t)m * D + 4 * k, vf);
    }
}

// ---------------------------------------------------------------------------------------------
// squared-error loss over the (compact) action-token rows (score_wrappers.py:70-79 with pred_last_action_only
// False: per-sample mean over (t, act), then the batch mean = the mean over all B*t*act elements), its gradient
// with respect to the prediction, operand typed, zero on the padding columns.
// ---------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                   E* __restrict__ dpred, float* __restrict__ loss, int M, int act, int ap,
                                                   float inv_count, float grad_scale, int t, int last_only) {
    __shared__ float part[4];
    float acc = 0.f;
    const size_t n = (size_t)M * ap;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t m = i / ap;                     // compact action row b*t + i: the layout of `target`
        const int a = (int)(i % ap);
        float g = 0.f;
        // pred_last_action_only: only the last step of every window is scored (score_wrappers.py:76-77)
        if (a < act && (!last_only || (int)(m % t) == t - 1)) {
            const float diff = pred[i] - target[m * act + a];
            acc = fmaf(diff, diff, acc);
            g = 2.0f * diff * inv_count * grad_scale;
        }
        dpred[i] = Act<E>::from(g);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(loss, (part[0] + part[1] + part[2] + part[3]) * inv_count);
}
// BESO_TRAIN_DETERMINISTIC: loss_kernel (the same elements per block, the same dpred; a kernel of its own, so that loss_kernel's
// instructions stay what they were) with the block's share of the loss stored into shares[blockIdx.x]; loss_reduce_kernel adds
// the shares up in index order
template <typename E>
__global__ __launch_bounds__(256) void loss_part_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        E* __restrict__ dpred, float* __restrict__ shares, int M, int act, int ap,
                                                        float inv_count, float grad_scale, int t, int last_only) {
    __shared__ float part[4];
    float acc = 0.f;
    const size_t n = (size_t)M * ap;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t m = i / ap;
        const int a = (int)(i % ap);
        float g = 0.f;
        if (a < act && (!last_only || (int)(m % t) == t - 1)) {
            const float diff = pred[i] - target[m * act + a];
            acc = fmaf(diff, diff, acc);
            g = 2.0f * diff * inv_count * grad_scale;
        }
        dpred[i] = Act<E>::from(g);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) shares[blockIdx.x] = (part[0] + part[1] + part[2] + part[3]) * inv_count;
}
// loss = part[0] + ... + part[n - 1] in a fixed order: thread i adds part[i], part[i + 256], ..., then the lanes of a wave
// (wave_sum's butterfly), then the four waves in order.  One block.
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ part, int n, float* __restrict__ loss) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) *loss = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------
// input VJP (beso_denoise_vjp): the seed in place of loss_kernel -- denoised = c_skip x + c_out F (compact action rows), and
// the cotangent of F, dpred = c_out u, operand typed, zero on the padding columns act..ap
// ---------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(256) void vjp_seed_kernel(const float* __restrict__ pred, const float* __restrict__ x,
                                                       const float* __restrict__ sigma, const float* __restrict__ cot,
                                                       E* __restrict__ dpred, float* __restrict__ denoised, int M, int act,
                                                       int ap, int t, float sigma_data) {
    const size_t n = (size_t)M * ap;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const size_t m = i / ap;
        const int a = (int)(i % ap);
        float g = 0.f;
        if (a < act) {
            const float sg = sigma[m / t];
            const float sd2 = sigma_data * sigma_data, den = sg * sg + sd2;
            const float c_skip = sd2 / den, c_out = sg * sigma_data / sqrtf(den);
            const size_t j = m * act + a;
            denoised[j] = c_skip * x[j] + c_out * pred[i];
            g = c_out * cot[j];
        }
        dpred[i] = Act<E>::from(g);
    }
}

// ... and the projection of dx0 (fp32, all token rows) back onto the action input: x_grad = c_skip u + c_in dx0[row] W_act,
// row = the action token of step i (train_embed_kernel's layout), W_act = action_emb.weight [D][act].  One workgroup per sample;
// dot[b] = sum over (t, act) of u x_grad as a fixed-order reduction (deterministic, no atomics).
__global__ __launch_bounds__(256) void vjp_input_kernel(const float* __restrict__ dx0, const float* __restrict__ w_act,
                                                        const float* __restrict__ sigma, const float* __restrict__ cot,
                                                        float* __restrict__ x_grad, float* __restrict__ dot, int t, int T,
                                                        int G, int D, int act, float sigma_data) {
    __shared__ float part[4];
    const int b = blockIdx.x;
    const float sg = sigma[b], den = sg * sg + sigma_data * sigma_data;
    const float c_skip = sigma_data * sigma_data / den, c_in = 1.0f / sqrtf(den);
    float acc = 0.f;
    for (int e = threadIdx.x; e < t * act; e += 256) {
        const int i = e / act, a = e % act;
        const float* r = dx0 + ((size_t)b * T + G + 2 + 2 * i) * D;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(r[d], w_act[(size_t)d * act + a], s);
        const size_t j = (size_t)b * t * act + e;
        const float u = cot[j], g = c_skip * u + c_in * s;
        x_grad[j] = g;
        acc = fmaf(u, g, acc);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && dot) dot[b] = (part[0] + part[1]) + (part[2] + part[3]);
}

// ... and onto the state and goal inputs (beso_loss_grad_inputs, beso_denoise_vjp_inputs): the rows of dx0 that belong to state
// and goal tokens (train_embed_kernel's layout: goal j at row 1 + j, state i at row G + 1 + 2 i) times W_tok = tok_emb.weight
// [D][obs], in fp32:
//   state_grad[b][i][c] = sum_d m(row, d) dx0[row][d] W_tok[d][c]
//   goal_grad[b][j][c]  = keep(b, j, c) sum_d m(row, d) dx0[row][d] W_tok[d][c]
// dx0 is the fp32 residual gradient layer 0's LayerNorm-1 backward leaves, i.e. the gradient of the embedding BEHIND its
// dropout: m is that dropout's keep-scale (embed_p = 0: 1), recomputed here as train_embed_kernel drew it; keep is mask_cond's
// keep-mask of the goal element (goal_p = 0: 1), so an element the mask zeroed on the way in gets exactly 0.
// A small GEMM ([rows][D] x [D][obs], obs <= 30 at the shipped shapes) on the VALU.  A workgroup stages a tile of kIgRows rows
// row-major in LDS (wave w its rows 8 w .. 8 w + 7: a lane loads 16 bytes of each, eight independent loads in flight, and
// stores them to consecutive banks) beside the columns [c0, c0 + kIgCols) of W_tok; thread (g, c) owns the four outputs of rows
// 4 g .. 4 g + 3 at column c and sums over d in index order, four features per step: one 16-byte read per row (the 32 lanes of
// a row group read one address) and four reads of the weight per sixteen multiply-adds.  No atomics, the same bits on every
// call.  D is walked in chunks of dc_max features (the LDS budget; D % 8 == 0 keeps every chunk a multiple of four); where one
// chunk covers D the weights are staged once per workgroup.  Either output may be nullptr (its rows are then left out of the
// tiles).
constexpr int kIgRows = 32, kIgCols = 32, kIgPad = 4, kIgChunk = 240;    // (32 (240 + 4) + 240 32) floats = 61,952 bytes of LDS
__global__ __launch_bounds__(256) void input_grad_kernel(const float* __restrict__ dx0, const float* __restrict__ tok_w,
                                                         float* __restrict__ state_grad, float* __restrict__ goal_grad,
                                                         int batch, int t, int T, int G, int D, int obs, int dc_max,
                                                         float embed_p, float goal_p, uint32_t seed) {
    extern __shared__ __attribute__((aligned(16))) float ig_lds[];
    const int ldx = dc_max + kIgPad;                      // row stride of the tile, a multiple of four floats
    float* xl = ig_lds;                                   // [kIgRows][ldx]
    float* wl = ig_lds + (size_t)kIgRows * ldx;           // [dc][kIgCols]
    const int n_g = goal_grad ? G : 0, n_s = state_grad ? t : 0, per = n_g + n_s;
    const int rows = batch * per;
    const int c0 = blockIdx.y * kIgCols, cw = min(kIgCols, obs - c0);
    const int g = threadIdx.x >> 5, cl = threadIdx.x & 31;
    const float inv_keep = embed_p > 0.f ? 1.0f / (1.0f - embed_p) : 1.f;
    // token row of tile row vr (sample b, k-th differentiated token of it: the goals first)
    auto token_row = [&](int b, int k) { return (size_t)b * T + (k < n_g ? 1 + k : G + 1 + 2 * (k - n_g)); };
    bool w_staged = false;
    for (int r0 = blockIdx.x * kIgRows; r0 < rows; r0 += gridDim.x * kIgRows) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int d0 = 0; d0 < D; d0 += dc_max) {
            const int dc = min(dc_max, D - d0);
            __syncthreads();                              // (the previous chunk has been read)
            if (!w_staged) {
                for (int i = threadIdx.x; i < dc * kIgCols; i += 256) {
                    const int dd = i >> 5, c = i & 31;
                    wl[i] = c < cw ? tok_w[(size_t)(d0 + dd) * obs + c0 + c] : 0.f;
                }
                w_staged = dc_max >= D;
            }
            {
                constexpr int kRw = kIgRows / 4;          // rows per wave
                const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
                size_t trow[kRw];
#pragma unroll
                for (int j = 0; j < kRw; ++j) {
                    const int vr = min(r0 + kRw * w + j, rows - 1);       // (a row past the end re-reads the last one; stored as zeros)
                    const int b = vr / per;
                    trow[j] = token_row(b, vr - b * per);
                }
                for (int dd = 4 * lane; dd < dc; dd += 256) {
                    f32x4 v[kRw];
#pragma unroll
                    for (int j = 0; j < kRw; ++j) v[j] = *(const f32x4*)(dx0 + trow[j] * D + d0 + dd);
#pragma unroll
                    for (int j = 0; j < kRw; ++j) {
                        if (embed_p > 0.f) {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                v[j][e] *= drop_scale(seed, kEmbedSite, drop_idx_row(trow[j], D, d0 + dd + e), embed_p, inv_keep);
                        }
                        if (r0 + kRw * w + j >= rows) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                        *(f32x4*)(xl + (size_t)(kRw * w + j) * ldx + dd) = v[j];
                    }
                }
            }
            __syncthreads();
            if (cl < cw) {
                const float* xr = xl + (size_t)(4 * g) * ldx;
                for (int dd = 0; dd < dc; dd += 4) {
                    f32x4 xv[4];
                    float wv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) xv[j] = *(const f32x4*)(xr + (size_t)j * ldx + dd);
#pragma unroll
                    for (int e = 0; e < 4; ++e) wv[e] = wl[(dd + e) * kIgCols + cl];
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv[j][e], wv[e], acc[j]);
                }
            }
        }
        if (cl < cw) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int vr = r0 + 4 * g + j;
                if (vr >= rows) break;
                const int b = vr / per, k = vr - b * per, c = c0 + cl;
                if (k < n_g) {
                    const size_t idx = ((size_t)b * G + k) * obs + c;
                    const bool kept = !(goal_p > 0.f) || goal_keep(seed, idx, goal_p) != 0.f;
                    goal_grad[idx] = kept ? acc[j] : 0.f;
                } else state_grad[((size_t)b * t + (k - n_g)) * obs + c] = acc[j];
            }
        }
    }
}
