// The tile GEMM family of the training step (train.hip), device code and its launchers.  Included by train.hip INSIDE its
// `namespace beso { namespace { ... } }`: everything here keeps the internal linkage it had as part of that file.
// Provides: the operand-typed GELU (gelu_t / gelu_grad_t); the operand loaders (GOp, make_gop, op_gload, op_lstore,
//   op_lstore_masked, op_frag), mma16, tgemm_tile, tgemm_kernel and its launcher tgemm; Vec4 and the epilogues EpiStore, EpiFc1,
//   EpiResid, EpiGeluBwd, EpiSilu, EpiSiluBwd with their deterministic forms, EpiAtomic (dev build), EpiStoreF; the grouped
//   weight gradients: GProb / GTable, tgemm_wgrad_group_kernel, wgrad_reduce_kernel, the panel-owning wgrad_panel_group_kernel
//   with wgrad_panel_lds / wgrad_panel_w / wgrad_panel_tiles.
// Needs: common.h only (included by the unit in front of its namespace).  Sees neither train_attn.h nor train_rows.h nor the host.
// Vec4 lives here although the row kernels use it too: the epilogues are its first users, and train_rows.h may look down on
// this header, not the other way round.
#pragma once

// GELU and its derivative (nn.GELU(), score_gpts.py:107): exact erf / exp in the fp32 mode, the fitted polynomial of
// the inference kernels (max |error| 1.9e-4, below the bf16 rounding of the stored value) in the bf16 mode
template <typename E> __device__ __forceinline__ float gelu_t(float v);
template <> __device__ __forceinline__ float gelu_t<float>(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
template <> __device__ __forceinline__ float gelu_t<uint16_t>(float v) { return gelu_poly(v); }
template <typename E> __device__ __forceinline__ float gelu_grad_t(float v);
template <> __device__ __forceinline__ float gelu_grad_t<float>(float v) {
    return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}
template <> __device__ __forceinline__ float gelu_grad_t<uint16_t>(float v) { return gelu_grad_poly(v); }

// ---------------------------------------------------------------------------------------------
// tgemm:  C[m][n] = sum_k Aop(m,k) * Bop(n,k)
//   AKS = false: A is [M][lda], k contiguous ("k-contig")      AKS = true: A is [K][lda], m contiguous ("k-slow")
//   BKS likewise for B ([N][ldb] / [K][ldb]).
// 128x128 block tile, 8 waves as 2x4 of 64x32, 16x16 MFMA tiles; one stage = 128 bytes of k per row
// (64 bf16 / 32 fp32); register-staged, two stages in flight; all loads predicated (zero fill), so M, N, K are
// arbitrary up to: K % (16/sizeof(E)) == 0 for a k-contig operand, rows % (16/sizeof(E)) == 0 for a k-slow one.
// blockIdx.y splits K (k_per_split, a multiple of the stage); the epilogue functor decides what a partial
// sum means (EpiAtomic accumulates).
// ---------------------------------------------------------------------------------------------
constexpr int kOpBytes = 16896;        // LDS bytes of one operand stage (k-slow images carry padding)
constexpr int kSubBytes = 2080;        // bf16 k-slow image: one 16-column subtile = 64 k-rows x 32 B + 32 B pad
constexpr int kRowBytes32 = 528;       // fp32 k-slow image: one k-row = 128 columns x 4 B + 16 B pad

// Global side of an operand: raw buffer loads with 32-bit per-lane byte offsets (computed once per tile) and the
// k advance in the scalar offset.  Nothing relies on the descriptor's range check: rows / columns outside the
// operand are read at offset 0 (their products land in outputs that are never stored), lanes past k_end are read
// at a valid address and replaced by zeros.
constexpr int kNW = 8;                     // waves of a tgemm workgroup: 2 x 4, 64 x 32 each
constexpr int kGT = 64 * kNW;              // threads of a tgemm workgroup
constexpr int kGL = 1024 / kGT;            // 16-byte chunks per thread, operand and stage
constexpr int kWN = 4;                     // waves along n
constexpr int kOcc = 4;                    // waves per SIMD asked of the compiler (two workgroups per CU)
template <int NCH> struct GOp { uint32_t voff[NCH]; };          // (the descriptor is rebuilt from the kernel argument at every use: a
                                           //  descriptor carried in VGPRs makes every load a waterfall loop)

template <typename E, bool KS, int NCH>
__device__ __forceinline__ GOp<NCH> make_gop(const E* __restrict__ P, int ld, int r0, int R, int tid) {
    constexpr int EPC = 16 / (int)sizeof(E);
    GOp<NCH> g;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = tid + kGT * i;
        if (!KS) {
            const int row = c >> 3, kc = c & 7, gr = r0 + row;
            g.voff[i] = gr < R ? (uint32_t)(((size_t)gr * ld + kc * EPC) * sizeof(E)) : 0u;
        } else {
            constexpr int CPR = 128 / EPC;               // 16-byte chunks per k-row
            const int krow = c / CPR, cc = c % CPR, gc = r0 + cc * EPC;
            g.voff[i] = gc < R ? (uint32_t)(((size_t)krow * ld + gc) * sizeof(E)) : 0u;
        }
    }
    return g;
}

template <typename E, bool KS, int NCH, bool RAW = false>      // RAW: lanes past k_end are zeroed by op_lstore_masked
__device__ __forceinline__ void op_gload(const E* __restrict__ P, const GOp<NCH>& g, int ld, int k0, int k_end, int tid,
                                         u32x4 (&r)[NCH]) {
    constexpr int EPC = 16 / (int)sizeof(E);
    // P and the k offset are wave-uniform; saying so keeps the descriptor and the scalar offset in SGPRs
    const uint64_t pv = (uint64_t)P;
    const uint64_t pu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(pv >> 32)) << 32) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)pv);      // (the builtin returns int)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)pu, 0, 0x7fffffff, 0x00020000);
    const bool stage_ok = k0 < k_end;                        // a whole stage past the end reads stage 0 (discarded)
    const u32x4 zero = {0u, 0u, 0u, 0u};
    if (!KS) {
        const uint32_t soff = (uint32_t)__builtin_amdgcn_readfirstlane(stage_ok ? (uint32_t)k0 * (uint32_t)sizeof(E) : 0u);
        const bool ok = k0 + (tid & 7) * EPC < k_end;        // the chunk index along k is the same for all loads of a thread
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? g.voff[i] : 0u, soff, 0);
            r[i] = (RAW || ok) ? v : zero;
        }
    } else {
        constexpr int CPR = 128 / EPC;
        const uint32_t soff = (uint32_t)__builtin_amdgcn_readfirstlane(stage_ok ? (uint32_t)k0 * (uint32_t)ld * (uint32_t)sizeof(E) : 0u);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const bool ok = k0 + (tid + kGT * i) / CPR < k_end;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? g.voff[i] : 0u, soff, 0);
            r[i] = (RAW || ok) ? v : zero;
        }
    }
}

// `ones`: bit i set = chunk i of this thread is replaced by (1, 0, 0, ...) -- the ONES COLUMN of the weight-gradient tiles: with
// a column of ones behind the last real column of the activation operand, the product dY^T [X | 1] carries the bias gradient
// (the column sums of dY) in that column for free (tgemm_wgrad_group_kernel)
template <typename E, bool KS, int NCH>
__device__ __forceinline__ void op_lstore(unsigned char* base, int tid, const u32x4 (&r)[NCH], uint32_t ones = 0u) {
    const u32x4 one = {sizeof(E) == 2 ? 0x3F80u : 0x3F800000u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = tid + kGT * i;
        int off;
        if (!KS) {
            const int row = c >> 3, kc = c & 7;
            off = row * 128 + ((kc ^ (row & 7)) << 4);
        } else if (sizeof(E) == 2) {
            const int krow = c >> 4, cc = c & 15;        // 8 columns per chunk: subtile cc/2, half cc%2
            // k-row r = 8g + 4h + j of a 32-row group is kept at row 16h + 4g + j: the four 16-lane groups of one
            // transpose read (fixed h) then fetch 512 contiguous bytes (no bank conflict; with the rows in natural
            // order groups 0/1 and 2/3 were 256 B apart = the same banks: half of all LDS cycles were conflicts)
            const int prow = (krow & ~31) | ((krow & 4) << 2) | ((krow & 24) >> 1) | (krow & 3);
            off = (cc >> 1) * kSubBytes + prow * 32 + (cc & 1) * 16;
        } else {
            const int krow = c >> 5, cc = c & 31;
            off = krow * kRowBytes32 + cc * 16;
        }
        *(u32x4*)(base + off) = (ones >> i) & 1u ? one : r[i];
    }
}

// op_lstore of a RAW-loaded stage that began at k0: the zeroing of the lanes past k_end happens here, when the data
// is consumed, so that nothing touches the registers of a load in flight
template <typename E, bool KS, int NCH>
__device__ __forceinline__ void op_lstore_masked(unsigned char* base, int tid, const u32x4 (&r)[NCH], int k0, int k_end,
                                                 uint32_t ones = 0u) {
    constexpr int EPC = 16 / (int)sizeof(E), CPR = 128 / EPC, KSTAGE = 128 / (int)sizeof(E);
    if (k0 + KSTAGE <= k_end) {                 // (wave-uniform) a whole stage: nothing to zero
        op_lstore<E, KS, NCH>(base, tid, r, ones);
        return;
    }
    const u32x4 one = {sizeof(E) == 2 ? 0x3F80u : 0x3F800000u, 0u, 0u, 0u};
    u32x4 m[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const bool ok = KS ? (k0 + (tid + kGT * i) / CPR < k_end) : (k0 + (tid & 7) * EPC < k_end);
        m[i] = ok ? ((ones >> i) & 1u ? one : r[i]) : u32x4{0u, 0u, 0u, 0u};       // (rows past k_end contribute nothing)
    }
    op_lstore<E, KS, NCH>(base, tid, m);
}

// MFMA operand fragment of 16-row tile `tile` (0..7 of the block tile), half-stage s (0/1).
// k mapping (both layouts, both operands): bf16 slot j of lane group g is k = 32 s + 8 g + j; fp32 element j of
// lane group g is k = 16 s + 4 g + j.
template <typename E, bool KS>
__device__ __forceinline__ u32x4 op_frag(const unsigned char* base, int tile, int s, int lane) {
    const int i = lane & 15, g = lane >> 4;
    if (!KS) {
        const int row = tile * 16 + i, kc = s * 4 + g;
        return *(const u32x4*)(base + row * 128 + ((kc ^ (row & 7)) << 4));
    } else if (sizeof(E) == 2) {
        // ds_read_b64_tr_b16: the 16 lanes of a group cover a [4 k][16 col] block (lane i: k-row i/4, columns
        // 4(i%4)..+3) and receive column i of it, k-rows 0..3.  Two reads (h = 0, 1) = k 8g .. 8g+7 of column i.
        const unsigned char* p = base + tile * kSubBytes + (s * 32 + 4 * g + (i >> 2)) * 32 + (i & 3) * 8;   // permuted rows
        typedef s16x4 __attribute__((address_space(3))) * lds_s16x4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p + 16 * 32));
        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        return u32x4{l2.x, l2.y, h2.x, h2.y};
    } else {
        u32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = *(const uint32_t*)(base + (s * 16 + 4 * g + j) * kRowBytes32 + (tile * 16 + i) * 4);
        return v;
    }
}

template <typename E> __device__ __forceinline__ void mma16(f32x4& acc, const u32x4& a, const u32x4& b);
template <> __device__ __forceinline__ void mma16<uint16_t>(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
template <> __device__ __forceinline__ void mma16<float>(f32x4& acc, const u32x4& a, const u32x4& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), acc, 0, 0, 0);
}

typedef unsigned char TileLds[2][2][kOpBytes];

// Workgroups are dealt to the 8 XCDs round robin by blockIdx.x, and every XCD has its own 4 MB L2.  Tiles that are
// neighbours in the logical order share an operand panel (same rows of A, next columns of B), so each XCD takes a
// CONTIGUOUS run of logical tiles: the panel is then fetched into one L2 instead of eight.
__device__ __forceinline__ int xcd_tile(int b, int nb) {
    const int per = nb >> 3, rem = nb & 7, x = b & 7, i = b >> 3;
    return x * per + (x < rem ? x : rem) + i;
}

// An epilogue with column sums (kColSum) that declares kColPart = true stores them per 64-row wave into a slab instead of
// adding them with atomics (BESO_TRAIN_DETERMINISTIC: part_reduce_kernel sums the slab's rows in index order).
template <typename Epi, typename = void> struct EpiColPart : std::false_type {};
template <typename Epi> struct EpiColPart<Epi, std::enable_if_t<Epi::kColPart>> : std::true_type {};

// One 128 x 128 output tile at (m0, n0), contraction over [k_begin, k_end): 8 waves as 2 (m) x 4 (n), 64 x 32 each.
// Register-staged pipeline with two register sets (see the loop).  Loads and LDS stores are unconditional -- a
// stage past k_end is read at a valid address and stored as zeros -- so that the compiler's vmcnt bookkeeping
// stays exact.  (Measured without effect on the six-stage GEMMs of the step: persistent workgroups that keep the
// pipeline filled across tiles, 128-byte aligned leading dimensions.)
template <typename E, bool AKS, bool BKS, typename Epi>
__device__ __forceinline__ void tgemm_tile(TileLds& lds, const E* __restrict__ A, int lda, const E* __restrict__ B, int ldb,
                                           int M, int N, int m0, int n0, int k_begin, int k_end, const Epi& epi) {
    constexpr int KSTAGE = 128 / (int)sizeof(E);
    constexpr int NA = kGL;                            // 16-byte chunks of A per thread and stage
    constexpr int NI = 128 / (16 * kWN);               // 16-column MFMA tiles per wave
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / kWN, wn = wid % kWN;
    const int nk = (k_end - k_begin + KSTAGE - 1) / KSTAGE;

    f32x4 acc[4][NI];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](const unsigned char* la, const unsigned char* lb) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            u32x4 bf[NI];                                 // (the two B fragments stay, the four A fragments pass through)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) bf[ni] = op_frag<E, BKS>(lb, wn * NI + ni, s, lane);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const u32x4 af = op_frag<E, AKS>(la, wm * 4 + mi, s, lane);
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) mma16<E>(acc[mi][ni], bf[ni], af);   // D[n][m]: 4 consecutive n per lane
            }
            __builtin_amdgcn_sched_barrier(0);              // keeps the second half-stage's fragment reads out of the first (VGPRs)
        }
    };
    if (nk > 0) {
        // Two register sets, ping-pong: the stage that landed during the previous iteration is written to LDS BEFORE
        // the MFMAs of the current one while the stage after it is being fetched -- no wait for memory inside the
        // loop, LDS writes under the matrix pipe (the weight-gradient launch, hundreds of stages per tile: -29 %).
        u32x4 a0[NA], b0[kGL], a1[NA], b1[kGL];
        const GOp<NA> ga = make_gop<E, AKS, NA>(A, lda, m0, M, tid);
        const GOp<kGL> gb = make_gop<E, BKS, kGL>(B, ldb, n0, N, tid);
        uint32_t b_ones = 0u;                             // chunks of this thread that start at column N of B (the ones column)
        if constexpr (Epi::kBiasCol) {
            static_assert(BKS, "the ones column is a column of a k-slow B operand");
            constexpr int EPC = 16 / (int)sizeof(E), CPR = 128 / EPC;
            if (epi.bias) {
#pragma unroll
                for (int i = 0; i < kGL; ++i) b_ones |= (n0 + ((tid + kGT * i) % CPR) * EPC == N ? 1u : 0u) << i;
            }
        }
        auto load0 = [&](int kt) {
            op_gload<E, AKS, NA, true>(A, ga, lda, k_begin + kt * KSTAGE, k_end, tid, a0);
            op_gload<E, BKS, kGL, true>(B, gb, ldb, k_begin + kt * KSTAGE, k_end, tid, b0);
        };
        auto load1 = [&](int kt) {
            op_gload<E, AKS, NA, true>(A, ga, lda, k_begin + kt * KSTAGE, k_end, tid, a1);
            op_gload<E, BKS, kGL, true>(B, gb, ldb, k_begin + kt * KSTAGE, k_end, tid, b1);
        };
        load0(0);
        load1(1);
        op_lstore_masked<E, AKS, NA>(lds[0][0], tid, a0, k_begin, k_end);
        op_lstore_masked<E, BKS, kGL>(lds[0][1], tid, b0, k_begin, k_end, b_ones);
        __syncthreads();
        for (int kt = 0; kt < nk; kt += 2) {
            load0(kt + 2);
            __builtin_amdgcn_sched_barrier(0);          // the loads are issued HERE (the scheduler sinks them below the MFMAs)
            op_lstore_masked<E, AKS, NA>(lds[1][0], tid, a1, k_begin + (kt + 1) * KSTAGE, k_end);
            op_lstore_masked<E, BKS, kGL>(lds[1][1], tid, b1, k_begin + (kt + 1) * KSTAGE, k_end, b_ones);
            compute(lds[0][0], lds[0][1]);
            __syncthreads();
            if (kt + 1 >= nk) break;
            load1(kt + 3);
            __builtin_amdgcn_sched_barrier(0);
            op_lstore_masked<E, AKS, NA>(lds[0][0], tid, a0, k_begin + (kt + 2) * KSTAGE, k_end);
            op_lstore_masked<E, BKS, kGL>(lds[0][1], tid, b0, k_begin + (kt + 2) * KSTAGE, k_end, b_ones);
            compute(lds[1][0], lds[1][1]);
            __syncthreads();
        }
    }
    int te = tid;
    asm volatile("" : "+v"(te));          // epilogue addresses are formed HERE, not hoisted above the k loop (spills)
    // The MFMA ran as D = Bfrag x Afrag^T: the lane holds C[m][n..n+3] with m = lane & 15, n = 4*(lane >> 4) + reg,
    // so every epilogue access is a 4-element vector (N % 4 == 0).
    const int le = te & 63, wme = (te >> 6) / kWN, wne = (te >> 6) % kWN;
    f32x4 cs[NI];                         // column sums of what this lane stored (epilogues with a bias gradient)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) cs[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int m = m0 + wme * 64 + mi * 16 + (le & 15);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int n = n0 + wne * (16 * NI) + ni * 16 + (le >> 4) * 4;
            if (m < M && n < N) {
                if constexpr (Epi::kColSum) cs[ni] += epi(m, n, acc[mi][ni]);
                else epi(m, n, acc[mi][ni]);
            }
            if constexpr (Epi::kBiasCol) {
                if (m < M && n == N && epi.bias) epi.bias[m] = acc[mi][ni][0] + (epi.add ? epi.bias[m] : 0.f);      // the ones column: sum over the rows of A's column m
            }
        }
    }
    if constexpr (Epi::kColSum) {
        // the 16 lanes with the same lane >> 4 hold the same four columns for 16 different rows: butterfly over
        // lane & 15, then one atomic per column, wave and tile (64 rows each)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1)
#pragma unroll
                for (int r = 0; r < 4; ++r) cs[ni][r] += __shfl_xor(cs[ni][r], o, 64);
            const int n = n0 + wne * (16 * NI) + ni * 16 + (le >> 4) * 4;
            if ((le & 15) == 0 && n < N) {
                if constexpr (EpiColPart<Epi>::value) {
                    // BESO_TRAIN_DETERMINISTIC: epi.colsum is a slab [2 * row tiles][N]; this wave's 64 rows are its row
                    // m0 / 64 + wave row, a plain store (every row of the slab is written: rows past M add zeros)
                    static_assert(kTileMN == 128, "two 64-row waves per tile");
                    *(f32x4*)(epi.colsum + (size_t)((m0 >> 6) + wme) * N + n) = cs[ni];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) unsafeAtomicAdd(epi.colsum + n + r, cs[ni][r]);
                }
            }
        }
    }
}

template <typename E, bool AKS, bool BKS, typename Epi>
__global__ __launch_bounds__(kGT, kOcc) void tgemm_kernel(const E* __restrict__ A, int lda, const E* __restrict__ B,
                                                       int ldb, int M, int N, int K, int k_per_split, int nt_n,
                                                       Epi epi) {
    __shared__ __attribute__((aligned(16))) TileLds lds;
    const int bt = xcd_tile(blockIdx.x, gridDim.x);
    const int tile_n = bt % nt_n, tile_m = bt / nt_n;
    const int k_begin = blockIdx.y * k_per_split;
    tgemm_tile<E, AKS, BKS, Epi>(lds, A, lda, B, ldb, M, N, tile_m * kTileMN, tile_n * kTileMN, k_begin,
                                 min(K, k_begin + k_per_split), epi);
}

// ---- epilogues: (m, n, v) = C[m][n..n+3] ------------------------------------------------------
template <typename E> struct Vec4;
template <> struct Vec4<float> {
    __device__ static __forceinline__ f32x4 load(const float* p) { return *(const f32x4*)p; }
    __device__ static __forceinline__ void store(float* p, const f32x4& v) { *(f32x4*)p = v; }
    __device__ static __forceinline__ f32x4 rounded(const f32x4& v) { return v; }
};
template <> struct Vec4<uint16_t> {
    __device__ static __forceinline__ f32x4 load(const uint16_t* p) {
        const uint2 u = *(const uint2*)p;
        return f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u)};
    }
    __device__ static __forceinline__ void store(uint16_t* p, const f32x4& v) {
        uint2 u;
        u.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
        u.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
        *(uint2*)p = u;
    }
    __device__ static __forceinline__ f32x4 rounded(const f32x4& v) {
        return f32x4{bf2f(f2bf(v[0])), bf2f(f2bf(v[1])), bf2f(f2bf(v[2])), bf2f(f2bf(v[3]))};
    }
};

template <typename E> struct EpiStore {          // out = acc + bias  (fp32 and / or operand-typed copy)
    static constexpr bool kColSum = false; static constexpr bool kBiasCol = false;
    float* o32; E* oe; const float* bias; int ld;
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        if (bias) v += *(const f32x4*)(bias + n);
        const size_t i = (size_t)m * ld + n;
#ifdef BESO_TGEMM_NOSTORE               // timing experiment: the GEMM without its output traffic
        if (v[0] != 12345.678f) return;
#endif
        if (o32) *(f32x4*)(o32 + i) = v;
        if (oe) Vec4<E>::store(oe + i, v);
    }
};
template <typename E> struct EpiFc1 {            // h = acc + bias (kept for GELU'), g = GELU(h)   (score_gpts.py:105-108)
    static constexpr bool kColSum = false; static constexpr bool kBiasCol = false;
    E* h; E* g; const float* bias; int ld;
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        v += *(const f32x4*)(bias + n);
        const size_t i = (size_t)m * ld + n;
        Vec4<E>::store(h + i, v);
        Vec4<E>::store(g + i, f32x4{gelu_t<E>(v[0]), gelu_t<E>(v[1]), gelu_t<E>(v[2]), gelu_t<E>(v[3])});
    }
};
struct EpiResid {                                // x_out = x_in + dropout(acc + bias)              (:79,:109,:113-114)
    static constexpr bool kColSum = false; static constexpr bool kBiasCol = false;
    const float* xin; float* xout; const float* bias; int ld; float p, inv_keep; uint32_t seed, site;
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        v += *(const f32x4*)(bias + n);
        const size_t i = (size_t)m * ld + n;
        if (p > 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= drop_scale(seed, site, i + j, p, inv_keep);
        }
        *(f32x4*)(xout + i) = *(const f32x4*)(xin + i) + v;
    }
};
template <typename E> struct EpiGeluBwd {        // dh = dg * GELU'(h); its column sums are the FC1 bias gradient
    static constexpr bool kColSum = true; static constexpr bool kBiasCol = false;
    const E* h; E* dh; float* colsum; int ld;
    __device__ __forceinline__ f32x4 operator()(int m, int n, f32x4 v) const {
        const size_t i = (size_t)m * ld + n;
        const f32x4 hv = Vec4<E>::load(h + i);
        const f32x4 d = {v[0] * gelu_grad_t<E>(hv[0]), v[1] * gelu_grad_t<E>(hv[1]), v[2] * gelu_grad_t<E>(hv[2]),
                         v[3] * gelu_grad_t<E>(hv[3])};
        Vec4<E>::store(dh + i, d);
        return Vec4<E>::rounded(d);      // the sum is taken over the values as stored (what the weight gradient sees)
    }
};
template <typename E> struct EpiSilu {           // z = acc + bias (kept for SiLU'), a = SiLU(z): the hidden layer of the MLP action head
    static constexpr bool kColSum = false; static constexpr bool kBiasCol = false;       // (score_gpts.py:187-191: Linear(D,100) - SiLU - Linear(100,act))
    E* z; E* a; const float* bias; int ld;
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        v += *(const f32x4*)(bias + n);
        const size_t i = (size_t)m * ld + n;
        Vec4<E>::store(z + i, v);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = v[j] / (1.0f + expf(-v[j]));
        Vec4<E>::store(a + i, o);
    }
};
template <typename E> struct EpiSiluBwd {        // dz = da * SiLU'(z); column sums = bias gradient of the hidden layer
    static constexpr bool kColSum = true; static constexpr bool kBiasCol = false;
    const E* z; E* dz; float* colsum; int ld;
    __device__ __forceinline__ f32x4 operator()(int m, int n, f32x4 v) const {
        const size_t i = (size_t)m * ld + n;
        const f32x4 zv = Vec4<E>::load(z + i);
        f32x4 d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float sg = 1.0f / (1.0f + expf(-zv[j]));
            d[j] = v[j] * sg * (1.0f + zv[j] * (1.0f - sg));
        }
        Vec4<E>::store(dz + i, d);
        return Vec4<E>::rounded(d);
    }
};
// ... and their deterministic forms: `colsum` is the slab [2 * ceil(M / 128)][N] (EpiColPart)
template <typename E> struct EpiGeluBwdPart : EpiGeluBwd<E> { static constexpr bool kColPart = true; };
template <typename E> struct EpiSiluBwdPart : EpiSiluBwd<E> { static constexpr bool kColPart = true; };
#if BESO_DEV_API
struct EpiAtomic {                               // split-K partial sums accumulated with atomics (debug entry point)
    static constexpr bool kColSum = false; static constexpr bool kBiasCol = false;
    float* out; int ld;
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        float* o = out + (size_t)m * ld + n;
#pragma unroll
        for (int r = 0; r < 4; ++r) unsafeAtomicAdd(o + r, v[r]);
    }
};
inline EpiAtomic epi_atomic(float* out, int ld) { return EpiAtomic{out, ld}; }
#endif
template <typename E, bool AKS, bool BKS, typename Epi>
hipError_t tgemm(const void* A, int lda, const void* B, int ldb, int M, int N, int K, int splits, Epi epi, hipStream_t s) {
    (void)hipGetLastError();
    constexpr int EPC = 16 / (int)sizeof(E), KSTAGE = 128 / (int)sizeof(E);
    if (M < 1 || N < 1 || K < 1) return hipErrorInvalidValue;
    if ((AKS ? M : K) % EPC != 0 || (BKS ? N : K) % EPC != 0 || lda % EPC != 0 || ldb % EPC != 0 || N % 4 != 0)
        return hipErrorInvalidValue;
    if (((uintptr_t)A | (uintptr_t)B) & 15) return hipErrorInvalidValue;
    // 32-bit byte offsets inside an operand (raw buffer loads)
    if ((size_t)(AKS ? K : M) * lda * sizeof(E) >= ((size_t)1 << 31) || (size_t)(BKS ? K : N) * ldb * sizeof(E) >= ((size_t)1 << 31))
        return hipErrorInvalidValue;
    const int nt_n = (N + kTileMN - 1) / kTileMN, nt_m = (M + kTileMN - 1) / kTileMN;
    if (splits < 1) splits = 1;
    const int kps = ((K + splits - 1) / splits + KSTAGE - 1) / KSTAGE * KSTAGE;
    splits = (K + kps - 1) / kps;
    // (64-row tiles for the GEMMs whose 128-row grid is under one round of workgroups measured 20 % SLOWER: the kernel
    //  is bound by operand bytes per FLOP through LDS, not by idle CUs)
    hipLaunchKernelGGL((tgemm_kernel<E, AKS, BKS, Epi>), dim3(nt_n * nt_m, splits), dim3(kGT), 0, s, (const E*)A, lda,
                       (const E*)B, ldb, M, N, K, kps, nt_n, epi);
    return hipGetLastError();
}

// All weight gradients of a step in ONE launch: problem p is C_p[Mo][No] = A_p^T B_p over the M token rows (both
// operands k-slow: the kept activation and the kept output gradient as they lie).  Every tile contracts over
// the whole token range and stores its result -- no split-K, no atomics (fp32 atomics sustain ~35 G/s on this
// part: a split-K version spent more time adding partial sums than multiplying), no reduction pass; a few hundred
// tiles of equal length fill the chip by themselves.
struct GProb { const void* A; const void* B; float* out; float* bias; int lda, ldb, Mo, No, tile_begin, nt_n, K;
               uint32_t slab_off; };   // bias: column sums of A (or nullptr); slab_off: this problem's floats in a split's slab (out, then bias)
constexpr int kMaxGroup = 56;                          // 6 per layer + 2: up to 9 layers per launch, more launches beyond (a 4 KiB kernel argument)
struct GTable { GProb p[kMaxGroup]; int n; };
struct EpiStoreF { static constexpr bool kColSum = false; static constexpr bool kBiasCol = true; float* out; int ld; float* bias;
    bool add;                                          // out += v (a later row window of the same product: launches in stream order)
    __device__ __forceinline__ void operator()(int m, int n, f32x4 v) const {
        f32x4* o = (f32x4*)(out + (size_t)m * ld + n);
        *o = add ? *o + v : v;
    } };

// splits > 1 (round 4): the contraction -- the TOKEN ROWS of the step -- is cut into `splits` ranges, one workgroup per (tile,
// range); range z writes its partial tile into slab z (wgrad_reduce_kernel adds the slabs up in a fixed order: deterministic,
// no atomics).  A 6-layer kitchen step has 75 output tiles for 256 CUs x 2 workgroup slots, each a latency chain over all
// 11,264 rows (176 stages): 417 us of the 2.26 ms step at 2 % of the matrix pipe.
template <typename E>
__global__ __launch_bounds__(kGT, kOcc) void tgemm_wgrad_group_kernel(GTable t, int n_tiles, int splits, float* slab,
                                                                      size_t slab_stride, int win, int n_win) {
    const int v = xcd_tile(blockIdx.x, gridDim.x);
    const int z = v / n_tiles, b = v - z * n_tiles;
    int pi = 0;
    while (pi + 1 < t.n && b >= t.p[pi + 1].tile_begin) ++pi;
    const GProb g = t.p[pi];
    const int local = b - g.tile_begin, tile_n = local % g.nt_n, tile_m = local / g.nt_n;
    __shared__ __attribute__((aligned(16))) TileLds lds;
    constexpr int KSTAGE = 128 / (int)sizeof(E);
    int k0 = 0, k1 = g.K;
    float* out = g.out; float* bias = g.bias;
    if (splits > 1) {
        const int kc = ((g.K + splits - 1) / splits + KSTAGE - 1) / KSTAGE * KSTAGE;
        k0 = min(z * kc, g.K); k1 = min(k0 + kc, g.K);
        out = slab + (size_t)z * slab_stride + g.slab_off;
        if (bias) bias = out + (size_t)g.Mo * g.No;
    }
    if (n_win > 1) {                                  // row window `win` of n_win (one launch per window)
        const int kc = ((g.K + n_win - 1) / n_win + KSTAGE - 1) / KSTAGE * KSTAGE;
        k0 = min(win * kc, g.K); k1 = min(k0 + kc, g.K);
    }
    tgemm_tile<E, true, true, EpiStoreF>(lds, (const E*)g.A, g.lda, (const E*)g.B, g.ldb, g.Mo, g.No, tile_m * kTileMN,
                                         tile_n * kTileMN, k0, k1, EpiStoreF{out, g.No, bias, n_win > 1 && win > 0});
}

// out (and bias) of every problem of a split launch = the sum of its slabs, z = 0 .. splits-1 in that order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(GTable t, const float* __restrict__ slab, size_t slab_stride,
                                                           int splits, uint32_t total) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        int lo = 0, hi = t.n - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.p[mid].slab_off <= i) lo = mid; else hi = mid - 1; }
        const GProb& g = t.p[lo];
        const uint32_t k = i - g.slab_off, no = (uint32_t)g.Mo * (uint32_t)g.No;
        float* dst = k < no ? g.out + k : ((g.bias && k < no + (uint32_t)g.Mo) ? g.bias + (k - no) : nullptr);
        if (!dst) continue;                                   // (alignment padding between two problems)
        float acc = 0.f;
        for (int z = 0; z < splits; ++z) acc += slab[(size_t)z * slab_stride + i];
        *dst = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// Round 5: PANEL-OWNING weight-gradient tiles (bf16).  The 128 x 128 tiles above read every operand panel once per tile that
// shares it -- 36 tiles of an FC1 / FC2 weight gradient share 15 panels -- and rely on an XCD's 4 MB L2 to serve the
// sharers, which drift apart over the 176 ... 1408 stages of a contraction: FETCH_SIZE 1.78 GB for 0.78 GB of operands at
// 1024 kitchen samples (3.7 x at 8192), the launch bound by the fabric behind L2.  Every weight gradient of the network has
// one side of width D (or less): here a tile covers ALL of that side -- 128 x (128 W) or (128 W) x 128, W = ceil(D / 128)
// in {2, 3} -- so the LARGE operand (GELU(h), dh, dqkv: 4 D or 3 D wide) is read exactly once by exactly one workgroup, and
// only the D-wide panel (dyo, xn2, y, xn1) is shared, by all tiles of its problem at the same stage.  Kitchen: 36 tiles per
// layer, 218 per step = ONE round of one workgroup per CU (no second round to start out of step), a wave tile of 64 x 96
// (or 96 x 64): 10 fragment reads per 24 MFMAs instead of 6 per 8.  Same operand images in LDS as tgemm_tile (k-slow
// 16-column subtiles, ds_read_b64_tr_b16), same epilogue and ones column; ONE register set in the pipeline (see the loop).
// ---------------------------------------------------------------------------------------------
template <int MT, int NT>
__device__ __forceinline__ void wgrad_panel_tile(unsigned char* lds, const uint16_t* __restrict__ A, int lda,
                                                 const uint16_t* __restrict__ B, int ldb, int M, int N, int m0, int n0,
                                                 int k_begin, int k_end, const EpiStoreF& epi) {
    typedef uint16_t E;
    static_assert(kNW == 8 && kGL == 2, "eight waves, two 16-byte chunks per thread and 128-column block");
    constexpr int KSTAGE = 64;
    constexpr int WM = MT >= NT ? 4 : 2, WN = 8 / WM;        // waves along m and n
    constexpr int MI = 8 * MT / WM, NI = 8 * NT / WN;        // 16-row MFMA tiles per wave: 4 x 6, 6 x 4 or 4 x 4
    constexpr int A_BYTES = 8 * MT * kSubBytes, STAGE = 8 * (MT + NT) * kSubBytes;      // one stage: A's subtiles, then B's
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int nk = (k_end - k_begin + KSTAGE - 1) / KSTAGE;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    // One stage = two k-steps of 32.  FRAGMENT PIPELINE: the A fragment of row tile mi + 1 -- in the last group of the first k-step,
    // the B fragments and the first A fragment of the second k-step -- is requested BEFORE the MFMAs of row tile mi, so the matrix
    // pipe works on group mi while the LDS pipe fetches group mi + 1 (with the reads issued just in time the two pipes took
    // turns: LDS 1750 + MFMA 1540 clocks of a 3400-clock stage).  `head` issues the stage's first fragments; the caller puts the
    // global -> LDS traffic of the next stage between `head` and `body`.
    u32x4 bf[NI], af;
    auto head = [&](const unsigned char* st) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) bf[ni] = op_frag<E, true>(st + A_BYTES, wn * NI + ni, 0, lane);
        af = op_frag<E, true>(st, wm * MI, 0, lane);
    };
    auto body = [&](const unsigned char* st) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                u32x4 an = af, bn[NI];
                if (mi + 1 < MI) an = op_frag<E, true>(st, wm * MI + mi + 1, s, lane);
                else if (s == 0) {
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) bn[ni] = op_frag<E, true>(st + A_BYTES, wn * NI + ni, 1, lane);
                    an = op_frag<E, true>(st, wm * MI, 1, lane);
                }
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) mma16<E>(acc[mi][ni], bf[ni], af);      // D[n][m]: 4 consecutive n per lane
                af = an;
                if (mi + 1 == MI && s == 0) {
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) bf[ni] = bn[ni];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    if (nk > 0) {
        // Global side: one 16-byte chunk = (k-row, 8 columns); per-chunk byte offsets inside a stage are formed once, a column
        // outside the operand gets an offset beyond every range (reads zeros).  The k advance goes into the buffer descriptor:
        // base = first row of the stage, num_records = the bytes up to k_end -- so rows past the end of the contraction, whole
        // stages past it included, are zeros BY THE DESCRIPTOR'S RANGE CHECK: no predicates, no masked LDS stores, exact vmcnt.
        uint32_t va[MT][kGL], vb[NT][kGL];
#pragma unroll
        for (int i = 0; i < kGL; ++i) {
            const int c = tid + kGT * i, krow = c >> 4, cc = c & 15;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int gc = m0 + 128 * j + cc * 8;
                va[j][i] = gc < M ? (uint32_t)((krow * lda + gc) * 2) : 0x80000000u;
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int gc = n0 + 128 * j + cc * 8;
                vb[j][i] = gc < N ? (uint32_t)((krow * ldb + gc) * 2) : 0x80000000u;
            }
        }
        uint32_t b_ones[NT];                               // chunks of this thread that start at column N of B (the ones column)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            b_ones[j] = 0u;
            if (epi.bias) {
#pragma unroll
                for (int i = 0; i < kGL; ++i) b_ones[j] |= (n0 + 128 * j + ((tid + kGT * i) & 15) * 8 == N ? 1u : 0u) << i;
            }
        }
        auto uniform_ptr = [](const void* p) {
            const uint64_t pv = (uint64_t)p;
            return (void*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(pv >> 32)) << 32) |
                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)pv));
        };
        auto load = [&](int kt, u32x4 (&ra)[MT][kGL], u32x4 (&rb)[NT][kGL]) {
            const int k0 = k_begin + kt * KSTAGE;
            const int rows = k0 < k_end ? k_end - k0 : 0;
            const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(
                uniform_ptr(A + (rows ? (size_t)k0 * lda : 0)), 0, rows * lda * 2, 0x00020000);
            const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(
                uniform_ptr(B + (rows ? (size_t)k0 * ldb : 0)), 0, rows * ldb * 2, 0x00020000);
#pragma unroll
            for (int j = 0; j < MT; ++j)
#pragma unroll
                for (int i = 0; i < kGL; ++i) ra[j][i] = __builtin_amdgcn_raw_buffer_load_b128(rsa, va[j][i], 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int i = 0; i < kGL; ++i) rb[j][i] = __builtin_amdgcn_raw_buffer_load_b128(rsb, vb[j][i], 0, 0);
        };
        auto store = [&](unsigned char* st, const u32x4 (&ra)[MT][kGL], const u32x4 (&rb)[NT][kGL]) {
#pragma unroll
            for (int j = 0; j < MT; ++j) op_lstore<E, true, kGL>(st + 8 * j * kSubBytes, tid, ra[j]);
#pragma unroll
            for (int j = 0; j < NT; ++j) op_lstore<E, true, kGL>(st + A_BYTES + 8 * j * kSubBytes, tid, rb[j], b_ones[j]);
        };
        // ONE register set (a stage is 128 B per thread): the stage that landed during the previous iteration's MFMAs is written
        // to the other LDS buffer, the stage after it requested, then the MFMAs of the current one run -- every load has a whole
        // compute phase to land
        u32x4 ar[MT][kGL], br[NT][kGL];
        load(0, ar, br);
        store(lds, ar, br);
        load(1, ar, br);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            head(lds + (kt & 1) * STAGE);
            __builtin_amdgcn_sched_barrier(0);
            store(lds + ((kt + 1) & 1) * STAGE, ar, br);      // (a stage past the end is zeros and never read)
            load(kt + 2, ar, br);
            __builtin_amdgcn_sched_barrier(0);          // the loads are issued HERE (the scheduler sinks them below the MFMAs)
            body(lds + (kt & 1) * STAGE);
            __syncthreads();
        }
    }
    int te = tid;
    asm volatile("" : "+v"(te));          // epilogue addresses are formed HERE, not hoisted above the k loop (spills)
    const int le = te & 63, wme = (te >> 6) / WN, wne = (te >> 6) % WN;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = m0 + wme * (16 * MI) + mi * 16 + (le & 15);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int n = n0 + wne * (16 * NI) + ni * 16 + (le >> 4) * 4;
            if (m < M && n < N) epi(m, n, acc[mi][ni]);
            if (m < M && n == N && epi.bias) epi.bias[m] = acc[mi][ni][0] + (epi.add ? epi.bias[m] : 0.f);      // the ones column
        }
    }
}

constexpr size_t wgrad_panel_lds(int W) { return (size_t)2 * 8 * (W + 1) * kSubBytes; }     // two stages of (1 + W) 128-column blocks

// The grouped launch on panel-owning tiles.  GProb::nt_n carries the orientation: 0 = the tile covers all No columns (128 rows
// of Mo per tile), -1 = it covers all Mo rows (128 columns of No per tile); tile_begin counts those tiles.
template <int W>
__global__ __launch_bounds__(kGT, 2) void wgrad_panel_group_kernel(GTable t, int n_tiles, int splits, float* slab,
                                                                  size_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plds[];
    const int v = xcd_tile(blockIdx.x, gridDim.x);
    const int z = v / n_tiles, b = v - z * n_tiles;
    int pi = 0;
    while (pi + 1 < t.n && b >= t.p[pi + 1].tile_begin) ++pi;
    const GProb g = t.p[pi];
    const int local = b - g.tile_begin;
    int k0 = 0, k1 = g.K;
    float* out = g.out; float* bias = g.bias;
    if (splits > 1) {
        const int kc = ((g.K + splits - 1) / splits + 63) / 64 * 64;
        k0 = min(z * kc, g.K); k1 = min(k0 + kc, g.K);
        out = slab + (size_t)z * slab_stride + g.slab_off;
        if (bias) bias = out + (size_t)g.Mo * g.No;
    }
    const EpiStoreF epi{out, g.No, bias, false};
    if (g.nt_n == 0)
        wgrad_panel_tile<1, W>(plds, (const uint16_t*)g.A, g.lda, (const uint16_t*)g.B, g.ldb, g.Mo, g.No, local * kTileMN, 0, k0, k1, epi);
    else
        wgrad_panel_tile<W, 1>(plds, (const uint16_t*)g.A, g.lda, (const uint16_t*)g.B, g.ldb, g.Mo, g.No, 0, local * kTileMN, k0, k1, epi);
}

// W of the panel kernel for a model of width D (0: the 128 x 128 tiles stay)
static int wgrad_panel_w(int D, size_t elem_bytes) {
    if (elem_bytes != 2) return 0;
    return D > 128 && D <= 256 ? 2 : (D > 256 && D <= 384 ? 3 : 0);
}
// tiles of problem (Mo, No) on panel tiles of width W; *orient = 0 / -1 as GProb::nt_n (a problem with neither side within
// 128 W does not exist in this network: every weight gradient has a side of width <= D)
static int wgrad_panel_tiles(int Mo, int No, int W, int* orient) {
    if (No <= 128 * W) { *orient = 0; return (Mo + kTileMN - 1) / kTileMN; }
    *orient = -1;
    return (No + kTileMN - 1) / kTileMN;
}
