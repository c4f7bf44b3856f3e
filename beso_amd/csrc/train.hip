// Training step of the score network in HIP (row f1): GCDenoiser.loss forward + the gradient of the loss
// with respect to every parameter, enqueued on one stream.
//   reference: score_wrappers.py:45-79 (loss), score_gpts.py:272-358 (network), beso_agent.py:215-248 (step)
//
// Structure (M = batch * T token rows; E = GEMM operand type: bf16, or fp32 in the parity mode):
//   forward    prep (noised action, target) -> embed (x0, feature matrix Xemb) -> L x [ LN1 -> QKV GEMM ->
//              attention (dropout on the probabilities) -> proj GEMM + residual -> LN2 -> FC1 GEMM (+GELU) ->
//              FC2 GEMM + residual ] -> ln_f -> head GEMM -> squared error.  Every GEMM input is kept.
//   backward   the same chain reversed.  All contractions run on ONE MFMA GEMM kernel (`tgemm_kernel`) whose
//              operands may be stored contraction-major ("k-slow"): dgrad reads W[out][in] as it lies
//              (contraction over `out`), wgrad reads dY[m][n] and X[m][k] as they lie (contraction over the
//              token index m).  k-slow bf16 tiles are fetched from LDS with ds_read_b64_tr_b16 (the gfx950
//              transpose read), k-slow fp32 tiles with plain ds_read_b32 (v_mfma_f32_16x16x4_f32 takes one
//              element per lane), so nothing is ever transposed through HBM.  The weight gradients of the whole
//              step run as ONE grouped launch after the data-gradient chain (every tile contracts over all token
//              rows and stores its result: no split-K, no atomics).
//   LayerNorm backward also carries the residual gradient and emits its operand-typed copy (with the
//   dropout mask of the consuming linear layer) and that layer's bias gradient; GELU' is the epilogue of the FC2
//   dgrad GEMM.  Bias / LayerNorm-affine gradients are the only accumulations (block partials + one reduction,
//   or a handful of atomics per block): the flat gradient buffer is zeroed first.  BESO_TRAIN_DETERMINISTIC replaces
//   the atomics (column-sum epilogues, colsum_kernel, loss_kernel) by partial sums in a workspace slab and a second
//   launch that adds them in index order (kColPart epilogues, colsum_part_kernel, loss_part_kernel).
// Dropout masks come from a counter-based hash of (seed, site, element index): the backward recomputes them.
//
// Contents.  The device code lies in three headers, included below in dependency order (none of them sees the host):
//   train_gemm.h   the tile GEMM family: operand loaders, tgemm, the epilogues, the grouped and panel weight-gradient kernels
//   train_attn.h   the four attention kernels
//   train_rows.h   the row and elementwise kernels: masks, packing, embedding, LayerNorm, column sums, gather / scatter, loss, VJP
// This file is the host, in this order:
//   device_cus, the step's events and side stream
//   workspace      TrainLayerWs / TrainWs, make_train_ws; train_validate, train_workspace_bytes, train_early_*, train_grad_floats
//   launch helpers tail_forward_enabled, capped_grid, with_ln_vec, part_reduce, colsum, launch_panel_group; TrainCall
//   plan           TrainPlan, make_train_plan
//   LnPartials     the slabs of the LayerNorm backward partial sums and their one reduction
//   WgradGroup     the grouped weight-gradient launch: add, arrange, flush
//   TrainStep      the phases in the order run() calls them; run_train_step
//   entry points   train_loss_grad, train_denoise_vjp, train_goal_mask, train_dropout_mask, train_debug_gemm (dev build)
#include <string.h>
#include <atomic>
#include <type_traits>
#include "common.h"
#include "fused.h"
#include "train.h"

namespace beso {
namespace {

#include "train_gemm.h"
#include "train_attn.h"
#include "train_rows.h"

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// compute units of the current device (cached per device; 256 on the MI355X): the row-range heuristics of the grouped
// weight-gradient launches fill THIS part's workgroup slots
static int device_cus() {
    constexpr int kMaxDev = 64;
    static std::atomic<int> cached[kMaxDev] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// Events that order the step's side streams, per calling thread AND per device (an event created on device A and
// recorded on a stream of device B is hipErrorInvalidHandle -- a thread that drives several GPUs one after the other)
enum { kEvFork = 0, kEvJoin, kEvCopies, kEvLoss, kEvEarly, kEvSideFork, kEvSideJoin, kEvWcat, kEvCount };
static hipError_t step_event(int which, hipEvent_t* out) {
    constexpr int kMaxDev = 64;
    static thread_local hipEvent_t ev[kMaxDev][kEvCount] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
    if (!ev[dev][which]) {
        e = hipEventCreateWithFlags(&ev[dev][which], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    *out = ev[dev][which];
    return hipSuccess;
}

// A stream of the library's own per calling thread and device: work of the step that depends on neither the caller's side
// streams nor the launch it runs beside (round 5: the small reductions of the bias / LayerNorm partial sums under the grouped
// weight-gradient launch).  Forked from and joined to the compute stream with events inside the call -- the caller never sees it.
static hipError_t step_side_stream(hipStream_t* out) {
    constexpr int kMaxDev = 64;
    static thread_local hipStream_t st[kMaxDev] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
    if (!st[dev]) {
        e = hipStreamCreateWithFlags(&st[dev], hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    *out = st[dev];
    return hipSuccess;
}

// records the calling thread's event `which` on stream st
static hipError_t record_event(int which, hipStream_t st, hipEvent_t* ev) {
    const hipError_t e = step_event(which, ev);
    return e != hipSuccess ? e : hipEventRecord(*ev, st);
}

struct TrainLayerWs {
    size_t w_qkv, b_qkv, w_proj, w_fc1, w_fc2;                    // operand-typed weight copies (b_qkv fp32 [3D])
    size_t x_mid, x_out, st1, st2, xn1, qkv, y, xn2, h, g;        // kept activations
    size_t dyo, dym, dh, dqkv;                                    // kept output gradients (operands of the weight gradients)
};
struct TrainWs {
    int M, T, Ke, ap;
    size_t noised, target, x0, xemb, stf, xf, pred, dpred, w_head, b_head, dw_cat, dw_head;
    size_t xemb32, wcat;                                            // fp32 feature matrix [M][Ke] and Wcat [D][Ke]: the embedding as one GEMM
    int Hp;                                                         // padded hidden width of the MLP head (0: linear head)
    size_t w_hid, b_hid, hz, ha, hdz, dw_hid, db_hid;
    size_t dx, dx0b, dxn, dy, ln_part;
    size_t ya, xa, dxa, dya;                                        // compact action rows of the last layer
    size_t fimg;                                                    // per-step fragment image of the weights (tail-block forward)
    size_t bimg;                                                    // ... of the transposed weights (data-gradient kernel)
    size_t b1slab;                                                  // [L][workgroups][4 D] fp32: FC1 bias sums per workgroup of that kernel
    size_t wslab; int w_splits, w_splits_panel; size_t wslab_floats;   // split weight-gradient launch: [splits][wslab_floats] partial outputs
    size_t det_part, det_floats;                                    // BESO_TRAIN_DETERMINISTIC: the slab of partial sums (one use at a time)
    TrainLayerWs layer[kMaxLayers];
    size_t total;
};

// (hp: the padded hidden width of the MLP action head, 0 with the linear head -- wider than 4 D when embed_dim < 32)
static size_t det_part_floats(size_t M, int D, int hp) {
    const size_t cols = 4 * (size_t)D > (size_t)hp ? 4 * (size_t)D : (size_t)hp;
    const size_t n = 2 * ((M + kTileMN - 1) / kTileMN) * cols;
    return n < 1024 ? 1024 : n;
}
static bool make_train_ws(const beso_config* c, int batch, int t, int precision, TrainWs* w) {
    memset(w, 0, sizeof(*w));
    const size_t e = precision == BESO_PREC_FP32 ? 4 : 2, f = 4;
    const int D = c->embed_dim, G = c->goal_seq_len;
    const int T = 1 + G + 2 * t;
    const size_t M = (size_t)batch * T;
    w->M = (int)M; w->T = T;
    w->Ke = round_up(c->obs_dim + c->act_dim + 4 + G + c->obs_seq_len + 1, 8);
    w->ap = round_up(c->act_dim, 16);
    size_t cur = 0;
    const size_t na = (size_t)batch * t * c->act_dim;
    w->noised = carve(cur, f * na); w->target = carve(cur, f * na);
    w->x0 = carve(cur, f * M * D); w->xemb = carve(cur, e * M * w->Ke);
    w->xemb32 = carve(cur, e == 4 ? 0 : f * M * w->Ke); w->wcat = carve(cur, f * (size_t)D * w->Ke);
    if (e == 4) w->xemb32 = w->xemb;                                // (fp32 mode: the operand-typed matrix IS the fp32 one)
    w->stf = carve(cur, f * M * 2); w->xf = carve(cur, e * M * D);
    w->pred = carve(cur, f * M * w->ap); w->dpred = carve(cur, e * M * w->ap);
    w->b_head = carve(cur, f * w->ap);
    w->dw_cat = carve(cur, f * (size_t)w->Ke * D);
    w->Hp = c->linear_output ? 0 : round_up(kHeadHidden, 8);
    {
        // linear head: w_head [ap][D]; MLP head: w_hid [Hp][D] (first layer) and w_head [ap][Hp] (second layer)
        const size_t Kh = w->Hp ? (size_t)w->Hp : (size_t)D, Ma = (size_t)batch * t;
        w->w_head = carve(cur, e * (size_t)w->ap * Kh); w->dw_head = carve(cur, f * (size_t)w->ap * Kh);
        w->w_hid = carve(cur, e * (size_t)w->Hp * D); w->b_hid = carve(cur, f * (size_t)(w->Hp + 8));
        w->dw_hid = carve(cur, f * (size_t)w->Hp * D); w->db_hid = carve(cur, f * (size_t)(w->Hp + 8));
        w->hz = carve(cur, e * Ma * w->Hp); w->ha = carve(cur, e * Ma * w->Hp); w->hdz = carve(cur, e * Ma * w->Hp);
    }
    // The partial sums of the deterministic step: the largest user is the FC1 bias gradient, one row of 4 D sums per 64 token
    // rows (two per 128-row tile) -- or the MLP head's hidden bias, Hp sums per row, where that is wider; the loss takes one
    // float per block of loss_kernel's grid (at most 1024).  The uses follow each other on the compute stream, each with its
    // second-stage launch behind it: one slab serves them all.
    w->det_floats = det_part_floats(M, D, w->Hp);
    w->det_part = carve(cur, f * w->det_floats);
    w->dx = carve(cur, f * M * D); w->dx0b = carve(cur, e * M * D); w->dxn = carve(cur, f * M * D);
    w->dy = carve(cur, e * M * D);
    {
        const size_t Ma = (size_t)batch * t;
        w->ya = carve(cur, e * Ma * D); w->xa = carve(cur, f * Ma * D);
        w->dxa = carve(cur, f * Ma * D); w->dya = carve(cur, e * Ma * D);
    }
    w->ln_part = carve(cur, f * (size_t)(2 * c->n_layers + 1) * ((M + 15) / 16) * 3 * D);     // LayerNorm backward block partials
    {
        Layout lay;
        const bool img = precision == BESO_PREC_BF16 && make_layout(c, BESO_PREC_BF16, &lay);
        const size_t tail_b = img ? fused_train_image_bytes(lay) : 0, whole_b = img ? fused_train_whole_image_bytes(lay) : 0;
        w->fimg = carve(cur, tail_b > whole_b ? tail_b : whole_b);
        w->bimg = carve(cur, img ? fused_train_dgrad_image_bytes(lay) : 0);
        w->b1slab = carve(cur, img && fused_train_dgrad_supported(lay)
                                     ? f * (size_t)c->n_layers * fused_train_dgrad_blocks((int)M) * 4 * D : 0);
    }
    {
        // row ranges of the grouped weight-gradient launch: enough workgroups for two per CU (small models: few output tiles,
        // long contractions); every output of the launch once per range
        const int tD = (D + kTileMN - 1) / kTileMN, tH = (4 * D + kTileMN - 1) / kTileMN;
        const int tiles = c->n_layers * (2 * tD * tH + 4 * tD * tD) + 4;
        const int cus = device_cus();
        int sp = (2 * cus + tiles - 1) / tiles;
        if (sp > 8) sp = 8;
        if ((size_t)sp > M / (4 * (128 / e))) sp = (int)(M / (4 * (128 / e)));      // (ranges of at least four stages)
        w->w_splits = sp < 2 ? 1 : sp;
        // ... and of the panel-owning tiles (one workgroup per CU, one round): as many row ranges as keep the launch within 256
        w->w_splits_panel = 1;
        if (const int W = wgrad_panel_w(D, e)) {
            (void)W;
            const int ptiles = c->n_layers * (2 * tH + 4 * tD) + 4;
            int psp = cus / ptiles;
            if (psp > 8) psp = 8;
            if ((size_t)psp > M / (4 * 64)) psp = (int)(M / (4 * 64));
            w->w_splits_panel = psp < 2 ? 1 : psp;
        }
        const int sp_max = w->w_splits > w->w_splits_panel ? w->w_splits : w->w_splits_panel;
        const size_t Kh = w->Hp ? (size_t)w->Hp : (size_t)D;
        w->wslab_floats = train_grad_floats(c) + (size_t)w->Ke * D + (size_t)w->ap * Kh + (size_t)w->Hp * D + 8 * (size_t)(6 * c->n_layers + 8);
        w->wslab = carve(cur, sp_max > 1 ? f * sp_max * w->wslab_floats : 0);
    }
    for (int l = 0; l < c->n_layers; ++l) {
        TrainLayerWs& y = w->layer[l];
        y.w_qkv = carve(cur, e * (size_t)3 * D * D); y.b_qkv = carve(cur, f * (size_t)3 * D);
        y.w_proj = carve(cur, e * (size_t)D * D);
        y.w_fc1 = carve(cur, e * (size_t)4 * D * D); y.w_fc2 = carve(cur, e * (size_t)4 * D * D);
        y.x_mid = carve(cur, f * M * D); y.x_out = carve(cur, f * M * D);
        y.st1 = carve(cur, f * M * 2); y.st2 = carve(cur, f * M * 2);
        y.xn1 = carve(cur, e * M * D); y.qkv = carve(cur, e * M * 3 * D); y.y = carve(cur, e * M * D);
        y.xn2 = carve(cur, e * M * D); y.h = carve(cur, e * M * 4 * D); y.g = carve(cur, e * M * 4 * D);
        y.dyo = carve(cur, e * M * D); y.dym = carve(cur, e * M * D); y.dh = carve(cur, e * M * 4 * D);
        y.dqkv = carve(cur, e * M * 3 * D);
    }
    w->total = cur;
    return true;
}

int train_validate(const beso_config* c, int batch, int t) {
    int st = validate_config(c);
    if (st != BESO_OK) return st;
    if (batch < 1 || t < 1 || t > c->obs_seq_len) return BESO_ERR_BAD_SHAPE;
    if (c->embed_dim % 8 != 0) return BESO_ERR_UNSUPPORTED;        // 16-byte operand chunks, float4 LayerNorm rows
    const int T = 1 + c->goal_seq_len + 2 * t;
    if (attn_lds_bytes(T, c->embed_dim / c->n_heads, true) > 150 * 1024) return BESO_ERR_UNSUPPORTED;
    // operands are addressed with 32-bit byte offsets (raw buffer loads): the widest one is [M][4D] in fp32
    if ((size_t)batch * T * 4 * c->embed_dim * sizeof(float) >= ((size_t)1 << 31)) return BESO_ERR_BAD_SHAPE;
    return BESO_OK;
}

size_t train_workspace_bytes(const beso_config* c, int batch, int t, int precision) {
    if (train_validate(c, batch, t) != BESO_OK) return 0;
    if (precision != BESO_PREC_BF16 && precision != BESO_PREC_FP32) return 0;
    TrainWs w;
    make_train_ws(c, batch, t, precision, &w);
    return w.total;
}

// The data-parallel exchange can start before the backward pass is over: the gradients of transformer layers
// train_early_layer(c) .. L-1 and of ln_f form one contiguous range of the flat gradient buffer and are completed first.
// Their weight gradients run as a grouped launch of their own, so the split is placed where that launch is one full
// round of workgroups (256 CUs x 2): as many upper layers as fit into 512 tiles.  (An even split of the kitchen model,
// 324 + 324 tiles, costs 0.15 ms per step -- two half-filled rounds; 432 + 216 costs nothing measurable.)
int train_early_layer(const beso_config* c) {
    const int L = c->n_layers;
    if (L < 2) return 0;
    const int td = (c->embed_dim + kTileMN - 1) / kTileMN, t4 = (4 * c->embed_dim + kTileMN - 1) / kTileMN;
    const int per_layer = 4 * td * td + 2 * t4 * td;               // q, k, v, proj + fc1 + fc2
    int n = 512 / per_layer;
    if (n < 1) n = 1;
    if (n > L - 1) n = L - 1;
    return L - n;
}
void train_early_range(const beso_config* c, size_t* begin, size_t* end) {
    const int l0 = train_early_layer(c);
    if (l0 < 1) { *begin = *end = 0; return; }                     // fewer than two layers: nothing is early
    const ModelParams m(c);
    *begin = m.layer[l0].ln1w.offset;
    *end = m.lnfb.offset + m.lnfb.count();
}
size_t train_grad_floats(const beso_config* c) { return validate_config(c) == BESO_OK ? ModelParams(c).floats : 0; }

// The tail-block forward pays off once its 96-token tiles are several rounds of workgroups (measured on MI355X, kitchen:
// 8192 samples = 939 tiles 16.57 vs 17.41 ms per step; 1024 samples = 118 tiles 3.43 vs 3.39 ms -- at under one round both
// forms are bound by a lone workgroup's latency): taken from kTailMinRows token rows on, unless the call's plan hint says
// otherwise (BESO_TRAIN_PLAN_PER_OP: never, BESO_TRAIN_PLAN_TILES: always -- the two forms write the same kept activations).
constexpr int kTailMinRows = 16000;       // kitchen: 3.39 = 3.40 ms at 1024 samples (11 k rows), 4.99 vs 5.37 at 2048, 8.61 vs 8.96 at 4096
static bool tail_forward_enabled(int rows, int flags) {
    if (flags & BESO_TRAIN_PLAN_PER_OP) return false;
    return (flags & BESO_TRAIN_PLAN_TILES) || rows >= kTailMinRows;
}

#define TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { *err = _e; *err_line = __LINE__; return BESO_ERR_HIP; } } while (0)
// ... for a BESO_* status (a fused.hip launch): BESO_OK, or the status the caller reports with the HIP error behind it
#define TRY_ST(call) do { const int st_ = (call); if (st_ != BESO_OK) { *err = hipGetLastError(); *err_line = __LINE__; return st_; } } while (0)
// ... and for a phase of the step, which has reported its error already
#define PHASE(call) do { const int st_ = (call); if (st_ != BESO_OK) return st_; } while (0)

// workgroups of a grid-stride kernel of 256 threads over n elements: at least one, at most `cap`
static int capped_grid(size_t n, size_t cap) { const size_t g = (n + 255) / 256; return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }
// nv: float4s per lane of a LayerNorm row (TrainPlan::nv); f(Int<nv>) launches that kernel instance
template <int N> using Int = std::integral_constant<int, N>;
template <typename F>
static void with_ln_vec(int nv, F&& f) { if (nv == 1) f(Int<1>{}); else if (nv == 2) f(Int<2>{}); else f(Int<4>{}); }
// the second stage of a deterministic sum: out[0 .. cols) = the rows of the slab `part` added in index order
static hipError_t part_reduce(const float* part, int nparts, int cols, float* out, hipStream_t s) {
    hipLaunchKernelGGL(part_reduce_kernel, dim3((cols + 63) / 64), dim3(256), 0, s, part, nparts, cols, out);
    return hipGetLastError();
}
// part != nullptr (BESO_TRAIN_DETERMINISTIC): a slab of part_floats floats for the row blocks' sums, added up by a second launch
template <typename E>
static hipError_t colsum(const E* a, int ld, int cols, int rows, float* out, hipStream_t s, float* part = nullptr, size_t part_floats = 0) {
    constexpr int EPC = 16 / (int)sizeof(E), rpb = 128;        // rpb: rows per block of the column sums
    const dim3 grid((cols + 64 * EPC - 1) / (64 * EPC), (rows + rpb - 1) / rpb);
    if (part) {
        if ((size_t)grid.y * cols > part_floats) return hipErrorInvalidValue;
        hipLaunchKernelGGL(colsum_part_kernel<E>, grid, dim3(256), 0, s, a, ld, rows, cols, part, rpb);
        return part_reduce(part, (int)grid.y, cols, out, s);
    }
    hipLaunchKernelGGL(colsum_kernel<E>, grid, dim3(256), 0, s, a, ld, rows, cols,
                       out, out, out, 1 << 30, rpb);
    return hipGetLastError();
}
template <int W>
static hipError_t launch_panel_group(const GTable& gt, int tiles, int splits, float* slab, size_t slab_floats, hipStream_t s) {
    return launch_lds<wgrad_panel_group_kernel<W>>(dim3(tiles * splits), dim3(kGT), wgrad_panel_lds(W), s, gt, tiles, splits, slab, slab_floats);
}

// The input-VJP mode of the step (beso_denoise_vjp): the same forward and chain of data gradients, seeded with the caller's
// cotangent instead of the loss, ending in the projection onto the action input.  No weight gradient, no reduction of partial
// sums, no gradient buffer: every gradient pointer of the chain is one workspace scratch slab (dw_cat: Ke D >= 8 D floats, unused
// in this mode) -- the kernels that write bias sums as side outputs write there.
struct VjpIo { const float* cot; float* denoised; float* x_grad; float* dot; };

// The arguments of one call of the step (train_loss_grad's; gflat: the scratch slab when vjp is set)
struct TrainCall {
    const beso_config* c; const float* const* p; float* gflat; int precision;
    const float *state, *action, *goal, *noise, *sigma; float* loss_out;
    int batch, t, flags; float embed_p, attn_p, resid_p, goal_p; uint32_t seed; float grad_scale;
    char* ws; hipStream_t s, early_stream, loss_stream; hipError_t* err; int* err_line; const VjpIo* vjp;
    float *state_grad, *goal_grad;                        // the gradients with respect to the state / goal inputs (nullptr: not asked for)
};

// ---- plan: which form every part of the step takes.  A pure host function of the call's shape and flags.
struct TrainPlan {
    Layout lay;                                           // bf16 layout of the fused kernels (valid when one of their forms is taken)
    bool use_whole, use_tail;                             // forward: one launch / tail blocks / (neither) per-op
    bool use_dgrad, use_mlp_bwd;                          // backward: transposed-formulation data gradients, ... as one launch per MLP
    int x16, panel_w;                                     // TrainWholeBufs::x_bf16; W of the panel weight-gradient tiles (0: 128 x 128 tiles)
    int nv;                                               // float4s per lane of a LayerNorm row
    bool attn_small, attn_mfma_bwd, wcat_side;
};
static TrainPlan make_train_plan(const beso_config* c, int flags, int M, int T, int t, float embed_p, float resid_p, size_t elem, bool fork) {
    TrainPlan pl;
    const int D = c->embed_dim, L = c->n_layers, hd = D / c->n_heads;
    const bool per_op = flags & BESO_TRAIN_PLAN_PER_OP;
    const bool lay = elem == 2 && make_layout(c, BESO_PREC_BF16, &pl.lay);
    // Which form the forward takes (decided here: its weight image is packed with the other per-step weight copies).
    // bf16, no dropout on the proj / MLP outputs, a shape with a fused tile kernel: everything of a layer behind its
    // attention and the LN1 + q/k/v of the next layer run as ONE launch (fused.hip: train_tail_kernel) on 96-token tiles
    // with the residual in registers -- six launches of the per-op forward below -- writing the same kept activations in
    // the same formats.  The last layer stays per-op (it continues on the compact action rows).
    pl.use_tail = lay && resid_p == 0.f && L >= 2 && L * 13 <= 96 && fused_train_supported(pl.lay) &&
                  fused_train_image_bytes(pl.lay) > 0 && tail_forward_enabled(M, flags);
    // ... and where the shape has the one-launch kernel (kitchen, block-push; bf16; round 5: with or without dropout on the
    // proj / MLP outputs), ALL layers run as ONE launch (fused.hip: train_fwd_kernel) -- 44 launches of the per-op forward at six
    // layers; the call's plan hints keep the other two forms reachable (BESO_TRAIN_PLAN_PER_OP, BESO_TRAIN_PLAN_TILES)
    pl.use_whole = lay && !(flags & (BESO_TRAIN_PLAN_PER_OP | BESO_TRAIN_PLAN_TILES)) && fused_train_whole_supported(pl.lay, T, t);
    // The data-gradient GEMMs of the backward pass in the transposed formulation (fused.hip: train_dgrad_kernel; bf16, the shapes
    // with the fused kernels); BESO_TRAIN_PLAN_PER_OP keeps the 128 x 128 tile kernel for them too
    // (they address the [M][D] ... [M][4 D] tensors with 32-bit byte offsets through buffer resources: M 4 D < 2^30 elements)
    pl.use_dgrad = lay && !per_op && fused_train_dgrad_supported(pl.lay) && (size_t)M * D < ((size_t)1 << 28);
    pl.use_mlp_bwd = pl.use_dgrad && fused_train_mlp_bwd_supported(pl.lay);
    // the one-launch forward keeps x_mid / x_out as bf16 when nothing but the fused LayerNorm-backward epilogues read them
    // (no residual dropout: with it the forward itself adds the residual back from the kept fp32 rows)
    pl.x16 = (pl.use_whole && pl.use_dgrad && pl.use_mlp_bwd && resid_p == 0.f) ? 1 : 0;
    // bf16, 128 < D <= 384: the grouped launch runs on panel-owning tiles (wgrad_panel_group_kernel); the per-op plan keeps the
    // 128 x 128 tiles
    pl.panel_w = per_op ? 0 : wgrad_panel_w(D, elem);
    pl.nv = D <= 256 ? 1 : (D <= 512 ? 2 : 4);
    pl.attn_small = T <= kTP && hd <= 64 && hd % 4 == 0;
    // (hd >= 8: row_chunk16 fetches a head's row in 16-byte chunks clamped to its last eight columns; a head of four dims
    //  has no such chunk inside its row and takes the VALU kernel)
    pl.attn_mfma_bwd = pl.attn_small && hd >= 8 && elem == 2 && !per_op;
    // (the embedding's concatenated weight -- parameters only -- is packed on the side stream too, first: the compute stream
    //  waits for it in front of the embedding GEMM, three small launches later)
    pl.wcat_side = fork && embed_p == 0.f;
    return pl;
}

// ---- LayerNorm backward partial sums: a slab [grid][3][D] per call (LayerNorm backward kernel, or the epilogue of a data
// gradient), reduced into the gradient tensors of the table by ln_reduce_kernel
struct LnPartials {
    LnRedTable tab;
    int calls = 0, reduced = 0, grid, D; float* base;     // grid: blocks of ln_bwd_kernel = the slab stride in block partials
    // the slab of the next call, which writes `blocks` block partials of (dgamma, dbeta, dbias)
    float* next(int blocks, float* dgam, float* dbet, float* dbias) {
        tab.nb[calls] = blocks; tab.c[calls] = LnRedCall{dgam, dbet, dbias};
        return base + (size_t)calls++ * grid * 3 * D;
    }
    hipError_t reduce(hipStream_t st) {                   // the calls since the last reduction, on stream st
        hipLaunchKernelGGL(ln_reduce_kernel, dim3((D + 63) / 64, 3, calls - reduced), dim3(256), 0, st, (const float*)base, tab, grid, D, reduced);
        reduced = calls;
        return hipGetLastError();
    }
};

// ---- The weight gradients are collected and run as one grouped launch after the chain of data gradients: every
// output gradient they need stays in its own buffer until then.
template <typename E>
struct WgradGroup {
    GTable gt;
    int tiles = 0; uint32_t floats = 0;                   // floats: of the collected problems in a range's slab
    bool off;                                             // input VJP: no weight gradient
    int panel_w, per_op, M, splits, splits_panel; float* slab; size_t slab_floats; hipStream_t s;
    float* det_part = nullptr; size_t det_floats = 0;     // BESO_TRAIN_DETERMINISTIC: the slab of colsum's partial sums
    int tiles_of(const GProb& q) const {
        if (panel_w) { int o; return wgrad_panel_tiles(q.Mo, q.No, panel_w, &o); }
        return q.nt_n * ((q.Mo + kTileMN - 1) / kTileMN);
    }
    static uint32_t floats_of(int Mo, int No, const float* bias) { return (uint32_t)round_up(Mo * No + (bias ? Mo : 0), 4); }
    // out[Mo][No] = A^T B over `rows` token rows.
    // bias: the gradient of the bias that goes with this weight = the column sums of A.  It rides along as a column of ones
    // behind B's last real column (free whenever No is not a multiple of the 128-column tile: every shipped shape -- on the
    // panel tiles too, whose n-wide tile holds column No unless No == 128 W); otherwise a colsum launch of its own.
    hipError_t add(const E* A, int lda, int Mo, const E* B, int ldb, int No, int rows, float* out, float* bias = nullptr) {
        if (off) return hipSuccess;
        if (gt.n == kMaxGroup) { hipError_t e = flush(); if (e != hipSuccess) return e; }
        if (bias && No % kTileMN == 0) {
            hipError_t e = colsum(A, lda, Mo, rows, bias, s, det_part, det_floats);
            if (e != hipSuccess) return e;
            bias = nullptr;
        }
        int orient = (No + kTileMN - 1) / kTileMN;        // (GProb::nt_n: tiles along n, or the panel tiles' orientation)
        const int nt = panel_w ? wgrad_panel_tiles(Mo, No, panel_w, &orient) : orient * ((Mo + kTileMN - 1) / kTileMN);
        gt.p[gt.n++] = GProb{A, B, out, bias, lda, ldb, Mo, No, tiles, orient, rows, floats};
        tiles += nt; floats += floats_of(Mo, No, bias);
        return hipSuccess;
    }
    // Order of the problems inside a launch: each XCD takes a contiguous run of the launch's tiles (xcd_tile), and a problem
    // whose tiles straddle two runs has its operand panels fetched into two L2s.  Units (problems sharing their B operand:
    // q | k | v of a layer) are packed into eight bins of ceil(tiles / 8), largest first, and emitted bin by bin -- kitchen:
    // six bins {FC2, FC1, out-projection} of 81 tiles and two of three q|k|v triples, against runs of 81 / 82.
    void arrange() {
        const int n = gt.n;
        if (n < 3 || per_op) return;
        int ufirst[kMaxGroup], ucnt[kMaxGroup], utiles[kMaxGroup], order[kMaxGroup], bin_of[kMaxGroup], nu = 0;
        for (int i = 0; i < n; ++i) {
            if (i > 0 && gt.p[i].B == gt.p[i - 1].B) { ++ucnt[nu - 1]; utiles[nu - 1] += tiles_of(gt.p[i]); }
            else { ufirst[nu] = i; ucnt[nu] = 1; utiles[nu] = tiles_of(gt.p[i]); ++nu; }
        }
        for (int u = 0; u < nu; ++u) {                    // (stable insertion sort, largest first)
            int j = u;
            while (j > 0 && utiles[order[j - 1]] < utiles[u]) { order[j] = order[j - 1]; --j; }
            order[j] = u;
        }
        const int cap = (tiles + 7) / 8;
        int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < nu; ++k) {
            const int u = order[k];
            int b = -1;
            for (int x = 0; x < 8 && b < 0; ++x) if (load[x] + utiles[u] <= cap) b = x;
            if (b < 0) { b = 0; for (int x = 1; x < 8; ++x) if (load[x] < load[b]) b = x; }
            bin_of[u] = b; load[b] += utiles[u];
        }
        GTable out;
        out.n = 0; int tile0 = 0; uint32_t float0 = 0;
        for (int b = 0; b < 8; ++b)
            for (int k = 0; k < nu; ++k) {
                const int u = order[k];
                if (bin_of[u] != b) continue;
                for (int i = ufirst[u]; i < ufirst[u] + ucnt[u]; ++i) {
                    GProb q = gt.p[i];
                    q.tile_begin = tile0; q.slab_off = float0;
                    tile0 += tiles_of(q);
                    float0 += floats_of(q.Mo, q.No, q.bias);
                    out.p[out.n++] = q;
                }
            }
        gt = out;
    }
    // launches the collected weight gradients behind everything issued on `s` so far.  (Measured and rejected, round 2: the
    // grouped launch of a layer on a side stream under the data gradients of the layers in front of it -- 3.63 vs 3.39 ms per
    // 1024-sample kitchen step, the two streams evict each other's operands from L2 / MALL.)
    hipError_t flush() {
        if (gt.n == 0) return hipSuccess;
        arrange();
        // row ranges into slabs of their own (make_train_ws), added up by wgrad_reduce_kernel
        const int want = panel_w ? splits_panel : splits, sp = (want > 1 && floats <= slab_floats) ? want : 1;
        if (panel_w) {
            const hipError_t e = panel_w == 2 ? launch_panel_group<2>(gt, tiles, sp, slab, slab_floats, s)
                                              : launch_panel_group<3>(gt, tiles, sp, slab, slab_floats, s);
            if (e != hipSuccess) return e;
        } else {
            // Long contractions (M >= ~18 k token rows) run as one launch per ROW WINDOW of ~12 k rows, window w > 0 adding to the
            // outputs of the windows before it (stream order: deterministic).  The tiles of a weight gradient share operand panels
            // through an XCD's L2, but the sharers drift apart over a long contraction -- FETCH_SIZE 24 GB for 6.2 GB of operands at
            // 8192 kitchen samples (90 k rows) against 1.9 GB for 0.78 GB at 1024 -- and a launch boundary lines them up again:
            // 14.6 -> 14.2 ms per 8192-sample step with 8 windows (4: 14.3, 16: 14.25, 32: 14.6); nothing to gain at 11 k rows.
            int n_win = (sp > 1 || per_op) ? 1 : (M + 6144) / 12288;
            n_win = n_win < 1 ? 1 : (n_win > 16 ? 16 : n_win);
            for (int win = 0; win < n_win; ++win)
                hipLaunchKernelGGL(tgemm_wgrad_group_kernel<E>, dim3(tiles * sp), dim3(kGT), 0, s, gt, tiles, sp, slab, slab_floats, win, n_win);
        }
        if (sp > 1)
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((floats + 1023) / 1024), dim3(256), 0, s, gt, (const float*)slab, slab_floats, sp, floats);
        gt.n = 0; tiles = 0; floats = 0;
        return hipGetLastError();
    }
};

// ---- the step: its phases in the order run() calls them.  A phase returns BESO_OK or a status it has reported in *err / *err_line.
template <typename E>
struct TrainStep : TrainCall {
    const TrainWs& w;
    const ModelParams& par;                               // the call's parameters and their gradients (VJP: all on the scratch slab)
    const int D = c->embed_dim, H = c->n_heads, hd = D / H, L = c->n_layers, G = c->goal_seq_len, obs = c->obs_dim, act = c->act_dim;
    const int seq = G + c->obs_seq_len + 1, M = w.M, T = w.T, Ke = w.Ke, ap = w.ap, D3 = 3 * D, D4 = 4 * D;
    const int Ma = batch * t;                             // compact action rows (last layer's projection, MLP, ln_f, head)
    const int Hh = kHeadHidden, Hp = w.Hp, mlp_head = !c->linear_output;
    const float scale = 1.0f / sqrtf((float)hd);
    const float attn_ik = attn_p > 0.f ? 1.0f / (1.0f - attn_p) : 1.f, resid_ik = resid_p > 0.f ? 1.0f / (1.0f - resid_p) : 1.f;
    const bool fork = loss_stream != nullptr;             // the weight copies run on the caller's second stream: ps
    const hipStream_t ps = fork ? loss_stream : s;
    const TrainPlan plan = make_train_plan(c, flags, M, T, t, embed_p, resid_p, sizeof(E), fork);
    const LayerParams* const lp = par.layer;
    // BESO_TRAIN_DETERMINISTIC: the three sums the step otherwise forms with atomics (column-sum epilogues, colsum_kernel, the loss)
    // go through the slab w.det_part and a second launch each
    const bool det = flags & BESO_TRAIN_DETERMINISTIC;
    hipEvent_t ev_join = nullptr, ev_copies = nullptr, ev_wcat = nullptr;      // recorded by copy_weights(), waited for by the forward
    static constexpr int kRpw = 4;                        // rows per wave of the LayerNorm backward
    LnPartials ln; WgradGroup<E> wg;
    // FC1 bias gradients of the transposed-formulation data-gradient kernel: per-workgroup sums in a slab per layer, added up
    // (assigned, not accumulated) where the LayerNorm partial sums are
    const float* b1_slabs[kMaxLayers]; float* b1_outs[kMaxLayers]; int b1_blocks[kMaxLayers]; int b1_n = 0;
    TrainStep(const TrainCall& call, const TrainWs& ws_, const ModelParams& par_) : TrainCall(call), w(ws_), par(par_) {
        ln.base = F(w.ln_part); ln.grid = (M + 4 * kRpw - 1) / (4 * kRpw); ln.D = D;
        wg.gt.n = 0; wg.off = vjp != nullptr; wg.panel_w = plan.panel_w; wg.per_op = flags & BESO_TRAIN_PLAN_PER_OP; wg.M = M; wg.s = s;
        wg.splits = w.w_splits; wg.splits_panel = w.w_splits_panel; wg.slab = F(w.wslab); wg.slab_floats = w.wslab_floats;
        if (det) { wg.det_part = F(w.det_part); wg.det_floats = w.det_floats; }
    }
    float* F(size_t off) const { return (float*)(ws + off); }
    E* P(size_t off) const { return (E*)(ws + off); }
    const float* layer_in(int l) const { return l == 0 ? F(w.x0) : F(w.layer[l - 1].x_out); }
    int run() {
        PHASE(copy_weights());
        PHASE(embed());
        if (plan.use_whole) PHASE(forward_whole());
        else for (int l = 0; l < L; ++l) PHASE(forward_layer(l));
        PHASE(head_and_seed());
        PHASE(backward_head());
        for (int l = L - 1; l >= 0; --l) {
            PHASE(backward_layer(l));
            if (early_stream && l == train_early_layer(c) && l > 0) PHASE(early_flush());
        }
        return finish();
    }
    // ---- weight copies
    // The per-step weight copies depend on the parameters only, the embedding on the batch only: when the caller handed over a
    // second stream (loss_stream: idle at this point), the copies run THERE beside the gradient buffer's memset, the
    // preconditioning and the embedding on `s` -- two short chains of small kernels side by side instead of one after the
    // other (round 4: -50 us of a 2.5 ms step).  The forward waits for both.
    int copy_weights() {
        if (fork) {
            hipEvent_t ev_fork = nullptr;
            TRY(record_event(kEvFork, s, &ev_fork));         // (behind the optimizer step that wrote the parameters)
            TRY(hipStreamWaitEvent(ps, ev_fork, 0));
        }
        // (loss_out and the padded head bias: prep_kernel.  Beside the store-bound forward the 37.5 MB memset measured slower; round 6:
        //  in FRONT of the forward image's pack on the side stream -- the forward waits for that stream anyway (ev_join), and the
        //  compute stream's chain of small launches in front of the forward is 9 us shorter)
        if (plan.wcat_side) {
            TRY(pack_wcat(ps));
            TRY(record_event(kEvWcat, ps, &ev_wcat));
        }
        if (!vjp) TRY(hipMemsetAsync(gflat, 0, sizeof(float) * par.floats, ps));
        // (first what the forward launch needs -- its fragment image --, then the plain copies the backward pass reads)
        if (plan.use_whole) TRY_ST(fused_train_whole_pack(plan.lay, par, ws + w.fimg, ps));
        else if (plan.use_tail) TRY_ST(fused_train_pack(plan.lay, par, ws + w.fimg, ps));
        if (fork) TRY(record_event(kEvJoin, ps, &ev_join));
        if (plan.use_dgrad) TRY_ST(fused_train_dgrad_pack(plan.lay, par, ws + w.bimg, ps));
        // (nobody reads the operand-typed copies when the forward is the one-launch kernel and the data gradients take the transposed weights)
        if (!(plan.use_whole && plan.use_dgrad)) TRY(pack_layer_weights());
        if (mlp_head) {
            TRY(launch_pack_matrix(par.h0w.p, Hh, D, ws + w.w_hid, Hp, D, precision, ps));          // zero rows Hh..Hp
            TRY(hipMemsetAsync(ws + w.b_hid, 0, sizeof(float) * Hp, ps));
            TRY(hipMemcpyAsync(ws + w.b_hid, par.h0b.p, sizeof(float) * Hh, hipMemcpyDeviceToDevice, ps));
            TRY(hipMemsetAsync(ws + w.db_hid, 0, sizeof(float) * Hp, ps));
            TRY(launch_pack_matrix(par.hw.p, act, Hh, ws + w.w_head, ap, Hp, precision, ps));       // zero columns Hh..Hp, rows act..ap
        } else TRY(launch_pack_matrix(par.hw.p, act, D, ws + w.w_head, ap, D, precision, ps));
        if (fork) TRY(record_event(kEvCopies, ps, &ev_copies));
        return BESO_OK;
    }
    hipError_t pack_wcat(hipStream_t st) {
        hipLaunchKernelGGL(wcat_pack_kernel, dim3((D * Ke + 255) / 256), dim3(256), 0, st, par.pos.p, par.tokw.p, par.tokb.p, par.sigw.p,
                           par.sigb.p, par.actw.p, par.actb.p, F(w.wcat), D, obs, act, seq, Ke);
        return hipGetLastError();
    }
    // operand-typed weight copies (fused q|k|v rows as in the inference image): one launch for up to seven layers
    hipError_t pack_layer_weights() {
        PackTable tab;
        tab.n = 0; uint32_t total4 = 0;
        auto flush = [&]() -> hipError_t {
            if (tab.n == 0) return hipSuccess;
            hipLaunchKernelGGL(pack_table_kernel<E>, dim3(capped_grid(total4, 4096)), dim3(256), 0, ps, tab, total4);
            tab.n = 0; total4 = 0;
            return hipGetLastError();
        };
        auto seg = [&](const float* src, void* dst, uint32_t n4, uint32_t f32) { tab.seg[tab.n++] = PackSeg{src, dst, total4, f32}; total4 += n4; };
        for (int l = 0; l < L; ++l) {
            const TrainLayerWs& y = w.layer[l];
            const size_t e = sizeof(E);
            const uint32_t dd4 = (uint32_t)((size_t)D * D / 4), d4 = (uint32_t)(D / 4);
            if (tab.n + 9 > kPackSegs) { const hipError_t st = flush(); if (st != hipSuccess) return st; }
            seg(lp[l].qw.p, ws + y.w_qkv, dd4, 0);
            seg(lp[l].kw.p, ws + y.w_qkv + e * (size_t)D * D, dd4, 0);
            seg(lp[l].vw.p, ws + y.w_qkv + e * (size_t)2 * D * D, dd4, 0);
            seg(lp[l].pw.p, ws + y.w_proj, dd4, 0);
            seg(lp[l].f1w.p, ws + y.w_fc1, 4 * dd4, 0);
            seg(lp[l].f2w.p, ws + y.w_fc2, 4 * dd4, 0);
            seg(lp[l].qb.p, ws + y.b_qkv, d4, 1);
            seg(lp[l].kb.p, ws + y.b_qkv + sizeof(float) * D, d4, 1);
            seg(lp[l].vb.p, ws + y.b_qkv + sizeof(float) * 2 * D, d4, 1);
        }
        return flush();
    }
    // ---- forward
    int embed() {
        // (VJP: the caller's x IS the noised action -- no elements to prepare, only the loss slot and the padded head bias)
        const size_t n = vjp ? 0 : (size_t)batch * t * act;
        hipLaunchKernelGGL(prep_kernel, dim3(capped_grid(n, 2048)), dim3(256), 0, s, action, noise, sigma, F(w.noised), F(w.target),
                           t * act, n, c->sigma_data, loss_out, F(w.b_head), par.hb.p, act, ap);
        TRY(hipGetLastError());
        if (embed_p == 0.f) {
            // the embedding as one exact-fp32 GEMM over the feature matrix (train_feat_kernel)
            if (!plan.wcat_side) TRY(pack_wcat(s));
            hipLaunchKernelGGL(train_feat_kernel<E>, dim3(capped_grid((size_t)M * Ke, 4096)), dim3(256), 0, s, state, vjp ? action : (const float*)F(w.noised),
                               goal, sigma, P(w.xemb), F(w.xemb32), M, t, T, G, obs, act, Ke, c->sigma_data, goal_p, seed);
            TRY(hipGetLastError());
            if (plan.wcat_side) TRY(hipStreamWaitEvent(s, ev_wcat, 0));
            TRY((tgemm<float, false, false>(F(w.xemb32), Ke, F(w.wcat), Ke, M, D, Ke, 1, EpiStore<float>{F(w.x0), nullptr, nullptr, D}, s)));
        } else {
            const int threads = D >= 256 ? 256 : round_up(D, 64);
            hipLaunchKernelGGL(train_embed_kernel<E>, dim3(M), dim3(threads), sizeof(float) * (size_t)(obs > act ? obs : act), s,
                               state, (const float*)F(w.noised), goal, sigma, par.pos.p, par.tokw.p, par.tokb.p, par.sigw.p, par.sigb.p,
                               par.actw.p, par.actb.p, F(w.x0), P(w.xemb), t, T, G, D, obs, act, Ke, c->sigma_data, embed_p, goal_p, seed);
            TRY(hipGetLastError());
        }
        return BESO_OK;
    }
    hipError_t ln_fwd(const float* x, const Param& gamma, const Param& beta, E* out, float* st, int rows) {
        with_ln_vec(plan.nv, [&](auto nv) {
            hipLaunchKernelGGL((ln_fwd_kernel<E, decltype(nv)::value>), dim3((rows + 3) / 4), dim3(256), 0, s, x, gamma.p, beta.p, out, st, rows, D);
        });
        return hipGetLastError();
    }
    // attention of layer l, forward (qkv -> y) or backward (qkv, dy -> dqkv)
    template <bool BWD>
    hipError_t launch_attention(int l) {
        const TrainLayerWs& y = w.layer[l];
        constexpr size_t kAttnLdsAttr = 150 * 1024;  // (the ceiling train_validate admits: the size changes with the window, the attribute need not)
        const uint32_t site = drop_site_attn(l);
        if (BWD && plan.attn_mfma_bwd) {
            const int n_pairs = batch * H;
            hipLaunchKernelGGL(attn_mfma_bwd_kernel, dim3((n_pairs + 3) / 4), dim3(256), 0, s, (const uint16_t*)P(y.qkv),
                               (const uint16_t*)P(w.dy), (uint16_t*)P(y.dqkv), n_pairs, T, D, H, hd, scale, attn_p, attn_ik, seed, site);
        } else if (plan.attn_small) {
            auto small = [&](auto tt) {
                hipLaunchKernelGGL((attn_small_kernel<E, BWD, decltype(tt)::value>), dim3(batch * H), dim3(64), 0, s, (const E*)P(y.qkv),
                                   BWD ? (const E*)P(w.dy) : (const E*)nullptr, BWD ? P(y.dqkv) : P(y.y), T, D, H, hd, scale, attn_p, attn_ik, seed, site);
            };
            if (T <= 8) small(Int<8>{}); else if (T <= 12) small(Int<12>{}); else small(Int<16>{});
        } else if (BWD)
            return launch_lds_attr<attn_bwd_kernel<E>>(kAttnLdsAttr, dim3(batch * H), dim3(64), attn_lds_bytes(T, hd, true), s, (const E*)P(y.qkv),
                                                       (const E*)P(w.dy), P(y.dqkv), T, D, H, hd, scale, attn_p, attn_ik, seed, site);
        else
            return launch_lds_attr<attn_fwd_kernel<E>>(kAttnLdsAttr, dim3(batch * H), dim3(64), attn_lds_bytes(T, hd, false), s, (const E*)P(y.qkv),
                                                       P(y.y), T, D, H, hd, scale, attn_p, attn_ik, seed, site);
        return hipGetLastError();
    }
    int forward_whole() {
        if (fork) TRY(hipStreamWaitEvent(s, ev_join, 0));             // the forward's weight image is in place
        const TrainLayerWs& y0 = w.layer[0];
        const size_t stride = L > 1 ? w.layer[1].x_mid - y0.x_mid : 0;
        const TrainWholeBufs b{F(w.x0), ws, y0.x_mid, y0.x_out, y0.st1, y0.st2, y0.xn1, y0.qkv, y0.y, y0.xn2, y0.h, y0.g,
                               stride, w.ya, t, attn_p, seed, resid_p, plan.x16};
        profile_begin(BESO_SITE_FUSED_LAYER, s);
        const int st = fused_train_whole(plan.lay, ws + w.fimg, batch, T, b, s);
        profile_end(BESO_SITE_FUSED_LAYER, s);
        TRY_ST(st);
        if (fork) TRY(hipStreamWaitEvent(s, ev_copies, 0));           // head weights and the backward's copies: ready long since
        return BESO_OK;
    }
    // layer l through the per-op kernels, or (use_tail) everything behind its attention as one tail-block launch
    int forward_layer(int l) {
        if (fork && l == 0) {
            TRY(hipStreamWaitEvent(s, ev_join, 0));                   // the forward's weight image is in place
            TRY(hipStreamWaitEvent(s, ev_copies, 0));                 // (per-op / tile forward: the plain copies too)
        }
        const TrainLayerWs& y = w.layer[l];
        const float* x_in = layer_in(l);
        const bool last = l == L - 1;
        if (!(plan.use_tail && l > 0)) {      // (behind a tail block these arrive from the previous layer's launch)
            TRY(ln_fwd(x_in, lp[l].ln1w, lp[l].ln1b, P(y.xn1), F(y.st1), M));
            TRY((tgemm<E, false, false>(P(y.xn1), D, P(y.w_qkv), D, M, D3, D, 1, EpiStore<E>{nullptr, P(y.qkv), F(y.b_qkv), D3}, s)));
        }
        TRY(launch_attention<false>(l));
        if (plan.use_tail && !last) {
            const TrainLayerWs& nx = w.layer[l + 1];
            TRY_ST(fused_train_tail(plan.lay, ws + w.fimg, l, M, x_in, P(y.y), D, F(y.x_mid), F(y.x_out), F(y.st2), P(y.xn2),
                                    P(y.h), P(y.g), F(nx.st1), P(nx.xn1), P(nx.qkv), s));
            return BESO_OK;
        }
        // the last layer continues on the compact action rows only (its buffers hold Ma rows from here on)
        const int rows = last ? Ma : M;
        const E* y_in = P(y.y);
        const float* res_in = x_in;
        if (last) {
            const int grid = capped_grid((size_t)Ma * (D / 4), 4096);
            hipLaunchKernelGGL(gather_rows_kernel<E>, dim3(grid), dim3(256), 0, s, (const E*)P(y.y), P(w.ya), Ma, t, T, G, D);
            hipLaunchKernelGGL(gather_rows_kernel<float>, dim3(grid), dim3(256), 0, s, x_in, F(w.xa), Ma, t, T, G, D);
            TRY(hipGetLastError());
            y_in = P(w.ya); res_in = F(w.xa);
        }
        TRY((tgemm<E, false, false>(y_in, D, P(y.w_proj), D, rows, D, D, 1,
                                    EpiResid{res_in, F(y.x_mid), lp[l].pb.p, D, resid_p, resid_ik, seed, drop_site_proj(l)}, s)));
        TRY(ln_fwd(F(y.x_mid), lp[l].ln2w, lp[l].ln2b, P(y.xn2), F(y.st2), rows));
        TRY((tgemm<E, false, false>(P(y.xn2), D, P(y.w_fc1), D, rows, D4, D, 1, EpiFc1<E>{P(y.h), P(y.g), lp[l].f1b.p, D4}, s)));
        TRY((tgemm<E, false, false>(P(y.g), D4, P(y.w_fc2), D4, rows, D, D4, 1,
                                    EpiResid{(const float*)F(y.x_mid), F(y.x_out), lp[l].f2b.p, D, resid_p, resid_ik, seed, drop_site_mlp(l)}, s)));
        return BESO_OK;
    }
    // ln_f and the action head on the compact rows, then the loss and its gradient dpred -- or the VJP's seed
    int head_and_seed() {
        TRY(ln_fwd(F(w.layer[L - 1].x_out), par.lnfw, par.lnfb, P(w.xf), F(w.stf), Ma));
        if (mlp_head) {
            TRY((tgemm<E, false, false>(P(w.xf), D, P(w.w_hid), D, Ma, Hp, D, 1, EpiSilu<E>{P(w.hz), P(w.ha), F(w.b_hid), Hp}, s)));
            TRY((tgemm<E, false, false>(P(w.ha), Hp, P(w.w_head), Hp, Ma, ap, Hp, 1, EpiStore<E>{F(w.pred), nullptr, F(w.b_head), ap}, s)));
        } else TRY((tgemm<E, false, false>(P(w.xf), D, P(w.w_head), D, Ma, ap, D, 1, EpiStore<E>{F(w.pred), nullptr, F(w.b_head), ap}, s)));
        const int grid = capped_grid((size_t)Ma * ap, 1024);
        if (vjp) {
            hipLaunchKernelGGL(vjp_seed_kernel<E>, dim3(grid), dim3(256), 0, s, (const float*)F(w.pred), action, sigma, vjp->cot,
                               P(w.dpred), vjp->denoised, Ma, act, ap, t, c->sigma_data);
            TRY(hipGetLastError());
            return BESO_OK;
        }
        const int last_only = flags & BESO_TRAIN_LAST_ACTION_ONLY;
        const float inv_count = 1.0f / (float)((size_t)batch * (last_only ? 1 : t) * act);
        if (det) {
            // one share per block, added up in index order -- in FRONT of the event below: the loss is final where loss_stream is released
            if ((size_t)grid > w.det_floats) { *err = hipErrorInvalidValue; *err_line = __LINE__; return BESO_ERR_HIP; }
            hipLaunchKernelGGL(loss_part_kernel<E>, dim3(grid), dim3(256), 0, s, (const float*)F(w.pred), (const float*)F(w.target), P(w.dpred),
                               F(w.det_part), Ma, act, ap, inv_count, grad_scale, t, last_only);
            hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)F(w.det_part), grid, loss_out);
        } else
            hipLaunchKernelGGL(loss_kernel<E>, dim3(grid), dim3(256), 0, s, (const float*)F(w.pred), (const float*)F(w.target), P(w.dpred),
                               loss_out, Ma, act, ap, inv_count, grad_scale, t, last_only);
        TRY(hipGetLastError());
        if (loss_stream) {
            // the loss is final here, long before the step is: a stream of the caller's is ordered behind this point, so that
            // reading the loss there (beso_agent.py:248 `loss.item()`) does not wait for the backward pass
            hipEvent_t ev_loss = nullptr;
            TRY(record_event(kEvLoss, s, &ev_loss));
            TRY(hipStreamWaitEvent(loss_stream, ev_loss, 0));
        }
        return BESO_OK;
    }
    // ---- backward
    // rows of the slab a kColPart epilogue writes for a GEMM over `rows` token rows (one per 64-row wave of every 128-row tile)
    static int det_rows(int rows) { return 2 * ((rows + kTileMN - 1) / kTileMN); }
    hipError_t det_rows_fit(int rows, int cols) const { return (size_t)det_rows(rows) * cols <= w.det_floats ? hipSuccess : hipErrorInvalidValue; }
    // (every call launches ln.grid blocks so that the partial slabs have one shape; blocks past `rows` write zeros)
    hipError_t ln_bwd(const float* x, size_t st, const float* gamma, const float* dres_in, float* dres_out, E* dxb, int rows,
                      float* dgam, float* dbet, float* dbias, float p_site, uint32_t site, int skip_mod = 0) {
        float* part = ln.next(ln.grid, dgam, dbet, dbias);
        with_ln_vec(plan.nv, [&](auto nv) {
            hipLaunchKernelGGL((ln_bwd_kernel<E, decltype(nv)::value>), dim3(ln.grid), dim3(256), 0, s, (const float*)F(w.dxn), x, (const float*)F(st),
                               gamma, dres_in, dres_out, dxb, part, rows, D, kRpw, p_site, p_site > 0.f ? 1.0f / (1.0f - p_site) : 1.f, seed, site, skip_mod);
        });
        return hipGetLastError();
    }
    // the arguments of the same LayerNorm backward as the epilogue of the data gradient in front of it (fused_train_dgrad's which = 0:
    // q|k|v, 2: FC1); dxn is never written (dropout at the site: the same (row, feature) hash, evaluated in the epilogue).
    TrainLnBwd ln_epilogue(int rows, const float* x, size_t st, const float* gamma, float* dres, E* dxb, float* dgam, float* dbet,
                           float* dbias, float p_site, uint32_t site, int skip_mod, int x_is_bf16) {
        float* part = ln.next(fused_train_dgrad_blocks(rows), dgam, dbet, dbias);
        return TrainLnBwd{x, (const float*)F(st), gamma, dres, dres, dxb, part, p_site, seed, site, skip_mod, x_is_bf16};
    }
    // head (compact rows): dW = dpred^T xf (the act real rows of dpred's ap columns, straight into the gradient tensor),
    // db = its column sums, dxf = dpred W; then ln_f
    int backward_head() {
        if (mlp_head) {
            if (!vjp) TRY(colsum(P(w.dpred), ap, act, Ma, par.hb.g, s, det ? F(w.det_part) : nullptr, w.det_floats));
            // second layer: dW1 = dpred^T a, da = dpred W1 -> dz = da * SiLU'(z) (+ its column sums = db0); first layer:
            // dW0 = dz^T xf, dxf = dz W0.  Padded rows / columns are zeros all the way.
            TRY(wg.add(P(w.dpred), ap, ap, P(w.ha), Hp, Hp, Ma, F(w.dw_head)));
            if (det) {
                TRY(det_rows_fit(Ma, Hp));
                TRY((tgemm<E, false, true>(P(w.dpred), ap, P(w.w_head), Hp, Ma, Hp, ap, 1, EpiSiluBwdPart<E>{{P(w.hz), P(w.hdz), F(w.det_part), Hp}}, s)));
                TRY(part_reduce(F(w.det_part), det_rows(Ma), Hp, F(w.db_hid), s));
            } else
                TRY((tgemm<E, false, true>(P(w.dpred), ap, P(w.w_head), Hp, Ma, Hp, ap, 1, EpiSiluBwd<E>{P(w.hz), P(w.hdz), F(w.db_hid), Hp}, s)));
            TRY(wg.add(P(w.hdz), Hp, Hp, P(w.xf), D, D, Ma, F(w.dw_hid)));
            TRY((tgemm<E, false, true>(P(w.hdz), Hp, P(w.w_hid), D, Ma, D, Hp, 1, EpiStore<E>{F(w.dxn), nullptr, nullptr, D}, s)));
        } else {
            TRY(wg.add(P(w.dpred), ap, act, P(w.xf), D, D, Ma, par.hw.g, par.hb.g));
            TRY((tgemm<E, false, true>(P(w.dpred), ap, P(w.w_head), D, Ma, D, ap, 1, EpiStore<E>{F(w.dxn), nullptr, nullptr, D}, s)));
        }
        TRY(ln_bwd(F(w.layer[L - 1].x_out), w.stf, par.lnfw.p, nullptr, F(w.dxa), P(w.layer[L - 1].dyo), Ma, par.lnfw.g, par.lnfb.g,
                   lp[L - 1].f2b.g, resid_p, drop_site_mlp(L - 1)));
        return BESO_OK;
    }
    // (Measured and rejected, round 2: the chain of data gradients between two attention backwards as ONE tile kernel, the mirror
    // image of the tail-block forward -- parity-green, 209 us per launch against 164 us + gaps for the eight per-op launches it
    // replaces: 3.60 vs 3.43 ms per 1024-sample step.  DESIGN.md section 7.)
    int backward_layer(int l) {
        const TrainLayerWs& y = w.layer[l];
        const float* x_in = layer_in(l);
        const bool last = l == L - 1, first = l == 0;
        const int rows = last ? Ma : M;
        float* dres = last ? F(w.dxa) : F(w.dx);          // residual gradient of this layer's second half
        // FC2: dW2 = dyo^T g, dh = (dyo W2) * GELU'(h)
        TRY(wg.add(P(y.dyo), D, D, P(y.g), D4, D4, rows, lp[l].f2w.g));
        E* dy_out = last ? P(w.dya) : P(w.dy);
        const uint32_t site2 = drop_site_proj(l);        // dropout site behind LayerNorm-2's branch (the out-projection)
        float* slab = F(w.b1slab) + (size_t)l * fused_train_dgrad_blocks(M) * D4;       // FC1 bias sums per workgroup (use_dgrad)
        if (plan.use_dgrad) {
            b1_slabs[b1_n] = slab; b1_outs[b1_n] = lp[l].f1b.g; b1_blocks[b1_n] = fused_train_dgrad_blocks(rows); ++b1_n;
            const TrainLnBwd e = ln_epilogue(rows, F(y.x_mid), y.st2, lp[l].ln2w.p, dres, P(y.dym), lp[l].ln2w.g, lp[l].ln2b.g,
                                             lp[l].pb.g, resid_p, site2, 0, plan.x16);
            if (plan.use_mlp_bwd) {
                // FC2 + GELU' -> FC1 -> LayerNorm-2 backward -> out-projection: one launch, dh and dym stay in LDS between the GEMMs
                TRY_ST(fused_train_mlp_bwd(plan.lay, ws + w.bimg, l, rows, P(y.dyo), P(y.h), P(y.dh), slab, dy_out, e, s));
            } else {
                // the same chain as three launches (shapes without the one-kernel form)
                TRY_ST(fused_train_dgrad(plan.lay, ws + w.bimg, l, 3, rows, P(y.dyo), nullptr, nullptr, P(y.h), P(y.dh), slab, s));
                TRY_ST(fused_train_dgrad(plan.lay, ws + w.bimg, l, 2, rows, P(y.dh), nullptr, nullptr, nullptr, nullptr, nullptr, s, &e));
                TRY_ST(fused_train_dgrad(plan.lay, ws + w.bimg, l, 1, rows, P(y.dym), nullptr, dy_out, nullptr, nullptr, nullptr, s));
            }
        } else {
            // per-op: dh = (dyo W2) * GELU'(h) (+ db1), dxn2 = dh W1, LayerNorm-2 backward, dy = dym Wp
            if (det) {
                TRY(det_rows_fit(rows, D4));
                TRY((tgemm<E, false, true>(P(y.dyo), D, P(y.w_fc2), D4, rows, D4, D, 1, EpiGeluBwdPart<E>{{P(y.h), P(y.dh), F(w.det_part), D4}}, s)));
                TRY(part_reduce(F(w.det_part), det_rows(rows), D4, lp[l].f1b.g, s));
            } else
                TRY((tgemm<E, false, true>(P(y.dyo), D, P(y.w_fc2), D4, rows, D4, D, 1, EpiGeluBwd<E>{P(y.h), P(y.dh), lp[l].f1b.g, D4}, s)));
            TRY((tgemm<E, false, true>(P(y.dh), D4, P(y.w_fc1), D, rows, D, D4, 1, EpiStore<E>{F(w.dxn), nullptr, nullptr, D}, s)));
            TRY(ln_bwd(F(y.x_mid), y.st2, lp[l].ln2w.p, dres, dres, P(y.dym), rows, lp[l].ln2w.g, lp[l].ln2b.g, lp[l].pb.g, resid_p, site2));
            TRY((tgemm<E, false, true>(P(y.dym), D, P(y.w_proj), D, rows, D, D, 1, EpiStore<E>{nullptr, dy_out, nullptr, D}, s)));
        }
        // FC1: dW1 = dh^T xn2; proj: dWp = dym^T y
        TRY(wg.add(P(y.dh), D4, D4, P(y.xn2), D, D, rows, lp[l].f1w.g));
        TRY(wg.add(P(y.dym), D, D, last ? P(w.ya) : P(y.y), D, D, rows, lp[l].pw.g));
        if (last) {
            // back to all token rows: dy and the residual gradient are zero off the action rows
            hipLaunchKernelGGL(scatter_rows2_kernel<E>, dim3(capped_grid((size_t)M * (D / 4), 4096)), dim3(256), 0, s, (const E*)P(w.dya),
                               P(w.dy), (const float*)F(w.dxa), F(w.dx), M, t, T, G, D);
            TRY(hipGetLastError());
        }
        TRY(launch_attention<true>(l));
        // q/k/v: three weight gradients from the column blocks of dqkv, bias gradients, dxn1 = dqkv Wqkv
        TRY(wg.add(P(y.dqkv), D3, D, P(y.xn1), D, D, M, lp[l].qw.g, lp[l].qb.g));
        TRY(wg.add(P(y.dqkv) + D, D3, D, P(y.xn1), D, D, M, lp[l].kw.g, lp[l].kb.g));
        TRY(wg.add(P(y.dqkv) + 2 * D, D3, D, P(y.xn1), D, D, M, lp[l].vw.g, lp[l].vb.g));
        // LayerNorm-1 backward: into the previous layer's dyo with its FC2 dropout -- first layer: into dx0b with the embedding's
        E* dxb = first ? P(w.dx0b) : P(w.layer[l - 1].dyo);
        float* dbias = first ? nullptr : lp[l - 1].f2b.g;
        const uint32_t site = first ? kEmbedSite : drop_site_mlp(l - 1);
        const float p_site = first ? embed_p : resid_p; const int skip_mod = first ? T : 0;
        if (plan.use_dgrad) {
            const TrainLnBwd e = ln_epilogue(M, x_in, y.st1, lp[l].ln1w.p, F(w.dx), dxb, lp[l].ln1w.g, lp[l].ln1b.g, dbias, p_site, site, skip_mod,
                                             first ? 0 : plan.x16);
            TRY_ST(fused_train_dgrad(plan.lay, ws + w.bimg, l, 0, M, P(y.dqkv), nullptr, nullptr, nullptr, nullptr, nullptr, s, &e));
        } else {
            TRY((tgemm<E, false, true>(P(y.dqkv), D3, P(y.w_qkv), D, M, D, D3, 1, EpiStore<E>{F(w.dxn), nullptr, nullptr, D}, s)));
            TRY(ln_bwd(x_in, y.st1, lp[l].ln1w.p, F(w.dx), F(w.dx), dxb, M, lp[l].ln1w.g, lp[l].ln1b.g, dbias, p_site, site, skip_mod));
        }
        return BESO_OK;
    }
    // the gradients of layers l .. L-1 and ln_f are complete once their weight gradients and LayerNorm sums have run: do those now and
    // order `early_stream` behind this point (the C1 exchange of that range can start under the backward of layers l-1 .. 0)
    int early_flush() {
        TRY(wg.flush());
        TRY_ST(fused_train_bias_reduce(b1_slabs, b1_outs, b1_blocks, b1_n, D4, s));
        b1_n = 0;
        TRY(ln.reduce(s));
        hipEvent_t ev = nullptr;
        TRY(record_event(kEvEarly, s, &ev));
        TRY(hipStreamWaitEvent(early_stream, ev, 0));
        return BESO_OK;
    }
    int finish() {
        if (vjp) {
            // F(w.dx) holds the fp32 gradient of x0 (layer 0's LayerNorm-1 backward): onto the action input
            hipLaunchKernelGGL(vjp_input_kernel, dim3(batch), dim3(256), 0, s, (const float*)F(w.dx), par.actw.p, sigma, vjp->cot,
                               vjp->x_grad, vjp->dot, t, T, G, D, act, c->sigma_data);
            TRY(hipGetLastError());
            if (state_grad || goal_grad) TRY(input_grads());
            return BESO_OK;
        }
        // embeddings: dWcat[Ke][D] = Xemb^T dx0, routed to pos_emb / tok_emb / action_emb / sigma_emb after the launch
        TRY(wg.add(P(w.xemb), Ke, Ke, P(w.dx0b), D, D, M, F(w.dw_cat)));
        // The reductions of the FC1-bias slabs and of the LayerNorm / bias partial sums read what the data-gradient kernels wrote
        // and write gradient tensors of their own: nothing ties them to the grouped weight-gradient launch, which leaves 38 of the
        // 256 CUs idle (218 panel tiles) -- they run BESIDE it on the library's side stream (three launches of 12 + 12 + 24 us off the
        // step's chain; a dependent launch costs ~5 us whatever it does: tools/microbench/launch_chain).
        hipEvent_t ev_sf = nullptr, ev_sj = nullptr;
        hipStream_t rs = s;                               // stream of the partial-sum reductions
        if (plan.panel_w) {
            TRY(step_side_stream(&rs));
            TRY(record_event(kEvSideFork, s, &ev_sf));
            TRY(hipStreamWaitEvent(rs, ev_sf, 0));
        } else TRY(wg.flush());
        TRY_ST(fused_train_bias_reduce(b1_slabs, b1_outs, b1_blocks, b1_n, D4, rs));
        b1_n = 0;
        TRY(ln.reduce(rs));
        if (plan.panel_w) {
            TRY(record_event(kEvSideJoin, rs, &ev_sj));
            TRY(wg.flush());
            TRY(hipStreamWaitEvent(s, ev_sj, 0));
        }
        if (mlp_head) {
            TRY(hipMemcpy2DAsync(par.hw.g, sizeof(float) * Hh, ws + w.dw_head, sizeof(float) * Hp, sizeof(float) * Hh, act,
                                 hipMemcpyDeviceToDevice, s));                                    // [act][Hp] -> [act][100]
            TRY(hipMemcpyAsync(par.h0w.g, ws + w.dw_hid, sizeof(float) * (size_t)Hh * D, hipMemcpyDeviceToDevice, s));
            TRY(hipMemcpyAsync(par.h0b.g, ws + w.db_hid, sizeof(float) * Hh, hipMemcpyDeviceToDevice, s));
        }
        hipLaunchKernelGGL(scatter_emb_kernel, dim3(64), dim3(256), 0, s, (const float*)F(w.dw_cat), par.pos.g, par.tokw.g, par.tokb.g,
                           par.sigw.g, par.sigb.g, par.actw.g, par.actb.g, D, obs, act, seq);
        TRY(hipGetLastError());
        if (state_grad || goal_grad) TRY(input_grads());
        return BESO_OK;
    }
    // F(w.dx), the fp32 gradient of x0 BEHIND the embedding dropout (the LayerNorm-1 backward of layer 0 stores it before it
    // applies that mask to the typed copy dx0b), onto the state / goal inputs through tok_emb.weight; the kernel applies the
    // embedding dropout and mask_cond's goal mask of this call (both off in the input-VJP mode)
    hipError_t input_grads() {
        const int rows = batch * ((state_grad ? t : 0) + (goal_grad ? G : 0));
        const int dc = D < kIgChunk ? D : kIgChunk;
        const int tiles = (rows + kIgRows - 1) / kIgRows;
        hipLaunchKernelGGL(input_grad_kernel, dim3(tiles < 1024 ? tiles : 1024, (obs + kIgCols - 1) / kIgCols), dim3(256),
                           sizeof(float) * ((size_t)kIgRows * (dc + kIgPad) + (size_t)dc * kIgCols), s, (const float*)F(w.dx), par.tokw.p, state_grad, goal_grad,
                           batch, t, T, G, D, obs, dc, embed_p, goal_p, seed);
        return hipGetLastError();
    }
};

// checks the call (train_validate's status first, then BESO_ERR_BAD_ARG, then the workspace) and runs it in its precision
static int run_train_step(TrainCall a, int n_params, size_t workspace_bytes) {
    const beso_config* c = a.c;
    int st = train_validate(c, a.batch, a.t);
    if (st != BESO_OK) return st;
    if (a.precision != BESO_PREC_BF16 && a.precision != BESO_PREC_FP32) return BESO_ERR_BAD_ARG;
    if (!a.p || !a.state || !a.action || !a.sigma || !a.ws) return BESO_ERR_BAD_ARG;
    if (a.vjp ? (!a.vjp->cot || !a.vjp->denoised || !a.vjp->x_grad) : (!a.gflat || !a.noise || !a.loss_out)) return BESO_ERR_BAD_ARG;
    if (c->goal_seq_len > 0 && !a.goal) return BESO_ERR_BAD_ARG;
    if ((a.goal_grad && c->goal_seq_len == 0) || (((uintptr_t)a.state_grad | (uintptr_t)a.goal_grad) & 3)) return BESO_ERR_BAD_ARG;
    ModelParams par(c);
    if (par.read(a.p, n_params) != BESO_OK) return BESO_ERR_BAD_ARG;
    // (the input VJP has neither a loss nor a bias gradient: BESO_TRAIN_DETERMINISTIC means nothing there and is refused)
    if (a.flags & ~((a.vjp ? 0 : BESO_TRAIN_LAST_ACTION_ONLY | BESO_TRAIN_DETERMINISTIC) | BESO_TRAIN_PLAN_PER_OP | BESO_TRAIN_PLAN_TILES)) return BESO_ERR_BAD_ARG;
    if (!(a.attn_p >= 0.f && a.attn_p < 1.f && a.resid_p >= 0.f && a.resid_p < 1.f && a.embed_p >= 0.f && a.embed_p < 1.f &&
          a.goal_p >= 0.f && a.goal_p <= 1.f))
        return BESO_ERR_BAD_ARG;
    TrainWs w;
    make_train_ws(c, a.batch, a.t, a.precision, &w);
    if (workspace_bytes < w.total) return BESO_ERR_WORKSPACE;
    if (a.vjp) {
        // (the step's loss slot: the target buffer, unused in this mode; the gradient pointers: the dw_cat slab, see VjpIo)
        a.loss_out = (float*)(a.ws + w.target);
        a.gflat = (float*)(a.ws + w.dw_cat);
        (void)hipGetLastError();
    }
    par.set_grads(a.gflat, !a.vjp);
    if (a.precision == BESO_PREC_FP32) return TrainStep<float>(a, w, par).run();
    return TrainStep<uint16_t>(a, w, par).run();
}

int train_loss_grad(const beso_config* c, const float* const* params, int n_params, float* grads_flat, int precision,
                    const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                    float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                    float goal_drop, uint32_t seed, float grad_scale,
                    void* workspace, size_t workspace_bytes, hipStream_t s, hipStream_t early_stream, hipStream_t loss_stream,
                    float* state_grad, float* goal_grad, hipError_t* err, int* err_line) {
    return run_train_step(TrainCall{c, params, grads_flat, precision, state, action, goal, noise, sigma, loss_out, batch, t, flags,
                                    embed_pdrop, attn_pdrop, resid_pdrop, goal_drop, seed, grad_scale, (char*)workspace, s, early_stream,
                                    loss_stream, err, err_line, nullptr, state_grad, goal_grad}, n_params, workspace_bytes);
}

int train_denoise_vjp(const beso_config* c, const float* const* params, int n_params, int precision, const float* state,
                      const float* x, const float* goal, const float* sigma, const float* cot, float* denoised, float* x_grad,
                      float* dot, int batch, int t, int flags, void* workspace, size_t workspace_bytes, hipStream_t s,
                      float* state_grad, float* goal_grad, hipError_t* err, int* err_line) {
    const VjpIo io{cot, denoised, x_grad, dot};
    return run_train_step(TrainCall{c, params, nullptr, precision, state, x, goal, nullptr, sigma, nullptr, batch, t, flags, 0.f, 0.f,
                                    0.f, 0.f, 0u, 1.f, (char*)workspace, s, nullptr, nullptr, err, err_line, &io, state_grad, goal_grad},
                          n_params, workspace_bytes);
}

int train_goal_mask(float* mask, size_t n, float goal_drop, uint32_t seed, hipStream_t s, hipError_t* err, int* err_line) {
    if (!mask || !(goal_drop >= 0.f && goal_drop <= 1.f)) return BESO_ERR_BAD_ARG;
    if (n == 0) return BESO_OK;
    (void)hipGetLastError();
    hipLaunchKernelGGL(goal_mask_kernel, dim3(capped_grid(n, 2048)), dim3(256), 0, s, mask, n, goal_drop, seed);
    TRY(hipGetLastError());
    return BESO_OK;
}

// the shapes are the step's (train_validate: the same statuses as beso_loss_grad for the same cfg, batch, t)
int train_dropout_mask(const beso_config* c, float* scale, int kind, int layer, int batch, int t, float p, uint32_t seed,
                       hipStream_t s, hipError_t* err, int* err_line) {
    if (!c || !scale) return BESO_ERR_BAD_ARG;
    const int st = train_validate(c, batch, t);
    if (st != BESO_OK) return st;
    if (kind < BESO_DROP_EMBED || kind > BESO_DROP_MLP || !(p >= 0.f && p < 1.f) || ((uintptr_t)scale & 15)) return BESO_ERR_BAD_ARG;
    if (kind != BESO_DROP_EMBED && (layer < 0 || layer >= c->n_layers)) return BESO_ERR_BAD_ARG;
    const int T = 1 + c->goal_seq_len + 2 * t, D = c->embed_dim, H = c->n_heads;
    const bool attn = kind == BESO_DROP_ATTN;
    const size_t n = attn ? (size_t)batch * H * T * T : (size_t)batch * T * D;
    const uint32_t site = kind == BESO_DROP_EMBED ? kEmbedSite : attn ? drop_site_attn(layer)
                        : kind == BESO_DROP_PROJ ? drop_site_proj(layer) : drop_site_mlp(layer);
    // the last layer continues on the compact action rows behind its attention (forward_layer, train_fwd_kernel's rows_act)
    const int compact = (kind == BESO_DROP_PROJ || kind == BESO_DROP_MLP) && layer == c->n_layers - 1;
    (void)hipGetLastError();
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(capped_grid((n + 3) / 4, 2048)), dim3(256), 0, s, scale, n, attn ? 0 : D, T, t,
                       c->goal_seq_len, kind == BESO_DROP_EMBED ? 1 : 0, compact, p, p > 0.f ? 1.0f / (1.0f - p) : 1.f, seed, site);
    TRY(hipGetLastError());
    return BESO_OK;
}

#if BESO_DEV_API
// development aid: C[M][N] = op(A) op(B)^T through tgemm (fp32 output), for the layout tests
int train_debug_gemm(int precision, int a_kslow, int b_kslow, const void* A, int lda, const void* B, int ldb, float* C,
                     int ldc, int M, int N, int K, int splits, hipStream_t s, hipError_t* err, int* err_line) {
    if (!A || !B || !C) return BESO_ERR_BAD_ARG;
    if (precision == BESO_PREC_BF16 && ((a_kslow == 1 && (b_kslow == 2 || b_kslow == 3)) || (b_kslow == 1 && (a_kslow == 2 || a_kslow == 3)))) {
        // the panel-owning weight-gradient tiles: (1, W) = tiles of 128 rows x all N <= 128 W columns, (W, 1) = all M <= 128 W rows
        // x 128 columns; both operands k-slow, C contiguous (ldc == N); splits > 1: row ranges into slabs behind C's M x N floats
        const int W = a_kslow > 1 ? a_kslow : b_kslow;
        if (ldc != N || (a_kslow > 1 ? M : N) > 128 * W || M % 8 || N % 8 || lda % 8 || ldb % 8) return BESO_ERR_BAD_ARG;
        GTable t;
        int orient = a_kslow > 1 ? -1 : 0;
        const int tiles = orient ? (N + kTileMN - 1) / kTileMN : (M + kTileMN - 1) / kTileMN;
        t.n = 1;
        t.p[0] = GProb{A, B, C, nullptr, lda, ldb, M, N, 0, orient, K, 0u};
        if (splits < 1) splits = 1;
        float* slab = C + (size_t)round_up(M * N, 4);
        const size_t stride = (size_t)round_up(M * N, 4);
        TRY(W == 2 ? launch_panel_group<2>(t, tiles, splits, slab, stride, s) : launch_panel_group<3>(t, tiles, splits, slab, stride, s));
        if (splits > 1) {
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((M * N + 1023) / 1024), dim3(256), 0, s, t, (const float*)slab,
                               (size_t)round_up(M * N, 4), splits, (uint32_t)(M * N));
            TRY(hipGetLastError());
        }
        return BESO_OK;
    }
#define DBG(E, AK, BK)                                                                                             \
    do {                                                                                                           \
        if (splits > 1) TRY((tgemm<E, AK, BK>(A, lda, B, ldb, M, N, K, splits, epi_atomic(C, ldc), s)));          \
        else TRY((tgemm<E, AK, BK>(A, lda, B, ldb, M, N, K, 1, EpiStore<E>{C, nullptr, nullptr, ldc}, s)));      \
        return BESO_OK;                                                                                            \
    } while (0)
    if (precision == BESO_PREC_FP32) {
        if (!a_kslow && !b_kslow) DBG(float, false, false);
        if (!a_kslow && b_kslow) DBG(float, false, true);
        if (a_kslow && b_kslow) DBG(float, true, true);
    } else if (precision == BESO_PREC_BF16) {
        if (!a_kslow && !b_kslow) DBG(uint16_t, false, false);
        if (!a_kslow && b_kslow) DBG(uint16_t, false, true);
        if (a_kslow && b_kslow) DBG(uint16_t, true, true);
    }
#undef DBG
    return BESO_ERR_UNSUPPORTED;
}
#endif

}  // namespace beso
