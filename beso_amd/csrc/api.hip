// extern "C" entry points of libbeso_hip.so (include/beso_hip.h) and the host-side orchestration of
// one score-network forward / one sampling loop.  No allocation, no synchronisation: everything is
// enqueued on the caller's stream.
#include <math.h>
#include <string.h>
#include <stdio.h>
#include <vector>
#include "common.h"
#include "fused.h"
#include "train.h"
#if BESO_DEV_API
#include "../../include/beso_hip_debug.h"
#endif

namespace beso {

// ---------------------------------------------------------------------------------------------
int validate_config(const beso_config* c) {
    if (!c) return BESO_ERR_BAD_ARG;
    if (c->obs_dim < 1 || c->act_dim < 1 || c->act_dim > 64 || c->embed_dim < 8 || c->n_layers < 1 ||
        c->n_layers > kMaxLayers || c->n_heads < 1 || c->goal_seq_len < 0 || c->obs_seq_len < 1)
        return BESO_ERR_BAD_CONFIG;
    if (c->embed_dim % c->n_heads != 0) return BESO_ERR_BAD_CONFIG;
    if (c->embed_dim > 1024) return BESO_ERR_UNSUPPORTED;              // LayerNorm keeps a row in registers
    if (c->embed_dim / c->n_heads > 128) return BESO_ERR_UNSUPPORTED;  // attention keeps q/o rows in registers
    if (!(c->sigma_data > 0.f)) return BESO_ERR_BAD_CONFIG;
    return BESO_OK;
}

bool make_layout(const beso_config* c, int precision, Layout* o) {
    if (validate_config(c) != BESO_OK) return false;
    if (precision != BESO_PREC_BF16 && precision != BESO_PREC_FP32 && precision != BESO_PREC_BF16X3 && precision != BESO_PREC_FP16)
        return false;
    memset(o, 0, sizeof(*o));
    o->D = c->embed_dim; o->H = c->n_heads; o->hd = o->D / o->H; o->L = c->n_layers;
    o->G = c->goal_seq_len; o->W = c->obs_seq_len; o->obs = c->obs_dim; o->act = c->act_dim;
    o->seq_size = o->G + o->W + 1;
    o->linear_output = c->linear_output ? 1 : 0;
    o->Kd = round_up(o->D, 64); o->Kh = round_up(4 * o->D, 64);
    o->Nqkv = round_up(3 * o->D, kTileMN); o->Nd = round_up(o->D, kTileMN); o->Nh = round_up(4 * o->D, kTileMN);
    o->elem_bytes = precision == BESO_PREC_FP32 ? 4 : 2;
    size_t cur = 0;
    const size_t f = sizeof(float), e = (size_t)o->elem_bytes;
    o->pos_emb = carve(cur, f * o->seq_size * o->D);
    o->tok_w = carve(cur, f * o->D * o->obs); o->tok_b = carve(cur, f * o->D);
    o->sig_w = carve(cur, f * o->D); o->sig_b = carve(cur, f * o->D);
    o->act_w = carve(cur, f * o->D * o->act); o->act_b = carve(cur, f * o->D);
    o->lnf_w = carve(cur, f * o->D); o->lnf_b = carve(cur, f * o->D);
    if (o->linear_output) {
        o->head_w0 = carve(cur, f * o->act * o->D); o->head_b0 = carve(cur, f * o->act);
        o->head_w1 = o->head_w0; o->head_b1 = o->head_b0;
    } else {
        o->head_w0 = carve(cur, f * kHeadHidden * o->D); o->head_b0 = carve(cur, f * kHeadHidden);
        o->head_w1 = carve(cur, f * o->act * kHeadHidden); o->head_b1 = carve(cur, f * o->act);
    }
    for (int l = 0; l < o->L; ++l) {
        LayerOff& y = o->layer[l];
        y.ln1_w = carve(cur, f * o->D); y.ln1_b = carve(cur, f * o->D);
        y.ln2_w = carve(cur, f * o->D); y.ln2_b = carve(cur, f * o->D);
        y.b_qkv = carve(cur, f * o->Nqkv); y.b_proj = carve(cur, f * o->Nd);
        y.b_fc1 = carve(cur, f * o->Nh); y.b_fc2 = carve(cur, f * o->Nd);
        y.w_qkv = carve(cur, e * o->Nqkv * o->Kd); y.w_proj = carve(cur, e * o->Nd * o->Kd);
        y.w_fc1 = carve(cur, e * o->Nh * o->Kd); y.w_fc2 = carve(cur, e * o->Nd * o->Kh);
    }
    const FusedUnit fu = fused_unit(precision);
    o->fused = carve(cur, fu.packed_bytes(*o, fu.precision));
    o->total = cur;
    return true;
}

bool make_workspace(const beso_config* c, const Layout& lay, int batch, int t, int precision, int cfg_guidance,
                    Workspace* w) {
    if (batch < 1 || t < 1 || t > c->obs_seq_len) return false;
    memset(w, 0, sizeof(*w));
    const size_t vb = (size_t)batch * (cfg_guidance ? 2 : 1);
    const size_t T = 1 + lay.G + 2 * (size_t)t;
    const size_t M = round_up_sz(vb * T, kTileMN);        // rows padded so tile loads never need a clamp
    // (the split-bf16 block kernels of the long-sequence shape exchange q/k/v and the attention output as fp32 rows)
    const size_t e = (precision == BESO_PREC_BF16X3 && fused_has_lin_blocks(lay, precision)) ? 4 : lay.elem_bytes, f = sizeof(float);
    size_t cur = 0;
    w->x = carve(cur, f * M * lay.D);
    w->xn = carve(cur, e * M * lay.Kd);
    w->qkv = carve(cur, e * M * 3 * lay.D);
    w->y = carve(cur, e * M * lay.Kd);
    w->h = carve(cur, e * M * lay.Kh);
    const size_t na = (size_t)batch * t * lay.act;
    w->den = carve(cur, f * na); w->x2 = carve(cur, f * na); w->d1 = carve(cur, f * na);
    w->sig = carve(cur, f * batch);
    w->small = carve(cur, f * (size_t)(lay.H + 1) * kSmallProjRows * lay.D);
    w->fused = carve(cur, 256);
    w->total = cur;
    return true;
}

// ---------------------------------------------------------------------------------------------
// profiling hooks
// ---------------------------------------------------------------------------------------------
// (state of the CALLING THREAD: a thread that times its launch sites does not see, and does not disturb, other callers)
static thread_local int g_prof_site = 0;
static thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_events;
static thread_local std::vector<hipEvent_t> g_prof_free;
static thread_local hipEvent_t g_prof_open = nullptr;

static hipEvent_t prof_get_event() {
    if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

void profile_begin(int site, hipStream_t s) {
    if (g_prof_site != site) return;
    hipEvent_t e = prof_get_event();
    if (!e) return;
    (void)hipEventRecord(e, s);
    g_prof_open = e;
}

void profile_end(int site, hipStream_t s) {
    if (g_prof_site != site) return;
    if (!g_prof_open) return;
    hipEvent_t e = prof_get_event();
    if (!e) return;
    (void)hipEventRecord(e, s);
    g_prof_events.emplace_back(g_prof_open, e);
    g_prof_open = nullptr;
}

// ---------------------------------------------------------------------------------------------
// one forward of the score network (unfused generic path)
// ---------------------------------------------------------------------------------------------
static thread_local char g_last_error[256] = "";
static int record_hip_error(hipError_t e, const char* what, int line) {
    snprintf(g_last_error, sizeof(g_last_error), "%s (%d) from `%s` at api.hip:%d", hipGetErrorName(e), (int)e, what, line);
    return BESO_ERR_HIP;
}
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return record_hip_error(_e, #expr, __LINE__); } while (0)

static int forward_generic(const Layout& lay, const Workspace& ws, const char* packed, int precision,
                           const FwdArgs& a, char* wsp, hipStream_t s, int fused) {
    float* x = (float*)(wsp + ws.x);
    void* xn = wsp + ws.xn; void* qkv = wsp + ws.qkv; void* y = wsp + ws.y; void* h = wsp + ws.h;
    const int M = a.vbatch * a.T;
    auto F = [&](size_t off) { return (const float*)(packed + off); };
    int fused_edges = 0;
    if (fused == 2) {
        // embed -> all transformer layers -> head as ONE launch: the residual tile of 8 samples never leaves
        // the CU's registers (shapes whose head cannot be fused store x and run the head kernel)
        const FusedUnit fu = fused_unit(precision);
        if (!(fu.layer_edges(lay) & 1)) {
            profile_begin(BESO_SITE_EMBED, s);
            HIP_TRY(launch_embed(lay, packed, a, x, s));
            profile_end(BESO_SITE_EMBED, s);
        }
        profile_begin(BESO_SITE_FUSED_LAYER, s);
        int st = fu.layers(lay, packed, a, x, &fused_edges, fu.precision, s, nullptr, nullptr, nullptr);
        profile_end(BESO_SITE_FUSED_LAYER, s);
        if (st != BESO_OK) return st;
    } else {
        profile_begin(BESO_SITE_EMBED, s);
        HIP_TRY(launch_embed(lay, packed, a, x, s));
        profile_end(BESO_SITE_EMBED, s);
    }
    const bool lin_blocks = fused == 1 && fused_has_lin_blocks(lay, precision);
    for (int l = 0; l < (fused == 2 ? 0 : lay.L); ++l) {
        const LayerOff& o = lay.layer[l];
        if (lin_blocks && precision == BESO_PREC_BF16X3) {
            // the same two-launch form in split-bf16 arithmetic: lin_block_x3_kernel around the split-bf16 attention kernel on the
            // matrix pipe (round 6; windows of <= 16 tokens and odd head dims: the exact-fp32 kernel)
            if (l == 0) {
                profile_begin(BESO_SITE_FUSED_LAYER, s);
                int st0 = fused_lin_x3(lay, packed, -1, 0, x, nullptr, 0, (float*)qkv, M, s);
                profile_end(BESO_SITE_FUSED_LAYER, s);
                if (st0 != BESO_OK) return st0;
            }
            profile_begin(BESO_SITE_ATTENTION, s);
            HIP_TRY(launch_attention(qkv, y, a.vbatch, a.T, lay.D, lay.H, lay.Kd, BESO_PREC_BF16X3, s));
            profile_end(BESO_SITE_ATTENTION, s);
            profile_begin(BESO_SITE_FUSED_LAYER, s);
            int st = fused_lin_x3(lay, packed, l, l + 1 < lay.L ? l + 1 : -1, x, (const float*)y, lay.Kd, (float*)qkv, M, s);
            profile_end(BESO_SITE_FUSED_LAYER, s);
            if (st != BESO_OK) return st;
            continue;
        } else if (lin_blocks) {
            // long sequences (no fused attention phase): two launches per layer --
            //   attention(q/k/v of this layer)  ->  [proj + residual -> LN2 -> MLP -> LN1 + q/k/v of the NEXT layer]
            // with the residual tile in registers through the second one; layer 0's q/k/v come from their own block
            if (l == 0) {
                profile_begin(BESO_SITE_GEMM_QKV, s);
                int st0 = fused_lin_block(lay, packed, 0, 0, x, qkv, 3 * lay.D, M, s);
                profile_end(BESO_SITE_GEMM_QKV, s);
                if (st0 != BESO_OK) return st0;
            }
            profile_begin(BESO_SITE_ATTENTION, s);
            HIP_TRY(launch_attention(qkv, y, a.vbatch, a.T, lay.D, lay.H, lay.Kd, precision, s));
            profile_end(BESO_SITE_ATTENTION, s);
            profile_begin(BESO_SITE_FUSED_LAYER, s);
            int st = fused_lin_tail(lay, packed, l, x, y, lay.Kd, qkv, M, s);
            profile_end(BESO_SITE_FUSED_LAYER, s);
            if (st != BESO_OK) return st;
            continue;
        } else {
            profile_begin(BESO_SITE_LAYERNORM, s);
            HIP_TRY(launch_layernorm(x, F(o.ln1_w), F(o.ln1_b), xn, M, lay.D, lay.Kd, precision, s));
            profile_end(BESO_SITE_LAYERNORM, s);
            profile_begin(BESO_SITE_GEMM_QKV, s);
            HIP_TRY(launch_gemm(precision, EPI_BIAS_STORE, xn, lay.Kd, packed + o.w_qkv, lay.Kd, F(o.b_qkv), qkv,
                                3 * lay.D, 3 * lay.D, M, lay.Nqkv, lay.Kd, s));
            profile_end(BESO_SITE_GEMM_QKV, s);
            profile_begin(BESO_SITE_ATTENTION, s);
            HIP_TRY(launch_attention(qkv, y, a.vbatch, a.T, lay.D, lay.H, lay.Kd, precision, s));
            profile_end(BESO_SITE_ATTENTION, s);
            profile_begin(BESO_SITE_GEMM_PROJ, s);
            HIP_TRY(launch_gemm(precision, EPI_BIAS_RESID, y, lay.Kd, packed + o.w_proj, lay.Kd, F(o.b_proj), x, lay.D,
                                lay.D, M, lay.Nd, lay.Kd, s));
            profile_end(BESO_SITE_GEMM_PROJ, s);
        }
        if (fused == 1) {
            // LN2 + FC1 + GELU + FC2 + residual as one kernel, hidden activations never leave the CU
            profile_begin(BESO_SITE_FUSED_LAYER, s);
            int st = fused_mlp_block(lay, packed, l, x, M, s);
            profile_end(BESO_SITE_FUSED_LAYER, s);
            if (st != BESO_OK) return st;
            continue;
        }
        HIP_TRY(launch_layernorm(x, F(o.ln2_w), F(o.ln2_b), xn, M, lay.D, lay.Kd, precision, s));
        profile_begin(BESO_SITE_GEMM_FC1, s);
        HIP_TRY(launch_gemm(precision, EPI_BIAS_GELU_STORE, xn, lay.Kd, packed + o.w_fc1, lay.Kd, F(o.b_fc1), h,
                            lay.Kh, lay.Kh, M, lay.Nh, lay.Kd, s));
        profile_end(BESO_SITE_GEMM_FC1, s);
        profile_begin(BESO_SITE_GEMM_FC2, s);
        HIP_TRY(launch_gemm(precision, EPI_BIAS_RESID, h, lay.Kh, packed + o.w_fc2, lay.Kh, F(o.b_fc2), x, lay.D,
                            lay.D, M, lay.Nd, lay.Kh, s));
        profile_end(BESO_SITE_GEMM_FC2, s);
    }
    if (!(fused_edges & 2)) {
        profile_begin(BESO_SITE_HEAD, s);
        HIP_TRY(launch_head(lay, packed, a, x, s));
        profile_end(BESO_SITE_HEAD, s);
    }
    return BESO_OK;
}

static int forward(const beso_config* cfg, const void* packed, int precision, const float* state,
                   const float* action, const float* goal, const float* sigma, float* out, int batch, int t,
                   int flags, float cond_lambda, int precondition, void* workspace, size_t workspace_bytes,
                   hipStream_t s) {
    int st = validate_config(cfg);
    if (st != BESO_OK) return st;
    if (precision != BESO_PREC_BF16 && precision != BESO_PREC_FP32 && precision != BESO_PREC_BF16X3 && precision != BESO_PREC_FP16)
        return BESO_ERR_BAD_ARG;
    if (batch < 1 || t < 1 || t > cfg->obs_seq_len) return BESO_ERR_BAD_SHAPE;
    if (!packed || !state || !action || !sigma || !out || !workspace) return BESO_ERR_BAD_ARG;
    if (cfg->goal_seq_len > 0 && !goal) return BESO_ERR_BAD_ARG;
    if (flags & ~(BESO_FLAG_UNCOND | BESO_PLAN_MASK)) return BESO_ERR_BAD_ARG;
    Layout lay;
    if (!make_layout(cfg, precision, &lay)) return BESO_ERR_BAD_CONFIG;
    // ClassifierFreeSampleModel (classifier_free_sampler.py:35-49)
    bool uncond = (flags & BESO_FLAG_UNCOND) != 0;
    bool two = false;
    if (precondition && !uncond) {
        if (cond_lambda == 0.f) uncond = true;
        else if (cond_lambda != 1.f) two = true;
    }
    Workspace ws;
    if (!make_workspace(cfg, lay, batch, t, precision, two ? 1 : 0, &ws)) return BESO_ERR_BAD_SHAPE;
    if (workspace_bytes < ws.total) return BESO_ERR_WORKSPACE;
    FwdArgs a;
    a.state = state; a.action = action; a.goal = goal; a.sigma = sigma; a.out = out;
    a.batch = batch; a.vbatch = two ? 2 * batch : batch; a.t = t; a.T = 1 + lay.G + 2 * t;
    a.precondition = precondition;
    a.uncond_from = two ? batch : (uncond ? 0 : a.vbatch);
    a.cond_lambda = cond_lambda; a.sigma_data = cfg->sigma_data;
    a.plan = flags & BESO_PLAN_MASK;
    if (precision == BESO_PREC_FP16) a.plan &= ~(BESO_PLAN_PER_OP | BESO_PLAN_BLOCKS);      // (no per-op / block form: the hint is ignored, as the header says)
    a.sig_flag = (uint32_t*)((char*)workspace + ws.fused);
    if (small_wanted(lay, a, precision)) {
        // few samples: the weights, not the samples, are spread over the chip (small.hip)
        hipError_t e = hipSuccess;
        profile_begin(BESO_SITE_FORWARD, s);
        const int r = forward_small(lay, ws, (const char*)packed, precision, a, (char*)workspace, s, &e);
        profile_end(BESO_SITE_FORWARD, s);
        return r == BESO_ERR_HIP ? record_hip_error(e, "forward_small", __LINE__) : r;
    }
    const FusedUnit fu = fused_unit(precision);
    const int level = fu.level(lay, a, fu.precision);
    // BF16X3 / FP16 are instances of the one-launch kernel (layers_kernel) -- BF16X3 also of its block-kernel form on the
    // long-sequence shape -- and have no per-op form
    if (precision == BESO_PREC_FP16 && level != 2) return BESO_ERR_UNSUPPORTED;
    if (precision == BESO_PREC_BF16X3 && level != 2 && !(level == 1 && fused_has_lin_blocks(lay, precision))) return BESO_ERR_UNSUPPORTED;
    profile_begin(BESO_SITE_FORWARD, s);
    int r = forward_generic(lay, ws, (const char*)packed, precision, a, (char*)workspace, s, level);
    profile_end(BESO_SITE_FORWARD, s);
    return r;
}

// Whether forward() has kernels for a raw-network (no preconditioning, no classifier-free pair) call of this shape, precision
// and plan: its BESO_ERR_UNSUPPORTED decision alone, for an entry point that enqueues work of its own in front of the forward
// and has made the other checks itself.  Nothing is enqueued.
static int forward_supported(const beso_config* cfg, int precision, int batch, int t, int flags) {
    Layout lay;
    if (!make_layout(cfg, precision, &lay)) return BESO_ERR_BAD_CONFIG;
    FwdArgs a{};
    a.batch = a.vbatch = batch; a.t = t; a.T = 1 + lay.G + 2 * t;
    a.uncond_from = (flags & BESO_FLAG_UNCOND) ? 0 : batch;
    a.cond_lambda = 1.0f; a.sigma_data = cfg->sigma_data;
    a.plan = flags & BESO_PLAN_MASK;
    if (precision == BESO_PREC_FP16) a.plan &= ~(BESO_PLAN_PER_OP | BESO_PLAN_BLOCKS);
    if (small_wanted(lay, a, precision)) return BESO_OK;
    const FusedUnit fu = fused_unit(precision);
    const int level = fu.level(lay, a, fu.precision);
    if (precision == BESO_PREC_FP16 && level != 2) return BESO_ERR_UNSUPPORTED;
    if (precision == BESO_PREC_BF16X3 && level != 2 && !(level == 1 && fused_has_lin_blocks(lay, precision))) return BESO_ERR_UNSUPPORTED;
    return BESO_OK;
}

// beso_loss_fwd's workspace: the forward's, then the forward's input, its output and the per-sample values
struct LossWorkspace { size_t forward, scaled, pred, rows, total; };
static bool loss_workspace(const beso_config* cfg, int batch, int t, int precision, LossWorkspace* w) {
    Layout lay;
    Workspace ws;
    if (!make_layout(cfg, precision, &lay) || !make_workspace(cfg, lay, batch, t, precision, 0, &ws)) return false;
    const size_t na = (size_t)batch * t * lay.act;
    size_t cur = 0;
    carve(cur, ws.total);
    w->forward = ws.total;
    w->scaled = carve(cur, sizeof(float) * na);
    w->pred = carve(cur, sizeof(float) * na);
    w->rows = carve(cur, sizeof(float) * (size_t)batch);
    w->total = cur;
    return true;
}

// ---------------------------------------------------------------------------------------------
// sampling loops: each sampler entry point lists its network evaluations (a plan) and one driver runs the list
// ---------------------------------------------------------------------------------------------
// One evaluation: its record (sigma, c0, c1, mode, c2), its fifth number (SampleExtra's c3) and the sampler step it belongs to.
// Every coefficient is an fp32 scalar computed as the reference computes it (numpy float32 / 0-d tensors).
struct PlanEval { StepRec rec; float c3; int step; };
struct Plan {
    std::vector<PlanEval> ev;
    std::vector<int> first;      // index of the first evaluation of every step, then ev.size()
    void add(int step, float sigma, float c0, float c1, int mode, float c2 = 0.f, float c3 = 0.f) {
        ev.push_back(PlanEval{StepRec{sigma, c0, c1, mode, c2}, c3, step});
    }
};

// get_ancestral_step (gc_sampling.py:107-114) in fp32
static void ancestral_step(float sf, float sn, float eta, float& down, float& up) {
    down = sn; up = 0.f;
    if (eta != 0.f) {
        up = eta * sqrtf(sn * sn * (sf * sf - sn * sn) / (sf * sf));
        if (sn < up) up = sn;
        down = sqrtf(sn * sn - up * up);
    }
}

// exp(lerp(log a, log b, 0.5))
static float log_midpoint(float a, float b) {
    const float la = logf(a), lb = logf(b);
    const float hm = 0.5f * (lb - la);
    return expf(la + hm);
}

// The exponential-integrator step from sigma a to sigma b (gc_sampling.py:921-923): t = -log a, h = -log b - t,
// x <- ratio*x - em1*den with ratio = sigma_fn(t + h)/sigma_fn(t), em1 = expm1(-h).  b == 0 -> h = +inf -> x = den exactly.
struct ExpStep { float t, h, ratio, em1; };
static ExpStep exp_step(float a, float b) {
    const float t = -logf(a), tn = -logf(b);
    const float h = tn - t;
    return ExpStep{t, h, expf(-tn) / expf(-t), expm1f(-h)};
}

// linear_multistep_coeff (gc_sampling.py:416-429): the integral over [t_i, t_{i+1}] of the Lagrange basis polynomial of node
// t_{i-j} on t_i ... t_{i-order+1}.  The reference integrates it with scipy's quad, exact for a polynomial of degree <= 3 up to
// rounding; so does the three-point Gauss-Legendre rule (exact to degree 5), in double.  The denominators are fp32 differences
// of the fp32 schedule, as the reference's numpy scalars.
static double lms_coeff(int order, const float* t, int i, int j) {
    auto basis = [&](double tau) {
        double prod = 1.0;
        for (int k = 0; k < order; ++k)
            if (k != j) prod *= (tau - (double)t[i - k]) / (double)(t[i - j] - t[i - k]);
        return prod;
    };
    const double a = t[i], b = t[i + 1], mid = 0.5 * (a + b), half = 0.5 * (b - a);
    const double xg = sqrt(0.6);
    return half * ((5.0 / 9.0) * basis(mid - half * xg) + (8.0 / 9.0) * basis(mid) + (5.0 / 9.0) * basis(mid + half * xg));
}

// beso_sample: DDIM (gc_sampling.py:921-923), Euler (:205-210) and Heun (:296-310, plain Euler on the last step :301-303)
static Plan plan_sample(int sampler, const float* sigmas, int n_sigmas) {
    Plan p;
    for (int i = 0; i + 1 < n_sigmas; ++i) {
        const float si = sigmas[i], sn = sigmas[i + 1];
        p.first.push_back((int)p.ev.size());
        if (sampler == BESO_SAMPLER_DDIM) {
            const ExpStep e = exp_step(si, sn);
            p.add(i, si, e.ratio, e.em1, BESO_STEP_DDIM);
        } else if (sampler == BESO_SAMPLER_EULER || sn == 0.f) {
            // gamma = 0: sigma_hat = sigma_i; d = (x - den)/sigma_hat; x += d*(sigma_next - sigma_hat)
            p.add(i, si, si, sn - si, BESO_STEP_EULER);
        } else {
            // Heun: predictor, second evaluation at sigma_{i+1}, trapezoid corrector
            p.add(i, si, si, sn - si, BESO_STEP_HEUN_PREDICT);
            p.add(i, sn, sn, sn - si, BESO_STEP_HEUN_CORRECT);
        }
    }
    p.first.push_back((int)p.ev.size());
    return p;
}

// beso_sample_ancestral: an Euler step to sigma_down, then the step's noise times sigma_up while sigma_down > 0 (:240-247)
static Plan plan_ancestral(const float* sigmas, int n_sigmas, float eta) {
    Plan p;
    for (int i = 0; i + 1 < n_sigmas; ++i) {
        const float sf = sigmas[i];
        float down, up;
        ancestral_step(sf, sigmas[i + 1], eta, down, up);
        p.first.push_back((int)p.ev.size());
        p.add(i, sf, sf, down - sf, BESO_STEP_EULER | (down > 0.f ? kStepAddNoise : 0), up);
    }
    p.first.push_back((int)p.ev.size());
    return p;
}

// beso_sample_solver's six loops (include/beso_hip.h lists their reference lines)
static Plan plan_solver(int solver, const float* sigmas, int n_sigmas, float eta, float s_noise, int order) {
    Plan p;
    for (int i = 0; i + 1 < n_sigmas; ++i) {
        const float si = sigmas[i], sn = sigmas[i + 1];
        p.first.push_back((int)p.ev.size());
        if (solver == BESO_SOLVER_DPM_2 || solver == BESO_SOLVER_DPM_2_ANCESTRAL) {
            float to = sn, up = 0.f;
            if (solver == BESO_SOLVER_DPM_2_ANCESTRAL) ancestral_step(si, sn, eta, to, up);
            if (to == 0.f) {
                p.add(i, si, si, to - si, BESO_STEP_EULER);
            } else {
                const float mid = log_midpoint(si, to);
                p.add(i, si, si, mid - si, kStepDpm2Predict);
                p.add(i, mid, mid, to - si, kStepDpm2Correct | (solver == BESO_SOLVER_DPM_2_ANCESTRAL ? kStepAddNoise : 0), up);
            }
        } else if (solver == BESO_SOLVER_DPMPP_2S || solver == BESO_SOLVER_DPMPP_2S_ANCESTRAL) {
            float to = sn, up = 0.f;
            const bool anc = solver == BESO_SOLVER_DPMPP_2S_ANCESTRAL;
            if (anc) ancestral_step(si, sn, eta, to, up);
            const int nz = anc ? kStepScaledNoise : 0;       // every step of the ancestral form draws, the last one included
            if (to == 0.f) {
                p.add(i, si, si, to - si, BESO_STEP_EULER | nz, up, s_noise);
            } else {
                // _dpmpp_2s_update: r = 1/2, s = t + r h, stage 1 to sigma = exp(-s), stage 2 from x to sigma_to
                const ExpStep e = exp_step(si, to);
                const float rh = e.h * 0.5f;
                const float smid = expf(-(e.t + rh));
                p.add(i, si, smid / expf(-e.t), expm1f(-rh), kStepExpPredict);
                p.add(i, smid, e.ratio, e.em1, kStepExpCorrect | nz, up, s_noise);
            }
        } else if (solver == BESO_SOLVER_DPMPP_2M) {
            const ExpStep e = exp_step(si, sn);
            if (i == 0 || sn == 0.f) {
                p.add(i, si, e.ratio, e.em1, i == 0 ? kStepDpm2mFirst : BESO_STEP_DDIM);
            } else {
                const float tp = -logf(sigmas[i - 1]);
                const float r = (e.t - tp) / e.h;
                const float c3 = 1.0f / (2.0f * r);
                p.add(i, si, e.ratio, e.em1, kStepDpm2m, 1.0f + c3, c3);
            }
        } else {
            const int cur = i + 1 < order ? i + 1 : order;
            float c[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < cur; ++j) c[j] = (float)lms_coeff(cur, sigmas, i, j);
            p.add(i, si, c[0], c[1], lms_mode(cur - 1, order - 1), c[2], c[3]);
        }
    }
    p.first.push_back((int)p.ev.size());
    return p;
}

// The arguments the three sampler entry points share; sample_prologue fills the rest
struct SampleCall {
    const beso_config* cfg; const void* packed; int precision; const float* state; const float* goal; float* x;
    int batch, t; const float* sigmas; int n_sigmas; float cond_lambda; int flags;
    const float* noise; float* history;           // (beso_sample_ancestral / beso_sample_solver)
    void* workspace; size_t workspace_bytes; hipStream_t s;
    float* trace_x = nullptr; size_t trace_x_floats = 0;         // (beso_sample_traced: the trajectory outputs and their
    float* trace_den = nullptr; size_t trace_den_floats = 0;     //  capacities in floats; null: not recorded)
    Layout lay; Workspace ws; FwdArgs a;          // the forward of the loop at x
};

// The checks every sampler entry point makes, in one order: config -> arguments and flags (`args_ok`: the entry point's own
// checks) -> batch / t -> layout -> workspace shape and bytes -> interior sigmas -> packed / state / goal.
static int sample_prologue(SampleCall& c, bool args_ok) {
    int st = validate_config(c.cfg);
    if (st != BESO_OK) return st;
    if (!args_ok || (c.flags & ~(BESO_SAMPLE_STEPWISE | BESO_PLAN_MASK)) || !c.sigmas || c.n_sigmas < 2 || !c.x || !c.workspace)
        return BESO_ERR_BAD_ARG;
    if (c.batch < 1 || c.t < 1 || c.t > c.cfg->obs_seq_len) return BESO_ERR_BAD_SHAPE;
    if (!make_layout(c.cfg, c.precision, &c.lay)) return BESO_ERR_BAD_ARG;
    const int two = (c.cond_lambda != 0.f && c.cond_lambda != 1.f) ? 1 : 0;
    if (!make_workspace(c.cfg, c.lay, c.batch, c.t, c.precision, two, &c.ws)) return BESO_ERR_BAD_SHAPE;
    if (c.workspace_bytes < c.ws.total) return BESO_ERR_WORKSPACE;
    for (int i = 0; i + 1 < c.n_sigmas; ++i) if (!(c.sigmas[i] > 0.f)) return BESO_ERR_BAD_ARG;
    if (!c.packed || !c.state || (c.cfg->goal_seq_len > 0 && !c.goal)) return BESO_ERR_BAD_ARG;
    FwdArgs& a = c.a;
    a.state = c.state; a.action = c.x; a.goal = c.goal; a.sigma = (float*)((char*)c.workspace + c.ws.sig); a.out = c.x;
    a.batch = c.batch; a.vbatch = two ? 2 * c.batch : c.batch; a.t = c.t; a.T = 1 + c.lay.G + 2 * c.t;
    a.precondition = 1;
    a.uncond_from = two ? c.batch : (c.cond_lambda == 0.f ? 0 : a.vbatch);
    a.cond_lambda = c.cond_lambda; a.sigma_data = c.cfg->sigma_data;
    a.plan = c.flags & BESO_PLAN_MASK;
    if (c.precision == BESO_PREC_FP16) a.plan &= ~(BESO_PLAN_PER_OP | BESO_PLAN_BLOCKS);      // (fp16 has no per-op / block form)
    // the trajectory outputs: n_sigmas slabs of x, n_sigmas - 1 of the denoised values; the loop updates x in place while the
    // slabs are written, so neither may overlap it
    const size_t n = (size_t)c.batch * c.t * c.lay.act;
    const size_t need_x = (size_t)c.n_sigmas * n, need_den = (size_t)(c.n_sigmas - 1) * n;
    if ((c.trace_x && c.trace_x_floats < need_x) || (c.trace_den && c.trace_den_floats < need_den)) return BESO_ERR_WORKSPACE;
    // ... nor each other, the workspace or the steps' noise (all written or read while the slabs are written)
    auto overlap = [](const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
        return a && b && (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
    };
    const size_t f = sizeof(float);
    const struct { const void* p; size_t bytes; } others[] = {{c.x, n * f}, {c.workspace, c.ws.total}, {c.noise, need_den * f}};
    for (const auto& o : others)
        if (overlap(c.trace_x, need_x * f, o.p, o.bytes) || overlap(c.trace_den, need_den * f, o.p, o.bytes)) return BESO_ERR_BAD_ARG;
    if (overlap(c.trace_x, need_x * f, c.trace_den, need_den * f)) return BESO_ERR_BAD_ARG;
    return BESO_OK;
}

// Runs a plan.  Where the shape has the one-launch kernel: ONE launch for the whole loop (K8 fused into K7: the workgroup that
// owns a sample from the embedding to the head also applies the update and feeds itself the next input), cut at step
// boundaries past kMaxLoopEvals evaluations -- x travels through `x`, two-evaluation steps park x there between their
// evaluations, Heun's slope lives in the workspace's d1 and the multistep state in `history`, the noise is indexed by step.
// The trajectory outputs (SampleCall::trace_x / trace_den) are written by the launches that run anyway -- the loop's head, or
// the update kernel of the step-by-step form; slab 0 of trace_x, the caller's x_T, is one copy in front of them.
// (Few samples: every evaluation runs on the chip-wide small-batch path, step by step -- one workgroup carrying a sample group
// through the whole loop would stream all the weights alone, evaluation after evaluation.)
static int run_plan(const SampleCall& c, const Plan& p) {
    char* wsp = (char*)c.workspace;
    float* den = (float*)(wsp + c.ws.den);
    float* x2 = (float*)(wsp + c.ws.x2);
    float* d1 = (float*)(wsp + c.ws.d1);
    float* sig = (float*)(wsp + c.ws.sig);
    const size_t n = (size_t)c.batch * c.t * c.lay.act;
    const FusedUnit fu = fused_unit(c.precision);
    if (c.trace_x) HIP_TRY(hipMemcpyAsync(c.trace_x, c.x, n * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    if (!(c.flags & BESO_SAMPLE_STEPWISE) && !small_wanted(c.lay, c.a, c.precision) &&
        fu.can_loop(c.lay, c.a, fu.precision)) {
        FwdArgs a = c.a;
        a.aux = c.history ? c.history : d1;
        const size_t n_steps = p.first.size() - 1;
        for (size_t i0 = 0, i1; i0 < n_steps; i0 = i1) {
            i1 = i0 + 1;
            while (i1 < n_steps && p.first[i1 + 1] - p.first[i0] <= kMaxLoopEvals) ++i1;
            SampleSteps S{};
            SampleExtra X3{};
            S.n = p.first[i1] - p.first[i0];
            for (int k = 0; k < S.n; ++k) {
                const PlanEval& e = p.ev[p.first[i0] + k];
                S.rec[k] = e.rec;
                S.rec[k].mode |= (e.step - (int)i0) << kStepShift;
                X3.c3[k] = e.c3;
            }
            a.noise = c.noise ? c.noise + i0 * n : nullptr;
            // (slab i0 + 1 of trace_x is x behind the launch's first step, slab i0 of trace_den that step's denoised value)
            const SampleTrace TR{c.trace_x ? c.trace_x + (i0 + 1) * n : nullptr, c.trace_den ? c.trace_den + i0 * n : nullptr};
            profile_begin(BESO_SITE_FUSED_LAYER, c.s);
            const int st = fu.layers(c.lay, (const char*)c.packed, a, (float*)(wsp + c.ws.x), nullptr, fu.precision, c.s, &S, &X3,
                                     &TR);
            profile_end(BESO_SITE_FUSED_LAYER, c.s);
            if (st != BESO_OK) return st;
        }
        return BESO_OK;
    }
    // step by step: per evaluation the forward (at x, or at x2 for the second stage of a step) and one update launch, which
    // also writes the sigma vector of the next evaluation (the first one is a fill); x2 / den / d1 are the workspace's, x
    // stays parked in place
    uint32_t bits; memcpy(&bits, &p.ev[0].rec.sigma, 4);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)sig, (int)bits, (size_t)c.batch, c.s));
    for (size_t k = 0; k < p.ev.size(); ++k) {
        const PlanEval& e = p.ev[k];
        const int mode = e.rec.mode & 0xff;
        const int st = forward(c.cfg, c.packed, c.precision, c.state, step_unparks(mode) ? x2 : c.x, c.goal, sig, den, c.batch, c.t,
                               c.flags & BESO_PLAN_MASK, c.cond_lambda, 1, c.workspace, c.workspace_bytes, c.s);
        if (st != BESO_OK) return st;
        SolverStepArgs sv;
        sv.c2 = e.rec.c2; sv.c3 = e.c3; sv.sigma = e.rec.sigma;
        sv.noise = c.noise ? c.noise + (size_t)e.step * n : nullptr;
        sv.hist = c.history;
        sv.trace_x = c.trace_x ? c.trace_x + (size_t)(e.step + 1) * n : nullptr;
        sv.trace_den = c.trace_den ? c.trace_den + (size_t)e.step * n : nullptr;
        const bool more = k + 1 < p.ev.size();
        HIP_TRY(launch_sampler_step(e.rec.mode, step_parks(mode) ? x2 : c.x, d1, c.x, x2, den, e.rec.c0, e.rec.c1, n, c.s,
                                    more ? sig : nullptr, more ? p.ev[k + 1].rec.sigma : 0.f, c.batch, sv));
    }
    return BESO_OK;
}

// The three sampler entry points (beso_sample_traced runs the same three with the trajectory outputs set in `c`)
static int sample_basic(SampleCall& c, int sampler) {
    const int st = sample_prologue(c, sampler >= BESO_SAMPLER_DDIM && sampler <= BESO_SAMPLER_HEUN);
    return st != BESO_OK ? st : run_plan(c, plan_sample(sampler, c.sigmas, c.n_sigmas));
}

static int sample_ancestral(SampleCall& c, float eta) {
    const int st = sample_prologue(c, c.noise && eta >= 0.f);
    return st != BESO_OK ? st : run_plan(c, plan_ancestral(c.sigmas, c.n_sigmas, eta));
}

static int sample_solver(SampleCall& c, int solver, float eta, float s_noise, int order) {
    const bool ancestral = solver == BESO_SOLVER_DPM_2_ANCESTRAL || solver == BESO_SOLVER_DPMPP_2S_ANCESTRAL;
    const bool lms_ok = solver != BESO_SOLVER_LMS || (order >= 1 && order <= 4);
    const int n_hist = solver == BESO_SOLVER_DPMPP_2M ? 1 : solver == BESO_SOLVER_LMS ? order - 1 : 0;
    const bool args_ok = solver >= BESO_SOLVER_DPM_2 && solver <= BESO_SOLVER_LMS && lms_ok && (!ancestral || c.noise) &&
                         (n_hist <= 0 || c.history) && eta >= 0.f;
    const int st = sample_prologue(c, args_ok);
    return st != BESO_OK ? st : run_plan(c, plan_solver(solver, c.sigmas, c.n_sigmas, eta, s_noise, order));
}

}  // namespace beso

using namespace beso;

extern "C" {

const char* beso_version(void) { return "beso_hip 0.1 (gfx950)"; }

const char* beso_last_error(void) { return g_last_error; }

const char* beso_status_string(int st) {
    switch (st) {
        case BESO_OK: return "ok";
        case BESO_ERR_BAD_CONFIG: return "bad model config";
        case BESO_ERR_BAD_SHAPE: return "bad shape (batch/t out of range; t must be <= obs_seq_len)";
        case BESO_ERR_BAD_ARG: return "bad argument (null pointer or unknown enum)";
        case BESO_ERR_WORKSPACE: return "workspace or packed buffer too small";
        case BESO_ERR_UNSUPPORTED: return "unsupported configuration";
        case BESO_ERR_HIP: return "HIP runtime error";
        default: return "unknown status";
    }
}

int beso_num_params(const beso_config* cfg) {
    if (validate_config(cfg) != BESO_OK) return 0;
    return ModelParams(cfg).count;
}

size_t beso_packed_bytes(const beso_config* cfg, int precision) {
    Layout lay;
    if (!make_layout(cfg, precision, &lay)) return 0;
    return lay.total;
}

int beso_pack_weights(const beso_config* cfg, const float* const* p, int n_params, void* packed_v,
                      size_t packed_bytes, int precision, void* stream) {
    int st = validate_config(cfg);
    if (st != BESO_OK) return st;
    Layout lay;
    if (!make_layout(cfg, precision, &lay)) return BESO_ERR_BAD_ARG;
    if ((precision == BESO_PREC_BF16X3 || precision == BESO_PREC_FP16) && lay.fused == lay.total)
        return BESO_ERR_UNSUPPORTED;   // no fused instance for this shape
    if (!p || !packed_v) return BESO_ERR_BAD_ARG;
    ModelParams m(cfg);
    if (m.read(p, n_params) != BESO_OK) return BESO_ERR_BAD_ARG;
    if (packed_bytes < lay.total) return BESO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* pk = (char*)packed_v;
    const int D = lay.D;
    // one tensor into the section at `off`, zero padded to [rp][cp]; prec -1: an fp32 section
    auto pack = [&](const Param& x, size_t off, int rp, int cp, int prec) {
        return launch_pack_matrix(x.p, x.rows, x.cols, pk + off, rp, cp, prec, s);
    };
    auto pack32 = [&](const Param& x, size_t off) { return pack(x, off, x.rows, x.cols, -1); };
    // (the GEMM operands of the per-op path are not used by BF16X3 / FP16: their weights live in the fused image only)
    const bool operands = precision != BESO_PREC_BF16X3 && precision != BESO_PREC_FP16;
    auto packw = [&](const Param& x, size_t off, int rp, int cp) { return operands ? pack(x, off, rp, cp, precision) : hipSuccess; };
    HIP_TRY(pack32(m.pos, lay.pos_emb)); HIP_TRY(pack32(m.tokw, lay.tok_w)); HIP_TRY(pack32(m.tokb, lay.tok_b));
    for (int l = 0; l < lay.L; ++l) {
        const LayerOff& o = lay.layer[l];
        const LayerParams& y = m.layer[l];
        HIP_TRY(pack32(y.ln1w, o.ln1_w)); HIP_TRY(pack32(y.ln1b, o.ln1_b));
        HIP_TRY(pack32(y.ln2w, o.ln2_w)); HIP_TRY(pack32(y.ln2b, o.ln2_b));
        const Qkv qkv = y.qkv();
        const size_t e = lay.elem_bytes;
        // zero the whole padded operand first (rows 3D..Nqkv), then drop q,k,v in
        HIP_TRY(hipMemsetAsync(pk + o.w_qkv, 0, e * lay.Nqkv * lay.Kd, s));
        HIP_TRY(hipMemsetAsync(pk + o.b_qkv, 0, sizeof(float) * lay.Nqkv, s));
        for (int part = 0; part < 3; ++part) HIP_TRY(packw(qkv.w[part], o.w_qkv + e * (size_t)part * D * lay.Kd, D, lay.Kd));
        for (int part = 0; part < 3; ++part) HIP_TRY(pack32(qkv.b[part], o.b_qkv + sizeof(float) * part * D));
        HIP_TRY(packw(y.pw, o.w_proj, lay.Nd, lay.Kd));
        HIP_TRY(pack(y.pb, o.b_proj, 1, lay.Nd, -1));
        HIP_TRY(packw(y.f1w, o.w_fc1, lay.Nh, lay.Kd));
        HIP_TRY(pack(y.f1b, o.b_fc1, 1, lay.Nh, -1));
        HIP_TRY(packw(y.f2w, o.w_fc2, lay.Nd, lay.Kh));
        HIP_TRY(pack(y.f2b, o.b_fc2, 1, lay.Nd, -1));
    }
    HIP_TRY(pack32(m.lnfw, lay.lnf_w)); HIP_TRY(pack32(m.lnfb, lay.lnf_b));
    HIP_TRY(pack32(m.sigw, lay.sig_w)); HIP_TRY(pack32(m.sigb, lay.sig_b));
    HIP_TRY(pack32(m.actw, lay.act_w)); HIP_TRY(pack32(m.actb, lay.act_b));
    // (the linear head's tensors are the image's head_w1 = head_w0 and head_b1 = head_b0)
    if (!lay.linear_output) { HIP_TRY(pack32(m.h0w, lay.head_w0)); HIP_TRY(pack32(m.h0b, lay.head_b0)); }
    HIP_TRY(pack32(m.hw, lay.head_w1)); HIP_TRY(pack32(m.hb, lay.head_b1));
    const FusedUnit fu = fused_unit(precision);
    return fu.pack(lay, m, pk, fu.precision, s);
}

size_t beso_workspace_bytes(const beso_config* cfg, int batch, int t, int precision, int cfg_guidance) {
    Layout lay;
    Workspace ws;
    if (!make_layout(cfg, precision, &lay)) return 0;
    if (!make_workspace(cfg, lay, batch, t, precision, cfg_guidance, &ws)) return 0;
    return ws.total;
}

int beso_score_fwd(const beso_config* cfg, const void* packed, int precision, const float* state,
                   const float* action, const float* goal, const float* sigma, float* out, int batch, int t,
                   int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return forward(cfg, packed, precision, state, action, goal, sigma, out, batch, t, flags, 1.0f, 0, workspace,
                   workspace_bytes, (hipStream_t)stream);
}

int beso_denoise_fwd(const beso_config* cfg, const void* packed, int precision, const float* state,
                     const float* action, const float* goal, const float* sigma, float* out, int batch, int t,
                     int flags, float cond_lambda, void* workspace, size_t workspace_bytes, void* stream) {
    return forward(cfg, packed, precision, state, action, goal, sigma, out, batch, t, flags, cond_lambda, 1,
                   workspace, workspace_bytes, (hipStream_t)stream);
}

int beso_sampler_step(int mode, float* out, float* aux, const float* x, const float* x2, const float* den,
                      float c0, float c1, size_t n, void* stream) {
    if (mode < BESO_STEP_DDIM || mode > BESO_STEP_ADD_NOISE || !out || !x || !den) return BESO_ERR_BAD_ARG;
    if (mode == BESO_STEP_ADD_NOISE && !x2) return BESO_ERR_BAD_ARG;
    if ((mode == BESO_STEP_HEUN_PREDICT || mode == BESO_STEP_HEUN_CORRECT) && !aux) return BESO_ERR_BAD_ARG;
    if (mode == BESO_STEP_HEUN_CORRECT && !x2) return BESO_ERR_BAD_ARG;
    if (n == 0) return BESO_OK;
    HIP_TRY(launch_sampler_step(mode, out, aux, x, x2, den, c0, c1, n, (hipStream_t)stream));
    return BESO_OK;
}

int beso_sample(const beso_config* cfg, const void* packed, int precision, int sampler, const float* state,
                const float* goal, float* x, int batch, int t, const float* sigmas, int n_sigmas,
                float cond_lambda, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    SampleCall c{cfg, packed, precision, state, goal, x, batch, t, sigmas, n_sigmas, cond_lambda, flags, nullptr, nullptr,
                 workspace, workspace_bytes, (hipStream_t)stream};
    return sample_basic(c, sampler);
}

int beso_sample_ancestral(const beso_config* cfg, const void* packed, int precision, const float* state, const float* goal,
                          float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda, float eta,
                          const float* noise, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    SampleCall c{cfg, packed, precision, state, goal, x, batch, t, sigmas, n_sigmas, cond_lambda, flags, noise, nullptr,
                 workspace, workspace_bytes, (hipStream_t)stream};
    return sample_ancestral(c, eta);
}

int beso_sample_solver(const beso_config* cfg, const void* packed, int precision, int solver, const float* state,
                       const float* goal, float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda,
                       float eta, float s_noise, int order, const float* noise, float* history, int flags,
                       void* workspace, size_t workspace_bytes, void* stream) {
    SampleCall c{cfg, packed, precision, state, goal, x, batch, t, sigmas, n_sigmas, cond_lambda, flags, noise, history,
                 workspace, workspace_bytes, (hipStream_t)stream};
    return sample_solver(c, solver, eta, s_noise, order);
}

int beso_sample_traced(const beso_config* cfg, const void* packed, int precision, int entry, int sampler, const float* state,
                       const float* goal, float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda,
                       float eta, float s_noise, int order, const float* noise, float* history, float* trace_x,
                       size_t trace_x_floats, float* trace_den, size_t trace_den_floats, int flags, void* workspace,
                       size_t workspace_bytes, void* stream) {
    SampleCall c{cfg, packed, precision, state, goal, x, batch, t, sigmas, n_sigmas, cond_lambda, flags,
                 entry == BESO_ENTRY_SAMPLE ? nullptr : noise, entry == BESO_ENTRY_SOLVER ? history : nullptr,
                 workspace, workspace_bytes, (hipStream_t)stream};
    c.trace_x = trace_x; c.trace_x_floats = trace_x_floats;
    c.trace_den = trace_den; c.trace_den_floats = trace_den_floats;
    if (entry == BESO_ENTRY_SAMPLE) return sample_basic(c, sampler);
    if (entry == BESO_ENTRY_ANCESTRAL) return sample_ancestral(c, eta);
    if (entry == BESO_ENTRY_SOLVER) return sample_solver(c, sampler, eta, s_noise, order);
    return BESO_ERR_BAD_ARG;
}

#if BESO_DEV_API
// development builds only (include/beso_hip_debug.h; `python -m beso_amd.build --dev` -> libbeso_hip_dev.so)
void beso_debug_set_stamps(void* device_buf, int capacity_u64) { fused_set_stamps(device_buf, capacity_u64); }
int beso_debug_sigma_cache_entries(const beso_config* cfg, const void* packed, int precision) {
    Layout lay;
    if (!packed || validate_config(cfg) != BESO_OK || (precision != BESO_PREC_BF16 && precision != BESO_PREC_FP16) ||
        !make_layout(cfg, precision, &lay)) return -1;
    return fused_sigma_cache_entries(lay, (const char*)packed);
}
#endif

int beso_adam_step(const beso_optim_chunk* chunks, int n_chunks, float* exp_avg, float* exp_avg_sq, float* ema,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled_wd, int step,
                   float ema_decay, void* stream) {
    if (!chunks || !exp_avg || !exp_avg_sq || n_chunks < 0 || step < 1) return BESO_ERR_BAD_ARG;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f)) return BESO_ERR_BAD_ARG;
    if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return BESO_ERR_BAD_ARG;
    if (n_chunks == 0) return BESO_OK;
    hipError_t e = launch_adam_ema(chunks, n_chunks, exp_avg, exp_avg_sq, ema, lr, beta1, beta2, eps, weight_decay,
                                   decoupled_wd ? 1 : 0, step, ema_decay, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "adam_ema_kernel", __LINE__);
    return BESO_OK;
}

int beso_grad_sumsq(const beso_optim_chunk* chunks, int n_chunks, double* partial, double* stats, void* stream) {
    if (!stats || n_chunks < 0 || (n_chunks > 0 && (!chunks || !partial))) return BESO_ERR_BAD_ARG;
    hipError_t e = launch_grad_sumsq(chunks, n_chunks, partial, stats, (hipStream_t)stream);     // n_chunks == 0: stats[0] = 0
    if (e != hipSuccess) return record_hip_error(e, "grad_sumsq_kernel", __LINE__);
    return BESO_OK;
}

int beso_adam_step_clipped(const beso_optim_chunk* chunks, int n_chunks, float* exp_avg, float* exp_avg_sq, float* ema,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled_wd, int step,
                           float ema_decay, double* stats, float max_grad_norm, int skip_nonfinite, void* stream) {
    if (!chunks || !exp_avg || !exp_avg_sq || !stats || n_chunks < 0 || step < 1) return BESO_ERR_BAD_ARG;
    if (!(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && lr >= 0.f)) return BESO_ERR_BAD_ARG;
    if (ema && !(ema_decay >= 0.f && ema_decay <= 1.f)) return BESO_ERR_BAD_ARG;
    if (!(max_grad_norm > 0.f)) return BESO_ERR_BAD_ARG;                                        // NaN too; +inf = do not clip
    if (n_chunks == 0) return BESO_OK;
    hipError_t e = launch_adam_ema_clipped(chunks, n_chunks, exp_avg, exp_avg_sq, ema, lr, beta1, beta2, eps, weight_decay,
                                           decoupled_wd ? 1 : 0, step, ema_decay, stats, max_grad_norm,
                                           skip_nonfinite ? 1 : 0, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "adam_ema_clipped_kernel", __LINE__);
    return BESO_OK;
}

int beso_gather_windows(const float* observations, const float* actions, const int* seq_len, int n_traj, int t_max,
                        int obs_dim, int act_dim, const int* slice_traj, const int* slice_start, long long n_slices,
                        const long long* batch_slices, const long long* draws, int batch, int window, int goal_len,
                        int goal_mode, int min_future_sep, float* obs_out, float* act_out, float* goal_out, void* stream) {
    if (!observations || !actions || !seq_len || !slice_traj || !slice_start || !batch_slices || !obs_out || !act_out)
        return BESO_ERR_BAD_ARG;
    if (n_traj < 1 || t_max < 1 || obs_dim < 1 || act_dim < 1 || n_slices < 1 || batch < 0 || window < 1 || window > t_max)
        return BESO_ERR_BAD_ARG;
    if (goal_len < 0 || goal_len > t_max || min_future_sep < 0) return BESO_ERR_BAD_ARG;
    if (goal_mode != BESO_GOAL_RANDOM && goal_mode != BESO_GOAL_TAIL && goal_mode != BESO_GOAL_SEQ_END) return BESO_ERR_BAD_ARG;
    if (goal_len > 0 && (!goal_out || (goal_mode == BESO_GOAL_RANDOM && !draws))) return BESO_ERR_BAD_ARG;
    if ((long long)window * (obs_dim > act_dim ? obs_dim : act_dim) > 0x7fffffffLL) return BESO_ERR_BAD_ARG;
    if (batch == 0) return BESO_OK;
    hipError_t e = launch_gather_windows(observations, actions, seq_len, n_traj, t_max, obs_dim, act_dim, slice_traj,
                                         slice_start, n_slices, batch_slices, draws, batch, window, goal_len, goal_mode,
                                         min_future_sep, obs_out, act_out, goal_out, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "gather_windows_kernel", __LINE__);
    return BESO_OK;
}

int beso_rollout_begin(const float* obs, const uint8_t* reset, const float* noise, const float* mean, const float* den,
                       float sigma_max, int32_t* lengths, float* obs_ctx, float* act_ctx, float* state_out, float* x_out,
                       int n_envs, int window, int obs_dim, int act_dim, void* stream) {
    if (!obs || !noise || !lengths || !obs_ctx || !act_ctx || !state_out || !x_out || (!mean) != (!den)) return BESO_ERR_BAD_ARG;
    if (n_envs < 0 || window < 1 || obs_dim < 1 || act_dim < 1) return BESO_ERR_BAD_ARG;
    if ((long long)window * ((long long)obs_dim + act_dim) * (n_envs > 1 ? n_envs : 1) > 0x7fffffffLL) return BESO_ERR_BAD_ARG;
    if (n_envs == 0) return BESO_OK;
    hipError_t e = launch_rollout_begin(obs, reset, noise, mean, den, sigma_max, lengths, obs_ctx, act_ctx, state_out, x_out,
                                        n_envs, window, obs_dim, act_dim, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "rollout_begin_kernel", __LINE__);
    return BESO_OK;
}

int beso_rollout_end(const float* x0, const int32_t* lengths, const double* lo, const double* hi, const float* den_y,
                     const float* mean_y, float* act_ctx, float* pred, int n_envs, int window, int act_dim, void* stream) {
    if (!x0 || !lengths || !lo || !hi || !act_ctx || !pred || (!den_y) != (!mean_y)) return BESO_ERR_BAD_ARG;
    if (n_envs < 0 || window < 1 || act_dim < 1) return BESO_ERR_BAD_ARG;
    if ((long long)window * act_dim * (n_envs > 1 ? n_envs : 1) > 0x7fffffffLL) return BESO_ERR_BAD_ARG;
    if (n_envs == 0) return BESO_OK;
    hipError_t e = launch_rollout_end(x0, lengths, lo, hi, den_y, mean_y, act_ctx, pred, n_envs, window, act_dim,
                                      (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "rollout_end_kernel", __LINE__);
    return BESO_OK;
}

size_t beso_train_workspace_bytes(const beso_config* cfg, int batch, int t, int precision) {
    return train_workspace_bytes(cfg, batch, t, precision);
}

size_t beso_grad_floats(const beso_config* cfg) { return train_grad_floats(cfg); }

int beso_loss_grad_inputs(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                          const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                          float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                          float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                          void* stream, void* early_stream, void* loss_stream, float* state_grad, float* goal_grad) {
    hipError_t e = hipSuccess;
    int line = 0;
    int st = train_loss_grad(cfg, params, n_params, grads_flat, precision, state, action, goal, noise, sigma, loss_out, batch,
                             t, flags, embed_pdrop, attn_pdrop, resid_pdrop, goal_drop, seed, grad_scale, workspace, workspace_bytes, (hipStream_t)stream,
                             (hipStream_t)early_stream, (hipStream_t)loss_stream, state_grad, goal_grad, &e, &line);
    if (st == BESO_ERR_HIP) {
        snprintf(g_last_error, sizeof(g_last_error), "%s (%d) at train.hip:%d", hipGetErrorName(e), (int)e, line);
    }
    return st;
}

int beso_loss_grad_streams(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                           const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                           float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                           float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream, void* early_stream, void* loss_stream) {
    return beso_loss_grad_inputs(cfg, params, n_params, grads_flat, precision, state, action, goal, noise, sigma, loss_out, batch, t,
                                 flags, embed_pdrop, attn_pdrop, resid_pdrop, goal_drop, seed, grad_scale, workspace, workspace_bytes,
                                 stream, early_stream, loss_stream, nullptr, nullptr);
}

int beso_loss_grad_overlap(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                           const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                           float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                           float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream, void* early_stream) {
    return beso_loss_grad_streams(cfg, params, n_params, grads_flat, precision, state, action, goal, noise, sigma, loss_out, batch, t,
                                  flags, embed_pdrop, attn_pdrop, resid_pdrop, goal_drop, seed, grad_scale, workspace,
                                  workspace_bytes, stream, early_stream, nullptr);
}

int beso_loss_grad(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                   const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                   float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                   float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return beso_loss_grad_overlap(cfg, params, n_params, grads_flat, precision, state, action, goal, noise, sigma, loss_out, batch, t,
                                  flags, embed_pdrop, attn_pdrop, resid_pdrop, goal_drop, seed, grad_scale, workspace, workspace_bytes,
                                  stream, nullptr);
}

int beso_denoise_vjp_inputs(const beso_config* cfg, const float* const* params, int n_params, int precision, const float* state,
                            const float* x, const float* goal, const float* sigma, const float* cot, float* denoised, float* x_grad,
                            float* dot, int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream,
                            float* state_grad, float* goal_grad) {
    hipError_t e = hipSuccess;
    int line = 0;
    int st = train_denoise_vjp(cfg, params, n_params, precision, state, x, goal, sigma, cot, denoised, x_grad, dot, batch, t, flags,
                               workspace, workspace_bytes, (hipStream_t)stream, state_grad, goal_grad, &e, &line);
    if (st == BESO_ERR_HIP) {
        snprintf(g_last_error, sizeof(g_last_error), "%s (%d) at train.hip:%d", hipGetErrorName(e), (int)e, line);
    }
    return st;
}

int beso_denoise_vjp(const beso_config* cfg, const float* const* params, int n_params, int precision, const float* state,
                     const float* x, const float* goal, const float* sigma, const float* cot, float* denoised, float* x_grad,
                     float* dot, int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    return beso_denoise_vjp_inputs(cfg, params, n_params, precision, state, x, goal, sigma, cot, denoised, x_grad, dot, batch, t,
                                   flags, workspace, workspace_bytes, stream, nullptr, nullptr);
}

size_t beso_loss_fwd_workspace_bytes(const beso_config* cfg, int batch, int t, int precision) {
    LossWorkspace w;
    return loss_workspace(cfg, batch, t, precision, &w) ? w.total : 0;
}

int beso_loss_fwd(const beso_config* cfg, const void* packed, int precision, const float* state, const float* action,
                  const float* goal, const float* noise, const float* sigma, float* loss_out, float* per_sample_out,
                  int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    int st = validate_config(cfg);
    if (st != BESO_OK) return st;
    if (precision != BESO_PREC_BF16 && precision != BESO_PREC_FP32 && precision != BESO_PREC_BF16X3 && precision != BESO_PREC_FP16)
        return BESO_ERR_BAD_ARG;
    if (flags & ~(BESO_FLAG_UNCOND | BESO_PLAN_MASK | BESO_FLAG_LAST_ACTION_ONLY)) return BESO_ERR_BAD_ARG;
    if (batch < 1 || t < 1 || t > cfg->obs_seq_len) return BESO_ERR_BAD_SHAPE;
    if (!packed || !state || !action || !noise || !sigma || !workspace || (cfg->goal_seq_len > 0 && !goal)) return BESO_ERR_BAD_ARG;
    if (!loss_out && !per_sample_out) return BESO_ERR_BAD_ARG;
    LossWorkspace w;
    if (!loss_workspace(cfg, batch, t, precision, &w)) return BESO_ERR_BAD_SHAPE;
    if (workspace_bytes < w.total) return BESO_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    char* wsp = (char*)workspace;
    float* scaled = (float*)(wsp + w.scaled);
    float* pred = (float*)(wsp + w.pred);
    float* rows = per_sample_out ? per_sample_out : (float*)(wsp + w.rows);
    const int fwd_flags = flags & (BESO_FLAG_UNCOND | BESO_PLAN_MASK);
    // the forward's own checks (a shape this precision has no kernel for) before the first launch of this call
    st = forward_supported(cfg, precision, batch, t, fwd_flags);
    if (st != BESO_OK) return st;
    HIP_TRY(launch_loss_prep(action, noise, sigma, scaled, batch, t, cfg->act_dim, cfg->sigma_data, s));
    // DiffusionGPT.forward at c_in * noised: the reference's operation order (score_wrappers.py:74)
    st = forward(cfg, packed, precision, state, scaled, goal, sigma, pred, batch, t, fwd_flags, 1.0f, 0, workspace, w.forward, s);
    if (st != BESO_OK) return st;
    HIP_TRY(launch_loss_reduce(pred, action, noise, sigma, rows, loss_out, batch, t, cfg->act_dim,
                               (flags & BESO_FLAG_LAST_ACTION_ONLY) ? 1 : 0, cfg->sigma_data, s));
    return BESO_OK;
}

int beso_log_logistic(const double* u, float* out, size_t n, double loc, double scale, double cdf_lo, double cdf_hi, void* stream) {
    if (!u || !out || !(scale > 0.0) || !(cdf_lo >= 0.0 && cdf_hi <= 1.0 && cdf_lo <= cdf_hi)) return BESO_ERR_BAD_ARG;
    if (n == 0) return BESO_OK;
    hipError_t e = launch_log_logistic(u, out, n, loc, scale, cdf_lo, cdf_hi, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "log_logistic_kernel", __LINE__);
    return BESO_OK;
}

int beso_scale_rows(const float* const* src, float* const* dst, const float* const* mean, const float* const* den,
                    const long long* rows, const int* cols, int n, void* stream) {
    if (n < 0 || n > kScaleMax || (n > 0 && (!src || !dst || !mean || !den || !rows || !cols))) return BESO_ERR_BAD_ARG;
    for (int k = 0; k < n; ++k)
        if (rows[k] < 0 || cols[k] < 1 || (rows[k] > 0 && (!src[k] || !dst[k] || !mean[k] || !den[k]))) return BESO_ERR_BAD_ARG;
    hipError_t e = launch_scale_rows(src, dst, mean, den, rows, cols, n, (hipStream_t)stream);
    if (e != hipSuccess) return record_hip_error(e, "scale_rows_kernel", __LINE__);
    return BESO_OK;
}

int beso_goal_mask(float* mask, int batch, int goal_seq_len, int obs_dim, float goal_drop, unsigned int seed, void* stream) {
    if (batch < 0 || goal_seq_len < 0 || obs_dim < 0) return BESO_ERR_BAD_ARG;
    hipError_t e = hipSuccess;
    int line = 0;
    int st = train_goal_mask(mask, (size_t)batch * goal_seq_len * obs_dim, goal_drop, seed, (hipStream_t)stream, &e, &line);
    if (st == BESO_ERR_HIP) snprintf(g_last_error, sizeof(g_last_error), "%s (%d) at train.hip:%d", hipGetErrorName(e), (int)e, line);
    return st;
}

int beso_dropout_mask(const beso_config* cfg, float* scale, int kind, int layer, int batch, int t, float p, unsigned int seed,
                      void* stream) {
    hipError_t e = hipSuccess;
    int line = 0;
    int st = train_dropout_mask(cfg, scale, kind, layer, batch, t, p, seed, (hipStream_t)stream, &e, &line);
    if (st == BESO_ERR_HIP) snprintf(g_last_error, sizeof(g_last_error), "%s (%d) at train.hip:%d", hipGetErrorName(e), (int)e, line);
    return st;
}

int beso_grad_early_range(const beso_config* cfg, size_t* begin, size_t* end) {
    if (!cfg || !begin || !end) return BESO_ERR_BAD_ARG;
    int st = train_validate(cfg, 1, 1);
    if (st != BESO_OK) return st;
    train_early_range(cfg, begin, end);
    return BESO_OK;
}

#if BESO_DEV_API
int beso_debug_gemm(int precision, int a_kslow, int b_kslow, const void* A, int lda, const void* B, int ldb, float* C,
                    int ldc, int M, int N, int K, int splits, void* stream) {
    hipError_t e = hipSuccess;
    int line = 0;
    int st = train_debug_gemm(precision, a_kslow, b_kslow, A, lda, B, ldb, C, ldc, M, N, K, splits, (hipStream_t)stream, &e,
                              &line);
    if (st == BESO_ERR_HIP) {
        snprintf(g_last_error, sizeof(g_last_error), "%s (%d) at train.hip:%d", hipGetErrorName(e), (int)e, line);
    }
    return st;
}
#endif

void beso_profile_enable(int site) { g_prof_site = site; }

int beso_profile_read(double* total_ms, int* launches) {
    double tot = 0.0;
    int n = 0;
    for (auto& pr : g_prof_events) {
        if (hipEventSynchronize(pr.second) != hipSuccess) return BESO_ERR_HIP;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { tot += ms; ++n; }
        g_prof_free.push_back(pr.first);
        g_prof_free.push_back(pr.second);
    }
    g_prof_events.clear();
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
    return BESO_OK;
}

}  // extern "C"
