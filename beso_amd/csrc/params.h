// The model's parameter list: the only implementation of the order that include/beso_hip.h states above beso_num_params
// (the reference module's named_parameters()).  Host code only.  Every reader of a caller's `params` array -- the packers of
// api.hip and fused.hip, the training step and the gradient buffer's sizes of train.hip -- takes roles, shapes and offsets from here.
#pragma once
#include "common.h"

namespace beso {

// One tensor of the list.  A weight has its torch shape [rows][cols]; a vector is one row (sigma_emb.weight, [D][1], too).
struct Param {
    const float* p;        // the caller's tensor (ModelParams::read)
    float* g;              // its gradient (ModelParams::set_grads)
    int rows, cols;
    size_t offset;         // floats in front of it in the flat gradient buffer
    size_t count() const { return (size_t)rows * cols; }
};
struct Qkv { Param w[3], b[3]; };
struct LayerParams {
    Param ln1w, ln1b, ln2w, ln2b, kw, kb, qw, qb, vw, vb, pw, pb, f1w, f1b, f2w, f2b;
    // the list has key, query, value (score_gpts.py:33-39); every fused operand has [q | k | v]
    Qkv qkv() const { return {{qw, kw, vw}, {qb, kb, vb}}; }
};
struct ModelParams {
    const beso_config* c;
    Param pos, tokw, tokb;
    LayerParams layer[kMaxLayers];
    Param lnfw, lnfb, sigw, sigb, actw, actb;
    // action head: Linear(D, act) = hw, hb -- or Linear(D, 100) = h0w, h0b, SiLU, Linear(100, act) = hw, hb (score_gpts.py:184-191)
    Param h0w{}, h0b{}, hw, hb;
    int count = 0;         // tensors
    size_t floats = 0;     // of the flat gradient buffer

    // THE LIST: f(tensor, rows, cols) for every parameter of the model, in order
    template <typename F>
    void each(F&& f) {
        const int D = c->embed_dim, act = c->act_dim, Hh = c->linear_output ? D : kHeadHidden;
        f(pos, c->goal_seq_len + c->obs_seq_len + 1, D); f(tokw, D, c->obs_dim); f(tokb, 1, D);
        for (int l = 0; l < c->n_layers; ++l) {
            LayerParams& y = layer[l];
            f(y.ln1w, 1, D); f(y.ln1b, 1, D); f(y.ln2w, 1, D); f(y.ln2b, 1, D);
            f(y.kw, D, D); f(y.kb, 1, D); f(y.qw, D, D); f(y.qb, 1, D); f(y.vw, D, D); f(y.vb, 1, D); f(y.pw, D, D); f(y.pb, 1, D);
            f(y.f1w, 4 * D, D); f(y.f1b, 1, 4 * D); f(y.f2w, D, 4 * D); f(y.f2b, 1, D);
        }
        f(lnfw, 1, D); f(lnfb, 1, D); f(sigw, 1, D); f(sigb, 1, D); f(actw, D, act); f(actb, 1, D);
        if (!c->linear_output) { f(h0w, Hh, D); f(h0b, 1, Hh); }
        f(hw, act, Hh); f(hb, 1, act);
    }
    // shapes, offsets, count and floats of a valid config's list; no pointers yet
    explicit ModelParams(const beso_config* cfg) : c(cfg) {
        each([&](Param& x, int rows, int cols) { x = Param{nullptr, nullptr, rows, cols, floats}; floats += x.count(); ++count; });
    }
    // takes a caller's array: BESO_ERR_BAD_ARG unless it holds exactly the list's tensors, none of them null
    int read(const float* const* p, int n_params) {
        if (!p || n_params != count) return BESO_ERR_BAD_ARG;
        for (int i = 0; i < n_params; ++i) if (!p[i]) return BESO_ERR_BAD_ARG;
        each([&](Param& x, int, int) { x.p = *p++; });
        return BESO_OK;
    }
    // advance = false: every gradient pointer stays on `g_flat` (one scratch slab for a caller that wants none of them)
    void set_grads(float* g_flat, bool advance) {
        each([&](Param& x, int, int) { x.g = advance ? g_flat + x.offset : g_flat; });
    }
};

}  // namespace beso
