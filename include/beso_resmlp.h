/*
 * beso_resmlp.h -- C ABI of libbeso_resmlp.so: the reference's networks/mlps/mlps.py::ResidualMLPNetwork (lines 76-133) over
 * the pre-activation residual blocks of networks/mlps/res_layers.py, forward and backward, on the MI355X (gfx950): the
 * stronger trainable observation / goal encoder beside include/beso_mlp.h's plain MLP.
 *
 * The network, applied row-wise to x [M, in]:
 *     u_0 = Linear(in, hidden)(x)
 *     for b in 0 .. n_blocks - 1:   v_b = l1_b(act(norm_b(u_b)));   u_{b+1} = l2_b(act(norm_b(v_b))) + u_b
 *     y = Linear(hidden, out)(u_{n_blocks})
 * There is no activation outside the blocks.  norm_b is the identity (BESO_RESMLP_NORM_NONE) or ONE LayerNorm(hidden,
 * eps = 1e-6, biased variance) per block applied at both places (BESO_RESMLP_NORM_LAYER): its gamma and beta receive gradient
 * from both uses.  BatchNorm, spectral norm and dropout masks are not provided.
 *
 * Conventions are those of include/beso_mlp.h: plain C, device pointers owned by the caller, contiguous fp32, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state.  Return value: a status of include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2,
 * BESO_ERR_BAD_ARG = -3, BESO_ERR_WORKSPACE = -4, BESO_ERR_HIP = -6).  Everything is checked before anything is enqueued.
 * Buffers the library writes (y, keep, dx, grads_flat without BESO_MLP_ACCUMULATE, the workspace) may hold anything on entry;
 * every element of a result is written and nothing outside a buffer's extent is.
 *
 * Arithmetic: fp32 throughout.  Every product of the GEMMs runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) with fp32
 * accumulation; the LayerNorm statistics of a row are two-pass (mean, then the mean of squared deviations), each reduced over
 * the 16 lanes that own the row in a fixed order; no atomics anywhere: the same inputs give the same bits, and a row of the
 * forward depends on that row alone.
 *
 * Supported: in_dim, out_dim in 1 ... 512; hidden_dim a multiple of 16 up to 512; n_blocks in 1 ... 4; any M >= 1.
 * Anything else is BESO_ERR_BAD_SHAPE (an unknown activation or norm: BESO_ERR_BAD_ARG).
 */
#ifndef BESO_RESMLP_H
#define BESO_RESMLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ResidualMLPNetwork.__init__ kwargs that shape the computation (mlps.py:83-95). */
typedef struct beso_resmlp_dims {
    int32_t in_dim;      /* input_dim                                                                  */
    int32_t hidden_dim;  /* hidden_dim                                                                 */
    int32_t n_blocks;    /* num_hidden_layers / 2: the residual blocks between the two outer Linears   */
    int32_t out_dim;     /* output_dim                                                                 */
    int32_t activation;  /* BESO_MLP_ACT_* of include/beso_mlp.h (0 ReLU, 1 Mish, 2 sigmoid)           */
    int32_t norm;        /* BESO_RESMLP_NORM_*                                                         */
} beso_resmlp_dims;

enum {
    BESO_RESMLP_NORM_NONE = 0,   /* use_norm = False                                                             */
    BESO_RESMLP_NORM_LAYER = 1   /* use_norm = True, norm_style = 'LayerNorm': torch.nn.LayerNorm(hidden, 1e-6)  */
};

/* Bytes of workspace beso_resmlp_bwd needs for M rows (training != 0); 0 for training == 0 (the forward takes none) and for
 * unsupported dims or M < 1.  Layout, every array [M, hidden] floats:
 *     dU_0                                      the gradient of the stream behind the first Linear (its dz)
 *     per block b:  dV_b, dU_{b+1}, A1_b, A2_b  the output gradients of l1_b and l2_b, and the inputs of l1_b and l2_b
 *                                               (A1_b = act(norm_b(u_b)), A2_b = act(norm_b(v_b)), recomputed by the chain)
 *     with a norm, per block b:  GP_b, BP_b     dn * xhat and dn summed over the block's two uses of its normalizer (dn: the
 *                                               gradient of the normalizer's output) -- their column sums are dgamma, dbeta
 * (the whole rounded up to 256 bytes), then the slab of partial sums, [S][P] floats: P the parameter count and S = ceil(M / R)
 * row ranges of R = max(256, 16 ceil(M / 1024)) rows -- the rule of beso_mlp_workspace_bytes: S <= 64 depends on M alone. */
size_t beso_resmlp_workspace_bytes(const beso_resmlp_dims* dims, long long M, int training);

/* y [M, out] = ResidualMLPNetwork.forward(x [M, in]) in eval mode.  ONE launch: a workgroup owns 16 rows and carries them
 * through all layers; three [16][pitch] tiles live in LDS (the residual stream and two ping-pong tiles), the weights are
 * streamed from memory as the MFMA's other operand.
 *   params  host array of n_params DEVICE pointers in named_parameters() order (torch layouts, fp32):
 *           layers.0.weight [hidden, in], layers.0.bias [hidden]; per block i = 1 .. n_blocks layers.i.l1.weight [hidden,
 *           hidden], layers.i.l1.bias, layers.i.l2.weight, layers.i.l2.bias and, with a norm, layers.i.normalizer.weight
 *           [hidden], layers.i.normalizer.bias; then layers.(n_blocks + 1).weight [out, hidden] and its bias [out]:
 *           n_params = 4 + 4 n_blocks (+ 2 n_blocks with a norm)
 *   keep    NULL, or (training) what beso_resmlp_bwd reads, M (in + (2 n_blocks + 1) hidden) floats:
 *           x [M, in]; u_0 .. u_{n_blocks}, each [M, hidden] (the stream at every block's entry and behind the last block);
 *           v_0 .. v_{n_blocks - 1}, each [M, hidden].  Normalised values, activations and the LayerNorm statistics are
 *           recomputed by the backward.                                                                                  */
int beso_resmlp_fwd(const float* const* params, int n_params, const beso_resmlp_dims* dims, const float* x, long long M,
                    float* y, float* keep, void* stream);

/* The gradients of a scalar L, given dy = dL/dy [M, out].  Three launches, whatever M:
 *   (1) the data-gradient chain, per 16-row tile in reverse order through the last Linear, the blocks (at both uses of a
 *       block's normalizer the activation's derivative and the LayerNorm backward; the residual add) and, with dx != NULL, the
 *       first Linear: dx [M, in].  It fills the workspace arrays listed above;
 *   (2) dW = dz^T a and db = column sums of dz of every Linear, and dgamma / dbeta as the column sums of GP_b / BP_b, as
 *       partial sums per row range into the workspace slab -- one workgroup per (parameter pair, 16 input columns, row range),
 *       the bias as one more input column that is constant 1;
 *   (3) the partial sums added in row-range order into grads_flat: the gradients of all parameters back to back in `params`
 *       order (P floats), written, or with BESO_MLP_ACCUMULATE (include/beso_mlp.h, = 1) added to as ONE addition per element.
 * The order of every addition depends on (dims, M) alone: equal bits from run to run.
 *   keep       as written by beso_resmlp_fwd for the same (params, dims, M)
 *   workspace  at least beso_resmlp_workspace_bytes(dims, M, 1) bytes, 16-byte aligned (BESO_ERR_WORKSPACE otherwise)    */
int beso_resmlp_bwd(const float* const* params, int n_params, const beso_resmlp_dims* dims, const float* keep,
                    const float* dy, long long M, float* dx, float* grads_flat, void* workspace, size_t workspace_bytes,
                    int flags, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_RESMLP_H */
