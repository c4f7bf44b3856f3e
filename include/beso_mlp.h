/*
 * beso_mlp.h -- C ABI of libbeso_mlp.so: the trainable MLP observation / goal encoder in front of the score network
 * (the reference's networks/mlps/mlps.py::MLPNetwork, lines 11-73), forward and backward, on the MI355X (gfx950).
 *
 * The network: Linear(in, hidden), then n_hidden - 1 layers Linear(hidden, hidden), then Linear(hidden, out); the
 * activation follows every layer but the last (mlps.py:40-66).  It is applied row-wise to x [M, in].
 *
 * Conventions are those of include/beso_hip.h: plain C, device pointers owned by the caller, contiguous fp32, work is
 * enqueued on `stream` (a hipStream_t passed as void*) and the call returns; the library allocates nothing, never
 * synchronises and keeps no state.  Return value: a status of include/beso_hip.h (BESO_OK = 0, BESO_ERR_BAD_SHAPE = -2,
 * BESO_ERR_BAD_ARG = -3, BESO_ERR_WORKSPACE = -4, BESO_ERR_HIP = -6: the same integers, beso_status_string names them).
 * Everything is checked before anything is enqueued.  Buffers the library writes (y, keep, dx, grads_flat without
 * BESO_MLP_ACCUMULATE, the workspace) may hold anything on entry; every element of a result is written and nothing outside
 * a buffer's extent is.
 *
 * Arithmetic: fp32 throughout.  Every product of the GEMMs runs on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) with fp32
 * accumulation; no atomics anywhere: the same inputs give the same bits, and a row of the forward depends on that row alone.
 *
 * Supported: in_dim, out_dim in 1 ... 512; hidden_dim a multiple of 16 up to 512; n_hidden in 1 ... 4; any M >= 1.
 * Anything else is BESO_ERR_BAD_SHAPE (an unknown activation: BESO_ERR_BAD_ARG).
 */
#ifndef BESO_MLP_H
#define BESO_MLP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* MLPNetwork.__init__ kwargs that shape the computation (mlps.py:17-27). */
typedef struct beso_mlp_dims {
    int32_t in_dim;      /* input_dim                                                            */
    int32_t hidden_dim;  /* hidden_dim                                                           */
    int32_t n_hidden;    /* num_hidden_layers: the network has n_hidden + 1 Linear layers        */
    int32_t out_dim;     /* output_dim                                                           */
    int32_t activation;  /* BESO_MLP_ACT_*                                                       */
} beso_mlp_dims;

/* return_activiation_fcn (networks/utils.py:33-51).  "tanh" is nn.Sigmoid there (utils.py:37-38): the binding maps it. */
enum {
    BESO_MLP_ACT_RELU = 0,    /* torch.nn.ReLU: max(z, 0); derivative 1 where z > 0                                   */
    BESO_MLP_ACT_MISH = 1,    /* torch.nn.Mish: z tanh(log1p(exp(z)))                                                 */
    BESO_MLP_ACT_SIGMOID = 2  /* torch.nn.Sigmoid                                                                     */
};

/* beso_mlp_bwd flags */
enum {
    BESO_MLP_ACCUMULATE = 1   /* grads_flat += the call's gradients, as ONE addition per element (g + (sum of the call's
                                 partial sums in index order)): the second call of a step whose state rows and goal rows
                                 go through the same network.  Without it grads_flat is overwritten. */
};

/* Bytes of workspace beso_mlp_bwd needs for M rows (training != 0); 0 for training == 0 (the forward takes none) and for
 * unsupported dims or M < 1.  Layout: dZ_0 .. dZ_{n_hidden-1}, each [M, hidden] -- the gradient with respect to every hidden
 * layer's pre-activation -- then the slab of partial weight-gradient sums, [S][P] floats: P the parameter count and
 * S = ceil(M / R) row ranges of R = max(256, 16 ceil(M / 1024)) rows (so S <= 64 and S depends on M alone).           */
size_t beso_mlp_workspace_bytes(const beso_mlp_dims* dims, long long M, int training);

/* y [M, out] = MLPNetwork.forward(x [M, in]).  ONE launch: a workgroup owns 16 rows and carries them through all layers;
 * the activations between layers live in LDS, the weights are streamed from memory as the MFMA's other operand.
 *   params  host array of n_params = 2 (n_hidden + 1) DEVICE pointers in named_parameters() order: layers.0.weight
 *           [hidden, in], layers.0.bias [hidden], layers.1.weight, ... (torch layouts, fp32)
 *   keep    NULL, or (training) what beso_mlp_bwd reads: x itself, [M, in], followed by the PRE-ACTIVATIONS z_l of the
 *           n_hidden hidden layers, each [M, hidden] -- M (in + n_hidden hidden) floats.  The backward recomputes
 *           act(z_l) where it needs a layer's input; Mish's derivative needs z in any case.                          */
int beso_mlp_fwd(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* x, long long M,
                 float* y, float* keep, void* stream);

/* The gradients of a scalar L, given dy = dL/dy [M, out].  Three launches:
 *   (1) the data-gradient chain, per 16-row tile in reverse layer order: dz_l = (dz_{l+1} W_{l+1}) * act'(z_l), written to
 *       the workspace; with dx != NULL also dx [M, in] = dz_0 W_0;
 *   (2) dW_l = dz_l^T a_{l-1} and db_l = column sums of dz_l as partial sums per row range into the workspace slab -- one
 *       workgroup per (layer, 16 input columns, row range), the bias as one more input column that is constant 1;
 *   (3) the partial sums added in row-range order into grads_flat: the gradients of all parameters back to back in
 *       `params` order (P floats), written, or added to with BESO_MLP_ACCUMULATE.
 * The order of every addition depends on (dims, M) alone: equal bits from run to run.
 *   keep       as written by beso_mlp_fwd for the same (params, dims, M)
 *   workspace  at least beso_mlp_workspace_bytes(dims, M, 1) bytes, 16-byte aligned (BESO_ERR_WORKSPACE otherwise)    */
int beso_mlp_bwd(const float* const* params, int n_params, const beso_mlp_dims* dims, const float* keep, const float* dy,
                 long long M, float* dx, float* grads_flat, void* workspace, size_t workspace_bytes, int flags,
                 void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_MLP_H */
