/*
 * beso_hip.h -- C ABI of libbeso_hip.so: the MI355X (gfx950) implementation of BESO's
 * score-denoising hot path.
 *
 * The reference (intuitive-robots/beso) is pure Python/PyTorch and has no FFI of its own; the
 * boundary below is what a binding for this path would bind.  Each entry point names the
 * reference interface it replaces (file:line relative to the reference checkout):
 *
 *   beso_pack_weights   <- GCDenoiser.state_dict() / load_state_dict   beso_agent.py:458-476
 *   beso_score_fwd      <- DiffusionGPT.forward                        k_diffusion/score_gpts.py:272-358
 *   beso_denoise_fwd    <- GCDenoiser.forward                          k_diffusion/score_wrappers.py:81-96
 *                          (+ ClassifierFreeSampleModel.forward        k_diffusion/classifier_free_sampler.py:35-49)
 *   beso_sampler_step   <- the per-step update of sample_ddim/_euler/_heun
 *                                                                      k_diffusion/gc_sampling.py:205-210,296-310,921-923
 *   beso_sample         <- sample_ddim / sample_euler / sample_heun    k_diffusion/gc_sampling.py:167-213,259-314,895-924
 *   beso_sample_ancestral <- sample_euler_ancestral                    k_diffusion/gc_sampling.py:216-256
 *   beso_sample_traced  <- any of the three with the trajectory recorded (what BesoAgent.visualize_ode and the samplers'
 *                          callbacks look at)                          agents/diffusion_agents/beso_agent.py:478-538
 *   beso_sample_solver  <- sample_dpm_2(_ancestral) / sample_dpmpp_2s(_ancestral) / sample_dpmpp_2m / sample_lms
 *   beso_loss_grad      <- GCDenoiser.loss + loss.backward()           k_diffusion/score_wrappers.py:45-79, beso_agent.py:228-233
 *                          (+ DiffusionGPT.mask_cond, training mode     k_diffusion/score_gpts.py:298-299, 360-371)
 *   beso_loss_fwd       <- GCDenoiser.loss under torch.no_grad(), eval mode: the held-out objective, per sample and as a scalar
 *                                                                      k_diffusion/score_wrappers.py:45-79
 *   beso_goal_mask      <- the Bernoulli mask of DiffusionGPT.mask_cond k_diffusion/score_gpts.py:365-368
 *   beso_dropout_mask   <- the masks of nn.Dropout in training mode      k_diffusion/score_gpts.py:72,79,109,321-325
 *   beso_log_logistic   <- rand_log_logistic (behind the uniform draw)   k_diffusion/utils.py:178-185 (beso_agent.py:227)
 *   beso_scale_rows     <- Scaler.scale_input / scale_output              networks/scaler/scaler_class.py:95-117 (base_agent.py:111-142)
 *   beso_loss_grad_overlap  (same, with the early gradient range for the overlapped all-reduce: SURVEY 8(e) C1)
 *   beso_loss_grad_streams  (same, plus a stream that is released as soon as the loss value is final)
 *   beso_denoise_vjp    <- GCDenoiser.forward + torch.autograd.grad w.r.t. the action   k_diffusion/gc_sampling.py:480-485
 *   beso_loss_grad_inputs   (beso_loss_grad_streams, plus the gradient of the loss with respect to `state` and `goal`: what
 *                          loss.backward() hands to a trainable observation / goal encoder in front of the denoiser)
 *   beso_denoise_vjp_inputs (beso_denoise_vjp, plus the same product with respect to `state` and `goal`)
 *   beso_adam_step      <- optimizer.step() + ema_helper.update()      beso_agent.py:236-244
 *   beso_grad_sumsq / beso_adam_step_clipped <- torch.nn.utils.clip_grad_norm_ in front of that step, and a guard that
 *                          drops a step whose gradient is not finite -- both without a host read (the reference has neither)
 *   beso_gather_windows <- TrajectorySlicerDataset.__getitem__ x batch envs/dataloaders/trajectory_loader.py:160-197
 *   beso_rollout_begin / beso_rollout_end <- the window bookkeeping around the sampler call of BesoAgent.predict, for N
 *                          environments with independent resets            agents/diffusion_agents/beso_agent.py:296-388
 *
 * Conventions
 *   - plain C, plain pointers and sizes.  No torch types.  `stream` is a hipStream_t passed as void*.
 *   - every tensor is device memory, contiguous, fp32, owned by the caller.  The library never
 *     allocates or frees device memory and never synchronises the stream; work is enqueued on
 *     `stream` and the call returns.
 *   - buffers the library writes are handed over UNINITIALISED: the workspace, every output (`out`, `denoised`, `x_grad`,
 *     `dot`, `loss_out`, `per_sample_out`, `state_grad`, `goal_grad`), the solver `history`, `grads_flat` and the `packed` image may hold anything on entry -- NaN bit
 *     patterns and what an earlier, larger call left behind included.  No result depends on a byte the call did not write,
 *     every element of a result is written, and nothing outside [ptr, ptr + size) of a buffer is written
 *     (tests/test_buffer_independence.py).  Inputs are read inside their extents only.
 *   - return value: 0 = ok, negative = error (see beso_status_string).  Bad shapes and unsupported
 *     configurations are rejected before anything is enqueued.
 *   - thread-safety: the library keeps no mutable process-wide state; calls on distinct workspaces/streams are
 *     independent (a workspace must not be shared by concurrent calls).  What a call may vary -- which kernels run --
 *     travels in its own `flags` (BESO_PLAN_*); the launch-site timers (beso_profile_*) are per calling thread.
 *     One piece of state lives in DEVICE memory the caller owns: the sigma-token cache inside a bf16 / fp16 packed image
 *     of the kitchen-class shape (beso_pack_weights), which forwards of a uniform-sigma batch read and extend.  Calls that
 *     share an image on one stream, or on streams the caller orders, need nothing.  Calls that share an image on
 *     streams running CONCURRENTLY are supported only while the image sees at most 128 distinct sigma values between two
 *     packs (no entry is ever replaced then; two calls that miss the same value at once each write an entry of their own,
 *     with equal contents).  Beyond that a miss on one stream replaces the oldest entry round-robin, and that entry may be
 *     the one a forward running on another stream hit and is still reading -- whatever its age when it was hit: such
 *     callers pass BESO_PLAN_SIGMA_PRIVATE with every concurrent call, or give each stream its own image.
 *     beso_pack_weights into an image must be ordered against every call that uses it, as before.
 *   - development aids (phase stamps, the GEMM layout probe) are not part of this library: they exist in the
 *     development build only (include/beso_hip_debug.h, libbeso_hip_dev.so).
 */
#ifndef BESO_HIP_H
#define BESO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: the entry points declared here are its whole dynamic symbol table */
#pragma GCC visibility push(default)

/* DiffusionGPT.__init__ kwargs that shape the computation (score_gpts.py:121-139) + GCDenoiser.sigma_data. */
typedef struct beso_config {
    int32_t obs_dim;        /* state_dim                                                      */
    int32_t act_dim;        /* action_dim                                                     */
    int32_t embed_dim;      /* D                                                              */
    int32_t n_layers;       /* L                                                              */
    int32_t n_heads;        /* H,  D % H == 0                                                 */
    int32_t goal_seq_len;   /* G actually used: 0 when goal_conditioned is False (:143-144)   */
    int32_t obs_seq_len;    /* W (window_size); block_size = G + 2W + 1 (:148)                */
    int32_t linear_output;  /* 1: action_pred = Linear(D, act); 0: Linear(D,100)-SiLU-Linear  */
    float   sigma_data;     /* GCDenoiser.sigma_data (score_wrappers.py:29)                   */
} beso_config;

/* arithmetic of the GEMMs (everything else -- residual stream, LayerNorm, softmax, GELU,
 * preconditioning, sampler update -- is fp32 in every mode) */
enum {
    BESO_PREC_BF16 = 0,   /* bf16 MFMA inputs, fp32 accumulate: throughput mode                 */
    BESO_PREC_FP32 = 1,   /* fp32-input MFMA (v_mfma_f32_16x16x4_f32), exact fp32: parity mode  */
    BESO_PREC_BF16X3 = 2, /* split-bf16 (hi*hi + hi*lo + lo*hi on the bf16 MFMA, fp32 accumulate): fp32-class
                             accuracy from the fused kernel: an instance of layers_kernel for kitchen and block-push,
                             split-bf16 block kernels for the long-horizon shape (D = 512); other shapes return
                             BESO_ERR_UNSUPPORTED; inference only */
    BESO_PREC_FP16 = 3    /* fp16 MFMA inputs (v_mfma_f32_16x16x32_f16: the bf16 rate, three more mantissa bits), fp32
                             accumulate: the one-launch kernel's shapes only (kitchen, block-push, long-horizon without
                             classifier-free pairs); operands must stay inside fp16's range (|v| < 65504: LayerNorm
                             outputs, GELU outputs, probabilities and N(0, 0.02)-scale weights do); inference only */
};

/* beso_loss_grad flags */
enum {
    BESO_TRAIN_LAST_ACTION_ONLY = 1, /* GCDenoiser.loss(pred_last_action_only=True): only the last step of every window
                                        is scored (score_wrappers.py:59-63,76-77; the caller zeroes the other steps' noise) */
    /* execution-plan hints (bf16): which kernels run the step, never what it computes -- all forms write the same kept
     * activations and evaluate the same dropout masks.  Default forward: ALL layers as one launch where the shape has that
     * kernel (kitchen, block-push; no dropout on the proj / MLP outputs); otherwise the per-op kernels below 16,000 token rows
     * and the tile kernel (a layer's out-projection .. the next layer's q/k/v as one launch) from there on.  Default backward:
     * the data gradients in the transposed formulation (GELU' / LayerNorm backward as GEMM epilogues, FC2 .. out-projection of a
     * layer as one launch), the attention backward on the matrix pipe, the weight gradients of >= 18 k token rows in row
     * windows. */
    BESO_TRAIN_PLAN_PER_OP = 2,      /* per-op kernels for every layer, forward and backward (the comparator of the above) */
    BESO_TRAIN_PLAN_TILES = 4,       /* the tile kernel (one launch per layer) wherever the shape has it */
    /* Bit-reproducible step: every sum the step otherwise accumulates with fp32 atomics -- the FC1 / MLP-head hidden bias
     * gradients that ride on a data-gradient GEMM's epilogue, the bias gradients formed by a column-sum launch, and the loss
     * value itself -- is written as per-workgroup (per-wave) partial sums into a slab of the workspace and added up by a
     * second small launch in slab-index order.  The order of every addition then depends on the shapes of the call only: two
     * calls with the same inputs, seed, flags, precision and library build give equal bits in the loss and in the whole
     * gradient buffer, whatever the workspace and the gradient buffer held before.  Orthogonal to the plan hints (every plan
     * honours it, in both precisions, for both action heads); the weight-matrix gradients are the same bits with and without
     * it.  The loss is still final where beso_loss_grad_streams releases loss_stream.  Without the flag the step launches
     * exactly the kernels it launched before the flag existed.  Not promised: equal bits across batch sizes, GPU counts,
     * plans or library builds.  beso_denoise_vjp has no such sums and rejects the flag. */
    BESO_TRAIN_DETERMINISTIC = 8
};

/* flags of the forward calls (beso_score_fwd, beso_denoise_fwd, beso_sample, beso_sample_ancestral) */
enum {
    BESO_FLAG_UNCOND = 1,     /* DiffusionGPT.forward(uncond=True): goals := 0 (score_gpts.py:301-302); forwards only */
    /* Execution-plan hints: WHICH kernels run, never what they compute.  They exist for parity tests (the per-op kernels are
     * the reference of the fused ones in the same arithmetic; the instances of the one-launch kernel agree bit for bit) and
     * for measurements; a hint the shape or precision cannot honour is ignored. */
    BESO_PLAN_PER_OP = 0x10,  /* per-op kernels only: LayerNorm, GEMMs, attention (bf16 / fp32; any shape) */
    BESO_PLAN_BLOCKS = 0x20,  /* at most the block kernels (LN2 + MLP block, tail block), not the one-launch kernel */
    BESO_PLAN_SMALL = 0x40,   /* the chip-wide small-batch path (bf16 / fp32, embed_dim <= 384: four short launches per layer --
                                 three up to 96 token rows in bf16 -- that spread every weight matrix over the CUs) at ANY batch
                                 size; without a hint the library
                                 takes it up to 448 token rows in bf16 (kitchen: 40 samples) and 4096 in fp32, where one
                                 workgroup per sample group would stream all the weights alone */
    BESO_PLAN_FUSED = 0x80,   /* the one-launch / block kernels at every batch size (never the small-batch path) */
    BESO_PLAN_SPW2 = 0x100,   /* samples per workgroup of the one-launch kernel: 2 (default up to 512 samples), */
    BESO_PLAN_SPW4 = 0x200,   /*   4 (up to 1024; the split-bf16 mode: above 512), */
    BESO_PLAN_SPW8 = 0x300,   /*   8 (larger batches) */
    BESO_PLAN_SPW_MASK = 0x300,
    BESO_PLAN_SIGMA_SHARED = 0x400,  /* one forward, kitchen-class shape (embed_dim 360, 6 heads), bf16 / fp16: the eight-sample
                                        plan with the sigma token shared (below, beso_pack_weights) at ANY batch size -- without
                                        a hint: wherever the eight-sample instance runs (more than 1024 samples, or SPW8) */
    BESO_PLAN_SIGMA_PRIVATE = 0x800, /* never shared: every sample computes its own sigma token, the image's cache is not touched */
    BESO_PLAN_MASK = 0xff0,
    BESO_SAMPLE_STEPWISE = 0x1000, /* beso_sample: enqueue evaluation by evaluation (see there) */
    BESO_FLAG_LAST_ACTION_ONLY = 0x2000 /* beso_loss_fwd: GCDenoiser.loss(pred_last_action_only=True) -- only the last step of
                                      every window is scored (score_wrappers.py:59-63,76-77; the caller zeroes the other
                                      steps' noise); what BESO_TRAIN_LAST_ACTION_ONLY is to beso_loss_grad */
};

/* sampler ids for beso_sample / beso_sampler_step */
enum {
    BESO_SAMPLER_DDIM = 0,   /* gc_sampling.py:895-924 */
    BESO_SAMPLER_EULER = 1,  /* gc_sampling.py:167-213, s_churn = 0 */
    BESO_SAMPLER_HEUN = 2    /* gc_sampling.py:259-314, s_churn = 0 */
};

/* status codes */
enum {
    BESO_OK = 0,
    BESO_ERR_BAD_CONFIG = -1,      /* config fields out of range / D % H != 0                      */
    BESO_ERR_BAD_SHAPE = -2,       /* batch < 1, t < 1, t > obs_seq_len (score_gpts.py:282)         */
    BESO_ERR_BAD_ARG = -3,         /* null pointer, unknown precision / sampler / flag              */
    BESO_ERR_WORKSPACE = -4,       /* workspace or packed buffer too small                          */
    BESO_ERR_UNSUPPORTED = -5,     /* configuration this build has no kernel for                    */
    BESO_ERR_HIP = -6              /* a HIP runtime call failed (hipGetLastError has the detail)     */
};

const char* beso_version(void);
const char* beso_status_string(int status);
/* Detail of the last BESO_ERR_HIP on the calling thread (HIP error name and the failing call). */
const char* beso_last_error(void);

/* Number of parameter tensors, in the order of the reference module's named_parameters():
 * pos_emb, tok_emb.{weight,bias}, per block {ln1,ln2}.{weight,bias}, attn.{key,query,value,proj}.{weight,bias},
 * mlp.{0,2}.{weight,bias}; ln_f.{weight,bias}, sigma_emb.{weight,bias}, action_emb.{weight,bias},
 * action_pred[.0/.2].{weight,bias}.  Linear weights are torch layout [out, in], fp32.
 * (beso_amd/csrc/params.h is the only implementation of this order.)                            */
int beso_num_params(const beso_config* cfg);

/* Size of the packed-weight image for `precision`, in bytes (0 on bad config). */
size_t beso_packed_bytes(const beso_config* cfg, int precision);

/* Re-lay the fp32 parameters (host array `params` of `n_params` DEVICE pointers, order above) into
 * the kernel-ready image `packed` (device, >= beso_packed_bytes): fused QKV rows, bf16 (or fp32)
 * GEMM operands zero-padded to the MFMA tile grid.  Call again whenever a parameter changes
 * (optimizer step, EMA swap, load_state_dict).
 * The bf16 / fp16 image of the kitchen-class shape ends in a sigma-token cache (1.1 MiB): 128 entries, each the k / v rows
 * of the sigma token in every layer for one sigma value -- token 0 has no position and attends to itself only, so they
 * depend on (weights, sigma) alone.  Packing zeroes it; a forward whose sigma[0 .. batch) is ONE value (every sampler's
 * calls) looks that value up on the device, computes the entry once if it is new, and runs the network on the other ten
 * tokens per sample.  The image is therefore written by the forward calls that take it as `const void* packed`
 * (that region only).  Results are bit-identical either way.                                      */
int beso_pack_weights(const beso_config* cfg, const float* const* params, int n_params,
                      void* packed, size_t packed_bytes, int precision, void* stream);

/* Scratch needed by one forward over `batch` samples with `t` observations in the window
 * (T = 1 + G + 2t tokens each).  `cfg_guidance` != 0 doubles the token count (cond + uncond).    */
size_t beso_workspace_bytes(const beso_config* cfg, int batch, int t, int precision, int cfg_guidance);

/* DiffusionGPT.forward (eval mode): out[batch,t,act] = F(states[batch,t,obs], actions[batch,t,act],
 * goals[batch,G,obs], sigma[batch]).  No preconditioning.                                        */
int beso_score_fwd(const beso_config* cfg, const void* packed, int precision,
                   const float* state, const float* action, const float* goal, const float* sigma,
                   float* out, int batch, int t, int flags,
                   void* workspace, size_t workspace_bytes, void* stream);

/* GCDenoiser.forward: out = F(state, action*c_in, goal, sigma)*c_out + action*c_skip.
 * cond_lambda reproduces ClassifierFreeSampleModel: 1 -> conditional only, 0 -> unconditional only,
 * otherwise out_u + cond_lambda*(out_c - out_u) evaluated as ONE 2*batch pass.                    */
int beso_denoise_fwd(const beso_config* cfg, const void* packed, int precision,
                     const float* state, const float* action, const float* goal, const float* sigma,
                     float* out, int batch, int t, int flags, float cond_lambda,
                     void* workspace, size_t workspace_bytes, void* stream);

/* One sampler update, elementwise over n fp32 values, in the reference's operation order:
 *   BESO_STEP_DDIM         out = c0*x - c1*den              c0 = sigma_fn(t_next)/sigma_fn(t), c1 = expm1(-h)   gc_sampling.py:921-923
 *   BESO_STEP_EULER        d = (x - den)/c0; out = x + d*c1                 c0 = sigma_hat, c1 = dt              :205-210
 *   BESO_STEP_HEUN_PREDICT d = (x - den)/c0; aux = d; out = x + d*c1        (out = action_2)                     :296-305
 *   BESO_STEP_HEUN_CORRECT d2 = (x2 - den)/c0; out = x + ((aux + d2)/2)*c1  c0 = sigma_{i+1}                     :306-310
 * out may alias x.  x2 / aux may be NULL for the modes that do not use them.                     */
enum { BESO_STEP_DDIM = 0, BESO_STEP_EULER = 1, BESO_STEP_HEUN_PREDICT = 2, BESO_STEP_HEUN_CORRECT = 3,
       BESO_STEP_ADD_NOISE = 4 /* out = x + x2 * c0 (x2 = the randn of an ancestral step, c0 = sigma_up; den unused, may be x)  :246-247 */ };
int beso_sampler_step(int mode, float* out, float* aux, const float* x, const float* x2, const float* den,
                      float c0, float c1, size_t n, void* stream);

/* A whole sampling loop: x[batch,t,act] holds x_T on entry and the sample on return.
 * `sigmas` is a HOST array of n_sigmas values, the last one 0 (get_sigmas_*: gc_sampling.py:26-44).
 * No host synchronisation inside.  Where the shape has the one-launch kernel (bf16 / bf16x3: kitchen, block-push,
 * long-horizon without classifier-free pairs) the WHOLE loop is ONE launch: the workgroup that owns a sample from the
 * embedding to the head also applies the step's update and feeds itself the next evaluation (up to 128 evaluations per
 * launch; longer loops are cut at step boundaries).  Otherwise, and with BESO_SAMPLE_STEPWISE, every evaluation is
 * enqueued as the forward launch(es) + one update launch.  Both forms run the same arithmetic (bit-identical results). */
int beso_sample(const beso_config* cfg, const void* packed, int precision, int sampler,
                const float* state, const float* goal, float* x, int batch, int t,
                const float* sigmas, int n_sigmas, float cond_lambda, int flags,
                void* workspace, size_t workspace_bytes, void* stream);

/* sample_euler_ancestral (gc_sampling.py:216-256, scaler = None) as one enqueue: per step an Euler step to sigma_down and,
 * while sigma_down > 0, x += noise_i * sigma_up (get_ancestral_step: :107-114, fp32).  `noise` is a DEVICE array of
 * n_sigmas - 1 standard-normal tensors [batch,t,act] back to back -- the reference's `torch.randn_like(action)` of each
 * step, drawn by the caller (the library has no random number generator); entries of steps with sigma_down = 0 are not
 * read.  Where the shape has the one-launch kernel the WHOLE loop is ONE launch, as in beso_sample: the workgroup that owns
 * a sample applies the Euler update and adds its slice of the step's noise in the kernel's head.  Otherwise, and with
 * BESO_SAMPLE_STEPWISE, one forward + one update launch per step (bit-identical results).
 * `flags`: BESO_PLAN_* hints | BESO_SAMPLE_STEPWISE.  Everything else as beso_sample.                                  */
int beso_sample_ancestral(const beso_config* cfg, const void* packed, int precision, const float* state, const float* goal,
                          float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda, float eta,
                          const float* noise, int flags, void* workspace, size_t workspace_bytes, void* stream);

/* The other fixed-schedule samplers of gc_sampling.py as one enqueue (scaler = None, no callback, s_churn = 0):
 *   BESO_SOLVER_DPM_2                sample_dpm_2               :317-375   2 evaluations per step, 1 on the last
 *   BESO_SOLVER_DPM_2_ANCESTRAL      sample_dpm_2_ancestral     :378-413   to sigma_down, then x += noise_i * sigma_up
 *   BESO_SOLVER_DPMPP_2S             sample_dpmpp_2s            :928-966   2 evaluations per step, 1 on the last
 *   BESO_SOLVER_DPMPP_2S_ANCESTRAL   sample_dpmpp_2s_ancestral  :969-1016  to sigma_down, then x += noise_i * s_noise * sigma_up
 *   BESO_SOLVER_DPMPP_2M             sample_dpmpp_2m            :702-736   1 evaluation per step
 *   BESO_SOLVER_LMS                  sample_lms (order 1 ... 4) :432-468   1 evaluation per step
 * Coefficients in fp32 on the host as the reference's scalars (the LMS integrals of its Lagrange basis in double, exactly).
 * `noise` (the ancestral solvers only; else may be NULL): a DEVICE array of n_sigmas - 1 standard-normal tensors
 * [batch,t,act] back to back, the draws of the reference's steps (entries of steps that draw nothing are not read).
 * `history` (DPMPP_2M: 1 slab, LMS: order - 1 slabs of batch*t*act floats; else may be NULL): caller-owned DEVICE scratch
 * for the state a multistep solver carries from step to step.  `eta` is the ancestral solvers', `s_noise` DPMPP_2S_ANCESTRAL's,
 * `order` LMS's.  One launch for the whole loop where beso_sample runs one (up to 128 evaluations per launch, cut at step
 * boundaries); otherwise, and with BESO_SAMPLE_STEPWISE, one forward + one update launch per evaluation (bit-identical).
 * BESO_ERR_BAD_ARG: unknown solver or flags, LMS order outside 1 ... 4, a missing noise / history, eta < 0, an interior
 * sigma <= 0.  Everything else as beso_sample; the workspace is beso_workspace_bytes'.                                   */
enum { BESO_SOLVER_DPM_2 = 0, BESO_SOLVER_DPM_2_ANCESTRAL = 1, BESO_SOLVER_DPMPP_2S = 2, BESO_SOLVER_DPMPP_2S_ANCESTRAL = 3,
       BESO_SOLVER_DPMPP_2M = 4, BESO_SOLVER_LMS = 5 };
int beso_sample_solver(const beso_config* cfg, const void* packed, int precision, int solver, const float* state,
                       const float* goal, float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda,
                       float eta, float s_noise, int order, const float* noise, float* history, int flags,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Any of the three sampler calls above with its denoising trajectory recorded by the launches the call makes anyway (the head
 * of the one-launch loop, or the update launch of the step-by-step form: recording adds no launch but one copy of x_T).
 * `entry` picks the call -- BESO_ENTRY_SAMPLE: beso_sample with `sampler` a BESO_SAMPLER_*; BESO_ENTRY_ANCESTRAL:
 * beso_sample_ancestral (`sampler` unused); BESO_ENTRY_SOLVER: beso_sample_solver with `sampler` a BESO_SOLVER_* -- and the
 * arguments are the union of theirs, checked as that call checks them (those it does not take are ignored).  With n =
 * n_sigmas - 1 steps and N = batch*t*act, two optional DEVICE outputs in fp32:
 *   trace_x    [n + 1][batch,t,act]  slab 0 is x_T as passed in; slab i + 1 is x after step i is COMPLETE -- behind the second
 *                                    evaluation of a two-evaluation step and behind the step's noise of the ancestral samplers
 *                                    -- so slab n equals the returned x bit for bit.  What a step parks between its two
 *                                    evaluations (Heun's x2, DPM-2's midpoint) is not recorded.
 *   trace_den  [n][batch,t,act]      slab i is the denoised value of the FIRST evaluation of step i, what the reference's loops
 *                                    hand their callback as 'denoised': the preconditioned output, the classifier-free
 *                                    combination when cond_lambda is neither 0 nor 1, the unconditional output when it is 0.
 * Either may be NULL (not recorded); with both NULL the call is the plain entry point.  `trace_x_floats` / `trace_den_floats`
 * are the buffers' capacities in floats: below (n + 1) N / n N the call returns BESO_ERR_WORKSPACE before anything is
 * enqueued.  The two buffers must be disjoint from each other and from every other buffer of the call; an overlap with x,
 * the workspace, `noise` or each other is refused (BESO_ERR_BAD_ARG), one with `history`, the inputs or the weights is the
 * caller's to avoid.  The result in x, the launches and their kernels are those of the plain call.                        */
enum { BESO_ENTRY_SAMPLE = 0, BESO_ENTRY_ANCESTRAL = 1, BESO_ENTRY_SOLVER = 2 };
int beso_sample_traced(const beso_config* cfg, const void* packed, int precision, int entry, int sampler, const float* state,
                       const float* goal, float* x, int batch, int t, const float* sigmas, int n_sigmas, float cond_lambda,
                       float eta, float s_noise, int order, const float* noise, float* history, float* trace_x,
                       size_t trace_x_floats, float* trace_den, size_t trace_den_floats, int flags, void* workspace,
                       size_t workspace_bytes, void* stream);

/* One Adam / AdamW step over ALL parameter tensors in one launch, optionally followed by the EMA update
 * of the shadow copy on the updated parameters.  Replaces `self.optimizer.step()` + `self.ema_helper.update`
 * of the training step (reference beso_agent.py:236-244; torch.optim.AdamW for kitchen, torch.optim.Adam
 * for block-push: configs/agents/beso_kitchen.yaml:9-12, beso_block_push.yaml:9-11; ema.py:45-53); the
 * arithmetic is torch's single-tensor Adam(W) with amsgrad = False, maximize = False, in fp32.
 *   chunks      DEVICE array: each entry is at most 4096 consecutive elements of one parameter tensor
 *   exp_avg, exp_avg_sq, ema   flat fp32 state buffers indexed by chunk.off + i (ema may be NULL)
 *   decoupled_wd 1 = AdamW (p *= 1 - lr*wd), 0 = Adam (g += wd*p);  step = 1-based step count
 *   ema_decay   the decay actually applied this step, min(decay, (1+n)/(10+n)) (ema.py:45-48)       */
typedef struct beso_optim_chunk {
    float* p;
    const float* g;
    unsigned long long off;
    unsigned int n;
    unsigned int pad;
} beso_optim_chunk;
int beso_adam_step(const beso_optim_chunk* chunks, int n_chunks, float* exp_avg, float* exp_avg_sq, float* ema,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled_wd, int step,
                   float ema_decay, void* stream);

/* Global gradient-norm clipping and the non-finite guard of the optimizer step, with no host read in between: the squared
 * L2 norm of the gradients is reduced on the device and the step launch consumes it.
 *   stats       DEVICE double[4], owned by the caller:
 *                 [0] sumsq   written by beso_grad_sumsq (a sharded data-parallel step sums it across ranks in place
 *                             before the step: every rank then applies the norm of the WHOLE gradient)
 *                 [1] norm    (float)sqrt(sumsq) of the last beso_adam_step_clipped, held as a double
 *                 [2] coef    the clip coefficient that step applied; 0 when it was skipped
 *                 [3] skipped number of skipped steps so far: INCREMENTED by a skipped step -- the caller zeroes it once
 *               [0..2] are fully overwritten on every use and may hold anything on entry (as may `partial`).
 * beso_grad_sumsq: stats[0] = sum of g^2 over all chunks (the `g` pointers of the table beso_adam_step walks, so a
 *   sharded table gives the shard's share).  Squares and sums are in double, in a fixed order (per chunk, then over
 *   partial[0 .. n_chunks)): no atomics, the same inputs give the same bits.  `partial`: at least n_chunks doubles of scratch.
 *   n_chunks == 0 is valid (chunks and partial may then be NULL) and writes stats[0] = 0.
 * beso_adam_step_clipped: beso_adam_step with every gradient element multiplied (one rounded fp32 multiply, in registers) by
 *   coef = min(1, max_grad_norm / (norm + 1e-6f)), norm = (float)sqrt(stats[0]) -- the rule of torch.nn.utils.clip_grad_norm_.
 *   DEPARTURE from clip_grad_norm_: the gradient buffer itself is NOT rescaled; a caller that reads the gradients after the
 *   step sees the unclipped values.  max_grad_norm = +inf gives coef == 1 exactly: the step is bit-equal to beso_adam_step
 *   and only measures (and guards).  max_grad_norm <= 0 or NaN is BESO_ERR_BAD_ARG.
 *   skip_nonfinite != 0: when stats[0] is inf or NaN the launch stores nothing into the parameters, exp_avg, exp_avg_sq and
 *   ema (they keep their bits), writes coef = 0 and increments stats[3].  The HOST cannot know: `step` (bias correction) and
 *   the EMA warm-up counter behind `ema_decay` are the caller's, and a caller that does not read stats[3] advances them over a
 *   skipped step as over any other.  With skip_nonfinite == 0 nothing is held back: a NaN norm gives
 *   coef = 1 (fminf drops the NaN), an infinite one coef = 0 under a finite max_grad_norm, and the non-finite gradient
 *   elements reach the parameters, as they do in torch.
 *   The norm is over the chunks of the call: a caller with several parameter groups (one call each) clips per group.
 *   n_chunks == 0 is a no-op that leaves stats untouched.                                                                    */
int beso_grad_sumsq(const beso_optim_chunk* chunks, int n_chunks, double* partial, double* stats, void* stream);
int beso_adam_step_clipped(const beso_optim_chunk* chunks, int n_chunks, float* exp_avg, float* exp_avg_sq, float* ema,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled_wd, int step,
                           float ema_decay, double* stats, float max_grad_norm, int skip_nonfinite, void* stream);

/* Training step, forward + backward: GCDenoiser.loss (score_wrappers.py:45-79; flags: BESO_TRAIN_LAST_ACTION_ONLY) of the
 * training-mode network (score_gpts.py:272-358 with the dropouts of :41,:79,:109) and the gradient of that loss with
 * respect to every parameter -- what `loss = model.loss(...); loss.backward()` leaves in `.grad`
 * (beso_agent.py:228-233).  Both action heads (linear_output 1 / 0).
 *   params      host array of n_params DEVICE pointers, order of beso_pack_weights (fp32, torch layouts)
 *   grads_flat  device fp32 buffer of beso_grad_floats(cfg) values: the gradients of all parameters back to back in
 *               the same order, each tensor contiguous.  OVERWRITTEN: zeroed first, then the weight gradients are
 *               plain stores of one grouped launch (no split-K, no atomics), while the bias / LayerNorm-affine /
 *               embedding gradients are accumulated from block partial sums (a few fp32 atomics per block: two runs
 *               agree to rounding in those tensors and in the loss, not bit for bit, unless BESO_TRAIN_DETERMINISTIC is
 *               set: then every such sum is formed in a fixed order and two runs give equal bits).
 *   state [batch,t,obs], action [batch,t,act] (clean), goal [batch,G,obs] (UNMASKED: see goal_drop),
 *   noise [batch,t,act], sigma [batch];  loss_out: one device float.
 *   goal_drop   DiffusionGPT's goal_drop (`cond_mask_prob`, configs: cond_mask_prob): training-mode mask_cond
 *               (score_gpts.py:298-299, 360-371) -- every ELEMENT of goal is zeroed with this probability, kept ones are
 *               not rescaled -- applied inside the embedding kernel; the mask is the counter-based hash of (seed, element),
 *               the one beso_goal_mask writes out.  0 disables (eval mode, or goals masked by the caller).
 *   embed_pdrop / attn_pdrop / resid_pdrop: dropout probabilities of the token embeddings (not the sigma token), of
 *   the attention weights and of the proj / MLP outputs (DiffusionGPT's embed_pdrob, attn_pdrop, resid_pdrop); the
 *   masks are a counter-based hash of (seed, site, element), recomputed in the backward.  0 disables.
 *   grad_scale multiplies every gradient (1/world_size for data-parallel averaging); the loss is unscaled.
 *   precision   BESO_PREC_BF16: bf16 GEMM operands (weights, kept activations, gradient operands), fp32 accumulation,
 *               fp32 residual stream / LayerNorm / softmax / loss;  BESO_PREC_FP32: everything fp32 (parity mode).  */
/* The workspace includes the slab of BESO_TRAIN_DETERMINISTIC's partial sums for every caller (the size does not depend on the
 * flags): 4 * max(1024, 2 * ceil(batch*T / 128) * max(4 * embed_dim, H)) bytes, T = 1 + goal_seq_len + 2 t, H = 104 with the
 * MLP action head (linear_output 0) and 0 with the linear one, rounded up to the
 * workspace's alignment -- 1.0 MB of the 1024-sample kitchen step's workspace.  Like the rest of the workspace it may hold
 * anything on entry: every slab element a call reads was written by that call. */
size_t beso_train_workspace_bytes(const beso_config* cfg, int batch, int t, int precision);
size_t beso_grad_floats(const beso_config* cfg);
int beso_loss_grad(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                   const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                   float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                   float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes, void* stream);
/* GCDenoiser.forward in eval mode at (state, x, goal, sigma), and the vector-Jacobian product of that output with
 * respect to x (reference log_likelihood's torch.autograd.grad, gc_sampling.py:480-485).  The training step's forward and
 * chain of data gradients (beso_loss_grad), seeded with the cotangent instead of the loss and ended by a projection of the
 * embedding gradient onto the action input; no weight gradient, no reduction of partial sums.
 *   params      n_params DEVICE pointers, order of beso_pack_weights (as beso_loss_grad); read only
 *   state [batch,t,obs], x [batch,t,act], goal [batch,G,obs] (may be NULL when G = 0), sigma [batch]
 *   cot         [batch,t,act] cotangent u
 *   denoised    [batch,t,act] out: c_skip*x + c_out*F(c_in*x, ...)
 *   x_grad      [batch,t,act] out: (d denoised / d x)^T u
 *   dot         [batch] out, may be NULL: sum over (t,act) of u * x_grad, per sample (a fixed-order reduction)
 *   flags       BESO_TRAIN_PLAN_PER_OP / BESO_TRAIN_PLAN_TILES only
 *   workspace   beso_train_workspace_bytes(cfg, batch, t, precision) bytes
 * precision: BESO_PREC_BF16 or BESO_PREC_FP32.  No dropout, no goal masking (uncond: pass zero goals).  No parameter
 * gradient is computed or written.  Bad shapes, embed_dim % 8 != 0, an unknown precision or flag bit, a NULL required
 * pointer and a short workspace are rejected before anything is enqueued.                                            */
int beso_denoise_vjp(const beso_config* cfg, const float* const* params, int n_params, int precision, const float* state,
                     const float* x, const float* goal, const float* sigma, const float* cot, float* denoised, float* x_grad,
                     float* dot, int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream);
/* The gradient-free score-matching objective: GCDenoiser.loss (score_wrappers.py:45-79) of the EVAL-mode network, as
 * `with torch.no_grad(): model.loss(state, action, goal, noise, sigma)` returns it -- the held-out loss of validation curves,
 * early stopping and loss-against-sigma diagnostics -- on the inference path: the network is evaluated from the packed image
 * (which may be the EMA image) in any precision, nothing is kept for a backward and no parameter gradient exists.
 * Three steps on `stream`: (1) scaled = (action + noise*sigma[b]) * c_in[b], elementwise; (2) pred = F(state, scaled, goal,
 * sigma), the launches of beso_score_fwd under the library's own plan choice (flags: BESO_PLAN_* hints, BESO_FLAG_UNCOND for
 * the unconditional branch's loss); (3) one wave per sample forms target = (action - c_skip*noised)/c_out from action, noise
 * and sigma again and reduces (pred - target)^2, then ONE workgroup reduces the per-sample values.  F(c_in*noised) is compared
 * with the target -- the reference's operation order; (D - action)/c_out would cancel at small sigma.  Every product, quotient
 * and sum of (1) and (3) is rounded on its own, as torch rounds them.
 *   state [batch,t,obs], action [batch,t,act] (clean), goal [batch,G,obs] (may be NULL when G = 0), noise [batch,t,act],
 *   sigma [batch] (> 0);  no dropout, no goal masking.
 *   per_sample_out [batch], may be NULL: the mean of (pred - target)^2 over the sample's t*act values -- with
 *                  BESO_FLAG_LAST_ACTION_ONLY over the act values of step t-1 only (score_wrappers.py:76-77).
 *   loss_out       one float, may be NULL: sum_b per_sample[b] / batch, the reference's `.flatten(1).mean()` / `.mean()`.
 *   At least one of the two must be given.
 * Both reductions run in a fixed order without atomics: per_sample[b] depends on sample b's values only (it equals the value of
 * that sample evaluated alone wherever the forward has that property), and two runs give equal bits wherever the forward does.
 * workspace: beso_loss_fwd_workspace_bytes(cfg, batch, t, precision) bytes (0 on a bad config / shape) -- the forward's
 * (beso_workspace_bytes(..., 0)) followed by `scaled`, `pred` and the per-sample values of a call without per_sample_out.
 * Before anything is enqueued: BESO_ERR_BAD_ARG for an unknown precision or flag bit, a NULL required pointer or both outputs
 * NULL; BESO_ERR_BAD_SHAPE for batch < 1, t < 1, t > obs_seq_len; BESO_ERR_WORKSPACE for a short workspace;
 * BESO_ERR_UNSUPPORTED where beso_score_fwd has no kernel for the shape in this precision.                              */
size_t beso_loss_fwd_workspace_bytes(const beso_config* cfg, int batch, int t, int precision);
int beso_loss_fwd(const beso_config* cfg, const void* packed, int precision, const float* state, const float* action,
                  const float* goal, const float* noise, const float* sigma, float* loss_out, float* per_sample_out,
                  int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream);
/* The keep-mask (1.0 / 0.0 per element of goal [batch,G,obs]) that beso_loss_grad applies for (goal_drop, seed):
 * `1 - torch.bernoulli(...)` of DiffusionGPT.mask_cond (score_gpts.py:365-368) with this library's generator.       */
int beso_goal_mask(float* mask, int batch, int goal_seq_len, int obs_dim, float goal_drop, unsigned int seed, void* stream);
/* The keep-scale (0 or 1/(1-p) per element) of one training dropout, exactly as beso_loss_grad applies it for the same
 * (cfg, batch, t, p, seed): the mask torch's nn.Dropout would have drawn, with this library's generator (a counter-based
 * hash of (seed, site, element): nothing is recorded during the step, the same function is evaluated here).  With these
 * masks and beso_goal_mask's a training step can be reproduced or audited elsewhere.
 *   kind / layer  which dropout: BESO_DROP_* of transformer layer `layer` in [0, n_layers) (ignored for BESO_DROP_EMBED)
 *   scale         out, fp32, contiguous, 16-byte aligned, reference layout with T = 1 + goal_seq_len + 2 t:
 *                 BESO_DROP_ATTN [batch, n_heads, T, T] -- every (query, key) pair is written, the causally masked ones too
 *                 (their probabilities are zero); the other kinds [batch, T, embed_dim] in natural token order
 *                 (sigma, goals, then state / action alternating).
 *   p             the probability the step is called with for that kind (embed_pdrop / attn_pdrop / resid_pdrop), in
 *                 [0, 1); 0 writes ones.
 * Elements the step draws no mask for are 1: the sigma-token row of every sample for BESO_DROP_EMBED (score_gpts.py:321-325
 * has no dropout there), and for BESO_DROP_PROJ / BESO_DROP_MLP of the LAST layer every row but the action tokens' -- the
 * loss reads the action tokens only (score_gpts.py:353), the step does not evaluate the other rows behind that layer's
 * attention, and no value there changes the loss or a gradient.
 * One difference to the reference: the embedding mask is drawn per sample row, while the reference, handed a goal with
 * batch dimension 1, draws one goal-embedding mask and expands it; pass goals as [batch, G, obs] when comparing.
 * Status as beso_loss_grad for (cfg, batch, t); BESO_ERR_BAD_ARG for a NULL cfg / scale, a misaligned scale, an unknown
 * kind, a layer outside [0, n_layers) or p outside [0, 1) -- before anything is enqueued.                              */
#define BESO_DROP_EMBED 0   /* self.drop on the token / action / goal embeddings   score_gpts.py:321-325 */
#define BESO_DROP_ATTN  1   /* attn_drop on the softmax output, before @ v         score_gpts.py:72      */
#define BESO_DROP_PROJ  2   /* resid_drop on the out-projection                    score_gpts.py:79      */
#define BESO_DROP_MLP   3   /* Dropout at the end of the MLP                       score_gpts.py:109     */
int beso_dropout_mask(const beso_config* cfg, float* scale, int kind, int layer, int batch, int t, float p,
                      unsigned int seed, void* stream);
/* The training feed on trajectories resident in HBM: one batch of TrajectorySlicerDataset.__getitem__
 * (envs/dataloaders/trajectory_loader.py:160-197; the collate of torch's DataLoader included) as one launch.
 *   observations [n_traj,t_max,obs_dim], actions [n_traj,t_max,act_dim]  padded trajectories (TensorDataset.tensors)
 *   seq_len [n_traj] int32        valid length of each trajectory (get_seq_length)
 *   slice_traj / slice_start [n_slices] int32   the slicer's table: window s = rows [start, start + window) (:128-135)
 *   batch_slices [batch] int64    which windows make up this batch (a chunk of a permutation)
 *   draws [batch] int64 >= 0      one random integer per sample; BESO_GOAL_RANDOM takes the future sequence at
 *                                 lo + draws % (hi - lo), lo = end + min_future_sep, hi = seq_len - goal_len (:169-182);
 *                                 may be NULL for the other modes or goal_len = 0
 *   goal_mode   BESO_GOAL_RANDOM | BESO_GOAL_TAIL (only_sample_tail, :175-176) | BESO_GOAL_SEQ_END (only_sample_seq_end, :177-178)
 *   goal_len    future_seq_len, 0 = not future conditional (goal_out may be NULL)
 *   obs_out [batch,window,obs_dim], act_out [batch,window,act_dim], goal_out [batch,goal_len,obs_dim]
 * Samples whose trajectory has no room for a future sequence get the reference's zeros placeholder (:185-186);
 * out-of-range slice ids produce zero rows instead of a fault.                                                     */
enum { BESO_GOAL_RANDOM = 0, BESO_GOAL_TAIL = 1, BESO_GOAL_SEQ_END = 2 };
int beso_gather_windows(const float* observations, const float* actions, const int* seq_len, int n_traj, int t_max,
                        int obs_dim, int act_dim, const int* slice_traj, const int* slice_start, long long n_slices,
                        const long long* batch_slices, const long long* draws, int batch, int window, int goal_len,
                        int goal_mode, int min_future_sep, float* obs_out, float* act_out, float* goal_out, void* stream);

/* The vectorised rollout: BesoAgent.predict's window bookkeeping (beso_agent.py:296-388) for n_envs environments whose episodes
 * start and end independently, one launch in front of the sampler call and one behind it.  The rollout's state is caller-owned
 * DEVICE memory that lives from step to step:
 *   lengths [n_envs] int32            observations in each environment's window, 0 ... window
 *   obs_ctx [n_envs, window, obs_dim] the scaled observations (the reference's deque(maxlen = window))
 *   act_ctx [n_envs, window, act_dim] the clipped actions in the scaled domain, slot j beside observation slot j (the
 *                                     reference's deque(maxlen = window - 1): the slot of the newest observation is filled by
 *                                     beso_rollout_end)
 * Slots at or behind an environment's length are never read; the buffers may start uninitialised once every environment's
 * first step carries its reset flag (or `lengths` starts at zero).
 *
 * beso_rollout_begin -- one environment step's inputs:
 *   reset [n_envs] uint8, may be NULL: where set, lengths[n] = 0 first (the reference's reset()).
 *   obs [n_envs, obs_dim] raw observations, scaled as (x - mean[c]) / den[c] -- beso_scale_rows' subtraction and correctly
 *   rounded division, the same bits; mean / den [obs_dim] both NULL: passed through.
 *   The scaled row is appended: with lengths[n] < window into slot lengths[n], and the length grows by one; otherwise both
 *   contexts move down one slot (the oldest leaves) and the row goes into slot window - 1.  The move happens in place and reads
 *   nothing the launch has overwritten.  With t = lengths[n] after the append, the sampler's inputs are written as FULL windows:
 *   state_out [n_envs, window, obs_dim]  the context, slots >= t zero
 *   x_out     [n_envs, window, act_dim]  slots 0 .. t-2 the previous actions, slot t-1 = noise[n] * sigma_max (one fp32 multiply:
 *                                        `torch.randn(...) * self.sigma_max`, noise [n_envs, act_dim]), slots >= t zero
 *   Attention is causal and positions belong to slots, so the tokens of slots < t never see the padding: rows < t of a
 *   denoiser or sampler call on these windows equal the t-slot call to fp32 rounding.  Every element of both outputs is written.
 *
 * beso_rollout_end -- behind the sampler call, with x0 [n_envs, window, act_dim] its result and t = lengths[n]:
 *   a = x0[n, t-1, :] is clipped to [lo, hi] (float64 [act_dim], as Scaler.clip_action's torch.clamp against float64 bounds:
 *   compared in double, rounded to fp32), stored into act_ctx[n, t-1] and written un-scaled to pred [n_envs, act_dim] as
 *   clipped * den_y + mean_y -- a separately rounded multiply and add, Scaler.inverse_scale_output's bits; den_y / mean_y
 *   [act_dim] both NULL: pred is the clipped row.
 *
 * No workspace.  BESO_ERR_BAD_ARG before anything is enqueued: a NULL required pointer, only one of a statistics pair, window,
 * obs_dim or act_dim < 1, n_envs < 0, more than 2^31 - 1 context elements.  n_envs == 0 returns BESO_OK and enqueues nothing.
 * A length outside [0, window] found on the device is clamped into it.                                                    */
int beso_rollout_begin(const float* obs, const uint8_t* reset, const float* noise, const float* mean, const float* den,
                       float sigma_max, int32_t* lengths, float* obs_ctx, float* act_ctx, float* state_out, float* x_out,
                       int n_envs, int window, int obs_dim, int act_dim, void* stream);
int beso_rollout_end(const float* x0, const int32_t* lengths, const double* lo, const double* hi, const float* den_y,
                     const float* mean_y, float* act_ctx, float* pred, int n_envs, int window, int act_dim, void* stream);

/* rand_log_logistic (k_diffusion/utils.py:178-185), the sigma density of the shipped training configs, behind the caller's
 * uniform draw: out[i] = (float) exp(logit(u[i] * (cdf_hi - cdf_lo) + cdf_lo) * scale + loc), every operation in float64 as the
 * reference evaluates it -- one launch instead of seven elementwise ones per training step.  u: n float64 values in [0, 1)
 * (torch.rand(..., dtype=float64): the library has no random number generator); cdf_lo / cdf_hi: the logistic CDF of
 * log(min_value) / log(max_value).                                                                                      */
int beso_log_logistic(const double* u, float* out, size_t n, double loc, double scale, double cdf_lo, double cdf_hi, void* stream);

/* Scaler.scale_input / scale_output (networks/scaler/scaler_class.py:95-117, called three times per batch by
 * BaseAgent.process_batch, base_agent.py:111-142): dst_k[r][c] = (src_k[r][c] - mean_k[c]) / den_k[c] for n <= 4 tensors of
 * rows_k x cols_k fp32 values in ONE launch (den = std + 1e-12, the reference's denominator; a subtraction and a correctly
 * rounded division per element: the reference's bits).  dst_k may be src_k.                                              */
int beso_scale_rows(const float* const* src, float* const* dst, const float* const* mean, const float* const* den,
                    const long long* rows, const int* cols, int n, void* stream);

/* The same call for data-parallel training, where the exchange of the gradients (one all-reduce per range) should start
 * before the backward pass is over.  The gradients of the upper transformer layers l0 .. n_layers-1 and of ln_f are one
 * contiguous range of grads_flat -- [*begin, *end) floats, beso_grad_early_range -- and are completed FIRST: their weight
 * gradients and LayerNorm sums run as soon as the chain of data gradients has passed layer l0 (chosen so that those weight
 * gradients fill one round of workgroups: 4 of the 6 kitchen layers), and `early_stream`
 * (a second hipStream_t) is then made to wait for exactly that point (an event recorded on `stream`).  Work the caller
 * enqueues on early_stream after the call returns -- the all-reduce of that range -- runs under the backward of the
 * lower layers; everything else in grads_flat is final at the end of `stream` as before.  early_stream = NULL is
 * beso_loss_grad.  With fewer than two layers the range is empty and early_stream is left alone.                    */
int beso_grad_early_range(const beso_config* cfg, size_t* begin, size_t* end);
int beso_loss_grad_overlap(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                           const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                           float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                           float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream, void* early_stream);
/* ... and with a third stream for the LOSS: `loss_stream` (NULL: none) is ordered behind the point where *loss_out is final --
 * the end of the forward half, a third of the way into the call's work.  The reference's train_step returns `loss.item()`
 * (beso_agent.py:248); reading the loss on loss_stream lets the host return with it while the backward pass and the optimizer
 * are still running on `stream`, and prepare the next step under them.  The call also uses loss_stream at its start, for the
 * step's copies of the weights (they depend on the parameters only and run beside the embedding of the batch on `stream`;
 * both streams are joined before the first layer): loss_stream must not carry unrelated work of the caller's that the step
 * should not wait for.  beso_loss_grad_streams zeroes `grads_flat` on `loss_stream` (with the weight copies: on `stream` when
 * loss_stream is NULL); the forward on `stream` is ordered behind it, so the caller need not -- and must not rely on an
 * earlier fill of its own surviving.                                          */
int beso_loss_grad_streams(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                           const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                           float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                           float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                           void* stream, void* early_stream, void* loss_stream);
/* ... and with the gradient of the loss with respect to the INPUTS `state` and `goal` -- what the reference's `loss.backward()`
 * passes on to whatever trainable module produced them (an observation or goal encoder).  One more launch at the end of the
 * call's work on `stream`: the rows of the fp32 gradient of the embedded sequence that belong to state and goal tokens,
 * projected back through tok_emb.weight, with this call's embedding dropout applied per (token, feature) and, for the goals,
 * mask_cond's keep-mask per element (the masks of `seed`: beso_dropout_mask(BESO_DROP_EMBED) / beso_goal_mask) -- a goal element
 * the mask zeroed gets gradient exactly 0.  grad_scale is included, as in grads_flat.
 *   state_grad [batch,t,obs], goal_grad [batch,G,obs]: fp32 out, UNINITIALISED on entry, every element written.  Either may be
 *   NULL (not computed); with both NULL the call is beso_loss_grad_streams and enqueues exactly what that enqueues.
 * Every element is summed by one thread in index order, without atomics: equal bits on every call with the same dx, with or
 * without BESO_TRAIN_DETERMINISTIC; the loss and grads_flat do not depend on whether the outputs are asked for.
 * Gradients with respect to action, noise and sigma are not computed.
 * BESO_ERR_BAD_ARG, before anything is enqueued and in addition to beso_loss_grad's checks: goal_grad != NULL with
 * goal_seq_len == 0, an output pointer that is not 4-byte aligned.                                                        */
int beso_loss_grad_inputs(const beso_config* cfg, const float* const* params, int n_params, float* grads_flat, int precision,
                          const float* state, const float* action, const float* goal, const float* noise, const float* sigma,
                          float* loss_out, int batch, int t, int flags, float embed_pdrop, float attn_pdrop, float resid_pdrop,
                          float goal_drop, unsigned int seed, float grad_scale, void* workspace, size_t workspace_bytes,
                          void* stream, void* early_stream, void* loss_stream, float* state_grad, float* goal_grad);
/* beso_denoise_vjp with the same two outputs: (d denoised / d state)^T cot [batch,t,obs] and (d denoised / d goal)^T cot
 * [batch,G,obs] (eval mode: no mask applies; for the unconditional branch the caller passed zero goals and the product with
 * respect to the goals it replaced is zero -- pass goal_grad = NULL).  Same kernel, same checks and NULL rules as above. */
int beso_denoise_vjp_inputs(const beso_config* cfg, const float* const* params, int n_params, int precision, const float* state,
                            const float* x, const float* goal, const float* sigma, const float* cot, float* denoised, float* x_grad,
                            float* dot, int batch, int t, int flags, void* workspace, size_t workspace_bytes, void* stream,
                            float* state_grad, float* goal_grad);
/* Launch-site timers (bench.py's roofline, the launch-count assertions of the tests): while a site is selected ON THE
 * CALLING THREAD, HIP events are recorded on the launch stream around every launch that thread makes at that site (site 0 =
 * off).  beso_profile_read synchronises the events the calling thread recorded, returns their summed elapsed time and count,
 * and clears them.  Thread-local: other threads' calls are neither timed nor affected.                                      */
enum {
    BESO_SITE_OFF = 0, BESO_SITE_GEMM_QKV = 1, BESO_SITE_GEMM_PROJ = 2, BESO_SITE_GEMM_FC1 = 3,
    BESO_SITE_GEMM_FC2 = 4, BESO_SITE_ATTENTION = 5, BESO_SITE_LAYERNORM = 6, BESO_SITE_EMBED = 7,
    BESO_SITE_HEAD = 8, BESO_SITE_FORWARD = 9 /* one whole score-net forward */,
    BESO_SITE_FUSED_LAYER = 10 /* the fused kernels (one-launch kernel, block kernels) */,
    BESO_SITE_SMALL = 11 /* the layers of a forward on the chip-wide small-batch path (one pair of events per forward) */
};
void beso_profile_enable(int site);
int  beso_profile_read(double* total_ms, int* launches);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* BESO_HIP_H */
