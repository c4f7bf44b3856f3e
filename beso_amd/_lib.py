"""ctypes binding of libbeso_hip.so (include/beso_hip.h).  The product path has no CPU fallback:
if the library is missing or fails to load, importing callers get a RuntimeError."""
from __future__ import annotations

import ctypes as C
import functools
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# BESO_HIP_LIB points the binding at another build of the same library (kernel experiments: tools/variants.py)
LIB_PATH = os.environ.get("BESO_HIP_LIB") or os.path.join(_HERE, "lib", "libbeso_hip.so")
DEV_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_hip_dev.so")
MLP_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_mlp.so")      # the MLP encoder (include/beso_mlp.h)
RESMLP_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_resmlp.so")   # the residual MLP encoder (include/beso_resmlp.h)
GUIDE_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_guide.so")     # the guide gradient of guided sampling (include/beso_guide.h)
GUIDEFIT_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_guidefit.so")   # the guide's fit step (include/beso_guide_fit.h)
SELECT_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_select.so")   # best-of-K action selection (include/beso_select.h)
SCALE_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_scale.so")     # MinMaxScaler's scalings (include/beso_scale.h)
NOISE_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_noise.so")     # the rollout's keyed noise (include/beso_noise.h)
RANK_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_rank.so")       # value-ranked best-of-K selection (include/beso_rank.h)
CRITIC_LIB_PATH = os.path.join(_HERE, "lib", "libbeso_critic.so")   # the IQL critic's fit step (include/beso_critic_fit.h)

# Every upper-case integer below is BESO_<name> of include/beso_hip.h, and every table one of its enums
# (tests/test_cabi.py compares the values, and SIGNATURES with the prototypes, against the header's text).
OK, ERR_BAD_CONFIG, ERR_BAD_SHAPE, ERR_BAD_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED, ERR_HIP = 0, -1, -2, -3, -4, -5, -6
PREC_BF16, PREC_FP32, PREC_BF16X3, PREC_FP16 = 0, 1, 2, 3
PRECISIONS = {"bf16": PREC_BF16, "fp32": PREC_FP32, "bf16x3": PREC_BF16X3, "fp16": PREC_FP16}
FLAG_UNCOND = 1
# execution-plan hints of the forward calls (include/beso_hip.h: which kernels run, never what they compute)
PLAN_PER_OP, PLAN_BLOCKS, PLAN_SMALL, PLAN_FUSED = 0x10, 0x20, 0x40, 0x80
PLAN_SPW2, PLAN_SPW4, PLAN_SPW8 = 0x100, 0x200, 0x300
# the sigma token shared across a uniform-sigma batch (kitchen-class shape, bf16 / fp16): at any batch size / never
PLAN_SIGMA_SHARED, PLAN_SIGMA_PRIVATE = 0x400, 0x800
SAMPLE_STEPWISE = 0x1000
FLAG_LAST_ACTION_ONLY = 0x2000     # beso_loss_fwd: only the last step of every window is scored
TRAIN_LAST_ACTION_ONLY, TRAIN_PLAN_PER_OP, TRAIN_PLAN_TILES, TRAIN_DETERMINISTIC = 1, 2, 4, 8
SAMPLER_IDS = {"ddim": 0, "euler": 1, "heun": 2}
# beso_sample_solver (include/beso_hip.h BESO_SOLVER_*): the gc_sampling.py function names without "sample_"
SOLVER_IDS = {"dpm_2": 0, "dpm_2_ancestral": 1, "dpmpp_2s": 2, "dpmpp_2s_ancestral": 3, "dpmpp_2m": 4, "lms": 5}
# every sampler loop the library runs as one enqueue: name -> (C entry point, its sampler / solver id)
SAMPLERS = {**{k: ("beso_sample", v) for k, v in SAMPLER_IDS.items()}, "euler_ancestral": ("beso_sample_ancestral", None),
            **{k: ("beso_sample_solver", v) for k, v in SOLVER_IDS.items()}}
# beso_sample_traced (include/beso_hip.h BESO_ENTRY_*): which of the three sampler calls it runs
ENTRY_IDS = {"beso_sample": 0, "beso_sample_ancestral": 1, "beso_sample_solver": 2}
GOAL_RANDOM, GOAL_TAIL, GOAL_SEQ_END = 0, 1, 2
# beso_dropout_mask (include/beso_hip.h BESO_DROP_*): which nn.Dropout of the network
DROP_EMBED, DROP_ATTN, DROP_PROJ, DROP_MLP = 0, 1, 2, 3
DROP_KINDS = {"embed": DROP_EMBED, "attn": DROP_ATTN, "proj": DROP_PROJ, "mlp": DROP_MLP}
STEP_DDIM, STEP_EULER, STEP_HEUN_PREDICT, STEP_HEUN_CORRECT = 0, 1, 2, 3
SITES = {"off": 0, "gemm_qkv": 1, "gemm_proj": 2, "gemm_fc1": 3, "gemm_fc2": 4, "attention": 5,
         "layernorm": 6, "embed": 7, "head": 8, "forward": 9, "fused_layer": 10, "small": 11}


class BesoConfig(C.Structure):
    """struct beso_config (include/beso_hip.h)."""
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("embed_dim", C.c_int32),
                ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("goal_seq_len", C.c_int32),
                ("obs_seq_len", C.c_int32), ("linear_output", C.c_int32), ("sigma_data", C.c_float)]


vp, i32, u32, i64, f32, f64, sz, cstr = (C.c_void_p, C.c_int, C.c_uint, C.c_longlong, C.c_float, C.c_double, C.c_size_t,
                                         C.c_char_p)
cfgp, vpp, floats = C.POINTER(BesoConfig), C.POINTER(vp), C.POINTER(f32)
# argument lists that several entry points share: each of those is this list plus its own trailing arguments
_adam = [vp, i32, vp, vp, vp, f32, f32, f32, f32, f32, i32, i32, f32]           # beso_adam_step without its stream
_loss_grad = [cfgp, vpp, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, u32, f32, vp, sz, vp]
_denoise_vjp = [cfgp, vpp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]

# every function include/beso_hip.h declares, in its order: name -> (restype, argtypes)
SIGNATURES = {
    "beso_version": (cstr, []),
    "beso_status_string": (cstr, [i32]),
    "beso_last_error": (cstr, []),
    "beso_num_params": (i32, [cfgp]),
    "beso_packed_bytes": (sz, [cfgp, i32]),
    "beso_pack_weights": (i32, [cfgp, vpp, i32, vp, sz, i32, vp]),
    "beso_workspace_bytes": (sz, [cfgp, i32, i32, i32, i32]),
    "beso_score_fwd": (i32, [cfgp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "beso_denoise_fwd": (i32, [cfgp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp, sz, vp]),
    "beso_sampler_step": (i32, [i32, vp, vp, vp, vp, vp, f32, f32, sz, vp]),
    "beso_sample": (i32, [cfgp, vp, i32, i32, vp, vp, vp, i32, i32, floats, i32, f32, i32, vp, sz, vp]),
    "beso_sample_ancestral": (i32, [cfgp, vp, i32, vp, vp, vp, i32, i32, floats, i32, f32, f32, vp, i32, vp, sz, vp]),
    "beso_sample_solver": (i32, [cfgp, vp, i32, i32, vp, vp, vp, i32, i32, floats, i32, f32, f32, f32, i32, vp, vp, i32,
                                 vp, sz, vp]),
    "beso_sample_traced": (i32, [cfgp, vp, i32, i32, i32, vp, vp, vp, i32, i32, floats, i32, f32, f32, f32, i32, vp, vp,
                                 vp, sz, vp, sz, i32, vp, sz, vp]),
    "beso_adam_step": (i32, _adam + [vp]),
    "beso_grad_sumsq": (i32, [vp, i32, vp, vp, vp]),
    "beso_adam_step_clipped": (i32, _adam + [vp, f32, i32, vp]),
    "beso_train_workspace_bytes": (sz, [cfgp, i32, i32, i32]),
    "beso_grad_floats": (sz, [cfgp]),
    "beso_loss_grad": (i32, _loss_grad),
    "beso_denoise_vjp": (i32, _denoise_vjp),
    "beso_loss_fwd_workspace_bytes": (sz, [cfgp, i32, i32, i32]),
    "beso_loss_fwd": (i32, [cfgp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "beso_goal_mask": (i32, [vp, i32, i32, i32, f32, u32, vp]),
    "beso_dropout_mask": (i32, [cfgp, vp, i32, i32, i32, i32, f32, u32, vp]),
    "beso_gather_windows": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp,
                                  vp]),
    "beso_rollout_begin": (i32, [vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "beso_rollout_end": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "beso_log_logistic": (i32, [vp, vp, sz, f64, f64, f64, f64, vp]),
    "beso_scale_rows": (i32, [vp, vp, vp, vp, vp, vp, i32, vp]),
    "beso_grad_early_range": (i32, [cfgp, C.POINTER(sz), C.POINTER(sz)]),
    "beso_loss_grad_overlap": (i32, _loss_grad + [vp]),                 # + early_stream
    "beso_loss_grad_streams": (i32, _loss_grad + [vp, vp]),             # + loss_stream
    "beso_loss_grad_inputs": (i32, _loss_grad + [vp, vp, vp, vp]),      # + state_grad, goal_grad
    "beso_denoise_vjp_inputs": (i32, _denoise_vjp + [vp, vp]),          # + state_grad, goal_grad
    "beso_profile_enable": (None, [i32]),
    "beso_profile_read": (i32, [C.POINTER(f64), C.POINTER(i32)]),
}
# include/beso_hip_debug.h: the development build only (libbeso_hip_dev.so); the product library exports none of them
DEV_SIGNATURES = {
    "beso_debug_set_stamps": (None, [vp, i32]),
    "beso_debug_sigma_cache_entries": (i32, [cfgp, vp, i32]),
    "beso_debug_gemm": (i32, [i32, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp]),
}
EXPORTS, DEV_EXPORTS = list(SIGNATURES), list(DEV_SIGNATURES)


class MlpDims(C.Structure):
    """struct beso_mlp_dims (include/beso_mlp.h)."""
    _fields_ = [("in_dim", C.c_int32), ("hidden_dim", C.c_int32), ("n_hidden", C.c_int32), ("out_dim", C.c_int32),
                ("activation", C.c_int32)]


# include/beso_mlp.h (libbeso_mlp.so): BESO_MLP_ACT_* by the reference's activation names -- "tanh" IS the sigmoid there
# (return_activiation_fcn, networks/utils.py:37-38) -- its flag, and every function it declares, in its order
MLP_ACTIVATIONS = {"ReLU": 0, "Mish": 1, "sigmoid": 2, "tanh": 2}
MLP_FLAGS = {"accumulate": 1}        # BESO_MLP_ACCUMULATE
dimsp = C.POINTER(MlpDims)
MLP_SIGNATURES = {
    "beso_mlp_workspace_bytes": (sz, [dimsp, i64, i32]),
    "beso_mlp_fwd": (i32, [vpp, i32, dimsp, vp, i64, vp, vp, vp]),
    "beso_mlp_bwd": (i32, [vpp, i32, dimsp, vp, vp, i64, vp, vp, vp, sz, i32, vp]),
}


class ResMlpDims(C.Structure):
    """struct beso_resmlp_dims (include/beso_resmlp.h)."""
    _fields_ = [("in_dim", C.c_int32), ("hidden_dim", C.c_int32), ("n_blocks", C.c_int32), ("out_dim", C.c_int32),
                ("activation", C.c_int32), ("norm", C.c_int32)]


# include/beso_resmlp.h (libbeso_resmlp.so): BESO_RESMLP_NORM_* and every function it declares, in its order; the activations
# and the accumulate flag are include/beso_mlp.h's
RESMLP_NORMS = {"none": 0, "LayerNorm": 1}
rdimsp = C.POINTER(ResMlpDims)
RESMLP_SIGNATURES = {
    "beso_resmlp_workspace_bytes": (sz, [rdimsp, i64, i32]),
    "beso_resmlp_fwd": (i32, [vpp, i32, rdimsp, vp, i64, vp, vp, vp]),
    "beso_resmlp_bwd": (i32, [vpp, i32, rdimsp, vp, vp, i64, vp, vp, vp, sz, i32, vp]),
}

# include/beso_guide.h (libbeso_guide.so): every function it declares, in its order; the dims struct and the activations are
# include/beso_mlp.h's
GUIDE_SIGNATURES = {
    "beso_guide_supported": (i32, [dimsp, i32, i32, i32]),
    "beso_guide_apply": (i32, [vpp, i32, dimsp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp]),
}
GUIDE_EXPORTS = list(GUIDE_SIGNATURES)

# include/beso_guide_fit.h (libbeso_guidefit.so): BESO_GUIDE_FIT_* by GuideTrainer's loss names, and every function it declares,
# in its order; beso_guide_apply_sigma is beso_guide_apply with c_noise behind sigma
GUIDEFIT_LOSSES = {"mse": 0, "bce": 1}
GUIDEFIT_SIGNATURES = {
    "beso_guide_fit_rows": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    "beso_guide_fit_loss": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp]),
    "beso_guide_supported_sigma": (i32, [dimsp, i32, i32, i32]),
    "beso_guide_apply_sigma": (i32, [vpp, i32, dimsp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp, vp]),
}
GUIDEFIT_EXPORTS = list(GUIDEFIT_SIGNATURES)

# include/beso_select.h (libbeso_select.so): BESO_SELECT_* by the rollout's names, its limits, and every function it declares,
# in its order
SELECT_MODES = {"mean": 0, "kde": 1}
SELECT_LIMITS = {"max_k": 256, "max_act": 64}        # BESO_SELECT_MAX_K, BESO_SELECT_MAX_ACT
SELECT_SIGNATURES = {
    "beso_candidates_last_error": (cstr, []),
    "beso_candidates_expand": (i32, [vp, vp, vp, vp, f32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "beso_candidates_select": (i32, [vp, vp, i32, f32, i32, i32, i32, i32, vp, vp, vp, vp]),
}
SELECT_EXPORTS = list(SELECT_SIGNATURES)

# include/beso_scale.h (libbeso_scale.so): BESO_SCALE_* by what MinMaxScaler.scale_many calls them, its limit, and every function
# it declares, in its order
SCALE_KINDS = {"zscore": 0, "minmax": 1}
SCALE_LIMITS = {"max_items": 4}                      # BESO_SCALE_MAX_ITEMS
SCALE_SIGNATURES = {
    "beso_scale_last_error": (cstr, []),
    "beso_scale_rows_mixed": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    "beso_rollout_end_minmax": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
}
SCALE_EXPORTS = list(SCALE_SIGNATURES)

# include/beso_noise.h (libbeso_noise.so): BESO_NOISE_* by what the rollout draws, its limit, and every function it declares, in
# its order
NOISE_PURPOSES = {"x_t": 0, "candidate": 1, "step": 2}
NOISE_LIMITS = {"max_purpose": 15}                   # BESO_NOISE_MAX_PURPOSE
NOISE_SIGNATURES = {
    "beso_noise_last_error": (cstr, []),
    "beso_noise_words": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "beso_noise_normal": (i32, [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp]),
    "beso_noise_rollout": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
}
NOISE_EXPORTS = list(NOISE_SIGNATURES)

# include/beso_rank.h (libbeso_rank.so): its limits and every function it declares, in its order; the dims struct and the
# activations are include/beso_mlp.h's
RANK_LIMITS = {"max_k": 256, "max_act": 64}          # BESO_RANK_MAX_K, BESO_RANK_MAX_ACT
RANK_SIGNATURES = {
    "beso_rank_last_error": (cstr, []),
    "beso_rank_supported": (i32, [dimsp, i32, i32, i32]),
    "beso_rank_candidates": (i32, [vpp, i32, dimsp, vp, vp, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
}
RANK_EXPORTS = list(RANK_SIGNATURES)

# include/beso_critic_fit.h (libbeso_critic.so): every function it declares, in its order
CRITIC_SIGNATURES = {
    "beso_critic_last_error": (cstr, []),
    "beso_critic_rows": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    "beso_critic_loss": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp]),
}
CRITIC_EXPORTS = list(CRITIC_SIGNATURES)


class BesoHipError(RuntimeError):
    pass


def _bind(lib: C.CDLL, table, tolerant: bool) -> C.CDLL:
    """Declare every function of `table` on `lib`.  A symbol the library lacks raises (AttributeError), unless `tolerant`:
    then that symbol alone stays unbound and a caller that needs it fails on first use."""
    for name, (restype, argtypes) in table.items():
        if tolerant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    return lib


_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load the HIP library (once).  Fails loudly -- there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch bundles its own libamdhip64.so.7; it must be the HIP runtime of the process BEFORE this
        # library is mapped, so that both resolve to the same runtime instance (streams and device
        # pointers are handed across).  Loading ours first would pull in /opt/rocm's copy as a second
        # runtime and every launch on a torch stream would fail.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise BesoHipError(
                f"{LIB_PATH} not found: build it with `python -m beso_amd.build` (hipcc, gfx950). "
                "beso_amd has no CPU or eager fallback for the score-denoising path.")
        # a library named by BESO_HIP_LIB may be an A/B build of an older revision (tools/variants.py '@<revision>') that
        # predates some entry points: those are skipped, one by one.  The tree's own library must have them all.
        _lib = _bind(C.CDLL(LIB_PATH), SIGNATURES, tolerant=bool(os.environ.get("BESO_HIP_LIB")))
    return _lib


# the libraries beside the product library, built with it: name -> (path, signatures, header, what has no fallback, the symbol
# of its own last-error message and the prefix of the exceptions check_side raises with it: None where it keeps no message)
_SIDE = {"mlp": (MLP_LIB_PATH, MLP_SIGNATURES, "beso_mlp.h", "the encoder", None, None),
         "resmlp": (RESMLP_LIB_PATH, RESMLP_SIGNATURES, "beso_resmlp.h", "the encoder", None, None),
         "guide": (GUIDE_LIB_PATH, GUIDE_SIGNATURES, "beso_guide.h", "the fused guide gradient", None, None),
         "guidefit": (GUIDEFIT_LIB_PATH, GUIDEFIT_SIGNATURES, "beso_guide_fit.h", "the guide's fit step", None, None),
         "select": (SELECT_LIB_PATH, SELECT_SIGNATURES, "beso_select.h", "best-of-K action selection",
                    "beso_candidates_last_error", "beso_select"),
         "scale": (SCALE_LIB_PATH, SCALE_SIGNATURES, "beso_scale.h", "MinMaxScaler's one-launch scalings",
                   "beso_scale_last_error", "beso_scale"),
         "noise": (NOISE_LIB_PATH, NOISE_SIGNATURES, "beso_noise.h", "the rollout's keyed noise",
                   "beso_noise_last_error", "beso_noise"),
         "rank": (RANK_LIB_PATH, RANK_SIGNATURES, "beso_rank.h", "value-ranked best-of-K action selection",
                  "beso_rank_last_error", "beso_rank"),
         "critic": (CRITIC_LIB_PATH, CRITIC_SIGNATURES, "beso_critic_fit.h", "the IQL critic's fit step",
                    "beso_critic_last_error", "beso_critic")}
_side = {}


def _load_side(name: str) -> C.CDLL:
    """Load one library of _SIDE (once), as load() does the product library.  No fallback either."""
    if name not in _side:
        with _lock:
            if name not in _side:
                import torch  # noqa: F401      (the HIP runtime of the process: see load())
                path, table, header, what = _SIDE[name][:4]
                if not os.path.exists(path):
                    raise BesoHipError(f"{path} (include/{header}) not found: build it with `python -m beso_amd.build` (hipcc, "
                                       f"gfx950). beso_amd has no CPU or eager fallback for {what}.")
                _side[name] = _bind(C.CDLL(path), table, tolerant=False)
    return _side[name]


def check_side(name: str, status: int, what: str) -> None:
    """check() for a library of _SIDE that keeps its own message (select, scale, noise, rank, critic): the message names what was refused."""
    if status == OK:
        return
    last_error, prefix = _SIDE[name][4:]
    text = f"{prefix}: {what}: {getattr(_load_side(name), last_error)().decode()} (status {status})"
    if status in (ERR_BAD_SHAPE, ERR_BAD_ARG, ERR_UNSUPPORTED):
        raise ValueError(text)
    raise BesoHipError(text)


check_select = functools.partial(check_side, "select")
check_scale = functools.partial(check_side, "scale")
check_noise_status = functools.partial(check_side, "noise")
check_rank = functools.partial(check_side, "rank")
check_critic = functools.partial(check_side, "critic")


def load_mlp() -> C.CDLL:
    """The MLP encoder's library (include/beso_mlp.h)."""
    return _load_side("mlp")


def load_resmlp() -> C.CDLL:
    """The residual MLP encoder's library (include/beso_resmlp.h)."""
    return _load_side("resmlp")


def load_guide() -> C.CDLL:
    """The guide-gradient library of classifier-guided sampling (include/beso_guide.h).  A guide it does not serve takes
    autograd over the guide's own HIP kernels, decided once per guide."""
    return _load_side("guide")


def load_guidefit() -> C.CDLL:
    """The library of the guide's fit step and of the guide gradient over rows with the noise-level column
    (include/beso_guide_fit.h)."""
    return _load_side("guidefit")


def load_select() -> C.CDLL:
    """The best-of-K action selection library of the rollout (include/beso_select.h)."""
    return _load_side("select")


def load_scale() -> C.CDLL:
    """The library of MinMaxScaler's scalings (include/beso_scale.h)."""
    return _load_side("scale")


def load_noise() -> C.CDLL:
    """The library of the rollout's keyed noise (include/beso_noise.h)."""
    return _load_side("noise")


def load_rank() -> C.CDLL:
    """The value-ranked best-of-K selection library of the rollout (include/beso_rank.h)."""
    return _load_side("rank")


def load_critic() -> C.CDLL:
    """The library of the IQL critic's fit step (include/beso_critic_fit.h)."""
    return _load_side("critic")


_dev = None


def load_dev() -> C.CDLL:
    """The development build (`python -m beso_amd.build --dev`, include/beso_hip_debug.h): phase stamps and the GEMM layout
    probe.  A separate library image with its own state; nothing in the package uses it."""
    global _dev
    if _dev is None:
        import torch  # noqa: F401      (the HIP runtime of the process: see load())
        if not os.path.exists(DEV_LIB_PATH):
            raise BesoHipError(f"{DEV_LIB_PATH} not found: build it with `python -m beso_amd.build --dev`")
        _dev = _bind(C.CDLL(DEV_LIB_PATH), DEV_SIGNATURES, tolerant=False)
    return _dev


def check(status: int, what: str = "") -> None:
    """Non-zero status -> exception.  Shape/config/argument errors are ValueError, matching the
    reference's conventions (ValueError for unknown sampler / schedule: beso_agent.py:455,598;
    `assert t <= block_size`: score_gpts.py:282); runtime failures are BesoHipError."""
    if status == OK:
        return
    msg = load().beso_status_string(status).decode()
    text = f"beso_hip: {what + ': ' if what else ''}{msg} (status {status})"
    if status in (ERR_BAD_CONFIG, ERR_BAD_SHAPE, ERR_BAD_ARG, ERR_UNSUPPORTED):
        raise ValueError(text)
    if status == ERR_HIP:
        text += ": " + load().beso_last_error().decode()
    raise BesoHipError(text)


def launch(name: str, entry: str, dev, *args) -> None:
    """Enqueue `entry` of the product library (`name` "hip") or of the library `name` of _SIDE on the current stream of `dev`,
    which is appended to `args`, and raise on a non-zero status with that library's checker ("beso_rollout_end" is reported as
    "rollout_end").  The entry point is looked up on the library object at every call, so that a test which replaces it there
    sees the call."""
    import torch
    from .runtime import stream_ptr
    side = name != "hip"
    lib = _load_side(name) if side else load()
    with torch.cuda.device(dev):
        status = getattr(lib, entry)(*args, stream_ptr(dev))
    (functools.partial(check_side, name) if side else check)(status, entry[len("beso_"):])
