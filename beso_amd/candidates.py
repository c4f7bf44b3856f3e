"""Best-of-K action selection (include/beso_select.h, csrc/select.hip): K x_T draws per environment go through ONE sampler
call on N K rows, and the rollout acts on the candidates' mean or on the candidate in the densest mode.  Two launches beside
the sampler's: ``expand`` (N windows -> N K sampler rows, a fresh x_T in each row's newest slot) and ``select`` (N K sampled
windows -> N chosen ones).  ``select='value'`` takes ``rank`` in place of ``select``: the candidate an ``MLPGuide`` q scores
highest (include/beso_rank.h, csrc/rank.hip).  ``VectorRollout.step(candidates=K)`` and ``BesoAgent.predict_best_of`` are the
callers.  GPU only: there is no torch-op form of any of them in the package."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

VALUE = "value"                                          # the mode of ``rank``: no BESO_SELECT_* value, a library of its own
SELECT_MODES = tuple(_lib.SELECT_MODES) + (VALUE,)


def check_arguments(k, select, bandwidth, use_kde: bool):
    """(K, mode name, bandwidth as a float: 0 is Scott's rule) of a best-of-K call, or ValueError.  Touches no device."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"candidates must be an integer of at least 1, got {k!r}")
    max_k = _lib.SELECT_LIMITS["max_k"]
    if k > max_k:
        raise ValueError(f"candidates = {k}: at most {max_k} per environment are supported")
    if select is None:
        select = "kde" if use_kde else "mean"
    if select not in SELECT_MODES:
        raise ValueError(f"select must be one of {SELECT_MODES} (None: 'kde' with use_kde, else 'mean'), got {select!r}")
    if select == VALUE and bandwidth is not None:
        raise ValueError(f"bandwidth belongs to select='kde'; select='value' ranks by the guide's q, got bandwidth={bandwidth!r}")
    if bandwidth is None:
        bandwidth = 0.0
    else:
        bandwidth = float(bandwidth)
        if not bandwidth > 0.0 or bandwidth == float("inf"):
            raise ValueError(f"bandwidth must be a positive finite number (None: Scott's rule), got {bandwidth!r}")
    return k, select, bandwidth


def check_guide(select, guide, obs_dim: int, act_dim: int, with_goal: bool, device, who: str = "candidates"):
    """The guide of a best-of-K call: None unless ``select == 'value'``, then an ``MLPGuide`` without ``use_sigma`` on `device`
    whose network ``beso_rank_supported`` serves over rows ``[obs | act (| obs: use_goal and a goal)]``.  Anything else is a
    ValueError (a callable that is no ``MLPGuide``: TypeError) by name.  Reads the guide's dims only: touches no device."""
    from .agents.diffusion_agents.k_diffusion.guides import MLPGuide
    if select != VALUE:
        if guide is not None:
            raise ValueError(f"{who}: guide belongs to select='value' (got select={select!r}): the other modes score nothing with it")
        return None
    if guide is None:
        raise ValueError(f"{who}: select='value' needs guide=<an MLPGuide>: the q that ranks the candidates")
    if not isinstance(guide, MLPGuide):
        raise TypeError(f"{who}: select='value' ranks with an MLPGuide (include/beso_rank.h), got {type(guide).__name__}; another "
                        "callable can steer ClassifierGuidedSampleModel, but the ranking launch cannot evaluate it")
    if guide.use_sigma:
        raise ValueError(f"{who}: a guide with use_sigma=True cannot rank: its rows carry a noise-level column, which final samples "
                         "do not have")
    net = guide.network
    with_goal = bool(with_goal and guide.use_goal)
    want = obs_dim + act_dim + (obs_dim if with_goal else 0)
    if net.input_dim != want:
        raise ValueError(f"{who}: the guide network's input_dim={net.input_dim}, but obs + act{' + obs' if with_goal else ''} = {want} "
                         f"(obs={obs_dim}, act={act_dim}, use_goal={guide.use_goal}, a goal {'is' if with_goal else 'is not'} ranked with)")
    first = next(iter(net.parameters()), None)
    if first is not None and torch.device(first.device) != torch.device(device):
        raise ValueError(f"{who}: the guide is on {first.device}, the model on {device}")
    lib = _lib.load_rank()
    status = lib.beso_rank_supported(C.byref(net.dims()), obs_dim, act_dim, int(with_goal))
    if status != _lib.OK:
        raise ValueError(f"{who}: the ranking launch does not serve this guide: {lib.beso_rank_last_error().decode()} (status {status})")
    return guide


def check_noise(noise, n: int, k: int, act_dim: int, device):
    """The x_T draws [n, k, act] of a best-of-K call on `device`: the caller's, or ``torch.randn``.  A wrong shape is a
    ValueError before anything is moved."""
    if noise is None:
        return torch.randn((n, k, act_dim), device=device)
    noise = torch.as_tensor(noise)
    if tuple(noise.shape) != (n, k, act_dim):
        raise ValueError(f"noise must be [{n}, {k}, {act_dim}], got {tuple(noise.shape)}")
    return noise.to(device=device, dtype=torch.float32).contiguous()


def _f32(v: torch.Tensor, shape, name: str) -> torch.Tensor:
    if not v.is_cuda or v.dtype != torch.float32 or tuple(v.shape) != tuple(shape):
        raise ValueError(f"{name} must be a float32 GPU tensor of shape {tuple(shape)}, got {v.dtype} {tuple(v.shape)} on {v.device}")
    return v.contiguous()


def expand(state: torch.Tensor, x: torch.Tensor, lengths: torch.Tensor, noise: torch.Tensor, sigma_max: float):
    """``beso_candidates_expand``: state [N, W, obs], x [N, W, act], lengths [N] int32 and noise [N, K, act] ->
    (state_k [N K, W, obs], x_k [N K, W, act]); slot ``lengths[n] - 1`` of row ``n K + k`` of x_k is ``noise[n, k] * sigma_max``."""
    N, W, obs = state.shape
    act, K = x.shape[2], noise.shape[1]
    state, x, noise = _f32(state, (N, W, obs), "state"), _f32(x, (N, W, act), "x"), _f32(noise, (N, K, act), "noise")
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (N,) or lengths.device != state.device:
        raise ValueError(f"lengths must be an int32 tensor [{N}] beside state")
    dev = state.device
    state_k = torch.empty((N * K, W, obs), dtype=torch.float32, device=dev)
    x_k = torch.empty((N * K, W, act), dtype=torch.float32, device=dev)
    _lib.launch("select", "beso_candidates_expand", dev, state.data_ptr(), x.data_ptr(), lengths.contiguous().data_ptr(),
                noise.data_ptr(), float(sigma_max), N, W, obs, act, K, state_k.data_ptr(), x_k.data_ptr())
    return state_k, x_k


def select(x0_k: torch.Tensor, lengths: torch.Tensor, k: int, mode: str, bandwidth: float = 0.0):
    """``beso_candidates_select``: the sampler's result x0_k [N K, W, act] -> (x0 [N, W, act], index [N] int32, scores [N, K]);
    `mode` is 'mean' or 'kde', `bandwidth` 0 Scott's rule."""
    NK, W, act = x0_k.shape
    if NK % k:
        raise ValueError(f"{NK} sampled rows are not a multiple of {k} candidates")
    N = NK // k
    x0_k = _f32(x0_k, (NK, W, act), "x0_k")
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (N,) or lengths.device != x0_k.device:
        raise ValueError(f"lengths must be an int32 tensor [{N}] beside x0_k")
    dev = x0_k.device
    x0 = torch.empty((N, W, act), dtype=torch.float32, device=dev)
    index = torch.empty(N, dtype=torch.int32, device=dev)
    scores = torch.empty((N, k), dtype=torch.float32, device=dev)
    _lib.launch("select", "beso_candidates_select", dev, x0_k.data_ptr(), lengths.contiguous().data_ptr(), _lib.SELECT_MODES[mode],
                float(bandwidth), N, W, act, k, x0.data_ptr(), index.data_ptr(), scores.data_ptr())
    return x0, index, scores


def rank(state: torch.Tensor, goal, x0_k: torch.Tensor, lengths: torch.Tensor, k: int, guide):
    """``beso_rank_candidates``: the un-expanded state [N, W, obs], the goal [N or 1, G, obs] or None, the sampler's result x0_k
    [N K, W, act] and an ``MLPGuide`` -> (x0 [N, W, act], index [N] int32, scores [N, K]): scores the guide's q of every
    candidate's newest action beside its environment's newest observation, index their argmax (the lowest k among equals, never
    a NaN score beside another), x0 the chosen rows' windows.  ONE launch.  The goal is read only with ``guide.use_goal``."""
    NK, W, act = x0_k.shape
    if NK % k:
        raise ValueError(f"{NK} sampled rows are not a multiple of {k} candidates")
    N = NK // k
    x0_k = _f32(x0_k, (NK, W, act), "x0_k")
    if state.dim() != 3:
        raise ValueError(f"state must be [N, W, obs], got {tuple(state.shape)}")
    obs = state.shape[2]
    state = _f32(state, (N, W, obs), "state")
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (N,) or lengths.device != x0_k.device:
        raise ValueError(f"lengths must be an int32 tensor [{N}] beside x0_k")
    goal = goal if guide.use_goal and goal is not None else None
    if goal is not None:
        if goal.dim() != 3 or goal.shape[0] not in (1, N) or goal.shape[2] != obs:
            raise ValueError(f"goal must be [{N} or 1, G, {obs}], got {tuple(goal.shape)}")
        goal = _f32(goal, tuple(goal.shape), "goal")
    dev = x0_k.device
    net = guide.network
    ptrs, n_params = net._pointers(None)
    x0 = torch.empty((N, W, act), dtype=torch.float32, device=dev)
    index = torch.empty(N, dtype=torch.int32, device=dev)
    scores = torch.empty((N, k), dtype=torch.float32, device=dev)
    _lib.launch("rank", "beso_rank_candidates", dev, ptrs, n_params, C.byref(net.dims()), state.data_ptr(),
                None if goal is None else goal.data_ptr(), 0 if goal is None else goal.shape[1], 0 if goal is None else goal.shape[0],
                x0_k.data_ptr(), lengths.contiguous().data_ptr(), N, W, obs, act, k, x0.data_ptr(), index.data_ptr(), scores.data_ptr())
    return x0, index, scores
