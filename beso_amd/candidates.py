"""Best-of-K action selection (include/beso_select.h, csrc/select.hip): K x_T draws per environment go through ONE sampler
call on N K rows, and the rollout acts on the candidates' mean or on the candidate in the densest mode.  Two launches beside
the sampler's: ``expand`` (N windows -> N K sampler rows, a fresh x_T in each row's newest slot) and ``select`` (N K sampled
windows -> N chosen ones).  ``VectorRollout.step(candidates=K)`` and ``BesoAgent.predict_best_of`` are the callers.  GPU only:
there is no torch-op form of either in the package."""
from __future__ import annotations

import torch

from . import _lib

SELECT_MODES = tuple(_lib.SELECT_MODES)


def check_arguments(k, select, bandwidth, use_kde: bool):
    """(K, mode name, bandwidth as a float: 0 is Scott's rule) of a best-of-K call, or ValueError.  Touches no device."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"candidates must be an integer of at least 1, got {k!r}")
    max_k = _lib.SELECT_LIMITS["max_k"]
    if k > max_k:
        raise ValueError(f"candidates = {k}: at most {max_k} per environment are supported")
    if select is None:
        select = "kde" if use_kde else "mean"
    if select not in _lib.SELECT_MODES:
        raise ValueError(f"select must be one of {SELECT_MODES} (None: 'kde' with use_kde, else 'mean'), got {select!r}")
    if bandwidth is None:
        bandwidth = 0.0
    else:
        bandwidth = float(bandwidth)
        if not bandwidth > 0.0 or bandwidth == float("inf"):
            raise ValueError(f"bandwidth must be a positive finite number (None: Scott's rule), got {bandwidth!r}")
    return k, select, bandwidth


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
