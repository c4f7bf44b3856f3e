"""Guides for ``ClassifierGuidedSampleModel`` (classifier_free_sampler.py): callables ``guide(state, a, goal) -> [B, T]`` whose
gradient with respect to ``a`` steers the sampler.  The reference ships the wrapper (classifier_free_sampler.py:56-90) and no
guide of its own; ``MLPGuide`` is the one this package can differentiate inside a single launch (include/beso_guide.h)."""
import ctypes as C

import torch
import torch.nn as nn

from .... import _lib
from ...._instantiate import instantiate
from ....networks.mlps.mlps import MLPNetwork


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class MLPGuide(nn.Module):
    """A learned value, reward or goal-reaching function q(state, a, goal) as an ``MLPNetwork`` with ``output_dim == 1``.

    The network's input row for sample b and window step t is ``[state[b, t, :] | a[b, t, :] | goal[b or 0, G-1, :]]``: the goal
    part only with ``use_goal`` and a goal, so ``input_dim = obs + act (+ obs)``; of a goal sequence the last step is read, and a
    goal given as ``[1, G, obs]`` is shared by all samples.  ``state`` may hold more steps than ``a`` (the first ``T`` are read);
    fewer are refused.

    ``network``: a config (``_target_`` + kwargs), a factory or an instance.  ``__call__`` goes through the network's own forward
    (``beso_mlp_fwd``; under autograd ``beso_mlp_bwd``), which makes the guide a valid generic-path guide of
    ``ClassifierGuidedSampleModel`` as well; ``apply`` is the fused launch ``beso_guide_apply``."""

    def __init__(self, network, use_goal: bool = True):
        super().__init__()
        self.network = network if isinstance(network, nn.Module) else instantiate(network)
        self.use_goal = bool(use_goal)
        if not isinstance(self.network, MLPNetwork):
            raise TypeError(f"MLPGuide: network must be an MLPNetwork, got {type(self.network).__name__} (any other guide is a plain "
                            "callable for ClassifierGuidedSampleModel)")
        if self.network.output_dim != 1:
            raise ValueError(f"MLPGuide: the network's output_dim must be 1 (a scalar q per row), got {self.network.output_dim}")
        self._fused = {}

    # ------------------------------------------------------------------ shapes
    def _dims(self, state, a, goal):
        """(B, T, obs, act, goal or None) of a call, refusing by name what the guide cannot read."""
        if state.dim() != 3 or a.dim() != 3 or state.shape[0] != a.shape[0]:
            raise ValueError(f"MLPGuide: state {tuple(state.shape)} and a {tuple(a.shape)} must be [B, steps, dim] with one B")
        B, T, act = a.shape
        if state.shape[1] < T:
            raise ValueError(f"MLPGuide: state has {state.shape[1]} steps, fewer than a's {T}")
        obs = state.shape[2]
        goal = goal if self.use_goal and goal is not None else None
        if goal is not None and (goal.dim() != 3 or goal.shape[2] != obs or goal.shape[0] not in (1, B)):
            raise ValueError(f"MLPGuide: goal {tuple(goal.shape)} must be [B or 1, G, obs={obs}]")
        want = obs + act + (obs if goal is not None else 0)
        if self.network.input_dim != want:
            raise ValueError(f"MLPGuide: the network's input_dim={self.network.input_dim}, but obs + act"
                             f"{' + obs' if goal is not None else ''} = {want} (use_goal={self.use_goal})")
        return B, T, obs, act, goal

    def forward(self, state, a, goal=None) -> torch.Tensor:
        """q [B, T] through ``MLPNetwork.forward``."""
        B, T, obs, act, goal = self._dims(state, a, goal)
        parts = [state[:, :T].to(torch.float32), a.to(torch.float32)]
        if goal is not None:
            parts.append(goal[:, -1:, :].to(torch.float32).expand(B, T, obs))
        return self.network(torch.cat(parts, dim=-1)).squeeze(-1)

    # ------------------------------------------------------------------ the fused launch
    def fused_supported(self, obs: int, act: int, with_goal: bool) -> bool:
        """Whether ``beso_guide_apply`` serves this network over rows of (obs, act, goal or not): asked of the library once per
        row layout and remembered (the network's dims are fixed at construction)."""
        key = (obs, act, bool(with_goal))
        hit = self._fused.get(key)
        if hit is None:
            st = _lib.load_guide().beso_guide_supported(C.byref(self.network.dims()), obs, act, int(with_goal))
            hit = self._fused[key] = st == _lib.OK
        return hit

    def apply(self, state, pred, goal, sigma, lam: float, out=None) -> torch.Tensor:
        """``pred + lam * sigma^2 * d sum(q(state, a, goal)) / da`` at ``a = pred`` as ONE launch; ``out`` may be ``pred``."""
        B, T, obs, act, goal = self._dims(state, pred, goal)
        f32c = lambda t: t.to(torch.float32).contiguous()                      # noqa: E731 (no-ops on what the denoiser returns)
        state, pred, sigma = f32c(state), f32c(pred), f32c(sigma)
        goal = None if goal is None else f32c(goal)
        if not pred.is_cuda or sigma.shape != (B,):
            raise ValueError(f"MLPGuide.apply: GPU tensors and sigma [B={B}] expected, got sigma {tuple(sigma.shape)} on {pred.device}")
        out = torch.empty_like(pred) if out is None else out
        ptrs, n = self.network._pointers(None)
        st = _lib.load_guide().beso_guide_apply(
            ptrs, n, C.byref(self.network.dims()), state.data_ptr(), None if goal is None else goal.data_ptr(), pred.data_ptr(),
            sigma.data_ptr(), B, T, state.shape[1], 0 if goal is None else goal.shape[1], 0 if goal is None else goal.shape[0],
            obs, act, float(lam), out.data_ptr(), _stream(pred))
        _lib.check(st, "beso_guide_apply")
        return out
