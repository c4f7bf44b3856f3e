"""Guides for ``ClassifierGuidedSampleModel`` (classifier_free_sampler.py): callables ``guide(state, a, goal) -> [B, T]`` whose
gradient with respect to ``a`` steers the sampler.  The reference ships the wrapper (classifier_free_sampler.py:56-90) and no
guide of its own; ``MLPGuide`` is the one this package can differentiate inside a single launch (include/beso_guide.h) and, with
``GuideTrainer`` (guide_fit.py), train."""
import ctypes as C

import torch
import torch.nn as nn

from .... import _lib
from ...._instantiate import instantiate
from ....networks.mlps.mlps import MLPNetwork
from .fit_common import row_dims


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class MLPGuide(nn.Module):
    """A learned value, reward or goal-reaching function q(state, a, goal) as an ``MLPNetwork`` with ``output_dim == 1``.

    The network's input row for sample b and window step t is ``[state[b, t, :] | a[b, t, :] | goal[b or 0, G-1, :]]``: the goal
    part only with ``use_goal`` and a goal, so ``input_dim = obs + act (+ obs)``; of a goal sequence the last step is read, and a
    goal given as ``[1, G, obs]`` is shared by all samples.  ``state`` may hold more steps than ``a`` (the first ``T`` are read);
    fewer are refused.

    ``use_sigma``: the guide is a classifier of the NOISED action and its noise level.  The row gains one last column,
    ``c_noise[b] = log(sigma[b]) / 4`` (the value ``GCDenoiser`` feeds its network), so ``input_dim = obs + act (+ obs) + 1``, and
    ``forward`` / ``apply`` take ``sigma [B]``; ``ClassifierGuidedSampleModel`` hands it the sampler's.

    ``network``: a config (``_target_`` + kwargs), a factory or an instance.  ``__call__`` goes through the network's own forward
    (``beso_mlp_fwd``; under autograd ``beso_mlp_bwd``), which makes the guide a valid generic-path guide of
    ``ClassifierGuidedSampleModel`` as well; ``apply`` is the fused launch ``beso_guide_apply`` (``use_sigma``:
    ``beso_guide_apply_sigma``, include/beso_guide_fit.h)."""

    def __init__(self, network, use_goal: bool = True, use_sigma: bool = False):
        super().__init__()
        self.network = network if isinstance(network, nn.Module) else instantiate(network)
        self.use_goal = bool(use_goal)
        self.use_sigma = bool(use_sigma)
        if not isinstance(self.network, MLPNetwork):
            raise TypeError(f"MLPGuide: network must be an MLPNetwork, got {type(self.network).__name__} (any other guide is a plain "
                            "callable for ClassifierGuidedSampleModel)")
        if self.network.output_dim != 1:
            raise ValueError(f"MLPGuide: the network's output_dim must be 1 (a scalar q per row), got {self.network.output_dim}")
        self._fused = {}

    # ------------------------------------------------------------------ shapes
    def _dims(self, state, a, goal):
        """(B, T, obs, act, goal or None) of a call, refusing by name what the guide cannot read."""
        return row_dims("MLPGuide", self.network.input_dim, state, a, goal, self.use_goal, extra=int(self.use_sigma),
                        use_sigma=self.use_sigma)

    def c_noise(self, sigma, B: int, who: str = "MLPGuide"):
        """``log(sigma) / 4`` [B] in fp32 torch ops (None without ``use_sigma``), refusing by name a ``sigma`` the guide cannot
        take: one it has no column for, a missing one, one that is not ``[B]``."""
        if not self.use_sigma:
            if sigma is not None:
                raise ValueError(f"{who}: sigma given to a guide without use_sigma (its rows have no noise-level column)")
            return None
        if sigma is None:
            raise ValueError(f"{who}: a guide with use_sigma needs sigma [B={B}]")
        if not torch.is_tensor(sigma) or sigma.shape != (B,):
            raise ValueError(f"{who}: sigma must be a tensor [B={B}] (use_sigma), got "
                             f"{tuple(sigma.shape) if torch.is_tensor(sigma) else type(sigma).__name__}")
        return sigma.to(torch.float32).log() / 4

    def forward(self, state, a, goal=None, sigma=None) -> torch.Tensor:
        """q [B, T] through ``MLPNetwork.forward``; ``sigma [B]`` with ``use_sigma``, and only then."""
        B, T, obs, act, goal = self._dims(state, a, goal)
        c_noise = self.c_noise(sigma, B)
        parts = [state[:, :T].to(torch.float32), a.to(torch.float32)]
        if goal is not None:
            parts.append(goal[:, -1:, :].to(torch.float32).expand(B, T, obs))
        if c_noise is not None:
            parts.append(c_noise.view(B, 1, 1).expand(B, T, 1))
        return self.network(torch.cat(parts, dim=-1)).squeeze(-1)

    # ------------------------------------------------------------------ the fused launch
    def fused_supported(self, obs: int, act: int, with_goal: bool) -> bool:
        """Whether ``beso_guide_apply`` (``use_sigma``: ``beso_guide_apply_sigma``) serves this network over rows of (obs, act,
        goal or not): asked of the library once per row layout and remembered (the network's dims are fixed at construction)."""
        key = (obs, act, bool(with_goal))
        hit = self._fused.get(key)
        if hit is None:
            supported = (_lib.load_guidefit().beso_guide_supported_sigma if self.use_sigma
                         else _lib.load_guide().beso_guide_supported)
            st = supported(C.byref(self.network.dims()), obs, act, int(with_goal))
            hit = self._fused[key] = st == _lib.OK
        return hit

    def apply(self, state, pred, goal, sigma, lam: float, out=None) -> torch.Tensor:
        """``pred + lam * sigma^2 * d sum(q(state, a, goal)) / da`` at ``a = pred`` as ONE launch; ``out`` may be ``pred``.  With
        ``use_sigma`` q reads ``log(sigma) / 4`` as its last column as well."""
        B, T, obs, act, goal = self._dims(state, pred, goal)
        f32c = lambda t: t.to(torch.float32).contiguous()                      # noqa: E731 (no-ops on what the denoiser returns)
        state, pred, sigma = f32c(state), f32c(pred), f32c(sigma)
        goal = None if goal is None else f32c(goal)
        if not pred.is_cuda or sigma.shape != (B,):
            raise ValueError(f"MLPGuide.apply: GPU tensors and sigma [B={B}] expected, got sigma {tuple(sigma.shape)} on {pred.device}")
        out = torch.empty_like(pred) if out is None else out
        ptrs, n = self.network._pointers(None)
        head = (ptrs, n, C.byref(self.network.dims()), state.data_ptr(), None if goal is None else goal.data_ptr(), pred.data_ptr(),
                sigma.data_ptr())
        tail = (B, T, state.shape[1], 0 if goal is None else goal.shape[1], 0 if goal is None else goal.shape[0], obs, act,
                float(lam), out.data_ptr(), _stream(pred))
        if self.use_sigma:
            c_noise = self.c_noise(sigma, B, "MLPGuide.apply")         # torch's log: the column's bits are the trainer's
            _lib.check(_lib.load_guidefit().beso_guide_apply_sigma(*head, c_noise.data_ptr(), *tail), "beso_guide_apply_sigma")
        else:
            _lib.check(_lib.load_guide().beso_guide_apply(*head, *tail), "beso_guide_apply")
        return out
