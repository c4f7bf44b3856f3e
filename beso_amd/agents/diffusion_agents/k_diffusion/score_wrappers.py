"""Drop-in for ``beso...k_diffusion.score_wrappers.GCDenoiser``: the Karras et al. (2022)
preconditioner around the score transformer (reference: score_wrappers.py:18-99).

With a ``beso_amd`` DiffusionGPT inside, ``forward`` is ONE call into the HIP library
(``beso_denoise_fwd``): c_in is folded into the token-embedding kernel, c_out / c_skip into the
action-head kernel.  Any other inner model is evaluated by the textbook formula on top of it.
"""
import torch
from torch import nn

from ...._instantiate import instantiate
from .score_gpts import DiffusionGPT
from .utils import append_dims
from ....training import HipTrainStep, ScoreMatchingLoss


class GCDenoiser(nn.Module):
    """D_theta(a; s, g, sigma) = c_skip * a + c_out * F(s, c_in * a, g, sigma)."""

    def __init__(self, inner_model, sigma_data=1.):
        super().__init__()
        self.inner_model = inner_model if isinstance(inner_model, nn.Module) else instantiate(inner_model)
        self.sigma_data = sigma_data
        self._train_steps = {}
        self.deterministic_training = False      # BESO_TRAIN_DETERMINISTIC on every HIP training step of this denoiser

    # -- reference surface ---------------------------------------------------------------------
    def get_scalings(self, sigma):
        """(c_skip, c_out, c_in) of score_wrappers.py:40-42."""
        sd2 = self.sigma_data ** 2
        total = sigma ** 2 + sd2
        return sd2 / total, sigma * self.sigma_data / total ** 0.5, 1 / total ** 0.5

    def get_params(self):
        return self.inner_model.parameters()

    def forward(self, state, action, goal, sigma, **kwargs):
        inner = self.inner_model
        if self._fused(inner, kwargs, state, action, goal, sigma):
            out = inner.runtime(self.sigma_data).denoise(
                inner.packed_weights(), state, action, goal, sigma,
                uncond=bool(kwargs.get("uncond", False)), precondition=True)
            return out
        c_skip, c_out, c_in = (append_dims(c, action.ndim) for c in self.get_scalings(sigma))
        return inner(state, action * c_in, goal, sigma, **kwargs) * c_out + action * c_skip

    def loss(self, state, action, goal, noise, sigma, **kwargs):
        """Score-matching objective (score_wrappers.py:45-79).  Mutates ``noise`` in place when
        ``pred_last_action_only`` is set, like the reference (:63).  Under autograd: the HIP training step -- ``backward()``
        delivers the parameter gradients and, where ``state`` / ``goal`` require grad (the outputs of a trainable observation or
        goal encoder), the gradients with respect to those; ``action``, ``noise`` and ``sigma`` must not require grad.  With autograd
        disabled and the module in eval mode: the held-out objective on the inference path (``beso_loss_fwd``), a plain
        tensor without ``grad_fn``, in the module's precision and on the weights ``packed_weights()`` returns (the EMA image
        inside ``use_weights``); in training mode that call raises -- the masked, dropped-out loss is a training-step quantity."""
        last_only = bool(kwargs.pop("pred_last_action_only", False))
        if last_only:
            noise[:, :-1, :] = 0                                   # in place, like the reference (:63)
        inner = self.inner_model
        if isinstance(inner, DiffusionGPT):
            # forward + every parameter gradient in one enqueue of beso_loss_grad (beso_amd/training.py); there is no
            # torch-op evaluation behind it: what the kernels cannot serve raises
            if kwargs:
                raise ValueError(f"GCDenoiser.loss: unsupported keyword arguments {sorted(kwargs)} for the HIP training step")
            if not torch.is_grad_enabled():
                # the held-out objective: the eval-mode network on the inference path (beso_loss_fwd), no gradient anywhere
                return self._loss_forward(state, action, goal, noise, sigma, last_only=last_only)
            step = self.hip_train_step(state, action, goal, noise, sigma)
            if step is None:
                raise ValueError("GCDenoiser.loss: " + self._why_no_hip_step(state, action, goal, noise, sigma))
            # (training-mode goal masking -- DiffusionGPT.mask_cond, score_gpts.py:298-299 -- happens inside the kernel)
            return ScoreMatchingLoss.apply(step, last_only, state, action, goal, noise, sigma, *inner.parameters())
        # a foreign inner model (any callable score network): the textbook objective on top of it
        noised = action + noise * append_dims(sigma, action.ndim)
        c_skip, c_out, c_in = (append_dims(c, action.ndim) for c in self.get_scalings(sigma))
        out = inner(state, noised * c_in, goal, sigma, **kwargs)
        target = (action - c_skip * noised) / c_out
        if last_only:
            return (out[:, -1, :] - target[:, -1, :]).pow(2).mean()
        return (out - target).pow(2).flatten(1).mean()

    def loss_per_sample(self, state, action, goal, noise, sigma, uncond: bool = False, pred_last_action_only: bool = False):
        """[B]: every sample's score-matching loss on the eval-mode network (``beso_loss_fwd``) -- the mean of
        (F(c_in * noised) - target)^2 over the sample's window, or over its last step with ``pred_last_action_only`` (which
        zeroes ``noise[:, :-1]`` in place, as ``loss`` does).  Their mean is the scalar ``loss`` returns under
        ``torch.no_grad()``.  No gradient is computed; the module must be in eval mode."""
        if pred_last_action_only:
            noise[:, :-1, :] = 0
        return self._loss_forward(state, action, goal, noise, sigma, uncond=uncond, last_only=bool(pred_last_action_only),
                                  per_sample=True)[1]

    def _loss_forward(self, state, action, goal, noise, sigma, uncond=False, last_only=False, per_sample=False):
        inner = self.inner_model
        if not isinstance(inner, DiffusionGPT):
            raise NotImplementedError("GCDenoiser: the gradient-free loss needs a beso_amd DiffusionGPT inside (the HIP kernels)")
        if inner.training:
            raise ValueError("GCDenoiser.loss: called with autograd disabled on a module in training mode (the masked, "
                             "dropped-out loss is a training-step quantity); call eval() for the held-out loss")
        if not (torch.is_tensor(action) and action.is_cuda):
            raise ValueError("GCDenoiser.loss: the inputs are not on the GPU (beso_amd has no CPU path)")
        with torch.no_grad():
            return inner.runtime(self.sigma_data).loss(inner.packed_weights(), state, action, goal, noise, sigma,
                                                       uncond=bool(uncond), last_only=bool(last_only), per_sample=per_sample)

    # -- HIP training step ---------------------------------------------------------------------
    def hip_train_step(self, state, action, goal, noise, sigma):
        """The ``HipTrainStep`` bound to the inner model if this call can run on it, else None."""
        inner = self.inner_model
        if not isinstance(inner, DiffusionGPT) or not torch.is_grad_enabled():
            return None
        if not HipTrainStep.supported(inner):
            return None
        if not (torch.is_tensor(action) and action.is_cuda):
            return None
        key = float(self.sigma_data)
        step = self._train_steps.get(key)
        if step is None:
            step = self._train_steps[key] = HipTrainStep(inner, key)
        # (BesoAgent(deterministic_training=True) sets the attribute on its denoiser: every step of it, the one behind
        # ``loss()`` under autograd included, then runs with BESO_TRAIN_DETERMINISTIC)
        step.deterministic = bool(self.deterministic_training)
        return step if step.eligible(state, action, goal, noise, sigma) else None

    # -- input vector-Jacobian product ---------------------------------------------------------
    def denoise_vjp(self, state, action, goal, sigma, cot, uncond: bool = False, input_grads: bool = False):
        """-> (denoised, x_grad, dot): ``forward`` at ``action`` (eval mode), ``(d denoised / d action)^T cot`` and
        ``(cot * x_grad).flatten(1).sum(1)`` -- what the reference's log_likelihood gets from torch.autograd.grad
        (gc_sampling.py:480-485), as one HIP call (``beso_denoise_vjp``).  No parameter gradient is touched.
        ``input_grads``: -> (denoised, x_grad, dot, state_grad, goal_grad), the same product with respect to ``state`` and
        ``goal`` as well (``HipTrainStep.denoise_vjp``)."""
        inner = self.inner_model
        if not isinstance(inner, DiffusionGPT):
            raise NotImplementedError("GCDenoiser.denoise_vjp needs a beso_amd DiffusionGPT inside (the HIP kernels)")
        key = float(self.sigma_data)
        step = self._train_steps.get(key)
        if step is None:
            step = self._train_steps[key] = HipTrainStep(inner, key)
        return step.denoise_vjp(state, action, goal, sigma, cot, uncond=uncond, input_grads=input_grads)

    def _why_no_hip_step(self, state, action, goal, noise, sigma) -> str:
        inner = self.inner_model
        if not HipTrainStep.supported(inner):
            return f"embed_dim={inner.embed_dim} is not a multiple of 8 (the HIP training kernels need that)"
        if not (torch.is_tensor(action) and action.is_cuda):
            return "the inputs are not on the GPU (beso_amd has no CPU path)"
        if any(torch.is_tensor(x) and x.requires_grad for x in (action, noise, sigma)):
            return ("gradients with respect to action, noise and sigma are not computed (state and goal may require grad; "
                    "action / noise / sigma must not)")
        return ("parameters must be contiguous fp32 HIP tensors that require grad, and state / action / goal / noise / "
                "sigma HIP tensors (state and goal may require grad; gradients with respect to action, noise and sigma are "
                "not computed)")

    # -- fused path ----------------------------------------------------------------------------
    @staticmethod
    def _fused(inner, kwargs, *tensors) -> bool:
        if not isinstance(inner, DiffusionGPT):
            return False
        if set(kwargs) - {"uncond", "keep_last_actions"} or kwargs.get("keep_last_actions", False):
            return False
        if inner.training:
            return False            # training-mode goal masking / dropout live in DiffusionGPT.forward
        return inner._hip_eligible(*tensors)

    def can_fuse_sampler(self, state, x_t, goal) -> bool:
        """True when ``fused_sampler`` runs these inputs (and does not return None for them)."""
        return self._fused(self.inner_model, {}, state, x_t, goal) and x_t.dim() == 3 and state.dim() == 3

    def fused_sampler(self, sampler: str, state, x_t, goal, sigmas, cond_lambda: float = 1.0, eta: float = 1.0, noise=None,
                      stepwise: bool = False, s_noise: float = 1.0, order: int = 4, trace=None):
        """A whole sampler loop of ``_lib.SAMPLERS`` as one enqueue (``ScoreNetRuntime.sample``); None if not applicable.
        ``trace`` (a subset of {'x', 'denoised'}): also record the trajectory; the result is then ``(x_0, {...})``."""
        inner = self.inner_model
        if not self.can_fuse_sampler(state, x_t, goal):
            return None
        return inner.runtime(self.sigma_data).sample(inner.packed_weights(), sampler, state, x_t, goal, sigmas,
                                                     cond_lambda=cond_lambda, eta=eta, s_noise=s_noise, order=order,
                                                     noise=noise, stepwise=stepwise, trace=trace)
