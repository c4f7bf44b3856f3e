"""Drop-in for ``beso...k_diffusion.classifier_free_sampler``: the two SAMPLING-time guidance wrappers.

``ClassifierFreeSampleModel`` (reference: classifier_free_sampler.py:12-52): classifier-free guidance,
``out_uncond + lambda * (out_cond - out_uncond)``.  Around a ``beso_amd`` GCDenoiser the conditional and unconditional passes
run as one 2B-sample launch sequence inside the HIP library (the second half of the batch embeds zero goals).

``ClassifierGuidedSampleModel`` (reference: classifier_free_sampler.py:56-90): guidance by a learned value, reward or
goal-reaching function, ``denoised + lambda * sigma^2 * d guide(state, a, goal) / da``.  With an ``MLPGuide`` (guides.py) on the
GPU the whole line behind the denoiser is ONE launch (``beso_guide_apply``, include/beso_guide.h)."""
from copy import deepcopy

import torch
import torch.nn as nn

from .guides import MLPGuide
from .score_wrappers import GCDenoiser
from .utils import append_dims


class ClassifierFreeSampleModel(nn.Module):
    def __init__(self, model, cond_lambda: float = 2):
        super().__init__()
        self.model = model
        self.cond_lambda = cond_lambda
        self.cond = bool(cond_lambda == 1)       # lambda == 1: purely conditional (:30-33)

    def forward(self, state, action, goal, sigma, **extra_args):
        if self.cond:
            return self.model(state, action, goal, sigma)
        if self.cond_lambda == 0:
            return self.model(state, action, goal, sigma, uncond=True)
        m = self.model
        if isinstance(m, GCDenoiser) and not extra_args and m._fused(m.inner_model, {}, state, action, goal, sigma):
            inner = m.inner_model
            return inner.runtime(m.sigma_data).denoise(inner.packed_weights(), state, action, goal, sigma,
                                                       cond_lambda=float(self.cond_lambda), precondition=True)
        action = deepcopy(action)
        out = m(state, action, goal, sigma, **extra_args)        # extra args reach the conditional call only (:45-47)
        out_uncond = m(state, action, goal, sigma, uncond=True)
        return out_uncond + self.cond_lambda * (out - out_uncond)

    def get_params(self):
        return self.model.get_params()


class ClassifierGuidedSampleModel(nn.Module):
    """``forward = pred + cond_lambda * grad * sigma^2`` with ``pred = model(state, action, goal, sigma, **extra_args)`` and
    ``grad`` the gradient of ``guide(state, a, goal).sum()`` with respect to ``a``, taken at ``a = pred``.  Same kwargs and
    attributes (``model``, ``guide``, ``cond_lambda``) as the reference; ``model`` is a GCDenoiser or a ClassifierFreeSampleModel
    around one (or anything callable the same way): the wrapper only calls it, under the caller's ``no_grad``, on its HIP path.

    Deviation from the reference's text: its ``forward`` (classifier_free_sampler.py:78-87) clones ``pred_action`` into ``a``
    (:83), then calls the guide on ``pred_action`` (:84) and differentiates with respect to ``a`` (:85), which is not part of
    that graph -- ``autograd.grad`` raises "One of the differentiated Tensors appears to not have been used in the graph", so the
    class cannot run as written.  Built here is the evident intent: the guide evaluated on ``a``.  ``outputs`` is the guide's
    sum (the reference hands ``q_value`` itself to ``autograd.grad``, which takes a scalar only), and no second-order graph
    is kept (``create_graph=True`` at :85 is detached on the same line).

    Two paths, decided once per guide and row layout (``MLPGuide.fused_supported``), never by catching an error per call:
      * ``cond_func`` an ``MLPGuide`` the library serves, on GPU tensors: ``beso_guide_apply`` -- one launch behind the denoiser
        (an ``MLPGuide(use_sigma=True)``, a classifier of the noised action trained by ``guide_fit.GuideTrainer``, is handed
        ``sigma`` on either path; its launch is ``beso_guide_apply_sigma``);
      * any other callable (a torch-op function, a ``ResidualMLPNetwork`` behind a lambda, an ``MLPGuide`` beyond the launch's
        shapes): ``torch.enable_grad()`` and ``autograd.grad`` over the guide alone.  This is also what runs on CPU tensors.

    The guide is frozen at sampling time: it is kept OUT of the module tree, so a guide that is an ``nn.Module`` changes neither
    ``get_params()`` / ``parameters()`` (the agent's optimizer and EMA shadow) nor ``state_dict()`` (its checkpoints) -- and is
    not moved by ``.to()``: build it on its device.  ``loss`` and ``hip_train_step`` hand through to the wrapped denoiser, so an
    agent built around the wrapper trains exactly what it would train without it."""

    def __init__(self, model, cond_func, cond_lambda: float = 2):
        super().__init__()
        self.model = model
        self.__dict__["guide"] = cond_func                  # not self.guide = ...: nn.Module would register a Module's parameters
        self.cond_lambda = cond_lambda

    def _fused_guide(self, state, pred, goal):
        g = self.guide
        if not isinstance(g, MLPGuide) or not (torch.is_tensor(pred) and pred.is_cuda and pred.dim() == 3 and state.dim() == 3):
            return False
        return g.fused_supported(state.shape[2], pred.shape[2], g.use_goal and goal is not None)

    def forward(self, state, action, goal, sigma, cond_lambda=None, **extra_args):
        if cond_lambda is None:
            cond_lambda = self.cond_lambda
        pred = self.model(state, action, goal, sigma, **extra_args)
        if self._fused_guide(state, pred, goal):
            return self.guide.apply(state, pred, goal, sigma, float(cond_lambda))
        with torch.enable_grad():
            a = pred.detach().clone().requires_grad_(True)
            # a noise-aware MLPGuide reads the noise level; every other guide keeps the reference's three arguments
            takes_sigma = isinstance(self.guide, MLPGuide) and self.guide.use_sigma
            q_value = self.guide(state, a, goal, sigma) if takes_sigma else self.guide(state, a, goal)
            grads = torch.autograd.grad(outputs=q_value.sum(), inputs=a, only_inputs=True)[0].detach()
        return pred + cond_lambda * grads * append_dims(sigma ** 2, action.ndim)

    def get_params(self):
        return self.model.get_params()

    # ------------------------------------------------------------------ training hands through
    def _denoiser(self):
        m = self.model
        return m.model if isinstance(m, ClassifierFreeSampleModel) else m

    def loss(self, *args, **kwargs):
        return self._denoiser().loss(*args, **kwargs)

    def hip_train_step(self, *args, **kwargs):
        den = self._denoiser()
        return den.hip_train_step(*args, **kwargs) if hasattr(den, "hip_train_step") else None
