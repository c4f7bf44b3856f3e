"""Training the guide of classifier-guided sampling: ``GuideTrainer`` fits an ``MLPGuide`` (guides.py) to targets given on
NOISED actions, so that the guide ``ClassifierGuidedSampleModel`` evaluates at the sampler's noisy ``a``, for every sigma of the
schedule, was trained there.  The reference ships the guided wrapper (classifier_free_sampler.py:56-90) and neither a guide nor a
way to make one.

One ``train_step`` is five enqueues and no torch-op evaluation of the network (include/beso_guide_fit.h, include/beso_mlp.h):

  1. ``beso_guide_fit_rows``   rows ``[state | action + sigma * noise | goal | log(sigma) / 4]`` -- no ``torch.cat``
  2. ``beso_mlp_fwd``          q, with the keep buffer
  3. ``beso_guide_fit_loss``   the weighted mean loss, each row's loss, and dq = dL/dq
  4. ``beso_mlp_bwd``          the parameter gradients, into the flat buffer the parameters' ``.grad`` are views of
  5. ``FusedAdam.step``

Nothing reads the device: the loss comes back as a 0-dim device tensor.  Equal inputs, seed and state give equal bits."""
import torch

from .... import _lib
from .fit_common import FitNet, check_bt, f32c, goal_args, ptr, require_gpu
from .guides import MLPGuide, _stream


class GuideTrainer:
    """``GuideTrainer(guide, lr, betas, weight_decay, loss='mse' | 'bce', sample_density=None, seed=None)``.

    ``guide``: an ``MLPGuide`` on the GPU; the trainer owns its optimizer (``FusedAdam``: Adam, or AdamW's decay with
    ``decoupled_weight_decay=True``), never the denoiser's.  ``loss``: ``'mse'`` for a value or reward regression, ``'bce'``
    for a goal-reaching classifier whose q is a logit and whose targets lie in [0, 1].  ``sample_density``: a callable
    ``(shape, device=...) -> sigma`` such as ``BesoAgent.make_sample_density()``; it draws from torch's global generator.
    ``seed`` seeds the trainer's own generator, which draws the noise.

    The guide is an ordinary module before and after: ``guide.eval()`` and handing it to ``ClassifierGuidedSampleModel`` freeze
    it exactly as a guide built elsewhere."""

    def __init__(self, guide, lr: float = 1e-3, betas=(0.9, 0.999), weight_decay: float = 0.0, loss: str = "mse",
                 sample_density=None, seed=None, decoupled_weight_decay: bool = False):
        if not isinstance(guide, MLPGuide):
            raise TypeError(f"GuideTrainer: guide must be an MLPGuide, got {type(guide).__name__}")
        if loss not in _lib.GUIDEFIT_LOSSES:
            raise ValueError(f"GuideTrainer: loss {loss!r} has no HIP kernel (supported: {', '.join(sorted(_lib.GUIDEFIT_LOSSES))})")
        self.guide, self.loss, self.sample_density = guide, loss, sample_density
        self._net = FitNet(guide.network, dict(lr=lr, betas=betas, weight_decay=weight_decay,
                                                 decoupled_weight_decay=decoupled_weight_decay))
        self.params, self.optimizer = self._net.params, self._net.optimizer
        self.generator = torch.Generator(device=self.params[0].device)
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.per_row = None             # [B, T]: each row's loss of the last step (device)

    # ------------------------------------------------------------------ the step
    def train_step(self, state, action, goal, target, weight=None, sigma=None, noise=None) -> torch.Tensor:
        """One fit step on ``state [B, >= T, obs]``, ``action [B, T, act]``, ``goal [B or 1, G, obs]`` or None, ``target [B, T]``
        and an optional ``weight [B, T]`` (the loss is the weighted mean; all-zero weights give loss 0 and no gradient).
        ``sigma [B]``: None draws it from ``sample_density``; without one (and without ``use_sigma``) the rows hold the clean
        action.  ``noise [B, T, act]``: None draws ``randn`` from the trainer's generator.  -> the loss before the update, a
        0-dim device tensor; ``per_row`` holds each row's loss."""
        guide = self.guide
        B, T, obs, act, goal = guide._dims(state, action, goal)
        check_bt("GuideTrainer", B, T, (("target", target), ("weight", weight)))
        if target is None:
            raise ValueError(f"GuideTrainer: target must be [B={B}, T={T}], got None")
        dev = action.device
        require_gpu("GuideTrainer", "the guide", (state, action, target, *self.params))
        if sigma is None and self.sample_density is not None:
            sigma = self.sample_density((B,), device=dev)
        if sigma is None and guide.use_sigma:
            raise ValueError("GuideTrainer: a guide with use_sigma needs sigma [B] or a sample_density to draw it from")
        if sigma is not None and (not torch.is_tensor(sigma) or sigma.shape != (B,)):
            raise ValueError(f"GuideTrainer: sigma must be a tensor [B={B}]")
        if sigma is None and noise is not None:
            raise ValueError("GuideTrainer: noise without sigma (no sample_density to draw it from)")
        if sigma is not None and noise is None:
            noise = torch.randn(B, T, act, generator=self.generator, device=dev, dtype=torch.float32)
        if noise is not None and noise.shape != (B, T, act):
            raise ValueError(f"GuideTrainer: noise must be [B={B}, T={T}, act={act}], got {tuple(noise.shape)}")
        state, action, goal, target, weight, sigma, noise = (f32c(t, dev) for t in (state, action, goal, target, weight, sigma, noise))
        c_noise = guide.c_noise(sigma, B, "GuideTrainer") if guide.use_sigma else None         # torch's log, as MLPGuide.apply's
        goal_steps, goal_rows = goal_args(goal)

        M = B * T
        fit = self._net
        b = fit.buffers(M, dev)
        rows, q, _, dq, _ = b
        flat = fit.grads(dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        self.per_row = torch.empty(B, T, dtype=torch.float32, device=dev)
        lib = _lib.load_guidefit()
        with torch.cuda.device(dev):
            stream = _stream(action)
            _lib.check(lib.beso_guide_fit_rows(
                state.data_ptr(), action.data_ptr(), ptr(goal), ptr(sigma), ptr(noise), ptr(c_noise), B, T, state.shape[1],
                goal_steps, goal_rows, obs, act, rows.data_ptr(), stream),
                "beso_guide_fit_rows")
            fit.forward(b)
            _lib.check(lib.beso_guide_fit_loss(q.data_ptr(), target.data_ptr(), ptr(weight), M, _lib.GUIDEFIT_LOSSES[self.loss],
                                               loss.data_ptr(), self.per_row.data_ptr(), dq.data_ptr(), stream),
                       "beso_guide_fit_loss")
            fit.backward(b, flat)
            self.optimizer.step()
        return loss

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        """The network, the optimizer's moments and step count (``FusedAdam.export_state``) and the noise generator, as CPU
        tensors: loaded into a trainer around an equally shaped guide, the next step's bits are those of the uninterrupted run."""
        network, optimizer = self._net.export()
        return dict(version=1, loss=self.loss, network=network, optimizer=optimizer, generator=self.generator.get_state().clone())

    def load_state_dict(self, d: dict) -> None:
        if d.get("loss") != self.loss:
            raise ValueError(f"GuideTrainer.load_state_dict: saved with loss {d.get('loss')!r}, this trainer has {self.loss!r}")
        self._net.load(d["network"], d["optimizer"])
        self.generator.set_state(d["generator"])
