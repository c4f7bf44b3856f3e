"""Drop-in for ``beso.agents.diffusion_agents.beso_agent.BesoAgent`` (reference: beso_agent.py:28-598).

Same constructor kwargs (Hydra ``_target_`` swap), same public methods and externally mutated
attributes (``model``, ``sigma_min/max``, ``use_kde`` ...).  What changes underneath:

  * ``predict`` / ``evaluate`` evaluate the EMA weights through a packed kernel image of the EMA
    shadow that is refreshed only after ``ema_helper.update`` -- the reference clones all parameters,
    copies the shadow in and copies the originals back on EVERY call (beso_agent.py:343-345,380-381);
  * ``sample_loop`` hands ddim / euler / heun to the HIP library as one enqueue of all steps;
  * ``train_step`` all-reduces the score-matching gradients over the data-parallel ranks (RCCL over
    xGMI) before the optimizer step when a process group is initialised;
  * two optional constructor arguments the reference does not have, ``max_grad_norm`` and ``skip_nonfinite_steps``
    (after ``patience``, both off by default): global gradient-norm clipping and a guard that drops a step whose
    gradient is not finite, both inside the fused optimizer launch (``FusedAdam.step``);
  * a trainable ``input_encoder`` (``MLPEncoder``: an ``MLPNetwork`` on HIP kernels, forward and backward) is trained by the
    same step from the loss's gradient with respect to ``state`` and ``goal``; the agent SCALES FIRST AND ENCODES SECOND (the
    scaler's statistics are those of the raw observations, the denoiser's ``obs_dim`` is the encoder's ``output_dim``) -- a
    deliberate choice: the reference has no trainable encoder that would define the order.  With ``NoEncoder`` nothing changes;
  * ``deterministic_training`` (off by default): every HIP training step runs with ``BESO_TRAIN_DETERMINISTIC`` -- the loss
    and all gradients are summed in a fixed order, so a re-run gives the same bits -- and ``store_training_state`` /
    ``load_training_state`` save and restore everything a step reads, so that a resumed run continues bit for bit.
"""
import contextlib
import logging
import math
import os
from collections import deque
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from ... import distributed as bdist
from ..._instantiate import instantiate
from ...networks.ema_helper.ema import ExponentialMovingAverage
from ...optim import FusedAdam, maybe_fuse
from ...data.prefetch import DevicePrefetcher
from ..base_agent import BaseAgent
from .k_diffusion import gc_sampling as ks
from .k_diffusion import utils
from .k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel, ClassifierGuidedSampleModel
from .k_diffusion.score_gpts import DiffusionGPT
from .k_diffusion.score_wrappers import GCDenoiser

log = logging.getLogger(__name__)

try:                      # logging only; absent on the GPU box
    import wandb
except ImportError:       # pragma: no cover
    wandb = None


def _wandb_log(payload):
    if wandb is not None and getattr(wandb, "run", None) is not None:
        wandb.log(payload)


class BesoAgent(BaseAgent):
    def __init__(self, model, input_encoder, optimization, device: str, obs_modalities: list,
                 goal_modalities: list, target_modality: str, max_train_steps: int, max_epochs: int,
                 train_method: str, eval_every_n_steps: int, use_ema: bool, goal_conditioned: bool,
                 pred_last_action_only: bool, rho: float, num_sampling_steps: int, lr_scheduler,
                 sampler_type: str, sigma_data: float, sigma_min: float, sigma_max: float,
                 sigma_sample_density_type: str, sigma_sample_density_mean: float,
                 sigma_sample_density_std: float, decay: float, update_ema_every_n_steps: int,
                 window_size: int, goal_window_size: int, use_kde: bool = False, patience: int = 10,
                 max_grad_norm: float | None = None, skip_nonfinite_steps: bool = False,
                 deterministic_training: bool = False):
        super().__init__(model, input_encoder, optimization, obs_modalities, goal_modalities, target_modality,
                         device, max_train_steps, eval_every_n_steps, max_epochs)
        self.ema_helper = ExponentialMovingAverage(self.model.get_params(), decay, self.device)
        self.use_ema = use_ema
        # torch Adam / AdamW on a HIP device -> the one-launch fused step (same hyper-parameters, same
        # param_groups surface for the LR scheduler); any other optimizer class is left as configured
        self.optimizer = maybe_fuse(self.optimizer)
        # gradient clipping / the non-finite guard: inside the fused launch, from a norm the host never reads.  The eager
        # optimizers clip through torch.nn.utils.clip_grad_norm_; the guard would need a host read per step there -- the
        # read it exists to avoid -- and is refused
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (or None)")
        if skip_nonfinite_steps and not isinstance(self.optimizer, FusedAdam):
            raise ValueError("skip_nonfinite_steps needs the fused optimizer (torch Adam / AdamW over fp32 parameters on "
                             "the GPU): the guard lives in its launch")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite_steps = bool(skip_nonfinite_steps)
        self._eager_grad_norm = None
        # fixed-order reductions in the HIP training step (BESO_TRAIN_DETERMINISTIC).  The flag lives on the denoiser, which
        # hands it to every HipTrainStep it gives out: the eager step and the one behind `model.loss()` in the captured graph
        self.deterministic_training = bool(deterministic_training)
        self.lr_scheduler = instantiate(lr_scheduler, optimizer=self.optimizer)
        # a trainable input encoder gets its own optimizer instance from the same config (with FusedAdam: its own one-group
        # instance, so fused EMA and clipping keep their one-group precondition -- the gradient norm of max_grad_norm is then
        # PER OPTIMIZER: the denoiser and the encoder are clipped separately), its own EMA with the agent's decay and update
        # period, and the same LR schedule
        self.encoder_optimizer = self.encoder_ema = self.encoder_lr_scheduler = None
        self._enc_flat = None
        if self._trainable_encoder() is not None:
            enc = self.input_encoder
            enc.to(device)
            self.encoder_optimizer = maybe_fuse(instantiate(optimization, params=enc.get_params()))
            self.encoder_ema = ExponentialMovingAverage(enc.get_params(), decay, self.device)
            self.encoder_lr_scheduler = instantiate(lr_scheduler, optimizer=self.encoder_optimizer)
        self.gc = goal_conditioned
        self.train_method = train_method
        self.epochs = max_epochs
        self.sampler_type = sampler_type
        self.num_sampling_steps = num_sampling_steps
        self.sigma_data = sigma_data
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self.rho = rho
        self.sigma_sample_density_type = sigma_sample_density_type
        self.sigma_sample_density_mean = sigma_sample_density_mean
        self.sigma_sample_density_std = sigma_sample_density_std
        self.decay = decay
        self.update_ema_every_n_steps = update_ema_every_n_steps
        self.patience = patience
        self.window_size = window_size
        self.goal_window_size = goal_window_size
        self.pred_last_action_only = pred_last_action_only
        # rolling contexts of the rollout (beso_agent.py:96-100)
        self.obs_context = deque(maxlen=self.window_size)
        self.goal_context = deque(maxlen=self.goal_window_size)
        self.action_context = deque(maxlen=self.window_size - 1)
        self.que_actions = True
        self.use_kde = use_kde
        self.noise_scheduler = 'exponential'
        # MI355X runtime state
        self._ema_packed = None
        self._ema_packed_key = None
        self._grad_bucket = None
        self._sharded_ex = None          # buffers of the sharded gradient exchange (BESO_AMD_C1=sharded)
        self._ema_partial = False        # sharded exchange: the EMA shadow is current for the owned range only
        self._train_graphs = {}          # batch shape -> captured forward+backward (train_step)
        self._train_graph_ok = True
        self._enc_graph_logged = False   # "BESO_AMD_TRAIN_GRAPH=1 ignored" is logged once
        self._replicas_synced = False    # data parallel: rank 0's weights were broadcast (C2)
        self._loss_stream = self._c1_stream = None           # the step's side streams, created on first use (_side_stream)
        # _hip_loss_backward leaves these: the HipTrainStep that ran (None: autograd), the early C1 stream, the early loss stream
        self._hip_step = self._c1_early = self._loss_ready = None

    # ------------------------------------------------------------------ reproducibility
    @property
    def deterministic_training(self) -> bool:
        """Whether the HIP training step runs with BESO_TRAIN_DETERMINISTIC: the denoiser's flag (one place, read by every step)."""
        den = self._hip_denoiser()
        return bool(den is not None and getattr(den, "deterministic_training", False))

    @deterministic_training.setter
    def deterministic_training(self, on: bool):
        den = self._hip_denoiser()
        if den is None:
            if on:
                raise ValueError("deterministic_training needs the beso_amd GCDenoiser / DiffusionGPT (the HIP training step)")
            return
        den.deterministic_training = bool(on)

    # ------------------------------------------------------------------ trainable input encoder
    def _trainable_encoder(self):
        """``self.input_encoder`` if it has parameters (``MLPEncoder``), else None: every code path of a ``NoEncoder`` agent is
        the one without an encoder."""
        enc = self.input_encoder
        if isinstance(enc, nn.Module) and hasattr(enc, "encode") and next(iter(enc.parameters()), None) is not None:
            return enc
        return None

    def _refuse_with_encoder(self, what: str):
        if self._trainable_encoder() is not None:
            raise NotImplementedError(f"{what} with a trainable input encoder ({type(self.input_encoder).__name__}) is not "
                                      "supported")

    def _encode_eval(self, state, goal):
        """Inference: (state, goal) through the trainable encoder under no_grad -- on its EMA weights with ``use_ema`` -- or
        unchanged without one."""
        enc = self._trainable_encoder()
        if enc is None:
            return state, goal
        params = tuple(self.encoder_ema.shadow_params) if self.use_ema else None
        run = partial(self._encode_rows, enc.network, keep=False, params=params)
        with torch.no_grad():
            return run(state)[0], (run(goal)[0] if goal is not None and enc.encode_goal else goal)

    @staticmethod
    def _encode_rows(net, x, *, keep, params=None):
        """``x`` [..., input_dim] through ``net`` (on ``params``: the EMA shadow) -> (y [..., output_dim], the kept rows or None)."""
        net._check_input(x)
        rows = x.reshape(-1, net.input_dim).to(torch.float32).contiguous()
        y, kept = net.run_forward(rows, keep=keep, params=params)
        return y.view(*x.shape[:-1], net.output_dim), kept

    def _encoder_grad_buffer(self, net):
        """The flat gradient buffer of the encoder; its views are the parameters' ``.grad`` (as for the denoiser)."""
        params = list(net.get_params())
        if self._enc_flat is None or self._enc_flat.device != params[0].device:
            self._enc_flat = torch.empty(net.num_param_floats(), dtype=torch.float32, device=params[0].device)
            off = 0
            for p in params:
                p.grad = self._enc_flat[off:off + p.numel()].view_as(p)
                off += p.numel()
        return self._enc_flat

    def _encoded_loss_backward(self, enc, state, action, goal):
        """``_loss_backward`` behind the encoder: encode keeping what the backward needs, the HIP step with
        ``input_grads=True``, then ``beso_mlp_bwd`` on (state_grad, goal_grad) -- enqueued on the compute stream behind the
        step's last launch; the early-released loss stream is not touched."""
        if bdist.is_distributed() and bdist.world_size() > 1:
            raise NotImplementedError("data-parallel training (world_size > 1) with a trainable input encoder "
                                      f"({type(enc).__name__}) is not supported: its gradients are not exchanged")
        if os.environ.get("BESO_AMD_TRAIN_GRAPH", "0") == "1" and not self._enc_graph_logged:
            self._enc_graph_logged = True
            log.info("BESO_AMD_TRAIN_GRAPH=1 ignored: the agent has a trainable input encoder")
        net = enc.network
        state_e, state_keep = self._encode_rows(net, state, keep=True)
        goal_e, goal_keep = self._encode_rows(net, goal, keep=True) if goal is not None and enc.encode_goal else (goal, None)
        loss, state_grad, goal_grad = self._hip_loss_backward(state_e, action, goal_e, input_grads=True, exchange=False)   # (world 1)
        flat = self._encoder_grad_buffer(net)
        net.run_backward(state_keep, state_grad, flat)
        if goal_keep is not None and goal_grad is not None:
            if goal_grad.numel() != goal_e.numel():
                goal_grad = goal_grad.sum(dim=0, keepdim=True)      # one goal for the whole batch: its gradient is the sum
            net.run_backward(goal_keep, goal_grad, flat, accumulate=True)
        return loss

    # ------------------------------------------------------------------ scaler / bounds
    def get_scaler(self, scaler):
        self.scaler = scaler

    def set_bounds(self, scaler):
        self.model.min_action = torch.from_numpy(scaler.y_bounds[0, :]).to(self.device)
        self.model.max_action = torch.from_numpy(scaler.y_bounds[1, :]).to(self.device)

    # ------------------------------------------------------------------ EMA evaluation scope
    def _hip_denoiser(self):
        """The beso_amd GCDenoiser behind ``self.model`` (which scripts may wrap in
        ClassifierFreeSampleModel: scripts/training.py:54-55, in ClassifierGuidedSampleModel, or in the latter around the
        former), or None."""
        m = self.model
        if isinstance(m, ClassifierGuidedSampleModel):
            m = m.model
        if isinstance(m, ClassifierFreeSampleModel):
            m = m.model
        if isinstance(m, GCDenoiser) and isinstance(m.inner_model, DiffusionGPT):
            return m
        return None

    @contextlib.contextmanager
    def _ema_scope(self):
        """Evaluate with the EMA weights.  HIP model on the GPU: swap in the packed image of the
        shadow.  Anything else: the reference's store / copy_to / restore (beso_agent.py:343-381)."""
        # (sharded C1: a collective when the shadow is partial -- reached by every rank at the same step, with or without
        # use_ema, so that no rank enters it alone)
        self._complete_ema()
        if not self.use_ema:
            yield
            return
        den = self._hip_denoiser()
        first = next(iter(self.model.parameters()), None)        # (listing all 113 parameters costs 0.3 ms per call)
        if den is not None and first is not None and first.is_cuda:
            inner = den.inner_model
            key = (self.ema_helper.version, inner.precision, id(self.ema_helper))
            if self._ema_packed is None or self._ema_packed_key != key:
                self._ema_packed = inner.pack_external(self.ema_helper.shadow_params, into=self._ema_packed)
                self._ema_packed_key = key
            with inner.use_weights(self._ema_packed):
                yield
            return
        self.ema_helper.store(self.model.parameters())
        self.ema_helper.copy_to(self.model.parameters())
        if den is not None:
            den.inner_model.mark_weights_dirty()
        try:
            yield
        finally:
            self.ema_helper.restore(self.model.parameters())
            if den is not None:
                den.inner_model.mark_weights_dirty()

    # ------------------------------------------------------------------ training
    def _sync_replicas(self):
        """Data parallel: every replica starts from rank 0's weights (C2, one flat broadcast), and the EMA shadow is
        re-seeded from them (a shadow built from the pre-broadcast init would make the ranks' EMA weights differ)."""
        if bdist.is_distributed() and not self._replicas_synced:
            bdist.broadcast_parameters(self.model.get_params(), src=0)
            den = self._hip_denoiser()
            if den is not None:
                den.inner_model.mark_weights_dirty()
            self.ema_helper.load_shadow_params(self.model.get_params())
            self._ema_packed_key = None
            # every rank must draw its OWN noise, sigma, dropout and goal masks: scripts seed all ranks with
            # the same cfg.seed (scripts/training.py:27), so the per-process generators are moved apart by the rank
            seed = (torch.initial_seed() + 7919 * (bdist.rank() + 1)) % (2 ** 63 - 1)
            torch.manual_seed(seed)
            self._replicas_synced = True

    def _c1_mode(self) -> str:
        """How the data-parallel gradient exchange (C1) runs: 'overlap' (default: all-reduce in three ranges, the first
        under the backward of the lower layers), 'flat' (one all-reduce after the backward), 'sharded' (reduce-scatter,
        Adam(W) + EMA on the owned 1/world of the parameters, all-gather of the updated parameters: SURVEY.md 2.2)."""
        mode = os.environ.get("BESO_AMD_C1", "overlap")
        if os.environ.get("BESO_AMD_C1_OVERLAP", "1") == "0" and mode == "overlap":
            mode = "flat"
        if mode not in ("overlap", "flat", "sharded"):
            raise ValueError(f"BESO_AMD_C1={mode!r}: choose overlap, flat or sharded")
        return mode

    def _sharded(self):
        if self._sharded_ex is None:
            self._sharded_ex = bdist.ShardedExchange(self.model.get_params())
        return self._sharded_ex

    def _complete_ema(self):
        """Sharded C1 updates the EMA shadow of the owned parameter range only; before the shadow is read (evaluation,
        checkpoint) the ranges are gathered -- a collective: every rank gets here at the same step."""
        if self._ema_partial and bdist.is_distributed():
            self._sharded().all_gather_flat_state(self.ema_helper._flat)
            self.ema_helper.version += 1
        self._ema_partial = False

    def train_agent(self, train_loader, test_loader):
        self._sync_replicas()
        if self.train_method == 'epochs':
            self.train_agent_on_epochs(train_loader, test_loader, self.epochs)
        elif self.train_method == 'steps':
            self.train_agent_on_steps(train_loader, test_loader)
        else:
            raise ValueError('Either epochs or n_steps must be specified!')

    def train_agent_on_epochs(self, train_loader, test_loader, epochs):
        """Epoch mode with the reference loop's cadence (beso_agent.py:129-175): the logged / early-stopping test MSE is the
        LAST test batch's (the reference re-creates its list inside the loop, :138-142), the step counter advances once
        more per batch on top of train_step's own increment (:152) -- which shifts the EMA cadence
        `steps % update_ema_every_n_steps` -- and the LR scheduler gets an extra step whenever that counter hits a
        multiple of eval_every_n_steps (:153-154)."""
        best_test_mse, mean_mse, avg_test_mse = 1e10, 1e10, 1e10
        for epoch in range(epochs):
            # (the all-gather that completes a sharded EMA shadow is issued HERE, on every rank: a rank whose test loader
            # is empty never reaches evaluate() and would meet the others' all-gather with job_mean's all-reduce)
            self._complete_ema()
            test_mse = [self.evaluate(batch) for batch in test_loader]
            # data parallel: the ranks draw different evaluation noise (and may hold different test shards), so the
            # early-stopping / checkpoint decision is taken on the job-wide mean -- the same on every rank; a rank deciding
            # alone would leave the others inside the next gradient exchange
            last = bdist.job_mean(test_mse[-1] if test_mse else 0.0, 1 if test_mse else 0, self.device)
            if last is not None:
                mean_mse = avg_test_mse = last
            stop, best_test_mse = self.early_stopping(best_test_mse, mean_mse, self.patience, epochs)
            if stop:
                log.info('Early stopping!')
                break
            losses = []
            for batch in train_loader:
                losses.append(self.train_step(batch))
                self.steps += 1
                if self.steps % self.eval_every_n_steps == 0:
                    self.lr_scheduler.step()
                _wandb_log({"training/loss": losses[-1], "training/test_loss": avg_test_mse})
            _wandb_log({'training/epoch_loss': float(np.mean(losses)) if losses else 0.0,
                        'training/epoch_test_loss': avg_test_mse, 'training/epoch': epoch})
            log.info("Epoch %d: mean test mse %s, mean train loss %s", epoch, avg_test_mse,
                     float(np.mean(losses)) if losses else None)
        self.store_model_weights(self.working_dir)
        log.info("Training done!")

    def train_agent_on_steps(self, train_loader, test_loader):
        """max_train_steps optimizer steps; every eval_every_n_steps: test MSE of the sampler and a
        checkpoint on improvement (beso_agent.py:177-213)."""
        best_test_mse, avg_test_mse = 1e10, 1e10
        # next batch is copied host -> device on a side stream while the current step runs
        train_loader = DevicePrefetcher(train_loader, self.device)
        stream = iter(train_loader)
        for step in range(self.max_train_steps):
            if not self.steps % self.eval_every_n_steps:
                self._complete_ema()          # on every rank, test batches or not (see train_agent_on_epochs)
                scores = [self.evaluate(batch) for batch in test_loader]
                # (job-wide mean: every rank takes the same checkpoint decision -- store_model_weights holds a collective)
                mean = bdist.job_mean(sum(scores), len(scores), self.device)
                if mean is not None:
                    avg_test_mse = mean
                log.info("Step %d: Mean test mse is %s", step, avg_test_mse)
                if avg_test_mse < best_test_mse:
                    best_test_mse = avg_test_mse
                    self.store_model_weights(self.working_dir)
                    log.info('New best test loss. Stored weights have been updated!')
            try:
                batch = next(stream)
            except StopIteration:
                stream = iter(train_loader)
                batch = next(stream)
            loss = self.train_step(batch)
            if not self.steps % 1000:
                if self.max_grad_norm is not None or self.skip_nonfinite_steps:
                    log.info("Step %d: Mean batch loss mse is %s, gradient norm %s", step, loss, float(self.last_grad_norm()))
                else:
                    log.info("Step %d: Mean batch loss mse is %s", step, loss)
            _wandb_log({"loss": loss, "test_loss": avg_test_mse})
        self.store_model_weights(self.working_dir)
        log.info("Training done!")

    # ------------------------------------------------------------------ training step internals
    def _side_stream(self, attr: str, device):
        """The step's side stream kept in ``self.<attr>``, created on first use."""
        if getattr(self, attr) is None:
            setattr(self, attr, torch.cuda.Stream(device))
        return getattr(self, attr)

    def _loss_backward(self, state, action, goal):
        """noise ~ N(0, I), sigma ~ the configured density, score-matching loss, backward (beso_agent.py:226-235)."""
        return self._hip_loss_backward(state, action, goal, input_grads=False, exchange=True)

    def _hip_loss_backward(self, state, action, goal, *, input_grads: bool, exchange: bool):
        """The one HIP forward + backward call (beso_loss_grad) -> what ``step.loss_backward`` returns: the loss, with
        ``input_grads`` (the encoder's caller) also (state_grad, goal_grad); the gradients land in views of one flat buffer.
        ``exchange``: they go to the data-parallel exchange next -- pre-divided by the world size, padded for the sharded mode,
        the early C1 stream opened in overlap mode.  The only place that sets ``_hip_step``, ``_c1_early`` and ``_loss_ready``
        (a graph replay clears the two streams).  Without a HIP step the plain caller gets ``model.loss`` + autograd."""
        noise = torch.randn_like(action)                           # (the draws keep this order, in front of zero_grad)
        sigma = self.make_sample_density()(shape=(len(action),), device=self.device)
        step = self.model.hip_train_step(state, action, goal, noise, sigma) if hasattr(self.model, "hip_train_step") else None
        if step is None and input_grads:
            raise NotImplementedError("a trainable input encoder needs the HIP training step (the beso_amd GCDenoiser / "
                                      "DiffusionGPT on the GPU)")
        self._hip_step, self._c1_early, self._loss_ready = step, None, None
        if step is None:
            loss = self.model.loss(state, action, goal, noise, sigma)
            self.optimizer.zero_grad()
            loss.backward()
            return loss
        self.optimizer.zero_grad(set_to_none=True)
        # side streams: on the GPU, outside a graph capture (the encoder's caller is not asked: it has its HIP step and no graph)
        streams = input_grads or (state.is_cuda and not torch.cuda.is_current_stream_capturing())
        if exchange and bdist.is_distributed() and self._c1_mode() == "sharded":
            step.pad_to = self._sharded().padded
        # under data parallelism the all-reduce of the upper layers' gradients starts under the backward of the lower ones: the
        # call orders self._c1_stream behind the completion of that range (BESO_AMD_C1_OVERLAP=0: one flat all-reduce afterwards)
        if exchange and streams and bdist.is_distributed() and self._c1_mode() == "overlap":
            self._c1_early = self._side_stream("_c1_stream", state.device)
        # the loss value is final a third of the way into the step: a side stream is released at that point, and train_step reads
        # the loss there -- its `loss.item()` (beso_agent.py:248) then returns while the backward pass and the optimizer are still
        # running, and the host prepares the next step under them (BESO_AMD_ASYNC_LOSS=0: the read waits for the whole step)
        if streams and os.environ.get("BESO_AMD_ASYNC_LOSS", "1") != "0":
            self._loss_ready = self._side_stream("_loss_stream", state.device)
        # (goal masking for classifier-free guidance, mask_cond, is applied by the kernel from cond_mask_prob)
        return step.loss_backward(state, action, goal, noise, sigma, grad_scale=1.0 / bdist.world_size() if exchange else 1.0,
                                  early_stream=self._c1_early, loss_stream=self._loss_ready, input_grads=input_grads)

    def _use_train_graph(self, state) -> bool:
        # opt-in: measured 16.6 vs 17.4 ms per 1024-sample step -- the eager step is bound by its fp32 kernels,
        # not by launches
        if not (state.is_cuda and self._train_graph_ok and os.environ.get("BESO_AMD_TRAIN_GRAPH", "0") == "1"):
            return False
        # the dropout / goal-mask seed of the HIP step is a host scalar: a captured graph would replay one mask forever, so
        # models with any dropout or cond_mask_prob > 0 are not captured at all (no warm-up steps spent on a doomed capture)
        den = self._hip_denoiser()
        if den is not None:
            inner = den.inner_model
            if any(float(p) > 0.0 for p in getattr(inner, "_pdrops", ())) or float(getattr(inner, "cond_mask_prob", 0.0) or 0.0) > 0.0:
                self._train_graph_ok = False
                log.info("BESO_AMD_TRAIN_GRAPH=1 ignored: the model has dropout / cond_mask_prob > 0 (host-drawn seed)")
                return False
        return True

    def _graphed_loss_backward(self, state, action, goal):
        """The same forward + backward replayed as ONE HIP graph per batch shape.  The eager training step issues several thousand
        small kernels; the graph removes the launch gaps and changes no arithmetic (opt-in, BESO_AMD_TRAIN_GRAPH=1: the measured
        gain is 5 %).  Inputs are copied into static buffers, noise / sigma / dropout masks are drawn inside the graph from torch's
        graph-safe generator, gradients land in static .grad tensors that the (fused) optimizer reads afterwards."""
        self._c1_early = self._loss_ready = None             # a replay releases no side stream (`_hip_step` stays what it was)
        key = (tuple(state.shape), tuple(action.shape), None if goal is None else tuple(goal.shape))
        g = self._train_graphs.get(key)
        if g is None:
            g = dict(state=state.clone(), action=action.clone(), goal=None if goal is None else goal.clone())

            def fwd_bwd():
                noise = torch.randn_like(g["action"])
                sigma = self.make_sample_density()(shape=(len(g["action"]),), device=self.device)
                loss = self.model.loss(g["state"], g["action"], g["goal"], noise, sigma)
                loss.backward()
                return loss

            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):                    # warm-up off the capture stream (allocator, autotuning)
                for _ in range(3):
                    self.optimizer.zero_grad(set_to_none=True)
                    fwd_bwd()
            cur.wait_stream(side)
            self.optimizer.zero_grad(set_to_none=True)       # the captured backward then WRITES (not accumulates) .grad
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):
                    g["loss"] = fwd_bwd()
            except RuntimeError as e:                        # e.g. a sigma density that copies from the host
                log.warning("training step could not be captured into a HIP graph (%s); running it eagerly", e)
                self._train_graph_ok = False
                self._train_graphs = {}
                return self._loss_backward(state, action, goal)
            g["graph"] = graph
            self._train_graphs = {key: g}                    # one shape at a time: grads belong to the latest graph
            graph.replay()                                   # capture records, it does not execute
        else:
            g["state"].copy_(state)
            g["action"].copy_(action)
            if goal is not None:
                g["goal"].copy_(goal)
            g["graph"].replay()
        return g["loss"]

    def _prepare_step(self, batch):
        """Phase 1, prepare: the batch as scaled (state, action, goal) and the model in training mode."""
        state, action, goal = self.process_batch(batch, predict=False)
        if not self.model.training:          # (.train() / .eval() set the whole tree: the root's flag tells; walking the 69 modules
            self.model.train()               #  costs 0.1 ms per step)
        self.model.training = True
        return state, action, goal

    def _forward_backward(self, state, action, goal):
        """Phase 2, forward/backward -> the loss (0-d tensor), the gradients in ``.grad``: behind the trainable encoder if there
        is one, else as a replayed graph (BESO_AMD_TRAIN_GRAPH=1), else the plain call.  Each sets what phases 3 and 5 read."""
        enc = self._trainable_encoder()
        if enc is not None:
            return self._encoded_loss_backward(enc, state, action, goal)
        if self._use_train_graph(state):
            return self._graphed_loss_backward(state, action, goal)
        return self._loss_backward(state, action, goal)

    def _exchange(self, loss):
        """Phase 3, exchange (data parallel only) -> (loss, shard).  C3 first, where the loss has its own stream: its mean over
        the global batch is exchanged there, in front of C1 (every rank issues its collectives in this order), so that it waits
        for the forward half only.  Then C1 as ``_c1_mode`` says; ``shard``: the range a reduce-scatter left this rank, or None."""
        if not bdist.is_distributed():
            return loss, None
        if self._loss_ready is not None:
            with torch.cuda.stream(self._loss_ready):
                loss = bdist.all_reduce_mean(loss.detach().clone())
        flat = self._hip_step.flat_grads() if self._hip_step is not None else None
        sharded = self._c1_mode() == "sharded"
        if flat is not None and sharded and isinstance(self.optimizer, FusedAdam):
            # reduce-scatter: this rank ends up with the summed gradient of the parameter range it owns
            ex = self._sharded()
            ex.reduce_scatter_grads(self._hip_step.flat_grads_padded())
            return loss, (ex.lo, ex.hi)
        if flat is not None and self._c1_early is not None:
            bdist.all_reduce_sum_overlapped(flat, self._hip_step.early_range(), self._c1_early)
        elif flat is not None:
            bdist.all_reduce_sum(flat)                    # C1 on the flat buffer the kernels wrote (pre-scaled)
        else:
            if self._grad_bucket is None:
                self._grad_bucket = bdist.GradientBucket(self.model.get_params())
            self._grad_bucket.sync(decomposed=sharded)   # (eager optimizer: the same exchange as its two halves)
        return loss, None

    def _update(self, shard):
        """Phase 4, update: count the step, then ``_optimizer_step`` of the denoiser -- over ``shard`` only after a reduce-scatter,
        which leaves the EMA shadow partial -- and of the trainable encoder.  ``last_grad_norm()`` is the denoiser's alone."""
        self.steps += 1
        do_ema = self.steps % self.update_ema_every_n_steps == 0
        norm = self._optimizer_step(self.optimizer, self.model.get_params, self.ema_helper, self.lr_scheduler, do_ema, shard,
                                    ema_params=self.model.parameters)
        if norm is not None:
            self._eager_grad_norm = norm
        if shard is not None:
            self._ema_partial = self._ema_partial or do_ema
        enc = self._trainable_encoder()
        if enc is not None:
            self._optimizer_step(self.encoder_optimizer, enc.get_params, self.encoder_ema, self.encoder_lr_scheduler, do_ema)

    def _optimizer_step(self, optimizer, params, ema, scheduler, do_ema, shard=None, ema_params=None):
        """Optimizer + LR scheduler + (with ``do_ema``) EMA, clipped / guarded as the agent was built -> the norm
        ``clip_grad_norm_`` measured, else None.  The eager path clips ``params()`` and updates the EMA from ``ema_params()``
        (default ``params``; the denoiser's walks ``model.parameters()``, as the reference's).  ``shard``: the denoiser's only."""
        if not isinstance(optimizer, FusedAdam):
            norm = torch.nn.utils.clip_grad_norm_(list(params()), self.max_grad_norm) if self.max_grad_norm is not None else None
            optimizer.step()
            scheduler.step()
            if do_ema:
                ema.update((ema_params or params)())
            return norm
        # Adam(W) over all tensors and the EMA of the updated parameters in ONE HIP launch -- over the owned range only in the
        # sharded exchange, followed by the all-gather of the updated parameters
        if self.max_grad_norm is None and not self.skip_nonfinite_steps:
            optimizer.step(ema=ema if do_ema else None, shard=shard)
        else:
            # (sharded exchange: each rank reduces the squared norm of its own range; the sum over the ranks is the whole
            # gradient's.  flat / overlap: every rank holds the full reduced gradient and computes the same norm)
            optimizer.step(ema=ema if do_ema else None, shard=shard, max_grad_norm=self.max_grad_norm,
                           skip_nonfinite=self.skip_nonfinite_steps, reduce_sumsq=bdist.all_reduce_sum if shard is not None else None)
        if shard is not None:
            self._sharded().all_gather_params()
        scheduler.step()

    def _read_loss(self, loss) -> float:
        """Phase 5, read the loss: on the loss stream where the step has one -- the read then returns behind the forward
        half -- else on the compute stream, behind the whole step and, data parallel, behind the late C3."""
        if self._loss_ready is not None:
            with torch.cuda.stream(self._loss_ready):
                return loss.item()
        if bdist.is_distributed():
            loss = bdist.all_reduce_mean(loss.detach().clone())      # C3: the logged loss is the global-batch mean
        return loss.item()

    def train_step(self, batch: dict):
        """One score-matching step (beso_agent.py:215-248) in five phases: noise ~ N(0, I), sigma ~ the configured density, loss =
        GCDenoiser.loss, optimizer + LR scheduler + EMA.  Under data parallelism the gradients are averaged over the ranks first.

        Completion semantics (BESO_AMD_ASYNC_LOSS=1, the default): the returned float is this step's loss, but the call
        returns when the FORWARD half is done -- the backward pass and the optimizer of this step are still queued on the
        compute stream.  Consequences: (i) a device fault in this step's backward / optimizer surfaces at the next
        synchronising call (the next step's loss read, `evaluate`, a checkpoint), not here; (ii) timing `train_step()` per
        call without `torch.cuda.synchronize()` measures the forward half, not the step; (iii) `self._loss_stream` belongs
        to the step (the library also runs the next step's weight copies on it): nothing else may be queued there.
        Everything later on the compute stream is ordered behind the update as usual; BESO_AMD_ASYNC_LOSS=0 restores the
        reference's full synchronisation per step."""
        state, action, goal = self._prepare_step(batch)
        loss = self._forward_backward(state, action, goal)
        loss, shard = self._exchange(loss)
        self._update(shard)
        return self._read_loss(loss)

    def last_grad_norm(self) -> torch.Tensor:
        """The global L2 norm of the last training step's gradient, before clipping (``max_grad_norm`` or
        ``skip_nonfinite_steps`` set): a 0-d tensor on the agent's device.  Calling this does not synchronise; reading the
        value does, and then waits for the whole step."""
        if isinstance(self.optimizer, FusedAdam):
            return self.optimizer.last_grad_norm()
        if self._eager_grad_norm is None:
            raise RuntimeError("no training step with max_grad_norm has run yet")
        return self._eager_grad_norm

    def skipped_steps(self) -> torch.Tensor:
        """How many training steps ``skip_nonfinite_steps`` has dropped so far (a 0-d device tensor; no synchronisation).
        ``steps``, the LR scheduler, Adam's bias-correction count and the EMA warm-up count advance over a dropped step as
        over any other: the host does not know it was dropped."""
        if not isinstance(self.optimizer, FusedAdam):
            raise RuntimeError("skipped_steps needs the fused optimizer")
        return self.optimizer.skipped_steps()

    @torch.no_grad()
    def evaluate(self, batch: dict):
        """MSE between sampled and ground-truth action windows; always the exponential schedule
        (beso_agent.py:250-289)."""
        state, action, goal = self.process_batch(batch, predict=True)
        state, goal = self._encode_eval(state, goal)
        with self._ema_scope():
            self.model.eval()
            self.model.training = False
            sigmas = ks.get_sigmas_exponential(self.num_sampling_steps, self.sigma_min, self.sigma_max, 'cpu')
            x = torch.randn_like(action) * self.sigma_max
            x_0 = self.sample_loop(sigmas, x, state, goal, self.sampler_type)
            if self.pred_last_action_only:
                x_0 = x_0.reshape(x_0.shape[0], 1, -1)
            mse = nn.functional.mse_loss(x_0, action, reduction="none").mean().item()
        return mse

    # ------------------------------------------------------------------ held-out denoising loss
    def _held_out_draws(self, action, n_sigma, sigma, noise, generator):
        """(sigma or None, noise) of a held-out loss call: what the caller passed, else a draw from the training density /
        N(0, I) -- from ``generator`` when given (the density functions take none: they draw from the global generator inside a
        forked RNG scope seeded from it, and the global stream is left where it was)."""
        dev = action.device
        if noise is None:
            noise = (torch.randn_like(action) if generator is None else
                     torch.randn(action.shape, generator=generator, device=generator.device, dtype=action.dtype).to(dev))
        else:
            noise = torch.as_tensor(noise, dtype=action.dtype, device=dev)
        if sigma is not None or n_sigma == 0:
            return (None if sigma is None else torch.as_tensor(sigma, dtype=torch.float32, device=dev).reshape(-1)), noise
        density = self.make_sample_density()
        if generator is None:
            return density(shape=(n_sigma,), device=self.device), noise
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=generator.device).item())
        with torch.random.fork_rng(devices=[dev] if dev.type == "cuda" else []):
            torch.manual_seed(seed)
            return density(shape=(n_sigma,), device=self.device), noise

    def _held_out_model(self):
        den = self._hip_denoiser()
        if den is None:
            raise NotImplementedError("the held-out denoising loss needs the beso_amd GCDenoiser / DiffusionGPT (the HIP kernels)")
        return den

    @torch.no_grad()
    def validation_loss(self, batch: dict, sigma=None, noise=None, generator=None) -> float:
        """The denoising (score-matching) loss on a held-out batch: ``GCDenoiser.loss`` of the eval-mode network on the EMA
        weights (with ``use_ema``), gradient-free, as ONE ``beso_loss_fwd`` call -- the model's own error, without the sampler
        error and the x_T draw that ``evaluate`` mixes in.  ``batch`` is a training-style batch (``process_batch(batch,
        predict=False)``); ``sigma`` [B] defaults to a draw from the training density (``make_sample_density``), ``noise``
        to ``randn_like(action)``, both from ``generator`` when given.  An agent built with ``pred_last_action_only`` scores the last step of
        every window only (``GCDenoiser.loss(..., pred_last_action_only=True)``), the step ``evaluate`` compares and ``predict`` keeps --
        NOT what ``train_step`` optimises: like the reference's, it calls ``model.loss`` without the keyword and scores the
        whole window; ``GCDenoiser.loss`` under ``torch.no_grad()`` gives that full-window value.
        ``steps``, the parameters, the optimizer and the EMA are left alone; the module is left in eval mode, as ``evaluate``
        leaves it (``train_step`` switches back to ``train()`` itself).  Fixed-order
        reductions: the same inputs give the same bits."""
        den = self._held_out_model()
        state, action, goal = self.process_batch(batch, predict=False)
        state, goal = self._encode_eval(state, goal)
        sigma, noise = self._held_out_draws(action, len(action), sigma, noise, generator)
        with self._ema_scope():
            if self.model.training:
                self.model.eval()
            return den.loss(state, action, goal, noise.clone(), sigma, pred_last_action_only=self.pred_last_action_only).item()

    @torch.no_grad()
    def loss_by_sigma(self, batch: dict, sigmas, noise=None, generator=None):
        """The held-out denoising loss as a function of the noise level: every one of the B windows of ``batch`` at every one
        of the K values of ``sigmas`` -> ``(curve [K], table [K, B])``, ``table[k, b]`` the loss of window b at ``sigmas[k]``
        and ``curve[k]`` its mean over the batch.  ONE ``beso_loss_fwd`` call over K * B virtual samples (state, goal and
        action repeated K times, sigma ``repeat_interleave``d).  ``noise`` is [B, t, act] (the same draw at every level: the
        curve then varies with sigma alone) or [K, B, t, act]; default N(0, I) of the first form, from ``generator`` when
        given.  EMA weights with ``use_ema``; ``pred_last_action_only``, the module's mode and the training state as in
        ``validation_loss``."""
        den = self._held_out_model()
        state, action, goal = self.process_batch(batch, predict=False)
        state, goal = self._encode_eval(state, goal)
        B = len(action)
        sigmas = torch.as_tensor(sigmas, dtype=torch.float32, device=action.device).reshape(-1)
        K = sigmas.numel()
        if K < 1:
            raise ValueError("loss_by_sigma: at least one sigma")
        if noise is not None and tuple(noise.shape) == (K,) + tuple(action.shape):
            noise = torch.as_tensor(noise, dtype=action.dtype, device=action.device).reshape((K * B,) + tuple(action.shape[1:])).clone()
        else:
            _, noise = self._held_out_draws(action, 0, None, noise, generator)
            if noise.shape != action.shape:
                raise ValueError(f"loss_by_sigma: noise must be {tuple(action.shape)} or {(K,) + tuple(action.shape)}")
            noise = noise.repeat(K, 1, 1)
        if goal is not None and goal.dim() == 2:
            goal = goal.unsqueeze(0)
        if goal is not None and goal.shape[0] == 1 and B > 1:
            goal = goal.expand(B, -1, -1)
        with self._ema_scope():
            if self.model.training:
                self.model.eval()
            rows = den.loss_per_sample(state.repeat(K, 1, 1), action.repeat(K, 1, 1), None if goal is None else goal.repeat(K, 1, 1),
                                       noise, sigmas.repeat_interleave(B), pred_last_action_only=self.pred_last_action_only)
        table = rows.view(K, B)
        return table.mean(dim=1), table

    # ------------------------------------------------------------------ rollout inference
    def reset(self):
        self.obs_context.clear()
        self.action_context.clear()

    @torch.no_grad()
    def predict(self, batch: dict, new_sampler_type=None, get_mean=None, new_sampling_steps=None,
                extra_args=None, noise_scheduler=None) -> torch.Tensor:
        """One environment step (beso_agent.py:296-388): append the observation to the window,
        draw x_T for the newest action, denoise the WHOLE action window (previous actions + fresh
        noise), keep the last action, clip, un-scale, remember it."""
        noise_scheduler = self.noise_scheduler if noise_scheduler is None else noise_scheduler
        state, goal, _ = self.process_batch(batch, predict=True)
        state, goal = self._encode_eval(state, goal)
        if state.dim() == 2 and self.window_size > 1:
            self.obs_context.append(state)
            input_state = torch.stack(tuple(self.obs_context), dim=1)
        else:
            input_state = state
        if goal.dim() == 2 and self.window_size > 1:
            goal = goal.unsqueeze(0)                                       # 'b d -> 1 b d'
        sampler_type = self.sampler_type if new_sampler_type is None else new_sampler_type
        n_steps = self.num_sampling_steps if new_sampling_steps is None else new_sampling_steps
        act_dim = self.scaler.y_bounds.shape[1]
        with self._ema_scope():
            if self.model.training:                          # (module.eval() walks ~100 submodules: 0.35 ms per call)
                self.model.eval()
            sigmas = self.get_noise_schedule(n_steps, noise_scheduler)
            n = len(input_state) * (get_mean if get_mean is not None else 1)
            if self.window_size > 1 or get_mean is None:
                x = torch.randn((n, 1, act_dim), device=self.device) * self.sigma_max
                if self.window_size > 1 and get_mean is None and len(self.action_context) > 0:
                    x = torch.cat((*self.action_context, x), dim=1)        # (= cat([cat(context), x]): one launch)
            else:
                x = torch.randn((n, act_dim), device=self.device) * self.sigma_max
            x_0 = self.sample_loop(sigmas, x, input_state, goal, sampler_type, extra_args)
            if x_0.dim() == 3 and x_0.size(1) > 1:
                x_0 = x_0[:, -1, :]
            x_0 = self.scaler.clip_action(x_0)
        model_pred = self.scaler.inverse_scale_output(x_0)
        if model_pred.dim() == 2:
            x_0 = x_0.unsqueeze(1)
        self.action_context.append(x_0)
        return model_pred

    @torch.no_grad()
    def predict_best_of(self, batch: dict, k: int, select=None, bandwidth=None, new_sampler_type=None, new_sampling_steps=None,
                        noise_scheduler=None, extra_args=None, noise=None, guide=None) -> torch.Tensor:
        """``predict`` with ``k`` action candidates per environment, reduced to ONE action each: ``select='mean'`` acts on the
        candidates' sample mean, ``'kde'`` on the candidate of the highest diagonal Gaussian kernel density among its
        siblings (``bandwidth=None``: Scott's rule); the default is 'kde' with ``use_kde``, else 'mean'.  The window
        bookkeeping on ``obs_context`` / ``action_context``, the EMA scope, the schedule, the clip and the inverse scale are
        ``predict``'s; the k draws go through one sampler call on ``len(state) * k`` rows between the two launches of
        beso_amd/candidates.py (include/beso_select.h), and the selected, clipped action is what ``action_context`` remembers.
        ``noise`` [B, k, act] is the x_T draw of the newest action (None: ``torch.randn``); with k = 1 the call returns
        ``predict``'s bits for the same draw, in ``predict``'s shape (a one-slot window gives [B, 1, act], as there).
        ``last_best_of`` holds the call's ``candidates`` [B, k, act], ``scores`` and ``index``.  ``select='value', guide=g`` acts
        on the candidate the ``MLPGuide`` g scores highest, q of ``[newest observation | candidate | goal]`` as the sampler sees
        them, in ONE launch behind the sampler (include/beso_rank.h); ``scores`` are then the q values, and a bad guide is refused
        before a context changes.  ``predict(get_mean=...)`` is the reference's call and stays what it is: it draws the extra rows
        and reduces nothing.  Needs the GPU."""
        from ... import candidates as best_of
        k, select, bandwidth = best_of.check_arguments(k, select, bandwidth, bool(self.use_kde))
        noise_scheduler = self.noise_scheduler if noise_scheduler is None else noise_scheduler
        state, goal, _ = self.process_batch(batch, predict=True)
        state, goal = self._encode_eval(state, goal)
        act_dim = self.scaler.y_bounds.shape[1]
        guide = best_of.check_guide(select, guide, state.shape[-1], act_dim, goal is not None, state.device, "predict_best_of")
        noise = best_of.check_noise(noise, len(state), k, act_dim, self.device)
        windowed = state.dim() == 2 and self.window_size > 1
        if windowed:
            self.obs_context.append(state)
            input_state = torch.stack(tuple(self.obs_context), dim=1)
        else:
            input_state = state
        if goal.dim() == 2 and self.window_size > 1:
            goal = goal.unsqueeze(0)                                       # 'b d -> 1 b d'
        sampler_type = self.sampler_type if new_sampler_type is None else new_sampler_type
        n_steps = self.num_sampling_steps if new_sampling_steps is None else new_sampling_steps
        B = len(input_state)
        state3 = (input_state if input_state.dim() == 3 else input_state.unsqueeze(1)).to(torch.float32).contiguous()
        t = state3.shape[1]
        with self._ema_scope():
            if self.model.training:
                self.model.eval()
            sigmas = self.get_noise_schedule(n_steps, noise_scheduler)
            # the window as predict lays it out: the remembered actions, then the newest slot (expand fills it per candidate)
            x = torch.zeros((B, 1, act_dim), dtype=torch.float32, device=state3.device)
            if windowed and len(self.action_context) > 0:
                x = torch.cat((*self.action_context, x), dim=1)
            if x.shape[1] != t:
                raise ValueError(f"predict_best_of: {x.shape[1]} action slots beside {t} observation slots")
            lengths = torch.full((B,), t, dtype=torch.int32, device=state3.device)
            state_k, x_k = best_of.expand(state3, x.contiguous(), lengths, noise, self.sigma_max)
            if input_state.dim() == 2:
                state_k = state_k[:, 0].contiguous()
            goal_n = goal if goal.dim() == 3 else goal.unsqueeze(0)          # what the ranking reads: one goal per environment, or one
            if goal.dim() == 3 and goal.shape[0] == B and B > 1:
                goal = torch.repeat_interleave(goal, k, dim=0)
            x0_k = self.sample_loop(sigmas, x_k, state_k, goal, sampler_type, extra_args)
            x0_k = x0_k.reshape(B * k, t, act_dim).to(torch.float32).contiguous()
            if guide is not None:
                x_0, index, scores = best_of.rank(state3, goal_n, x0_k, lengths, k, guide)
            else:
                x_0, index, scores = best_of.select(x0_k, lengths, k, select, bandwidth)
            if t > 1:
                x_0 = x_0[:, -1, :]
            x_0 = self.scaler.clip_action(x_0)
        model_pred = self.scaler.inverse_scale_output(x_0)
        if model_pred.dim() == 2:
            x_0 = x_0.unsqueeze(1)
        self.action_context.append(x_0)
        self.last_best_of = {"candidates": x0_k.view(B, k, t, act_dim)[:, :, -1], "scores": scores, "index": index}
        return model_pred

    def vector_rollout(self, n_envs: int):
        """A ``VectorRollout`` over ``n_envs`` environments that finish and reset independently: one sampler call per
        environment step for all of them, the windows kept per environment on the device (beso_amd/rollout.py).  ``predict``
        and ``reset`` keep serving the reference's single set of environments; the two share nothing but the agent."""
        self._refuse_with_encoder("vector_rollout")
        from ...rollout import VectorRollout
        return VectorRollout(self, n_envs)

    @torch.no_grad()
    def visualize_ode(self, state: torch.Tensor, goal, get_mean=1000, new_sampling_steps=None, noise_scheduler=None):
        """The denoising trajectory of ``get_mean`` DDIM samples per observation (beso_agent.py:478-538): the list of
        ``n_sampling_steps + 1`` action tensors ``[x_T, x after step 0, ..., x_0]``, each [N * get_mean, t, act].

        The reference calls ``sample_ddim`` once per step on a two-entry schedule; here the whole loop is ONE
        ``gc_sampling.sample_trajectory('ddim', ...)`` call whose launch records x behind every step (equal bits: a loop and
        its steps run one after the other agree).  Scaling, the observation window, the EMA weights, the schedule and the
        ``repeat_interleave`` of state and goal are the reference's; ``get_mean=None`` means 100 with ``use_kde``;
        ``noise_scheduler=None`` takes the agent's, and a 2-D goal is one goal sequence for every observation, as in ``predict``.
        Deviation: the reference draws a 2-D x [N * get_mean, act], which only fits a window of one; x is drawn here as
        [N * get_mean, t, act] with t the length of the observation context, the shape ``evaluate`` and ``predict`` feed the
        network.  Needs the HIP denoiser on the GPU (``sample_trajectory`` raises NotImplementedError otherwise)."""
        if self.use_kde:
            get_mean = 100 if get_mean is None else get_mean
        if get_mean is None:
            raise ValueError("visualize_ode: get_mean must be a number of samples per observation")
        n_steps = self.num_sampling_steps if new_sampling_steps is None else new_sampling_steps
        noise_scheduler = self.noise_scheduler if noise_scheduler is None else noise_scheduler
        state = self.scaler.scale_input(state)
        goal = self.scaler.scale_input(goal)
        state, goal = self._encode_eval(state, goal)
        if self.window_size > 1 and state.dim() == 2:
            self.obs_context.append(state)
            input_state = torch.stack(tuple(self.obs_context), dim=1)
        else:
            input_state = state.unsqueeze(1) if state.dim() == 2 else state
        if goal.dim() == 2:
            goal = goal.unsqueeze(0)                                       # 'b d -> 1 b d', as predict
        if goal.shape[0] == 1 and len(input_state) > 1:
            goal = goal.expand(len(input_state), -1, -1)
        act_dim = self.scaler.y_bounds.shape[1]
        with self._ema_scope():
            if self.model.training:
                self.model.eval()
            sigmas = self.get_noise_schedule(n_steps, noise_scheduler)
            x = torch.randn((len(input_state) * get_mean, input_state.shape[1], act_dim), device=self.device) * self.sigma_max
            state_rpt = torch.repeat_interleave(input_state, repeats=get_mean, dim=0)
            goal_rpt = torch.repeat_interleave(goal, repeats=get_mean, dim=0)
            _, xs, _ = ks.sample_trajectory('ddim', self.model, state_rpt, x, goal_rpt, sigmas, trace=('x',))
        return list(xs.unbind(0))

    def sample_loop(self, sigmas, x_t: torch.Tensor, state: torch.Tensor, goal: torch.Tensor, sampler_type: str,
                    extra_args={}):
        """Dispatch on ``sampler_type`` (beso_agent.py:390-456).  Only 'heun' receives s_churn / s_min;
        a non-empty ``extra_args`` must carry both 's_churn' and 'keep_last_actions' (KeyError
        otherwise, as in the reference :408-410)."""
        extra_args = {} if extra_args is None else extra_args
        s_churn = extra_args.get('s_churn', 0)
        s_min = extra_args.get('s_min', 0)
        reduced = {k: extra_args[k] for k in ('s_churn', 'keep_last_actions')} if extra_args else {}
        scaler = self.scaler if extra_args.get('use_scaler', False) else None
        m = self.model
        if isinstance(m, ClassifierGuidedSampleModel) and m.cond_lambda == 0:
            # a guidance scale of zero is no guidance (as ClassifierFreeSampleModel takes cond_lambda 0 and 1 as the plain
            # calls): the wrapped model, and with it the one-enqueue sampler loops an agent without the wrapper runs
            m = m.model
        if sampler_type == 'lms':
            return ks.sample_lms(m, state, x_t, goal, sigmas, scaler=scaler, disable=True, extra_args=reduced)
        if sampler_type == 'heun':
            return ks.sample_heun(m, state, x_t, goal, sigmas, scaler=scaler, s_churn=s_churn, s_tmin=s_min,
                                  disable=True)
        if sampler_type == 'euler':
            return ks.sample_euler(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'ancestral':
            return ks.sample_dpm_2_ancestral(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'euler_ancestral':
            return ks.sample_euler_ancestral(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'dpm':
            return ks.sample_dpm_2(m, state, x_t, goal, sigmas, disable=True)
        if sampler_type == 'ddim':
            return ks.sample_ddim(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'dpm_adaptive':
            return ks.sample_dpm_adaptive(m, state, x_t, goal, sigmas[-2].item(), sigmas[0].item(), disable=True)
        if sampler_type == 'dpm_fast':
            return ks.sample_dpm_fast(m, state, x_t, goal, sigmas[-2].item(), sigmas[0].item(), len(sigmas),
                                      disable=True)
        if sampler_type == 'dpmpp_2s_ancestral':
            return ks.sample_dpmpp_2s_ancestral(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'dpmpp_2s':
            return ks.sample_dpmpp_2s(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'dpmpp_2m':
            return ks.sample_dpmpp_2m(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        if sampler_type == 'dpmpp_2m_sde':
            return ks.sample_dpmpp_sde(m, state, x_t, goal, sigmas, scaler=scaler, disable=True)
        raise ValueError('desired sampler type not found!')

    # ------------------------------------------------------------------ checkpoints
    def load_pretrained_model(self, weights_path: str, **kwargs) -> None:
        """``model_state_dict.pth`` holds the EMA weights (beso_agent.py:458-464); the EMA shadow is
        re-seeded from the loaded parameters."""
        state = torch.load(os.path.join(weights_path, "model_state_dict.pth"), map_location=self.device)
        self.model.load_state_dict(state)
        self.ema_helper = ExponentialMovingAverage(self.model.get_params(), self.decay, self.device)
        self._ema_packed_key = None
        enc = self._trainable_encoder()
        if enc is not None:
            # ``encoder_state_dict.pth`` (the EMA weights) likewise; a directory without it loads into a ``NoEncoder`` agent only
            path = os.path.join(weights_path, "encoder_state_dict.pth")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: the agent has a trainable input encoder ({type(enc).__name__}) but the "
                                        "checkpoint directory holds no encoder weights")
            enc.network.load_state_dict(torch.load(path, map_location=self.device))
            self.encoder_ema = ExponentialMovingAverage(enc.get_params(), self.decay, self.device)
        log.info('Loaded pre-trained model parameters')

    def store_model_weights(self, store_path: str) -> None:
        """EMA weights -> model_state_dict.pth, raw weights -> non_ema_model_state_dict.pth
        (beso_agent.py:466-476)."""
        self._complete_ema()
        if bdist.rank() != 0:
            return
        ema, raw = self._state_pair(self.model, self.ema_helper)
        torch.save(ema, os.path.join(store_path, "model_state_dict.pth"))
        torch.save(raw, os.path.join(store_path, "non_ema_model_state_dict.pth"))
        enc = self._trainable_encoder()
        if enc is not None:
            # the encoder beside them: encoder_state_dict.pth (EMA) and non_ema_encoder_state_dict.pth
            ema, raw = self._state_pair(enc.network, self.encoder_ema)
            torch.save(ema, os.path.join(store_path, "encoder_state_dict.pth"))
            torch.save(raw, os.path.join(store_path, "non_ema_encoder_state_dict.pth"))

    def _state_pair(self, module, ema_helper):
        """(EMA, raw) state dicts of ``module``: the EMA one holds ``ema_helper``'s shadow (without ``use_ema``: the raw values)."""
        raw = {k: v.detach().clone() for k, v in module.state_dict().items()}
        ema = dict(raw)
        if self.use_ema:
            names = [n for n, p in module.named_parameters() if p.requires_grad]
            for n, s in zip(names, ema_helper.shadow_params):
                ema[n] = s.detach().clone()
        return ema, raw

    # ------------------------------------------------------------------ exact resume
    def _training_state_guard(self):
        self._refuse_with_encoder("store_training_state / load_training_state")
        if bdist.is_distributed() and bdist.world_size() > 1:
            raise NotImplementedError("store_training_state / load_training_state: single process only (sharded EMA shadows and "
                                      "per-rank generators are not saved)")

    def _sync_device(self):
        # (the asynchronous loss stream and the step's side streams are drained too: a device-wide synchronise)
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize(self.device)

    def store_training_state(self, store_path: str, feed=None) -> None:
        """Everything the next ``train_step`` reads -> ``training_state.pth`` beside the files of ``store_model_weights``:
        the raw parameters, the EMA shadow with its counters, the optimizer's moments and step counts
        (``FusedAdam.export_state()``; ``state_dict()`` of an eager optimizer), the LR scheduler, ``steps``, torch's CPU
        generator (the dropout seed is drawn there) and the device generator (noise, sigma), and the position of ``feed``
        (a ``DeviceTrajectoryFeed``) when given.  With ``deterministic_training`` a run that loads this file continues with
        the bits of the run that wrote it.  Synchronises.  Single process only."""
        self._training_state_guard()
        self._sync_device()
        dev = torch.device(self.device)
        ema = self.ema_helper
        fused = isinstance(self.optimizer, FusedAdam)
        state = dict(
            version=1,
            params=[p.detach().cpu().clone() for p in self.model.parameters()],
            ema=dict(flat=ema._flat.detach().cpu().clone(), decay=ema.decay, num_updates=ema.num_updates, steps=ema.steps,
                     version=ema.version),
            optimizer_kind="fused" if fused else "eager",
            optimizer=self.optimizer.export_state() if fused else self.optimizer.state_dict(),
            lr_scheduler=self.lr_scheduler.state_dict() if self.lr_scheduler is not None else None,
            steps=int(self.steps),
            cpu_rng=torch.get_rng_state(),
            device_rng=torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,
            feed=feed.state_dict() if feed is not None else None)
        torch.save(state, os.path.join(store_path, "training_state.pth"))

    def load_training_state(self, store_path: str, feed=None) -> None:
        """Load ``training_state.pth`` written by ``store_training_state`` into an agent of the same construction (and into
        ``feed``, when the file holds a feed's position).  The packed-weight caches are marked stale and the parameters'
        version counters bumped, as after an optimizer step.  Synchronises.  Single process only."""
        self._training_state_guard()
        self._sync_device()
        dev = torch.device(self.device)
        state = torch.load(os.path.join(store_path, "training_state.pth"), map_location="cpu", weights_only=False)
        params = list(self.model.parameters())
        saved = state["params"]
        if len(saved) != len(params) or any(tuple(s.shape) != tuple(p.shape) for s, p in zip(saved, params)):
            raise ValueError("load_training_state: the saved parameters do not match this model")
        ema, se = self.ema_helper, state["ema"]
        if se["flat"].numel() != ema._flat.numel():
            raise ValueError("load_training_state: the saved EMA shadow does not match this model")
        fused = isinstance(self.optimizer, FusedAdam)
        if (state["optimizer_kind"] == "fused") != fused:
            raise ValueError("load_training_state: the file was written with another optimizer class")
        if (feed is None) != (state["feed"] is None):
            raise ValueError("load_training_state: the file %s a feed's position" % ("holds" if feed is None else "does not hold"))
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.data.copy_(s)
            ema._flat.copy_(se["flat"])
        ema.decay, ema.num_updates, ema.steps = se["decay"], se["num_updates"], se["steps"]
        ema.version = max(int(se["version"]), ema.version) + 1        # (never a version this agent has packed an image of)
        if fused:
            self.optimizer.import_state(state["optimizer"])
        else:
            self.optimizer.load_state_dict(state["optimizer"])
        if self.lr_scheduler is not None and state["lr_scheduler"] is not None:
            self.lr_scheduler.load_state_dict(state["lr_scheduler"])
        self.steps = int(state["steps"])
        torch.set_rng_state(state["cpu_rng"])
        if dev.type == "cuda" and state["device_rng"] is not None:
            torch.cuda.set_rng_state(state["device_rng"], dev)
        if feed is not None:
            feed.load_state_dict(state["feed"])
        # the parameters and the shadow changed under every cache keyed on them
        torch.autograd.graph.increment_version(params)
        den = self._hip_denoiser()
        if den is not None:
            den.inner_model.mark_weights_dirty()
        self._ema_packed_key = None
        self._ema_partial = False
        self._sync_device()

    # ------------------------------------------------------------------ sigma density / schedules
    def make_sample_density(self):
        """Training distribution of sigma (beso_agent.py:541-580)."""
        kind = self.sigma_sample_density_type
        if kind == 'lognormal':
            return partial(utils.rand_log_normal, loc=self.sigma_sample_density_mean,
                           scale=self.sigma_sample_density_std)
        if kind == 'loglogistic':
            return partial(utils.rand_log_logistic, loc=math.log(self.sigma_data), scale=0.5,
                           min_value=self.sigma_min, max_value=self.sigma_max)
        if kind == 'loguniform':
            return partial(utils.rand_log_uniform, min_value=self.sigma_min, max_value=self.sigma_max)
        if kind == 'uniform':
            return partial(utils.rand_uniform, min_value=self.sigma_min, max_value=self.sigma_max)
        if kind == 'v-diffusion':
            return partial(utils.rand_v_diffusion, sigma_data=self.sigma_data, min_value=self.sigma_min,
                           max_value=self.sigma_max)
        if kind == 'discrete':
            return partial(utils.rand_discrete, values=self.get_noise_schedule(self.num_sampling_steps, 'exponential'))
        raise ValueError('Unknown sample density type')

    def get_noise_schedule(self, n_sampling_steps, noise_schedule_type):
        """(beso_agent.py:582-598).  Schedules are built on the host: the samplers read them there."""
        if noise_schedule_type == 'karras':
            return ks.get_sigmas_karras(n_sampling_steps, self.sigma_min, self.sigma_max, self.rho, 'cpu')
        if noise_schedule_type == 'exponential':
            return ks.get_sigmas_exponential(n_sampling_steps, self.sigma_min, self.sigma_max, 'cpu')
        if noise_schedule_type == 'vp':
            return ks.get_sigmas_vp(n_sampling_steps, device='cpu')
        if noise_schedule_type == 'linear':
            return ks.get_sigmas_linear(n_sampling_steps, self.sigma_min, self.sigma_max, device='cpu')
        if noise_schedule_type == 'cosine_beta':
            return ks.cosine_beta_schedule(n_sampling_steps, device='cpu')
        if noise_schedule_type == 've':
            return ks.get_sigmas_ve(n_sampling_steps, self.sigma_min, self.sigma_max, device='cpu')
        if noise_schedule_type == 'iddpm':
            return ks.get_iddpm_sigmas(n_sampling_steps, self.sigma_min, self.sigma_max, device='cpu')
        raise ValueError('Unknown noise schedule type')
