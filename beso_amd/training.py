"""HIP training step of the score network: ``GCDenoiser.loss`` forward and the
gradient of the loss with respect to every parameter as ONE enqueue of ``beso_loss_grad``
(beso_amd/csrc/train.hip), replacing ``loss = model.loss(...); loss.backward()`` of the reference's
``train_step`` (beso_agent.py:226-235).

Two ways in:

* ``GCDenoiser.loss`` (training mode, HIP parameters) returns ``ScoreMatchingLoss.apply(...)``, an autograd
  node whose backward hands the precomputed gradients to autograd -- user code that calls ``loss.backward()``
  keeps working unchanged;
* ``HipTrainStep.loss_backward`` is what ``BesoAgent.train_step`` uses: it writes ``p.grad`` as views of one
  persistent flat buffer (stable addresses for the fused optimizer's chunk table, one flat tensor for the
  data-parallel all-reduce) and returns the loss.

There is no CPU implementation and no second evaluation of the network behind it: what the kernels do not cover
(``embed_dim`` not a multiple of 8, attention windows beyond the LDS budget, unknown ``loss`` kwargs) raises
(``GCDenoiser.loss``); the torch-autograd evaluation of the same function lives in ``tests/autograd_reference.py`` as
the comparator of this step.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from . import _lib
from .runtime import _f32c, prepare_inputs, stream_ptr, train_hints, train_precision, workspace

# The training entry points, widest first: (name, how many trailing arguments it takes behind `stream`).  On the C side each
# is the next one with trailing NULLs: a call passes all of them, None where it has nothing, cut to the entry point's count.
_LOSS_GRAD = (("beso_loss_grad_inputs", 4), ("beso_loss_grad_streams", 2), ("beso_loss_grad_overlap", 1))
_DENOISE_VJP = (("beso_denoise_vjp_inputs", 2), ("beso_denoise_vjp", 0))


def _entry(lib, entries, need: int, most: int):
    """-> (function, its trailing-argument count): the widest of ``entries`` that ``lib`` has among those that take at least
    the ``need`` trailing arguments the call cannot do without and at most the ``most`` it has a use for (a library loaded
    through BESO_HIP_LIB may predate the wider ones: tools/variants.py's '@<revision>' A/B builds)."""
    for name, n in entries:
        fn = getattr(lib, name, None) if need <= n <= most else None
        if fn is not None:
            return fn, n
    raise _lib.BesoHipError(f"beso_hip: the loaded library has none of {[name for name, n in entries if need <= n <= most]}")


class HipTrainStep:
    """Binds one ``DiffusionGPT`` to ``beso_loss_grad``: flat gradient buffer, workspace, dropout seed."""

    def __init__(self, inner, sigma_data: float):
        self.inner = inner
        self.sigma_data = float(sigma_data)
        self.lib = _lib.load()
        self.cfg = inner.shape(self.sigma_data).c_struct()
        self.n_params = self.lib.beso_num_params(C.byref(self.cfg))
        self.n_grad = int(self.lib.beso_grad_floats(C.byref(self.cfg)))
        self._flat: Optional[torch.Tensor] = None
        self._flat_full: Optional[torch.Tensor] = None      # _flat plus the zero tail of the sharded exchange
        self.pad_to = 0
        self._views: Optional[List[torch.Tensor]] = None
        self._ws: Optional[torch.Tensor] = None
        # every call of this step runs with BESO_TRAIN_DETERMINISTIC: GCDenoiser.hip_train_step copies its own
        # `deterministic_training` here (BesoAgent(deterministic_training=True) sets that), which reaches loss_backward and
        # GCDenoiser.loss under autograd; run()'s keyword is for a caller that drives the step itself
        self.deterministic = False

    # ------------------------------------------------------------------ eligibility
    @staticmethod
    def supported(inner) -> bool:
        return inner.embed_dim % 8 == 0

    def _params(self):
        """(Parameter list, their data pointers as a tuple).  Walking the module tree costs ~50 us per traversal and a step
        used to do four; the list is kept (a module's Parameter objects do not change identity under .to(), load_state_dict
        or the EMA swap -- their storage may, which the pointer tuple shows) and rebuilt when its length stops matching."""
        pl = self.__dict__.get("_plist")
        if pl is None or len(pl) != self.n_params or self.__dict__.get("_plist_epoch") != getattr(self.inner, "_dirty_epoch", 0):
            pl = list(self.inner.parameters())
            self._plist, self._plist_epoch = pl, getattr(self.inner, "_dirty_epoch", 0)
            self._ptrs_ok = None
        return pl, tuple(p.data_ptr() for p in pl)

    def eligible(self, state, action, goal, noise, sigma) -> bool:
        params, ptrs = self._params()
        if self.__dict__.get("_ptrs_ok") != ptrs:             # (checked once per set of storages)
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.requires_grad for p in params):
                return False
            if sum(p.numel() for p in params) != self.n_grad or len(params) != self.n_params:
                return False
            self._ptrs_ok = ptrs
        elif not all(p.requires_grad for p in params):
            return False
        for x in (state, action, noise, sigma) + ((goal,) if goal is not None else ()):
            if not torch.is_tensor(x) or not x.is_cuda:
                return False
        # (state / goal may require grad: run(input_grads=True).  Gradients with respect to action, noise and sigma are not computed)
        if action.requires_grad or noise.requires_grad or sigma.requires_grad:
            return False
        if self.inner.goal_seq_len > 0 and goal is None:
            return False
        return self.supported(self.inner)

    # ------------------------------------------------------------------ buffers
    def _grad_buffer(self, dev, fresh: bool):
        if fresh:
            flat = torch.empty(self.n_grad, dtype=torch.float32, device=dev)
        else:
            if (self._flat is None or self._flat_full is None or self._flat.device != dev
                    or self._flat_full.numel() != max(self.n_grad, self.pad_to)):
                # (pad_to: the sharded data-parallel exchange reduce-scatters a buffer of world * ceil(n / world) floats;
                # the kernels write the first n_grad, the tail stays zero)
                self._flat_full = torch.zeros(max(self.n_grad, self.pad_to), dtype=torch.float32, device=dev)
                self._flat = self._flat_full[: self.n_grad]
                self._views = None
            flat = self._flat
        views, off = [], 0
        if fresh or self._views is None:
            for p in self._params()[0]:
                views.append(flat[off:off + p.numel()].view_as(p))
                off += p.numel()
            if not fresh:
                self._views = views
        else:
            views = self._views
        return flat, views

    def _workspace(self, batch: int, t: int, precision: int, dev) -> torch.Tensor:
        need = int(self.lib.beso_train_workspace_bytes(C.byref(self.cfg), batch, t, precision))
        if need == 0:
            raise ValueError(f"beso_hip: training step unsupported for batch={batch} t={t} with this model shape")
        return workspace(self, need, dev)

    # ------------------------------------------------------------------ the call
    def early_range(self):
        """[begin, end) floats of the flat gradient buffer that are complete first (the upper layers + ln_f):
        what ``run(..., early_stream=...)`` releases to that stream while the rest of the backward still runs."""
        b, e = C.c_size_t(0), C.c_size_t(0)
        _lib.check(self.lib.beso_grad_early_range(C.byref(self.cfg), C.byref(b), C.byref(e)), "grad_early_range")
        return int(b.value), int(e.value)

    def run(self, state, action, goal, noise, sigma, grad_scale: float = 1.0, seed: Optional[int] = None,
            fresh_grads: bool = False, last_action_only: bool = False, early_stream=None, goal_drop: Optional[float] = None,
            loss_stream=None, deterministic: bool = False, input_grads: bool = False):
        """-> (loss 0-d tensor, flat gradient tensor, list of per-parameter views).  Inputs are NOT modified.
        ``input_grads``: the result gains ``(state_grad, goal_grad)`` -- the gradient of the loss (times ``grad_scale``) with
        respect to ``state`` [B,t,obs] and to the goals as the kernel saw them [B,G,obs] (a goal given without batch dimension
        was expanded over the batch: sum over dim 0 for its own gradient), fp32, with this call's embedding dropout and goal
        mask; ``goal_grad`` is None when G = 0 (``beso_loss_grad_inputs``).
        ``early_stream`` (a torch.cuda.Stream): ordered behind the completion of ``early_range()`` by the call.
        ``loss_stream`` (a torch.cuda.Stream): ordered behind the point where the loss value is final (the end of the forward
        half) -- a host read of the loss on that stream does not wait for the backward pass.
        ``goal_drop``: None = the module's ``cond_mask_prob`` (training mode); 0 = the goals are taken as they are.
        ``deterministic`` (or ``self.deterministic``): ``BESO_TRAIN_DETERMINISTIC`` -- the loss and every gradient are summed in
        a fixed order, so the same inputs and ``seed`` give the same bits on every call (include/beso_hip.h)."""
        inner = self.inner
        dev = action.device
        G = inner.goal_seq_len
        n_sigma = sigma.numel()
        state, action, goal, sigma = prepare_inputs(state.detach(), action.detach(), None if goal is None else goal.detach(),
                                                    sigma.detach(), inner.obs_dim, inner.action_dim, G, dev)
        B, t, _ = state.shape
        noise = _f32c(noise.detach(), dev)
        if noise.shape != action.shape or n_sigma != B:          # (one sigma per sample: no scalar is spread over a training batch)
            raise ValueError("action / noise must be [B,t,act] and sigma [B]")
        gptr = goal.data_ptr() if goal is not None else None
        embed_p, attn_p, resid_p = inner._pdrops
        # training-mode goal masking (DiffusionGPT.mask_cond, score_gpts.py:298-299) is part of the kernel: the goals
        # go in unmasked together with the drop probability
        goal_p = float(getattr(inner, "cond_mask_prob", 0.0) or 0.0) if (G > 0 and goal_drop is None) else float(goal_drop or 0.0)
        if not inner.training:
            embed_p = attn_p = resid_p = goal_p = 0.0
        if seed is None:
            if (embed_p > 0.0 or attn_p > 0.0 or resid_p > 0.0 or goal_p > 0.0) and torch.cuda.is_current_stream_capturing():
                # the seed is a host scalar: a captured graph would replay one mask forever
                raise RuntimeError("beso_amd: the HIP training step with dropout cannot be captured into a graph")
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,), device="cpu").item())
        precision = train_precision(inner.precision)
        params, ptrs = self._params()
        if self.__dict__.get("_arr_ptrs") != ptrs:
            self._arr, self._arr_ptrs = (C.c_void_p * len(ptrs))(*ptrs), ptrs
        arr = self._arr
        flat, views = self._grad_buffer(dev, fresh_grads)
        ws = self._workspace(B, t, precision, dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        if loss_stream is not None:
            loss.record_stream(loss_stream)          # (read there; the caching allocator must not hand it out before that)
        common = (C.byref(self.cfg), arr, len(params), flat.data_ptr(), precision,
                  state.data_ptr(), action.data_ptr(), gptr, noise.data_ptr(), sigma.data_ptr(),
                  loss.data_ptr(), B, t, (_lib.TRAIN_LAST_ACTION_ONLY if last_action_only else 0) | train_hints()
                  | (_lib.TRAIN_DETERMINISTIC if (deterministic or self.deterministic) else 0), float(embed_p), float(attn_p), float(resid_p),
                  float(goal_p), C.c_uint(seed & 0xFFFFFFFF), float(grad_scale), ws.data_ptr(), ws.numel(), stream_ptr(dev))
        state_grad = goal_grad = None
        if input_grads:
            state_grad = torch.empty_like(state)
            goal_grad = torch.empty_like(goal) if G > 0 else None
        trailing = (early_stream.cuda_stream if early_stream is not None else None,
                    loss_stream.cuda_stream if loss_stream is not None else None,
                    state_grad.data_ptr() if state_grad is not None else None,
                    goal_grad.data_ptr() if goal_grad is not None else None)
        # (the input gradients need their entry point; a call without them stays on beso_loss_grad_streams, the symbol that
        # tools/train_host_profile.py and the flag test of tests/test_reproducible_training.py wrap)
        fn, n = _entry(self.lib, _LOSS_GRAD, 4 if input_grads else 1, 4 if input_grads else 2)
        with torch.cuda.device(dev):
            st = fn(*common, *trailing[:n])
            if n < 2 and loss_stream is not None:
                # (a library that predates the loss stream: the loss is then final at the end of the call's work on the
                # compute stream; order the caller's stream behind that instead of failing)
                loss_stream.wait_stream(torch.cuda.current_stream(dev))
        _lib.check(st, "loss_grad")
        if input_grads:
            return loss, flat, views, state_grad, goal_grad
        return loss, flat, views

    def denoise_vjp(self, state, x, goal, sigma, cot, uncond: bool = False, input_grads: bool = False):
        """-> (denoised, x_grad, dot): ``GCDenoiser.forward`` in eval mode at x, the vector-Jacobian product
        (d denoised / d x)^T cot and its per-sample dot product with cot, as ONE enqueue of ``beso_denoise_vjp``
        (the training step's forward and data-gradient chain, no weight gradient).  The parameters need not require
        grad and the call works under ``torch.no_grad()``; no ``.grad`` is created or changed.
        ``input_grads``: -> (denoised, x_grad, dot, state_grad, goal_grad) with (d denoised / d state)^T cot [B,t,obs] and
        (d denoised / d goal)^T cot [B,G,obs] (``beso_denoise_vjp_inputs``); ``goal_grad`` is None when G = 0 and exactly zero
        with ``uncond`` (the goals are replaced by zeros there)."""
        inner = self.inner
        if inner.training and any(p > 0 for p in inner._pdrops):
            raise RuntimeError("beso_amd: denoise_vjp evaluates the eval-mode function; call eval() on a model with dropout")
        params, ptrs = self._params()
        if self.__dict__.get("_vjp_ptrs_ok") != ptrs:
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params):
                raise ValueError("beso_amd: denoise_vjp needs contiguous fp32 parameters on the GPU")
            if sum(p.numel() for p in params) != self.n_grad or len(params) != self.n_params:
                raise ValueError("beso_amd: the module's parameters do not match its HIP layout")
            self._vjp_ptrs_ok = ptrs
        if not self.supported(inner):
            raise ValueError(f"beso_amd: denoise_vjp needs embed_dim % 8 == 0 (embed_dim={inner.embed_dim})")
        dev = x.device
        if not x.is_cuda:
            raise ValueError("beso_amd: denoise_vjp inputs must be on the GPU (there is no CPU path)")
        G = inner.goal_seq_len
        # the goals are a live input of this call; uncond or no goal: DiffusionGPT.forward puts zeros in their place
        # (score_gpts.py:301-302), nothing depends on them -- the kernel gets no goal output (NULL) and the gradient is zeros
        goal_live = G > 0 and not uncond and goal is not None
        state, x, goal, sigma = prepare_inputs(state.detach(), x.detach(), goal.detach() if goal_live else None,
                                               torch.as_tensor(sigma).detach(), inner.obs_dim, inner.action_dim,
                                               G if goal_live else 0, dev)
        B, t, _ = state.shape
        cot = _f32c(cot.detach(), dev)
        if cot.shape != x.shape:
            raise ValueError("state must be [B,t,obs], x and cot [B,t,act]")
        if G > 0 and not goal_live:
            goal = torch.zeros(B, G, inner.obs_dim, dtype=torch.float32, device=dev)
        gptr = goal.data_ptr() if goal is not None else None
        precision = train_precision(inner.precision)
        if self.__dict__.get("_arr_ptrs") != ptrs:
            self._arr, self._arr_ptrs = (C.c_void_p * len(ptrs))(*ptrs), ptrs
        ws = self._workspace(B, t, precision, dev)
        denoised, x_grad = torch.empty_like(x), torch.empty_like(x)
        dot = torch.empty(B, dtype=torch.float32, device=dev)
        flags = train_hints() & (_lib.TRAIN_PLAN_PER_OP | _lib.TRAIN_PLAN_TILES)
        args = (C.byref(self.cfg), self._arr, len(params), precision, state.data_ptr(), x.data_ptr(), gptr, sigma.data_ptr(),
                cot.data_ptr(), denoised.data_ptr(), x_grad.data_ptr(), dot.data_ptr(), B, t, flags, ws.data_ptr(), ws.numel(),
                stream_ptr(dev))
        state_grad = goal_grad = None
        if input_grads:
            state_grad = torch.empty_like(state)
            if G > 0:
                goal_grad = torch.empty_like(goal) if goal_live else torch.zeros_like(goal)
        trailing = (state_grad.data_ptr() if state_grad is not None else None,
                    goal_grad.data_ptr() if goal_live and goal_grad is not None else None)
        n = 2 if input_grads else 0
        fn, n = _entry(self.lib, _DENOISE_VJP, n, n)
        with torch.cuda.device(dev):
            st = fn(*args, *trailing[:n])
        _lib.check(st, "denoise_vjp")
        if input_grads:
            return denoised, x_grad, dot, state_grad, goal_grad
        return denoised, x_grad, dot

    def goal_mask(self, batch: int, seed: int, goal_drop: Optional[float] = None, device=None) -> torch.Tensor:
        """The keep-mask [batch, G, obs] the kernel applies to the goals for (goal_drop, seed) (``beso_goal_mask``)."""
        inner = self.inner
        p = float(inner.cond_mask_prob if goal_drop is None else goal_drop)
        dev = torch.device(device) if device is not None else next(inner.parameters()).device
        mask = torch.empty(batch, inner.goal_seq_len, inner.obs_dim, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self.lib.beso_goal_mask(mask.data_ptr(), batch, inner.goal_seq_len, inner.obs_dim, p,
                                               C.c_uint(seed & 0xFFFFFFFF),
                                               stream_ptr(dev)), "goal_mask")
        return mask

    def dropout_mask(self, kind, layer: int, batch: int, t: int, seed: int, p: Optional[float] = None, device=None) -> torch.Tensor:
        """The keep-scale (0 or 1/(1-p) per element) of one training dropout as ``run(..., seed=seed)`` applies it to a
        batch of ``batch`` windows of ``t`` steps (``beso_dropout_mask``): what the module's ``nn.Dropout`` would have
        multiplied by, drawn with the library's counter hash instead of torch's generator.

        ``kind``: ``"embed"`` (``inner.drop``), ``"attn"`` (``blocks[layer].attn.attn_drop``), ``"proj"``
        (``blocks[layer].attn.resid_drop``), ``"mlp"`` (``blocks[layer].mlp[3]``), or the ``_lib.DROP_*`` integer; ``layer``
        is ignored for ``"embed"``.  ``p=None`` takes the module's own probability for that kind.  Returns
        ``[batch, H, T, T]`` for ``"attn"`` (every query / key pair, the causally masked ones too) and ``[batch, T, D]`` for
        the others, ``T = 1 + G + 2 t`` in the network's token order (sigma, goals, then state / action alternating).
        Elements the step draws no mask for are 1: the sigma-token row of ``"embed"``, and every row but the action
        tokens' of ``"proj"`` / ``"mlp"`` in the last layer (the loss reads the action tokens only; the step does not
        evaluate the others there).

        Caveat for comparisons against the reference network: the kernel draws the embedding mask per sample row, while
        the reference, given a goal with batch dimension 1, draws ONE goal-embedding mask and expands it over the batch.
        Pass goals as ``[B, G, obs]`` when a torch evaluation is to reproduce the step with these masks."""
        inner = self.inner
        k = _lib.DROP_KINDS[kind] if isinstance(kind, str) else int(kind)
        if p is None:
            embed_p, attn_p, resid_p = inner._pdrops
            p = {_lib.DROP_EMBED: embed_p, _lib.DROP_ATTN: attn_p}.get(k, resid_p)
        dev = torch.device(device) if device is not None else next(inner.parameters()).device
        T = 1 + inner.goal_seq_len + 2 * int(t)
        shape = (batch, inner.n_heads, T, T) if k == _lib.DROP_ATTN else (batch, T, inner.embed_dim)
        if batch < 1 or t < 1:
            raise ValueError(f"beso_amd: dropout_mask needs batch >= 1 and t >= 1 (batch={batch}, t={t})")
        scale = torch.empty(shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(self.lib.beso_dropout_mask(C.byref(self.cfg), scale.data_ptr(), k, int(layer), int(batch), int(t), float(p),
                                                  C.c_uint(seed & 0xFFFFFFFF),
                                                  stream_ptr(dev)), "dropout_mask")
        return scale

    def loss_backward(self, state, action, goal, noise, sigma, grad_scale: float = 1.0, seed: Optional[int] = None,
                      early_stream=None, loss_stream=None, input_grads: bool = False):
        """The training step's ``loss = model.loss(...); loss.backward()``: returns the loss and leaves the
        gradients in ``p.grad`` (views of the persistent flat buffer; accumulated into an existing ``.grad``).
        ``input_grads``: -> (loss, state_grad, goal_grad) as ``run`` returns them (no ``.grad`` of an input is touched)."""
        loss, flat, views, *extra = self.run(state, action, goal, noise, sigma, grad_scale, seed, fresh_grads=False,
                                             early_stream=early_stream, loss_stream=loss_stream, input_grads=input_grads)
        for p, v in zip(self._params()[0], views):
            if p.grad is None or p.grad.data_ptr() == v.data_ptr():
                p.grad = v
            else:
                p.grad.add_(v)
        return (loss, *extra) if input_grads else loss

    def flat_grads_padded(self) -> Optional[torch.Tensor]:
        """flat_grads() with its zero tail (``pad_to`` floats in all), for the reduce-scatter of the sharded exchange."""
        return None if self.flat_grads() is None else self._flat_full

    def flat_grads(self) -> Optional[torch.Tensor]:
        """The flat buffer if every ``p.grad`` currently is its view of it (then one all-reduce covers them)."""
        if self._flat is None or self._views is None:
            return None
        for p, v in zip(self._params()[0], self._views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                return None
        return self._flat


class ScoreMatchingLoss(torch.autograd.Function):
    """loss = GCDenoiser.loss(...) with the parameter gradients computed alongside (HIP); backward hands them over --
    and, where ``state`` / ``goal`` require grad (the outputs of a trainable encoder), the gradients with respect to those.
    Gradients with respect to action, noise and sigma are not computed (None)."""

    @staticmethod
    def forward(ctx, step: HipTrainStep, last_action_only: bool, state, action, goal, noise, sigma, *params):
        # (argument positions of forward: step 0, last_action_only 1, state 2, action 3, goal 4)
        want_state, want_goal = ctx.needs_input_grad[2], ctx.needs_input_grad[4] and step.inner.goal_seq_len > 0
        out = step.run(state, action, goal, noise, sigma, fresh_grads=True, last_action_only=last_action_only,
                       input_grads=want_state or want_goal)
        loss, ctx.flat, ctx.views = out[:3]
        # (fp32 gradient as run() returned it, the input's own shape, its dtype) per differentiated input
        ctx.state_grad = (out[3], state.shape, state.dtype) if want_state else None
        ctx.goal_grad = (out[4], goal.shape, goal.dtype) if want_goal else None
        return loss

    @staticmethod
    def _input_grad(kept, grad_out):
        """grad_out times the kept fp32 gradient, in the input's own shape and dtype: a goal given as [G,obs] or [1,G,obs] was
        expanded over the batch by run(), so its gradient is the sum over the samples.  Out of place, like the parameter
        gradients; a constant to autograd (no double backward)."""
        if kept is None:
            return None
        g, shape, dtype = kept
        return (g * grad_out.to(g.dtype)).sum_to_size(shape).to(dtype)

    @staticmethod
    def backward(ctx, grad_out):
        scaled = ctx.flat * grad_out               # out of place: a second backward through a retained graph stays right
        grads, off = [], 0
        for v in ctx.views:
            grads.append(scaled[off:off + v.numel()].view_as(v))
            off += v.numel()
        return (None, None, ScoreMatchingLoss._input_grad(ctx.state_grad, grad_out), None,
                ScoreMatchingLoss._input_grad(ctx.goal_grad, grad_out), None, None) + tuple(grads)
