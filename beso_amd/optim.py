"""Fused optimizer step for the score-matching training step (kernels K11/K12).

``FusedAdam`` is a ``torch.optim.Optimizer`` with the constructor and ``param_groups`` of
``torch.optim.Adam`` / ``torch.optim.AdamW`` (the two optimizers the reference configures:
configs/agents/beso_kitchen.yaml:9-12, beso_block_push.yaml:9-11), so LR schedulers attach to it
unchanged.  ``step()`` updates ALL parameters -- and, when an EMA helper is handed over, its shadow copy
(ema.py:45-53) -- in one HIP launch (``beso_adam_step``) instead of several hundred eager launches.
There is no CPU implementation: ``maybe_fuse`` leaves a CPU optimizer untouched.  The moments live in flat
buffers owned by the optimizer object (not in ``Optimizer.state``), so ``state_dict()`` does not carry them (the
reference's training loop, ``beso_agent.py:466-476``, stores model weights only); ``export_state()`` /
``import_state()`` save and restore them for an exact resume (``BesoAgent.store_training_state``).

``step(max_grad_norm=..., skip_nonfinite=...)`` adds global gradient-norm clipping and a guard that drops a step whose
gradient is not finite.  Both consume the norm ON THE DEVICE (``beso_grad_sumsq`` -> ``beso_adam_step_clipped``): the
host never reads it, so the asynchronous training step stays asynchronous."""
from __future__ import annotations

import math

import torch

from . import _lib
from .runtime import stream_ptr

CHUNK = 4096


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or weight_decay < 0.0:
            raise ValueError("invalid Adam hyper-parameter")
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self._groups = [None] * len(self.param_groups)      # per group: flat state + chunk table

    @classmethod
    def from_torch(cls, opt: torch.optim.Optimizer) -> "FusedAdam":
        """Same parameters and hyper-parameters as a freshly constructed torch Adam / AdamW."""
        decoupled = isinstance(opt, torch.optim.AdamW)
        groups = [dict(params=g["params"], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"],
                       decoupled_weight_decay=decoupled) for g in opt.param_groups]
        return cls(groups)

    def _prepare(self, gi: int, group: dict, shard=None):
        params = [p for p in group["params"] if p.grad is not None]
        sig = (shard,) + tuple((p.data_ptr(), p.grad.data_ptr(), p.numel()) for p in params)
        st = self._groups[gi]
        if st is not None and st["sig"] == sig:
            return st
        all_params = list(group["params"])
        dev = all_params[0].device
        for p in all_params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or not p.is_cuda:
                raise ValueError("FusedAdam needs contiguous fp32 parameters on one HIP device")
        offs, total = {}, 0
        for p in all_params:                                  # state offsets are fixed by the parameter order
            offs[id(p)] = total
            total += p.numel()
        if st is None:
            st = dict(m=torch.zeros(total, device=dev), v=torch.zeros(total, device=dev), step=0, offs=offs, total=total)
        rows = []
        for p in params:
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError("FusedAdam needs contiguous fp32 gradients")
            n, off = p.numel(), offs[id(p)]
            # shard = [lo, hi) of the flat parameter order (ZeRO-1 style data parallelism: this rank owns and updates
            # only that range; the moments of the rest are never touched here)
            s0, s1 = (0, n) if shard is None else (max(0, shard[0] - off), min(n, shard[1] - off))
            for s in range(s0, s1, CHUNK):
                c = min(CHUNK, s1 - s)
                rows.append((p.data_ptr() + 4 * s, g.data_ptr() + 4 * s, off + s, c))
        st["table"] = torch.tensor(rows, dtype=torch.int64).to(dev) if rows else None      # 32-byte beso_optim_chunk rows
        st["n_chunks"] = len(rows)
        st["sig"] = sig
        self._groups[gi] = st
        return st

    def _clip_scratch(self, st: dict):
        """``stats`` (double[4]: sumsq, norm, coefficient, skipped steps -- include/beso_hip.h) and ``partial`` (one double
        per chunk) of a group, next to its moments.  ``partial`` is re-made when the chunk table changes; ``stats`` is made
        once, so that the skip counter and the views the accessors handed out stay valid."""
        dev = st["m"].device
        if "stats" not in st:
            st["stats"] = torch.zeros(4, dtype=torch.float64, device=dev)
        if st.get("partial") is None or st["partial"].numel() < st["n_chunks"]:
            st["partial"] = torch.empty(max(st["n_chunks"], 1), dtype=torch.float64, device=dev)
        return st["partial"], st["stats"]

    def _stats(self, group: int) -> torch.Tensor:
        st = self._groups[group]
        if st is None or "stats" not in st:
            raise RuntimeError("no step with max_grad_norm / skip_nonfinite has run yet")
        return st["stats"]

    def last_grad_norm(self, group: int = 0) -> torch.Tensor:
        """The global L2 norm of the gradient the last clipped / guarded step saw (before clipping; the fp32 value, as a
        0-d float64 DEVICE view: reading it is the caller's synchronisation, calling this is none)."""
        return self._stats(group)[1]

    def last_clip_coef(self, group: int = 0) -> torch.Tensor:
        """The coefficient the last clipped / guarded step multiplied the gradient by (1: not clipped, 0: step skipped);
        a 0-d device view."""
        return self._stats(group)[2]

    def skipped_steps(self, group: int = 0) -> torch.Tensor:
        """How many steps ``skip_nonfinite`` has dropped so far; a 0-d device view."""
        return self._stats(group)[3]

    # ------------------------------------------------------------------ checkpoint
    _HYPER = ("lr", "betas", "eps", "weight_decay", "decoupled_weight_decay")

    def export_state(self) -> dict:
        """Everything ``step()`` carries from one call to the next, as CPU tensors and scalars: per parameter group the
        moments ``m`` / ``v`` (flat, parameter order; None before the group's first step), the step count, the four ``stats``
        doubles of the clipped step when they exist (``skipped_steps()`` survives), the element count, and the group's
        hyper-parameters (``lr`` as the scheduler left it, and ``initial_lr`` when a scheduler set one).  Synchronises."""
        groups = []
        for st, group in zip(self._groups, self.param_groups):
            total = sum(p.numel() for p in group["params"])
            g = dict(numel=total, step=0, m=None, v=None, stats=None, hyper={k: group[k] for k in self._HYPER})
            if "initial_lr" in group:
                g["hyper"]["initial_lr"] = group["initial_lr"]
            if st is not None:
                g.update(step=int(st["step"]), m=st["m"].detach().cpu().clone(), v=st["v"].detach().cpu().clone())
                if "stats" in st:
                    g["stats"] = st["stats"].detach().cpu().clone()
            groups.append(g)
        return dict(version=1, groups=groups)

    def import_state(self, d: dict) -> None:
        """Load what ``export_state()`` returned into this optimizer -- before or after its first ``step()``.  The number
        of groups and every group's element count must match (ValueError otherwise; nothing is changed then).  The chunk
        tables are rebuilt by the next step; tensors that accessors handed out (``skipped_steps()`` ...) stay valid."""
        groups = d.get("groups") if isinstance(d, dict) else None
        if groups is None or len(groups) != len(self.param_groups):
            raise ValueError(f"FusedAdam.import_state: {0 if groups is None else len(groups)} parameter groups saved, "
                             f"{len(self.param_groups)} here")
        for gi, (g, group) in enumerate(zip(groups, self.param_groups)):
            total = sum(p.numel() for p in group["params"])
            if int(g["numel"]) != total:
                raise ValueError(f"FusedAdam.import_state: group {gi} holds {total} elements, the saved state {g['numel']}")
            for k in ("m", "v"):
                if g[k] is not None and (g[k].numel() != total or g[k].dtype != torch.float32):
                    raise ValueError(f"FusedAdam.import_state: group {gi}: '{k}' must be {total} fp32 values")
            if (g["m"] is None) != (g["v"] is None):
                raise ValueError(f"FusedAdam.import_state: group {gi}: one moment without the other")
            if g["stats"] is not None and (g["stats"].numel() != 4 or g["stats"].dtype != torch.float64):
                raise ValueError(f"FusedAdam.import_state: group {gi}: 'stats' must be four doubles")
        for gi, (g, group) in enumerate(zip(groups, self.param_groups)):
            for k, val in g["hyper"].items():
                group[k] = tuple(val) if k == "betas" else val
            st = self._groups[gi]
            if g["m"] is None:                               # saved before the group's first step
                if st is not None:
                    st["m"].zero_()
                    st["v"].zero_()
                    st["step"] = 0
                    if "stats" in st:
                        st["stats"].zero_()
                continue
            params = list(group["params"])
            dev = params[0].device
            if st is None:
                offs, total = {}, 0
                for p in params:
                    offs[id(p)] = total
                    total += p.numel()
                # (sig None: the next step's _prepare builds the chunk table and keeps these buffers)
                st = self._groups[gi] = dict(m=torch.empty(total, device=dev), v=torch.empty(total, device=dev), step=0,
                                             offs=offs, total=total, sig=None, table=None, n_chunks=0)
            st["m"].copy_(g["m"])
            st["v"].copy_(g["v"])
            st["step"] = int(g["step"])
            if g["stats"] is not None:
                if "stats" not in st:
                    st["stats"] = torch.zeros(4, dtype=torch.float64, device=dev)
                st["stats"].copy_(g["stats"])
            elif "stats" in st:
                st["stats"].zero_()

    @torch.no_grad()
    def step(self, closure=None, ema=None, shard=None, max_grad_norm=None, skip_nonfinite=False, reduce_sumsq=None):
        """One step.  ``ema``: an ``ExponentialMovingAverage`` over exactly this optimizer's parameters (in
        order) whose shadow is updated in the same launch, with its own warm-up rule.  ``shard = (lo, hi)``: update
        only the elements [lo, hi) of the flat parameter order (one parameter group) -- the sharded data-parallel
        step, where this rank holds the reduced gradients of that range only.

        ``max_grad_norm``: clip the gradient to this global L2 norm by the rule of ``torch.nn.utils.clip_grad_norm_``
        (coefficient ``min(1, max_grad_norm / (norm + 1e-6))``), applied inside the step launch.  Unlike
        ``clip_grad_norm_`` the ``.grad`` tensors are NOT rescaled: they keep the unclipped values.  ``inf`` measures
        (and guards) without clipping, bit-equal to the plain step.  ``skip_nonfinite``: a step whose squared gradient
        norm is inf / NaN writes nothing -- parameters, both moments and the EMA shadow keep their bits -- and counts
        itself in ``skipped_steps()``; alone it means ``max_grad_norm=inf``.  With neither, the step is the plain
        ``beso_adam_step`` call.  ``reduce_sumsq``: called with the 1-element device view of the squared norm between
        the reduction and the step, to sum it in place across the ranks of a sharded exchange (each rank's table covers
        its shard only).  With several parameter groups the norm, the clipping and the guard are PER GROUP.
        Nothing here synchronises: ``last_grad_norm()``, ``last_clip_coef()`` and ``skipped_steps()`` are device views.

        Host counters on a skipped step: the host cannot know that the device skipped, so the bias-correction step count
        and the EMA warm-up counter (``ema.next_decay()``, ``ema.version``) advance as on any other step -- a decision,
        not an oversight: the alternative is the per-step host read this feature exists to avoid."""
        clipped = max_grad_norm is not None or skip_nonfinite
        if clipped:
            max_grad_norm = math.inf if max_grad_norm is None else float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError("max_grad_norm must be positive (inf: measure and guard without clipping)")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if shard is not None and len(self.param_groups) != 1:
            raise ValueError("a sharded step needs one parameter group")
        shard = None if shard is None else (int(shard[0]), int(shard[1]))
        prepared = [self._prepare(gi, group, shard) for gi, group in enumerate(self.param_groups)]   # validates devices/dtypes
        lib = _lib.load()
        ema_decay, ema_ptr = 0.0, None
        if ema is not None:
            if len(self.param_groups) != 1 or ema._flat.numel() != sum(p.numel() for p in self.param_groups[0]["params"]):
                raise ValueError("fused EMA needs one parameter group that matches the EMA helper")
            ema_decay = ema.next_decay()
            ema_ptr = ema._flat.data_ptr()
        stream = stream_ptr()
        for st, group in zip(prepared, self.param_groups):
            st["step"] += 1
            if clipped:
                # (an empty table -- a rank that owns nothing of a sharded exchange -- still contributes its 0 to the sum:
                # reduce_sumsq is a collective)
                partial, stats = self._clip_scratch(st)
                table = st["table"].data_ptr() if st["n_chunks"] else None
                _lib.check(lib.beso_grad_sumsq(table, st["n_chunks"], partial.data_ptr(), stats.data_ptr(), stream),
                           "beso_grad_sumsq")
                if reduce_sumsq is not None:
                    reduce_sumsq(stats[0:1])
            if st["n_chunks"] == 0:
                continue
            b1, b2 = group["betas"]
            if clipped:
                _lib.check(lib.beso_adam_step_clipped(
                    st["table"].data_ptr(), st["n_chunks"], st["m"].data_ptr(), st["v"].data_ptr(), ema_ptr,
                    float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                    1 if group["decoupled_weight_decay"] else 0, st["step"], float(ema_decay), stats.data_ptr(),
                    max_grad_norm, 1 if skip_nonfinite else 0, stream), "beso_adam_step_clipped")
                continue
            _lib.check(lib.beso_adam_step(st["table"].data_ptr(), st["n_chunks"], st["m"].data_ptr(), st["v"].data_ptr(),
                                          ema_ptr, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                          float(group["weight_decay"]), 1 if group["decoupled_weight_decay"] else 0,
                                          st["step"], float(ema_decay), stream), "beso_adam_step")
        # the kernel writes the parameters through raw pointers: bump their version counters so that everything keyed on
        # them (the packed-weight cache of DiffusionGPT, autograd's saved-tensor checks) sees the update
        torch.autograd.graph.increment_version([p for g in self.param_groups for p in g["params"] if p.grad is not None])
        if ema is not None:
            ema.version += 1
        return loss


def maybe_fuse(opt: torch.optim.Optimizer) -> torch.optim.Optimizer:
    """torch Adam / AdamW over HIP fp32 parameters with default flags -> FusedAdam; anything else unchanged."""
    if type(opt) not in (torch.optim.Adam, torch.optim.AdamW):
        return opt
    for g in opt.param_groups:
        if g.get("amsgrad") or g.get("maximize") or g.get("capturable") or g.get("differentiable"):
            return opt
        if type(opt) is torch.optim.Adam and g.get("decoupled_weight_decay"):
            return opt
        for p in g["params"]:
            if not p.is_cuda or p.dtype != torch.float32:
                return opt
    if any(len(s) for s in opt.state.values()):
        return opt                                             # already stepped: keep its state
    return FusedAdam.from_torch(opt)
