"""Training the critic behind ``select='value'``: ``CriticTrainer`` fits Q(s, a, g) (an ``MLPGuide``, guides.py) and V(s, g) (a
``StateValue``) by Implicit Q-Learning (Kostrikov et al. 2021), the critic of Implicit Diffusion Q-Learning with the diffusion
policy as the behaviour prior.  V is an expectile regression onto a slowly moving target copy of Q, Q a TD regression onto
``r + gamma (1 - done) V(s')``; no action outside the data set is ever evaluated.  The reference ships neither critic nor a way to
make one.

One ``train_step`` is ten enqueues and no torch-op evaluation of either network (include/beso_critic_fit.h, include/beso_mlp.h):

  1. ``beso_critic_rows``   Q rows ``[s_t | a_t | g]``, V rows ``[s_t | g]`` and behind them ``[s_{t+1} | g]`` -- no ``torch.cat``
  2. ``beso_mlp_fwd``       q, with the keep buffer
  3. ``beso_mlp_fwd``       q_target: Q's network on the target parameters
  4. ``beso_mlp_fwd``       v and v_next: V's network on the 2 M rows, with the keep buffer
  5. ``beso_critic_loss``   both weighted mean losses, each row's two losses, the advantage, dq and dv
  6. ``beso_mlp_bwd`` x 2   Q's gradients from dq; V's from ``[dv ; M zeros]``
  7. ``FusedAdam.step`` x 2 Q's launch also moves the target: ``target <- (1 - tau) target + tau q``

Nothing reads the device: both losses come back as 0-dim device tensors.  Equal inputs and state give equal bits."""
import torch
import torch.nn as nn

from .... import _lib
from ...._instantiate import instantiate
from ....networks.ema_helper.ema import ExponentialMovingAverage
from ....networks.mlps.mlps import MLPNetwork
from ....optim import FusedAdam
from .guides import MLPGuide, _stream


class StateValue(nn.Module):
    """A learned state value V(state, goal) as an ``MLPNetwork`` with ``output_dim == 1``: the V counterpart of ``MLPGuide``.

    The network's input row for sample b and step t is ``[state[b, t, :] | goal[b or 0, G-1, :]]``: the goal part only with
    ``use_goal`` and a goal, so ``input_dim = obs (+ obs)``; of a goal sequence the last step is read, and a goal given as
    ``[1, G, obs]`` is shared by all samples.  ``network``: a config (``_target_`` + kwargs), a factory or an instance."""

    def __init__(self, network, use_goal: bool = True):
        super().__init__()
        self.network = network if isinstance(network, nn.Module) else instantiate(network)
        self.use_goal = bool(use_goal)
        if not isinstance(self.network, MLPNetwork):
            raise TypeError(f"StateValue: network must be an MLPNetwork, got {type(self.network).__name__}")
        if self.network.output_dim != 1:
            raise ValueError(f"StateValue: the network's output_dim must be 1 (a scalar v per row), got {self.network.output_dim}")

    def _dims(self, state, goal):
        """(B, steps, obs, goal or None) of a call, refusing by name what the network cannot read."""
        if state.dim() != 3:
            raise ValueError(f"StateValue: state {tuple(state.shape)} must be [B, steps, obs]")
        B, S, obs = state.shape
        goal = goal if self.use_goal and goal is not None else None
        if goal is not None and (goal.dim() != 3 or goal.shape[2] != obs or goal.shape[0] not in (1, B)):
            raise ValueError(f"StateValue: goal {tuple(goal.shape)} must be [B or 1, G, obs={obs}]")
        want = obs + (obs if goal is not None else 0)
        if self.network.input_dim != want:
            raise ValueError(f"StateValue: the network's input_dim={self.network.input_dim}, but obs"
                             f"{' + obs' if goal is not None else ''} = {want} (use_goal={self.use_goal})")
        return B, S, obs, goal

    def forward(self, state, goal=None) -> torch.Tensor:
        """v [B, steps] through ``MLPNetwork.forward``."""
        B, S, obs, goal = self._dims(state, goal)
        parts = [state.to(torch.float32)]
        if goal is not None:
            parts.append(goal[:, -1:, :].to(torch.float32).expand(B, S, obs))
        return self.network(torch.cat(parts, dim=-1)).squeeze(-1)


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t).__name__


class CriticTrainer:
    """``CriticTrainer(q, v, gamma, expectile, tau, lr, betas, weight_decay, decoupled_weight_decay)``.

    ``q``: an ``MLPGuide`` without ``use_sigma``; ``v``: a ``StateValue``.  Both are on the GPU when the trainer is made: the
    target copy of Q is made there and then, from q.  The trainer owns one ``FusedAdam`` per network and that target
    (``q_target_params``: views of one flat buffer, in the order of ``q.network.layers.parameters()``).  The target moves inside
    Q's optimizer launch, by that launch's EMA arithmetic with the constant decay ``1 - tau``:
    ``target -= (1 - decay) * (target - q)`` on the updated q, in fp32.

    After a step: ``per_row_q`` / ``per_row_v`` [B, T] hold each row's loss, ``advantage`` [B, T] holds
    ``q_target(s, a) - v(s)`` (all on the device).  ``q`` is an ordinary ``MLPGuide`` before and after: hand it as ``guide=`` to
    ``VectorRollout.step(..., select='value')`` or ``BesoAgent.predict_best_of(..., select='value')``."""

    def __init__(self, q, v, gamma: float = 0.99, expectile: float = 0.7, tau: float = 0.005, lr: float = 3e-4,
                 betas=(0.9, 0.999), weight_decay: float = 0.0, decoupled_weight_decay: bool = False):
        if not isinstance(q, MLPGuide):
            raise TypeError(f"CriticTrainer: q must be an MLPGuide, got {type(q).__name__}")
        if not isinstance(v, StateValue):
            raise TypeError(f"CriticTrainer: v must be a StateValue, got {type(v).__name__}")
        if q.use_sigma:
            raise ValueError("CriticTrainer: q is a guide with use_sigma: a noise-level-aware critic has no fit step (the data "
                             "set's actions are clean)")
        if q.use_goal != v.use_goal:
            raise ValueError(f"CriticTrainer: q and v disagree on use_goal (q: {q.use_goal}, v: {v.use_goal})")
        if q.network.input_dim <= v.network.input_dim:
            raise ValueError(f"CriticTrainer: q and v disagree on obs_dim: q's input_dim={q.network.input_dim} must be v's "
                             f"input_dim={v.network.input_dim} plus the action's")
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"CriticTrainer: gamma={gamma} must lie in [0, 1]")
        if not 0.0 < expectile < 1.0:
            raise ValueError(f"CriticTrainer: expectile={expectile} must lie in (0, 1)")
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f"CriticTrainer: tau={tau} must lie in [0, 1]")
        self.q, self.v = q, v
        self.gamma, self.expectile, self.tau = float(gamma), float(expectile), float(tau)
        self.q_params = list(q.network.layers.parameters())
        self.v_params = list(v.network.layers.parameters())
        adam = dict(lr=lr, betas=betas, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay)
        self.q_optimizer = FusedAdam(self.q_params, **adam)
        self.v_optimizer = FusedAdam(self.v_params, **adam)
        # the Polyak target as the shadow of an EMA helper without its warm-up rule: next_decay() is 1 - tau at every step
        self.target = ExponentialMovingAverage(self.q_params, decay=1.0 - self.tau, use_num_updates=False)
        self.per_row_q = self.per_row_v = self.advantage = None         # [B, T] of the last step (device)
        self._flat = {}                 # 'q' / 'v' -> the flat gradient; every parameter's .grad is a view of it
        self._bufs = {}                 # M -> the step's buffers

    @property
    def q_target_params(self):
        return self.target.shadow_params

    # ------------------------------------------------------------------ buffers
    def _grads(self, which: str, dev):
        net, params = (self.q.network, self.q_params) if which == "q" else (self.v.network, self.v_params)
        flat = self._flat.get(which)
        if flat is None or flat.device != dev:
            flat = self._flat[which] = torch.empty(net.num_param_floats(), dtype=torch.float32, device=dev)
        off = 0
        for p in params:                    # (re-attached every step: zero_grad(set_to_none=True) elsewhere may have dropped them)
            view = flat[off:off + p.numel()].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                p.grad = view
            off += p.numel()
        return flat

    def _buffers(self, M: int, dev):
        hit = self._bufs.get(M)
        if hit is None or hit["q_rows"].device != dev:
            qn, vn = self.q.network, self.v.network
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)                  # noqa: E731
            u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)                       # noqa: E731
            hit = self._bufs[M] = dict(
                q_rows=f32(M, qn.input_dim), v_rows=f32(2 * M, vn.input_dim), q=f32(M, 1), q_target=f32(M, 1), v=f32(2 * M, 1),
                keep_q=f32(qn.keep_floats(M)), keep_v=f32(vn.keep_floats(2 * M)), dq=f32(M),
                dv=torch.zeros(2 * M, dtype=torch.float32, device=dev),        # [dv ; M zeros]: only the first M are ever written
                ws_q=u8(qn.workspace_bytes(M)), ws_v=u8(vn.workspace_bytes(2 * M)))
        return hit

    # ------------------------------------------------------------------ the step
    def _check(self, state, action, goal, reward, done, next_state, weight):
        """(B, T, obs, act, goal or None) of a step, refusing by name what it cannot take; touches nothing."""
        for name, t in (("state", state), ("action", action)):
            if not torch.is_tensor(t):
                raise ValueError(f"CriticTrainer: {name} must be a tensor, got {type(t).__name__}")
        B, T, obs, act, goal = self.q._dims(state, action, goal)
        want = obs + (obs if goal is not None else 0)
        if self.v.network.input_dim != want:
            raise ValueError(f"CriticTrainer: q and v disagree on obs_dim: v's input_dim={self.v.network.input_dim}, but obs"
                             f"{' + obs' if goal is not None else ''} = {want} by q's rows")
        for name, t in (("reward", reward), ("done", done), ("weight", weight)):
            if (t is None and name != "weight") or (t is not None and (not torch.is_tensor(t) or t.shape != (B, T))):
                raise ValueError(f"CriticTrainer: {name} must be [B={B}, T={T}], got {_shape(t)}")
        if next_state is None:
            if state.shape[1] < T + 1:
                raise ValueError(f"CriticTrainer: state has {state.shape[1]} steps, but next_state=None reads state[:, 1 : T + 1] "
                                 f"and needs T + 1 = {T + 1}")
        elif not torch.is_tensor(next_state) or next_state.shape != (B, T, obs):
            raise ValueError(f"CriticTrainer: next_state must be [B={B}, T={T}, obs={obs}], got {_shape(next_state)}")
        on_gpu = (state, action, reward, done, *(t for t in (goal, next_state, weight) if t is not None), *self.q_params,
                  *self.v_params, *self.q_target_params)
        if not all(t.is_cuda for t in on_gpu):
            raise RuntimeError("CriticTrainer runs on the GPU only (HIP kernels, no CPU or eager fallback): q, v, the target and "
                               "every tensor of a step must be on it")
        return B, T, obs, act, goal

    def train_step(self, state, action, goal, reward, done, next_state=None, weight=None):
        """One IQL critic step on ``state [B, S, obs]``, ``action [B, T, act]``, ``goal [B or 1, G, obs]`` or None, ``reward`` and
        ``done`` ``[B, T]`` (done: 0 / 1, or bool) and an optional ``weight [B, T]`` (both losses are weighted means; all-zero
        weights give losses 0 and no gradient).  ``next_state [B, T, obs]``: None takes ``state[:, 1 : T + 1]`` and needs
        ``S >= T + 1`` -- a ``DeviceTrajectoryFeed`` window of W states with its first ``W - 1`` actions serves it directly.
        -> ``(loss_q, loss_v)`` before the update, 0-dim device tensors."""
        B, T, obs, act, goal = self._check(state, action, goal, reward, done, next_state, weight)
        dev = action.device
        f32c = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
        state, action, goal, reward, done, next_state, weight = (f32c(t) for t in (state, action, goal, reward, done, next_state, weight))
        ptr = lambda t: None if t is None else t.data_ptr()                                      # noqa: E731

        M = B * T
        b = self._buffers(M, dev)
        flat_q, flat_v = self._grads("q", dev), self._grads("v", dev)
        loss_q, loss_v = (torch.empty((), dtype=torch.float32, device=dev) for _ in range(2))
        self.per_row_q, self.per_row_v, self.advantage = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(3))
        qn, vn = self.q.network, self.v.network
        lib = _lib.load_critic()
        with torch.cuda.device(dev):
            stream = _stream(action)
            _lib.check_critic(lib.beso_critic_rows(
                state.data_ptr(), ptr(next_state), action.data_ptr(), ptr(goal), B, T, state.shape[1],
                0 if goal is None else goal.shape[1], 0 if goal is None else goal.shape[0], obs, act, b["q_rows"].data_ptr(),
                b["v_rows"].data_ptr(), stream), "critic_rows")
            qn.run_forward(b["q_rows"], keep=True, params=self.q_params, out=b["q"], keep_out=b["keep_q"])
            qn.run_forward(b["q_rows"], keep=False, params=self.q_target_params, out=b["q_target"])
            vn.run_forward(b["v_rows"], keep=True, params=self.v_params, out=b["v"], keep_out=b["keep_v"])
            _lib.check_critic(lib.beso_critic_loss(
                b["q"].data_ptr(), b["q_target"].data_ptr(), b["v"].data_ptr(), b["v"].data_ptr() + 4 * M, reward.data_ptr(),
                done.data_ptr(), ptr(weight), M, self.gamma, self.expectile, loss_q.data_ptr(), loss_v.data_ptr(),
                self.per_row_q.data_ptr(), self.per_row_v.data_ptr(), b["dq"].data_ptr(), b["dv"].data_ptr(),
                self.advantage.data_ptr(), stream), "critic_loss")
            qn.run_backward(b["keep_q"], b["dq"], flat_q, params=self.q_params, workspace=b["ws_q"])
            vn.run_backward(b["keep_v"], b["dv"], flat_v, params=self.v_params, workspace=b["ws_v"])
            self.q_optimizer.step(ema=self.target)
            self.v_optimizer.step()
        return loss_q, loss_v

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        """Both networks, the target and both optimizers' moments and step counts (``FusedAdam.export_state``), as CPU tensors:
        loaded into a trainer around equally shaped networks, the next step's bits are those of the uninterrupted run."""
        cpu = lambda sd: {k: t.detach().cpu().clone() for k, t in sd.items()}                  # noqa: E731
        return dict(version=1, gamma=self.gamma, expectile=self.expectile, tau=self.tau,
                    q=cpu(self.q.network.state_dict()), v=cpu(self.v.network.state_dict()),
                    q_target=[t.detach().cpu().clone() for t in self.target.state_dict()["shadow_params"]],
                    q_optimizer=self.q_optimizer.export_state(), v_optimizer=self.v_optimizer.export_state())

    def load_state_dict(self, d: dict) -> None:
        for name in ("gamma", "expectile", "tau"):
            if d.get(name) != getattr(self, name):
                raise ValueError(f"CriticTrainer.load_state_dict: saved with {name}={d.get(name)!r}, this trainer has "
                                 f"{name}={getattr(self, name)!r}")
        if [t.shape for t in d["q_target"]] != [t.shape for t in self.q_target_params]:
            raise ValueError(f"CriticTrainer.load_state_dict: the saved target's shapes {[tuple(t.shape) for t in d['q_target']]} "
                             f"are not this trainer's {[tuple(t.shape) for t in self.q_target_params]}")
        self.q.network.load_state_dict(d["q"])                         # in place: the parameters keep their storage
        self.v.network.load_state_dict(d["v"])
        # (in place as well: the shadow stays the flat buffer Q's optimizer launch updates; the decay stays constant)
        self.target.load_state_dict(dict(decay=1.0 - self.tau, num_updates=None, shadow_params=d["q_target"]))
        self.q_optimizer.import_state(d["q_optimizer"])
        self.v_optimizer.import_state(d["v_optimizer"])
