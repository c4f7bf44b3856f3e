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
from .fit_common import FitNet, check_bt, f32c, goal_args, ptr, require_gpu, row_dims, shape_of
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
        B, S, obs, _, goal = row_dims("StateValue", self.network.input_dim, state, None, goal, self.use_goal)
        return B, S, obs, goal

    def forward(self, state, goal=None) -> torch.Tensor:
        """v [B, steps] through ``MLPNetwork.forward``."""
        B, S, obs, goal = self._dims(state, goal)
        parts = [state.to(torch.float32)]
        if goal is not None:
            parts.append(goal[:, -1:, :].to(torch.float32).expand(B, S, obs))
        return self.network(torch.cat(parts, dim=-1)).squeeze(-1)


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
        adam = dict(lr=lr, betas=betas, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay)
        self._q, self._v = FitNet(q.network, adam), FitNet(v.network, adam)          # Q over M rows, V over 2 M
        self.q_params, self.q_optimizer = self._q.params, self._q.optimizer
        self.v_params, self.v_optimizer = self._v.params, self._v.optimizer
        # the Polyak target as the shadow of an EMA helper without its warm-up rule: next_decay() is 1 - tau at every step
        self.target = ExponentialMovingAverage(self.q_params, decay=1.0 - self.tau, use_num_updates=False)
        self.per_row_q = self.per_row_v = self.advantage = None         # [B, T] of the last step (device)

    @property
    def q_target_params(self):
        return self.target.shadow_params

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
        check_bt("CriticTrainer", B, T, (("reward", reward), ("done", done), ("weight", weight)), required=("reward", "done"))
        if next_state is None:
            if state.shape[1] < T + 1:
                raise ValueError(f"CriticTrainer: state has {state.shape[1]} steps, but next_state=None reads state[:, 1 : T + 1] "
                                 f"and needs T + 1 = {T + 1}")
        elif not torch.is_tensor(next_state) or next_state.shape != (B, T, obs):
            raise ValueError(f"CriticTrainer: next_state must be [B={B}, T={T}, obs={obs}], got {shape_of(next_state)}")
        require_gpu("CriticTrainer", "q, v, the target", (state, action, reward, done, *(t for t in (goal, next_state, weight) if t is not None),
                                                           *self.q_params, *self.v_params, *self.q_target_params))
        return B, T, obs, act, goal

    def train_step(self, state, action, goal, reward, done, next_state=None, weight=None):
        """One IQL critic step on ``state [B, S, obs]``, ``action [B, T, act]``, ``goal [B or 1, G, obs]`` or None, ``reward`` and
        ``done`` ``[B, T]`` (done: 0 / 1, or bool) and an optional ``weight [B, T]`` (both losses are weighted means; all-zero
        weights give losses 0 and no gradient).  ``next_state [B, T, obs]``: None takes ``state[:, 1 : T + 1]`` and needs
        ``S >= T + 1`` -- a ``DeviceTrajectoryFeed`` window of W states with its first ``W - 1`` actions serves it directly.
        -> ``(loss_q, loss_v)`` before the update, 0-dim device tensors."""
        B, T, obs, act, goal = self._check(state, action, goal, reward, done, next_state, weight)
        dev = action.device
        state, action, goal, reward, done, next_state, weight = (f32c(t, dev) for t in (state, action, goal, reward, done, next_state, weight))
        goal_steps, goal_rows = goal_args(goal)

        M = B * T
        fq, fv = self._q, self._v
        bq = fq.buffers(M, dev, spare_out=True)                       # (the spare out: q_target)
        bv = fv.buffers(2 * M, dev, zero_d_out=True)                  # [dv ; M zeros]: only the first M are ever written
        flat_q, flat_v = fq.grads(dev), fv.grads(dev)
        (q_rows, q, _, dq, _, q_target), (v_rows, v, _, dv, _) = bq, bv
        loss_q, loss_v = (torch.empty((), dtype=torch.float32, device=dev) for _ in range(2))
        self.per_row_q, self.per_row_v, self.advantage = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(3))
        lib = _lib.load_critic()
        with torch.cuda.device(dev):
            stream = _stream(action)
            _lib.check_critic(lib.beso_critic_rows(
                state.data_ptr(), ptr(next_state), action.data_ptr(), ptr(goal), B, T, state.shape[1], goal_steps, goal_rows, obs, act,
                q_rows.data_ptr(), v_rows.data_ptr(), stream), "critic_rows")
            fq.forward(bq)
            fq.forward(bq, params=self.q_target_params, keep=False, out=q_target)
            fv.forward(bv)
            _lib.check_critic(lib.beso_critic_loss(
                q.data_ptr(), q_target.data_ptr(), v.data_ptr(), v.data_ptr() + 4 * M, reward.data_ptr(),
                done.data_ptr(), ptr(weight), M, self.gamma, self.expectile, loss_q.data_ptr(), loss_v.data_ptr(),
                self.per_row_q.data_ptr(), self.per_row_v.data_ptr(), dq.data_ptr(), dv.data_ptr(),
                self.advantage.data_ptr(), stream), "critic_loss")
            fq.backward(bq, flat_q)
            fv.backward(bv, flat_v)
            self.q_optimizer.step(ema=self.target)
            self.v_optimizer.step()
        return loss_q, loss_v

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self) -> dict:
        """Both networks, the target and both optimizers' moments and step counts (``FusedAdam.export_state``), as CPU tensors:
        loaded into a trainer around equally shaped networks, the next step's bits are those of the uninterrupted run."""
        (q, q_optimizer), (v, v_optimizer) = self._q.export(), self._v.export()
        return dict(version=1, gamma=self.gamma, expectile=self.expectile, tau=self.tau, q=q, v=v,
                    q_target=[t.detach().cpu().clone() for t in self.target.state_dict()["shadow_params"]],
                    q_optimizer=q_optimizer, v_optimizer=v_optimizer)

    def load_state_dict(self, d: dict) -> None:
        for name in ("gamma", "expectile", "tau"):
            if d.get(name) != getattr(self, name):
                raise ValueError(f"CriticTrainer.load_state_dict: saved with {name}={d.get(name)!r}, this trainer has "
                                 f"{name}={getattr(self, name)!r}")
        if [t.shape for t in d["q_target"]] != [t.shape for t in self.q_target_params]:
            raise ValueError(f"CriticTrainer.load_state_dict: the saved target's shapes {[tuple(t.shape) for t in d['q_target']]} "
                             f"are not this trainer's {[tuple(t.shape) for t in self.q_target_params]}")
        self._q.load(d["q"], d["q_optimizer"])
        self._v.load(d["v"], d["v_optimizer"])
        # (in place as well: the shadow stays the flat buffer Q's optimizer launch updates; the decay stays constant)
        self.target.load_state_dict(dict(decay=1.0 - self.tau, num_updates=None, shadow_params=d["q_target"]))
