"""Vectorised rollout inference: ONE sampler call per environment step for N environments whose episodes start and end
independently (``gym.vector``, a pool of simulator processes) -- what ``BesoAgent.predict`` (reference beso_agent.py:296-388)
does for one set of environments that are reset together.

The observation / action windows live on the device as ``[N, W, .]`` contexts with a length per environment.  Every step runs
``beso_rollout_begin`` (append the observation, write the sampler's inputs), the agent's ``sample_loop`` and
``beso_rollout_end`` (take the newest action, clip, remember, un-scale): three launches beside the sampler's.  An environment
with ``t < W`` observations is run as a full ``W``-slot window whose unused slots are zero: attention is causal and positions
belong to slots, so the tokens of the ``t`` valid slots never see the padding, and the padded action slots evolve on their own
through a sampler loop without anything reading them.  No denoiser or sampler kernel knows about ragged windows.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import _lib
from . import candidates as best_of

# What ``_scaler_plan`` hands the launch behind the sampler: ``kind`` names the entry point (_TAIL_ENTRY), ``lo`` / ``hi`` are
# clip_action's float64 bounds, ``stats`` the fp32 statistics in the entry point's argument order -- (den_y, mean_y) for 'zscore',
# (new_lo, span, range, lo_y) for 'minmax' -- or as many None with ``scale_data`` off.
_Tail = namedtuple("_Tail", "kind lo hi stats")
# kind -> (library, entry point): the package's Scaler and its MinMaxScaler (include/beso_scale.h)
_TAIL_ENTRY = {"zscore": ("hip", "beso_rollout_end"), "minmax": ("scale", "beso_rollout_end_minmax")}
# A step's checked arguments (``VectorRollout._arguments``).  ``K`` is None without candidates; ``sigmas`` is the host-side schedule
# of the sampler settings; ``slabs`` counts the step-noise slabs a seeded step draws (0: none).
_StepArgs = namedtuple("_StepArgs", "obs K select bandwidth sampler_type sigmas slabs guide", defaults=(None,))


def _ptr(v):
    return None if v is None else v.data_ptr()


class _Last(dict):
    """``VectorRollout.last``.  ``candidates`` [N, K, act] -- the newest-slot actions of the N K sampled rows ``x0_k`` -- is an
    audit value no step needs: it is gathered on first access (small launches the step does not pay), from the live
    ``lengths``, so ask for it before the next step."""

    def __missing__(self, key):
        if key != "candidates" or "x0_k" not in self:
            raise KeyError(key)
        x0_k, lengths = self["x0_k"], self["lengths"]
        N = lengths.numel()
        rows = torch.arange(N, device=x0_k.device)
        self[key] = x0_k.view(N, -1, *x0_k.shape[1:])[rows, :, (lengths - 1).long()]
        return self[key]


class VectorRollout:
    """``agent.vector_rollout(n_envs)``.  ``step(obs)`` returns the actions ``[N, act]`` of one environment step; ``reset`` /
    ``set_goal`` act on all environments or on the listed ones.  The rollout reads the agent's scaler, sampler settings and
    EMA weights at every step, so whatever ``predict`` would pick up it picks up.  GPU only: there is no CPU path.

    ``lengths`` [N] int32, ``obs_ctx`` [N, W, obs] and ``act_ctx`` [N, W, act] are the device-resident state (slots at or
    behind an environment's length are dead); ``last`` holds the latest step's ``state`` / ``x`` (the sampler's inputs),
    ``x0`` (its result; with ``candidates`` the selected windows) and ``lengths`` (the live tensor), for audit.

    ``seed(seeds)`` turns keyed noise on (beso_amd/noise.py, include/beso_noise.h): every draw of an environment -- its x_T, its
    K candidates, an ancestral sampler's step noise -- then depends on the environment's seed, episode and step alone, not on
    ``n_envs``, its row or the global generator, and comes from ONE launch in front of the step's.  ``last`` gains
    ``noise_episode`` / ``noise_step`` [N] int32, the counters the step used (read them before the step after next)."""

    _keyed = None        # the KeyedNoise of a seeded rollout (seed / unseed)

    def __init__(self, agent, n_envs: int):
        n_envs = int(n_envs)
        if n_envs < 1:
            raise ValueError("n_envs must be at least 1")
        den = agent._hip_denoiser()
        if den is None:
            raise RuntimeError("beso_amd: the vectorised rollout needs the HIP denoiser (GCDenoiser around DiffusionGPT)")
        first = next(iter(agent.model.parameters()), None)
        if first is None or not first.is_cuda:
            raise RuntimeError("beso_amd: the vectorised rollout runs on the GPU only (no CPU path); move the model to the MI355X")
        shape = den.inner_model.shape(den.sigma_data)
        self.agent = agent
        self.lib = _lib.load()
        self.device = first.device
        self.n_envs = n_envs
        self.window = max(1, int(agent.window_size))
        if self.window > shape.obs_seq_len:
            raise ValueError(f"window_size {self.window} exceeds the model's obs_seq_len {shape.obs_seq_len}")
        self.obs_dim, self.act_dim, self.goal_len = shape.obs_dim, shape.act_dim, shape.goal_seq_len
        dev, N, W = self.device, n_envs, self.window
        self.lengths = torch.zeros(N, dtype=torch.int32, device=dev)
        self.obs_ctx = torch.zeros((N, W, self.obs_dim), dtype=torch.float32, device=dev)
        self.act_ctx = torch.zeros((N, W, self.act_dim), dtype=torch.float32, device=dev)
        self.goal = None
        self.last = {}
        self._reset = torch.ones(N, dtype=torch.uint8, device=dev)
        self._reset_pending = True
        self._rows = torch.arange(N, device=dev)
        self._plan_key = None
        self._plan = None

    # ------------------------------------------------------------------ episode control
    def _ids(self, env_ids):
        ids = torch.as_tensor(env_ids, dtype=torch.long).reshape(-1)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.n_envs):
            raise IndexError(f"environment ids must be in [0, {self.n_envs})")
        return ids.to(self.device)

    def reset(self, env_ids=None) -> None:
        """Mark environments (default: all) for reset: their windows start empty at their next step."""
        if env_ids is None:
            self._reset.fill_(1)
        else:
            self._reset.index_fill_(0, self._ids(env_ids), 1)
        self._reset_pending = True
        if self._keyed is not None:
            self._keyed.mark_reset(None if env_ids is None else self._ids(env_ids))

    # ------------------------------------------------------------------ keyed noise
    def seed(self, seeds, env_ids=None) -> None:
        """Turn keyed noise on.  ``seeds``: an int (environment i takes ``seeds + i`` modulo 2^64) or one int in [0, 2^64) per
        listed environment (default: all).  The listed environments start at noise episode 0, and their step counter restarts
        with their next step; every ``reset`` of an environment then begins its next episode.  Their windows are not touched.
        The first call seeds all environments; later calls may re-seed some.  Equal seeds give equal draws: distinct
        environments want distinct seeds."""
        from .noise import KeyedNoise, check_seeds
        if env_ids is None:
            self._keyed = KeyedNoise(check_seeds(seeds, list(range(self.n_envs))), self.device)
            return
        ids = self._ids(env_ids).tolist()
        if self._keyed is None:
            raise ValueError("seed(): the first call seeds every environment (env_ids=None); later calls may re-seed some")
        self._keyed.set_seeds(seeds, ids)

    def unseed(self) -> None:
        """Back to the global generator: ``noise=None`` draws ``torch.randn`` again, as a rollout that was never seeded."""
        self._keyed = None

    # what a seeded step can serve: the samplers whose one-enqueue path takes its step noise as an argument, and the ones that
    # draw nothing that enters their result (agent.sample_loop's names)
    _KEYED_STEP_SAMPLERS = ("euler_ancestral", "ancestral", "dpmpp_2s_ancestral")
    _DETERMINISTIC_SAMPLERS = ("ddim", "euler", "heun", "dpm", "dpmpp_2m", "dpmpp_2s", "lms", "dpm_fast", "dpm_adaptive")

    def _keyed_step_slabs(self, sampler_type, sigmas, rows: int) -> int:
        """How many slabs of step noise the sampler call of a seeded step takes (0: a deterministic sampler), or ValueError for a
        sampler that would draw from the global generator inside a Python loop.  Decided before anything is enqueued."""
        from .agents.diffusion_agents.k_diffusion import gc_sampling as ks
        from .agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierGuidedSampleModel
        if sampler_type in self._DETERMINISTIC_SAMPLERS:
            return 0
        if sampler_type not in self._KEYED_STEP_SAMPLERS:
            raise ValueError(f"seeded rollout: sampler {sampler_type!r} draws its noise from the global generator inside a Python "
                             f"loop, which keyed noise does not serve (no silent unkeyed draws); keyed step noise serves "
                             f"{self._KEYED_STEP_SAMPLERS}, and {self._DETERMINISTIC_SAMPLERS} need none")
        agent, dev = self.agent, self.device
        m = agent.model
        if m.training:
            m.eval()
        if isinstance(m, ClassifierGuidedSampleModel) and m.cond_lambda == 0:
            m = m.model                                          # (as sample_loop)
        probe = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # noqa: E731  (shapes only: nothing reads them)
        goal = None if self.goal is None else probe(rows, *self.goal.shape[1:])
        if ks._fused_call(m, probe(rows, self.window, self.obs_dim), probe(rows, self.window, self.act_dim), goal, sigmas,
                          None, {}, None) is None:
            raise ValueError(f"seeded rollout: sampler {sampler_type!r} is forced off its one-launch path here (the model, its "
                             "precision or shape, or the schedule), where it would draw its step noise from the global "
                             "generator inside a Python loop (no silent unkeyed draws)")
        return len(sigmas) - 1

    @torch.no_grad()
    def set_goal(self, goal, env_ids=None) -> None:
        """Raw goals: ``[G, obs]`` for the listed environments (default: all of them), or one per environment as
        ``[N, G, obs]`` (``[len(env_ids), G, obs]``).  Scaled once, as ``predict`` scales its goal, and kept on the device."""
        agent = self.agent
        goal = agent.scaler.scale_input(torch.as_tensor(goal)).to(device=self.device, dtype=torch.float32)
        if goal.shape[-1] == 10:                                           # base_agent.py:119-120, as process_batch
            keep = torch.ones(10, dtype=torch.bool, device=self.device)
            keep[[2, 5, 6, 7, 8, 9]] = False
            goal = torch.where(keep, goal, 0.0)
        if goal.dim() not in (2, 3) or goal.shape[-1] != self.obs_dim or (self.goal_len and goal.shape[-2] != self.goal_len):
            raise ValueError(f"goal must be [{self.goal_len}, {self.obs_dim}] or [n, {self.goal_len}, {self.obs_dim}], "
                             f"got {tuple(goal.shape)}")
        if self.goal is None:
            self.goal = torch.zeros((self.n_envs,) + tuple(goal.shape[-2:]), dtype=torch.float32, device=self.device)
        if env_ids is None:
            if goal.dim() == 3 and goal.shape[0] != self.n_envs:
                raise ValueError(f"expected {self.n_envs} goals, got {goal.shape[0]}")
            self.goal.copy_(goal if goal.dim() == 3 else goal.unsqueeze(0).expand_as(self.goal))
        else:
            ids = self._ids(env_ids)
            if goal.dim() == 3 and goal.shape[0] != ids.numel():
                raise ValueError(f"expected {ids.numel()} goals, got {goal.shape[0]}")
            self.goal[ids] = goal

    # ------------------------------------------------------------------ what of the scaler the two launches can take over
    def _scaler_plan(self):
        """(x statistics for beso_rollout_begin or None, the _Tail of the launch behind the sampler or None), rebuilt when the
        scaler, one of its tensors or a tensor's version changes.  The tail is 'zscore' for the package's Scaler and 'minmax' for
        its MinMaxScaler (whose scale_input is Scaler's arithmetic: the same begin launch serves it).  The launches take fp32
        statistics and float64 bounds of the package's two scalers; anything else is served by the scaler's own methods."""
        from .networks.scaler.scaler_class import MinMaxScaler, Scaler
        sc = self.agent.scaler
        parts = tuple(getattr(sc, k, None) for k in ("x_mean", "x_std", "y_mean", "y_std", "y_bounds_tensor", "y_min", "y_max",
                                                     "new_min_y", "new_max_y"))
        key = (sc, getattr(sc, "scale_data", None)) + tuple((p, getattr(p, "_version", None)) for p in parts)
        old = self._plan_key
        if old is not None and len(old) == len(key) and all(
                (a[0] is b[0] and a[1] == b[1]) if isinstance(a, tuple) else (a is b) for a, b in zip(old, key)):
            return self._plan
        dev = self.device
        f32 = lambda v, n: (isinstance(v, torch.Tensor) and v.device == dev and v.dtype == torch.float32     # noqa: E731
                            and v.dim() == 1 and v.numel() == n and v.is_contiguous())
        ours = isinstance(sc, Scaler) and all(getattr(type(sc), m) is getattr(Scaler, m)
                                              for m in ("scale_input", "clip_action", "inverse_scale_output", "_den"))
        minmax = isinstance(sc, MinMaxScaler) and all(getattr(type(sc), m) is getattr(MinMaxScaler, m) for m in (
            "scale_input", "clip_action", "inverse_scale_output", "_den", "_y_range", "_y_span"))
        xs = ys = None
        if (ours or minmax) and sc.scale_data and not (self.obs_dim == 7 and len(sc.x_mean) == 30):
            mean, den = sc.x_mean, sc._den("x") if ours else sc._den()
            if f32(mean, self.obs_dim) and f32(den, self.obs_dim):
                xs = (mean, den)
        b = parts[4]
        if (ours or minmax) and isinstance(b, torch.Tensor) and b.device == dev and b.dtype == torch.float64 and tuple(b.shape) == (2, self.act_dim):
            lo, hi = (b[0] * 1.1).contiguous(), (b[1] * 1.1).contiguous()        # clip_action's bounds, in float64
            kind = "minmax" if minmax else "zscore"
            if not sc.scale_data:
                ys = _Tail(kind, lo, hi, (None,) * (4 if minmax else 2))
            else:
                stats = (sc.new_min_y, sc._y_span(), sc._y_range(), sc.y_min) if minmax else (sc._den("y"), sc.y_mean)
                if all(f32(s, self.act_dim) for s in stats):
                    ys = _Tail(kind, lo, hi, stats)
        self._plan_key, self._plan = key, (xs, ys)
        return self._plan

    # ------------------------------------------------------------------ one environment step
    @torch.no_grad()
    def step(self, obs, new_sampler_type=None, new_sampling_steps=None, noise_scheduler=None, noise=None, candidates=None,
             select=None, bandwidth=None, guide=None) -> torch.Tensor:
        """Raw observations ``[N, obs]`` (device or host) -> actions ``[N, act]``.  ``noise`` ``[N, 1, act]`` is the x_T draw
        of the newest action; None draws ``torch.randn((N, 1, act), device=...)``, the draw ``predict`` makes.

        ``candidates=K`` draws K actions per environment in ONE sampler call on N K rows and acts on one action per
        environment (beso_amd/candidates.py, include/beso_select.h): ``select='mean'`` on the candidates' sample mean,
        ``'kde'`` on the candidate of the highest kernel density among its siblings (``bandwidth=None``: Scott's rule); the
        default is 'kde' with ``agent.use_kde``, else 'mean'.  ``noise`` is then ``[N, K, act]``.  Two launches more than a
        plain step.  Clip, un-scale and the remembered context take the selected action only; ``last`` gains ``candidates``
        ``[N, K, act]`` (the newest-slot actions before the clip), ``scores`` ``[N, K]`` and ``index`` ``[N]``, and the
        sampler call's ``state_k`` / ``x_k`` / ``x0_k`` on N K rows.

        ``select='value', guide=g``: the candidate the ``MLPGuide`` g scores highest -- q of ``[newest observation | candidate's
        newest action | goal]`` as the sampler sees them (scaled) -- in ONE launch behind the sampler (include/beso_rank.h);
        ``scores`` are then the q values.  Every sampler works: nothing is differentiated.  g (without ``use_sigma``, on the
        model's device) may be the ``cond_func`` of the agent's ``ClassifierGuidedSampleModel`` as well.

        Seeded (``seed``): ``noise=None`` is the keyed draw -- x_T, the K candidates and the step noise of 'euler_ancestral',
        'ancestral' and 'dpmpp_2s_ancestral' on their one-launch path, all from one launch -- and a sampler that would draw
        from the global generator inside a Python loop is a ValueError.  An explicit ``noise`` still wins."""
        a = self._arguments(obs, noise, new_sampler_type, new_sampling_steps, noise_scheduler, candidates, select, bandwidth, guide)
        xs, ys = self._scaler_plan()
        noise, noise_k, step_noise = self._draws(a, noise)
        state, x = self._begin(a.obs, noise, xs)
        x0, picked = self._sample(a, state, x, noise_k, step_noise)
        pred = self._end(x0, ys)
        if self._keyed is not None:
            picked.update(noise_episode=self._keyed.episodes, noise_step=self._keyed.steps)
            if step_noise is not None:
                picked["step_noise"] = step_noise
        self.last = _Last({"state": state, "x": x, "lengths": self.lengths, "x0": x0, **picked})
        return pred

    def _arguments(self, obs, noise, new_sampler_type, new_sampling_steps, noise_scheduler, candidates, select, bandwidth,
                   guide=None):
        """Phase 1: every refusal of a step -- the best-of-K arguments and the guide of ``select='value'``, the shapes of ``obs``
        and of an explicit ``noise``, the goal, the schedule, what a seeded step can serve (_keyed_step_slabs) -- as a ValueError
        (a guide of the wrong type: TypeError), and the sampler settings resolved.  Touches no device state and enqueues nothing:
        after a refusal no window, counter or reset flag has changed."""
        agent, N = self.agent, self.n_envs
        K = None
        if candidates is not None:
            K, select, bandwidth = best_of.check_arguments(candidates, select, bandwidth, bool(getattr(agent, "use_kde", False)))
            max_act = _lib.SELECT_LIMITS["max_act"]
            if self.act_dim > max_act:
                raise ValueError(f"candidates: act_dim {self.act_dim} exceeds the {max_act} components the selection takes")
            guide = best_of.check_guide(select, guide, self.obs_dim, self.act_dim, getattr(self, "goal", None) is not None,
                                        self.device, "VectorRollout.step")
        elif select is not None or bandwidth is not None or guide is not None:
            raise ValueError("select, bandwidth and guide belong to candidates=K")
        if noise is not None and tuple(torch.as_tensor(noise).shape) != (N, K or 1, self.act_dim):
            raise ValueError(f"noise must be [{N}, {K or 1}, {self.act_dim}], got {tuple(torch.as_tensor(noise).shape)}")
        if self.goal_len and self.goal is None:
            raise ValueError("set_goal() must be called before the first step of a goal-conditioned model")
        obs = torch.as_tensor(obs)
        if tuple(obs.shape) != (N, self.obs_dim):
            raise ValueError(f"obs must be [{N}, {self.obs_dim}], got {tuple(obs.shape)}")
        sampler_type = agent.sampler_type if new_sampler_type is None else new_sampler_type
        n_steps = agent.num_sampling_steps if new_sampling_steps is None else new_sampling_steps
        sigmas = agent.get_noise_schedule(n_steps, agent.noise_scheduler if noise_scheduler is None else noise_scheduler)
        slabs = 0 if self._keyed is None else self._keyed_step_slabs(sampler_type, sigmas, N * (K or 1))
        return _StepArgs(obs, K, select, bandwidth, sampler_type, sigmas, slabs, guide)

    def _draws(self, a, noise):
        """Phase 2, the one place that says where a step's draws come from -> (noise [N, 1, act] for begin's newest slot, noise_k
        [N, K, act] or None, step_noise [slabs, N K, W, act] or None).  An explicit ``noise`` wins; without one a seeded rollout
        takes every draw from its ONE keyed launch (include/beso_noise.h) and an unseeded one makes its one global-generator
        draw.  A seeded step runs the keyed launch in either case: its counters advance, and its step noise is keyed."""
        N, W, K, keyed, given = self.n_envs, self.window, a.K, self._keyed, noise is not None
        rows = K or 1
        noise_k = step_noise = None
        if given:
            noise = torch.as_tensor(noise).to(device=self.device, dtype=torch.float32).contiguous()
        elif keyed is None:
            noise = torch.randn((N, rows, self.act_dim), device=self.device)
        if K is not None and noise is not None:
            noise_k, noise = noise, noise[:, :1].contiguous()            # begin's newest slot: expand overwrites it in every row
        if keyed is not None:
            x_t, cand, step_noise = keyed.rollout(self.act_dim, 0 if K is None or given else K, a.slabs, rows * W * self.act_dim)
            if not given:
                noise, noise_k = x_t, cand
            if step_noise is not None:
                step_noise = step_noise.view(a.slabs, N * rows, W, self.act_dim)
        return noise, noise_k, step_noise

    def _begin(self, obs, noise, xs):
        """Phase 3: beso_rollout_begin -- the marked environments start empty, the observation joins every window, the sampler's
        inputs (state [N, W, obs], x [N, W, act]) are written -- then the reset flags are cleared."""
        agent, dev, N, W = self.agent, self.device, self.n_envs, self.window
        if xs is None:                                           # a scaler the launch cannot serve: its own method
            obs = agent.scaler.scale_input(obs)
            if tuple(obs.shape) != (N, self.obs_dim):
                raise RuntimeError(f"the scaler returned {tuple(obs.shape)}, expected {(N, self.obs_dim)}")
        obs = obs.to(device=dev, dtype=torch.float32).contiguous()
        mean, den = xs or (None, None)
        state = torch.empty((N, W, self.obs_dim), dtype=torch.float32, device=dev)
        x = torch.empty((N, W, self.act_dim), dtype=torch.float32, device=dev)
        _lib.launch("hip", "beso_rollout_begin", dev, obs.data_ptr(), self._reset.data_ptr() if self._reset_pending else None,
                    noise.data_ptr(), _ptr(mean), _ptr(den), float(agent.sigma_max), self.lengths.data_ptr(),
                    self.obs_ctx.data_ptr(), self.act_ctx.data_ptr(), state.data_ptr(), x.data_ptr(), N, W, self.obs_dim, self.act_dim)
        if self._reset_pending:
            self._reset.zero_()
            self._reset_pending = False
        return state, x

    def _sample(self, a, state, x, noise_k, step_noise):
        """Phase 4: ONE sampler call on the EMA weights in eval mode -> (x0 [N, W, act], the best-of-K entries of ``last``).
        With candidates the N windows are expanded to N K rows in front of it and the selection picks N of them behind it
        ('value': the ranking, which reads the un-expanded state and goal); a seeded step hands its keyed step noise to the
        sampler (gc_sampling.keyed_step_noise)."""
        agent, N, W, K = self.agent, self.n_envs, self.window, a.K
        state_n = state
        with agent._ema_scope():
            if agent.model.training:
                agent.model.eval()
            goal = self.goal
            if K is not None:                                    # from here on N K rows
                state, x = best_of.expand(state, x, self.lengths, noise_k, agent.sigma_max)
                goal = None if goal is None else torch.repeat_interleave(goal, K, dim=0)
            if self._keyed is None:
                x0 = agent.sample_loop(a.sigmas, x, state, goal, a.sampler_type)
            else:
                from .agents.diffusion_agents.k_diffusion.gc_sampling import keyed_step_noise
                with keyed_step_noise(step_noise):
                    x0 = agent.sample_loop(a.sigmas, x, state, goal, a.sampler_type)
        if x0.dtype != torch.float32 or not x0.is_contiguous():
            x0 = x0.to(torch.float32).contiguous()
        if tuple(x0.shape) != (N * (K or 1), W, self.act_dim):
            raise RuntimeError(f"the sampler returned {tuple(x0.shape)}, expected {(N * (K or 1), W, self.act_dim)}")
        if K is None:
            return x0, {}
        x0_k = x0
        if a.select == best_of.VALUE:
            x0, index, scores = best_of.rank(state_n, self.goal, x0_k, self.lengths, K, a.guide)
        else:
            x0, index, scores = best_of.select(x0_k, self.lengths, K, a.select, a.bandwidth)
        return x0, {"scores": scores, "index": index, "state_k": state, "x_k": x, "x0_k": x0_k}

    def _end(self, x0, ys):
        """Phase 5: the newest action of every window is clipped, remembered in ``act_ctx`` and un-scaled -> pred [N, act].  One
        launch (_TAIL_ENTRY) where the plan has a tail; else the scaler's own methods on the gathered rows."""
        if ys is None:                                           # (other dtypes, another class)
            scaler, slot = self.agent.scaler, (self.lengths - 1).long()
            clipped = scaler.clip_action(x0[self._rows, slot])
            self.act_ctx[self._rows, slot] = clipped
            return scaler.inverse_scale_output(clipped)
        pred = torch.empty((self.n_envs, self.act_dim), dtype=torch.float32, device=self.device)
        _lib.launch(*_TAIL_ENTRY[ys.kind], self.device, x0.data_ptr(), self.lengths.data_ptr(), ys.lo.data_ptr(), ys.hi.data_ptr(),
                    *[_ptr(s) for s in ys.stats], self.act_ctx.data_ptr(), pred.data_ptr(), self.n_envs, self.window,
                    self.act_dim)
        return pred
