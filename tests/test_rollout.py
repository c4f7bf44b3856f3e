"""The vectorised rollout (beso_amd/rollout.py, csrc/rollout.hip): N environments per sampler call, windows of different
lengths run as full windows with zero padding behind the valid slots.

The argument checks of the two entry points need no GPU.  The GPU tests hold ``VectorRollout`` against the existing paths: the
reference's recorded ``predict`` trace, one batched ``sample_loop`` call on windows the test stacks itself (bit for bit once
every window is full), and the per-environment UNPADDED ``sample_loop`` call on the test's own deques (to the parity
tolerances of tests/test_gpu_parity.py: padded and unpadded calls run different shapes, hence different kernels)."""
import ctypes as C
import dataclasses
from collections import deque

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import load_golden, weights_from_fixture, rel_err
from support import build_agent, count_site_launches, lib, make_denoiser  # noqa: F401
from beso_amd import _lib
from beso_amd.networks.scaler.scaler_class import Scaler

gpu = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ no GPU
def test_rollout_argument_errors_do_not_touch_the_device(lib):
    """beso_rollout_begin / beso_rollout_end reject NULL required pointers, a statistics pair with one half missing, a window,
    obs_dim or act_dim below one and a negative n_envs before anything is enqueued (status -3); n_envs == 0 is a no-op."""
    one = C.c_void_p(0x1000)
    begin = lambda **k: lib.beso_rollout_begin(*[k.get(n, d) for n, d in (          # noqa: E731
        ("obs", one), ("reset", one), ("noise", one), ("mean", one), ("den", one), ("sigma_max", 1.0), ("lengths", one),
        ("obs_ctx", one), ("act_ctx", one), ("state_out", one), ("x_out", one), ("n_envs", 4), ("window", 3), ("obs_dim", 7),
        ("act_dim", 3), ("stream", None))])
    end = lambda **k: lib.beso_rollout_end(*[k.get(n, d) for n, d in (              # noqa: E731
        ("x0", one), ("lengths", one), ("lo", one), ("hi", one), ("den_y", one), ("mean_y", one), ("act_ctx", one),
        ("pred", one), ("n_envs", 4), ("window", 3), ("act_dim", 3), ("stream", None))])
    assert begin(n_envs=0) == 0
    assert begin(n_envs=0, reset=None, mean=None, den=None) == 0
    for bad in (dict(obs=None), dict(noise=None), dict(lengths=None), dict(obs_ctx=None), dict(act_ctx=None),
                dict(state_out=None), dict(x_out=None), dict(mean=None), dict(den=None), dict(window=0), dict(window=-2),
                dict(obs_dim=0), dict(act_dim=0), dict(n_envs=-1), dict(n_envs=0, window=0), dict(n_envs=0, obs=None),
                dict(n_envs=1 << 20, window=1 << 10, obs_dim=1 << 10)):
        assert begin(**bad) == -3, bad
    assert end(n_envs=0) == 0
    assert end(n_envs=0, den_y=None, mean_y=None) == 0
    for bad in (dict(x0=None), dict(lengths=None), dict(lo=None), dict(hi=None), dict(act_ctx=None), dict(pred=None),
                dict(den_y=None), dict(mean_y=None), dict(window=0), dict(act_dim=0), dict(act_dim=-1), dict(n_envs=-1),
                dict(n_envs=0, window=0), dict(n_envs=0, pred=None)):
        assert end(**bad) == -3, bad
    with pytest.raises(ValueError):
        _lib.check(begin(window=0), "rollout_begin")


def test_vector_rollout_has_no_cpu_path():
    """A model on the CPU raises when the rollout is made: there is no CPU path and no fallback to ``predict``."""
    cfg = dataclasses.replace(O.TINY, linear_output=False)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, precision=None, device="cpu", train=True))
    with pytest.raises(RuntimeError, match="no CPU path"):
        agent.vector_rollout(4)


# ------------------------------------------------------------------------------------------------ GPU
def _agent(cfg, precision="fp32", sampler="ddim"):
    """An agent around the HIP module of `cfg` with seeded weights, the EMA shadow equal to them, and an fp32 scaler."""
    w = O.make_weights(cfg, seed=3, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, precision), device=DEV, sampler=sampler)
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    rng = np.random.default_rng(7)
    sc = Scaler(rng.standard_normal((64, cfg.obs_dim)).astype(np.float32) * 2 + 0.5,
                rng.standard_normal((64, cfg.act_dim)).astype(np.float32) * 1.5 - 0.25, True, DEV)
    agent.get_scaler(sc)
    agent.set_bounds(sc)
    return agent


class _Feed:
    """Seeded raw observations [N, obs], x_T draws [N, 1, act] per step and raw goals [N, G, obs]."""

    def __init__(self, cfg, n_envs, seed):
        self.cfg, self.n, self.g = cfg, n_envs, torch.Generator(DEV).manual_seed(seed)
        self.goal = torch.randn((n_envs, cfg.goal_seq_len, cfg.obs_dim), device=DEV, generator=self.g)

    def __call__(self):
        return (torch.randn((self.n, self.cfg.obs_dim), device=DEV, generator=self.g) * 2 + 0.5,
                torch.randn((self.n, 1, self.cfg.act_dim), device=DEV, generator=self.g))


class _RefEnv:
    """The reference's rollout state for ONE environment (beso_agent.py:96-100): the two deques, and predict's step on them
    through the existing path -- sample_loop on the unpadded [1, t, .] window, clip_action, inverse_scale_output."""

    def __init__(self, agent, goal):
        W = agent.window_size
        self.agent, self.goal = agent, agent.scaler.scale_input(goal).unsqueeze(0)
        self.obs, self.act = deque(maxlen=W), deque(maxlen=W - 1)

    def reset(self):
        self.obs.clear()
        self.act.clear()

    def inputs(self, obs, noise):
        """Appends the observation; the sampler's inputs (state [1, t, obs], x [1, t, act]) as predict builds them."""
        self.obs.append(self.agent.scaler.scale_input(obs.reshape(1, -1)))
        x = noise.reshape(1, 1, -1) * self.agent.sigma_max
        if len(self.act) > 0:
            x = torch.cat((*self.act, x), dim=1)
        return torch.stack(tuple(self.obs), dim=1), x

    def step(self, obs, noise, sampler, n_steps):
        agent = self.agent
        state, x = self.inputs(obs, noise)
        with torch.no_grad(), agent._ema_scope():
            x0 = agent.sample_loop(agent.get_noise_schedule(n_steps, "exponential"), x, state, self.goal, sampler)
        a = agent.scaler.clip_action(x0[:, -1, :])
        self.act.append(a.unsqueeze(1))
        return agent.scaler.inverse_scale_output(a)[0]


def _staggered(agent, cfg, n_envs, n_steps_total, sampler, n_steps, tol, tag):
    """Environment k is reset at steps k and k + W + 2 (and, like every environment, starts empty): every action and every
    length of the rollout against the per-environment unpadded calls."""
    W = cfg.obs_seq_len
    feed = _Feed(cfg, n_envs, seed=21)
    roll = agent.vector_rollout(n_envs)
    roll.set_goal(feed.goal)
    refs = [_RefEnv(agent, feed.goal[k]) for k in range(n_envs)]
    rows = torch.arange(n_envs, device=DEV)
    worst, inside, total = 0.0, 0, 0
    for step in range(n_steps_total):
        who = [k for k in range(n_envs) if step in (k, k + W + 2)]
        if who:
            roll.reset(who)
            for k in who:
                refs[k].reset()
        obs, noise = feed()
        got = roll.step(obs, new_sampler_type=sampler, new_sampling_steps=n_steps, noise=noise)
        want = torch.stack([refs[k].step(obs[k], noise[k], sampler, n_steps) for k in range(n_envs)])
        assert tuple(got.shape) == (n_envs, cfg.act_dim)
        assert roll.last["lengths"].tolist() == [len(r.obs) for r in refs], step
        err = rel_err(got.cpu().numpy(), want.cpu().numpy())
        worst = max(worst, err)
        assert err < tol, (tag, step, err)
        raw = roll.last["x0"][rows, (roll.last["lengths"] - 1).long()]
        inside += int((agent.scaler.clip_action(raw) == raw).sum())
        total += raw.numel()
    print(f"[rollout] {tag}: worst relative difference to the unpadded per-environment calls {worst:.3e} (bound {tol:.0e}); "
          f"{inside} of {total} action components inside the clip bounds")
    assert 2 * inside > total, "the comparison is degenerate: most actions sit on the clip bounds"
    return worst


@gpu
def test_vector_rollout_replays_the_reference_trace():
    """N = 1 on tests/golden/tiny_agent_trace.npz with the fixture's draws injected: the reference's own predictions, within
    the bound test_agent_predict_trace_on_gpu holds predict to.  Its first W - 1 calls are short windows, run padded here."""
    fx = load_golden("tiny_agent_trace.npz")
    cfg = O.TINY
    w = weights_from_fixture(fx)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32"), device=DEV)
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    agent.get_scaler(Scaler(fx["x_data"], fx["y_data"], True, DEV))
    agent.set_bounds(agent.scaler)
    roll = agent.vector_rollout(1)
    roll.set_goal(torch.from_numpy(fx["goal"].copy()))
    assert int(fx["n_calls"]) > cfg.obs_seq_len
    for c in range(int(fx["n_calls"])):
        pred = roll.step(torch.from_numpy(fx[f"call{c}::obs"].copy()), new_sampler_type="ddim", new_sampling_steps=3,
                         noise_scheduler="exponential", noise=torch.from_numpy(fx[f"call{c}::noise"].copy()))
        assert tuple(pred.shape) == (1, cfg.act_dim)                       # always [N, act]: no [1, 1, act] first call
        err = rel_err(pred.cpu().numpy().reshape(fx[f"call{c}::pred"].shape), fx[f"call{c}::pred"])
        print(f"[rollout] tiny_agent_trace call {c}: {err:.3e}")
        assert err < 5e-5, (c, err)
        assert roll.last["lengths"].tolist() == [min(c + 1, cfg.obs_seq_len)]
    assert agent._ema_packed is not None, "the EMA packed image must have been used"


@gpu
def test_synchronous_environments_equal_the_batched_call_bit_for_bit():
    """N = 7 environments reset together, per-environment goals, 2W + 1 steps.  From the step at which every window is full
    the test's own deques stack into one [N, W, .] sample_loop call -- the same batch and shape, hence the same kernels -- and
    the rollout's inputs and actions equal that call's bit for bit, through the in-place shift of the full windows too."""
    cfg = O.TINY
    W, N = cfg.obs_seq_len, 7
    agent = _agent(cfg)
    sc = agent.scaler
    feed = _Feed(cfg, N, seed=5)
    roll = agent.vector_rollout(N)
    roll.set_goal(feed.goal)
    goal = sc.scale_input(feed.goal)
    assert torch.equal(roll.goal, goal)
    refs = [_RefEnv(agent, feed.goal[k]) for k in range(N)]
    rows = torch.arange(N, device=DEV)
    compared = 0
    for step in range(2 * W + 1):
        obs, noise = feed()
        got = roll.step(obs, noise=noise)
        t = min(step + 1, W)
        assert roll.last["lengths"].tolist() == [t] * N
        ins = [refs[k].inputs(obs[k], noise[k]) for k in range(N)]
        state, x = torch.cat([i[0] for i in ins]), torch.cat([i[1] for i in ins])
        # (short windows: the valid slots are the deques' bits, the rest is zero)
        assert torch.equal(roll.last["state"][:, :t], state) and torch.equal(roll.last["x"][:, :t], x), step
        assert not roll.last["state"][:, t:].any() and not roll.last["x"][:, t:].any(), step
        if t < W:
            a = sc.clip_action(roll.last["x0"][rows, t - 1])
        else:
            with torch.no_grad(), agent._ema_scope():
                x0 = agent.sample_loop(agent.get_noise_schedule(agent.num_sampling_steps, "exponential"), x, state, goal,
                                       agent.sampler_type)
            a = sc.clip_action(x0[:, -1, :])
            assert torch.equal(roll.last["x0"], x0), step
            assert torch.equal(got, sc.inverse_scale_output(a)), step
            compared += 1
        for k in range(N):
            refs[k].act.append(a[k].reshape(1, 1, -1))
    assert compared == W + 2


@gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_staggered_resets_match_the_unpadded_per_environment_calls(precision):
    """N = 5 for 3W steps, environment k reset at steps k and k + W + 2: windows of every length side by side in one call."""
    from test_gpu_parity import TOL
    cfg = O.TINY
    _staggered(_agent(cfg, precision), cfg, 5, 3 * cfg.obs_seq_len, "ddim", 3, TOL[precision], f"tiny {precision} ddim-3")


@gpu
def test_nothing_survives_a_reset():
    """A rollout that ran W + 2 steps and is then reset behaves as a fresh one: fed the same observations and draws from
    there on, the two return equal bits -- the stale context and the stale slots behind the window are dead."""
    cfg = O.TINY
    W, N = cfg.obs_seq_len, 3
    agent = _agent(cfg)
    feed = _Feed(cfg, N, seed=9)
    used, fresh = agent.vector_rollout(N), agent.vector_rollout(N)
    for r in (used, fresh):
        r.set_goal(feed.goal)
    for _ in range(W + 2):
        obs, noise = feed()
        used.step(obs * 3.0, noise=noise)
    used.reset()
    for step in range(W + 2):
        obs, noise = feed()
        a, b = used.step(obs, noise=noise), fresh.step(obs, noise=noise)
        assert torch.equal(a, b), step
        assert torch.equal(used.last["state"], fresh.last["state"]) and torch.equal(used.last["x"], fresh.last["x"]), step
        assert torch.equal(used.lengths, fresh.lengths)


@gpu
def test_environments_do_not_see_each_other():
    """Two runs at the same N that differ in environment j's observations and resets only: every other environment's actions
    are equal bit for bit, and j's are not."""
    cfg = O.TINY
    W, N, j = cfg.obs_seq_len, 6, 2
    agent = _agent(cfg)
    others = [k for k in range(N) if k != j]
    runs = []
    for variant in (0, 1):
        feed = _Feed(cfg, N, seed=13)
        roll = agent.vector_rollout(N)
        roll.set_goal(feed.goal)
        acts = []
        for step in range(2 * W + 2):
            obs, noise = feed()
            if step == W + 1:
                roll.reset([0, N - 1])                     # both runs: partial resets beside untouched environments
            if variant:
                obs[j] = obs[j] * -1.5 + 0.3
                if step in (1, W, W + 2):
                    roll.reset([j])
            acts.append(roll.step(obs, noise=noise))
        runs.append(torch.stack(acts))
    assert torch.equal(runs[0][:, others], runs[1][:, others])
    assert not torch.equal(runs[0][:, j], runs[1][:, j])


@gpu
def test_tail_is_the_scalers_clip_and_inverse_scale_bit_for_bit():
    """pred = inverse_scale_output(clip_action(x0[n, t_n - 1])) and the remembered row is the clipped one, with y-bounds
    tightened (x 0.05) so that the clip acts; then the same for the scalers the launch does not serve (float64 statistics:
    the scaler's own methods; scale_data off: no statistics)."""
    cfg = O.TINY
    W, N = cfg.obs_seq_len, 6
    agent = _agent(cfg)
    rng = np.random.default_rng(11)
    x64, y64 = rng.standard_normal((64, cfg.obs_dim)) * 2 + 0.5, rng.standard_normal((64, cfg.act_dim)) * 1.5
    scalers = {"fp32": agent.scaler, "float64": Scaler(x64, y64, True, DEV),
               "unscaled": Scaler(x64.astype(np.float32), y64.astype(np.float32), False, DEV)}
    rows = torch.arange(N, device=DEV)
    for name, sc in scalers.items():
        sc.y_bounds_tensor = sc.y_bounds_tensor * 0.05
        agent.get_scaler(sc)
        feed = _Feed(cfg, N, seed=17)
        roll = agent.vector_rollout(N)
        roll.set_goal(feed.goal)
        n_clipped = n_kept = 0
        ragged = False
        for step in range(W + 2):
            if step == 2:
                roll.reset([1, 4])                         # lengths differ from here on
            obs, noise = feed()
            pred = roll.step(obs, noise=noise)
            slot = (roll.last["lengths"] - 1).long()
            raw = roll.last["x0"][rows, slot]
            clipped = sc.clip_action(raw)
            assert pred.dtype == torch.float32 or name == "float64"
            assert torch.equal(pred, sc.inverse_scale_output(clipped)), (name, step)
            assert torch.equal(roll.act_ctx[rows, slot], clipped), (name, step)
            assert torch.equal(roll.last["state"][rows, slot], sc.scale_input(obs).to(torch.float32)), (name, step)
            n_clipped += int((clipped != raw).sum())
            n_kept += int((clipped == raw).sum())
            ragged = ragged or len(set(roll.lengths.tolist())) > 1
        assert ragged
        assert n_clipped > 0, f"{name}: the tightened bounds clipped nothing"
        print(f"[rollout] tail {name}: {n_clipped} components clipped, {n_kept} inside the bounds")
    assert scalers["fp32"].x_mean.dtype == torch.float32 and scalers["float64"].x_mean.dtype == torch.float64


@gpu
def test_kitchen_bf16_staggered_rollout_runs_the_one_launch_sampler():
    """KITCHEN shape, bf16, N = 8 with staggered resets, DDIM-3 and Heun against the unpadded per-environment calls; with the
    one-launch kernel asked for, a whole rollout step launches it once."""
    from beso_amd.runtime import set_plan
    from test_gpu_parity import TOL
    cfg = O.KITCHEN
    agent = _agent(cfg, "bf16")
    set_plan(forward=_lib.PLAN_FUSED)
    try:
        for sampler in ("ddim", "heun"):
            _staggered(agent, cfg, 8, 3 * cfg.obs_seq_len, sampler, 3, TOL["bf16"], f"kitchen bf16 {sampler}-3")
        feed = _Feed(cfg, 8, seed=2)
        roll = agent.vector_rollout(8)
        roll.set_goal(feed.goal)
        for sampler in ("ddim", "heun"):
            obs, noise = feed()
            out = {}
            n = count_site_launches("fused_layer", lambda: out.__setitem__("a", roll.step(
                obs, new_sampler_type=sampler, new_sampling_steps=3, noise=noise)))
            assert n == 1, (sampler, n)
            assert torch.isfinite(out["a"]).all()
    finally:
        set_plan(forward=0)
