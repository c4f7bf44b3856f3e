"""Best-of-K action selection in the rollout: ``VectorRollout.step(candidates=K)`` and ``BesoAgent.predict_best_of`` on the
TINY model.  The yardsticks are the existing paths -- ``step`` without candidates, ``predict``, ``sample_loop`` on a torch-op
expansion -- and the sequential float32 mean of tests/test_candidate_selection.py; everything is compared bit for bit."""
import types

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from support import bits, build_agent, make_denoiser
from beso_amd.networks.scaler.scaler_class import Scaler
from beso_amd.rollout import VectorRollout
from test_candidate_selection import sequential_mean

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _agent(cfg, device=DEV, **extra):
    """test_rollout.py's agent: seeded weights, the EMA shadow equal to them, an fp32 scaler."""
    w = O.make_weights(cfg, seed=3, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32" if device == DEV else None, device=device), device=device,
                        sampler="ddim", **extra)
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    rng = np.random.default_rng(7)
    sc = Scaler(rng.standard_normal((64, cfg.obs_dim)).astype(np.float32) * 2 + 0.5,
                rng.standard_normal((64, cfg.act_dim)).astype(np.float32) * 1.5 - 0.25, True, device)
    agent.get_scaler(sc)
    agent.set_bounds(sc)
    return agent


class _Feed:
    """Seeded raw observations [N, obs] and x_T draws [N, K, act] per step, raw goals [N, G, obs]."""

    def __init__(self, cfg, n_envs, K, seed):
        self.cfg, self.n, self.K, self.g = cfg, n_envs, K, torch.Generator(DEV).manual_seed(seed)
        self.goal = torch.randn((n_envs, cfg.goal_seq_len, cfg.obs_dim), device=DEV, generator=self.g)

    def __call__(self):
        return (torch.randn((self.n, self.cfg.obs_dim), device=DEV, generator=self.g) * 2 + 0.5,
                torch.randn((self.n, self.K, self.cfg.act_dim), device=DEV, generator=self.g))


def _pair(agent, N, goal):
    a, b = agent.vector_rollout(N), agent.vector_rollout(N)
    a.set_goal(goal)
    b.set_goal(goal)
    return a, b


def _same_state(a, b):
    return torch.equal(a.lengths, b.lengths) and torch.equal(bits(a.obs_ctx), bits(b.obs_ctx)) and torch.equal(bits(a.act_ctx), bits(b.act_ctx))


# ------------------------------------------------------------------------------------------------ no GPU
def test_bad_best_of_arguments_raise_value_error():
    """A bad ``select``, ``candidates < 1`` and a wrong ``noise`` shape raise ValueError from ``step`` and from
    ``predict_best_of`` before either touches a device or a context."""
    cfg = O.TINY
    roll = VectorRollout.__new__(VectorRollout)        # (the constructor needs the GPU; the checks in front of the step do not)
    roll.agent, roll.device, roll.n_envs, roll.window = types.SimpleNamespace(use_kde=False), torch.device("cpu"), 3, cfg.obs_seq_len
    roll.obs_dim, roll.act_dim = cfg.obs_dim, cfg.act_dim
    obs = torch.zeros(3, cfg.obs_dim)
    for bad in (dict(candidates=0), dict(candidates=-2), dict(candidates=2.0), dict(candidates=True), dict(candidates=257),
                dict(candidates=2, select="median"), dict(candidates=2, bandwidth=0.0), dict(candidates=2, bandwidth=float("nan")),
                dict(candidates=2, noise=torch.zeros(3, 1, cfg.act_dim)), dict(candidates=2, noise=torch.zeros(3, 2, cfg.act_dim + 1)),
                dict(select="kde"), dict(bandwidth=0.5)):
        with pytest.raises(ValueError):
            roll.step(obs, **bad)
    agent = _agent(cfg, device="cpu")
    batch = {"observation": torch.zeros(2, cfg.obs_dim), "goal_observation": torch.zeros(cfg.goal_seq_len, cfg.obs_dim)}
    for bad in (dict(k=0), dict(k=-1), dict(k=1.5), dict(k=2, select="mode"), dict(k=2, bandwidth=-1.0),
                dict(k=2, noise=torch.zeros(2, 1, cfg.act_dim)), dict(k=2, noise=torch.zeros(3, 2, cfg.act_dim))):
        with pytest.raises(ValueError):
            agent.predict_best_of(batch, **bad)
    assert len(agent.obs_context) == 0 and len(agent.action_context) == 0


# ------------------------------------------------------------------------------------------------ GPU
@gpu
def test_one_candidate_is_the_plain_step_bit_for_bit():
    """N = 3, 5 steps, environment 1 reset before step 3: ``step(obs, candidates=1, noise=z[:, None, 0])`` returns the bits of
    ``step(obs, noise=z)`` on a twin, and lengths, obs_ctx and act_ctx stay equal; 'kde' with one candidate too."""
    cfg, N = O.TINY, 3
    agent = _agent(cfg)
    feed = _Feed(cfg, N, 1, seed=13)
    for select in ("mean", "kde"):
        plain, best = _pair(agent, N, feed.goal)
        for step in range(5):
            if step == 3:
                plain.reset([1])
                best.reset([1])
            obs, z = feed()
            a = plain.step(obs, noise=z)
            b = best.step(obs, candidates=1, select=select, noise=z[:, None, 0])
            assert torch.equal(bits(a), bits(b)), (select, step)
            assert _same_state(plain, best), (select, step)
            assert torch.equal(bits(plain.last["x0"]), bits(best.last["x0"]))
            assert best.last["index"].tolist() == ([-1] * N if select == "mean" else [0] * N)
    W = cfg.obs_seq_len
    assert plain.lengths.tolist() == [min(5, W), min(2, W), min(5, W)]


@gpu
def test_mean_and_kde_against_an_independent_sampler_call():
    """N = 3, K = 4, 5 steps, environment 2 reset before step 2.  Every step: ONE independent ``sample_loop`` on the torch-op
    expansion of ``last['state']`` / ``last['x']`` (repeat_interleave + an indexed write of noise * sigma_max) gives the rows
    the step sampled (equal bits: the same batch, hence the same kernels); their newest slots are ``last['candidates']``;
    'mean' acts on their sequential float32 mean, 'kde' on ``candidates[n, index[n]]`` -- clipped and un-scaled by the
    scaler's own methods -- and ``act_ctx`` remembers the clipped selected action."""
    cfg, N, K = O.TINY, 3, 4
    W = cfg.obs_seq_len
    agent = _agent(cfg)
    sc = agent.scaler
    rows = torch.arange(N, device=DEV)
    for select in ("mean", "kde"):
        feed = _Feed(cfg, N, K, seed=17)
        roll = agent.vector_rollout(N)
        roll.set_goal(feed.goal)
        for step in range(5):
            if step == 2:
                roll.reset([2])
            obs, z = feed()
            got = roll.step(obs, candidates=K, select=select, noise=z)
            last = roll.last
            slot = (last["lengths"] - 1).long()
            state_k = torch.repeat_interleave(last["state"], K, dim=0)
            x_k = torch.repeat_interleave(last["x"], K, dim=0)
            x_k[torch.arange(N * K, device=DEV), torch.repeat_interleave(slot, K)] = (z * agent.sigma_max).reshape(N * K, -1)
            assert torch.equal(bits(last["x_k"]), bits(x_k)) and torch.equal(bits(last["state_k"]), bits(state_k))
            with torch.no_grad(), agent._ema_scope():
                x0_k = agent.sample_loop(agent.get_noise_schedule(agent.num_sampling_steps, agent.noise_scheduler), x_k, state_k,
                                         torch.repeat_interleave(roll.goal, K, dim=0), agent.sampler_type)
            cand = x0_k.view(N, K, W, cfg.act_dim)[rows, :, slot]
            assert tuple(last["candidates"].shape) == (N, K, cfg.act_dim)
            assert torch.equal(bits(last["candidates"]), bits(cand)), (select, step)
            if select == "mean":
                chosen = torch.stack([torch.from_numpy(sequential_mean(c)) for c in cand.cpu().numpy()]).to(DEV)
                assert last["index"].tolist() == [-1] * N
                # the other slots are candidate 0's
                want = x0_k.view(N, K, W, cfg.act_dim)[:, 0].clone()
                want[rows, slot] = chosen
                assert torch.equal(bits(last["x0"]), bits(want)), step
            else:
                idx = last["index"].long()
                assert bool(((idx >= 0) & (idx < K)).all())
                chosen = cand[rows, idx]
                assert torch.equal(bits(last["x0"]), bits(x0_k.view(N, K, W, cfg.act_dim)[rows, idx])), step
                assert torch.equal(last["scores"].argmax(dim=1), idx) and bool((last["scores"] >= 0).all())
            clipped = sc.clip_action(chosen)
            assert torch.equal(bits(got), bits(sc.inverse_scale_output(clipped))), (select, step)
            assert torch.equal(bits(roll.act_ctx[rows, slot]), bits(clipped)), (select, step)
        assert roll.lengths.tolist() == [min(5, W), min(5, W), min(3, W)]


@gpu
def test_default_select_follows_use_kde_and_nothing_leaks_into_plain_steps():
    """``select=None`` is 'kde' on an agent built with ``use_kde``, else 'mean'.  A rollout that took candidate steps and a twin
    fed the same executed history agree on the next plain step bit for bit: the candidate step leaves nothing behind but the
    contexts."""
    cfg, N, K = O.TINY, 3, 4
    for use_kde in (False, True):
        agent = _agent(cfg, use_kde=use_kde)
        feed = _Feed(cfg, N, K, seed=19)
        roll, twin = _pair(agent, N, feed.goal)
        for step in range(3):
            obs, z = feed()
            a = roll.step(obs, candidates=K, noise=z)
            assert (roll.last["index"] >= 0).all() if use_kde else roll.last["index"].tolist() == [-1] * N
            b = twin.step(obs, candidates=K, select="kde" if use_kde else "mean", noise=z)
            assert torch.equal(bits(a), bits(b))
        # the twin that never used candidates: a fresh rollout given the same contexts
        fresh = agent.vector_rollout(N)
        fresh.set_goal(feed.goal)
        fresh.lengths.copy_(roll.lengths)
        fresh.obs_ctx.copy_(roll.obs_ctx)
        fresh.act_ctx.copy_(roll.act_ctx)
        fresh._reset.zero_()
        fresh._reset_pending = False
        obs, z = feed()
        a, b = roll.step(obs, noise=z[:, :1]), fresh.step(obs, noise=z[:, :1])
        assert torch.equal(bits(a), bits(b)) and _same_state(roll, fresh)
        assert "candidates" not in roll.last and "index" not in roll.last


@gpu
def test_predict_best_of_one_is_predict_and_eight_grows_the_contexts():
    """``predict_best_of(batch, 1)`` equals ``predict`` on a twin agent under the same RNG draw bit for bit over 4 steps (shape
    included); k = 8 runs 'mean' and 'kde' with the observation window and ``action_context`` growing as in ``predict``."""
    cfg, B = O.TINY, 2
    W = cfg.obs_seq_len
    a1, a2 = _agent(cfg), _agent(cfg)
    g = torch.Generator(DEV).manual_seed(23)
    goal = torch.randn((cfg.goal_seq_len, cfg.obs_dim), device=DEV, generator=g)
    for step in range(4):
        batch = {"observation": torch.randn((B, cfg.obs_dim), device=DEV, generator=g), "goal_observation": goal}
        torch.manual_seed(100 + step)
        want = a1.predict(batch)
        torch.manual_seed(100 + step)
        got = a2.predict_best_of(batch, 1)
        assert got.shape == want.shape and torch.equal(bits(got), bits(want)), step
        assert len(a1.action_context) == len(a2.action_context) and len(a1.obs_context) == len(a2.obs_context)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(a1.action_context, a2.action_context))
    for select in ("mean", "kde"):
        agent = _agent(cfg)
        for step in range(W + 1):
            batch = {"observation": torch.randn((B, cfg.obs_dim), device=DEV, generator=g), "goal_observation": goal}
            z = torch.randn((B, 8, cfg.act_dim), device=DEV, generator=g)
            pred = agent.predict_best_of(batch, 8, select=select, noise=z)
            assert pred.reshape(B, cfg.act_dim).isfinite().all()
            assert len(agent.obs_context) == min(step + 1, W) and len(agent.action_context) == min(step + 1, W - 1)
            info = agent.last_best_of
            assert tuple(info["candidates"].shape) == (B, 8, cfg.act_dim) and tuple(info["scores"].shape) == (B, 8)
            newest = agent.action_context[-1].reshape(B, cfg.act_dim)
            if select == "kde":
                chosen = info["candidates"][torch.arange(B, device=DEV), info["index"].long()]
            else:
                chosen = torch.stack([torch.from_numpy(sequential_mean(c)) for c in info["candidates"].cpu().numpy()]).to(DEV)
            assert torch.equal(bits(newest), bits(agent.scaler.clip_action(chosen))), (select, step)
            assert torch.equal(bits(pred.reshape(B, -1)), bits(agent.scaler.inverse_scale_output(newest)))


@gpu
def test_predict_best_of_accepts_an_mlp_encoder_agent():
    """An agent with a trainable MLPEncoder may use ``predict_best_of`` (``_encode_eval`` runs in front, as in ``predict``),
    while ``vector_rollout`` keeps refusing it."""
    from test_encoder_agent import RAW, make_agent
    cfg, B = O.TINY, 2
    agent = make_agent(DEV)
    g = torch.Generator(DEV).manual_seed(29)
    goal = torch.randn((cfg.goal_seq_len, RAW), device=DEV, generator=g)
    for step in range(3):
        batch = {"observation": torch.randn((B, RAW), device=DEV, generator=g), "goal_observation": goal}
        pred = agent.predict_best_of(batch, 4, select="kde")
        assert pred.reshape(B, cfg.act_dim).isfinite().all() and len(agent.action_context) == min(step + 1, cfg.obs_seq_len - 1)
        assert bool(((agent.last_best_of["index"] >= 0) & (agent.last_best_of["index"] < 4)).all())
    with pytest.raises(NotImplementedError, match="vector_rollout"):
        agent.vector_rollout(2)
