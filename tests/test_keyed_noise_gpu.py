"""The rollout's keyed noise on the MI355X (include/beso_noise.h, csrc/noise.hip, beso_amd/noise.py, VectorRollout.seed) against
the numpy restatement of tests/test_keyed_noise.py: the words bit for bit, the normals to a measured bound, their moments, and
the point of the feature -- what an environment draws does not depend on its neighbours."""
import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import rel_err
from support import bits, lib  # noqa: F401
from test_gpu_parity import TOL
from test_keyed_noise import keyed_normals, keyed_words, normals_from_words
from test_rollout import _agent

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KEYS = [11, (7 << 32) | 5, 0xFFFFFFFFFFFFFFFF]       # one below 2^32, one at or above it, the largest
EPISODES, STEPS = [0, 3, 0x0FFFFFFF], [5, 0, 0xFFFFFFFF]
# |GPU fp32 normal - float64 evaluation of the same expression from the same words| over 2^16 values (MOMENT_KEY, purpose x_t):
# measured 8.44e-07 on the first MI355X run (ROCm 7 device library logf / cosf / sinf); the bound is 4 x that,
# the margin for device-library differences between ROCm builds.  For scale: one fp32 ulp at the largest radius, 5.77, is 4.8e-7.
NORMAL_MEASURED = 8.44e-07
NORMAL_BOUND = 4 * NORMAL_MEASURED
# the restatement's 2^16 normals of this key (a fresh key: episode 0xffffffff, step 0) sit at 0.12 / 0.10 / 0.12 of the three
# sampling bounds the moments test asserts: mean +2.33e-3, var - 1 -2.66e-3, corr +4.69e-3
MOMENT_KEY = 0x1234567890ABCDEF


def _keyed(keys, episodes=None, steps=None):
    from beso_amd.noise import KeyedNoise
    kn = KeyedNoise(keys, DEV)
    if episodes is not None:
        as_i32 = lambda v: torch.from_numpy(np.array(v, dtype=np.uint32).view(np.int32)).to(DEV)      # noqa: E731
        kn.episodes.copy_(as_i32(episodes))
        kn.steps.copy_(as_i32(steps))
    return kn


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("E", [7, 45])
def test_words_are_bit_equal_to_the_restatement(lib, E):
    """N = 3 keys (one with a high word), counters that are not all zero, S = 2; E = 7 (no multiple of 4: the scalar tail) and
    E = 9 * 5; every purpose the rollout uses."""
    kn = _keyed(KEYS, EPISODES, STEPS)
    for name, purpose in (("x_t", 0), ("candidate", 1), ("step", 2)):
        got = _u32(kn.words(name, 2, E))
        want = keyed_words(KEYS, EPISODES, STEPS, purpose, 2, E)
        assert got.shape == want.shape == (2, 3, E) and np.array_equal(got, want), (name, E)


def test_normals_against_float64_and_their_moments(lib):
    """2^16 normals of one key: finite, within NORMAL_BOUND of the float64 evaluation of the header's Box-Muller expression on
    the words the GPU itself returned (bit-equal to the restatement's), and with mean, variance and the correlation between
    the normals e % 4 = 0 and 1 inside 5-sigma sampling bounds."""
    n = 1 << 16
    kn = _keyed([MOMENT_KEY])
    words = _u32(kn.words("x_t", 1, n))
    assert np.array_equal(words, keyed_words([MOMENT_KEY], [0xFFFFFFFF], [0], 0, 1, n))      # (a fresh key: episode -1, step 0)
    z = kn.normal("x_t", 1, n).cpu().numpy()
    assert z.dtype == np.float32 and np.isfinite(z).all()
    want = normals_from_words(words, np.float64)
    dev = float(np.abs(z.astype(np.float64) - want).max())
    print(f"[keyed noise] largest deviation of 2^16 fp32 normals from the float64 expression: {dev:.3e} (bound {NORMAL_BOUND:.3e})")
    assert dev < NORMAL_BOUND
    z = z.astype(np.float64).reshape(-1)
    q = z.reshape(-1, 4)
    mean, var, corr = z.mean(), z.var(), np.corrcoef(q[:, 0], q[:, 1])[0, 1]
    print(f"[keyed noise] mean {mean:+.3e}, var - 1 {var - 1:+.3e}, corr(z0, z1) {corr:+.3e}")
    assert abs(mean) < 5 / np.sqrt(n) and abs(var - 1) < 5 * np.sqrt(2 / n) and abs(corr) < 5 / np.sqrt(n / 4)
    half = kn.normal("x_t", 1, 64, scale=0.5).cpu().numpy()
    assert np.array_equal(half, (z[:64] * 0.5).astype(np.float32).reshape(1, 1, 64)), "scale is one fp32 multiply"


def test_outputs_do_not_depend_on_what_the_buffers_held(lib):
    """Every output of the three calls pre-filled with NaN and with 0 gives equal bits, and the guard rows in front of and
    behind each extent stay as they were.  E = 7 and act = 3 take the scalar stores, E = 8 the 16-byte ones."""
    guard = 64

    def banded(count, fill, dtype=torch.float32):
        buf = torch.full((count + 2 * guard,), fill, dtype=dtype, device=DEV)
        buf[:guard] = 77
        buf[-guard:] = 77
        return buf, buf[guard:guard + count]

    def guards_intact(buf):
        return bool((buf[:guard] == 77).all()) and bool((buf[-guard:] == 77).all())

    results = []
    for fill in (float("nan"), 0.0):
        out = []
        for E in (7, 8):
            kn = _keyed(KEYS, EPISODES, STEPS)
            wbuf, w = banded(2 * 3 * E, 0 if fill == 0.0 else -1, torch.int32)
            zbuf, z = banded(2 * 3 * E, fill)
            kn.words("step", 2, E, out=w)
            kn.normal("step", 2, E, out=z)
            torch.cuda.synchronize()
            assert guards_intact(wbuf) and guards_intact(zbuf), E
            out += [w.clone(), bits(z)]
        for act in (3, 4):                                   # (scalar stores; 16-byte stores)
            kn = _keyed(KEYS, EPISODES, STEPS)
            N, K, n, elems = 3, 2, 4, 2 * 3 * act
            bufs = [banded(N * act, fill), banded(N * K * act, fill), banded(n * N * elems, fill)]
            kn.rollout(act, K, n, elems, out=tuple(v for _, v in bufs))
            torch.cuda.synchronize()
            assert all(guards_intact(b) for b, _ in bufs), act
            out += [bits(v) for _, v in bufs] + [kn.episodes.clone(), kn.steps.clone()]
            assert not any(torch.isnan(v).any() for _, v in bufs)
        results.append(out)
    assert all(torch.equal(a, b) for a, b in zip(*results))


def test_rollout_call_advances_the_counters_and_draws_at_the_advanced_ones(lib):
    """beso_noise_rollout on its own: a marked environment goes to (episode + 1, 0), the others to (episode, step + 1), uint32
    arithmetic; the three outputs are the restatement's normals at the advanced counters in the layouts the rollout's launches
    read -- x_t [N, act], cand [N, K, act], step noise [n, N, elems] -- and the pair of counter arrays read is left as it was."""
    kn = _keyed(KEYS, EPISODES, STEPS)
    kn.reset.zero_()
    kn.reset[1] = 1
    before = (kn.episodes, kn.steps)
    x_t, cand, step_noise = kn.rollout(3, 2, 4, 18)
    episodes, steps = [0, 4, 0x0FFFFFFF], [6, 0, 0]
    assert _u32(kn.episodes).tolist() == episodes and _u32(kn.steps).tolist() == steps
    assert _u32(before[0]).tolist() == EPISODES and _u32(before[1]).tolist() == STEPS and kn.episodes is not before[0]
    assert int(kn.reset.sum()) == 0
    for got, want in ((x_t.view(3, 3), keyed_normals(KEYS, episodes, steps, 0, 1, 3)[0]),
                      (cand, keyed_normals(KEYS, episodes, steps, 1, 2, 3).transpose(1, 0, 2)),
                      (step_noise, keyed_normals(KEYS, episodes, steps, 2, 4, 18))):
        assert tuple(got.shape) == want.shape
        assert float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) < NORMAL_BOUND
    x_t2, _, _ = kn.rollout(3)                               # no reset pending: NULL flags, everyone steps on
    assert _u32(kn.episodes).tolist() == episodes and _u32(kn.steps).tolist() == [7, 1, 1] and kn.episodes is before[0]
    assert float(np.abs(x_t2.view(3, 3).cpu().numpy() - keyed_normals(KEYS, episodes, [7, 1, 1], 0, 1, 3)[0]).max()) < NORMAL_BOUND


# ------------------------------------------------------------------------------------------------ the rollout
SEEDS = [101, (9 << 32) | 2, 303, 0xABCDEF0123456789, 505]
CFG = O.TINY


@pytest.fixture(scope="module")
def agent():
    return _agent(CFG, "fp32")


class _World:
    """Raw observations and goals per ENVIRONMENT IDENTITY (0 ... 4), so that a rollout over any subset of the environments
    feeds each of them what every other rollout feeds it."""

    def __init__(self, steps=4):
        g = torch.Generator("cpu").manual_seed(5)
        self.goal = torch.randn((5, CFG.goal_seq_len, CFG.obs_dim), generator=g).to(DEV)
        self.obs = (torch.randn((steps, 5, CFG.obs_dim), generator=g) * 2 + 0.5).to(DEV)


def _run(agent, who, world, steps=4, seeded=True, **step_args):
    """A rollout over the environments `who` (identities), seeded with their SEEDS; environment 1 is reset before the third
    step.  -> per step (actions, last)."""
    roll = agent.vector_rollout(len(who))
    roll.set_goal(world.goal[who])
    if seeded:
        roll.seed([SEEDS[w] for w in who])
    out = []
    for i in range(steps):
        if i == 2 and 1 in who:
            roll.reset([who.index(1)])
        pred = roll.step(world.obs[i, who], **step_args)
        out.append((pred, {k: v.clone() for k, v in roll.last.items()}))     # (lengths and the counters are live tensors)
    return out


def _newest(x, lengths, K=1):
    """The newest slot of every row of x [N K, W, act] -> [N K, act]."""
    at = torch.repeat_interleave((lengths - 1).long(), K)
    return x[torch.arange(x.shape[0], device=x.device), at]


@pytest.mark.parametrize("variant", ["ddim", "candidates", "euler_ancestral"])
def test_an_environments_draws_do_not_depend_on_its_neighbours(agent, variant):
    """Rollout A runs environments 0 ... 4, rollout B environments [3, 1]; 4 steps, environment 1 reset before the third.  At
    every step the x_T in the newest slot of the sampler's input, the counters, the K candidate draws and the step noise
    handed to euler_ancestral are bit-equal for the matching environments, and are the restatement's normals of
    (seed, episode, step).  The actions agree to the fp32 parity tolerance: equal bits across batch sizes are not promised by
    the denoiser's kernels."""
    world = _World()
    args = {"ddim": {}, "candidates": dict(candidates=3, select="mean"),
            "euler_ancestral": dict(new_sampler_type="euler_ancestral")}[variant]
    A, B = _run(agent, [0, 1, 2, 3, 4], world, **args), _run(agent, [3, 1], world, **args)
    rows_a, who = [3, 1], [3, 1]
    keys = [SEEDS[w] for w in who]
    sigma_max, act, W = float(agent.sigma_max), CFG.act_dim, CFG.obs_seq_len
    for i, ((pa, la), (pb, lb)) in enumerate(zip(A, B)):
        episodes, steps = [0, 0 if i < 2 else 1], [i, i if i < 2 else i - 2]
        for last, rows in ((la, rows_a), (lb, [0, 1])):
            assert _u32(last["noise_episode"][rows]).tolist() == episodes and _u32(last["noise_step"][rows]).tolist() == steps, i
        assert la["lengths"][rows_a].tolist() == lb["lengths"].tolist()
        if variant == "candidates":
            xa = _newest(la["x_k"], la["lengths"], 3).view(5, 3, act)[rows_a]
            xb = _newest(lb["x_k"], lb["lengths"], 3).view(2, 3, act)
            want = keyed_normals(keys, episodes, steps, 1, 3, act).transpose(1, 0, 2)
        else:
            xa, xb = _newest(la["x"], la["lengths"])[rows_a], _newest(lb["x"], lb["lengths"])
            want = keyed_normals(keys, episodes, steps, 0, 1, act)[0]
        assert torch.equal(bits(xa), bits(xb)), (variant, i)
        assert float(np.abs(xa.cpu().numpy().astype(np.float64) - want * sigma_max).max()) < NORMAL_BOUND * sigma_max
        if variant == "euler_ancestral":
            na, nb = la["step_noise"], lb["step_noise"]
            assert tuple(na.shape) == (3, 5, W, act) and tuple(nb.shape) == (3, 2, W, act)
            assert torch.equal(bits(na[:, rows_a]), bits(nb)), i
            want = keyed_normals(keys, episodes, steps, 2, 3, W * act).reshape(3, 2, W, act)
            assert float(np.abs(nb.cpu().numpy().astype(np.float64) - want).max()) < NORMAL_BOUND
        else:
            assert "step_noise" not in la
        err = rel_err(pa[rows_a].cpu().numpy(), pb.cpu().numpy())
        assert err < TOL["fp32"], (variant, i, err)
    if variant == "candidates":
        # candidate k of an environment is not candidate k of another, nor its own x_T draw
        x = _newest(A[0][1]["x_k"], A[0][1]["lengths"], 3).view(5, 3, act)
        assert len({tuple(r.tolist()) for r in x.reshape(15, act)}) == 15


def test_seeded_runs_repeat_and_unseed_restores_the_global_draws(agent):
    """Two seeded runs give equal bits whatever the global generator holds, and draw nothing from it; after unseed() the
    rollout's actions are, bit for bit, those of a rollout that was never seeded under the same torch.manual_seed."""
    world = _World()
    for args in ({}, dict(new_sampler_type="euler_ancestral", candidates=2, select="mean")):
        torch.manual_seed(1)
        first = _run(agent, [0, 1, 2], world, **args)
        state = torch.cuda.get_rng_state(DEV)
        torch.manual_seed(2)
        second = _run(agent, [0, 1, 2], world, **args)
        assert all(torch.equal(bits(a), bits(b)) for (a, _), (b, _) in zip(first, second))
        torch.manual_seed(1)
        assert torch.equal(torch.cuda.get_rng_state(DEV), state), "a seeded step drew from the global generator"
    torch.manual_seed(9)
    never = _run(agent, [0, 1, 2], world, seeded=False, new_sampler_type="euler_ancestral")
    roll = agent.vector_rollout(3)
    roll.set_goal(world.goal[[0, 1, 2]])
    roll.seed(4)
    roll.step(world.obs[0, [0, 1, 2]])
    roll.unseed()
    roll.reset()
    torch.manual_seed(9)
    for i in range(4):
        if i == 2:
            roll.reset([1])
        got = roll.step(world.obs[i, [0, 1, 2]], new_sampler_type="euler_ancestral")
        assert torch.equal(bits(got), bits(never[i][0])), i
        assert "noise_episode" not in roll.last


def test_seed_arguments_and_reseeding(agent):
    """An int seed gives environment i the key seed + i; a partial seed() needs a seeded rollout, restarts the listed
    environments at episode 0 / step 0 and leaves the others' counters running."""
    world = _World()
    roll = agent.vector_rollout(3)
    roll.set_goal(world.goal[[0, 1, 2]])
    with pytest.raises(ValueError, match="first call seeds every environment"):
        roll.seed([5], env_ids=[1])
    with pytest.raises(ValueError):
        roll.seed([1, 2])
    roll.seed(2 ** 64 - 1)
    assert [k % 2 ** 64 for k in roll._keyed.keys.tolist()] == [2 ** 64 - 1, 0, 1]
    roll.step(world.obs[0, [0, 1, 2]])
    roll.step(world.obs[1, [0, 1, 2]])
    roll.seed([77], env_ids=[2])
    roll.step(world.obs[2, [0, 1, 2]])
    assert roll.last["noise_episode"].tolist() == [0, 0, 0] and roll.last["noise_step"].tolist() == [2, 2, 0]
    x = _newest(roll.last["x"], roll.last["lengths"]).cpu().numpy().astype(np.float64)
    want = keyed_normals([2 ** 64 - 1, 0, 77], [0, 0, 0], [2, 2, 0], 0, 1, CFG.act_dim)[0] * float(agent.sigma_max)
    assert float(np.abs(x - want).max()) < NORMAL_BOUND * float(agent.sigma_max)
    assert roll.last["lengths"].tolist() == [3, 3, 3], "re-seeding does not touch the windows"


def test_seeded_rollout_refuses_samplers_that_draw_in_a_python_loop(agent, monkeypatch):
    """dpmpp_2m_sde raises ValueError naming it before anything is enqueued (the windows and the counters stay as they were);
    so does an ancestral sampler forced off its one-launch path; an explicit noise= still passes through untouched."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    world = _World()
    roll = agent.vector_rollout(2)
    roll.set_goal(world.goal[[0, 1]])
    roll.seed([1, 2])
    with pytest.raises(ValueError, match="dpmpp_2m_sde"):
        roll.step(world.obs[0, [0, 1]], new_sampler_type="dpmpp_2m_sde")
    assert roll.lengths.tolist() == [0, 0] and roll._keyed.steps.tolist() == [0, 0] and roll._keyed.episodes.tolist() == [-1, -1]
    with monkeypatch.context() as mp:
        mp.setattr(ks, "_fused_call", lambda *a, **k: None)              # what a model or schedule the fused loop does not run gives
        with pytest.raises(ValueError, match="euler_ancestral.*one-launch path"):
            roll.step(world.obs[0, [0, 1]], new_sampler_type="euler_ancestral")
        roll.step(world.obs[0, [0, 1]], new_sampler_type="euler")        # a deterministic sampler works under every plan
    assert roll.lengths.tolist() == [1, 1] and roll.last["noise_step"].tolist() == [0, 0]
    given = torch.full((2, 1, CFG.act_dim), 0.25, device=DEV)
    roll.step(world.obs[1, [0, 1]], noise=given)
    assert torch.equal(_newest(roll.last["x"], roll.last["lengths"]), given[:, 0] * float(agent.sigma_max))
    assert roll.last["noise_episode"].tolist() == [0, 0] and roll.last["noise_step"].tolist() == [1, 1]
    # the samplers' own refusal inside a keyed context, for callers other than the rollout
    state, x = roll.last["state"], roll.last["x"].clone()
    sig = agent.get_noise_schedule(3, "exponential")
    with agent._ema_scope(), ks.keyed_step_noise(None):
        with pytest.raises(ValueError, match="dpmpp_2m_sde"):
            ks.sample_dpmpp_sde(agent.model, state, x, roll.goal, sig)
        with pytest.raises(ValueError, match="heun.*s_churn"):
            ks.sample_heun(agent.model, state, x, roll.goal, sig, s_churn=1.0)
        with pytest.raises(ValueError, match="euler_ancestral.*one-enqueue"):
            ks.sample_euler_ancestral(agent.model, state, x, roll.goal, sig, callback=lambda d: None)
        with pytest.raises(ValueError, match="drew none"):
            ks.sample_euler_ancestral(agent.model, state, x, roll.goal, sig)
    assert ks.keyed_step_noise.active is None
