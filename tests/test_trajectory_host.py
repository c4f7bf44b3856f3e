"""Host-side checks of the trajectory feature (no GPU): ``replay_callback``, the refusals of ``sample_trajectory``, the
binding list, and the fixture tests/golden/tiny_trajectory.npz pinned to the numpy oracle like the other sampler fixtures."""
import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import load_golden, rel_err
from support import load_lib

TOL = 5e-5   # fp32 oracle vs fp32 reference over a loop of <= 10 steps (test_oracle_golden.test_samplers_match_reference)


def test_replay_callback_calls_in_order_with_the_documented_keys():
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    n = 4
    sig = ks.get_sigmas_exponential(n, 0.05, 1.0)
    xs, den = torch.randn(n + 1, 2, 3, 2), torch.randn(n, 2, 3, 2)
    seen = []
    ks.replay_callback(seen.append, sig, xs, den)
    assert [d["i"] for d in seen] == list(range(n))
    for i, d in enumerate(seen):
        assert set(d) == {"x", "i", "sigma", "sigma_hat", "denoised"}
        assert d["x"] is not None and torch.equal(d["x"], xs[i]) and torch.equal(d["denoised"], den[i])
        assert float(d["sigma"]) == float(sig[i]) == float(d["sigma_hat"])


def test_sample_trajectory_is_fused_only():
    """A foreign model, and CPU tensors, raise NotImplementedError with the reason: there is no second evaluation path."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT
    from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser
    s, a, g = torch.zeros(2, 3, 7), torch.zeros(2, 3, 3), torch.zeros(2, 2, 7)
    sig = ks.get_sigmas_exponential(3, 0.05, 1.0)
    foreign = lambda state, action, goal, sigma, **kw: action      # noqa: E731
    with pytest.raises(NotImplementedError, match="GCDenoiser"):
        ks.sample_trajectory("ddim", foreign, s, a, g, sig)
    inner = DiffusionGPT(state_dim=7, device="cpu", goal_conditioned=True, action_dim=3, embed_dim=48,
                         embed_pdrob=0, attn_pdrop=0, resid_pdrop=0, n_layers=2, n_heads=6, goal_seq_len=2,
                         obs_seq_len=3, sigma_vocab_size=3, time_embedding_fn=None, linear_output=True)
    m = GCDenoiser(inner, sigma_data=0.5).eval()
    with pytest.raises(NotImplementedError, match="GPU"):
        ks.sample_trajectory("ddim", m, s, a, g, sig)
    with pytest.raises(ValueError):
        ks.sample_trajectory("no_such_sampler", m, s, a, g, sig)


def test_binding_list_carries_the_traced_entry_point():
    from beso_amd import _lib
    assert "beso_sample_traced" in _lib.EXPORTS
    assert set(_lib.ENTRY_IDS) == {entry for entry, _ in _lib.SAMPLERS.values()}


def test_trajectory_fixture_matches_the_oracle():
    """The final outputs of tiny_trajectory.npz (reference) are what the numpy oracle's samplers compute, and the recorded
    per-step values are consistent with them: x of step 0 is x_T, `denoised` of step i is the oracle's model at x of step i."""
    fx = load_golden("tiny_trajectory.npz")
    cfg = O.TINY
    model = O.make_model(O.make_weights(cfg, seed=int(fx["seed"]), std=float(fx["std"])), cfg)
    s, g, x_t = fx["state"], fx["goal"], fx["x_t"]
    for name in ("euler", "heun", "dpmpp_2m"):
        sig = fx[name + "::sigmas"]
        assert rel_err(O.SAMPLERS[name](model, s, x_t, g, sig), fx[name + "::out"]) < TOL, name
        assert np.array_equal(fx[name + "::x"][0], x_t)
        for i in range(len(sig) - 1):
            den = model(s, fx[name + "::x"][i], g, np.full(len(s), sig[i], np.float32))
            assert rel_err(den, fx[name + "::denoised"][i]) < TOL, (name, i)
    sig = fx["euler_ancestral::sigmas"]
    out = O.sample_euler_ancestral(model, s, x_t, g, sig, noise_list=fx["euler_ancestral::noise"])
    assert rel_err(out, fx["euler_ancestral::out"]) < TOL
    # the visualize_ode list: every entry is one DDIM step from the one before it, the whole list one DDIM loop
    acts, sig, k = fx["ode::actions"], fx["ode::sigmas"], int(fx["ode::get_mean"])
    s2, g2 = np.repeat(fx["ode::state"], k, axis=0), np.repeat(fx["ode::goal"], k, axis=0)
    assert len(acts) == len(sig)
    for i in range(len(sig) - 1):
        assert rel_err(O.sample_ddim(model, s2, acts[i], g2, sig[i:i + 2]), acts[i + 1]) < TOL, i
    assert rel_err(O.sample_ddim(model, s2, acts[0], g2, sig), acts[-1]) < TOL


def test_traced_entry_point_rejects_bad_arguments_before_touching_the_device():
    """beso_sample_traced checks as the call it stands for checks, then its own: an unknown entry, capacities one float short
    (BESO_ERR_WORKSPACE) and a trace buffer that overlaps x (BESO_ERR_BAD_ARG) -- nothing is enqueued (the pointers are fake)."""
    import ctypes as C
    from beso_amd import _lib
    from beso_amd.runtime import ScoreNetShape
    lib = load_lib()
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()
    B, t, act, n_sig = 2, 2, 3, 3
    n = B * t * act
    sig = (C.c_float * n_sig)(1.0, 0.5, 0.0)
    base = 0x100000
    x, far = base, base + 0x10000

    def call(entry=0, sampler=0, xp=x, noise=None, hist=None, tx=None, tx_cap=0, td=None, td_cap=0, wsb=1 << 30):
        p = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
        return lib.beso_sample_traced(C.byref(cfg), p(far * 2), 0, entry, sampler, p(far * 3), p(far * 4), p(xp), B, t, sig, n_sig,
                                      1.0, 1.0, 1.0, 4, p(noise), p(hist), p(tx), tx_cap, p(td), td_cap, 0, p(far * 5), wsb, None)
    assert call(entry=3) == -3 and call(entry=-1) == -3
    assert call(sampler=9) == -3                                   # beso_sample's check
    assert call(entry=1) == -3 and call(entry=2, sampler=1) == -3  # the ancestral calls need their noise
    assert call(entry=2, sampler=4) == -3                          # DPM-Solver++(2M) needs its state slab
    assert call(wsb=16) == -4
    assert call(tx=far, tx_cap=n_sig * n - 1) == -4
    assert call(td=far, td_cap=(n_sig - 1) * n - 1) == -4
    assert call(tx=far, tx_cap=n_sig * n, td=far + 0x1000, td_cap=(n_sig - 1) * n - 1) == -4
    for ptr in (x, x - 4 * (n_sig * n - 1), x + 4 * (n - 1)):      # any overlap of [x, x + n) with the slabs
        assert call(tx=ptr, tx_cap=n_sig * n) == -3, hex(ptr)
    assert call(td=x + 4, td_cap=(n_sig - 1) * n) == -3
    # ... and of the slabs with each other, the workspace (at far * 5) or the steps' noise
    assert call(tx=far, tx_cap=n_sig * n, td=far + 4 * (n_sig * n - 1), td_cap=(n_sig - 1) * n) == -3
    assert call(tx=far * 5 + 64, tx_cap=n_sig * n) == -3 and call(td=far * 5 - 4, td_cap=(n_sig - 1) * n) == -3
    assert call(entry=1, noise=far * 6, tx=far * 6 + 4, tx_cap=n_sig * n) == -3
