"""The denoising trajectory recorded by the sampler loops (beso_sample_traced, ``trace=`` of ScoreNetRuntime.sample /
GCDenoiser.fused_sampler, gc_sampling.sample_trajectory, BesoAgent.visualize_ode) on a real MI355X.

The first test asks for the one-launch kernels (BESO_PLAN_FUSED, as tests/test_gpu_parity.py does: short windows of 64 kitchen
samples are few enough token rows for the small-batch route) in every case but kitchen bf16 with 3 samples, which is there
for the chip-wide small-batch route, whose update kernel writes the slabs.  The other tests run the library's own choice."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import load_golden, weights_from_fixture, rel_err
from support import build_agent, count_site_launches, make_denoiser, to_dev
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (sampler, steps, network evaluations, extra arguments); the last step of every two-evaluation sampler is a single evaluation
SAMPLERS = [("ddim", 3, 3, {}), ("euler", 7, 7, {}), ("heun", 4, 7, {}), ("dpm_2", 4, 7, {}), ("dpmpp_2s", 3, 5, {}),
            ("dpmpp_2m", 4, 4, {}), ("lms", 5, 5, {"order": 4}), ("euler_ancestral", 5, 5, {}), ("dpm_2_ancestral", 3, 5, {})]


def _sigmas(n):
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    return ks.get_sigmas_exponential(n, 0.05, 1.0)


def _noise(sampler, n_steps, x):
    if not sampler.endswith("_ancestral"):
        return None
    return torch.randn((n_steps,) + tuple(x.shape), device=DEV, generator=torch.Generator(DEV).manual_seed(5))


@pytest.mark.parametrize("cfg_name,precision,B,lam", [
    ("kitchen", "bf16", 3, 1.0), ("kitchen", "bf16", 64, 1.0), ("kitchen", "bf16", 700, 1.0), ("kitchen", "bf16x3", 5, 1.0),
    ("kitchen", "fp16", 64, 1.0), ("block_push", "bf16", 130, 2.0), ("block_push", "bf16", 9, 0.0),
    ("long_horizon", "bf16", 5, 1.0), ("long_horizon", "bf16", 3, 1.5)])
def test_trajectory_is_recorded_by_the_loop_itself_and_equals_the_stepwise_form(cfg_name, precision, B, lam):
    """With a trace requested the loop is still ceil(evaluations / 128) launches (none where the small-batch route serves the
    call step by step: kitchen bf16, 3 samples), x_0 is the plain call's, and xs / denoised equal those of the step-by-step
    form bit for bit; xs[0] is x_T, xs[-1] is x_0, the caller's x_T is untouched."""
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.03), precision)
    s_np, g_np, x_np = O.make_inputs(cfg, B, seed=11)
    from beso_amd import _lib
    from beso_amd.runtime import set_plan
    small_route = (cfg_name, precision, B) == ("kitchen", "bf16", 3)
    set_plan(forward=0 if small_route else _lib.PLAN_FUSED, train=0)
    try:
        _loop_equals_stepwise(cfg, m, cfg_name, precision, B, lam, s_np, g_np, x_np, small_route)
    finally:
        set_plan(forward=0, train=0)


def _loop_equals_stepwise(cfg, m, cfg_name, precision, B, lam, s_np, g_np, x_np, small_route):
    with torch.no_grad():
        for t in sorted({cfg.obs_seq_len, max(1, cfg.obs_seq_len - 2)}):
            s, g, x = to_dev(s_np[:, :t]), to_dev(g_np), to_dev(x_np[:, :t])
            keep = x.clone()
            specs = list(SAMPLERS)
            if (cfg_name, precision, B) == ("kitchen", "bf16", 64) and t == cfg.obs_seq_len:
                specs.append(("heun", 70, 139, {}))                  # two launches: the slab offset across the cut
            for sampler, n_steps, n_evals, kw in specs:
                sig = _sigmas(n_steps)
                kw = dict(kw, cond_lambda=lam, noise=_noise(sampler, n_steps, x))
                out = {}
                n_loop = count_site_launches("fused_layer", lambda: out.__setitem__(
                    "loop", m.fused_sampler(sampler, s, x, g, sig, trace=("x", "denoised"), **kw)))
                out["step"] = m.fused_sampler(sampler, s, x, g, sig, trace=("x", "denoised"), stepwise=True, **kw)
                n_plain = count_site_launches("fused_layer", lambda: out.__setitem__("plain", m.fused_sampler(sampler, s, x, g, sig, **kw)))
                plain = out["plain"]
                what = (cfg_name, precision, B, t, sampler, n_steps)
                assert n_loop == n_plain == (0 if small_route else (n_evals + 127) // 128), what
                x0, rec = out["loop"]
                x0s, recs = out["step"]
                assert tuple(rec["x"].shape) == (n_steps + 1,) + tuple(x.shape), what
                assert tuple(rec["denoised"].shape) == (n_steps,) + tuple(x.shape), what
                assert torch.isfinite(rec["x"]).all() and torch.isfinite(rec["denoised"]).all(), what
                assert torch.equal(rec["x"], recs["x"]), what
                assert torch.equal(rec["denoised"], recs["denoised"]), what
                assert torch.equal(rec["x"][0], keep), what
                assert torch.equal(rec["x"][-1], x0), what
                assert torch.equal(x0, plain) and torch.equal(x0s, plain), what
                assert torch.equal(x, keep), what
                # each output alone is the same tensor
                _, only_x = m.fused_sampler(sampler, s, x, g, sig, trace={"x"}, **kw)
                _, only_d = m.fused_sampler(sampler, s, x, g, sig, trace={"denoised"}, **kw)
                assert set(only_x) == {"x"} and set(only_d) == {"denoised"}
                assert torch.equal(only_x["x"], rec["x"]) and torch.equal(only_d["denoised"], rec["denoised"]), what
                if small_route:
                    # loop and step-by-step are one path here: hold the update kernel's slabs to the model itself -- the first
                    # evaluation of step i is the forward at (xs[i], sigmas[i]) in every sampler
                    for i in range(n_steps):
                        den = m(s, rec["x"][i], g, torch.full((B,), float(sig[i]), device=DEV))
                        assert torch.equal(den, rec["denoised"][i]), (what, i)


@pytest.mark.parametrize("cfg_name,B,lam", [("kitchen", 64, 1.0), ("block_push", 130, 2.0)])
def test_trajectory_is_the_chain_of_two_entry_schedules(cfg_name, B, lam):
    """The reference's visualize_ode loop: the sampler on sigmas[i : i + 2] from xs[i] gives xs[i + 1], and denoised[i] is
    the model's own forward at (xs[i], sigmas[i]) -- equal bits."""
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.03), "bf16")
    model = m if lam == 1.0 else ClassifierFreeSampleModel(m, lam)
    s, g, x = (to_dev(v) for v in O.make_inputs(cfg, B, seed=11))
    with torch.no_grad():
        for sampler, n_steps in (("ddim", 3), ("euler", 4), ("heun", 3), ("dpm_2", 3), ("dpmpp_2s", 3)):
            sig = _sigmas(n_steps)
            _, rec = m.fused_sampler(sampler, s, x, g, sig, cond_lambda=lam, trace=("x", "denoised"))
            for i in range(n_steps):
                nxt = m.fused_sampler(sampler, s, rec["x"][i], g, sig[i:i + 2], cond_lambda=lam)
                assert torch.equal(nxt, rec["x"][i + 1]), (cfg_name, sampler, i)
                den = model(s, rec["x"][i], g, torch.full((B,), float(sig[i]), device=DEV))
                assert torch.equal(den, rec["denoised"][i]), (cfg_name, sampler, i)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sample_trajectory_vs_reference_vectors(precision):
    """sample_trajectory's slabs against what the reference's loops hand their callback step by step
    (tests/golden/tiny_trajectory.npz), under the bounds test_fused_sampler_loops_vs_reference_vectors applies to whole loops:
    a slab is the result of a prefix of such a loop."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    fx = load_golden("tiny_trajectory.npz")
    cfg = O.TINY
    m = make_denoiser(cfg, O.make_weights(cfg, seed=int(fx["seed"]), std=float(fx["std"])), precision)
    tol = TOL["fp32"] if precision == "fp32" else 2e-2
    s, g, x_t = to_dev(fx["state"]), to_dev(fx["goal"]), to_dev(fx["x_t"])
    worst = {}
    with torch.no_grad():
        for name in ("euler", "heun", "dpmpp_2m", "euler_ancestral"):
            nz = to_dev(fx[name + "::noise"]) if name + "::noise" in fx else None
            x0, xs, den = ks.sample_trajectory(name, m, s, x_t, g, torch.from_numpy(fx[name + "::sigmas"]), noise=nz)
            n = len(fx[name + "::sigmas"]) - 1
            assert xs.shape[0] == n + 1 and den.shape[0] == n
            ex = [rel_err(xs[i].cpu().numpy(), fx[name + "::x"][i]) for i in range(n)]
            ex.append(rel_err(xs[n].cpu().numpy(), fx[name + "::out"]))
            ed = [rel_err(den[i].cpu().numpy(), fx[name + "::denoised"][i]) for i in range(n)]
            print(f"[trajectory] {name} {precision}: x " + " ".join(f"{e:.2e}" for e in ex) + " | denoised " +
                  " ".join(f"{e:.2e}" for e in ed))
            worst[name] = max(ex + ed)
            assert torch.equal(xs[n], x0)
        k = int(fx["ode::get_mean"])
        s2 = torch.repeat_interleave(to_dev(fx["ode::state"]), repeats=k, dim=0)
        g2 = torch.repeat_interleave(to_dev(fx["ode::goal"]), repeats=k, dim=0)
        _, xs, _ = ks.sample_trajectory("ddim", m, s2, to_dev(fx["ode::actions"][0]), g2, torch.from_numpy(fx["ode::sigmas"]),
                                        trace=("x",))
        eo = [rel_err(xs[i].cpu().numpy(), fx["ode::actions"][i]) for i in range(len(xs))]
        print(f"[trajectory] visualize_ode list {precision}: " + " ".join(f"{e:.2e}" for e in eo))
        worst["ode"] = max(eo)
    for name, e in worst.items():
        assert e < tol, (name, e)


def _agent(cfg, module, x_data, y_data):
    from beso_amd.networks.scaler.scaler_class import Scaler
    agent = build_agent(cfg, lambda: module, device=DEV)
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    agent.get_scaler(Scaler(x_data, y_data, True, DEV))
    agent.set_bounds(agent.scaler)
    agent.reset()
    return agent


@pytest.mark.parametrize("which", ["tiny", "kitchen"])
def test_agent_visualize_ode(which):
    """BesoAgent.visualize_ode: n_sampling_steps + 1 tensors [N * get_mean, t, act] from ONE sampler call; the last one is
    sample_loop(..., 'ddim') on the same x_T; the EMA scope is left as found.  The tiny agent is the construction of
    test_agent_predict_trace_on_gpu (fp32: no one-launch kernel for that shape, the update kernel records); the kitchen
    agent in bf16 is where the call is one fused launch."""
    if which == "tiny":
        fx = load_golden("tiny_agent_trace.npz")
        cfg, get_mean, n_launch = O.TINY, 4, 0
        agent = _agent(cfg, make_denoiser(cfg, weights_from_fixture(fx), "fp32"), fx["x_data"], fx["y_data"])
    else:
        cfg, get_mean, n_launch = O.KITCHEN, 100, 1
        rng = np.random.default_rng(2)
        agent = _agent(cfg, make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.03), "bf16"),
                       rng.standard_normal((64, cfg.obs_dim)).astype(np.float32),
                       rng.standard_normal((64, cfg.act_dim)).astype(np.float32))
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    rng = np.random.default_rng(9)
    N = 2
    goal = torch.from_numpy(rng.standard_normal((cfg.goal_seq_len, cfg.obs_dim)).astype(np.float32))
    # the live weights move away from the EMA shadow: what visualize_ode evaluates must be the shadow, and the live
    # weights must come back as they were
    with torch.no_grad():
        for p in agent.model.parameters():
            p.add_(0.05)
    before = [p.detach().clone() for p in agent.model.parameters()]
    for call in range(2):                         # the observation context grows: t = 1, then t = 2
        state = torch.from_numpy(rng.standard_normal((N, cfg.obs_dim)).astype(np.float32))
        out = {}
        n = count_site_launches("fused_layer", lambda: out.__setitem__(0, agent.visualize_ode(
            state, goal, get_mean=get_mean, new_sampling_steps=3, noise_scheduler="exponential")))
        acts = out[0]
        t = call + 1
        assert n == n_launch, (which, n)
        assert isinstance(acts, list) and len(acts) == 3 + 1
        for a in acts:
            assert tuple(a.shape) == (N * get_mean, t, cfg.act_dim) and torch.isfinite(a).all()
        # the same loop through sample_loop, from the same x_T
        s_rpt = torch.repeat_interleave(torch.stack(tuple(agent.obs_context), dim=1), repeats=get_mean, dim=0)
        g_rpt = torch.repeat_interleave(agent.scaler.scale_input(goal).unsqueeze(0).expand(N, -1, -1), repeats=get_mean, dim=0)
        with torch.no_grad(), agent._ema_scope():
            ref = agent.sample_loop(agent.get_noise_schedule(3, "exponential"), acts[0], s_rpt, g_rpt, "ddim")
        assert torch.equal(acts[-1], ref), which
        assert agent._ema_packed is not None, "the EMA packed image must have been used"
        with torch.no_grad():
            live = ks.sample_ddim(agent.model, s_rpt, acts[0], g_rpt, agent.get_noise_schedule(3, "exponential"), disable=True)
        assert not torch.equal(acts[-1], live), "visualize_ode evaluated the live weights, not the EMA shadow"
    for p, q in zip(agent.model.parameters(), before):
        assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------ the C entry point itself
def _raw(m, cfg, s, g, x, sig, tx, tx_cap, td, td_cap, sampler=0, lam=1.0):
    """beso_sample_traced through ctypes (entry BESO_ENTRY_SAMPLE) with caller-owned trace buffers and capacities."""
    inner = m.inner_model
    rt, packed = inner.runtime(cfg.sigma_data), inner.packed_weights()
    B, t = x.shape[:2]
    ws = rt._workspace(B, t, lam not in (0.0, 1.0), x.device)
    arr = (C.c_float * len(sig))(*[float(v) for v in sig])
    ptr = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())      # noqa: E731
    with torch.cuda.device(x.device):
        return rt.lib.beso_sample_traced(C.byref(rt.cfg), packed.buf.data_ptr(), packed.precision, 0, sampler, s.data_ptr(),
                                         g.data_ptr(), x.data_ptr(), B, t, arr, len(sig), lam, 1.0, 1.0, 4, None, None,
                                         ptr(tx), tx_cap, ptr(td), td_cap, 0, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream(x.device).cuda_stream)


def test_traced_entry_point_checks_its_arguments():
    """Capacities one float short -> BESO_ERR_WORKSPACE with x untouched; a trace buffer over x -> BESO_ERR_BAD_ARG; both
    pointers NULL -> beso_sample's result."""
    cfg = O.KITCHEN
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.03), "bf16")
    B, n_steps = 64, 3
    s, g, x_t = (to_dev(v) for v in O.make_inputs(cfg, B, seed=11))
    sig = [float(v) for v in _sigmas(n_steps)]
    n = x_t.numel()
    tx = torch.zeros((n_steps + 1) * n, device=DEV)
    td = torch.zeros(n_steps * n, device=DEV)
    x = x_t.clone()
    assert _raw(m, cfg, s, g, x, sig, tx, tx.numel() - 1, td, td.numel()) == -4
    assert _raw(m, cfg, s, g, x, sig, tx, tx.numel(), td, td.numel() - 1) == -4
    assert _raw(m, cfg, s, g, x, sig, tx, tx.numel() - 1, None, 0) == -4
    assert _raw(m, cfg, s, g, x, sig, None, 0, td, td.numel() - 1) == -4
    big = torch.zeros((n_steps + 2) * n, device=DEV)            # x inside the trace buffer: its last slab
    xin = big[(n_steps + 1) * n - 8:][:n].view_as(x_t)
    assert _raw(m, cfg, s, g, xin, sig, big, (n_steps + 1) * n, None, 0) == -3
    assert _raw(m, cfg, s, g, x, sig, x.data_ptr(), (n_steps + 1) * n, None, 0) == -3
    assert _raw(m, cfg, s, g, x, sig, None, 0, x.data_ptr(), n_steps * n) == -3
    torch.cuda.synchronize()
    assert torch.equal(x, x_t) and not tx.any() and not td.any()                 # nothing was enqueued
    assert _raw(m, cfg, s, g, x, sig, None, 0, None, 0) == 0
    with torch.no_grad():
        assert torch.equal(x, m.fused_sampler("ddim", s, x_t, g, sig))


@pytest.mark.parametrize("B", [5, 70])
def test_trace_buffers_are_written_not_read(B):
    """What the trace buffers hold before the call changes nothing (zeros, NaN bits, a large finite value): results and
    traces are identical, and the rows behind the stated capacity keep their fill."""
    cfg = O.KITCHEN
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.03), "bf16")
    n_steps = 3
    s, g, x_t = (to_dev(v) for v in O.make_inputs(cfg, B, seed=11))
    sig = [float(v) for v in _sigmas(n_steps)]
    n = x_t.numel()
    cap_x, cap_d, guard = (n_steps + 1) * n, n_steps * n, 2 * x_t.shape[1] * x_t.shape[2]
    runs = []
    for bits in (0, 0x7FC00000, 0x7F000000):                     # 0.0, a quiet NaN, 1.7e38
        tx = torch.full((cap_x + guard,), bits, dtype=torch.int32, device=DEV)
        td = torch.full((cap_d + guard,), bits, dtype=torch.int32, device=DEV)
        x = x_t.clone()
        assert _raw(m, cfg, s, g, x, sig, tx, cap_x, td, cap_d, sampler=2) == 0          # Heun: parks between evaluations
        torch.cuda.synchronize()
        assert (tx[cap_x:] == bits).all() and (td[cap_d:] == bits).all(), hex(bits)
        runs.append((x.view(torch.int32).flatten(), tx[:cap_x].clone(), td[:cap_d].clone()))
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    x0, tx0, _ = runs[0]
    assert torch.equal(tx0[:n], x_t.view(torch.int32).flatten()) and torch.equal(tx0[-n:], x0)
    assert torch.isfinite(tx0.view(torch.float32)).all() and torch.isfinite(runs[0][2].view(torch.float32)).all()
