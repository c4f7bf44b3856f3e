"""DPM-2, DPM-2 ancestral, DPM-Solver++(2S), its ancestral form, DPM-Solver++(2M) and LMS as one enqueue (beso_sample_solver).

CPU: the C ABI's argument checks.
GPU: the one-launch loop against the step-by-step form (bit for bit, with launch counts) in every instance of the kernel, against
the CPU oracle, against today's Python loop, at the agent level, the fallbacks that keep the Python loop, and determinism."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from oracle import beso_oracle as O
from conftest import rel_err
from support import build_agent, count_site_launches, lib, make_denoiser, to_dev  # noqa: F401
from beso_amd import _lib
from beso_amd.runtime import ScoreNetShape

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ("dpm_2", "dpm_2_ancestral", "dpmpp_2s", "dpmpp_2s_ancestral", "dpmpp_2m", "lms")
ANCESTRAL = ("dpm_2_ancestral", "dpmpp_2s_ancestral")


def n_evals(solver, n_steps):
    """Network evaluations of a loop whose last sigma is 0 (two per step, one on the last, for the two-stage solvers)."""
    return n_steps if solver in ("dpmpp_2m", "lms") else 2 * n_steps - 1


# ------------------------------------------------------------------------------------------------ CPU
def test_sample_solver_is_exported_and_checks_its_arguments(lib):
    from beso_amd.build import LIB
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "beso_sample_solver" in out.split()
    assert "beso_sample_solver" in _lib.EXPORTS
    assert "int beso_sample_solver(" in open(os.path.join(ROOT, "include", "beso_hip.h")).read()
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()
    one = C.c_void_p(16)
    big = 1 << 40
    f = lib.beso_sample_solver

    def call(sig=(1.0, 0.5, 0.0), **kw):
        arr = (C.c_float * len(sig))(*sig)
        a = dict(cfg=C.byref(cfg), packed=one, prec=0, solver=0, state=one, goal=one, x=one, batch=2, t=2, sig=arr,
                 n_sig=len(sig), lam=1.0, eta=1.0, s_noise=1.0, order=4, noise=one, hist=one, flags=0, ws=one, wsb=big,
                 stream=None)
        a.update(kw)
        return f(*a.values())

    assert call(solver=-1) == -3 and call(solver=6) == -3                          # unknown solver
    assert call(solver=5, order=0) == -3 and call(solver=5, order=5) == -3          # LMS order outside 1 ... 4
    for s in (1, 3):
        assert call(solver=s, noise=None) == -3, s                                  # the ancestral solvers need their noise
    assert call(solver=4, hist=None) == -3                                          # DPM++(2M): one state slab
    assert call(solver=5, order=2, hist=None) == -3                                 # LMS: order - 1 slabs
    assert call(solver=0, eta=-0.5) == -3 and call(solver=1, eta=float("nan")) == -3
    assert call(sig=(1.0, 0.0, 0.0)) == -3 and call(sig=(1.0, -0.5, 0.0)) == -3    # an interior sigma <= 0
    assert call(flags=0x4000) == -3 and call(flags=0x1) == -3                       # unknown flags
    assert call(sig=(1.0,)) == -3 and call(x=None) == -3 and call(ws=None) == -3
    assert call(t=9) == -2 and call(batch=0) == -2
    assert call(wsb=16) == -4
    assert call(prec=7) == -3
    # where nothing is needed, the buffers may be NULL: the checks pass and the argument errors left are the others'
    assert call(solver=5, order=1, hist=None, wsb=16) == -4
    assert call(solver=0, noise=None, hist=None, wsb=16) == -4


# ------------------------------------------------------------------------------------------------ GPU helpers
def make_module(cfg, precision, seed=3, std=0.03):
    return make_denoiser(cfg, O.make_weights(cfg, seed=seed, std=std), precision)


@pytest.fixture
def fused_plan():
    """The one-launch kernel at every batch size (BESO_PLAN_FUSED: small batches would otherwise take the chip-wide
    small-batch path, step by step)."""
    from beso_amd.runtime import set_plan
    set_plan(forward=_lib.PLAN_FUSED, train=0)
    yield
    set_plan(forward=0, train=0)


def _sampler_fns():
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    return {"dpm_2": ks.sample_dpm_2, "dpm_2_ancestral": ks.sample_dpm_2_ancestral, "dpmpp_2s": ks.sample_dpmpp_2s,
            "dpmpp_2s_ancestral": ks.sample_dpmpp_2s_ancestral, "dpmpp_2m": ks.sample_dpmpp_2m, "lms": ks.sample_lms}


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision,B,lam", [
    ("kitchen", "bf16", 3, 1.0), ("kitchen", "bf16", 64, 1.0), ("kitchen", "bf16", 700, 1.0), ("kitchen", "bf16", 1100, 1.0),
    ("kitchen", "bf16x3", 5, 1.0), ("kitchen", "bf16x3", 600, 1.0),
    ("block_push", "bf16", 130, 2.0), ("block_push", "bf16", 9, 0.0), ("block_push", "bf16x3", 258, 2.0),
    ("long_horizon", "bf16", 5, 1.0), ("long_horizon", "bf16", 3, 1.5)])
def test_solver_loop_is_one_launch_and_equals_the_stepwise_loop(fused_plan, cfg_name, precision, B, lam):
    """The six solvers run as ONE launch of layers_kernel (up to 128 evaluations, cut at step boundaries beyond) and equal
    the step-by-step form (one forward + one update launch per evaluation) BIT FOR BIT in every instance of the kernel, for
    full and short windows; the schedules of more than 128 evaluations carry the 2M / LMS state across launches."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    cfg = O.CONFIGS[cfg_name]
    m = make_module(cfg, precision)
    s_np, g_np, x_np = O.make_inputs(cfg, B, seed=11)
    with torch.no_grad():
        for t in sorted({cfg.obs_seq_len, max(1, cfg.obs_seq_len - 2)}):
            s, g, x = to_dev(s_np[:, :t]), to_dev(g_np), to_dev(x_np[:, :t])
            keep = x.clone()
            for solver in SOLVERS:
                long = 130 if solver in ("dpmpp_2m", "lms") else 70
                cases = [(4, 1.0, 4), (long, 1.0, 4)]
                if solver in ANCESTRAL:
                    cases.append((3, 0.0, 4))
                if solver == "lms":
                    cases += [(5, 1.0, 1), (5, 1.0, 2), (6, 1.0, 3)]
                for n_steps, eta, order in cases:
                    if n_steps > 10 and (B > 200 or t != cfg.obs_seq_len):
                        continue
                    sig = ks.get_sigmas_exponential(n_steps, 0.05, 1.0)
                    nz = torch.randn((n_steps,) + tuple(x.shape), device=DEV, generator=torch.Generator(DEV).manual_seed(5))
                    kw = dict(cond_lambda=lam, eta=eta, noise=nz, order=order, s_noise=0.75)
                    out = {}
                    n_loop = count_site_launches("fused_layer", lambda: out.__setitem__("loop", m.fused_sampler(solver, s, x, g, sig, **kw)))
                    n_step = count_site_launches("fused_layer", lambda: out.__setitem__(
                        "step", m.fused_sampler(solver, s, x, g, sig, stepwise=True, **kw)))
                    ne = n_evals(solver, n_steps)
                    what = (cfg_name, precision, B, t, solver, n_steps, eta, order)
                    assert n_loop == (ne + 127) // 128, (what, n_loop)
                    assert n_step == ne, (what, n_step)
                    assert torch.isfinite(out["loop"]).all(), what
                    assert torch.equal(out["loop"], out["step"]), what
                    assert torch.equal(x, keep), "the solver must not overwrite the caller's x_T"
                    if solver in ANCESTRAL and eta == 1.0 and n_steps == 4:      # the noise matters
                        other = m.fused_sampler(solver, s, x, g, sig, **dict(kw, noise=nz * 0.5))
                        assert not torch.equal(other, out["loop"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("precision,tol", [("bf16x3", 1e-4), ("bf16", 2e-2)])
def test_solvers_against_the_oracle(fused_plan, precision, tol):
    """ks.sample_* over the CPU oracle (OracleModel: the reference's network in numpy) against the one-launch loop, on kitchen
    and on block-push with classifier-free guidance (lambda = 2); the ancestral solvers at eta = 0."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    from test_host_logic import OracleModel
    fns = _sampler_fns()
    for cfg_name, lam, B in (("kitchen", 1.0, 6), ("block_push", 2.0, 4)):
        cfg = O.CONFIGS[cfg_name]
        w = O.make_weights(cfg, seed=3, std=0.03)
        m = make_module(cfg, precision)
        model = m if lam == 1.0 else ClassifierFreeSampleModel(m, lam)
        oracle = OracleModel(w, cfg, None if lam == 1.0 else lam)
        s_np, g_np, x_np = O.make_inputs(cfg, B, seed=21)
        sig = ks.get_sigmas_exponential(5, 0.05, 1.0)
        for solver, fn in fns.items():
            kw = {"eta": 0.0} if solver in ANCESTRAL else {}
            box = {}
            with torch.no_grad():
                ref = fn(oracle, *(torch.from_numpy(v.copy()) for v in (s_np, x_np, g_np)), sig, disable=True, **kw)
                n = count_site_launches("fused_layer", lambda: box.__setitem__("x", fn(model, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True,
                                                                        **kw)))
            assert n == 1, (cfg_name, solver, n)
            err = rel_err(box["x"].cpu().numpy(), ref.numpy())
            print(f"[solvers] {cfg_name} {solver} {precision} one launch vs oracle: {err:.3e}")
            assert err <= tol, (cfg_name, solver, err)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,stepwise", [("bf16x3", False), ("fp32", True)])
def test_solvers_against_the_python_loop(fused_plan, precision, stepwise):
    """The one enqueue against today's Python loop on the GPU (forced by a no-op callback), at equal seeds: the bf16x3 one-launch
    loop and the fp32 step-by-step form (fp32 has no one-launch instance), kitchen and block-push CFG."""
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    fns = _sampler_fns()
    for cfg_name, lam, B in (("kitchen", 1.0, 16), ("block_push", 2.0, 8)):
        cfg = O.CONFIGS[cfg_name]
        m = make_module(cfg, precision)
        model = m if lam == 1.0 else ClassifierFreeSampleModel(m, lam)
        s_np, g_np, x_np = O.make_inputs(cfg, B, seed=31)
        sig = ks.get_sigmas_exponential(6, 0.05, 1.0)
        for solver, fn in fns.items():
            kw = {"s_noise": 0.5} if solver == "dpmpp_2s_ancestral" else {}
            with torch.no_grad():
                torch.manual_seed(7)
                box = {}
                n = count_site_launches("fused_layer", lambda: box.__setitem__("one", fn(model, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True,
                                                                          **kw)))
                torch.manual_seed(7)
                loop = fn(model, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True, callback=lambda d: None, **kw)
            if not stepwise:
                assert n == 1, (cfg_name, solver, n)
            err = rel_err(box["one"].cpu().numpy(), loop.cpu().numpy())
            print(f"[solvers] {cfg_name} {solver} {precision} one enqueue vs the Python loop: {err:.3e}")
            assert err <= 1e-5, (cfg_name, solver, err)


@pytest.mark.gpu
def test_agent_sample_loop_runs_each_solver_as_one_launch():
    """BesoAgent.sample_loop with the sampler types of the six solvers: one fused launch each (kitchen bf16, B = 64)."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    cfg = O.KITCHEN
    agent = build_agent(cfg, lambda: make_module(cfg, "bf16"), device=DEV)
    agent.model.eval()
    s_np, g_np, x_np = O.make_inputs(cfg, 64, seed=41)
    sig = ks.get_sigmas_exponential(5, 0.05, 1.0).to(DEV)
    with torch.no_grad():
        for sampler_type in ("dpm", "ancestral", "lms", "dpmpp_2s", "dpmpp_2s_ancestral", "dpmpp_2m"):
            box = {}
            n = count_site_launches("fused_layer", lambda: box.__setitem__("x", agent.sample_loop(sig, to_dev(x_np), to_dev(s_np), to_dev(g_np), sampler_type)))
            assert n == 1, (sampler_type, n)
            assert torch.isfinite(box["x"]).all() and box["x"].shape == (64, cfg.obs_seq_len, cfg.act_dim)


class _IdentityScaler:
    def clip_output(self, x):
        return x


@pytest.mark.gpu
def test_fallbacks_keep_the_python_loop_off_the_runtime_sampler(monkeypatch):
    """s_churn > 0, a scaler, a callback, LMS of order 5 and non-empty extra_args keep today's Python loop: no call reaches
    the fused sampler (ScoreNetRuntime.sample), the fused kernel runs one plain forward per evaluation, and the result equals
    the loop bit for bit."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    from beso_amd.runtime import ScoreNetRuntime as Runtime
    calls = []
    real = Runtime.sample
    monkeypatch.setattr(Runtime, "sample", lambda self, *a, **k: calls.append(a[1]) or real(self, *a, **k))
    cfg = O.KITCHEN
    m = make_module(cfg, "bf16")
    s_np, g_np, x_np = O.make_inputs(cfg, 64, seed=51)
    sig = ks.get_sigmas_exponential(4, 0.05, 1.0)
    noop = lambda d: None        # noqa: E731
    cases = [(ks.sample_dpm_2, dict(s_churn=1.0), 7), (ks.sample_dpm_2_ancestral, dict(scaler=_IdentityScaler()), 7),
             (ks.sample_dpmpp_2s, dict(callback=noop), 7), (ks.sample_dpmpp_2s_ancestral, dict(scaler=_IdentityScaler()), 7),
             (ks.sample_dpmpp_2m, dict(callback=noop), 4), (ks.sample_lms, dict(order=5), 4),
             (ks.sample_lms, dict(extra_args={"uncond": False}), 4)]
    with torch.no_grad():
        for fn, kw, evals in cases:
            torch.manual_seed(3)
            box = {}
            n = count_site_launches("fused_layer", lambda: box.__setitem__("x", fn(m, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True, **kw)))
            torch.manual_seed(3)
            loop_kw = dict(kw, callback=noop) if "extra_args" not in kw else kw
            ref = fn(m, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True, **loop_kw)
            assert not calls, (fn.__name__, kw, calls)
            assert n == evals, (fn.__name__, kw, n)
            assert torch.equal(box["x"], ref), (fn.__name__, kw)
    # ... and the plain call does reach it
    with torch.no_grad():
        ks.sample_lms(m, to_dev(s_np), to_dev(x_np), to_dev(g_np), sig, disable=True)
    assert calls == ["lms"]


@pytest.mark.gpu
def test_solvers_are_deterministic():
    """Two identical calls give equal bits (one launch at B = 1100 and B = 64, kitchen bf16; the ancestral noise injected)."""
    from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
    cfg = O.KITCHEN
    m = make_module(cfg, "bf16")
    for B in (64, 1100):
        s_np, g_np, x_np = O.make_inputs(cfg, B, seed=61)
        s, g, x = to_dev(s_np), to_dev(g_np), to_dev(x_np)
        sig = ks.get_sigmas_exponential(7, 0.05, 1.0)
        nz = torch.randn((7,) + tuple(x.shape), device=DEV, generator=torch.Generator(DEV).manual_seed(9))
        with torch.no_grad():
            for solver in SOLVERS:
                a = m.fused_sampler(solver, s, x, g, sig, noise=nz)
                b = m.fused_sampler(solver, s, x, g, sig, noise=nz)
                assert torch.equal(a, b), (B, solver)
