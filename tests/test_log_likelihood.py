"""log_likelihood and the input vector-Jacobian product of GCDenoiser (beso_denoise_vjp).

CPU: the private dopri5 integrator and the log-likelihood ODE driver on closed forms, the C ABI's argument checks.
GPU: denoise_vjp against torch autograd over the comparator of tests/autograd_reference.py (Karras preconditioning around
forward_autograd), a finite difference, determinism, and log_likelihood against a closed form and a fixed-step fp64 RK4."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import rel_err
from support import lib, make_denoiser  # noqa: F401
from beso_amd import _lib
from beso_amd.runtime import ScoreNetShape
from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VJP = {"fp32": 2e-4, "bf16": 2.6e-2}         # the bounds of the training-gradient tests
PLANS = {"default": 0, "tiles": _lib.TRAIN_PLAN_TILES, "per_op": _lib.TRAIN_PLAN_PER_OP}


# ------------------------------------------------------------------------------------------------ CPU
def test_dopri5_on_a_closed_form_tuple_ode():
    """y' = -t y (tensor), l' = cos t (vector): y(2) = y0 e^-2, l(2) = sin 2."""
    torch.manual_seed(0)
    y0 = (torch.randn(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    fn = lambda t, y: (-t * y[0], torch.full((3,), math.cos(t), dtype=torch.float64))
    tol = 1e-6
    (y, l), st = ks._dopri5(fn, y0, 0.0, 2.0, tol, tol)
    err_y = float(((y - y0[0] * math.exp(-2.0)).abs() / (tol + tol * y.abs())).max())
    err_l = float(((l - math.sin(2.0)).abs() / (tol + tol * l.abs())).max())
    assert err_y < 10 and err_l < 10, (err_y, err_l)
    # two evaluations to choose the first step (f(t0) is the first stage of step 1), then six per attempted step (FSAL)
    assert st["steps"] >= 1 and st["fevals"] == 2 + 6 * (st["steps"] + st["rejected"])


def _gaussian_closed_form(x0, s_min, s_max, sd):
    n = x0[0].numel()
    s0, s1 = s_min ** 2 + sd ** 2, s_max ** 2 + sd ** 2
    lat = x0 * math.sqrt(s1 / s0)
    return torch.distributions.Normal(0, s_max).log_prob(lat).flatten(1).sum(1) + n / 2 * math.log(s1 / s0)


def test_log_likelihood_ode_on_the_gaussian_flow():
    """F = 0: D(x) = c_skip x, so dx/dsigma = x sigma / (sigma^2 + sd^2) and Hutchinson's trace is exact."""
    torch.manual_seed(1)
    sd, s_min, s_max = 0.5, 0.005, 1.0
    x0 = torch.randn(64, 4, 9, dtype=torch.float64) * 0.1
    n = x0[0].numel()
    rhs = lambda x, s: (x * (s / (s * s + sd * sd)), x.new_full((x.shape[0],), n * s / (s * s + sd * sd)))
    ll, _, st = ks._log_likelihood_ode(rhs, x0, s_min, s_max, 1e-6, 1e-6)
    ref = _gaussian_closed_form(x0, s_min, s_max, sd)
    assert float(((ll - ref).abs() / ref.abs()).max()) < 1e-4
    assert st["fevals"] == 2 + 6 * (st["steps"] + st["rejected"])


def test_log_likelihood_rejects_models_without_the_hip_vjp():
    model = lambda state, action, goal, sigma, **kw: action
    x = torch.zeros(2, 3, 4)
    with pytest.raises(NotImplementedError):
        ks.log_likelihood(model, torch.zeros(2, 3, 5), x, None, 0.01, 1.0)


def test_denoise_vjp_is_exported_and_checks_its_arguments(lib):
    from beso_amd.build import LIB
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "beso_denoise_vjp" in out.split()
    assert "beso_denoise_vjp" in _lib.EXPORTS
    assert "int beso_denoise_vjp(" in open(os.path.join(ROOT, "include", "beso_hip.h")).read()
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()
    n = lib.beso_num_params(C.byref(cfg))
    one = C.c_void_p(16)
    arr = (C.c_void_p * n)(*([16] * n))
    big = 1 << 40
    f = lib.beso_denoise_vjp

    def call(**kw):
        a = dict(cfg=C.byref(cfg), params=arr, n=n, prec=0, state=one, x=one, goal=one, sigma=one, cot=one, den=one, xg=one,
                 dot=None, batch=2, t=2, flags=0, ws=one, wsb=big, stream=None)
        a.update(kw)
        return f(*a.values())

    assert call(t=9) == -2 and call(batch=0) == -2                       # t > obs_seq_len, batch < 1
    for k in ("params", "state", "x", "sigma", "cot", "den", "xg", "ws", "goal"):
        assert call(**{k: None}) == -3, k
    assert call(n=n - 1) == -3
    assert call(prec=7) == -3
    assert call(flags=_lib.TRAIN_LAST_ACTION_ONLY) == -3 and call(flags=8) == -3
    assert call(wsb=16) == -4
    odd = ScoreNetShape(7, 3, 36, 2, 6, 2, 3, True, 0.5).c_struct()        # embed_dim % 8 != 0
    arr2 = (C.c_void_p * lib.beso_num_params(C.byref(odd)))(*([16] * lib.beso_num_params(C.byref(odd))))
    assert call(cfg=C.byref(odd), params=arr2, n=len(arr2)) == -5


# ------------------------------------------------------------------------------------------------ GPU helpers
def make_module(cfg, precision="fp32", seed=0, std=0.02, device=DEV):
    return make_denoiser(cfg, O.make_weights(cfg, seed=seed, std=std), precision, device=device)


def den_autograd(m, state, x, goal, sigma, uncond=False):
    """GCDenoiser.forward over the autograd comparator (Karras preconditioning around forward_autograd)."""
    from autograd_reference import forward_autograd
    c_skip, c_out, c_in = (c.reshape(-1, 1, 1) for c in m.get_scalings(sigma))
    return c_skip * x + c_out * forward_autograd(m.inner_model, state, x * c_in, goal, sigma, uncond)


def vjp_autograd(m, state, x, goal, sigma, u, uncond=False, lam=None):
    with torch.enable_grad():
        x = x.detach().clone().requires_grad_()
        if lam is None:
            den = den_autograd(m, state, x, goal, sigma, uncond)
        else:
            den = lam * den_autograd(m, state, x, goal, sigma) + (1 - lam) * den_autograd(m, state, x, goal, sigma, True)
        g, = torch.autograd.grad(den, x, u)
    return den.detach(), g


def inputs(cfg, B, t, seed, device=DEV):
    s, g, x = O.make_inputs(cfg, B, seed=seed, t=t)
    rng = np.random.default_rng(seed)
    sig = np.exp(rng.uniform(np.log(0.02), np.log(2.0), B)).astype(np.float32)
    u = rng.standard_normal(x.shape).astype(np.float32)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return T(s), T(x), T(g), T(sig), T(u)


class _CastSigma(torch.nn.Module):
    """forward_autograd feeds sigma_emb fp32; the fp64 copy takes fp64."""
    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, v):
        return self.lin(v.to(self.lin.weight.dtype))


def cpu_fp64(m, cfg):
    c = make_module(cfg, "fp32", device="cpu")
    c.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    c = c.double()
    c.inner_model.sigma_emb = _CastSigma(c.inner_model.sigma_emb)
    return c


def rk4_ll(m64, state, x0, goal, v, s_min, s_max, steps=400, lam=None):
    """Fixed-step fp64 RK4 in log sigma over the autograd comparator: the reference's ODE with the same v."""
    def rhs(x, sig):
        sv = torch.full((x.shape[0],), sig, dtype=torch.float64)
        den, g = vjp_autograd(m64, state, x, goal, sv, v, lam=lam)
        d = (x - den) / sig
        dll = ((v * v).flatten(1).sum(1) - (v * g).flatten(1).sum(1)) / sig
        return d * sig, dll * sig                     # d/d(log sigma)
    a, b = math.log(s_min), math.log(s_max)
    h = (b - a) / steps
    x, ll = x0.clone(), torch.zeros(x0.shape[0], dtype=torch.float64)
    for i in range(steps):
        s = a + i * h
        k1 = rhs(x, math.exp(s))
        k2 = rhs(x + 0.5 * h * k1[0], math.exp(s + 0.5 * h))
        k3 = rhs(x + 0.5 * h * k2[0], math.exp(s + 0.5 * h))
        k4 = rhs(x + h * k3[0], math.exp(s + h))
        x = x + h / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0])
        ll = ll + h / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1])
    return torch.distributions.Normal(0, s_max).log_prob(x).flatten(1).sum(1) + ll


# ------------------------------------------------------------------------------------------------ GPU
VJP_CASES = [(c, p, pl) for c in ("kitchen", "block_push", "long_horizon", "tiny", "tiny_mlp_head", "tiny_nogoal")
             for p, pls in (("fp32", ("default",)), ("bf16", ("default", "tiles", "per_op"))) for pl in pls]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision,plan", VJP_CASES)
def test_denoise_vjp_against_autograd(cfg_name, precision, plan):
    from beso_amd.runtime import plan as run_plan
    cfg = O.CONFIGS[cfg_name]
    m = make_module(cfg, precision)
    W = cfg.obs_seq_len
    for t in sorted({max(1, W - 1), W}):
        for uncond in (False, True):
            s, x, g, sig, u = inputs(cfg, 6, t, seed=t)
            with torch.no_grad(), run_plan(train=PLANS[plan]):
                den, xg, dot = m.denoise_vjp(s, x, g, sig, u, uncond=uncond)
                fwd = m(s, x, g, sig, uncond=uncond)
            ref_den, ref_g = vjp_autograd(m, s, x, g, sig, u, uncond)
            e_g, e_d, e_f = rel_err(xg.cpu(), ref_g.cpu()), rel_err(den.cpu(), ref_den.cpu()), rel_err(den.cpu(), fwd.cpu())
            print(f"{cfg_name} {precision} {plan} t={t} uncond={uncond}: x_grad {e_g:.2e} denoised {e_d:.2e} vs forward {e_f:.2e}")
            assert e_g <= TOL_VJP[precision] and e_d <= TOL_VJP[precision] and e_f <= TOL_VJP[precision]
            ref_dot = (u.double() * xg.double()).flatten(1).sum(1)
            assert rel_err(dot.cpu(), ref_dot.cpu()) < 1e-5


@pytest.mark.gpu
def test_denoise_vjp_finite_difference_determinism_and_no_grads():
    cfg = O.KITCHEN
    m = make_module(cfg, "fp32", std=0.05)
    s, x, g, sig, u = inputs(cfg, 4, cfg.obs_seq_len, seed=3)
    delta = torch.randn_like(x, generator=torch.Generator(DEV).manual_seed(4))
    assert all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        den, xg, dot = m.denoise_vjp(s, x, g, sig, u)
        den2, xg2, dot2 = m.denoise_vjp(s, x, g, sig, u)
        eps = 1e-2
        dp = m.denoise_vjp(s, x + eps * delta, g, sig, u)[0]
        dm = m.denoise_vjp(s, x - eps * delta, g, sig, u)[0]
    assert torch.equal(den, den2) and torch.equal(xg, xg2) and torch.equal(dot, dot2)
    lhs = float((delta.double() * xg.double()).sum())
    rhs = float((u.double() * (dp.double() - dm.double())).sum() / (2 * eps))
    print(f"finite difference: {lhs:.6e} vs {rhs:.6e}")
    assert abs(lhs - rhs) <= 1e-3 * abs(rhs)
    assert all(p.grad is None for p in m.parameters())
    # parameters that do not require grad, and autograd enabled: the same bits
    for p in m.parameters():
        p.requires_grad_(False)
    den3, xg3, _ = m.denoise_vjp(s, x, g, sig, u)
    assert torch.equal(den, den3) and torch.equal(xg, xg3)


@pytest.mark.gpu
def test_denoise_vjp_refuses_training_mode_dropout():
    from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT
    from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser
    cfg = O.TINY
    inner = DiffusionGPT(state_dim=cfg.obs_dim, device=DEV, goal_conditioned=True, action_dim=cfg.act_dim,
                         embed_dim=cfg.embed_dim, embed_pdrob=0.1, attn_pdrop=0.1, resid_pdrop=0.1, n_layers=cfg.n_layers,
                         n_heads=cfg.n_heads, goal_seq_len=cfg.goal_seq_len, obs_seq_len=cfg.obs_seq_len,
                         sigma_vocab_size=3, time_embedding_fn=None, linear_output=True, precision="fp32")
    m = GCDenoiser(inner, sigma_data=cfg.sigma_data).to(DEV).train()
    s, x, g, sig, u = inputs(cfg, 2, cfg.obs_seq_len, seed=0)
    with pytest.raises(RuntimeError):
        m.denoise_vjp(s, x, g, sig, u)
    m.eval()
    m.denoise_vjp(s, x, g, sig, u)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_log_likelihood_is_exact_on_the_gaussian_flow(precision):
    cfg = O.KITCHEN
    m = make_module(cfg, precision)
    head = m.inner_model.action_pred
    last = head if isinstance(head, torch.nn.Linear) else head[-1]
    with torch.no_grad():
        last.weight.zero_()
        last.bias.zero_()
    s, x, g, _, _ = inputs(cfg, 64, cfg.obs_seq_len, seed=5)
    x = x * 0.1
    torch.manual_seed(0)
    ll, info = ks.log_likelihood(m, s, x, g, 0.005, 1.0, atol=1e-6, rtol=1e-6)
    ref = _gaussian_closed_form(x.double().cpu(), 0.005, 1.0, cfg.sigma_data)
    err = float(((ll.double().cpu() - ref).abs() / ref.abs()).max())
    print(f"gaussian flow [{precision}]: max rel err {err:.2e}, fevals {info['fevals']}")
    assert err < 1e-4


@pytest.mark.gpu
def test_log_likelihood_of_a_random_network_against_fp64_rk4():
    cfg = O.KITCHEN
    s, x, g, _, _ = inputs(cfg, 4, cfg.obs_seq_len, seed=6)
    x = x * 0.2
    torch.manual_seed(11)
    v = torch.randint_like(x, 2) * 2 - 1                 # the draw log_likelihood makes after the same reseed
    m32 = make_module(cfg, "fp32", std=0.05)
    ref = rk4_ll(cpu_fp64(m32, cfg), s.double().cpu(), x.double().cpu(), g.double().cpu(), v.double().cpu(), 0.005, 1.0)
    for precision in ("fp32", "bf16"):
        m = m32 if precision == "fp32" else make_module(cfg, "bf16", std=0.05)
        torch.manual_seed(11)
        ll, info = ks.log_likelihood(m, s, x, g, 0.005, 1.0, atol=1e-5, rtol=1e-5)
        dev = float(((ll.double().cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print(f"random network [{precision}]: ll {ll.cpu().numpy()}, rk4 {ref.numpy()}, max deviation {dev:.2e}, "
              f"fevals {info['fevals']}")
        if precision == "fp32":
            assert dev <= 1e-3


@pytest.mark.gpu
def test_log_likelihood_with_classifier_free_guidance():
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    cfg, lam = O.TINY, 1.5
    m = make_module(cfg, "fp32", std=0.1)
    cf = ClassifierFreeSampleModel(m, lam)
    s, x, g, sig, u = inputs(cfg, 4, cfg.obs_seq_len, seed=7)
    with torch.no_grad():
        dc, gc, tc = m.denoise_vjp(s, x, g, sig, u)
        du, gu, tu = m.denoise_vjp(s, x, g, sig, u, uncond=True)
    ref_den, ref_g = vjp_autograd(m, s, x, g, sig, u, lam=lam)
    assert rel_err((lam * dc + (1 - lam) * du).cpu(), ref_den.cpu()) <= TOL_VJP["fp32"]
    assert rel_err((lam * gc + (1 - lam) * gu).cpu(), ref_g.cpu()) <= TOL_VJP["fp32"]
    torch.manual_seed(12)
    v = torch.randint_like(x, 2) * 2 - 1
    ref = rk4_ll(cpu_fp64(m, cfg), s.double().cpu(), x.double().cpu(), g.double().cpu(), v.double().cpu(), 0.01, 1.0, lam=lam)
    torch.manual_seed(12)
    ll, info = ks.log_likelihood(cf, s, x, g, 0.01, 1.0, atol=1e-5, rtol=1e-5)
    dev = float(((ll.double().cpu() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print(f"cfg lam={lam}: max deviation {dev:.2e}, fevals {info['fevals']}")
    assert dev <= 1e-3
