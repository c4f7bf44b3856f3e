"""Drop-in for ``beso...k_diffusion.gc_sampling``: noise schedules and the iterative samplers of the
goal-conditioned score model (reference: gc_sampling.py).

Signature of every sampler, as in the reference:
    sample_X(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
             disable=None, ...) -> action
where ``model(state, action, goal, sigma[B], **extra_args) -> [B, t, act]``.

MI355X-first differences that do not change results:
  * the sigma schedule is read back to the HOST once and all step coefficients are computed there
    as fp32 scalars, so the loop never branches on a device tensor (the reference syncs on every
    ``sigmas[i + 1] == 0`` / ``s_tmin <= sigmas[i]`` test: gc_sampling.py:198,289,301,360);
  * when ``model`` is a ``beso_amd`` GCDenoiser (optionally inside ClassifierFreeSampleModel) and the
    call is the plain one (no churn, no callback, no scaler, no extra args), ddim / euler / heun / euler_ancestral / dpm_2 /
    dpm_2_ancestral / dpmpp_2s / dpmpp_2s_ancestral / dpmpp_2m / lms run as ONE enqueue of the whole loop
    (``GCDenoiser.fused_sampler``, include/beso_hip.h) -- otherwise the generic loops below call ``model`` once per evaluation.
"""
import math

import numpy as np
import torch
from scipy import integrate

from . import utils
from .classifier_free_sampler import ClassifierFreeSampleModel
from .score_wrappers import GCDenoiser

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# noise schedules (gc_sampling.py:22-95): n values + a trailing zero, fp32
# ------------------------------------------------------------------------------------------------
def append_zero(action):
    return torch.cat([action, action.new_zeros([1])])


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7., device='cpu'):
    """Karras et al. (2022) schedule (:26-32)."""
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return append_zero((hi + torch.linspace(0, 1, n) * (lo - hi)) ** rho).to(device)


def get_sigmas_exponential(n, sigma_min, sigma_max, device='cpu'):
    """Log-linear schedule (:35-38)."""
    return append_zero(torch.linspace(math.log(sigma_max), math.log(sigma_min), n, device=device).exp())


def get_sigmas_linear(n, sigma_min, sigma_max, device='cpu'):
    """Linear schedule (:41-44)."""
    return append_zero(torch.linspace(sigma_max, sigma_min, n, device=device))


def cosine_beta_schedule(n, s=0.008, device='cpu'):
    """Cosine beta schedule (:47-58)."""
    steps = n + 1
    grid = np.linspace(0, steps, steps)
    abar = np.cos(((grid / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    abar = abar / abar[0]
    betas = np.clip(1 - abar[1:] / abar[:-1], a_min=0, a_max=0.999)
    return append_zero(torch.tensor(np.flip(betas).copy(), device=device, dtype=torch.float32))


def get_sigmas_ve(n, sigma_min=0.02, sigma_max=100, device='cpu'):
    """(:61-68)"""
    t = torch.linspace(0, n + 1, n, device=device)
    return append_zero(torch.sqrt((sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (t / (n - 1)))))


def get_iddpm_sigmas(n, sigma_min=0.02, sigma_max=100, M=1000, j_0=0, C_1=0.001, C_2=0.008, device='cpu'):
    """(:71-81)"""
    idx = torch.arange(n, dtype=torch.float64, device=device)
    u = torch.zeros(M + 1, dtype=torch.float64, device=device)
    abar = lambda j: (0.5 * np.pi * j / M / (C_2 + 1)).sin() ** 2        # noqa: E731
    for j in torch.arange(M, j_0, -1, device=device):
        u[j - 1] = ((u[j] ** 2 + 1) / (abar(j - 1) / abar(j)).clip(min=C_1) - 1).sqrt()
    u = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
    return append_zero(u[((len(u) - 1) / (n - 1) * idx).round().to(torch.int64)]).to(torch.float32)


def get_sigmas_vp(n, beta_d=19.9, beta_min=0.1, eps_s=1e-3, device='cpu'):
    """(:84-88)"""
    t = torch.linspace(1, eps_s, n, device=device)
    return append_zero(torch.sqrt(torch.exp(beta_d * t ** 2 / 2 + beta_min * t) - 1))


def get_sigmas_polyexponential(n, sigma_min, sigma_max, rho=1., device='cpu'):
    """(:91-95)"""
    ramp = torch.linspace(1, 0, n, device=device) ** rho
    return append_zero(torch.exp(ramp * (math.log(sigma_max) - math.log(sigma_min)) + math.log(sigma_min)))


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def to_d(action, sigma, denoised):
    """Karras ODE derivative (x - D(x)) / sigma (:98-100)."""
    if not torch.is_tensor(sigma):
        return (action - denoised) / float(sigma)
    return (action - denoised) / utils.append_dims(sigma, action.ndim)


def default_noise_sampler(x):
    return lambda sigma, sigma_next: torch.randn_like(x)


def get_ancestral_step(sigma_from, sigma_to, eta=1.):
    """sigma_down / sigma_up of an ancestral step (:107-114), fp32 scalars."""
    if not eta:
        return sigma_to, 0.
    sf, st = f32(sigma_from), f32(sigma_to)
    up = min(st, f32(eta) * (st ** 2 * (sf ** 2 - st ** 2) / sf ** 2) ** f32(0.5))
    down = (st ** 2 - up ** 2) ** f32(0.5)
    return f32(down), f32(up)


def _host_sigmas(sigmas):
    """The schedule as host fp32 scalars: the single device->host read of a sampling loop."""
    if torch.is_tensor(sigmas):
        return sigmas.detach().to('cpu', torch.float32).numpy()
    return np.asarray(sigmas, dtype=np.float32)


def _sig_vec(action, value):
    return action.new_full([action.shape[0]], float(value))


def _neg_log(s):
    with np.errstate(divide='ignore'):
        return -np.log(f32(s))


def _fused_target(model):
    """(GCDenoiser, cond_lambda) when ``model`` is one the HIP sampler loop understands."""
    if isinstance(model, GCDenoiser):
        return model, 1.0
    if isinstance(model, ClassifierFreeSampleModel) and isinstance(model.model, GCDenoiser):
        return model.model, float(model.cond_lambda)
    return None, None


def _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback):
    """(GCDenoiser, cond_lambda, host sigmas) when a sampler call can run as one enqueue (``GCDenoiser.fused_sampler``), else
    None: the plain call (no scaler, callback or extra_args) on a ``beso_amd`` denoiser whose inputs it runs, with a schedule
    that is positive up to its trailing value (get_sigmas_linear(sigma_min=0), the clipped cosine_beta: the Python loop serves
    them).  Each sampler adds its own conditions.  Checked before anything is drawn: the ancestral samplers pre-draw their
    noise only for a call that takes this path."""
    if scaler is not None or callback is not None or extra_args:
        return None
    den, lam = _fused_target(model)
    if den is None or not action.is_cuda or not den.can_fuse_sampler(state, action, goal):
        return None
    sig = _host_sigmas(sigmas)
    if len(sig) < 2 or not all(float(v) > 0.0 for v in sig[:-1]):
        return None
    return den, lam, sig


class keyed_step_noise:
    """``with keyed_step_noise(noise):`` -- the sampler calls inside draw nothing from the global generator: an ancestral sampler
    on its one-enqueue path takes `noise` [n_steps, *action.shape] (the rollout's keyed draws, beso_amd/noise.py; None: the
    step drew none) as its step noise, and a call that would draw inside a Python loop raises ValueError naming the sampler.
    One context per thread of control; only the branches below consult it, and without one everything draws as it always has."""
    active = None

    def __init__(self, noise):
        self.noise = noise

    def __enter__(self):
        if keyed_step_noise.active is not None:
            raise RuntimeError("keyed_step_noise contexts do not nest")
        keyed_step_noise.active = self
        return self

    def __exit__(self, *exc):
        keyed_step_noise.active = None
        return False


def _keyed_noise(sampler):
    """The active keyed context's step noise for the one-enqueue path of `sampler`, None without a context."""
    ctx = keyed_step_noise.active
    if ctx is None:
        return None
    if ctx.noise is None:
        raise ValueError(f"keyed noise: sampler {sampler!r} needs step noise and the keyed step drew none")
    return ctx.noise


_OFF_FUSED = 'is off its one-enqueue path (a scaler, callback, extra_args, eta < 0, or inputs the fused loop does not run)'


def _refuse_keyed(sampler, why):
    """ValueError inside a keyed context for a call that is about to draw from the global generator; nothing otherwise."""
    if keyed_step_noise.active is not None:
        raise ValueError(f"keyed noise: sampler {sampler!r} {why}: it would draw from the global generator inside a Python "
                         "loop, and a seeded rollout makes no unkeyed draws")


def predraw_noise(sampler, sig, action, eta, noise_sampler=None, noise=None):
    """The draws of an ancestral sampler's loop made up front for its one enqueue, in the loop's order and number:
    [len(sig) - 1, *action.shape], zero where a step draws nothing.  dpmpp_2s_ancestral draws on every step (through
    ``noise_sampler``), euler_ancestral and dpm_2_ancestral on the steps whose sigma_down != 0 (``get_ancestral_step``).
    ``noise``: draws made elsewhere, of that shape; they are returned as they are and nothing is drawn here (the entries of
    steps that draw nothing are not read by the enqueue: include/beso_hip.h)."""
    if noise is not None:
        want = (len(sig) - 1,) + tuple(action.shape)
        if tuple(noise.shape) != want or noise.dtype != torch.float32 or noise.device != action.device:
            raise ValueError(f"predraw_noise: noise must be float32 {want} on {action.device}, got {noise.dtype} "
                             f"{tuple(noise.shape)} on {noise.device}")
        return noise
    noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
    noise = torch.zeros((len(sig) - 1,) + tuple(action.shape), dtype=torch.float32, device=action.device)
    for i in range(len(sig) - 1):
        if sampler == 'dpmpp_2s_ancestral' or get_ancestral_step(sig[i], sig[i + 1], eta=eta)[0] != 0:
            noise[i] = noise_sampler(sig[i], sig[i + 1])
    return noise


def _churn(i, n, sig, s_churn, s_tmin, s_tmax):
    gamma = min(s_churn / n, 2 ** 0.5 - 1) if s_tmin <= sig[i] <= s_tmax else 0.
    return gamma, f32(sig[i] * f32(gamma + 1))


# ------------------------------------------------------------------------------------------------
# samplers
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def sample_euler(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                 s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """Algorithm 2 of Karras et al. (2022) without the second-order correction (:167-213).
    The generic loop draws ``eps`` every step like the reference (:199), used or not; the fused
    loop draws nothing (with s_churn = 0 the draws never enter the result)."""
    extra_args = {} if extra_args is None else extra_args
    tgt = None if s_churn else _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('euler', state, action, goal, sig, cond_lambda=lam)
    if s_churn:
        _refuse_keyed('euler', 'with s_churn > 0')
    sig = _host_sigmas(sigmas)
    n = len(sig) - 1
    for i in range(n):
        gamma, sigma_hat = _churn(i, n, sig, s_churn, s_tmin, s_tmax)
        eps = torch.randn_like(action) * s_noise
        if gamma > 0:
            action = action + eps * float((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
        denoised = model(state, action, goal, _sig_vec(action, sigma_hat), **extra_args)
        d = to_d(action, sigma_hat, denoised)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
        action = action + d * float(sig[i + 1] - sigma_hat)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_euler_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                           disable=None, eta=1.):
    """Euler steps to sigma_down, then fresh noise of scale sigma_up (:216-256).  The plain call on a ``beso_amd``
    denoiser runs as one enqueue (``beso_sample_ancestral``) with the same sequence of ``randn_like`` draws."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback) if eta >= 0 else None
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('euler_ancestral', state, action, goal, sig, cond_lambda=lam, eta=eta,
                                 noise=predraw_noise('euler_ancestral', sig, action, eta, noise=_keyed_noise('euler_ancestral')))
    _refuse_keyed('euler_ancestral', _OFF_FUSED)
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        d = to_d(action, sig[i], denoised)
        action = action + d * float(sigma_down - sig[i])
        if sigma_down > 0:
            action = action + torch.randn_like(action) * float(sigma_up)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_heun(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """Algorithm 2 of Karras et al. (2022): Euler predictor + trapezoid corrector; the last step
    (sigma_next == 0) is plain Euler (:259-314)."""
    extra_args = {} if extra_args is None else extra_args
    tgt = None if s_churn else _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('heun', state, action, goal, sig, cond_lambda=lam)
    if s_churn:
        _refuse_keyed('heun', 'with s_churn > 0')
    sig = _host_sigmas(sigmas)
    n = len(sig) - 1
    for i in range(n):
        gamma, sigma_hat = _churn(i, n, sig, s_churn, s_tmin, s_tmax)
        eps = torch.randn_like(action) * s_noise
        if gamma > 0:
            action = action + eps * float((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
        denoised = model(state, action, goal, _sig_vec(action, sigma_hat), **extra_args)
        d = to_d(action, sigma_hat, denoised)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
        dt = float(sig[i + 1] - sigma_hat)
        if sig[i + 1] == 0:
            action = action + d * dt
        else:
            action_2 = action + d * dt
            denoised_2 = model(state, action_2, goal, _sig_vec(action, sig[i + 1]), **extra_args)
            d_2 = to_d(action_2, sig[i + 1], denoised_2)
            action = action + (d + d_2) / 2 * dt
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


def _log_midpoint(a, b):
    la, lb = np.log(f32(a)), np.log(f32(b))
    return f32(np.exp(f32(la + f32(0.5) * (lb - la))))        # torch.lerp(a, b, 0.5) = a + 0.5 (b - a)


@torch.no_grad()
def sample_dpm_2(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                 s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """DPM-Solver-2-like midpoint steps in log sigma (:317-375).  With s_churn = 0 the plain call on a ``beso_amd`` denoiser
    runs as one enqueue (``beso_sample_solver``; the generic loop's unused ``eps`` draws are not made)."""
    extra_args = {} if extra_args is None else extra_args
    tgt = None if s_churn else _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('dpm_2', state, action, goal, sig, cond_lambda=lam)
    if s_churn:
        _refuse_keyed('dpm_2', 'with s_churn > 0')
    sig = _host_sigmas(sigmas)
    n = len(sig) - 1
    for i in range(n):
        gamma, sigma_hat = _churn(i, n, sig, s_churn, s_tmin, s_tmax)
        eps = torch.randn_like(action) * s_noise
        if gamma > 0:
            action = action + eps * float((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
        denoised = model(state, action, goal, _sig_vec(action, sigma_hat), **extra_args)
        d = to_d(action, sigma_hat, denoised)
        if callback is not None:
            callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
        if sig[i + 1] == 0:
            action = action + d * float(sig[i + 1] - sigma_hat)
        else:
            sigma_mid = _log_midpoint(sigma_hat, sig[i + 1])
            action_2 = action + d * float(sigma_mid - sigma_hat)
            denoised_2 = model(state, action_2, goal, _sig_vec(action, sigma_mid), **extra_args)
            d_2 = to_d(action_2, sigma_mid, denoised_2)
            action = action + d_2 * float(sig[i + 1] - sigma_hat)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_dpm_2_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                           disable=None, eta=1.):
    """Ancestral variant of the DPM-Solver-2-like sampler (:378-413).  The plain call on a ``beso_amd`` denoiser runs as one
    enqueue (``beso_sample_solver``) with the loop's ``randn_like`` draws made up front, in the same order and number."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback) if eta >= 0 else None
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('dpm_2_ancestral', state, action, goal, sig, cond_lambda=lam, eta=eta,
                                 noise=predraw_noise('dpm_2_ancestral', sig, action, eta, noise=_keyed_noise('dpm_2_ancestral')))
    _refuse_keyed('dpm_2_ancestral', _OFF_FUSED)
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        d = to_d(action, sig[i], denoised)
        if sigma_down == 0:
            action = action + d * float(sigma_down - sig[i])
        else:
            sigma_mid = _log_midpoint(sig[i], sigma_down)
            action_2 = action + d * float(sigma_mid - sig[i])
            denoised_2 = model(state, action_2, goal, _sig_vec(action, sigma_mid), **extra_args)
            d_2 = to_d(action_2, sigma_mid, denoised_2)
            action = action + d_2 * float(sigma_down - sig[i])
            action = action + torch.randn_like(action) * float(sigma_up)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


def linear_multistep_coeff(order, t, i, j):
    """Adams-Bashforth-style coefficient of the j-th stored derivative at step i (:416-429)."""
    if order - 1 > i:
        raise ValueError(f'Order {order} too high for step {i}')

    def basis(tau):
        prod = 1.
        for k in range(order):
            if k != j:
                prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
        return prod
    return integrate.quad(basis, t[i], t[i + 1], epsrel=1e-4)[0]


@torch.no_grad()
def sample_lms(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
               order=4):
    """Linear multistep sampler (:432-468).  Orders up to 4 on a ``beso_amd`` denoiser run as one enqueue
    (``beso_sample_solver``: the coefficients are the exact integrals that quad approximates)."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback) if 1 <= order <= 4 else None
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('lms', state, action, goal, sig, cond_lambda=lam, order=order)
    sig = _host_sigmas(sigmas)
    history = []
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        history.append(to_d(action, sig[i], denoised))
        if len(history) > order:
            history.pop(0)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        cur = min(i + 1, order)
        coeffs = [linear_multistep_coeff(cur, sig, i, j) for j in range(cur)]
        action = action + sum(c * d for c, d in zip(coeffs, reversed(history)))
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


def _exp_step_coeffs(s_from, s_to):
    """(sigma_fn(t_to)/sigma_fn(t_from), expm1(-h)) of the exponential-integrator update
    x <- ratio * x - expm1(-h) * denoised, in fp32 like the reference's 0-d tensors (:921-923)."""
    t, t_next = _neg_log(s_from), _neg_log(s_to)
    h = t_next - t
    with np.errstate(over='ignore', invalid='ignore'):
        return float(f32(np.exp(-t_next)) / f32(np.exp(-t))), float(f32(np.expm1(-h))), t, t_next, h


@torch.no_grad()
def sample_dpmpp_2m(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None):
    """DPM-Solver++(2M) (:702-736); one enqueue (``beso_sample_solver``) on a ``beso_amd`` denoiser."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('dpmpp_2m', state, action, goal, sig, cond_lambda=lam)
    sig = _host_sigmas(sigmas)
    old_denoised = None
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        if callback is not None:
            callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        ratio, em1, t, t_next, h = _exp_step_coeffs(sig[i], sig[i + 1])
        if old_denoised is None or sig[i + 1] == 0:
            action = ratio * action - em1 * denoised
        else:
            r = (t - _neg_log(sig[i - 1])) / h
            blended = float(1 + 1 / (2 * r)) * denoised - float(1 / (2 * r)) * old_denoised
            action = ratio * action - em1 * blended
        old_denoised = denoised
    return action


@torch.no_grad()
def sample_ddim(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                eta=1.):
    """DPM-Solver-1 / DDIM (:895-924).  The final step (sigma_next = 0) returns the denoised action."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, None, extra_args, callback)       # (ddim ignores the scaler)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('ddim', state, action, goal, sig, cond_lambda=lam)
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        if callback is not None:
            callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        ratio, em1, *_ = _exp_step_coeffs(sig[i], sig[i + 1])
        action = ratio * action - em1 * denoised
    return action


@torch.no_grad()
def sample_dpmpp_2s(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                    eta=1.):
    """DPM-Solver++(2S) (:928-966); one enqueue (``beso_sample_solver``) on a ``beso_amd`` denoiser."""
    extra_args = {} if extra_args is None else extra_args
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback)
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('dpmpp_2s', state, action, goal, sig, cond_lambda=lam)
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        if callback is not None:
            callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        if sig[i + 1] == 0:
            action = action + to_d(action, sig[i], denoised) * float(sig[i + 1] - sig[i])
        else:
            action = _dpmpp_2s_update(model, state, action, goal, denoised, sig[i], sig[i + 1], extra_args)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


def _dpmpp_2s_update(model, state, action, goal, denoised, s_from, s_to, extra_args):
    t, t_next = _neg_log(s_from), _neg_log(s_to)
    r = f32(0.5)
    h = t_next - t
    s = t + r * h
    x_2 = float(f32(np.exp(-s)) / f32(np.exp(-t))) * action - float(f32(np.expm1(-h * r))) * denoised
    denoised_2 = model(state, x_2, goal, _sig_vec(action, f32(np.exp(-s))), **extra_args)
    return float(f32(np.exp(-t_next)) / f32(np.exp(-t))) * action - float(f32(np.expm1(-h))) * denoised_2


@torch.no_grad()
def sample_dpmpp_2s_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                              disable=None, eta=1., s_noise=1., noise_sampler=None):
    """Ancestral DPM-Solver++(2S) (:969-1016).  The plain call on a ``beso_amd`` denoiser runs as one enqueue
    (``beso_sample_solver``) with the loop's ``noise_sampler`` calls made up front, in the same order and number."""
    extra_args = {} if extra_args is None else extra_args
    noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
    tgt = _fused_call(model, state, action, goal, sigmas, scaler, extra_args, callback) if eta >= 0 else None
    if tgt is not None:
        den, lam, sig = tgt
        return den.fused_sampler('dpmpp_2s_ancestral', state, action, goal, sig, cond_lambda=lam, eta=eta, s_noise=s_noise,
                                 noise=predraw_noise('dpmpp_2s_ancestral', sig, action, eta, noise_sampler, noise=_keyed_noise('dpmpp_2s_ancestral')))
    _refuse_keyed('dpmpp_2s_ancestral', _OFF_FUSED)
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
        if callback is not None:
            callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        if sigma_down == 0:
            action = action + to_d(action, sig[i], denoised) * float(sigma_down - sig[i])
        else:
            action = _dpmpp_2s_update(model, state, action, goal, denoised, sig[i], sigma_down, extra_args)
        action = action + noise_sampler(sig[i], sig[i + 1]) * s_noise * float(sigma_up)
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


# ------------------------------------------------------------------------------------------------
# Brownian-path noise for the SDE sampler (:117-165)
# ------------------------------------------------------------------------------------------------
class BrownianTreeNoiseSampler:
    """``sampler(sigma, sigma_next) -> (W(t1) - W(t0)) / sqrt|t1 - t0|`` with t = transform(sigma): increments of
    ONE Brownian path per sample, so that overlapping intervals are correlated the way the reference's
    torchsde-backed sampler makes them (:144-165).  torchsde is not a dependency here: the path is built lazily on
    the action's device -- W is drawn at every time that is asked for, conditioned on the values already drawn at
    its neighbours (Brownian bridge inside the known range, a free increment outside it).  Same law as a Brownian
    tree, different random numbers; ``seed`` (an int, or one int per batch row) makes it repeatable."""

    def __init__(self, x, sigma_min, sigma_max, seed=None, transform=lambda x: x):
        self.transform = transform
        self._like = x
        t0, t1 = float(transform(torch.as_tensor(sigma_min))), float(transform(torch.as_tensor(sigma_max)))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, []).item())
        try:
            seeds = [int(v) for v in seed]
            if len(seeds) != x.shape[0]:
                raise ValueError("one seed per batch row expected")
        except TypeError:
            seeds = None
        self._gens = [torch.Generator(device=x.device).manual_seed(v) for v in (seeds if seeds is not None else [int(seed)])]
        self._batched = seeds is not None
        self._times = [min(t0, t1)]                       # sorted; W(first time) = 0
        self._w = [torch.zeros_like(x)]
        self._at(max(t0, t1))

    def _randn(self):
        x = self._like
        if not self._batched:
            return torch.randn(x.shape, generator=self._gens[0], device=x.device, dtype=x.dtype)
        return torch.stack([torch.randn(x.shape[1:], generator=g, device=x.device, dtype=x.dtype) for g in self._gens])

    def _at(self, t):
        import bisect
        k = bisect.bisect_left(self._times, t)
        if k < len(self._times) and self._times[k] == t:
            return self._w[k]
        if k == 0:                                         # before the first known time
            w = self._w[0] - self._randn() * math.sqrt(self._times[0] - t)
        elif k == len(self._times):                        # beyond the last
            w = self._w[-1] + self._randn() * math.sqrt(t - self._times[-1])
        else:                                              # bridge between the neighbours
            a, b = self._times[k - 1], self._times[k]
            f = (t - a) / (b - a)
            w = torch.lerp(self._w[k - 1], self._w[k], f) + self._randn() * math.sqrt((t - a) * (b - t) / (b - a))
        self._times.insert(k, t)
        self._w.insert(k, w)
        return w

    def __call__(self, sigma, sigma_next):
        t0, t1 = float(self.transform(torch.as_tensor(sigma))), float(self.transform(torch.as_tensor(sigma_next)))
        lo, hi = min(t0, t1), max(t0, t1)
        w = self._at(hi) - self._at(lo)
        return (w if t1 >= t0 else -w) / math.sqrt(abs(t1 - t0))


# ------------------------------------------------------------------------------------------------
# DPM-Solver (:498-672): eps-prediction steps of order 1/2/3 in t = -log(sigma), fixed and adaptive step size
# ------------------------------------------------------------------------------------------------
class PIDStepSizeController:
    """Step-size controller of the adaptive solver (:498-524): h <- h * limiter(prod_k (1/err_k)^b_k)."""

    def __init__(self, h, pcoeff, icoeff, dcoeff, order=1, accept_safety=0.81, eps=1e-8):
        self.h = h
        self.b = ((pcoeff + icoeff + dcoeff) / order, -(pcoeff + 2 * dcoeff) / order, dcoeff / order)
        self.accept_safety = accept_safety
        self.eps = eps
        self.errs = []

    @staticmethod
    def limiter(x):
        return 1 + math.atan(x - 1)

    def propose_step(self, error):
        inv = 1 / (float(error) + self.eps)
        self.errs = [inv, inv, inv] if not self.errs else [inv] + self.errs[1:]
        factor = self.limiter(math.prod(e ** b for e, b in zip(self.errs, self.b)))
        accept = factor >= self.accept_safety
        if accept:
            self.errs = [self.errs[0], self.errs[0], self.errs[1]]
        self.h *= factor
        return accept


def _sigma_of(t):
    return f32(np.exp(-f32(t)))


class DPMSolver:
    """DPM-Solver steps (arXiv 2206.00927; reference :527-672).  All times are host fp32 scalars, the network is
    evaluated through ``model`` (the HIP denoiser on a GPU), the state update is a handful of axpy's on the device."""

    def __init__(self, model, extra_args=None, eps_callback=None, info_callback=None):
        self.model = model
        self.extra_args = {} if extra_args is None else extra_args
        self.eps_callback = eps_callback
        self.info_callback = info_callback

    t = staticmethod(lambda sigma: _neg_log(sigma))
    sigma = staticmethod(_sigma_of)

    def eps(self, state, action, goal, t):
        sig = _sigma_of(t)
        out = (action - self.model(state, action, goal, _sig_vec(action, sig), **self.extra_args)) / float(sig)
        if self.eps_callback is not None:
            self.eps_callback()
        return out

    def steps(self, orders, state, action, goal, t, t_next, eps, r1=None):
        """The updates of every order in ``orders`` from (action, t) to t_next, sharing the network evaluations
        (the reference's eps_cache): eps at t is given; order 2 needs eps at t + r1 h, order 3 also at t + 2/3 h."""
        h = f32(t_next - t)
        sn, em1 = float(_sigma_of(t_next)), float(f32(np.expm1(h)))
        out = {}
        if 1 in orders:
            out[1] = action - (sn * em1) * eps
        if 2 in orders or 3 in orders:
            r1 = f32(r1 if r1 is not None else (1 / 3 if 3 in orders else 1 / 2))
            s1 = f32(t + r1 * h)
            u1 = action - float(_sigma_of(s1) * f32(np.expm1(f32(r1 * h)))) * eps
            d1 = self.eps(state, u1, goal, s1) - eps
            if 2 in orders:
                out[2] = action - (sn * em1) * eps - float(f32(sn) / (2 * r1) * f32(em1)) * d1
            if 3 in orders:
                r2 = f32(2 / 3)
                s2 = f32(t + r2 * h)
                e2 = f32(np.expm1(f32(r2 * h)))
                u2 = action - float(_sigma_of(s2) * e2) * eps - float(_sigma_of(s2) * (r2 / r1) * (e2 / f32(r2 * h) - 1)) * d1
                d2 = self.eps(state, u2, goal, s2) - eps
                out[3] = action - (sn * em1) * eps - float(f32(sn) / r2 * (f32(em1) / h - 1)) * d2
        return out

    def _ancestral_target(self, t, t_next, t_end, eta):
        """(t_next_, sigma_up) of a step with added noise (:614-619)."""
        if not eta:
            return t_next, 0.
        sd, _ = get_ancestral_step(_sigma_of(t), _sigma_of(t_next), eta)
        t_down = min(f32(t_end), _neg_log(sd))
        return t_down, float((_sigma_of(t_next) ** 2 - _sigma_of(t_down) ** 2) ** f32(0.5))

    def dpm_solver_fast(self, state, action, goal, t_start, t_end, nfe, eta=0., s_noise=1., noise_sampler=None):
        # the reference draws from randn_like whatever sampler it is given (:604), also when the noise is scaled by 0
        noise_sampler = default_noise_sampler(action)
        t_start, t_end = f32(t_start), f32(t_end)
        if not t_end > t_start and eta:
            raise ValueError('eta must be 0 for reverse sampling')
        m = nfe // 3 + 1
        ts = torch.linspace(float(t_start), float(t_end), m + 1, dtype=torch.float32).numpy()
        orders = [3] * (m - 2) + [2, 1] if nfe % 3 == 0 else [3] * (m - 1) + [nfe % 3]
        for i, order in enumerate(orders):
            t, t_next = ts[i], ts[i + 1]
            t_next_, su = self._ancestral_target(t, t_next, t_end, eta)
            eps = self.eps(state, action, goal, t)
            if self.info_callback is not None:
                self.info_callback({'x': action, 'i': i, 't': t, 't_up': t, 'denoised': action - float(_sigma_of(t)) * eps})
            action = self.steps((order,), state, action, goal, t, t_next_, eps, r1=None if order == 3 else 0.5)[order]
            action = action + (su * s_noise) * noise_sampler(_sigma_of(t), _sigma_of(t_next))
        return action

    def dpm_solver_adaptive(self, state, action, goal, t_start, t_end, order=3, rtol=0.05, atol=0.0078, h_init=0.05,
                            pcoeff=0., icoeff=1., dcoeff=0., accept_safety=0.81, eta=0., s_noise=1.):
        """Embedded pairs 1/2 or 2/3 with a PID step size (:629-672).  The error norm runs over the WHOLE batch, so
        the accepted step sequence depends on which samples share a call: one device->host scalar per step."""
        noise_sampler = default_noise_sampler(action)
        if order not in {2, 3}:
            raise ValueError('order should be 2 or 3')
        t_start, t_end = f32(t_start), f32(t_end)
        forward = t_end > t_start
        if not forward and eta:
            raise ValueError('eta must be 0 for reverse sampling')
        pid = PIDStepSizeController(abs(h_init) * (1 if forward else -1), pcoeff, icoeff, dcoeff,
                                    1.5 if eta else order, accept_safety)
        info = {'steps': 0, 'nfe': 0, 'n_accept': 0, 'n_reject': 0}
        s, action_prev = t_start, action
        while (s < t_end - 1e-5) if forward else (s > t_end + 1e-5):
            t = min(t_end, f32(s + f32(pid.h))) if forward else max(t_end, f32(s + f32(pid.h)))
            t_, su = self._ancestral_target(s, t, t_end, eta)
            eps = self.eps(state, action, goal, s)
            cand = self.steps((order - 1, order), state, action, goal, s, t_, eps, r1=1 / 3 if order == 3 else 1 / 2)
            low, high = cand[order - 1], cand[order]
            delta = (rtol * torch.maximum(low.abs(), action_prev.abs())).clamp_min(atol)
            error = torch.linalg.norm((low - high) / delta) / action.numel() ** 0.5
            if pid.propose_step(error):
                action_prev = low
                action = high + (su * s_noise) * noise_sampler(_sigma_of(s), _sigma_of(t))
                s = t
                info['n_accept'] += 1
            else:
                info['n_reject'] += 1
            info['nfe'] += order
            info['steps'] += 1
            if self.info_callback is not None:
                self.info_callback({'x': action, 'i': info['steps'] - 1, 't': s, 't_up': s,
                                    'denoised': action - float(_sigma_of(s)) * eps, 'error': error, 'h': pid.h, **info})
        return action, info


def _solver(model, extra_args, callback):
    solver = DPMSolver(model, extra_args)
    if callback is not None:
        solver.info_callback = lambda info: callback({'sigma': _sigma_of(info['t']), 'sigma_hat': _sigma_of(info['t_up']), **info})
    return solver


@torch.no_grad()
def sample_dpm_fast(model, state, action, goal, sigma_min, sigma_max, n, scaler=None, extra_args=None, callback=None,
                    disable=None, eta=0., s_noise=1., noise_sampler=None):
    """DPM-Solver-fast: ``n`` network evaluations in steps of order 3, 3, ..., (2, 1 | n mod 3), uniform in
    log sigma from sigma_max to sigma_min (:675-699)."""
    if sigma_min <= 0 or sigma_max <= 0:
        raise ValueError('sigma_min and sigma_max must not be 0')
    if eta:
        _refuse_keyed('dpm_fast', 'with eta > 0')
    return _solver(model, extra_args, callback).dpm_solver_fast(
        state, action, goal, _neg_log(sigma_max), _neg_log(sigma_min), n, eta, s_noise, noise_sampler)


@torch.no_grad()
def sample_dpm_adaptive(model, state, action, goal, sigma_min, sigma_max, extra_args=None, callback=None, disable=None,
                        order=3, rtol=0.05, atol=0.0078, h_init=0.05, pcoeff=0., icoeff=1., dcoeff=0.,
                        accept_safety=0.81, eta=0., s_noise=1., return_info=False):
    """DPM-Solver-12 / -23 with adaptive step size (:855-892)."""
    if sigma_min <= 0 or sigma_max <= 0:
        raise ValueError('sigma_min and sigma_max must not be 0')
    if eta:
        _refuse_keyed('dpm_adaptive', 'with eta > 0')
    action, info = _solver(model, extra_args, callback).dpm_solver_adaptive(
        state, action, goal, _neg_log(sigma_max), _neg_log(sigma_min), order, rtol, atol, h_init, pcoeff, icoeff,
        dcoeff, accept_safety, eta, s_noise)
    return (action, info) if return_info else action


@torch.no_grad()
def sample_dpmpp_sde(model, state, action, goal, sigmas, extra_args=None, callback=None, disable=None, eta=1.,
                     s_noise=1., scaler=None, noise_sampler=None, r=1 / 2):
    """Stochastic DPM-Solver++ (:739-795): two exponential-integrator half steps per sigma interval, each to the
    ancestral sigma_down of its sub-interval followed by the matching amount of Brownian noise.  This is what
    ``sampler_type='dpmpp_2m_sde'`` runs (beso_agent.py:452-453)."""
    extra_args = {} if extra_args is None else extra_args
    _refuse_keyed('dpmpp_2m_sde', '(sample_dpmpp_sde) draws Brownian-path noise per step')
    sig = _host_sigmas(sigmas)
    if noise_sampler is None:
        noise_sampler = BrownianTreeNoiseSampler(action, sig[sig > 0].min(), sig.max())
    r = f32(r)
    fac = float(1 / (2 * r))

    def to(x, denoised, t, t_to):                          # x at t -> t_to along the denoised direction
        return float(_sigma_of(t_to) / _sigma_of(t)) * x - float(f32(np.expm1(f32(t - t_to)))) * denoised

    for i in range(len(sig) - 1):
        denoised = model(state, action, goal, _sig_vec(action, sig[i]), **extra_args)
        if callback is not None:
            callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
        if sig[i + 1] == 0:
            action = action + to_d(action, sig[i], denoised) * float(sig[i + 1] - sig[i])
            continue
        t, t_next = _neg_log(sig[i]), _neg_log(sig[i + 1])
        s = f32(t + f32(t_next - t) * r)
        sd, su = get_ancestral_step(_sigma_of(t), _sigma_of(s), eta)
        x_2 = to(action, denoised, t, _neg_log(sd))
        x_2 = x_2 + noise_sampler(_sigma_of(t), _sigma_of(s)) * (s_noise * float(su))
        denoised_2 = model(state, x_2, goal, _sig_vec(action, _sigma_of(s)), **extra_args)
        sd, su = get_ancestral_step(_sigma_of(t), _sigma_of(t_next), eta)
        action = to(action, (1 - fac) * denoised + fac * denoised_2, t, _neg_log(sd))
        action = action + noise_sampler(_sigma_of(t), _sigma_of(t_next)) * (s_noise * float(su))
        if scaler is not None:
            action = scaler.clip_output(action)
    return action


# ------------------------------------------------------------------------------------------------
# the denoising trajectory of a one-launch sampler loop
# ------------------------------------------------------------------------------------------------
@torch.no_grad()
def sample_trajectory(sampler, model, state, action, goal, sigmas, eta=1., s_noise=1., order=4, noise=None,
                      trace=('x', 'denoised')):
    """The sampler loop ``sampler`` (a key of ``_lib.SAMPLERS``: 'ddim', 'euler', 'heun', 'euler_ancestral', 'dpm_2', ...) from
    ``action`` = x_T as ONE enqueue that also records its trajectory (``beso_sample_traced``: the launches of the plain call
    write it, nothing is evaluated twice) -> ``(x_0, xs, denoised)``:

      * ``xs`` [n + 1, B, t, act]: ``xs[0]`` is x_T, ``xs[i + 1]`` is x after step i is complete (behind the second evaluation of
        a two-evaluation step and behind the noise of an ancestral step), so ``xs[n]`` equals ``x_0`` bit for bit -- the list
        the reference's ``visualize_ode`` builds from repeated two-entry schedules (beso_agent.py:525-531);
      * ``denoised`` [n, B, t, act]: the model's output at the first evaluation of step i, what the reference's loops hand
        their callback as 'denoised' (classifier-free combination included).

    An entry not named in ``trace`` is returned as None.  ``model`` is a ``beso_amd`` GCDenoiser, or a
    ClassifierFreeSampleModel around one.  The ancestral samplers draw through ``predraw_noise`` when ``noise`` is None, as the
    samplers do.  Fused-only by design: where ``_fused_call`` would decline (a foreign model, CPU tensors, a non-positive
    interior sigma) this raises NotImplementedError -- there is no second evaluation path behind it.

    The samplers' own ``callback=`` argument is NOT routed here: those calls keep the Python loop and the bits it returns
    today.  ``replay_callback`` feeds an existing callback from a recorded launch instead."""
    from .... import _lib
    if sampler not in _lib.SAMPLERS:
        raise ValueError('desired sampler type not found!')
    den, lam = _fused_target(model)
    if den is None:
        raise NotImplementedError('sample_trajectory records inside the HIP sampler loop: the model must be a beso_amd '
                                  'GCDenoiser (optionally inside ClassifierFreeSampleModel)')
    if not (torch.is_tensor(action) and action.is_cuda):
        raise NotImplementedError('sample_trajectory runs on the GPU only (the inputs are CPU tensors)')
    if not den.can_fuse_sampler(state, action, goal):
        raise NotImplementedError('sample_trajectory: the denoiser does not run these inputs as one enqueue (eval mode, '
                                  'fp32 HIP tensors [B, t, .] and a beso_amd DiffusionGPT inside are required)')
    trace = {trace} if isinstance(trace, str) else set(trace)
    if not trace or trace - {'x', 'denoised'}:
        raise ValueError("trace must be a non-empty subset of {'x', 'denoised'} (the plain samplers record nothing)")
    sig = _host_sigmas(sigmas)
    if len(sig) < 2 or not all(float(v) > 0.0 for v in sig[:-1]):
        raise NotImplementedError('sample_trajectory: the schedule must be positive up to its trailing value')
    if sampler.endswith('_ancestral') and noise is None:
        noise = predraw_noise(sampler, sig, action, eta)
    x_0, rec = den.fused_sampler(sampler, state, action, goal, sig, cond_lambda=lam, eta=eta, s_noise=s_noise, order=order,
                                 noise=noise, trace=trace)
    return x_0, rec.get('x'), rec.get('denoised')


def replay_callback(callback, sigmas, xs, denoised):
    """Hands ``callback`` the dict the sampler loops hand it, once per step of a trajectory recorded by
    ``sample_trajectory``: {'x': xs[i], 'i': i, 'sigma': sigmas[i], 'sigma_hat': sigmas[i], 'denoised': denoised[i]} for
    i = 0 .. n - 1 (no churn in the one-launch loops: sigma_hat is sigma)."""
    sig = _host_sigmas(sigmas)
    for i in range(len(sig) - 1):
        callback({'x': xs[i], 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised[i]})


def _out_of_scope(name, why):
    def fn(*a, **k):
        raise NotImplementedError(f"{name} is outside the MI355X hot-path scope ({why}); see DESIGN.md")
    fn.__name__ = name
    return fn


# the reference's sample_dpmpp_2m_sde cannot run (it reads undefined names, gc_sampling.py:817-820) and nothing
# dispatches to it (beso_agent.py:452 maps 'dpmpp_2m_sde' to sample_dpmpp_sde): there is no behaviour to reproduce
sample_dpmpp_2m_sde = _out_of_scope('sample_dpmpp_2m_sde', 'the reference function raises NameError; use sample_dpmpp_sde')


# ------------------------------------------------------------------------------------------------
# log-likelihood (:471-497): the probability-flow ODE from sigma_min to sigma_max with Hutchinson's trace estimate
# ------------------------------------------------------------------------------------------------
# Dormand-Prince 5(4) (Hairer, Norsett & Wanner, Solving ODEs I, II.5): nodes, stage weights, 5th-order weights and the
# difference of the 5th- and 4th-order weights (the error estimate)
_DP_C = (0., 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.)
_DP_A = ((),
         (1 / 5,),
         (3 / 40, 9 / 40),
         (44 / 45, -56 / 15, 32 / 9),
         (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
         (35 / 384, 0., 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_E = (71 / 57600, 0., -71 / 16695, 71 / 1920, -17253 / 339200, 22 / 525, -1 / 40)


def _rms(x):
    return x.pow(2).mean().sqrt()


def _dopri5(fn, y0, t0, t1, atol, rtol, safety=0.9, fmin=0.2, fmax=10.):
    """Integrate dy/dt = fn(t, y) for a tuple of tensors y from t0 to t1 (t1 > t0): adaptive Dormand-Prince 5(4) with
    one step size for the whole state, FSAL (the 7th stage at the accepted point is the next step's 1st), Hairer's
    initial step, the error ratio max over tensors of RMS(err / (atol + rtol max(|y0|, |y1|))) and the step factor
    safety * ratio^(-1/5) clamped to [fmin, fmax].  Stage combinations are tensor ops on y's device; the one host read
    per step is the error ratio.  -> (y(t1), {'steps': accepted, 'rejected': n, 'fevals': n}).

    Departures from torchdiffeq's dopri5: the last step is clamped to end at t1 (no dense-output interpolation);
    the step factor after an accepted step may also shrink; no step-size floor (a non-finite ratio raises)."""
    t0, t1 = float(t0), float(t1)
    stats = {'steps': 0, 'rejected': 0, 'fevals': 0}

    def f(t, y):
        stats['fevals'] += 1
        return tuple(fn(t, y))

    def comb(y, h, ks, ws):                     # y + h sum_j w_j k_j, per tensor
        out = []
        for i, yi in enumerate(y):
            acc = yi
            for w, k in zip(ws, ks):
                if w != 0.:
                    acc = acc + (h * w) * k[i]
            out.append(acc)
        return tuple(out)

    y = tuple(y0)
    k1 = f(t0, y)
    # initial step (Hairer's HINIT, as torchdiffeq's _select_initial_step)
    scale = [atol + rtol * yi.abs() for yi in y]
    d0 = max(float(_rms(yi / s)) for yi, s in zip(y, scale))
    d1 = max(float(_rms(ki / s)) for ki, s in zip(k1, scale))
    h0 = 0.01 * d0 / d1 if (d0 >= 1e-5 and d1 >= 1e-5) else 1e-6
    f1 = f(t0 + h0, comb(y, h0, (k1,), (1.,)))
    d2 = max(float(_rms((a - b) / s)) for a, b, s in zip(f1, k1, scale)) / h0
    h1 = max(1e-6, h0 * 1e-3) if max(d1, d2) <= 1e-15 else (0.01 / max(d1, d2)) ** (1. / 5)
    h = min(100 * h0, h1, t1 - t0)
    t = t0
    while t < t1:
        last = t + h >= t1 or (t1 - (t + h)) <= 1e-12 * max(1., abs(t1))
        if last:
            h = t1 - t
        ks = [k1]
        for j in range(1, 7):
            ks.append(f(t + _DP_C[j] * h, comb(y, h, ks, _DP_A[j])))
        y_new = comb(y, h, ks[:6], _DP_A[6])
        err = comb(tuple(torch.zeros_like(yi) for yi in y), h, ks, _DP_E)
        ratio = torch.stack([_rms(e / (atol + rtol * torch.maximum(a.abs(), b.abs())))
                             for e, a, b in zip(err, y, y_new)]).max()
        ratio = float(ratio)                    # the step's one host read
        if not math.isfinite(ratio):
            raise FloatingPointError("dopri5: non-finite error estimate")
        if ratio <= 1.:
            t = t1 if last else t + h
            y, k1 = y_new, ks[6]                # FSAL
            stats['steps'] += 1
        else:
            stats['rejected'] += 1
        factor = fmax if ratio == 0. else min(fmax, max(fmin, safety * ratio ** (-1. / 5)))
        h = h * factor
    return y, stats


def _log_likelihood_ode(rhs, action, sigma_min, sigma_max, atol, rtol):
    """The ODE of log_likelihood: state (x, ll), integrated in sigma from sigma_min to sigma_max; ``rhs(x, sigma) ->
    (dx/dsigma, dll/dsigma [B])``.  -> (ll [B], latent, stats): the Gaussian prior N(0, sigma_max^2) of the latent plus
    the accumulated log-density change (:487-496)."""
    y0 = (action, action.new_zeros([action.shape[0]]))
    (latent, delta_ll), stats = _dopri5(lambda s, y: rhs(y[0], s), y0, sigma_min, sigma_max, atol, rtol)
    ll_prior = torch.distributions.Normal(0, sigma_max).log_prob(latent).flatten(1).sum(1)
    return ll_prior + delta_ll, latent, stats


@torch.no_grad()
def log_likelihood(model, state, action, goal, sigma_min, sigma_max, extra_args=None, atol=1e-4, rtol=1e-4):
    """Log-density of ``action`` under the probability-flow ODE of ``model`` (:471-497) -> (ll [B], {'fevals': n}).

    One evaluation of the right-hand side is ONE ``GCDenoiser.denoise_vjp`` call (the denoiser and its input
    vector-Jacobian product with the Hutchinson vector v), two for ``ClassifierFreeSampleModel`` (cond and uncond,
    combined as lam * cond + (1 - lam) * uncond).  v is drawn once per call from the global generator of the action's
    device, as the reference draws it.  The integrator is the self-contained ``_dopri5`` above (torchdiffeq's method,
    the reference's atol / rtol)."""
    extra_args = {} if extra_args is None else dict(extra_args)
    den, lam = _fused_target(model)
    if den is None:
        raise NotImplementedError("log_likelihood needs a beso_amd GCDenoiser (optionally in ClassifierFreeSampleModel): "
                                  "the input vector-Jacobian product is a HIP call of that model, there is no autograd path")
    uncond = bool(extra_args.pop('uncond', False))
    if extra_args:
        raise NotImplementedError(f"log_likelihood: unsupported extra_args {sorted(extra_args)}")
    v = torch.randint_like(action, 2) * 2 - 1
    vv = (v * v).flatten(1).sum(1)
    fevals = 0

    def rhs(x, sigma):
        nonlocal fevals
        fevals += 1
        if lam == 1.0:
            denoised, _, dot = den.denoise_vjp(state, x, goal, sigma, v, uncond=uncond)
        else:
            dc, _, tc = den.denoise_vjp(state, x, goal, sigma, v)
            du, _, tu = den.denoise_vjp(state, x, goal, sigma, v, uncond=True)
            denoised, dot = lam * dc + (1 - lam) * du, lam * tc + (1 - lam) * tu
        return (x - denoised) / sigma, (vv - dot) / sigma

    ll, _, _ = _log_likelihood_ode(rhs, action.float(), sigma_min, sigma_max, atol, rtol)
    return ll, {'fevals': fevals}
