"""The gradient of the training loss, and of the denoiser output, with respect to the ``state`` and ``goal`` inputs
(``beso_loss_grad_inputs`` / ``beso_denoise_vjp_inputs``, ``input_grad_kernel`` of train_rows.h).

Comparator: tests/autograd_reference.py (``loss_autograd`` / ``forward_autograd``) with ``state`` / ``goal`` as leaf tensors
that require grad; the masked cases inject the library's own masks the way tests/test_dropout_parity.py does.

Error measure and bounds are that file's: per tensor ``||got - ref|| / max(||ref||, floor * max|ref| * sqrt(numel))`` with
``max|ref|`` the largest entry of the tensors compared together; gradients 1e-4 (fp32, floor 1e-4) / 2.6e-2 (bf16, floor 2e-3),
loss 2e-5 / 2e-3.  ``state_grad`` and ``goal_grad`` are linear images of the same dx0 that ``tok_emb.weight``'s gradient is an
image of, so they are held to the parameter gradients' bounds; the input gradients are measured against their own largest
entry, not against the (larger) parameter gradients'.  Every case prints what it measured."""
import contextlib
import ctypes as C

import pytest
import torch

from beso_amd import _lib
from beso_amd.runtime import ScoreNetShape
from oracle import beso_oracle as O
from support import Scale, TRAIN_BOUNDS, grad_errors, lib, make_denoiser, train_inputs  # noqa: F401

DEV = "cuda:0"
TOL_VJP = {"fp32": 2e-4, "bf16": 2.6e-2}                                  # tests/test_log_likelihood.py
PLANS = {"default": 0, "tiles": _lib.TRAIN_PLAN_TILES, "per_op": _lib.TRAIN_PLAN_PER_OP}


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_bound(lib):
    for name in ("beso_loss_grad_inputs", "beso_denoise_vjp_inputs"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.beso_loss_grad_inputs.argtypes) == len(lib.beso_loss_grad_streams.argtypes) + 2
    assert len(lib.beso_denoise_vjp_inputs.argtypes) == len(lib.beso_denoise_vjp.argtypes) + 2


def test_loss_grad_inputs_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers, as test_dropout_mask_argument_errors_do_not_touch_the_device: a call that got past its
    argument checks would write through them."""
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()        # G = 2, W = 3
    nogoal = ScoreNetShape(6, 4, 40, 2, 5, 0, 3, True, 0.5).c_struct()     # G = 0
    one = C.c_void_p(16)

    def call(c=cfg, null_cfg=False, **kw):
        n = lib.beso_num_params(C.byref(c))
        a = dict(cfg=None if null_cfg else C.byref(c), params=(C.c_void_p * n)(*([16] * n)), n=n, grads=one, prec=_lib.PREC_FP32,
                 state=one, action=one, goal=one, noise=one, sigma=one, loss=one, batch=2, t=2, flags=0, embed_p=0.0, attn_p=0.0,
                 resid_p=0.0, goal_p=0.0, seed=C.c_uint(1), scale=1.0, ws=one, wsb=1 << 40, stream=None, early=None,
                 loss_stream=None, state_grad=one, goal_grad=one)
        a.update(kw)
        return lib.beso_loss_grad_inputs(*a.values())

    assert call(c=nogoal, goal=None) == -3                                  # goal_grad with G = 0
    assert call(state_grad=C.c_void_p(18)) == -3 and call(goal_grad=C.c_void_p(17)) == -3       # not 4-byte aligned
    assert call(null_cfg=True) == -3
    assert call(t=9) == -2 and call(batch=0) == -2
    assert call(state=None) == -3 and call(grads=None) == -3
    assert call(wsb=16) == -4                                               # (the last check: everything else was accepted)
    with pytest.raises(ValueError):
        _lib.check(call(c=nogoal, goal=None), "loss_grad_inputs")
    # the VJP entry point shares the checks
    n = lib.beso_num_params(C.byref(nogoal))
    arr = (C.c_void_p * n)(*([16] * n))
    vjp = lambda sg, gg: lib.beso_denoise_vjp_inputs(C.byref(nogoal), arr, n, _lib.PREC_FP32, one, one, None, one, one, one, one,   # noqa: E731
                                                     None, 2, 2, 0, one, 1 << 40, None, sg, gg)
    assert vjp(one, one) == -3 and vjp(C.c_void_p(18), None) == -3


def test_backward_reduces_a_broadcast_goal_to_its_own_shape():
    """ScoreMatchingLoss with the HIP call stubbed out: the gradients run() returns for the expanded inputs come back times
    grad_out, in the input's dtype, summed over the batch where the goal was given without (or with a unit) batch dimension;
    action / noise / sigma get None; nothing is asked of run() when no input requires grad."""
    from beso_amd.training import ScoreMatchingLoss
    B, t, G, obs = 3, 2, 2, 4
    gen = torch.Generator().manual_seed(0)
    sg, gg = torch.randn(B, t, obs, generator=gen), torch.randn(B, G, obs, generator=gen)
    w = torch.zeros(5, requires_grad=True)
    asked = []

    class Step:
        inner = type("Inner", (), {"goal_seq_len": G})()

        def run(self, state, action, goal, noise, sigma, fresh_grads=False, last_action_only=False, input_grads=False):
            asked.append(input_grads)
            flat = torch.arange(5, dtype=torch.float32)
            out = (torch.tensor(1.5), flat, [flat])
            return out + (sg.clone(), gg.clone()) if input_grads else out

    action = noise = torch.zeros(B, t, 1)
    sigma = torch.ones(B)
    for goal_shape, want in (((G, obs), gg.sum(0)), ((1, G, obs), gg.sum(0, keepdim=True)), ((B, G, obs), gg)):
        state = torch.zeros(B, t, obs, dtype=torch.float64, requires_grad=True)
        goal = torch.zeros(goal_shape, requires_grad=True)
        loss = ScoreMatchingLoss.apply(Step(), False, state, action, goal, noise, sigma, w)
        (loss * 2.0).backward()
        assert asked[-1] is True
        assert goal.grad.shape == goal_shape and torch.equal(goal.grad, 2.0 * want)
        assert state.grad.dtype == torch.float64 and torch.equal(state.grad, (2.0 * sg).double())
        assert torch.equal(w.grad, 2.0 * torch.arange(5, dtype=torch.float32))
        w.grad = None
    # only the goal requires grad; then nothing does
    goal = torch.zeros(G, obs, requires_grad=True)
    ScoreMatchingLoss.apply(Step(), False, torch.zeros(B, t, obs), action, goal, noise, sigma, w).backward()
    assert asked[-1] is True and torch.equal(goal.grad, gg.sum(0))
    ScoreMatchingLoss.apply(Step(), False, torch.zeros(B, t, obs), action, torch.zeros(G, obs), noise, sigma, w).backward()
    assert asked[-1] is False


@contextlib.contextmanager
def _injected_embed_mask(inner, step, batch, t, seed):
    """inner.drop replaced by the library's embedding mask for (batch, t, seed): forward_autograd calls it for the states,
    the actions and the goals, in that order (rows G+1+2k, G+2+2k and 1..G of the [B, T, D] mask)."""
    G = inner.goal_seq_len
    old = inner._modules["drop"]
    try:
        if inner._pdrops[0] > 0:
            e = step.dropout_mask("embed", 0, batch, t, seed)
            inner._modules["drop"] = Scale(e[:, G + 1::2], e[:, G + 2::2], e[:, 1:G + 1])
        yield
    finally:
        inner._modules["drop"] = old


def _reference(m, inputs, last_only=False, step=None, seed=None, goal_mask=True):
    """(loss, d loss / d state, d loss / d goal or None, parameter gradients) of the autograd comparator; with `step` and
    `seed` the library's embedding-dropout and goal masks of that seed are injected (goal_mask=False leaves the goal mask
    out: the deliberately wrong comparator of test_the_comparison_bites)."""
    from autograd_reference import loss_autograd
    inner = m.inner_model
    state, action, goal, noise, sigma = inputs
    B, t = state.shape[0], state.shape[1]
    state = state.detach().clone().requires_grad_()
    goal = goal.detach().clone().requires_grad_()
    goal_p = inner.cond_mask_prob
    inner.cond_mask_prob = 0.0                                               # (its own mask_cond off: the mask is injected)
    try:
        g_in = goal
        if step is not None and goal_p and goal_mask and inner.goal_seq_len > 0:
            g_in = goal * step.goal_mask(B, seed, goal_drop=goal_p)
        with (_injected_embed_mask(inner, step, B, t, seed) if step is not None else contextlib.nullcontext()):
            loss = loss_autograd(m, state, action, g_in, noise.clone(), sigma, last_only)
            loss.backward()
        return loss.item(), state.grad, goal.grad, [p.grad.clone() for p in m.parameters()]
    finally:
        inner.cond_mask_prob = goal_p
        for p in m.parameters():
            p.grad = None


def _report(tag, precision, m, got_loss, got_in, got_par, ref):
    """prints and returns (loss error, worst input-gradient error, worst parameter-gradient error)"""
    ref_loss, ref_s, ref_g, ref_par = ref
    _, _, floor = TRAIN_BOUNDS[precision]
    lerr = abs(got_loss - ref_loss) / abs(ref_loss)
    pairs = [(g, r) for g, r in zip(got_in, (ref_s, ref_g)) if r is not None]
    ierrs = grad_errors([g for g, _ in pairs], [r for _, r in pairs], floor)
    perrs = grad_errors(got_par, ref_par, floor)
    worst = max(range(len(perrs)), key=lambda i: perrs[i])
    print(f"[parity] input grads {tag} {precision}: loss {lerr:.2e}, state_grad {ierrs[0]:.2e}, goal_grad "
          f"{ierrs[1] if len(ierrs) > 1 else float('nan'):.2e}, worst parameter gradient {perrs[worst]:.2e} "
          f"({list(dict(m.named_parameters()))[worst]})")
    return lerr, max(ierrs), perrs[worst]


def _through_autograd(m, inputs, last_only=False):
    """m.loss(...).backward() with state and goal as leaves: (loss, state.grad, goal.grad, parameter gradients)"""
    state, action, goal, noise, sigma = inputs
    state = state.detach().clone().requires_grad_()
    goal = goal.detach().clone().requires_grad_()
    kw = {"pred_last_action_only": True} if last_only else {}
    loss = m.loss(state, action, goal, noise.clone(), sigma, **kw)
    loss.backward()
    grads = [p.grad.clone() for p in m.parameters()]
    for p in m.parameters():
        p.grad = None
    return loss.item(), state.grad, goal.grad, grads


# -------------------------------------------------------------------------------------------------
# GPU 1: parity through autograd
# -------------------------------------------------------------------------------------------------
PARITY = [(c, p, pl) for c in ("tiny", "tiny_mlp_head", "tiny_nogoal", "kitchen", "block_push")
          for p, pls in (("fp32", ("default",)), ("bf16", ("default", "tiles", "per_op"))) for pl in pls]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision,plan", PARITY)
def test_loss_backward_reaches_state_and_goal(cfg_name, precision, plan):
    """m.loss(state, action, goal, noise, sigma).backward() with state and goal requiring grad: state.grad, goal.grad and, in
    the same call, the loss and every parameter gradient against the comparator; t = W and t = max(1, W - 1), and once with
    pred_last_action_only.  B = 5: no multiple of a tile, and with the goals two partial row tiles of input_grad_kernel."""
    from beso_amd.runtime import plan as run_plan
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, train=True)
    W = cfg.obs_seq_len
    ltol, gtol, _ = TRAIN_BOUNDS[precision]
    for t, last_only in [(t, False) for t in sorted({max(1, W - 1), W})] + [(W, True)]:
        inputs = train_inputs(cfg, 5, t, seed=4 + t)
        with run_plan(train=PLANS[plan]):
            loss, s_grad, g_grad, par = _through_autograd(m, inputs, last_only)
        ref = _reference(m, inputs, last_only)
        assert s_grad is not None and s_grad.shape == inputs[0].shape
        if m.inner_model.goal_seq_len > 0:
            assert g_grad is not None and g_grad.shape == inputs[2].shape
        else:
            assert g_grad is None and ref[2] is None                      # the goals are not an input of this network
        lerr, ierr, perr = _report(f"{cfg_name} {plan} t={t}{' last-only' if last_only else ''}", precision, m, loss,
                                   (s_grad, g_grad), par, ref)
        assert lerr < ltol and ierr < gtol and perr < gtol, (lerr, ierr, perr)


# -------------------------------------------------------------------------------------------------
# GPU 2: a goal without batch dimension
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_broadcast_goal_gets_the_sum_over_samples():
    cfg = O.TINY
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), "fp32", train=True)
    state, action, goal, noise, sigma = train_inputs(cfg, 6, cfg.obs_seq_len, seed=9)
    shared = goal[0].contiguous()                                          # [G, obs]
    _, s_b, g_b, par_b = _through_autograd(m, [state, action, shared, noise, sigma])
    _, s_e, g_e, par_e = _through_autograd(m, [state, action, shared.unsqueeze(0).expand(6, -1, -1).contiguous(), noise, sigma])
    assert g_b.shape == shared.shape and g_e.shape == (6,) + shared.shape
    err = ((g_b - g_e.sum(0)).norm() / g_e.sum(0).norm()).item()
    print(f"[parity] broadcast goal: goal.grad vs sum over samples {err:.2e}")
    assert err < 1e-6
    assert ((s_b - s_e).norm() / s_e.norm()).item() < 1e-6
    ref = _reference(m, [state, action, shared, noise, sigma])
    assert ref[2].shape == shared.shape
    assert grad_errors([g_b], [ref[2]], 1e-4)[0] < 1e-4


# -------------------------------------------------------------------------------------------------
# GPU 3 / 4: the training-time masks
# -------------------------------------------------------------------------------------------------
def _masked_case(cfg_name, precision, goal_drop, B=6, seed=20240):
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, embed_pdrop=0.1, goal_drop=goal_drop, train=True)
    inputs = train_inputs(cfg, B, cfg.obs_seq_len, seed=4)
    step = m.hip_train_step(*inputs)
    assert step is not None and m.inner_model.training
    loss, _, views, s_grad, g_grad = step.run(*inputs, seed=seed, fresh_grads=True, input_grads=True)
    return m, inputs, step, seed, loss.item(), (s_grad, g_grad), [v.clone() for v in views]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision", [("tiny", "fp32"), ("tiny", "bf16"), ("kitchen", "fp32"), ("kitchen", "bf16")])
def test_masked_step_matches_autograd_with_the_librarys_masks(cfg_name, precision):
    """Training mode, embed_pdrop 0.1 and goal_drop 0.3, then goal_drop 1.0: parity with the library's masks injected; a goal
    element whose keep-mask is 0 has gradient exactly 0.0 -- with goal_drop 1.0 the whole goal gradient."""
    ltol, gtol, _ = TRAIN_BOUNDS[precision]
    for goal_drop in (0.3, 1.0):
        m, inputs, step, seed, loss, got_in, par = _masked_case(cfg_name, precision, goal_drop)
        ref = _reference(m, inputs, step=step, seed=seed)
        lerr, ierr, perr = _report(f"{cfg_name} embed_pdrop=0.1 goal_drop={goal_drop}", precision, m, loss, got_in, par, ref)
        assert lerr < ltol and ierr < gtol and perr < gtol, (lerr, ierr, perr)
        keep = step.goal_mask(inputs[0].shape[0], seed)
        dropped = keep == 0
        assert bool(dropped.any()) and bool((got_in[1][dropped] == 0.0).all())
        if goal_drop == 1.0:
            assert bool(dropped.all()) and bool((got_in[1] == 0.0).all())
        else:
            assert bool((got_in[1][~dropped] != 0.0).any())


@pytest.mark.gpu
def test_the_comparison_bites():
    """The same comparison with the goal mask left out of the comparator exceeds the bound (while the right one passes)."""
    m, inputs, step, seed, loss, got_in, par = _masked_case("kitchen", "fp32", 0.3)
    _, gtol, _ = TRAIN_BOUNDS["fp32"]
    _, ierr, _ = _report("kitchen goal_drop=0.3 (right masks)", "fp32", m, loss, got_in, par, _reference(m, inputs, step=step, seed=seed))
    assert ierr < gtol
    _, ierr, _ = _report("kitchen goal_drop=0.3 (no goal mask in the comparator)", "fp32", m, loss, got_in, par,
                         _reference(m, inputs, step=step, seed=seed, goal_mask=False))
    assert ierr > gtol, ierr


# -------------------------------------------------------------------------------------------------
# GPU 5: reproducibility and non-interference
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_input_grads_are_reproducible_and_leave_the_step_alone(precision):
    cfg = O.KITCHEN
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, embed_pdrop=0.1, goal_drop=0.3, train=True)
    inputs = train_inputs(cfg, 6, cfg.obs_seq_len, seed=4)
    step = m.hip_train_step(*inputs)
    a = step.run(*inputs, seed=7, fresh_grads=True, input_grads=True)
    b = step.run(*inputs, seed=7, fresh_grads=True, input_grads=True)
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])             # without BESO_TRAIN_DETERMINISTIC
    c = step.run(*inputs, seed=8, fresh_grads=True, input_grads=True)
    assert not torch.equal(a[4], c[4])                                     # (another seed: other masks)
    on = step.run(*inputs, seed=7, fresh_grads=True, input_grads=True, deterministic=True)
    off = step.run(*inputs, seed=7, fresh_grads=True, deterministic=True)
    assert len(off) == 3
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])       # loss and flat gradient: the same bits
    assert torch.equal(on[3], a[3]) and torch.equal(on[4], a[4])
    # loss_backward hands the same tensors over and touches no input's .grad
    loss, sg, gg = step.loss_backward(*inputs, seed=7, input_grads=True)
    assert torch.equal(sg, a[3]) and torch.equal(gg, a[4]) and inputs[0].grad is None
    for p in m.parameters():
        p.grad = None


# -------------------------------------------------------------------------------------------------
# GPU 6: denoise_vjp(..., input_grads=True)
# -------------------------------------------------------------------------------------------------
def _rel_max(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.double().abs().max()), 1e-30))   # conftest.rel_err


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision", [(c, p) for c in ("tiny", "tiny_nogoal", "kitchen") for p in ("fp32", "bf16")])
def test_denoise_vjp_input_grads_against_autograd(cfg_name, precision):
    """(d denoised / d state)^T cot and (d denoised / d goal)^T cot against torch.autograd.grad over the preconditioned
    forward_autograd (test_log_likelihood.vjp_autograd's construction); uncond: the goal gradient is exactly zero; the
    first three outputs are the bits of the call without the option."""
    from autograd_reference import forward_autograd
    cfg = O.CONFIGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=0, std=0.02), precision, train=False)
    G = m.inner_model.goal_seq_len
    W = cfg.obs_seq_len
    for t in sorted({max(1, W - 1), W}):
        state, x, goal, cot, sigma = train_inputs(cfg, 5, t, seed=t)
        for uncond in (False, True):
            with torch.no_grad():
                den, xg, dot, s_grad, g_grad = m.denoise_vjp(state, x, goal, sigma, cot, uncond=uncond, input_grads=True)
                den0, xg0, dot0 = m.denoise_vjp(state, x, goal, sigma, cot, uncond=uncond)
            assert torch.equal(den, den0) and torch.equal(xg, xg0) and torch.equal(dot, dot0)
            with torch.enable_grad():
                s_l, g_l = state.clone().requires_grad_(), goal.clone().requires_grad_()
                c_skip, c_out, c_in = (c.reshape(-1, 1, 1) for c in m.get_scalings(sigma))
                ref_den = c_skip * x + c_out * forward_autograd(m.inner_model, s_l, x * c_in, g_l, sigma, uncond)
                ref_s, ref_g = torch.autograd.grad(ref_den, (s_l, g_l), cot, allow_unused=True)
            e_s = _rel_max(s_grad, ref_s)
            assert s_grad.shape == state.shape
            if G == 0:
                assert g_grad is None and ref_g is None
                e_g = float("nan")
            elif uncond:
                assert bool((g_grad == 0.0).all()) and (ref_g is None or bool((ref_g == 0).all()))
                e_g = 0.0
            else:
                assert g_grad.shape == goal.shape
                e_g = _rel_max(g_grad, ref_g)
                assert e_g <= TOL_VJP[precision]
            print(f"[parity] vjp input grads {cfg_name} {precision} t={t} uncond={uncond}: state_grad {e_s:.2e} goal_grad {e_g:.2e}")
            assert e_s <= TOL_VJP[precision]


# -------------------------------------------------------------------------------------------------
# GPU 7: what is still refused
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_action_noise_and_sigma_that_require_grad_are_refused():
    cfg = O.TINY
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), "fp32", train=True)
    for i in (1, 3, 4):                                                     # action, noise, sigma
        inputs = train_inputs(cfg, 5, cfg.obs_seq_len, seed=4)
        inputs[i].requires_grad_()
        with pytest.raises(ValueError, match="gradients with respect to action, noise and sigma are not computed"):
            m.loss(*inputs)
