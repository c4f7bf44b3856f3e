"""The guide's fit step on the MI355X: ``beso_guide_fit_rows`` / ``beso_guide_fit_loss`` / ``beso_guide_apply_sigma``
(include/beso_guide_fit.h, csrc/guide_fit.hip, csrc/guide_tile.h) and ``GuideTrainer`` (k_diffusion/guide_fit.py).

Arbiters: torch re-statements of the rows (``cat``, bit for bit), tests/test_guide_fit.py's float32 numpy re-statement of the loss
launch's summation order (mse: bit for bit) and its float64 one (bce: ``TRAIN_BOUNDS['fp32']``), torch autograd in fp64 over a
torch copy of the network (gradients: tests/test_mlp_encoder.py's rule, at most 4x what fp32 torch autograd errs), the generic
autograd path of ``ClassifierGuidedSampleModel`` (the fused launch with the noise-level column: tests/test_classifier_guidance.py's
fused-against-generic bars) and a float64 torch twin with plain Adam (20 training steps).  Shapes: obs 5, act 3, G 2.  Every case
prints what it measured."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from beso_amd import _lib
from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierGuidedSampleModel
from beso_amd.agents.diffusion_agents.k_diffusion.guide_fit import GuideTrainer
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
from beso_amd.networks.mlps.mlps import MLPNetwork
from support import TRAIN_BOUNDS, bits, grad_errors
from test_classifier_guidance import Stub, banded_out, check_bars, guards_intact
from test_guide_fit import restated_f64, restated_mse

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OBS, ACT, G = 5, 3, 2
ACTS = {"ReLU": nn.ReLU, "Mish": nn.Mish, "sigmoid": nn.Sigmoid}
EPS = 2.0 ** -24        # one fp32 rounding
FILLS = {"ZERO": 0x00, "NAN": 0xFF, "HUGE": 0x7B}          # tests/test_buffer_independence.py
KINDS = _lib.GUIDEFIT_LOSSES
# (B, T, state_steps): M = 6, under one 16-row tile; M = 33, a partial third tile
ROW_SHAPES = [(3, 2, 3), (11, 3, 3)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def inputs(B, T, steps, goal, seed=1):
    """state, action, goal (None / 'own' [B, G, obs] / 'shared' [1, G, obs]), sigma, noise on the device."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    state, action, goals, noise = r(B, steps, OBS), r(B, T, ACT), r(B, G, OBS), r(B, T, ACT)
    sigma = (0.05 + 1.5 * torch.rand(B, generator=g)).to(DEV)                           # distinct per sample
    return state, action, (None if goal is None else goals[:1].contiguous() if goal == "shared" else goals), sigma, noise


def torch_rows(state, action, goal, sigma, noise, c_noise):
    B, T, _ = action.shape
    parts = [state[:, :T], action if sigma is None else action + sigma[:, None, None] * noise]
    if goal is not None:
        parts.append(goal[:, -1:, :].expand(B, T, -1))
    if c_noise is not None:
        parts.append(c_noise.view(B, 1, 1).expand(B, T, 1))
    return torch.cat(parts, dim=-1).reshape(B * T, -1)


def fit_rows(state, action, goal, sigma, noise, c_noise, out=None):
    B, T, _ = action.shape
    width = OBS + ACT + (OBS if goal is not None else 0) + (1 if c_noise is not None else 0)
    out = torch.empty(B * T, width, device=DEV) if out is None else out
    st = _lib.load_guidefit().beso_guide_fit_rows(ptr(state), ptr(action), ptr(goal), ptr(sigma), ptr(noise), ptr(c_noise), B, T,
                                                  state.shape[1], 0 if goal is None else goal.shape[1],
                                                  0 if goal is None else goal.shape[0], OBS, ACT, out.data_ptr(), stream())
    assert st == _lib.OK
    return out


def fit_loss(q, y, w, kind, outs=None):
    M = q.numel()
    loss, per_row, dq = outs or (torch.empty(1, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV))
    st = _lib.load_guidefit().beso_guide_fit_loss(ptr(q), ptr(y), ptr(w), M, KINDS[kind], loss.data_ptr(), per_row.data_ptr(),
                                                  dq.data_ptr(), stream())
    assert st == _lib.OK
    return loss, per_row, dq


# -------------------------------------------------------------------------------------------------
# 1. rows
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_col", [False, True], ids=["blind", "c_noise"])
@pytest.mark.parametrize("goal", [None, "shared", "own"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_are_the_bits_of_the_torch_restatement(shape, goal, sigma_col):
    state, action, goal, sigma, noise = inputs(*shape, goal)
    c_noise = sigma.log() / 4 if sigma_col else None
    got = fit_rows(state, action, goal, sigma, noise, c_noise)
    want = torch_rows(state, action, goal, sigma, noise, c_noise)
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))
    assert not torch.equal(got[:, OBS:OBS + ACT], action.reshape(-1, ACT))              # the action columns are noised
    clean = fit_rows(state, action, goal, None, None, c_noise)                          # no sigma, no noise: the clean action
    assert torch.equal(bits(clean), bits(torch_rows(state, action, goal, None, None, c_noise)))


# -------------------------------------------------------------------------------------------------
# 2. the loss launch
# -------------------------------------------------------------------------------------------------
def loss_inputs(M, kind, seed=3):
    rng = np.random.default_rng(seed)
    q = (2.0 * rng.standard_normal(M)).astype(np.float32)
    y = rng.standard_normal(M).astype(np.float32) if kind == "mse" else rng.random(M).astype(np.float32)
    w = rng.random(M).astype(np.float32)
    w[::3] = 0.0                                                                        # rows that do not count
    return q, y, w


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weights_with_zeros"])
@pytest.mark.parametrize("M", [6, 33, 600])
def test_mse_loss_launch_is_the_bits_of_the_stated_order(M, weighted):
    """M = 600: lanes 0 ... 87 add three rows, the others two."""
    q, y, w = loss_inputs(M, "mse")
    w = w if weighted else None
    d = lambda v: None if v is None else torch.from_numpy(v).to(DEV)                    # noqa: E731
    loss, per_row, dq = fit_loss(d(q), d(y), d(w), "mse")
    want = restated_mse(q, y, w)
    for name, got, ref in zip(("loss", "per_row", "dq"), (loss, per_row, dq), want):
        got, ref = got.cpu().numpy().reshape(-1), np.asarray(ref, dtype=np.float32).reshape(-1)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (name, np.abs(got - ref).max())
    assert float(loss) > 0 and (not weighted or not dq.cpu().numpy()[::3].any())


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weights_with_zeros"])
@pytest.mark.parametrize("M", [6, 33, 600])
def test_bce_loss_launch_against_float64(M, weighted):
    q, y, w = loss_inputs(M, "bce")
    q[0], q[1] = 30.0, -30.0                                                            # both tails of log1p(exp(-|q|))
    w = w if weighted else None
    d = lambda v: None if v is None else torch.from_numpy(v).to(DEV)                    # noqa: E731
    loss, per_row, dq = fit_loss(d(q), d(y), d(w), "bce")
    l64, p64, g64 = restated_f64(q, y, w, "bce")
    bound_loss, bound_tensor, floor = TRAIN_BOUNDS["fp32"]
    lerr = abs(float(loss) - l64) / abs(l64)
    errs = grad_errors([per_row.cpu().double(), dq.cpu().double()], [torch.from_numpy(p64), torch.from_numpy(g64)], floor)
    print(f"bce M={M} {'weighted' if weighted else 'unweighted'}: loss rel err {lerr:.3e}, per_row {errs[0]:.3e}, dq {errs[1]:.3e}")
    assert lerr <= bound_loss and max(errs) <= bound_tensor
    assert bool(torch.isfinite(per_row).all()) and bool(torch.isfinite(dq).all())


@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_all_zero_weights_give_exact_zero(kind):
    q, y, _ = loss_inputs(33, kind)
    loss, per_row, dq = fit_loss(torch.from_numpy(q).to(DEV), torch.from_numpy(y).to(DEV), torch.zeros(33, device=DEV), kind)
    assert torch.equal(bits(loss), torch.zeros(1, dtype=torch.int32, device=DEV))
    assert torch.equal(bits(dq), torch.zeros(33, dtype=torch.int32, device=DEV))
    assert bool((per_row > 0).any()) and bool(torch.isfinite(per_row).all())             # each row's loss is still reported


# -------------------------------------------------------------------------------------------------
# 3. rows -> forward -> loss -> backward against autograd
# -------------------------------------------------------------------------------------------------
def torch_stack(net, dtype, device="cpu"):
    layers = [copy.deepcopy(lin).to(device, dtype) for lin in net.layers]
    mods = []
    for i, lin in enumerate(layers):
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(ACTS[net.activation]())
    return nn.Sequential(*mods)


def torch_loss(q, y, w, kind):
    if kind == "mse":
        return (w * (q - y) ** 2).sum() / w.sum()
    return F.binary_cross_entropy_with_logits(q, y, weight=w, reduction="sum") / w.sum()


@pytest.mark.parametrize("kind", ["mse", "bce"])
@pytest.mark.parametrize("activation", ["ReLU", "Mish"])
@pytest.mark.parametrize("hidden,layers", [(32, 1), (48, 3)], ids=["32x1", "48x3"])
def test_whole_step_gradients_match_fp64_autograd_as_closely_as_torch_fp32_does(hidden, layers, activation, kind):
    B, T = 11, 3
    torch.manual_seed(0)
    net = MLPNetwork(2 * OBS + ACT + 1, hidden, layers, 1, activation=activation, device=DEV)
    state, action, goal, sigma, noise = inputs(B, T, 3, "own")
    c_noise = sigma.log() / 4
    g = torch.Generator().manual_seed(5)
    y = (torch.randn(B * T, generator=g) if kind == "mse" else torch.rand(B * T, generator=g)).to(DEV)
    w = torch.rand(B * T, generator=g).to(DEV)

    rows = fit_rows(state, action, goal, sigma, noise, c_noise)
    q, keep = net.run_forward(rows, keep=True)
    loss, _, dq = fit_loss(q, y, w, kind)
    flat = torch.empty(net.num_param_floats(), device=DEV)
    net.run_backward(keep, dq, flat)
    got, off = [], 0
    for p in net.parameters():
        got.append(flat[off:off + p.numel()].view(p.shape).cpu().double())
        off += p.numel()

    def torch_grads(dtype):
        stack = torch_stack(net, dtype)
        c = lambda t: t.cpu().to(dtype)                                                  # noqa: E731
        x = torch_rows(c(state), c(action), c(goal), c(sigma), c(noise), c(c_noise))
        value = torch_loss(stack(x).squeeze(-1), c(y), c(w), kind)
        value.backward()
        return value.item(), [p.grad.double() for p in stack.parameters()]

    l64, ref = torch_grads(torch.float64)
    _, t32 = torch_grads(torch.float32)
    floor = TRAIN_BOUNDS["fp32"][2]
    e_hip, e_t32 = grad_errors(got, ref, floor), grad_errors(t32, ref, floor)
    lerr = abs(float(loss) - l64) / abs(l64)
    ratios = [h / max(t, EPS) for h, t in zip(e_hip, e_t32)]
    print(f"fit step {hidden}x{layers} {activation} {kind}: loss rel err {lerr:.3e}; max HIP grad err {max(e_hip):.3e}, max torch fp32 "
          f"err {max(e_t32):.3e}, max ratio {max(ratios):.2f}")
    assert lerr <= TRAIN_BOUNDS["fp32"][0]
    for i, (h, t) in enumerate(zip(e_hip, e_t32)):
        assert h <= 4.0 * max(t, EPS), (i, h, t)


# -------------------------------------------------------------------------------------------------
# 4. the noise-level column in the fused apply
# -------------------------------------------------------------------------------------------------
LAM = 1.5


def restated_guided(guide, state, pred, goal, sigma, dtype):
    """pred + lam * sigma^2 * d sum(q) / da in torch ops on the CPU over copies of the guide's parameters."""
    stack = torch_stack(guide.network, dtype)
    c = lambda t: None if t is None else t.cpu().to(dtype)                              # noqa: E731
    state, pred, goal, sigma = c(state), c(pred), c(goal), c(sigma)
    c_noise = sigma.log() / 4 if guide.use_sigma else None
    with torch.enable_grad():
        a = pred.clone().requires_grad_(True)
        x = torch_rows(state, a, goal, None, None, c_noise)
        grad = torch.autograd.grad(stack(x).sum(), a)[0]
    return (pred + LAM * grad * sigma.view(-1, 1, 1) ** 2).detach()


@pytest.mark.parametrize("goal", [None, "shared", "own"])
@pytest.mark.parametrize("hidden,layers,activation,B,T", [(48, 2, "Mish", 11, 3), (32, 1, "ReLU", 3, 2), (512, 2, "sigmoid", 17, 1)],
                         ids=["48x2", "32x1", "512x2"])
def test_fused_apply_with_the_sigma_column_against_the_generic_path(hidden, layers, activation, B, T, goal):
    torch.manual_seed(0)
    net = MLPNetwork(OBS + ACT + (OBS if goal else 0) + 1, hidden, layers, 1, activation=activation, device=DEV)
    if activation == "sigmoid":                # as tests/test_classifier_guidance.py: keep the gradient off the rounding floor
        with torch.no_grad():
            for lin in net.layers:
                lin.weight.mul_(4.0)
    guide = MLPGuide(net, use_goal=goal is not None, use_sigma=True)
    state, pred, goal, sigma, _ = inputs(B, T, T + 1, goal)
    sigma = sigma + 0.3
    assert guide.fused_supported(OBS, ACT, goal is not None)
    calls = []
    real = guide.apply
    guide.apply = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    fused = ClassifierGuidedSampleModel(Stub(pred), guide, cond_lambda=LAM)
    generic = ClassifierGuidedSampleModel(Stub(pred), lambda s, a, g: guide(s, a, g, sigma), cond_lambda=LAM)
    with torch.no_grad():
        out = fused(state, pred, goal, sigma)
        n_fused = len(calls)
        out_generic = generic(state, pred, goal, sigma)
    assert n_fused == 1 and len(calls) == 1
    ref, t32 = restated_guided(guide, state, pred, goal, sigma, torch.float64), restated_guided(guide, state, pred, goal, sigma, torch.float32)
    tag = f"sigma-column guide {hidden}x{layers} {activation} B={B} T={T}"
    check_bars(tag + " fused", out, pred, t32, ref)
    check_bars(tag + " fused against generic", out, pred, t32, out_generic.cpu().double(), increment=False)
    # the column is read: another sigma in the column alone (lam sigma^2 as before) moves the output
    c_other = (sigma * 3.0).log() / 4
    ptrs, n = net._pointers(None)
    moved = torch.empty_like(pred)
    st = _lib.load_guidefit().beso_guide_apply_sigma(ptrs, n, C.byref(net.dims()), ptr(state), ptr(goal), ptr(pred), ptr(sigma), ptr(c_other),
                                                     B, T, state.shape[1], 0 if goal is None else goal.shape[1],
                                                     0 if goal is None else goal.shape[0], OBS, ACT, LAM, moved.data_ptr(), stream())
    assert st == _lib.OK and not torch.equal(moved, out)


@pytest.mark.parametrize("goal", [None, "own"])
def test_a_guide_without_use_sigma_returns_the_bits_of_beso_guide_apply(goal):
    B, T = 11, 3
    torch.manual_seed(0)
    net = MLPNetwork(OBS + ACT + (OBS if goal else 0), 48, 2, 1, activation="Mish", device=DEV)
    guide = MLPGuide(net, use_goal=goal is not None)
    state, pred, goal, sigma, _ = inputs(B, T, T, goal)
    got = guide.apply(state, pred, goal, sigma, LAM)
    ptrs, n = net._pointers(None)
    want = torch.empty_like(pred)
    st = _lib.load_guide().beso_guide_apply(ptrs, n, C.byref(net.dims()), ptr(state), ptr(goal), ptr(pred), ptr(sigma), B, T, T,
                                            0 if goal is None else G, 0 if goal is None else B, OBS, ACT, LAM, want.data_ptr(), stream())
    assert st == _lib.OK and torch.equal(got, want) and not torch.equal(got, pred)
    with pytest.raises(ValueError, match="without use_sigma"):
        guide(state, pred, goal, sigma)


# -------------------------------------------------------------------------------------------------
# 5. twenty steps against a float64 twin
# -------------------------------------------------------------------------------------------------
# The largest relative deviation of a step's loss from the twin's over the 20 steps, measured on an MI355X on the first run of this
# test.  The bound is 4x that (box-to-box fp32 differences in expf, the reduction order) and may never exceed 1e-3.
TWIN_MEASURED = 3.087e-07
TWIN_BOUND = 4 * TWIN_MEASURED


def test_twenty_steps_follow_a_float64_twin_with_plain_adam():
    """B = 64, T = 2, target -|a - a*(state)|^2 with a* a fixed linear map of the state, guide 14 -> 48 x 2 -> 1 Mish with the
    noise-level column, lr 1e-2, the same sigma and noise in both runs.  Measured on an MI355X: loss 39.064 at step 1, 32.262 at
    step 20; largest relative deviation of a step's loss from the twin 3.087e-7; parameters after the 20 steps within 3.3e-6 of
    max |twin|."""
    B, T, steps, lr = 64, 2, 20, 1e-2
    torch.manual_seed(0)
    net = MLPNetwork(2 * OBS + ACT + 1, 48, 2, 1, activation="Mish", device=DEV)
    guide = MLPGuide(net, use_sigma=True)
    twin = torch_stack(net, torch.float64, DEV)
    opt = torch.optim.Adam(twin.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    trainer = GuideTrainer(guide, lr=lr, betas=(0.9, 0.999), weight_decay=0.0, loss="mse", seed=0)
    g = torch.Generator().manual_seed(7)
    a_star = torch.randn(OBS, ACT, generator=g).to(DEV) / OBS ** 0.5
    got, want = [], []
    for i in range(steps):
        state, action, goal, sigma, noise = inputs(B, T, T, "own", seed=100 + i)
        target = -((action - state @ a_star) ** 2).sum(-1)
        got.append(trainer.train_step(state, action, goal, target, sigma=sigma, noise=noise))
        d = lambda t: t.double()                                                        # noqa: E731
        x = torch_rows(d(state), d(action), d(goal), d(sigma), d(noise), d(sigma).log() / 4)
        loss = ((twin(x).squeeze(-1) - d(target).reshape(-1)) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        want.append(loss.detach())
    assert all(v.dim() == 0 and v.is_cuda for v in got)
    got, want = torch.stack(got).cpu().double(), torch.stack(want).cpu()
    dev = ((got - want).abs() / want.abs()).max().item()
    perr = max(((p.detach().double() - q.detach()).abs().max() / q.detach().abs().max()).item() for p, q in zip(net.parameters(), twin.parameters()))
    print(f"twin run: loss step 1 {got[0]:.6f} -> step 20 {got[-1]:.6f}; max relative deviation of a step's loss from the fp64 twin "
          f"{dev:.3e}; parameters after 20 steps: {perr:.3e} of max |twin|")
    assert got[-1] < got[0]
    assert TWIN_BOUND <= 1e-3 and dev <= TWIN_BOUND


# -------------------------------------------------------------------------------------------------
# 6. determinism and resume
# -------------------------------------------------------------------------------------------------
def _three_steps(kind, resume_after=None):
    torch.manual_seed(1)
    guide = MLPGuide(MLPNetwork(2 * OBS + ACT + 1, 32, 2, 1, activation="Mish", device=DEV), use_sigma=True)
    draw = torch.Generator().manual_seed(11)
    density = lambda shape, device: (0.05 + torch.rand(shape, generator=draw)).to(device)      # noqa: E731
    trainer = GuideTrainer(guide, lr=1e-2, loss=kind, sample_density=density, seed=5)
    losses = []
    for i in range(3):
        if resume_after == i:                       # a new guide and trainer, other weights and seed, loaded from the old one's state
            saved = trainer.state_dict()
            torch.manual_seed(99)
            guide = MLPGuide(MLPNetwork(2 * OBS + ACT + 1, 32, 2, 1, activation="Mish", device=DEV), use_sigma=True)
            trainer = GuideTrainer(guide, lr=1e-2, loss=kind, sample_density=density, seed=77)
            trainer.load_state_dict(saved)
        state, action, goal, _, _ = inputs(11, 3, 3, "shared", seed=20 + i)
        target = torch.rand(11, 3, generator=torch.Generator().manual_seed(30 + i)).to(DEV)
        weight = torch.rand(11, 3, generator=torch.Generator().manual_seed(40 + i)).to(DEV)
        losses.append(trainer.train_step(state, action, goal, target, weight=weight))
    return torch.stack(losses), [p.detach().clone() for p in guide.parameters()]


@pytest.mark.parametrize("kind", ["mse", "bce"])
def test_same_seed_same_bits_and_a_checkpoint_resumes_them(kind):
    l0, p0 = _three_steps(kind)
    l1, p1 = _three_steps(kind)
    assert bool(torch.isfinite(l0).all()) and torch.equal(bits(l0), bits(l1))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(p0, p1))
    l2, p2 = _three_steps(kind, resume_after=2)
    assert torch.equal(bits(l0), bits(l2)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(p0, p2))
    assert not torch.equal(l0[0], l0[2])


# -------------------------------------------------------------------------------------------------
# 7. no result depends on what its buffer held
# -------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_what_the_buffers_held_and_guards_stay():
    B, T = 11, 3
    torch.manual_seed(0)
    net = MLPNetwork(2 * OBS + ACT + 1, 48, 2, 1, activation="Mish", device=DEV)
    guide = MLPGuide(net, use_sigma=True)
    state, action, goal, sigma, noise = inputs(B, T, 4, "own")
    c_noise = sigma.log() / 4
    y, w = torch.rand(B * T, device=DEV), torch.rand(B * T, device=DEV)
    rows0 = fit_rows(state, action, goal, sigma, noise, c_noise)
    q = net.run_forward(rows0, keep=False)[0].reshape(-1)
    base = {kind: fit_loss(q, y, w, kind) for kind in KINDS}
    out0 = guide.apply(state, action, goal, sigma, LAM)
    for name, fill in FILLS.items():
        buf, rows = banded_out(rows0.shape, fill)
        fit_rows(state, action, goal, sigma, noise, c_noise, out=rows)
        assert torch.equal(bits(rows), bits(rows0)) and guards_intact(buf), name
        for kind in KINDS:
            pairs = [banded_out(s, fill) for s in ((1,), (B * T,), (B * T,))]
            fit_loss(q, y, w, kind, outs=tuple(p[1] for p in pairs))
            for (buf, got), want, what in zip(pairs, base[kind], ("loss", "per_row", "dq")):
                assert torch.equal(bits(got), bits(want)) and guards_intact(buf), (name, kind, what)
        buf, out = banded_out(action.shape, fill)
        guide.apply(state, action, goal, sigma, LAM, out=out)
        assert torch.equal(bits(out), bits(out0)) and guards_intact(buf), name
