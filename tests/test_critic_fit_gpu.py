"""The IQL critic's fit step on the MI355X: ``beso_critic_rows`` / ``beso_critic_loss`` (include/beso_critic_fit.h,
csrc/critic_fit.hip) and ``CriticTrainer`` (k_diffusion/critic_fit.py).

Arbiters: tests/test_critic_fit.py's torch re-statement of the rows (``cat``, bit for bit) and its float32 numpy re-statement of the
loss launch's rounding order (bit for bit); torch autograd in fp64 over torch copies of both networks with a detached target and a
detached v_next (gradients: tests/test_guide_fit_gpu.py's rule, at most 4x what fp32 torch autograd errs); the optimizer launch's EMA
arithmetic evaluated exactly (the target, bit for bit); a float64 torch twin with plain Adam and a Polyak target (20 steps); and
``beso_mlp_fwd`` on the assembled rows (the scores ``select='value'`` ranks by, bit for bit).  Shapes: obs 3, act 2, T 3, G 2."""
import copy
from fractions import Fraction

import numpy as np
import pytest
import torch

from beso_amd import _lib
from beso_amd.agents.diffusion_agents.k_diffusion.critic_fit import CriticTrainer, StateValue
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
from beso_amd.networks.mlps.mlps import MLPNetwork
from oracle import beso_oracle as O
from support import TRAIN_BOUNDS, bits, grad_errors
from test_classifier_guidance import FILLS, banded_out, guards_intact
from test_critic_fit import EXPECTILE, GAMMA, SIZES, loss_inputs, restated_losses, torch_rows
from test_guide_fit_gpu import torch_stack
from test_rollout_candidates import _agent, _Feed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OBS, ACT, T, G = 3, 2, 3, 2
EPS = 2.0 ** -24        # one fp32 rounding
LOSS_OUTPUTS = ("loss_q", "loss_v", "per_row_q", "per_row_v", "dq", "dv", "adv")


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def inputs(B, goal, steps=T + 1, seed=1):
    """state [B, steps, obs], action, goal (None / 'own' [B, G, obs] / 'shared' [1, G, obs]), next_state, reward, done, weight."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    state, action, goals, nxt, reward = r(B, steps, OBS), r(B, T, ACT), r(B, G, OBS), r(B, T, OBS), r(B, T)
    done = (torch.rand(B, T, generator=g) < 0.25).float().to(DEV)
    weight = torch.rand(B, T, generator=g).to(DEV)
    return state, action, (None if goal is None else goals[:1].contiguous() if goal == "shared" else goals), nxt, reward, done, weight


def critic_rows(state, action, goal, next_state, outs=None):
    B = action.shape[0]
    gw = 0 if goal is None else OBS
    q_rows, v_rows = outs or (torch.empty(B * T, OBS + ACT + gw, device=DEV), torch.empty(2 * B * T, OBS + gw, device=DEV))
    st = _lib.load_critic().beso_critic_rows(ptr(state), ptr(next_state), ptr(action), ptr(goal), B, T, state.shape[1],
                                             0 if goal is None else goal.shape[1], 0 if goal is None else goal.shape[0], OBS, ACT,
                                             q_rows.data_ptr(), v_rows.data_ptr(), stream())
    assert st == _lib.OK, _lib.load_critic().beso_critic_last_error()
    return q_rows, v_rows


def critic_loss(arrays, w, outs=None, gamma=GAMMA, expectile=EXPECTILE):
    """``arrays``: q, q_target, v, v_next, reward, done as numpy float32 [M] -> the seven outputs by name (device tensors)."""
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    w = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float32)).to(DEV)
    M = dev[0].numel()
    outs = outs or [torch.empty(1 if name.startswith("loss") else M, device=DEV) for name in LOSS_OUTPUTS]
    st = _lib.load_critic().beso_critic_loss(*(t.data_ptr() for t in dev), ptr(w), M, gamma, expectile, *(t.data_ptr() for t in outs), stream())
    assert st == _lib.OK, _lib.load_critic().beso_critic_last_error()
    return dict(zip(LOSS_OUTPUTS, outs))


def same_bits(got, want):
    got, want = got.cpu().numpy().reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    return np.array_equal(got.view(np.int32), want.view(np.int32))


# -------------------------------------------------------------------------------------------------
# 1. rows
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given_next", [False, True], ids=["next_from_state", "next_state_given"])
@pytest.mark.parametrize("goal", [None, "shared", "own"])
@pytest.mark.parametrize("B", [3, 11])
def test_rows_are_the_bits_of_the_torch_restatement_whatever_the_buffers_held(B, goal, given_next):
    """M = 9 and 33 rows: under one and over one 256-thread workgroup of elements per block, three blocks in one launch."""
    state, action, goal, nxt, _, _, _ = inputs(B, goal, steps=T + (0 if given_next else 2))
    nxt = nxt if given_next else None
    want = torch_rows(state, action, goal, nxt)
    assert want[0].shape == (B * T, OBS + ACT + (0 if goal is None else OBS)) and want[1].shape[0] == 2 * B * T
    for name, fill in FILLS.items():
        (bq, q_rows), (bv, v_rows) = banded_out(want[0].shape, fill), banded_out(want[1].shape, fill)
        critic_rows(state, action, goal, nxt, outs=(q_rows, v_rows))
        assert torch.equal(bits(q_rows), bits(want[0])) and torch.equal(bits(v_rows), bits(want[1])), name
        assert guards_intact(bq) and guards_intact(bv), name
    # the next-state block is what it says: state shifted by one step, or the given tensor
    M = B * T
    assert torch.equal(v_rows[M:, :OBS], (state[:, 1:T + 1] if nxt is None else nxt).reshape(M, OBS))
    assert not torch.equal(v_rows[M:, :OBS], v_rows[:M, :OBS])


# -------------------------------------------------------------------------------------------------
# 2. the loss launch
# -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weights_with_zeros"])
@pytest.mark.parametrize("M", SIZES)
def test_loss_launch_is_the_bits_of_the_stated_order(M, weighted):
    *arrays, w = loss_inputs(M)
    w = w if weighted else None
    want = restated_losses(*arrays, w)
    pairs = [banded_out((1 if name.startswith("loss") else M,), 0xFF) for name in LOSS_OUTPUTS]
    got = critic_loss(arrays, w, outs=[p[1] for p in pairs])
    for name, (buf, _) in zip(LOSS_OUTPUTS, pairs):
        assert same_bits(got[name], want[name]), (name, np.abs(got[name].cpu().numpy().reshape(-1) - np.asarray(want[name]).reshape(-1)).max())
        assert guards_intact(buf), name
    assert float(got["loss_q"]) > 0 and float(got["loss_v"]) > 0
    if weighted:
        assert not got["dq"].cpu().numpy()[1::3].any() and not got["dv"].cpu().numpy()[1::3].any()


def test_zero_weights_nan_containment_and_the_expectile_branch_at_zero():
    *arrays, _ = loss_inputs(33)
    got = critic_loss(arrays, np.zeros(33))
    zero = torch.zeros(33, dtype=torch.int32, device=DEV)
    assert torch.equal(bits(got["loss_q"]), zero[:1]) and torch.equal(bits(got["loss_v"]), zero[:1])
    assert torch.equal(bits(got["dq"]), zero) and torch.equal(bits(got["dv"]), zero)
    assert bool((got["per_row_q"] > 0).any()) and bool(torch.isfinite(got["per_row_q"]).all())      # each row's loss is still reported
    # a NaN reward in one row: L_Q is NaN, L_V is not, and no other row's dq sees it
    arrays[4][5] = np.nan
    for w in (None, loss_inputs(33)[-1]):
        got = critic_loss(arrays, w)
        want = restated_losses(*arrays, w)
        dq = got["dq"].cpu().numpy()
        assert np.isnan(float(got["loss_q"])) and np.isfinite(float(got["loss_v"])) and np.isnan(dq[5])
        assert np.isfinite(np.delete(dq, 5)).all() and bool(torch.isfinite(got["dv"]).all())
        assert same_bits(got["loss_v"], want["loss_v"]) and same_bits(got["dv"], want["dv"]) and same_bits(torch.from_numpy(np.delete(dq, 5)), np.delete(want["dq"], 5))
    # u = 0 and u = -0 take `expectile`; done = 1 removes v_next
    z = np.zeros(4, dtype=np.float32)
    q_target, v = np.array([1.5, -0.0, 0.0, -2.0], dtype=np.float32), np.array([1.5, 0.0, -0.0, 0.0], dtype=np.float32)
    v_next, done = np.array([3.0, -1e30, 250.0, 7.0], dtype=np.float32), np.array([1.0, 1.0, 1.0, 0.0], dtype=np.float32)
    edge = (z + np.float32(0.3), q_target, v, v_next, z + np.float32(0.7), done)
    got, want = critic_loss(edge, None), restated_losses(*edge)
    for name in LOSS_OUTPUTS:
        assert same_bits(got[name], want[name]), name
    d = np.float32(0.3) - np.float32(0.7)
    assert got["per_row_q"].cpu().numpy()[:3].tolist() == [d * d] * 3 and not got["per_row_v"].cpu().numpy()[:3].any()


# -------------------------------------------------------------------------------------------------
# 3. the whole step against autograd
# -------------------------------------------------------------------------------------------------
def make_trainer(hidden, layers, goal=True, activation="Mish", seed=0, **kw):
    torch.manual_seed(seed)
    gw = OBS if goal else 0
    q = MLPGuide(MLPNetwork(OBS + ACT + gw, hidden, layers, 1, activation=activation, device=DEV), use_goal=goal)
    v = StateValue(MLPNetwork(OBS + gw, hidden, layers, 1, activation=activation, device=DEV), use_goal=goal)
    return CriticTrainer(q, v, **kw)


def twin_losses(q_stack, target_stack, v_stack, state, action, goal, nxt, reward, done, weight, gamma, expectile, dtype, nodes=None):
    """(L_Q, L_V) in torch ops over torch copies of the networks: the target's q and v_next are detached.  ``nodes``: a list that
    takes the graph's q [M] and v [M]."""
    c = lambda t: None if t is None else t.to(dtype)                                      # noqa: E731
    q_rows, v_rows = torch_rows(c(state), c(action), c(goal), c(nxt))
    M = q_rows.shape[0]
    q = q_stack(q_rows).squeeze(-1)
    with torch.no_grad():
        q_target = target_stack(q_rows).squeeze(-1)
    v2 = v_stack(v_rows).squeeze(-1)
    v, v_next = v2[:M], v2[M:].detach()
    if nodes is not None:
        nodes.extend((q, v))
    w = torch.ones(M, dtype=dtype, device=q.device) if weight is None else c(weight).reshape(-1)
    gamma, tau = float(np.float32(gamma)), float(np.float32(expectile))                   # the fp32 values the C ABI takes
    u = q_target - v
    e = torch.where(u < 0, torch.full_like(u, 1.0 - tau), torch.full_like(u, tau))
    d = q - (c(reward).reshape(-1) + gamma * (1.0 - c(done).reshape(-1)) * v_next)
    return (w * d * d).sum() / w.sum(), (w * e * u * u).sum() / w.sum()


@pytest.mark.parametrize("target", ["above_v", "around_v"])
@pytest.mark.parametrize("activation", ["ReLU", "Mish"])
@pytest.mark.parametrize("hidden,layers,B", [(16, 1, 3), (48, 2, 11)], ids=["16x1_B3", "48x2_B11"])
def test_whole_step_gradients_match_fp64_autograd_as_closely_as_torch_fp32_does(hidden, layers, B, activation, target):
    """One ``train_step`` with lr = 0: the parameters' ``.grad`` against fp64 autograd of L_Q alone (Q) and of L_V alone (V), no
    worse than 4x what torch's own fp32 evaluation deviates.  The target is not q here, so that L_V is not a function of q - v;
    tau = 0 holds it still (with tau > 0 it would move towards q whatever the learning rate): it keeps its bits.

    ``around_v``: u = q_target - v takes both signs, so both expectile branches of dv go through V's backward.  V's output-bias
    gradient -- one number, the sum of dv -- is then a cancelling sum (at 48 x 2 ReLU 24x smaller than the sum of |dv|), and every
    fp32 evaluation of it, torch's included, is that much worse conditioned: 4x what ONE fp32 evaluation of one number happens to
    deviate measures the draw.  That single entry is therefore measured against what it is the sum of, sum |dv|, in this case; every
    other tensor, and every tensor of ``above_v`` (the target's output bias shifted by 0.5: u > 0 almost everywhere, no cancellation),
    is measured against itself."""
    tr = make_trainer(hidden, layers, activation=activation, lr=0.0, tau=0.0)
    with torch.no_grad():                       # a target that is not q: q_target - v must not be q - v
        for t in tr.q_target_params:
            t.add_(0.05 * torch.randn(t.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
        if target == "above_v":
            tr.q_target_params[-1].add_(0.5)
    state, action, goal, nxt, reward, done, weight = inputs(B, "own")
    before = [t.detach().clone() for t in (*tr.q_target_params, *tr.q_params, *tr.v_params)]
    loss_q, loss_v = tr.train_step(state, action, goal, reward, done, weight=weight)
    assert loss_q.dim() == 0 and loss_v.dim() == 0 and loss_q.is_cuda and loss_v.is_cuda
    after = (*tr.q_target_params, *tr.q_params, *tr.v_params)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(before, after)), "lr = 0, tau = 0: the target and the parameters keep their bits"
    got_q, got_v = [p.grad.cpu().double() for p in tr.q_params], [p.grad.cpu().double() for p in tr.v_params]

    def torch_grads(dtype):
        q_stack, v_stack = torch_stack(tr.q.network, dtype), torch_stack(tr.v.network, dtype)
        target_stack = copy.deepcopy(q_stack)
        with torch.no_grad():
            for p, t in zip(target_stack.parameters(), before):
                p.copy_(t.cpu().to(dtype))
        cpu = lambda t: t.cpu()                                                            # noqa: E731
        nodes = []
        lq, lv = twin_losses(q_stack, target_stack, v_stack, cpu(state), cpu(action), cpu(goal), None, cpu(reward), cpu(done), cpu(weight),
                             tr.gamma, tr.expectile, dtype, nodes=nodes)
        sum_abs_dv = torch.autograd.grad(lv, nodes[1], retain_graph=True)[0].abs().sum().item()
        # L_Q alone into Q, L_V alone into V: neither reaches the other network (allow_unused would hide a None: none is asked for)
        gq = torch.autograd.grad(lq, list(q_stack.parameters()), retain_graph=True)
        gv = torch.autograd.grad(lv, list(v_stack.parameters()), retain_graph=True)
        assert all(g is None for g in torch.autograd.grad(lv, list(q_stack.parameters()), allow_unused=True, retain_graph=True))
        assert all(g is None for g in torch.autograd.grad(lv, list(target_stack.parameters()), allow_unused=True, retain_graph=True))
        return lq.item(), lv.item(), [g.double() for g in gq], [g.double() for g in gv], sum_abs_dv

    lq64, lv64, ref_q, ref_v, sum_abs_dv = torch_grads(torch.float64)
    _, _, t32_q, t32_v, _ = torch_grads(torch.float32)
    floor = TRAIN_BOUNDS["fp32"][2]
    adv = tr.advantage.cpu()
    if target == "around_v" and B > 3:
        assert int((adv < 0).sum()) >= 3 and int((adv > 0).sum()) >= 3, "both expectile branches are to be taken"
    for name, got, ref, t32, loss, l64 in (("Q", got_q, ref_q, t32_q, loss_q, lq64), ("V", got_v, ref_v, t32_v, loss_v, lv64)):
        e_hip, e_t32 = grad_errors(got, ref, floor), grad_errors(t32, ref, floor)
        if name == "V" and target == "around_v":        # the output bias: the sum of dv, against the sum of |dv|
            cond = sum_abs_dv / abs(ref[-1].item())
            e_hip[-1], e_t32[-1] = (abs((x[-1] - ref[-1]).item()) / sum_abs_dv for x in (got, t32))
            print(f"critic step {hidden}x{layers} {activation} {target}: sum |dv| / |sum dv| = {cond:.1f}")
        lerr = abs(float(loss) - l64) / abs(l64)
        print(f"critic step {hidden}x{layers} {activation} {target} {name}: loss rel err {lerr:.3e}; max HIP grad err {max(e_hip):.3e}, max torch fp32 "
              f"err {max(e_t32):.3e}, max ratio {max(h / max(t, EPS) for h, t in zip(e_hip, e_t32)):.2f}")
        assert lerr <= TRAIN_BOUNDS["fp32"][0]
        for i, (h, t) in enumerate(zip(e_hip, e_t32)):
            assert h <= 4.0 * max(t, EPS), (name, i, h, t)
    assert tr.advantage.shape == (B, T) and tr.per_row_q.shape == (B, T) and tr.per_row_v.shape == (B, T)


# -------------------------------------------------------------------------------------------------
# 4. the target update
# -------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """a * b + c rounded ONCE to float32 (round to nearest, ties to even), from exact rational arithmetic."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = np.float32(float(exact))
    best = None
    for cand in (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        key = (abs(Fraction(float(cand)) - exact), int(np.float32(cand).view(np.int32)) & 1)
        if best is None or key < best[0]:
            best = (key, np.float32(cand))
    return best[1]


def test_the_target_moves_inside_qs_optimizer_launch_by_its_ema_arithmetic():
    """After a step with lr > 0 the target is (1 - tau) old + tau new_q, in the optimizer launch's arithmetic (csrc/optim.hip):
    ``ema = s - (1.0f - decay) * (s - p)`` with decay the fp32 value of 1 - tau, the subtractions rounded to fp32 and the product
    fused into the last one (the launch is compiled with the default contraction: one v_fma_f32) -- bit for bit."""
    tau = 0.05
    tr = make_trainer(16, 1, lr=1e-2, tau=tau)
    state, action, goal, nxt, reward, done, weight = inputs(11, "own")
    for _ in range(2):                            # the second step starts from a target that is no longer q
        old = torch.cat([t.reshape(-1) for t in tr.q_target_params]).cpu().numpy().copy()
        q_before = torch.cat([p.detach().reshape(-1) for p in tr.q_params]).cpu().numpy().copy()
        tr.train_step(state, action, goal, reward, done, next_state=nxt)
        new_q = torch.cat([p.detach().reshape(-1) for p in tr.q_params]).cpu().numpy()
        got = torch.cat([t.reshape(-1) for t in tr.q_target_params]).cpu().numpy()
        c = np.float32(1.0) - np.float32(1.0 - tau)
        diff = old - new_q                                                                # float32, rounded on its own
        want = np.array([fma32(-c, dj, sj) for dj, sj in zip(diff, old)], dtype=np.float32)
        assert (new_q != q_before).mean() > 0.9 and (got != old).mean() > 0.9
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.abs(got - want).max()
        assert np.abs(got.astype(np.float64) - ((1 - tau) * old.astype(np.float64) + tau * new_q.astype(np.float64))).max() <= 4 * EPS * np.abs(old).max()
    assert tr.target.version == 2


# -------------------------------------------------------------------------------------------------
# 5. twenty steps against a float64 twin
# -------------------------------------------------------------------------------------------------
# The largest deviation of a parameter tensor (Q, V and the target) from the twin's after the 20 steps, relative to max |twin| of
# that tensor, measured on an MI355X on the first run of this test.  The bound is 4x that, the margin and form of
# tests/test_guide_fit_gpu.py's twin, and may never exceed 1e-3.
TWIN_MEASURED = 6.845e-07
TWIN_BOUND = 4 * TWIN_MEASURED


def test_twenty_steps_follow_a_float64_twin_with_plain_adam_and_a_polyak_target():
    """B = 32, T = 3, reward -|a - a*(state)|^2 with a* a fixed linear map of the state, a quarter of the rows terminal, Q 8 -> 48 x 2
    -> 1 and V 6 -> 48 x 2 -> 1 Mish, lr 3e-3, tau 0.05, the same data in both runs.  Measured on an MI355X: L_Q 26.7348 at step 1,
    22.0832 at step 20, L_V 0.010451 -> 0.007512; largest relative deviation of a step's losses from the twin 5.159e-7; parameters
    (Q, V and the target) after the 20 steps within 6.845e-7 of max |twin|."""
    B, steps, lr, tau = 32, 20, 3e-3, 0.05
    tr = make_trainer(48, 2, lr=lr, tau=tau)
    q_twin, v_twin = torch_stack(tr.q.network, torch.float64, DEV), torch_stack(tr.v.network, torch.float64, DEV)
    target_twin = copy.deepcopy(q_twin)
    opt_q = torch.optim.Adam(q_twin.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    opt_v = torch.optim.Adam(v_twin.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8)
    g = torch.Generator().manual_seed(7)
    a_star = torch.randn(OBS, ACT, generator=g).to(DEV) / OBS ** 0.5
    got, want = [], []
    for i in range(steps):
        state, action, goal, _, _, done, weight = inputs(B, "own", seed=100 + i)
        reward = -((action - state[:, :T] @ a_star) ** 2).sum(-1)
        got.append(torch.stack(tr.train_step(state, action, goal, reward, done, weight=weight)))
        lq, lv = twin_losses(q_twin, target_twin, v_twin, state, action, goal, None, reward, done, weight, tr.gamma, tr.expectile, torch.float64)
        opt_q.zero_grad()
        opt_v.zero_grad()
        (lq + lv).backward()
        opt_q.step()
        opt_v.step()
        with torch.no_grad():
            for t, p in zip(target_twin.parameters(), q_twin.parameters()):
                t.mul_(1 - tau).add_(tau * p)
        want.append(torch.stack((lq.detach(), lv.detach())))
    got, want = torch.stack(got).cpu().double(), torch.stack(want).cpu()
    ldev = ((got - want).abs() / want.abs()).max().item()
    pairs = list(zip((*tr.q_params, *tr.v_params, *tr.q_target_params), (*q_twin.parameters(), *v_twin.parameters(), *target_twin.parameters())))
    perr = max(((p.detach().double() - t.detach()).abs().max() / t.detach().abs().max()).item() for p, t in pairs)
    print(f"twin run: L_Q {got[0, 0]:.6f} -> {got[-1, 0]:.6f}, L_V {got[0, 1]:.6f} -> {got[-1, 1]:.6f}; max relative deviation of a step's "
          f"losses from the fp64 twin {ldev:.3e}; parameters after 20 steps: {perr:.3e} of max |twin|")
    assert bool(torch.isfinite(got).all()) and got[-1, 0] < got[0, 0]
    assert TWIN_BOUND <= 1e-3 and perr <= TWIN_BOUND


# -------------------------------------------------------------------------------------------------
# 6. determinism and resume
# -------------------------------------------------------------------------------------------------
def _five_steps(resume_after=None):
    tr = make_trainer(16, 2, seed=1, lr=1e-2, tau=0.05, weight_decay=0.01, decoupled_weight_decay=True)
    losses = []
    for i in range(5):
        if resume_after == i:                     # new networks and a new trainer, other weights, loaded from the old one's state
            saved = tr.state_dict()
            tr = make_trainer(16, 2, seed=99, lr=1e-2, tau=0.05, weight_decay=0.01, decoupled_weight_decay=True)
            tr.load_state_dict(saved)
        state, action, goal, nxt, reward, done, weight = inputs(11, "shared", seed=20 + i)
        losses.append(torch.stack(tr.train_step(state, action, goal, reward, done, weight=weight if i % 2 else None)))
    return torch.stack(losses), [t.detach().clone() for t in (*tr.q_params, *tr.v_params, *tr.q_target_params)]


def test_same_inputs_same_bits_and_a_checkpoint_resumes_them():
    l0, p0 = _five_steps()
    l1, p1 = _five_steps()
    assert bool(torch.isfinite(l0).all()) and torch.equal(bits(l0), bits(l1))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(p0, p1))
    l2, p2 = _five_steps(resume_after=2)
    assert torch.equal(bits(l0), bits(l2)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(p0, p2))
    assert not torch.equal(l0[0], l0[4])


# -------------------------------------------------------------------------------------------------
# 7. the trained q ranks candidates
# -------------------------------------------------------------------------------------------------
def test_a_trained_q_is_the_guide_of_value_selection_end_to_end():
    """Three critic steps on O.TINY's dimensions, then ``trainer.q`` as ``guide=`` of ``predict_best_of`` and of
    ``VectorRollout.step`` with ``select='value'``, K = 4: accepted, indices in [0, 4), and the scores are ``beso_mlp_fwd`` of the rows
    ``[newest state | candidate | goal]`` bit for bit."""
    cfg, N, K = O.TINY, 3, 4
    torch.manual_seed(4)
    q = MLPGuide(MLPNetwork(2 * cfg.obs_dim + cfg.act_dim, 48, 2, 1, activation="Mish", device=DEV))
    v = StateValue(MLPNetwork(2 * cfg.obs_dim, 48, 2, 1, activation="Mish", device=DEV))
    tr = CriticTrainer(q, v, lr=1e-2, tau=0.05)
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    start = [p.detach().clone() for p in q.parameters()]
    for _ in range(3):
        losses = tr.train_step(r(8, T + 1, cfg.obs_dim), r(8, T, cfg.act_dim), r(8, cfg.goal_seq_len, cfg.obs_dim), r(8, T), (r(8, T) > 1).float())
    assert all(bool(torch.isfinite(x)) for x in losses) and not any(torch.equal(a, b) for a, b in zip(start, q.parameters()))
    assert tr.q is q

    def scores_of(state, candidates, goal):
        """state [N, obs], candidates [N, K, act], goal [N, G, obs] -> beso_mlp_fwd of the N K rows, [N, K]."""
        rows = torch.cat([state[:, None, :].expand(N, K, -1), candidates, goal[:, -1:, :].expand(N, K, -1)], dim=-1)
        return q.network.run_forward(rows.reshape(N * K, -1).contiguous(), keep=False)[0].view(N, K)

    agent = _agent(cfg)
    feed = _Feed(cfg, N, K, seed=17)
    roll = agent.vector_rollout(N)
    roll.set_goal(feed.goal)
    for step in range(2):
        obs, z = feed()
        roll.step(obs, candidates=K, select="value", guide=tr.q, noise=z)
        last = roll.last
        index, slot = last["index"].long(), (last["lengths"] - 1).long()
        assert bool(((index >= 0) & (index < K)).all()) and tuple(last["scores"].shape) == (N, K)
        want = scores_of(last["state"][torch.arange(N, device=DEV), slot], last["candidates"], roll.goal)
        assert torch.equal(bits(last["scores"]), bits(want)), step
        assert torch.equal(index, last["scores"].argmax(dim=1)), step
    agent.reset()
    obs, z = feed()
    agent.predict_best_of({"observation": obs, "goal_observation": feed.goal}, K, select="value", guide=tr.q, noise=z)
    info = agent.last_best_of
    index = info["index"].long()
    assert bool(((index >= 0) & (index < K)).all()) and tuple(info["scores"].shape) == (N, K)
    want = scores_of(agent.obs_context[-1].to(torch.float32), info["candidates"], roll.goal)
    assert torch.equal(bits(info["scores"]), bits(want)) and torch.equal(index, info["scores"].argmax(dim=1))
