"""Global gradient-norm clipping and the non-finite guard of the fused optimizer step: ``beso_grad_sumsq`` +
``beso_adam_step_clipped`` (include/beso_hip.h), ``FusedAdam.step(max_grad_norm=, skip_nonfinite=, reduce_sumsq=)`` and
``BesoAgent(max_grad_norm=, skip_nonfinite_steps=)``.  The GPU tests drive a standalone ``FusedAdam`` (no network) except
the agent test; the CPU tests cover the argument checks of the two entry points and the eager-optimizer path."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import rel_err
from support import build_agent, lib, make_denoiser  # noqa: F401

DEV = "cuda:0"
# a 1-element chunk, a chunk that is no multiple of 256, a full 4096 chunk + a 4-element tail, and 280 chunks in all:
# more than the finishing workgroup has threads
SHAPES = [(1,), (7, 5), (4100,), (3, 9000), (1_100_000,)]
BAR = 2e-6          # test_fused_adam_matches_torch's bar for parameters and EMA shadow
ULP = 2.0 ** -23    # one fp32 ulp, relative


def make(kind="adamw", seed=1, shapes=SHAPES):
    """(parameters, FusedAdam, EMA helper) -- the same bits for the same seed."""
    from beso_amd.optim import FusedAdam
    from beso_amd.networks.ema_helper.ema import ExponentialMovingAverage
    torch.manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(*sh, device=DEV) * 0.1) for sh in shapes]
    if kind == "adamw":
        opt = FusedAdam(ps, lr=1e-3, weight_decay=0.01, decoupled_weight_decay=True)
    else:
        opt = FusedAdam(ps, lr=2e-3, weight_decay=0.05)
    return ps, opt, ExponentialMovingAverage(ps, 0.999, DEV)


def make_torch(kind, ps):
    """The torch optimizer + eager EMA over clones of ``ps`` with the hyper-parameters of make()."""
    from beso_amd.networks.ema_helper.ema import ExponentialMovingAverage
    ref_p = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ref = (torch.optim.AdamW(ref_p, lr=1e-3, weight_decay=0.01) if kind == "adamw"
           else torch.optim.Adam(ref_p, lr=2e-3, weight_decay=0.05))
    return ref_p, ref, ExponentialMovingAverage(ref_p, 0.999, DEV)


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        p.grad = g.clone()


def norm64(grads) -> float:
    """sqrt(sum g^2) in float64 on the host (numpy): independent of the code under test."""
    return math.sqrt(sum(float((g.detach().cpu().numpy().astype(np.float64) ** 2).sum()) for g in grads))


def coef_from_norm64(grads, max_norm) -> np.float32:
    """clip_grad_norm_'s coefficient in fp32 arithmetic, from the float64 norm."""
    norm = np.float32(norm64(grads))
    with np.errstate(over="ignore"):
        return np.float32(min(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6))))


def state_bits(ps, opt, ema):
    st = opt._groups[0]
    return [p.detach().clone() for p in ps] + [st["m"].clone(), st["v"].clone(), ema._flat.clone()]


def assert_bit_equal(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_grad_norm_matches_float64_within_one_ulp():
    """last_grad_norm() == float32(sqrt(sum(float64(g)^2))) within 1 fp32 ulp: the squares are exact in double, the double
    sum of 1.2 M terms is good to ~1e-10, one rounding to fp32 remains.  randn gradients, gradients scaled by 1e-20 and 1e15
    (their squares leave fp32's range; the reduction is in double) and all-zero gradients (norm 0, coefficient 1)."""
    ps, opt, ema = make()
    torch.manual_seed(3)
    base = [torch.randn_like(p) for p in ps]
    for scale in (1.0, 1e-20, 1e15, 0.0):
        grads = [g * scale for g in base]
        set_grads(ps, grads)
        opt.step(ema=ema, max_grad_norm=math.inf)
        got, want = float(opt.last_grad_norm()), float(np.float32(norm64(grads)))
        print(f"[grad_clip] scale {scale:g}: norm {got!r} expected {want!r} rel diff {abs(got - want) / max(want, 1e-300):.3e}")
        assert got == float(np.float32(got))                       # an fp32 value
        assert abs(got - want) <= ULP * want
        assert float(opt.last_clip_coef()) == 1.0 and float(opt.skipped_steps()) == 0.0
        if scale == 0.0:
            assert got == 0.0
    assert opt.last_grad_norm().dim() == 0 and opt.last_grad_norm().is_cuda and opt.skipped_steps().is_cuda


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adamw", "adam_l2"])
def test_clipped_step_matches_torch(kind):
    """4 steps of AdamW / Adam with L2 decay, with EMA, max_grad_norm = 1: two steps clip (norm ~1e3), two do not (norm
    ~0.1).  Reference: the coefficient in fp32 from the FLOAT64 norm of the gradients, g * coef as a torch multiply,
    torch.optim.AdamW / Adam and the eager EMA.  Bar: rel_err < 2e-6 on parameters and EMA shadow.  The gradient tensors
    are not rescaled."""
    max_norm = 1.0
    ps, opt, ema = make(kind)
    ref_p, ref, ref_ema = make_torch(kind, ps)
    torch.manual_seed(5)
    coefs = []
    for scale in (1.0, 1e-4, 1e-4, 1.0):
        grads = [torch.randn_like(p) * scale for p in ps]
        set_grads(ps, grads)
        coef = coef_from_norm64(grads, max_norm)
        for p, g in zip(ref_p, grads):
            p.grad = g * float(coef)
        ref.step()
        ref_ema.update(ref_p)
        opt.step(ema=ema, max_grad_norm=max_norm)
        got = float(opt.last_clip_coef())
        coefs.append(got)
        print(f"[grad_clip] {kind} scale {scale:g}: coef {got!r} reference {float(coef)!r}")
        # the norm is within 1 ulp (test above), the division rounds once on either side: 4 ulp covers it
        assert abs(got - float(coef)) <= 4 * ULP * float(coef)
        for p, g in zip(ps, grads):
            assert torch.equal(p.grad, g)                           # the buffer keeps the unclipped gradient
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)
    errs = [rel_err(q.detach().cpu().numpy(), p.detach().cpu().numpy()) for p, q in zip(ref_p, ps)]
    errs_ema = [rel_err(b.cpu().numpy(), a.cpu().numpy()) for a, b in zip(ref_ema.shadow_params, ema.shadow_params)]
    print(f"[grad_clip] {kind}: worst rel err parameters {max(errs):.3e}, EMA {max(errs_ema):.3e}")
    assert max(errs) < BAR and max(errs_ema) < BAR


@pytest.mark.gpu
def test_clipped_step_matches_clip_grad_norm_():
    """One clipped AdamW step against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW + the eager EMA at the same bar
    (torch reduces the norm in fp32; measured on an MI355X: torch's norm and ours are the same fp32 value, 1063.78515625,
    the parameters differ by 6.9e-8 and the EMA shadow by 6.9e-8 relative -- inside the bar, so this comparison is an
    assertion too)."""
    ps, opt, ema = make()
    ref_p, ref, ref_ema = make_torch("adamw", ps)
    torch.manual_seed(6)
    grads = [torch.randn_like(p) for p in ps]
    set_grads(ps, grads)
    set_grads(ref_p, grads)
    total = torch.nn.utils.clip_grad_norm_(ref_p, 1.0)
    ref.step()
    ref_ema.update(ref_p)
    opt.step(ema=ema, max_grad_norm=1.0)
    print(f"[grad_clip] torch's fp32 norm {float(total)!r}, ours {float(opt.last_grad_norm())!r}, float64 {norm64(grads)!r}")
    errs = [rel_err(q.detach().cpu().numpy(), p.detach().cpu().numpy()) for p, q in zip(ref_p, ps)]
    errs_ema = [rel_err(b.cpu().numpy(), a.cpu().numpy()) for a, b in zip(ref_ema.shadow_params, ema.shadow_params)]
    print(f"[grad_clip] against clip_grad_norm_: worst rel err parameters {max(errs):.3e}, EMA {max(errs_ema):.3e}")
    assert float(opt.last_clip_coef()) < 1.0
    assert max(errs) < BAR and max(errs_ema) < BAR


@pytest.mark.gpu
def test_infinite_max_norm_is_the_plain_step_bit_for_bit():
    """max_grad_norm = inf: coefficient exactly 1 -- parameters, moments and EMA bit-equal to a plain step(), and the
    gradient tensors bit-equal to before the call."""
    pa, oa, ea = make()
    pb, ob, eb = make()
    torch.manual_seed(7)
    for _ in range(2):
        grads = [torch.randn_like(p) for p in pa]
        set_grads(pa, grads)
        set_grads(pb, grads)
        oa.step(ema=ea)
        ob.step(ema=eb, max_grad_norm=math.inf)
        assert float(ob.last_clip_coef()) == 1.0
        for p, g in zip(pb, grads):
            assert torch.equal(p.grad.view(torch.int32), g.view(torch.int32))
    assert_bit_equal(state_bits(pa, oa, ea), state_bits(pb, ob, eb))


@pytest.mark.gpu
def test_guard_skips_a_nonfinite_step_and_nothing_else():
    """skip_nonfinite: one inf as the last element of the last chunk, then one NaN in the (1,) tensor -- p, m, v and the EMA
    shadow keep their bits, skipped_steps() reads 1 then 2, last_clip_coef() reads 0.  The finite step that follows equals
    the torch reference of the clipped-step test fed with the step counts the optimizer used (the host counted the two
    skipped steps: bias correction at step 3, EMA warm-up at update 3), and leaves the counter alone.  Without the guard a
    NaN gradient does reach the parameters."""
    max_norm = 1.0
    ps, opt, ema = make()
    ref_p, ref, ref_ema = make_torch("adamw", ps)
    torch.manual_seed(8)
    grads = [torch.randn_like(p) for p in ps]
    set_grads(ps, grads)
    opt.step(ema=ema, max_grad_norm=math.inf, skip_nonfinite=True)          # a good step first: non-trivial m, v, shadow
    set_grads(ref_p, grads)
    ref.step()
    ref_ema.update(ref_p)
    before = state_bits(ps, opt, ema)
    for n_bad, (tensor, value) in enumerate([(len(SHAPES) - 1, math.inf), (0, math.nan)], start=1):
        bad = [g.clone() for g in grads]
        bad[tensor].view(-1)[-1] = value
        set_grads(ps, bad)
        opt.step(ema=ema, max_grad_norm=max_norm, skip_nonfinite=True)
        assert_bit_equal(before, state_bits(ps, opt, ema))
        assert float(opt.skipped_steps()) == n_bad and float(opt.last_clip_coef()) == 0.0
        assert not math.isfinite(float(opt.last_grad_norm()))
    grads = [torch.randn_like(p) for p in ps]
    set_grads(ps, grads)
    opt.step(ema=ema, max_grad_norm=max_norm, skip_nonfinite=True)
    assert opt._groups[0]["step"] == 4 and ema.num_updates == 4
    for p in ref_p:
        ref.state[p]["step"] += 2                                       # the two skipped steps the host counted
    ref_ema.num_updates += 2
    coef = coef_from_norm64(grads, max_norm)
    for p, g in zip(ref_p, grads):
        p.grad = g * float(coef)
    ref.step()
    ref_ema.update(ref_p)
    assert float(opt.skipped_steps()) == 2.0 and 0.0 < float(opt.last_clip_coef()) < 1.0
    errs = [rel_err(q.detach().cpu().numpy(), p.detach().cpu().numpy()) for p, q in zip(ref_p, ps)]
    errs_ema = [rel_err(b.cpu().numpy(), a.cpu().numpy()) for a, b in zip(ref_ema.shadow_params, ema.shadow_params)]
    print(f"[grad_clip] finite step after two skipped: worst rel err parameters {max(errs):.3e}, EMA {max(errs_ema):.3e}")
    assert max(errs) < BAR and max(errs_ema) < BAR
    # the guard is what protects: without it the NaN arrives, as in torch
    pn, on, en = make()
    bad = [g.clone() for g in grads]
    bad[0].view(-1)[-1] = math.nan
    set_grads(pn, bad)
    on.step(ema=en, max_grad_norm=max_norm)
    assert torch.isnan(pn[0]).all() and torch.isnan(en.shadow_params[0]).all() and float(on.skipped_steps()) == 0.0


@pytest.mark.gpu
def test_sharded_clipped_steps_equal_the_full_clipped_step():
    """The 3-way split of test_fused_adam_sharded_steps_equal_the_full_step with clipping: every shard's step gets a
    reduce_sumsq that adds the other shards' stats[0] (from beso_grad_sumsq calls on their tables), as the sharded
    exchange's cross-rank sum does.  Parameters and EMA equal the unsharded clipped step's at rel_err < 2e-6 (the sum order
    differs: no bit equality); everything outside a shard is bit-untouched."""
    from beso_amd import _lib
    from beso_amd.optim import FusedAdam
    shapes = [(7, 5), (4100,), (3, 9000), (1,), (64, 33)]
    max_norm = 1.0

    def make_s():
        ps, opt, ema = make(seed=1, shapes=shapes)
        torch.manual_seed(2)
        for p in ps:
            p.grad = torch.randn_like(p)
        return ps, opt, ema

    pf, of, ef = make_s()
    ps, os_, es = make_s()
    n = sum(p.numel() for p in pf)
    cuts = [0, 4099, 4099 + 13001, n]
    shards = list(zip(cuts[:-1], cuts[1:]))
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    probe = FusedAdam(ps, lr=1e-3)                       # chunk tables over the same gradients, nothing else
    share = []
    for sh in shards:
        st = probe._prepare(0, probe.param_groups[0], sh)
        partial = torch.empty(st["n_chunks"], dtype=torch.float64, device=DEV)
        stats = torch.zeros(4, dtype=torch.float64, device=DEV)
        _lib.check(lib.beso_grad_sumsq(st["table"].data_ptr(), st["n_chunks"], partial.data_ptr(), stats.data_ptr(), stream))
        share.append(stats[0].clone())
    for it in range(3):
        of.step(ema=ef, max_grad_norm=max_norm)
        decay_counted = False
        for k, (lo, hi) in enumerate(shards):
            before = torch.cat([p.detach().reshape(-1) for p in ps]).clone()
            if decay_counted:                       # one EMA update per step: the warm-up counter advances once
                es.num_updates -= 1
            for st in os_._groups:                  # (the step counter too: three launches, one Adam step)
                if st is not None:
                    st["step"] = it
            others = [share[j] for j in range(len(shards)) if j != k]

            def reduce_sumsq(view):
                assert view.shape == (1,) and view.dtype == torch.float64 and view.is_cuda
                for s in others:
                    view.add_(s)

            os_.step(ema=es, shard=(lo, hi), max_grad_norm=max_norm, reduce_sumsq=reduce_sumsq)
            decay_counted = True
            after = torch.cat([p.detach().reshape(-1) for p in ps])
            assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:])
            assert not torch.equal(after[lo:hi], before[lo:hi])
            assert float(os_.last_clip_coef()) < 1.0
            assert abs(float(os_.last_grad_norm()) - float(of.last_grad_norm())) <= ULP * float(of.last_grad_norm())
        for a, b in zip(pf, ps):
            assert rel_err(b.detach().cpu().numpy(), a.detach().cpu().numpy()) < BAR
        assert rel_err(es._flat.cpu().numpy(), ef._flat.cpu().numpy()) < BAR


@pytest.mark.gpu
@pytest.mark.parametrize("fill", ["nan", "0xff"])
def test_results_do_not_depend_on_the_scratch_contents(fill):
    """The tests/test_buffer_independence.py contract for `partial` and stats[0..2]: filled with NaN / 0xFF bytes before a
    call, the results and skipped_steps() are bit-equal to a call on zeroed scratch; two identical calls give equal bits."""
    twins = [make(), make()]
    torch.manual_seed(9)
    grads = [[torch.randn_like(p) for p in twins[0][0]] for _ in range(2)]
    for ps, opt, ema in twins:                                          # two identical calls (they also make the scratch)
        set_grads(ps, grads[0])
        opt.step(ema=ema, max_grad_norm=1.0, skip_nonfinite=True)
    assert_bit_equal(state_bits(*twins[0]), state_bits(*twins[1]))
    assert torch.equal(twins[0][1]._groups[0]["stats"].view(torch.int64), twins[1][1]._groups[0]["stats"].view(torch.int64))
    for i, (ps, opt, ema) in enumerate(twins):
        st = opt._groups[0]
        assert st["partial"].numel() >= st["n_chunks"] == 280
        if i == 0:
            st["partial"].zero_()
            st["stats"][0:3].zero_()
        elif fill == "nan":
            st["partial"].fill_(math.nan)
            st["stats"][0:3].fill_(math.nan)
        else:
            st["partial"].view(torch.uint8).fill_(255)
            st["stats"][0:3].view(torch.uint8).fill_(255)
        set_grads(ps, grads[1])
        opt.step(ema=ema, max_grad_norm=1.0, skip_nonfinite=True)
    assert_bit_equal(state_bits(*twins[0]), state_bits(*twins[1]))
    s0, s1 = (t[1]._groups[0]["stats"] for t in twins)
    assert torch.equal(s0.view(torch.int64), s1.view(torch.int64))
    assert float(twins[1][1].skipped_steps()) == 0.0 and 0.0 < float(twins[1][1].last_clip_coef()) < 1.0


@pytest.mark.gpu
def test_agent_clips_and_guards_through_train_step():
    """A TINY agent with max_grad_norm small enough to clip and skip_nonfinite_steps: two train_steps run, last_grad_norm()
    is finite and positive, nothing was skipped.  Then a batch with a NaN action -- a non-finite gradient through the
    ordinary path -- leaves the parameters and the EMA shadow bit-equal and the counter at 1 (the returned loss may be
    NaN: that is what the user sees)."""
    from beso_amd.optim import FusedAdam
    from beso_amd.networks.scaler.scaler_class import Scaler
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32"), device=DEV, max_grad_norm=1e-3, skip_nonfinite_steps=True)
    assert isinstance(agent.optimizer, FusedAdam) and agent.max_grad_norm == 1e-3 and agent.skip_nonfinite_steps
    agent.get_scaler(Scaler(np.random.default_rng(0).standard_normal((64, cfg.obs_dim)).astype(np.float32),
                            np.random.default_rng(1).standard_normal((64, cfg.act_dim)).astype(np.float32), True, DEV))
    agent.set_bounds(agent.scaler)
    torch.manual_seed(7)
    batch = {"observation": torch.randn(16, cfg.obs_seq_len, cfg.obs_dim, device=DEV),
             "action": torch.randn(16, cfg.obs_seq_len, cfg.act_dim, device=DEV),
             "goal_observation": torch.randn(16, cfg.goal_seq_len, cfg.obs_dim, device=DEV)}
    losses = [agent.train_step(batch) for _ in range(2)]
    norm = float(agent.last_grad_norm())
    assert all(math.isfinite(v) for v in losses) and math.isfinite(norm) and norm > 1e-3
    assert float(agent.optimizer.last_clip_coef()) < 1.0 and float(agent.skipped_steps()) == 0.0
    params = [p.detach().clone() for p in agent.model.parameters()]
    shadow = agent.ema_helper._flat.clone()
    bad = dict(batch, action=batch["action"].clone())
    bad["action"][3, 0, 0] = math.nan
    agent.train_step(bad)
    assert float(agent.skipped_steps()) == 1.0 and not math.isfinite(float(agent.last_grad_norm()))
    for a, b in zip(params, agent.model.parameters()):
        assert torch.equal(a.view(torch.int32), b.detach().view(torch.int32))
    assert torch.equal(shadow.view(torch.int32), agent.ema_helper._flat.view(torch.int32))
    assert math.isfinite(agent.train_step(batch)) and float(agent.skipped_steps()) == 1.0       # and training goes on
    assert not torch.equal(shadow, agent.ema_helper._flat)


# ------------------------------------------------------------------------------------------------ CPU
def test_new_entry_points_reject_bad_arguments_without_touching_the_device(lib):
    """beso_grad_sumsq / beso_adam_step_clipped: null pointers with n_chunks > 0, a negative count, max_grad_norm <= 0 and
    NaN are the ABI's bad-argument status (-3) before anything is enqueued -- this test runs without a GPU.  An empty step
    (n_chunks == 0) is a no-op."""
    one = C.c_void_p(0x1000)
    assert lib.beso_grad_sumsq(None, 3, one, one, None) == -3
    assert lib.beso_grad_sumsq(one, 3, None, one, None) == -3
    assert lib.beso_grad_sumsq(one, 3, one, None, None) == -3
    assert lib.beso_grad_sumsq(None, 0, None, None, None) == -3           # stats is written even for an empty table
    assert lib.beso_grad_sumsq(one, -1, one, one, None) == -3

    def step(**k):
        args = dict(chunks=one, n=3, m=one, v=one, ema=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, dec=1, step=1,
                    decay=0.0, stats=one, max_norm=1.0, skip=1, stream=None)
        args.update(k)
        return lib.beso_adam_step_clipped(*args.values())

    for bad in (dict(chunks=None), dict(m=None), dict(v=None), dict(stats=None), dict(n=-1), dict(step=0),
                dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=math.nan), dict(max_norm=-math.inf),
                dict(b1=1.0), dict(ema=one, decay=1.5)):
        assert step(**bad) == -3, bad
    assert step(n=0) == 0 and step(n=0, max_norm=math.inf) == 0
    from beso_amd import _lib
    with pytest.raises(ValueError):
        _lib.check(step(max_norm=0.0), "beso_adam_step_clipped")


def cpu_agent(**extra):
    from test_host_logic import make_module
    from beso_amd.networks.scaler.scaler_class import Scaler
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    agent = build_agent(cfg, lambda: make_module(cfg, w), **extra)
    rng = np.random.default_rng(0)
    agent.get_scaler(Scaler(rng.standard_normal((40, cfg.obs_dim)).astype(np.float32),
                            rng.uniform(-1, 1, (40, cfg.act_dim)).astype(np.float32), True, "cpu"))
    return agent


def manual_step(agent, batch, clip):
    """The eager training step piece by piece (beso_agent.py:215-248), with clip_grad_norm_ in front of optimizer.step()."""
    state, action, goal = agent.process_batch(batch, predict=False)
    agent.model.train()
    loss = agent._loss_backward(state, action, goal)
    if clip is not None:
        torch.nn.utils.clip_grad_norm_(agent.model.get_params(), clip)
    agent.optimizer.step()
    agent.lr_scheduler.step()
    agent.ema_helper.update(agent.model.parameters())
    return loss.item()


def test_cpu_agent_clips_through_clip_grad_norm_(autograd_training):
    """A CPU agent (eager AdamW) with max_grad_norm = m steps exactly like clip_grad_norm_ + optimizer.step() on a twin; the
    default construction takes the unclipped step, bit-equal on a twin; skip_nonfinite_steps without the fused optimizer
    is refused."""
    cfg = O.TINY
    m = 1e-3
    torch.manual_seed(0)
    batch = {"observation": torch.randn(8, cfg.obs_seq_len, cfg.obs_dim),
             "goal_observation": torch.randn(8, cfg.goal_seq_len, cfg.obs_dim),
             "action": torch.rand(8, cfg.obs_seq_len, cfg.act_dim) * 2 - 1}
    finals = {}
    for name, extra, clip in (("clipped", dict(max_grad_norm=m), m), ("default", {}, None)):
        agent, twin = cpu_agent(**extra), cpu_agent()
        assert type(agent.optimizer) is torch.optim.AdamW
        for _ in range(2):
            torch.manual_seed(11)
            la = agent.train_step(batch)
            torch.manual_seed(11)
            lb = manual_step(twin, batch, clip)
            assert la == lb
        for a, b in zip(agent.model.parameters(), twin.model.parameters()):
            assert torch.equal(a, b)
        for a, b in zip(agent.ema_helper.shadow_params, twin.ema_helper.shadow_params):
            assert torch.equal(a, b)
        finals[name] = [p.detach().clone() for p in agent.model.parameters()]
        if clip is not None:
            assert float(agent.last_grad_norm()) > m                    # the step did clip
    assert any(not torch.equal(a, b) for a, b in zip(finals["clipped"], finals["default"]))
    with pytest.raises(ValueError):
        cpu_agent(skip_nonfinite_steps=True)
    with pytest.raises(ValueError):
        cpu_agent(max_grad_norm=0.0)
