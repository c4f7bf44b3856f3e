"""A bit-reproducible training step and exact checkpoint resume.

``BESO_TRAIN_DETERMINISTIC`` (include/beso_hip.h): the three sums the training step otherwise forms with fp32 atomics -- the
column-sum epilogues of the data-gradient GEMM (FC1 bias, the MLP head's hidden bias), ``colsum_kernel`` and the loss -- are
written as partial sums into a slab of the workspace and added up by a second launch in index order.  On top of it:
``HipTrainStep.run(deterministic=)``, ``BesoAgent(deterministic_training=)``, ``FusedAdam.export_state / import_state``,
``DeviceTrajectoryFeed.state_dict / load_state_dict`` and ``BesoAgent.store_training_state / load_training_state``.

Bounds of the same-function test: ``support.TRAIN_BOUNDS`` (imported) -- the importable form of the bounds that
``test_gpu_parity.test_hip_loss_and_gradients_match_autograd`` applies to the same comparator (tests/autograd_reference.py):
fp32 loss 2e-5, gradients 1e-4 per tensor; bf16 loss 2e-3, gradients 2.6e-2 per tensor.  Everything else here is bit equality.

The feed: 7 trajectories of lengths 12, 15, ..., 30.  With a window of 5 that is 119 windows, eight batches of 16 with a
short last one of 7 (a feed of 7 such trajectories cannot be as small as four batches: the shortest possible one has 74
windows).  The agent test needs the kitchen model's window (4) and uses the same trajectories with it: 126 windows."""

import numpy as np
import pytest
import torch

from beso_amd import _lib
from oracle import beso_oracle as O
from support import TRAIN_BOUNDS, bits, build_agent, make_denoiser, train_inputs

DEV = "cuda:0"
SEED = 4242

_HD4 = O.ScoreGPTConfig(obs_dim=6, act_dim=4, embed_dim=32, n_layers=2, n_heads=8, goal_seq_len=2, obs_seq_len=3,
                        linear_output=True, sigma_data=0.5)                 # hd = 4 (tests/test_buffer_independence.py)
# D = 128: the q / k / v and head weight gradients are a whole number of 128-column tiles wide, so their bias gradients have no
# room for the ones column and go through the column-sum launch (WgradGroup::add -> colsum)
_D128 = O.ScoreGPTConfig(obs_dim=6, act_dim=4, embed_dim=128, n_layers=2, n_heads=4, goal_seq_len=2, obs_seq_len=3,
                         linear_output=True, sigma_data=0.5)
# D = 8 with the MLP head: the head's hidden bias slab (104 columns) is wider than the FC1 one (4 D = 32); at B = 400 it needs
# 14 rows x 104 floats, more than the 38 x 32 the FC1 sums of the 2400 token rows take -- the workspace must cover both
_MLP_D8 = O.ScoreGPTConfig(obs_dim=5, act_dim=2, embed_dim=8, n_layers=1, n_heads=2, goal_seq_len=1, obs_seq_len=2,
                           linear_output=False, sigma_data=1.0)
_CFGS = dict(O.CONFIGS, hd4=_HD4, d128=_D128, mlp_d8=_MLP_D8)
PLANS = {"default": 0, "per_op": _lib.TRAIN_PLAN_PER_OP, "tiles": _lib.TRAIN_PLAN_TILES}

# (shape, batch, precision, plan, attn / resid / embed dropout, cond_mask_prob).  Which site a case reaches, and with how many
# partials per sum:
#   loss (loss_part_kernel, one share per block of 256 elements): every case; kitchen B = 48: 12 shares, B = 192: 48.
#   column-sum epilogue (EpiGeluBwdPart: fp32 and per_op -- the other bf16 plans form the FC1 bias sum elsewhere; two slab rows
#     per 128-row tile): kitchen B = 48 (528 rows): 10 rows, part_reduce_kernel's tail loop only; kitchen B = 192 (2112 rows): 34
#     rows, its eight-loads main loop (from 29 rows on) and the tail.  EpiSiluBwdPart: tiny_mlp_head, B = 70: 4 rows.
#   column-sum launch (colsum_part_kernel, one slab row per 128 rows): d128 B = 40 (360 rows): 3 row blocks for each of q / k / v
#     of both layers, 1 for the head bias; tiny_mlp_head B = 70: 2 row blocks (B = 9: 1).
# Kitchen never reaches the column-sum launch, and under the default bf16 plan it reaches the loss site only.
CASES = [
    ("kitchen", 48, "bf16", "default", 0.0, 0.0, 0.0, 0.0),
    ("kitchen", 48, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("kitchen", 48, "bf16", "per_op", 0.3, 0.1, 0.1, 0.1),
    ("kitchen", 48, "bf16", "tiles", 0.3, 0.1, 0.1, 0.1),
    ("block_push", 40, "bf16", "default", 0.0, 0.05, 0.0, 0.0),
    ("block_push", 40, "fp32", "default", 0.0, 0.05, 0.0, 0.0),
    ("tiny_mlp_head", 9, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("tiny_mlp_head", 70, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("tiny_mlp_head", 70, "bf16", "default", 0.0, 0.0, 0.0, 0.0),
    ("mlp_d8", 400, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("d128", 40, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("d128", 40, "bf16", "default", 0.0, 0.0, 0.0, 0.0),
    ("kitchen", 192, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
    ("kitchen", 192, "bf16", "per_op", 0.0, 0.0, 0.0, 0.0),
    ("hd4", 7, "fp32", "default", 0.0, 0.0, 0.0, 0.0),
]
IDS = ["-".join(str(v) for v in c[:4]) + ("-dropout" if any(c[4:]) else "") for c in CASES]


def _case(cfg_name, B, precision, attn_p, resid_p, embed_p, goal_p):
    cfg = _CFGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, attn_pdrop=attn_p, resid_pdrop=resid_p,
                      embed_pdrop=embed_p, goal_drop=goal_p, train=True)
    return m, train_inputs(cfg, B, seed=4)


def _run(step, inputs, plan, deterministic, **kw):
    """(loss tensor, clone of the flat gradient) of one step into the step's PERSISTENT gradient buffer"""
    from beso_amd.runtime import set_plan
    set_plan(train=PLANS[plan])
    try:
        loss, flat, _ = step.run(*inputs, seed=SEED, fresh_grads=False, deterministic=deterministic, **kw)
    finally:
        set_plan(train=0)
    torch.cuda.synchronize()
    return loss.clone(), flat.clone()


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B,precision,plan,attn_p,resid_p,embed_p,goal_p", CASES, ids=IDS)
def test_flagged_step_gives_equal_bits(cfg_name, B, precision, plan, attn_p, resid_p, embed_p, goal_p):
    """Three flagged runs on the same inputs and seed: the workspace and the gradient buffer hold zeros, then 0xFF bytes, then
    what the previous run left.  The loss and the whole flat gradient are bit-equal."""
    m, inputs = _case(cfg_name, B, precision, attn_p, resid_p, embed_p, goal_p)
    step = m.hip_train_step(*inputs)
    assert step is not None
    ref = _run(step, inputs, plan, True)                                  # (also makes the workspace and the buffer)
    assert torch.isfinite(ref[0]) and bool(torch.isfinite(ref[1]).all())
    for fill in (0, 255, None):
        if fill is not None:
            step._ws.fill_(fill)
            step._flat_full.view(torch.uint8).fill_(fill)
        got = _run(step, inputs, plan, True)
        assert torch.equal(bits(got[0]), bits(ref[0])), (fill, got[0].item(), ref[0].item())
        assert torch.equal(bits(got[1]), bits(ref[1])), fill


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B,precision,plan,attn_p,resid_p,embed_p,goal_p", CASES, ids=IDS)
def test_flagged_step_is_the_same_function(cfg_name, B, precision, plan, attn_p, resid_p, embed_p, goal_p):
    """The flagged step against torch autograd with the library's masks (the comparator and bounds of
    tests/test_dropout_parity.py), and against the unflagged step at the same seed: the six weight-matrix gradients of every
    block are plain stores of the grouped launch, which nothing of the three sites feeds -- bit-equal."""
    from test_dropout_parity import _autograd, _compare
    m, inputs = _case(cfg_name, B, precision, attn_p, resid_p, embed_p, goal_p)
    step = m.hip_train_step(*inputs)
    loss_d, flat_d = _run(step, inputs, plan, True)
    loss_u, flat_u = _run(step, inputs, plan, False)
    views, off = {}, 0
    for n, p in m.named_parameters():
        views[n] = (off, off + p.numel())
        off += p.numel()
    assert off == flat_d.numel()
    weights = [n for n in views if ".blocks." in n and n.endswith(".weight") and ".ln" not in n]
    assert len(weights) == 6 * _CFGS[cfg_name].n_layers, weights
    for n in weights:
        a, b = views[n]
        assert torch.equal(bits(flat_d[a:b]), bits(flat_u[a:b])), n
    got = [flat_d[a:b].view_as(p) for (a, b), p in zip(views.values(), m.parameters())]
    ref_loss, ref = _autograd(m, step, inputs, SEED)
    lerr, gerr = _compare(f"deterministic {cfg_name} B={B} {plan}", m, precision, loss_d.item(), got, ref_loss, ref)
    ltol, gtol, _ = TRAIN_BOUNDS[precision]
    print(f"[reproducible] {cfg_name} {precision} {plan}: flagged loss {loss_d.item()!r}, unflagged {loss_u.item()!r}")
    assert lerr < ltol and gerr < gtol, (lerr, gerr)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_flagged_loss_is_final_on_the_loss_stream(precision):
    """With loss_stream given, the value read on that stream (ordered behind the end of the forward half only) is, bit for
    bit, the value read after a full synchronise: the second-stage reduce of the loss runs in front of the release."""
    m, inputs = _case("kitchen", 48, precision, 0.0, 0.0, 0.0, 0.0)
    step = m.hip_train_step(*inputs)
    side = torch.cuda.Stream(DEV)
    loss, _, _ = step.run(*inputs, seed=SEED, fresh_grads=False, deterministic=True, loss_stream=side)
    with torch.cuda.stream(side):
        early = loss.item()
    torch.cuda.synchronize()
    late = loss.item()
    assert np.float32(early).tobytes() == np.float32(late).tobytes() and np.isfinite(early)
    plain, _ = _run(step, inputs, "default", True)
    assert np.float32(plain.item()).tobytes() == np.float32(late).tobytes()


@pytest.mark.gpu
def test_flag_mirrors_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "beso_hip.h")).read()
    assert int(re.search(r"BESO_TRAIN_DETERMINISTIC\s*=\s*(\d+)", text).group(1)) == _lib.TRAIN_DETERMINISTIC == 8


# ------------------------------------------------------------------------------------------------ optimizer
_OPT_SHAPES = [(1,), (7, 5), (4100,), (3, 9000)]


def _clipped_steps(ps, opt, ema, grads):
    from test_grad_clip import set_grads
    for g in grads:
        set_grads(ps, g)
        opt.step(ema=ema, max_grad_norm=1.0, skip_nonfinite=True)


@pytest.mark.gpu
@pytest.mark.parametrize("receiver_stepped", [False, True])
def test_optimizer_state_round_trip(receiver_stepped):
    """Three clipped steps with skip_nonfinite, the second fed an inf gradient; export_state, import_state into a fresh FusedAdam
    over clones of the parameters (before its first step, or after a step of its own on other gradients); one more step on both:
    parameters, m, v and the EMA shadow bit-equal, skipped_steps() equal (1).  Mismatched sizes raise ValueError."""
    from beso_amd.networks.ema_helper.ema import ExponentialMovingAverage
    from beso_amd.optim import FusedAdam
    from test_grad_clip import assert_bit_equal, make, state_bits
    ps, opt, ema = make(shapes=_OPT_SHAPES)
    torch.manual_seed(21)
    grads = [[torch.randn_like(p) for p in ps] for _ in range(5)]
    grads[1][2].view(-1)[17] = float("inf")
    _clipped_steps(ps, opt, ema, grads[:3])
    assert float(opt.skipped_steps()) == 1.0
    saved = opt.export_state()
    g0 = saved["groups"][0]
    assert all(not t.is_cuda for t in (g0["m"], g0["v"], g0["stats"])) and g0["step"] == 3 and g0["stats"].numel() == 4
    assert g0["hyper"]["lr"] == 1e-3 and g0["hyper"]["decoupled_weight_decay"] is True

    ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = FusedAdam(ps2, lr=5e-2, weight_decay=0.3)                        # (other hyper-parameters: the import brings its own)
    ema2 = ExponentialMovingAverage(ps2, 0.999, DEV)
    if receiver_stepped:
        _clipped_steps(ps2, opt2, ema2, [grads[4]])
        with torch.no_grad():
            for a, b in zip(ps2, ps):
                a.copy_(b)
        handed_out = opt2.skipped_steps()
    opt2.import_state(saved)
    ema2._flat.copy_(ema._flat)
    ema2.num_updates = ema.num_updates
    assert float(opt2.skipped_steps()) == 1.0
    if receiver_stepped:
        assert float(handed_out) == 1.0                                     # a view handed out before the import stays valid
    _clipped_steps(ps, opt, ema, [grads[3]])
    _clipped_steps(ps2, opt2, ema2, [grads[3]])
    assert_bit_equal(state_bits(ps, opt, ema), state_bits(ps2, opt2, ema2))
    assert float(opt2.skipped_steps()) == float(opt.skipped_steps()) == 1.0
    assert opt2._groups[0]["step"] == opt._groups[0]["step"] == 4
    assert torch.equal(opt._groups[0]["stats"].view(torch.int64), opt2._groups[0]["stats"].view(torch.int64))

    other = FusedAdam([torch.nn.Parameter(torch.zeros(9, device=DEV))], lr=1e-3)
    with pytest.raises(ValueError):
        other.import_state(saved)
    two = FusedAdam([dict(params=[ps2[0]]), dict(params=ps2[1:])], lr=1e-3)
    with pytest.raises(ValueError):
        two.import_state(saved)
    assert set(opt.state_dict()) == {"state", "param_groups"}              # torch's own surface is left alone


# ------------------------------------------------------------------------------------------------ feed
_LENGTHS = [12, 15, 18, 21, 24, 27, 30]


def _small_feed(seed, window=5, obs_dim=30, act_dim=9, goal_len=2, batch_size=16):
    from beso_amd.data.trajectory_feed import DeviceTrajectoryFeed
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((len(_LENGTHS), max(_LENGTHS), obs_dim)).astype(np.float32)
    act = rng.uniform(-1, 1, (len(_LENGTHS), max(_LENGTHS), act_dim)).astype(np.float32)
    return DeviceTrajectoryFeed(obs, act, _LENGTHS, window, batch_size, DEV, future_conditional=True, min_future_sep=0,
                                future_seq_len=goal_len, seed=seed)


def _same_batch(a, b):
    return set(a) == set(b) and all(torch.equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.gpu
def test_feed_round_trip():
    """The uninterrupted feed runs three epochs.  A twin is stopped behind batch 2 of epoch 2, its state loaded into a NEW
    feed built with another seed: the remaining batches of epoch 2 and all of epoch 3 are bit-equal to the uninterrupted
    feed's (random future goals: the goal-draw generator continues too).  A feed of another batch size refuses the state."""
    full = _small_feed(seed=11)
    assert full.n_windows == 119 and len(full) == 8
    epochs = [[b for b in full] for _ in range(3)]
    assert epochs[0][-1]["action"].shape[0] == 7                           # the short last batch
    twin = _small_feed(seed=11)
    for _ in twin:
        pass
    it = iter(twin)
    first_two = [next(it), next(it)]
    assert all(_same_batch(a, b) for a, b in zip(first_two, epochs[1][:2]))
    saved = twin.state_dict()
    assert saved["in_epoch"] and saved["yielded"] == 2 and not saved["perm_state"].is_cuda
    fresh = _small_feed(seed=99)
    fresh.load_state_dict(saved)
    # a state taken right after a load -- nothing iterated yet -- is the loaded position, and so is one taken after iter()
    # but before the first batch (a generator starts at its first next())
    echo = fresh.state_dict()
    assert echo["in_epoch"] and echo["yielded"] == 2 and torch.equal(echo["perm_state"], saved["perm_state"])
    assert torch.equal(echo["draw_state"], saved["draw_state"])
    relay = _small_feed(seed=7)
    relay.load_state_dict(echo)
    started = iter(relay)
    echo2 = relay.state_dict()
    assert echo2["in_epoch"] and echo2["yielded"] == 2 and torch.equal(echo2["perm_state"], saved["perm_state"])
    assert _same_batch(next(started), epochs[1][2]) and relay.state_dict()["yielded"] == 3
    rest = [b for b in fresh]
    assert len(rest) == 6 and all(_same_batch(a, b) for a, b in zip(rest, epochs[1][2:]))
    third = [b for b in fresh]
    assert len(third) == 8 and all(_same_batch(a, b) for a, b in zip(third, epochs[2]))
    assert not _same_batch(third[0], epochs[1][0])
    # between two epochs: nothing in progress, the next epoch is a new permutation of the same stream
    between = _small_feed(seed=11)
    for _ in between:
        pass
    s2 = between.state_dict()
    assert not s2["in_epoch"] and s2["yielded"] == 0
    again = _small_feed(seed=5)
    again.load_state_dict(s2)
    assert all(_same_batch(a, b) for a, b in zip([b for b in again], epochs[1]))
    with pytest.raises(ValueError):
        _small_feed(seed=11, batch_size=8).load_state_dict(saved)
    with pytest.raises(ValueError):
        _small_feed(seed=11, window=6).load_state_dict(saved)             # another window table (n_windows)


# ------------------------------------------------------------------------------------------------ agent
def _agent(weight_seed, torch_seed, **extra):
    from beso_amd.networks.scaler.scaler_class import Scaler
    cfg = O.KITCHEN
    torch.manual_seed(torch_seed)
    w = O.make_weights(cfg, seed=weight_seed, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "bf16", attn_pdrop=0.3, train=True), device=DEV, lr=1e-3, **extra)
    agent.lr_scheduler = torch.optim.lr_scheduler.StepLR(agent.optimizer, 1, 0.9)      # changes every step
    rng = np.random.default_rng(0)
    agent.get_scaler(Scaler(rng.standard_normal((64, cfg.obs_dim)).astype(np.float32),
                            rng.uniform(-1, 1, (64, cfg.act_dim)).astype(np.float32), True, DEV))
    agent.set_bounds(agent.scaler)
    return agent


def _steps(agent, stream, feed, n):
    out = []
    for _ in range(n):
        try:
            batch = next(stream[0])
        except StopIteration:
            stream[0] = iter(feed)
            batch = next(stream[0])
        out.append(agent.train_step(batch))
    return out


def _held_out(agent):
    cfg = O.KITCHEN
    g = torch.Generator(device="cpu").manual_seed(77)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                     # noqa: E731
    batch = {"observation": r(8, cfg.obs_seq_len, cfg.obs_dim), "action": r(8, cfg.obs_seq_len, cfg.act_dim).clamp(-1, 1),
             "goal_observation": r(8, cfg.goal_seq_len, cfg.obs_dim)}
    sigma = (torch.rand(8, generator=g) * 0.9 + 0.05).to(DEV)
    noise = r(8, cfg.obs_seq_len, cfg.act_dim)
    return agent.validation_loss(batch, sigma=sigma, noise=noise)


def _agent_state(agent):
    st = agent.optimizer._groups[0]
    torch.cuda.synchronize()
    return ([p.detach().clone() for p in agent.model.parameters()] + [agent.ema_helper._flat.clone(), st["m"].clone(), st["v"].clone(),
            agent.optimizer.last_grad_norm().clone().view(1)])


@pytest.mark.gpu
def test_exact_resume(tmp_path):
    """Agent A takes 6 steps.  Agent B (same construction) takes 3 and stores its training state with the feed's.  Agent C,
    constructed from other weights under another seed and with a feed of another seed, loads it and takes 3 steps: its losses
    equal A's losses 4-6 bit for bit, as do the parameters, the EMA shadow, both moments, `steps`, the scheduler's last LR
    and last_grad_norm(); a validation_loss on a fixed batch right after loading equals A's at step 3 (the packed EMA image
    was rebuilt)."""
    from beso_amd.optim import FusedAdam
    cfg = O.KITCHEN
    kw = dict(deterministic_training=True, max_grad_norm=1.0)
    feed_a = _small_feed(seed=11, window=cfg.obs_seq_len)
    a = _agent(3, 100, **kw)
    assert isinstance(a.optimizer, FusedAdam) and a.deterministic_training
    sa = [iter(feed_a)]
    losses_a = _steps(a, sa, feed_a, 3)
    val_a = _held_out(a)
    losses_a += _steps(a, sa, feed_a, 3)

    feed_b = _small_feed(seed=11, window=cfg.obs_seq_len)
    b = _agent(3, 100, **kw)
    sb = [iter(feed_b)]
    losses_b = _steps(b, sb, feed_b, 3)
    assert [np.float32(v).tobytes() for v in losses_b] == [np.float32(v).tobytes() for v in losses_a[:3]]
    b.store_training_state(str(tmp_path), feed_b)
    assert (tmp_path / "training_state.pth").exists()

    feed_c = _small_feed(seed=500, window=cfg.obs_seq_len)
    c = _agent(4, 200, **kw)
    _held_out(c)                                                           # (C has packed an EMA image of its own weights)
    c.load_training_state(str(tmp_path), feed_c)
    val_c = _held_out(c)
    assert np.float32(val_c).tobytes() == np.float32(val_a).tobytes(), (val_c, val_a)
    sc = [iter(feed_c)]
    losses_c = _steps(c, sc, feed_c, 3)
    print(f"[reproducible] A {losses_a}, C {losses_c}")
    assert [np.float32(v).tobytes() for v in losses_c] == [np.float32(v).tobytes() for v in losses_a[3:]]
    for x, y in zip(_agent_state(a), _agent_state(c)):
        assert torch.equal(bits(x.float()) if x.dtype != torch.float64 else x.view(torch.int64),
                           bits(y.float()) if y.dtype != torch.float64 else y.view(torch.int64))
    assert a.steps == c.steps == 6
    assert a.lr_scheduler.get_last_lr() == c.lr_scheduler.get_last_lr() != [1e-3]
    assert a.optimizer.param_groups[0]["lr"] == c.optimizer.param_groups[0]["lr"]
    assert a.optimizer._groups[0]["step"] == c.optimizer._groups[0]["step"] == 6
    assert a.ema_helper.num_updates == c.ema_helper.num_updates


@pytest.mark.gpu
def test_off_means_off(monkeypatch):
    """An agent built without the keyword runs the existing path: the flags word of its beso_loss_grad_streams call carries
    no bit 8; with the keyword it does."""
    seen = []
    lib = _lib.load()
    real = lib.beso_loss_grad_streams

    def spy(*args):
        seen.append(int(args[13]))
        return real(*args)

    monkeypatch.setattr(lib, "beso_loss_grad_streams", spy)
    cfg = O.KITCHEN
    feed = _small_feed(seed=11, window=cfg.obs_seq_len)
    for extra, want in ((dict(), 0), (dict(deterministic_training=True), _lib.TRAIN_DETERMINISTIC)):
        seen.clear()
        agent = _agent(3, 100, **extra)
        agent.train_step(next(iter(feed)))
        torch.cuda.synchronize()
        assert len(seen) == 1 and seen[0] & _lib.TRAIN_DETERMINISTIC == want, seen
