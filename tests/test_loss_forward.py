"""The gradient-free score-matching loss (beso_loss_fwd, beso_amd/csrc/lossfwd.hip): ``GCDenoiser.loss`` under
``torch.no_grad()`` in eval mode, ``GCDenoiser.loss_per_sample``, ``BesoAgent.validation_loss`` / ``loss_by_sigma``.

References: the reference implementation's own ``m.loss(...)`` values (tests/golden/*_loss.npz, generated with dropout 0 and
goal_drop 0, so train equals eval) for the scalar, and the CPU oracle evaluated sample by sample -- ``O.score_gpt_forward`` on
``noised * c_in`` and the target formula of ``O.score_matching_loss``, in fp32 as torch evaluates them -- for the per-sample
values.

Bars (relative; per-sample values relative to the largest per-sample value of the call):
  fp32    2e-5, the bar test_hip_training_step_matches_reference_gradients holds the fp32 loss to.
  bf16x3  twice the largest value measured against the fixtures on MI355X, no looser than 1e-4.
  bf16 /  twice the largest value measured against the fixtures on MI355X, capped at the 2e-3 the bf16 TRAINING step's loss
  fp16    is held to.
The measured values are in MEASURED_BY_FIXTURE below (and DESIGN.md 6.1f); every test prints what it measures before it asserts.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import load_golden, weights_from_fixture
from support import bits, count_site_launches, lib, make_denoiser, to_dev  # noqa: F401
from beso_amd import _lib

gpu = pytest.mark.gpu
DEV = "cuda:0"

# relative error of the scalar against the reference's fixture value, measured on MI355X (test_loss_matches_the_reference_values
# prints them), and the largest per precision.  bf16 measures above 1e-3 at the kitchen fixture: its bar is the 2e-3 cap, not 2 x.
MEASURED_BY_FIXTURE = {
    "bf16x3": {"kitchen_loss.npz": 1.688e-6, "block_push_loss.npz": 1.325e-6},
    "bf16": {"tiny_loss.npz": 8.948e-5, "kitchen_loss.npz": 1.056e-3, "block_push_loss.npz": 4.606e-4, "tiny_mlp_head_loss.npz": 5.523e-5},
    "fp16": {"kitchen_loss.npz": 1.579e-5, "block_push_loss.npz": 2.164e-4},
}       # (fp32: 0 ... 2.0e-7)
MEASURED = {p: max(v.values()) for p, v in MEASURED_BY_FIXTURE.items()}
BAR = {"fp32": 2e-5, "bf16x3": min(2 * MEASURED["bf16x3"], 1e-4), "bf16": min(2 * MEASURED["bf16"], 2e-3),
       "fp16": min(2 * MEASURED["fp16"], 2e-3)}

_FIXTURES = [("tiny_loss.npz", "tiny"), ("kitchen_loss.npz", "kitchen"), ("block_push_loss.npz", "block_push"),
             ("tiny_mlp_head_loss.npz", "tiny_mlp_head")]
_ONE_LAUNCH = ("kitchen", "block_push", "long_horizon")       # shapes with the one-launch kernel: bf16x3 and fp16 instances


def _precisions(cfg_name):
    return ("fp32", "bf16", "bf16x3", "fp16") if cfg_name in _ONE_LAUNCH else ("fp32", "bf16")


# ------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _weights(cfg_name, seed=0, std=0.02):
    return O.make_weights(O.CONFIGS[cfg_name], seed=seed, std=std)


@functools.lru_cache(maxsize=None)
def _module(cfg_name, precision, seed=0, std=0.02):
    return make_denoiser(O.CONFIGS[cfg_name], _weights(cfg_name, seed, std), precision)


@functools.lru_cache(maxsize=None)
def _inputs(cfg_name, B, t=None, seed=0):
    """numpy (state, action, goal, noise, sigma): sigma in [0.05, 0.95]"""
    cfg = O.CONFIGS[cfg_name]
    t = cfg.obs_seq_len if t is None else t
    rng = np.random.Generator(np.random.PCG64([seed, B, t]))
    r = lambda *s: rng.standard_normal(s, dtype=np.float32)        # noqa: E731
    return (r(B, t, cfg.obs_dim), r(B, t, cfg.act_dim), r(B, cfg.goal_seq_len, cfg.obs_dim), r(B, t, cfg.act_dim),
            (rng.random(B, dtype=np.float32) * np.float32(0.9) + np.float32(0.05)))


def oracle_rows(w, cfg, state, action, goal, noise, sigma, last_only=False, uncond=False):
    """[B]: the oracle sample by sample -- O.score_gpt_forward on noised * c_in against the target of O.score_matching_loss."""
    sigma = np.asarray(sigma, dtype=np.float32).reshape(-1)
    noised = action + noise * sigma.reshape(-1, 1, 1)
    c_skip, c_out, c_in = [s.reshape(-1, 1, 1) for s in O.get_scalings(sigma, cfg.sigma_data)]
    out = O.score_gpt_forward(w, cfg, state, noised * c_in, goal, sigma, uncond=uncond)
    target = (action - c_skip * noised) / c_out
    sq = (out - target) ** 2
    if last_only:
        sq = sq[:, -1, :]
    return sq.reshape(action.shape[0], -1).mean(1)


@functools.lru_cache(maxsize=None)
def _oracle(cfg_name, B, t=None, last_only=False, seed=0):
    """computed once per case and shared (read only)"""
    s, a, g, n, sg = _inputs(cfg_name, B, t, seed)
    if last_only:
        n = n.copy()
        n[:, :-1] = 0
    rows = oracle_rows(_weights(cfg_name), O.CONFIGS[cfg_name], s, a, g, n, sg, last_only=last_only)
    rows.setflags(write=False)
    return rows


def _rel_rows(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(got.double().cpu().numpy() - ref).max() / ref.max())


def _call(m, cfg_name, B, t=None, seed=0, last_only=False, uncond=False):
    """(loss, per_sample) of ONE runtime call on the module's weights"""
    s, a, g, n, sg = (to_dev(v) for v in _inputs(cfg_name, B, t, seed))
    if last_only:
        n[:, :-1] = 0
    inner = m.inner_model
    with torch.no_grad():
        return inner.runtime(m.sigma_data).loss(inner.packed_weights(), s, a, g, n, sg, uncond=uncond, last_only=last_only,
                                                per_sample=True)


# ------------------------------------------------------------------------------------------------ 1. reference parity
@gpu
@pytest.mark.parametrize("fixture,cfg_name,precision", [(f, c, p) for f, c in _FIXTURES for p in _precisions(c)])
def test_loss_matches_the_reference_values(fixture, cfg_name, precision):
    """model.eval(); with torch.no_grad(): model.loss(...) against the value the REFERENCE's m.loss(...) returned, in every
    precision that has a kernel for the shape (bf16x3 and fp16: the two shipped shapes, as ONE launch at the fused site).
    MEASURED_BY_FIXTURE holds what an MI355X gave."""
    fx = load_golden(fixture)
    cfg = O.CONFIGS[cfg_name]
    w = weights_from_fixture(fx) or O.make_weights(cfg, seed=int(fx["seed"]), std=float(fx["std"]))
    m = make_denoiser(cfg, w, precision)
    m.eval()
    T = lambda k: to_dev(fx[k])          # noqa: E731
    box = [None]

    def run():
        with torch.no_grad():
            box[0] = m.loss(T("state"), T("action"), T("goal"), T("noise"), T("sigma"))

    n_fused = count_site_launches("fused_layer", run)
    loss = box[0]
    assert loss.grad_fn is None and not loss.requires_grad and loss.dim() == 0
    assert all(p.grad is None for p in m.parameters())
    err = abs(loss.item() - float(fx["loss"])) / abs(float(fx["loss"]))
    print(f"[loss_fwd] {fixture} {precision}: loss {loss.item():.7f} reference {float(fx['loss']):.7f} rel err {err:.3e}, "
          f"fused launches {n_fused}")
    if precision == "bf16x3":
        assert n_fused == 1, n_fused                 # all layers of the forward as one launch
    assert err <= BAR[precision], (err, BAR[precision])


# ------------------------------------------------------------------------------------------------ 2. per-sample values
_ROW_CASES = [("tiny", 5, 1), ("tiny", 5, None), ("long_horizon", 3, 32), ("kitchen", 6, None)]


@gpu
@pytest.mark.parametrize("cfg_name,B,t", _ROW_CASES)
def test_per_sample_values_match_the_oracle(cfg_name, B, t):
    """loss_per_sample against the oracle sample by sample: t = 1 (one row, t * act < 64: most lanes idle), the full TINY window,
    the long-horizon window (t * act = 288: several elements per lane) and kitchen; the mean of the per-sample values is the
    scalar of the same call."""
    ref = _oracle(cfg_name, B, t)
    for precision in _precisions(cfg_name):
        m = _module(cfg_name, precision)
        s, a, g, n, sg = (to_dev(v) for v in _inputs(cfg_name, B, t))
        with torch.no_grad():
            rows = m.loss_per_sample(s, a, g, n, sg)
        assert rows.shape == (B,) and rows.grad_fn is None
        err = _rel_rows(rows, ref)
        loss, rows2 = _call(m, cfg_name, B, t)
        mean_err = abs(rows2.double().mean().item() - loss.item()) / abs(loss.item())
        print(f"[loss_fwd] per-sample {cfg_name} B={B} t={t} {precision}: rel err {err:.3e} (largest value {ref.max():.4f}), "
              f"mean-vs-scalar {mean_err:.2e}")
        assert torch.equal(bits(rows), bits(rows2))
        assert mean_err <= 1e-6
        assert err <= BAR[precision], (precision, err)


# ------------------------------------------------------------------------------------------------ 3. pred_last_action_only
@gpu
@pytest.mark.parametrize("cfg_name", ["tiny", "kitchen"])
def test_pred_last_action_only_scores_the_last_step(cfg_name):
    """t = W with noise[:, :-1] zeroed (GCDenoiser.loss does that in place): the oracle's (out[:, -1] - target[:, -1])^2 mean,
    and not the full-window value."""
    cfg = O.CONFIGS[cfg_name]
    B = 5
    ref = _oracle(cfg_name, B, None, last_only=True)
    for precision in _precisions(cfg_name):
        m = _module(cfg_name, precision)
        s, a, g, n, sg = (to_dev(v) for v in _inputs(cfg_name, B))
        with torch.no_grad():
            last = m.loss(s, a, g, n, sg, pred_last_action_only=True)
            assert float(n[:, :-1].abs().max()) == 0.0 and float(n[:, -1].abs().max()) > 0.0      # zeroed in place, like the reference
            rows = m.loss_per_sample(s, a, g, n, sg, pred_last_action_only=True)
            full = m.loss(s, a, g, n, sg)
        err = abs(last.item() - float(ref.astype(np.float64).mean())) / float(ref.astype(np.float64).mean())
        err_rows = _rel_rows(rows, ref)
        gap = abs(full.item() - last.item()) / abs(last.item())
        print(f"[loss_fwd] last-action-only {cfg_name} {precision}: scalar {err:.3e} rows {err_rows:.3e}; full-window value differs by {gap:.2e}")
        assert last.grad_fn is None
        assert err <= BAR[precision] and err_rows <= BAR[precision], (precision, err, err_rows)
        assert gap > BAR[precision], (precision, gap)
    assert cfg.obs_seq_len > 1


# ------------------------------------------------------------------------------------------------ 4. unconditional branch
@gpu
@pytest.mark.parametrize("cfg_name,precision", [("tiny", "fp32"), ("kitchen", "bf16")])
def test_uncond_equals_zero_goals_bit_for_bit(cfg_name, precision):
    m = _module(cfg_name, precision)
    B = 5
    s, a, g, n, sg = (to_dev(v) for v in _inputs(cfg_name, B))
    inner = m.inner_model
    rt, packed = inner.runtime(m.sigma_data), inner.packed_weights()
    with torch.no_grad():
        lu, ru = rt.loss(packed, s, a, g, n, sg, uncond=True, per_sample=True)
        lz, rz = rt.loss(packed, s, a, torch.zeros_like(g), n, sg, per_sample=True)
        lc, rc = rt.loss(packed, s, a, g, n, sg, per_sample=True)
        ru2 = m.loss_per_sample(s, a, g, n, sg, uncond=True)
    assert torch.equal(bits(lu), bits(lz)) and torch.equal(bits(ru), bits(rz)) and torch.equal(bits(ru), bits(ru2))
    assert abs(lu.item() - lc.item()) > BAR[precision] * abs(lc.item())
    assert not torch.equal(bits(ru), bits(rc))
    ref = oracle_rows(_weights(cfg_name), O.CONFIGS[cfg_name], *_inputs(cfg_name, B), uncond=True)
    assert _rel_rows(ru, ref) <= BAR[precision]


# ------------------------------------------------------------------------------------------------ 5. batch sizes
@gpu
@pytest.mark.parametrize("B", [1, 2, 3, 65, 257, 1030])
def test_per_sample_values_do_not_depend_on_the_batch(B):
    """Kitchen bf16 under the PLAN_FUSED hint: around the waves-per-workgroup of the row reduction (4), the 256 threads of the
    final reduction and the instances of the one-launch kernel.  per_sample[b] equals sample b evaluated alone, bit for bit (the
    forward has that property; the per-sample reduction keeps it), and two calls give the same scalar bits."""
    from beso_amd.runtime import plan
    m = _module("kitchen", "bf16")
    inner = m.inner_model
    rt, packed = inner.runtime(m.sigma_data), inner.packed_weights()
    s, a, g, n, sg = (to_dev(v) for v in _inputs("kitchen", B))
    with torch.no_grad(), plan(forward=_lib.PLAN_FUSED):
        loss, rows = rt.loss(packed, s, a, g, n, sg, per_sample=True)
        loss2, rows2 = rt.loss(packed, s, a, g, n, sg, per_sample=True)
        only = rt.loss(packed, s, a, g, n, sg)
        alone = torch.stack([rt.loss(packed, s[b:b + 1], a[b:b + 1], g[b:b + 1], n[b:b + 1], sg[b:b + 1], per_sample=True)[1][0]
                             for b in range(B)])
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(rows), bits(rows2)) and torch.equal(bits(loss), bits(only))
    assert torch.isfinite(rows).all()
    mismatch = (bits(rows) != bits(alone)).nonzero().flatten().tolist()
    assert not mismatch, (B, mismatch[:8])
    assert abs(rows.double().mean().item() - loss.item()) <= 1e-6 * abs(loss.item())


@gpu
@pytest.mark.parametrize("B", [1, 257])
def test_library_plan_choice_matches_the_oracle(B):
    """No hint: B = 1 takes the chip-wide small-batch path, B = 257 the one-launch kernel; both within the bf16 bar."""
    m = _module("kitchen", "bf16")
    box = [None]
    n_small = count_site_launches("small", lambda: box.__setitem__(0, _call(m, "kitchen", B)))
    loss, rows = box[0]
    ref = _oracle("kitchen", B)
    err, err_rows = abs(loss.item() - float(ref.astype(np.float64).mean())) / float(ref.astype(np.float64).mean()), _rel_rows(rows, ref)
    print(f"[loss_fwd] kitchen bf16 B={B}, the library's plan (small-batch launches {n_small}): scalar {err:.3e} rows {err_rows:.3e}")
    assert n_small == (1 if B == 1 else 0)
    assert err <= BAR["bf16"] and err_rows <= BAR["bf16"]


# ------------------------------------------------------------------------------------------------ 6. buffer independence
@gpu
@pytest.mark.parametrize("cfg_name,precision,B", [("tiny", "fp32", 4), ("kitchen", "bf16", 5)])
def test_results_do_not_depend_on_what_the_buffers_held(cfg_name, precision, B):
    """Workspace, loss_out and per_sample_out pre-filled with 0x00 / 0xFF / 0x7B, the inputs between bands of the same fill:
    equal bits, the bands untouched, no element of a result left as the fill."""
    from test_buffer_independence import FILLS, Guarded, _carries_fill
    m = _module(cfg_name, precision)
    inner = m.inner_model
    rt, packed = inner.runtime(m.sigma_data), inner.packed_weights()
    lib = rt.lib
    s, a, g, n, sg = (to_dev(v) for v in _inputs(cfg_name, B))
    t = s.shape[1]
    wsb = lib.beso_loss_fwd_workspace_bytes(C.byref(rt.cfg), B, t, packed.precision)
    assert wsb > lib.beso_workspace_bytes(C.byref(rt.cfg), B, t, packed.precision, 0) + 2 * a.numel() * 4
    got = {}
    for name, byte in FILLS.items():
        for with_rows in (True, False):
            ws, out, rows = Guarded(wsb, byte), Guarded(4, byte), Guarded(4 * B, byte)
            ins = [Guarded(x.numel() * 4, byte, x) for x in (s, a, g, n, sg)]
            st = lib.beso_loss_fwd(C.byref(rt.cfg), packed.buf.data_ptr(), packed.precision, ins[0].ptr, ins[1].ptr, ins[2].ptr,
                                   ins[3].ptr, ins[4].ptr, out.ptr, rows.ptr if with_rows else None, B, t, 0, ws.ptr, wsb,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert st == 0, (name, st)
            ok = torch.stack([x.guards_ok() for x in [ws, out, rows] + ins]).all()
            assert bool(ok), f"{name}: a guard band was written"
            for x, src in zip(ins, (s, a, g, n, sg)):
                assert torch.equal(bits(x.f32()), bits(src.reshape(-1))), f"{name}: an input was modified"
            assert not bool(_carries_fill(out.f32(), byte)), name
            if with_rows:
                assert not bool(_carries_fill(rows.f32(), byte)), name
                got[name] = (out.f32().clone(), rows.f32().clone())
            else:
                assert bool((rows.big == byte).all()), f"{name}: per_sample_out = NULL, yet the buffer was written"
                assert torch.equal(bits(out.f32()), bits(got[name][0])), f"{name}: the scalar differs without per_sample_out"
    assert torch.isfinite(got["ZERO"][0]).all() and torch.isfinite(got["ZERO"][1]).all()
    for name in ("NAN", "HUGE"):
        assert torch.equal(bits(got[name][0]), bits(got["ZERO"][0])), name
        assert torch.equal(bits(got[name][1]), bits(got["ZERO"][1])), name
    # loss_out = NULL: the per-sample values alone, the same bits
    ws, rows = Guarded(wsb, 0xFF), Guarded(4 * B, 0xFF)
    st = lib.beso_loss_fwd(C.byref(rt.cfg), packed.buf.data_ptr(), packed.precision, s.data_ptr(), a.data_ptr(), g.data_ptr(),
                           n.data_ptr(), sg.data_ptr(), None, rows.ptr, B, t, 0, ws.ptr, wsb,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0 and bool(ws.guards_ok() & rows.guards_ok())
    assert torch.equal(bits(rows.f32()), bits(got["ZERO"][1]))


# ------------------------------------------------------------------------------------------------ 7. argument checking (no GPU)
def test_argument_errors_do_not_touch_the_device(lib):
    """Every rejection happens before anything is enqueued (the pointers below are not memory): the documented status, and
    _lib.check turns it into the exception of that status -- ValueError for bad arguments / shapes, BesoHipError (the library's
    exception for BESO_ERR_WORKSPACE, as for every other entry point) for a short workspace."""
    from beso_amd.runtime import ScoreNetShape
    cfg = ScoreNetShape(7, 3, 48, 2, 6, 2, 3, True, 0.5).c_struct()
    one = C.c_void_p(0x1000)
    need = lib.beso_loss_fwd_workspace_bytes(C.byref(cfg), 2, 3, _lib.PREC_FP32)
    assert need > lib.beso_workspace_bytes(C.byref(cfg), 2, 3, _lib.PREC_FP32, 0) > 0
    assert lib.beso_loss_fwd_workspace_bytes(C.byref(cfg), 2, 4, _lib.PREC_FP32) == 0
    assert lib.beso_loss_fwd_workspace_bytes(C.byref(cfg), 0, 3, _lib.PREC_FP32) == 0
    assert lib.beso_loss_fwd_workspace_bytes(C.byref(cfg), 2, 3, 7) == 0
    call = lambda **k: lib.beso_loss_fwd(*[k.get(n, d) for n, d in (          # noqa: E731
        ("cfg", C.byref(cfg)), ("packed", one), ("precision", _lib.PREC_FP32), ("state", one), ("action", one), ("goal", one),
        ("noise", one), ("sigma", one), ("loss_out", one), ("per_sample_out", one), ("batch", 2), ("t", 3), ("flags", 0),
        ("workspace", one), ("workspace_bytes", need), ("stream", None))])
    cases = [(dict(loss_out=None, per_sample_out=None), -3), (dict(t=4), -2), (dict(t=0), -2), (dict(batch=0), -2),
             (dict(workspace_bytes=need - 1), -4), (dict(workspace_bytes=16), -4), (dict(flags=8), -3),
             (dict(flags=_lib.SAMPLE_STEPWISE), -3), (dict(flags=0x4000), -3), (dict(precision=7), -3), (dict(packed=None), -3),
             (dict(state=None), -3), (dict(action=None), -3), (dict(goal=None), -3), (dict(noise=None), -3),
             (dict(sigma=None), -3), (dict(workspace=None), -3), (dict(cfg=None), -3)]
    for bad, status in cases:
        st = call(**bad)
        assert st == status, (bad, st)
        with pytest.raises(_lib.BesoHipError if status == -4 else ValueError):
            _lib.check(st, "loss_fwd")
    # bf16x3 / fp16 on a shape without the one-launch kernel: unsupported, before anything is enqueued
    for prec in (_lib.PREC_BF16X3, _lib.PREC_FP16):
        nb = lib.beso_loss_fwd_workspace_bytes(C.byref(cfg), 2, 3, prec)
        st = call(precision=prec, workspace_bytes=max(nb, need))
        assert st == -5, (prec, st)
        with pytest.raises(ValueError):
            _lib.check(st, "loss_fwd")
    assert _lib.FLAG_LAST_ACTION_ONLY & (0x3f0 | _lib.SAMPLE_STEPWISE | _lib.FLAG_UNCOND) == 0


# ------------------------------------------------------------------------------------------------ 8. BesoAgent
def _agent(cfg, precision="fp32", last_only=False):
    """The TINY agent of tests/test_rollout.py; the EMA shadow is moved away from the raw weights so that the two differ."""
    from test_rollout import _agent as rollout_agent
    agent = rollout_agent(cfg, precision)
    gen = torch.Generator(DEV).manual_seed(11)
    with torch.no_grad():
        for sh in agent.ema_helper.shadow_params:
            sh.add_(0.02 * torch.randn(sh.shape, device=DEV, generator=gen))
    agent.ema_helper.version += 1
    agent.pred_last_action_only = last_only
    return agent


def _batch(cfg, B, seed=2):
    gen = torch.Generator("cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)       # noqa: E731
    return {"observation": r(B, cfg.obs_seq_len, cfg.obs_dim) * 2 + 0.5, "goal_observation": r(B, cfg.goal_seq_len, cfg.obs_dim),
            "action": r(B, cfg.obs_seq_len, cfg.act_dim) * 1.5 - 0.25}


def _training_state(agent):
    inner = agent._hip_denoiser().inner_model
    return (agent.steps, [p.detach().clone() for p in agent.model.parameters()], [p._version for p in agent.model.parameters()],
            [s.detach().clone() for s in agent.ema_helper.shadow_params], agent.ema_helper.version,
            None if inner._packed is None else inner._packed.key, agent._ema_packed_key,
            [g["lr"] for g in agent.optimizer.param_groups], agent.lr_scheduler.last_epoch)


def _same_state(a, b):
    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4] and a[5] == b[5] and a[6] == b[6] and a[7] == b[7] and a[8] == b[8]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


@gpu
@pytest.mark.parametrize("last_only", [False, True])
def test_agent_validation_loss_is_the_ema_loss_of_the_scaled_batch(last_only):
    cfg = O.TINY
    agent = _agent(cfg, last_only=last_only)
    B = 4
    batch = _batch(cfg, B)
    gen = torch.Generator(DEV).manual_seed(5)
    sigma = torch.rand(B, device=DEV, generator=gen) * 0.9 + 0.05
    noise = torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=DEV, generator=gen)
    # fill the packed caches once (the EMA image and the image of the raw weights), so that their keys are the ones the calls
    # below must leave alone
    agent.validation_loss(batch, sigma=sigma, noise=noise)
    agent._hip_denoiser().inner_model.packed_weights()
    before = _training_state(agent)
    noise_before = noise.clone()
    got = agent.validation_loss(batch, sigma=sigma, noise=noise)
    _same_state(before, _training_state(agent))
    assert torch.equal(noise, noise_before)
    assert isinstance(got, float)
    # the same value from GCDenoiser.loss on a module that CARRIES the EMA weights, on the scaled batch
    state, action, goal = agent.process_batch(batch, predict=False)
    names = [k for k, _ in agent.model.named_parameters()]
    ema = make_denoiser(cfg, {k: v.detach().cpu().numpy() for k, v in zip(names, agent.ema_helper.shadow_params)}, "fp32")
    raw = make_denoiser(cfg, {k: v.detach().cpu().numpy() for k, v in agent.model.named_parameters()}, "fp32")
    with torch.no_grad():
        want = ema.loss(state, action, goal, noise.clone(), sigma, pred_last_action_only=last_only).item()
        other = raw.loss(state, action, goal, noise.clone(), sigma, pred_last_action_only=last_only).item()
    assert got == want, (got, want)
    assert abs(other - want) > 1e-4 * abs(want)            # (the EMA weights, not the raw ones)
    agent.use_ema = False
    assert agent.validation_loss(batch, sigma=sigma, noise=noise) == other
    agent.use_ema = True
    # default draws: reproducible from a generator, positive and finite; the global generator is left where it was
    torch.manual_seed(123)
    probe = torch.rand(3)
    torch.manual_seed(123)
    a1 = agent.validation_loss(batch, generator=torch.Generator(DEV).manual_seed(9))
    assert torch.equal(torch.rand(3), probe)
    a2 = agent.validation_loss(batch, generator=torch.Generator(DEV).manual_seed(9))
    a3 = agent.validation_loss(batch)
    assert a1 == a2 and np.isfinite([a1, a3]).all() and a1 > 0 and a3 > 0
    _same_state(before, _training_state(agent))


@gpu
def test_agent_loss_by_sigma_is_one_call_over_all_levels(monkeypatch):
    from beso_amd.runtime import plan
    cfg = O.TINY
    agent = _agent(cfg)
    B, sigmas = 4, [0.05, 0.3, 0.9]
    batch = _batch(cfg, B, seed=4)
    noise = torch.randn(B, cfg.obs_seq_len, cfg.act_dim, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    den = agent._hip_denoiser()
    lib = den.inner_model.runtime(den.sigma_data).lib
    with agent._ema_scope():                     # fill the packed caches (the EMA image, the raw weights' image): see above
        pass
    den.inner_model.packed_weights()
    calls, real = [], lib.beso_loss_fwd
    monkeypatch.setattr(lib, "beso_loss_fwd", lambda *a: (calls.append(a[10]), real(*a))[1])
    before = _training_state(agent)
    with plan(forward=_lib.PLAN_PER_OP):
        curve, table = agent.loss_by_sigma(batch, sigmas, noise=noise)
        assert len(calls) == 1 and calls[0] == len(sigmas) * B, calls
        assert curve.shape == (3,) and table.shape == (3, B) and curve.grad_fn is None
        assert torch.allclose(curve, table.mean(1), rtol=1e-6, atol=0)
        state, action, goal = agent.process_batch(batch, predict=False)
        with agent._ema_scope(), torch.no_grad():
            agent.model.eval()
            for k, sg in enumerate(sigmas):
                rows = den.loss_per_sample(state, action, goal, noise.clone(), torch.full((B,), sg, device=DEV))
                assert torch.equal(bits(rows), bits(table[k])), k
        # a draw per level: [K, B, t, act]
        nk = torch.randn(3, B, cfg.obs_seq_len, cfg.act_dim, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
        _, table_k = agent.loss_by_sigma(batch, sigmas, noise=nk)
        with agent._ema_scope(), torch.no_grad():
            rows = den.loss_per_sample(state, action, goal, nk[2].clone(), torch.full((B,), sigmas[2], device=DEV))
        assert torch.equal(bits(rows), bits(table_k[2]))
    assert table[0].mean() != table[2].mean()
    _same_state(before, _training_state(agent))


# ------------------------------------------------------------------------------------------------ 9. CPU
def _cpu_module(train):
    from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT
    from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser
    inner = DiffusionGPT(state_dim=7, device="cpu", goal_conditioned=True, action_dim=3, embed_dim=48, embed_pdrob=0, attn_pdrop=0,
                         resid_pdrop=0, n_layers=2, n_heads=6, goal_seq_len=2, obs_seq_len=3, linear_output=True)
    m = GCDenoiser(inner, sigma_data=0.5)
    return m.train() if train else m.eval()


def test_no_grad_loss_in_training_mode_raises_with_the_eval_hint():
    m = _cpu_module(train=True)
    s, a, g, n, sg = torch.zeros(2, 3, 7), torch.zeros(2, 3, 3), torch.zeros(2, 2, 7), torch.zeros(2, 3, 3), torch.ones(2)
    with torch.no_grad(), pytest.raises(ValueError, match=r"eval\(\)"):
        m.loss(s, a, g, n, sg)
    with torch.no_grad(), pytest.raises(ValueError, match=r"eval\(\)"):
        m.loss_per_sample(s, a, g, n, sg)


def test_no_grad_loss_has_no_cpu_path():
    m = _cpu_module(train=False)
    s, a, g, n, sg = torch.zeros(2, 3, 7), torch.zeros(2, 3, 3), torch.zeros(2, 2, 7), torch.zeros(2, 3, 3), torch.ones(2)
    with torch.no_grad(), pytest.raises(ValueError, match="no CPU path"):
        m.loss(s, a, g, n, sg)
    with pytest.raises(ValueError, match="no CPU path"):
        m.loss_per_sample(s, a, g, n, sg)
    with pytest.raises(ValueError, match="no CPU path"):          # under autograd: the existing error of the training step
        m.train().loss(s, a, g, n, sg)
