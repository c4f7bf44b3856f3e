"""Classifier-guided sampling: ``ClassifierGuidedSampleModel`` (k_diffusion/classifier_free_sampler.py), ``MLPGuide``
(k_diffusion/guides.py) and the one-launch guide gradient ``beso_guide_apply`` (include/beso_guide.h, csrc/guide.hip).

Arbiter of the launch: a torch re-statement of ``pred + lam * sigma^2 * d/da sum(MLP(cat))`` in fp64 over copies of the guide's
parameters.  Bars (those of tests/test_resmlp.py): values 2e-5 of max |reference| (``FP32_BAR``); what depends on the gradient --
the output, and its increment over ``pred`` -- may err at most 4x what the same re-statement in fp32 torch errs against the fp64
values, torch's error taken as at least one fp32 rounding (``compare_grads``'s rule, on ``grad_errors``).  Every case prints what
it measured."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from beso_amd import _lib
from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks
from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
from beso_amd.networks.mlps.mlps import MLPNetwork
from beso_amd.networks.scaler.scaler_class import Scaler
from oracle import beso_oracle as O
from support import TRAIN_BOUNDS, bits, build_agent, check_side_library, grad_errors, lib, make_denoiser  # noqa: F401

DEV = "cuda:0"
ACTS = {"ReLU": nn.ReLU, "Mish": nn.Mish, "sigmoid": nn.Sigmoid}
FP32_BAR = 2e-5
EPS = 2.0 ** -24        # one fp32 rounding
LAM = 1.5
FILLS = {"ZERO": 0x00, "NAN": 0xFF, "HUGE": 0x7B}          # tests/test_buffer_independence.py


def guided_cls():
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierGuidedSampleModel
    return ClassifierGuidedSampleModel


class Stub(nn.Module):
    """A denoiser that returns a fixed tensor and owns two parameters."""

    def __init__(self, pred):
        super().__init__()
        self.lin = nn.Linear(2, 2)
        self.pred, self.calls = pred, []

    def forward(self, state, action, goal, sigma, **kw):
        self.calls.append(kw)
        return self.pred

    def get_params(self):
        return self.parameters()


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_the_class_imports_and_has_the_references_surface():
    G = guided_cls()
    pred = torch.zeros(2, 1, 3)
    guide = lambda s, a, g: a.sum(-1)                                                    # noqa: E731
    m = G(Stub(pred), guide)
    assert m.cond_lambda == 2 and m.guide is guide and isinstance(m.model, Stub)
    m = G(model=Stub(pred), cond_func=guide, cond_lambda=0.5)
    assert m.cond_lambda == 0.5
    assert "84" in G.__doc__ and "85" in G.__doc__                     # the deviation is stated with the reference's lines


def test_library_exports_what_its_header_declares(lib):
    """libbeso_guide.so: the two symbols of include/beso_guide.h, no more; the binding table has the header's argument counts;
    the matrix-pipe hazard check of DESIGN.md 4.1c passes on it."""
    check_side_library("beso_guide.h", "beso_guide_", _lib.GUIDE_SIGNATURES, _lib.GUIDE_LIB_PATH, _lib.load_guide, 2, min_kernels=1,
                       min_mfma=12)
    assert sorted(_lib.GUIDE_SIGNATURES) == sorted(_lib.GUIDE_EXPORTS)


def test_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers: a call that got past its checks would read and write through them."""
    g = _lib.load_guide()
    D = _lib.MlpDims
    one = C.c_void_p(16)
    arr = lambda n: (C.c_void_p * n)(*([16] * n))                                       # noqa: E731
    good = D(13, 48, 2, 1, 1)                                                           # obs 5, act 3, goal: 5 + 3 + 5

    def call(d=good, n=None, goal=one, B=4, T=3, steps=3, G=2, rows=4, obs=5, act=3, state=one, out=one):
        n = 2 * (d.n_hidden + 1) if n is None else n
        return g.beso_guide_apply(arr(max(n, 1)), n, C.byref(d), state, goal, one, one, B, T, steps, G, rows, obs, act, 1.5, out, None)

    sup = lambda d, obs=5, act=3, goal=1: g.beso_guide_supported(C.byref(d), obs, act, goal)       # noqa: E731
    assert sup(good) == _lib.OK and sup(D(8, 48, 2, 1, 1), goal=0) == _lib.OK
    for bad in (D(13, 40, 2, 1, 1), D(13, 0, 2, 1, 1), D(13, 528, 2, 1, 1), D(13, 48, 0, 1, 1), D(13, 48, 5, 1, 1),
                D(13, 48, 2, 2, 1), D(13, 48, 2, 0, 1), D(12, 48, 2, 1, 1), D(8, 48, 2, 1, 1),
                D(13, 512, 3, 1, 1), D(13, 432, 4, 1, 1)):                              # the last two: beyond the LDS rule
        assert call(bad) == _lib.ERR_BAD_SHAPE and sup(bad) == _lib.ERR_BAD_SHAPE, tuple(getattr(bad, f) for f, _ in D._fields_)
    assert sup(D(13, 512, 2, 1, 1)) == _lib.OK and sup(D(13, 416, 4, 1, 1)) == _lib.OK   # the widest the rule admits
    assert sup(D(516, 48, 2, 1, 1), obs=256, act=4) == _lib.ERR_BAD_SHAPE                # in_dim > 512
    assert call(goal=None) == _lib.ERR_BAD_SHAPE                                         # 13 != 5 + 3 without a goal
    assert call(obs=0) == _lib.ERR_BAD_SHAPE and call(act=0) == _lib.ERR_BAD_SHAPE
    assert call(B=0) == _lib.ERR_BAD_SHAPE and call(T=0) == _lib.ERR_BAD_SHAPE and call(B=-3) == _lib.ERR_BAD_SHAPE   # bad M
    assert call(B=1 << 20, T=1 << 12, steps=1 << 12, rows=1) == _lib.ERR_BAD_SHAPE       # M = 2^32
    assert call(steps=2) == _lib.ERR_BAD_SHAPE                                           # state shorter than the window
    assert call(G=0) == _lib.ERR_BAD_SHAPE and call(rows=3) == _lib.ERR_BAD_SHAPE
    assert call(D(13, 48, 2, 1, 3)) == _lib.ERR_BAD_ARG and sup(D(13, 48, 2, 1, -1)) == _lib.ERR_BAD_ARG   # unknown activation
    assert call(n=4) == _lib.ERR_BAD_ARG and call(n=8) == _lib.ERR_BAD_ARG
    assert call(state=None) == _lib.ERR_BAD_ARG and call(out=None) == _lib.ERR_BAD_ARG
    assert call(out=C.c_void_p(18)) == _lib.ERR_BAD_ARG                                  # not 4-byte aligned
    assert g.beso_guide_apply(None, 6, C.byref(good), one, one, one, one, 4, 3, 3, 2, 4, 5, 3, 1.5, one, None) == _lib.ERR_BAD_ARG
    assert g.beso_guide_supported(None, 5, 3, 1) == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="beso_guide_apply"):
        _lib.check(call(steps=2), "beso_guide_apply")


def test_generic_path_on_cpu_is_the_formula():
    """q = -0.5 |a - c|^2: d q / d a = c - a in closed form."""
    G = guided_cls()
    gen = torch.Generator().manual_seed(0)
    B, T, A = 5, 3, 4
    c, pred, action = (torch.randn(B, T, A, generator=gen) for _ in range(3))
    state, goal = torch.randn(B, T, 6, generator=gen), torch.randn(B, 2, 6, generator=gen)
    sigma = torch.rand(B, generator=gen) + 0.2                                          # distinct per sample
    seen = []

    def guide(s, a, g):
        seen.append((s, g, a.requires_grad))
        return -0.5 * (a - c).pow(2).sum(-1)

    stub = Stub(pred)
    m = G(stub, guide, cond_lambda=LAM)
    want = lambda lam: pred + lam * (c - pred) * sigma.view(B, 1, 1) ** 2               # noqa: E731
    with torch.no_grad():                                                               # the samplers call under no_grad
        out = m(state, action, goal, sigma)
        assert torch.allclose(out, want(LAM), rtol=0, atol=1e-6) and not out.requires_grad
        assert torch.allclose(m(state, action, goal, sigma, cond_lambda=0.25), want(0.25), rtol=0, atol=1e-6)   # per call
        assert torch.equal(m(state, action, goal, sigma, cond_lambda=0), pred)
        assert torch.equal(G(stub, guide, cond_lambda=0)(state, action, goal, sigma), pred)
        m(state, action, goal, sigma, uncond=True)                                      # extra args reach the model
    assert stub.calls[-1] == {"uncond": True} and stub.calls[0] == {}
    assert seen[0][0] is state and seen[0][1] is goal and seen[0][2]
    assert [id(p) for p in m.get_params()] == [id(p) for p in stub.get_params()]


def _cpu_guide(obs, act, goal=True, out=1, hidden=16):
    return MLPNetwork(obs + act + (obs if goal else 0), hidden, 1, out, device="cpu")


def test_a_module_guide_stays_out_of_parameters_and_checkpoints():
    G = guided_cls()
    cfg = O.TINY
    den = make_denoiser(cfg, device="cpu")
    keys, params = list(den.state_dict()), [id(p) for p in den.get_params()]
    guide = MLPGuide(_cpu_guide(cfg.obs_dim, cfg.act_dim))
    for model in (den, ClassifierFreeSampleModel(den, 1.5)):
        m = G(model, guide, cond_lambda=LAM)
        prefix = "model." if model is den else "model.model."
        assert list(den.state_dict()) == keys and list(m.state_dict()) == [prefix + k for k in keys]
        assert [id(p) for p in m.get_params()] == params == [id(p) for p in m.parameters()] == [id(p) for p in den.get_params()]
        assert [n for n, _ in m.named_parameters()] == [prefix + n for n, _ in den.named_parameters()]
        assert m.guide is guide and not any(mod is guide for mod in m.modules())
    assert len(list(guide.parameters())) == 4                                           # the guide's own: its checkpoint, not the agent's
    agent = build_agent(cfg, lambda: G(make_denoiser(cfg, device="cpu"), guide, LAM))
    assert agent._hip_denoiser() is agent.model.model
    assert sum(p.numel() for g in agent.optimizer.param_groups for p in g["params"]) == sum(p.numel() for p in den.parameters())
    assert len(list(agent.ema_helper.shadow_params)) == len(params)
    agent = build_agent(cfg, lambda: G(ClassifierFreeSampleModel(make_denoiser(cfg, device="cpu"), 1.5), guide, LAM))
    assert agent._hip_denoiser() is agent.model.model.model


def test_mlp_guide_refusals_are_by_name():
    with pytest.raises(ValueError, match="output_dim"):
        MLPGuide(_cpu_guide(5, 3, out=2))
    with pytest.raises(TypeError, match="MLPNetwork"):
        MLPGuide(lambda: nn.Linear(3, 1))
    state, a, goal = torch.zeros(4, 3, 5), torch.zeros(4, 3, 3), torch.zeros(4, 2, 5)
    g = MLPGuide(lambda: _cpu_guide(5, 3))                                              # a factory
    assert g.use_goal and g.network.input_dim == 13
    with pytest.raises(ValueError, match="input_dim"):
        g(state, a, None)                                                               # 13 != 5 + 3
    with pytest.raises(ValueError, match="input_dim"):
        MLPGuide(_cpu_guide(5, 3), use_goal=False)(state, a, goal)
    with pytest.raises(ValueError, match="input_dim"):
        g(state, torch.zeros(4, 3, 4), goal)
    with pytest.raises(ValueError, match="fewer than"):
        g(state[:, :2], a, goal)
    with pytest.raises(ValueError, match="goal"):
        g(state, a, torch.zeros(3, 2, 5))
    with pytest.raises(RuntimeError, match="GPU"):                                      # the network has no CPU evaluation
        g(state, a, goal)
    cfgd = MLPGuide({"_target_": "beso_amd.networks.mlps.mlps.MLPNetwork", "input_dim": 8, "hidden_dim": 16, "device": "cpu"}, False)
    assert cfgd.network.output_dim == 1 and not cfgd.use_goal


# -------------------------------------------------------------------------------------------------
# GPU: the launch
# -------------------------------------------------------------------------------------------------
# (obs, act, goal: None / "own" [B, 2, obs] / "shared" [1, 2, obs], hidden, num_hidden_layers, activation, B, T, extra state steps)
# M = B T: 1, a full tile, one row above it, a partial third tile.  (5, 3) with a goal: input_dim 13, no multiple of 4 -- the
# scalar weight loads; (60, 9) without: 69; (30, 9) with: 69.  hidden 512 x 2 layers and 416 x 4 layers: the most LDS the rule
# admits (132096 and 161280 bytes).
SWEEP = [(5, 3, "own", 16, 1, "ReLU", 1, 1, 0), (5, 3, "shared", 48, 4, "Mish", 4, 4, 0), (5, 3, "own", 48, 1, "sigmoid", 17, 1, 0),
         (60, 9, None, 48, 4, "ReLU", 11, 3, 2), (60, 9, None, 16, 4, "sigmoid", 4, 4, 0), (30, 9, "shared", 512, 1, "Mish", 11, 3, 0),
         (30, 9, "own", 512, 2, "ReLU", 17, 1, 0), (30, 9, "own", 16, 1, "Mish", 11, 3, 1), (5, 3, "own", 416, 4, "sigmoid", 11, 3, 0)]
OUTSIDE = (30, 9, "own", 512, 3, "Mish", 17, 1, 0)          # five 16 x 516 tiles: 165120 bytes > 160 KiB -> the generic path
case_id = lambda s: "x".join(map(str, s))                                                # noqa: E731


def make_guide(case, seed=0):
    obs, act, goal, hidden, layers, activation = case[:6]
    torch.manual_seed(seed)
    net = MLPNetwork(obs + act + (obs if goal else 0), hidden, layers, 1, activation=activation, device=DEV)
    if activation == "sigmoid":                # sigmoid' <= 1 / 4: at nn.Linear's init scale four layers leave a gradient of 1e-4
        with torch.no_grad():
            for lin in net.layers:
                lin.weight.mul_(4.0)
    return MLPGuide(net, use_goal=goal is not None)


def make_inputs(case, seed=1, extra_b=0):
    obs, act, goal = case[:3]
    B, T, more = case[6] + extra_b, case[7], case[8]
    g = torch.Generator().manual_seed(seed)
    state, pred = torch.randn(B, T + more, obs, generator=g), torch.randn(B, T, act, generator=g)
    goals = torch.randn(B, 2, obs, generator=g)
    sigma = 0.3 + 1.2 * torch.rand(B, generator=g)                                      # distinct per sample
    return state, pred, (None if goal is None else goals[:1] if goal == "shared" else goals), sigma


def restated(guide, state, pred, goal, sigma, lam, dtype, device="cpu"):
    """-> (q [B, T], pred + lam * sigma^2 * d sum(q) / da) in torch ops over copies of the guide's parameters."""
    layers = copy.deepcopy(guide.network.layers).to(device, dtype)
    act = ACTS[guide.network.activation]()
    B, T, _ = pred.shape
    state, pred, sigma = state.to(device, dtype), pred.to(device, dtype), sigma.to(device, dtype)
    with torch.enable_grad():
        a = pred.clone().requires_grad_(True)
        parts = [state[:, :T], a]
        if goal is not None:
            parts.append(goal.to(device, dtype)[:, -1:, :].expand(B, T, -1))
        x = torch.cat(parts, dim=-1)
        for i, lin in enumerate(layers):
            x = lin(x)
            if i < len(layers) - 1:
                x = act(x)
        q = x.squeeze(-1)
        grad = torch.autograd.grad(q.sum(), a)[0]
    return q.detach(), (pred + lam * grad * sigma.view(B, 1, 1) ** 2).detach()


def check_bars(tag, got, pred, t32, ref, increment=True):
    """`got` (HIP, fp32) against `ref`, `t32` the fp32 torch re-statement: the module docstring's bars.  increment=False (a
    `ref` that is itself an fp32 result, rounded to the output's ulp): the output alone, not its difference from `pred`, whose
    relative error is that rounding divided by the increment's size."""
    got, t32, p64 = got.cpu().double(), t32.cpu().double(), pred.cpu().double()
    val = ((got - ref).abs().max() / ref.abs().max()).item()
    floor = TRAIN_BOUNDS["fp32"][2]
    n = 2 if increment else 1
    e_hip = grad_errors([got, got - p64][:n], [ref, ref - p64][:n], floor)
    e_t32 = grad_errors([t32, t32 - p64][:n], [ref, ref - p64][:n], floor)
    ratios = [h / max(t, EPS) for h, t in zip(e_hip, e_t32)]
    print(f"{tag}: max err / max |ref| {val:.3e}; output err {e_hip[0]:.3e} (torch fp32 {e_t32[0]:.3e}), increment err "
          f"{e_hip[-1]:.3e} (torch fp32 {e_t32[-1]:.3e}), max ratio {max(ratios):.2f}")
    assert (ref - p64).abs().max() > 1e-3 * ref.abs().max(), "the guide moves nothing: the case checks nothing"
    assert val <= FP32_BAR
    for h, t in zip(e_hip, e_t32):
        assert h <= 4.0 * max(t, EPS), (tag, h, t)


def run_case(case, expect_fused):
    G = guided_cls()
    guide = make_guide(case)
    state, pred, goal, sigma = make_inputs(case)
    q64, ref = restated(guide, state, pred, goal, sigma, LAM, torch.float64)
    _, t32 = restated(guide, state, pred, goal, sigma, LAM, torch.float32)
    d = lambda t: None if t is None else t.to(DEV)                                      # noqa: E731
    sd, pd, gd, sgd = d(state), d(pred), d(goal), d(sigma)
    calls = []
    real = guide.apply
    guide.apply = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    fused = G(Stub(pd), guide, cond_lambda=LAM)
    generic = G(Stub(pd), lambda s, a, g: guide(s, a, g), cond_lambda=LAM)               # any callable: autograd over the guide
    with torch.no_grad():
        q = guide(sd, pd, gd)
        out = fused(sd, pd, gd, sgd)
        n_fused = len(calls)
        out_generic = generic(sd, pd, gd, sgd)
    assert n_fused == (1 if expect_fused else 0) and len(calls) == n_fused
    assert guide.fused_supported(case[0], case[1], goal is not None) == expect_fused
    qerr = ((q.cpu().double() - q64).abs().max() / q64.abs().max()).item()
    print(f"guide {case}: q max err / max |ref| = {qerr:.3e}")
    assert q.shape == pred.shape[:2] and qerr <= FP32_BAR
    assert out.shape == pred.shape and out.dtype == torch.float32 and not out.requires_grad
    check_bars(f"guide {case} {'fused' if expect_fused else 'outside the rule -> generic'}", out, pred, t32, ref)
    check_bars(f"guide {case} generic", out_generic, pred, t32, ref)
    check_bars(f"guide {case} fused against generic", out, pred, t32, out_generic.cpu().double(), increment=False)
    return guide, (sd, pd, gd, sgd)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_fused_launch_against_the_fp64_restatement_and_the_generic_path(case):
    run_case(case, expect_fused=True)


@pytest.mark.gpu
def test_a_guide_outside_the_lds_rule_takes_the_generic_path():
    guide, (sd, pd, gd, sgd) = run_case(OUTSIDE, expect_fused=False)
    with pytest.raises(ValueError, match="status -2"):                                  # the entry point refuses; nothing is enqueued
        guide.apply(sd, pd, gd, sgd, LAM)


BIT_CASES = [(5, 3, "own", 48, 4, "Mish", 11, 3, 0), (30, 9, "shared", 512, 2, "ReLU", 17, 1, 0), (60, 9, None, 16, 1, "sigmoid", 17, 1, 1)]


def banded_out(shape, fill):
    band = 256
    n = 4 * int(np.prod(shape))
    buf = torch.full((n + 2 * band,), fill, dtype=torch.uint8, device=DEV)
    buf[:band] = 0x5C
    buf[-band:] = 0x5C
    return buf, buf[band:band + n].view(torch.float32).view(*shape)


def guards_intact(buf):
    return bool((buf[:256] == 0x5C).all()) and bool((buf[-256:] == 0x5C).all())


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_equal_bits_rows_independent_alias_fills_and_guard_bands(case):
    guide = make_guide(case)
    B = case[6]
    state, pred, goal, sigma = (None if t is None else t.to(DEV) for t in make_inputs(case, extra_b=5))
    head = lambda t, n=B: None if t is None else (t if t.shape[0] == 1 else t[:n].contiguous())   # noqa: E731
    s, p, g, sg = head(state), head(pred), head(goal), head(sigma)
    base = guide.apply(s, p, g, sg, LAM)
    assert bool(torch.isfinite(base).all()) and torch.equal(bits(guide.apply(s, p, g, sg, LAM)), bits(base))       # run to run
    # rows: B + 5 samples give the first B the same bits; so does changing every other sample's inputs
    assert torch.equal(bits(guide.apply(state, pred, goal, sigma, LAM)[:B]), bits(base))
    k = B // 2
    s2, p2, sg2 = torch.randn_like(s), torch.randn_like(p), torch.rand_like(sg) + 0.1
    s2[k], p2[k], sg2[k] = s[k], p[k], sg[k]
    g2 = g
    if g is not None and g.shape[0] > 1:
        g2 = torch.randn_like(g)
        g2[k] = g[k]
    other = guide.apply(s2, p2, g2, sg2, LAM)
    assert torch.equal(bits(other[k]), bits(base[k])) and not torch.equal(other[k - 1], base[k - 1])
    # only step G - 1 of the goal is read
    if g is not None:
        g3 = g.clone()
        g3[:, :-1] = 7.0
        assert torch.equal(bits(guide.apply(s, p, g3, sg, LAM)), bits(base))
    # out aliasing pred
    alias = p.clone()
    assert guide.apply(s, alias, g, sg, LAM, out=alias) is alias and torch.equal(bits(alias), bits(base))
    # what out held; nothing outside its extent
    for name, fill in FILLS.items():
        buf, out = banded_out(p.shape, fill)
        guide.apply(s, p, g, sg, LAM, out=out)
        assert torch.equal(bits(out), bits(base)), name
        assert guards_intact(buf), name
    buf, both = banded_out(p.shape, 0xFF)                                               # aliased AND banded
    both.copy_(p)
    guide.apply(s, both, g, sg, LAM, out=both)
    assert torch.equal(bits(both), bits(base)) and guards_intact(buf)


# -------------------------------------------------------------------------------------------------
# GPU: through a sampler
# -------------------------------------------------------------------------------------------------
def tiny_setup(lam_cfg=None, seed=3):
    cfg = O.TINY
    den = make_denoiser(cfg, O.make_weights(cfg, seed=2, std=0.05), "fp32")
    model = den if lam_cfg is None else ClassifierFreeSampleModel(den, lam_cfg)
    torch.manual_seed(seed)
    guide = MLPGuide(MLPNetwork(2 * cfg.obs_dim + cfg.act_dim, 48, 2, 1, activation="Mish", device=DEV))
    state, goal, x_t = (torch.from_numpy(v).to(DEV) for v in O.make_inputs(cfg, 4, seed=1))
    return cfg, den, model, guide, state, goal, x_t


class RestatedGuided:
    """The library's own denoiser forward, then the guide's gradient in fp32 torch ops."""

    def __init__(self, model, guide, lam):
        self.model, self.guide, self.lam = model, guide, lam

    def __call__(self, state, action, goal, sigma):
        pred = self.model(state, action, goal, sigma)
        return restated(self.guide, state, pred, goal, sigma, self.lam, torch.float32, device=DEV)[1]


def restated_sampler(name, model, state, x, goal, sig):
    """ddim (DPM-Solver-1 in t = -log sigma; the last step returns the denoised action) and euler, step by step."""
    sig = [float(v) for v in sig]
    for i in range(len(sig) - 1):
        den = model(state, x, goal, torch.full((x.shape[0],), sig[i], device=x.device))
        if name == "ddim":
            x = den if sig[i + 1] == 0 else (sig[i + 1] / sig[i]) * x - np.expm1(-(np.log(sig[i]) - np.log(sig[i + 1]))) * den
        else:
            x = x + (x - den) / sig[i] * (sig[i + 1] - sig[i])
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("lam_cfg", [None, 1.5], ids=["GCDenoiser", "ClassifierFree1.5"])
def test_guided_samplers_match_their_step_by_step_restatement(lam_cfg):
    G = guided_cls()
    cfg, den, model, guide, state, goal, x_t = tiny_setup(lam_cfg)
    guided = G(model, guide, cond_lambda=LAM)
    assert ks._fused_target(guided) == (None, None)                    # an unknown wrapper: every sampler is the Python loop
    sig = ks.get_sigmas_exponential(3, 0.005, 1.0)
    calls = []
    real = guide.apply
    guide.apply = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    for name, fn in (("ddim", ks.sample_ddim), ("euler", ks.sample_euler)):
        with torch.no_grad():
            got = fn(guided, state, x_t, goal, sig, disable=True)
            ref = restated_sampler(name, RestatedGuided(model, guide, LAM), state, x_t, goal, sig)
            plain = fn(model, state, x_t, goal, sig, disable=True, callback=lambda d: None)      # the unguided Python loop
            zero = fn(G(model, guide, cond_lambda=0), state, x_t, goal, sig, disable=True)
        err = grad_errors([got], [ref], TRAIN_BOUNDS["fp32"][2])[0]
        moved = ((got - plain).abs().max() / plain.abs().max()).item()
        print(f"guided {name} ({'cfg 1.5' if lam_cfg else 'plain'}), 3 steps, B = 4: err vs re-statement {err:.3e}; guidance moved "
              f"the sample by {moved:.3e} of max |x_0|")
        assert got.shape == x_t.shape and moved > 1e-3
        assert err <= TRAIN_BOUNDS["fp32"][1]
        assert torch.equal(zero, plain)                                # cond_lambda = 0: the bits of the unguided loop
    assert len(calls) == 2 * 2 * 3                                     # one launch per denoiser evaluation, lambda = 0 included


# -------------------------------------------------------------------------------------------------
# GPU: agent
# -------------------------------------------------------------------------------------------------
def make_agent(lam, guide=None):
    cfg = O.TINY
    w = O.make_weights(cfg, seed=2, std=0.05)
    factory = lambda: make_denoiser(cfg, w, "fp32")                                      # noqa: E731
    if lam is not None:
        G, plain = guided_cls(), factory
        factory = lambda: G(plain(), guide, cond_lambda=lam)                             # noqa: E731
    agent = build_agent(cfg, factory, device=DEV, lr=1e-3)
    agent.get_scaler(Scaler(np.random.default_rng(0).standard_normal((64, cfg.obs_dim)).astype(np.float32),
                            np.random.default_rng(1).standard_normal((64, cfg.act_dim)).astype(np.float32), True, DEV))
    agent.set_bounds(agent.scaler)
    return agent


def agent_batch(B=6, seed=7):
    cfg = O.TINY
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    return {"observation": r(B, cfg.obs_seq_len, cfg.obs_dim), "action": r(B, cfg.obs_seq_len, cfg.act_dim),
            "goal_observation": r(B, cfg.goal_seq_len, cfg.obs_dim)}


@pytest.mark.gpu
def test_guided_agent_trains_stores_and_predicts_on_the_ema_image(tmp_path, monkeypatch):
    from beso_amd.optim import FusedAdam
    cfg = O.TINY
    torch.manual_seed(3)
    guide = MLPGuide(MLPNetwork(2 * cfg.obs_dim + cfg.act_dim, 48, 2, 1, activation="Mish", device=DEV))
    agent = make_agent(LAM, guide)
    den = agent._hip_denoiser()
    assert den is agent.model.model and isinstance(agent.optimizer, FusedAdam)
    guide_before = [p.detach().clone() for p in guide.parameters()]
    init = [p.detach().clone() for p in den.parameters()]
    batch = agent_batch()
    losses = [agent.train_step(batch) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses)
    assert max((p.detach() - q).abs().max().item() for p, q in zip(den.parameters(), init)) > 1e-4      # the denoiser trained
    assert all(torch.equal(p, q) for p, q in zip(guide.parameters(), guide_before)) and all(p.grad is None for p in guide.parameters())
    agent.store_model_weights(str(tmp_path))
    want = ["model." + k for k in den.state_dict()]
    assert list(torch.load(tmp_path / "model_state_dict.pth")) == want
    assert list(torch.load(tmp_path / "non_ema_model_state_dict.pth")) == want

    # use_ema: the packed EMA image, never the store / copy_to / restore fallback
    monkeypatch.setattr(agent.ema_helper, "store", lambda *a: (_ for _ in ()).throw(AssertionError("the parameters() fallback ran")))
    obs = {"observation": batch["observation"][:, 0], "goal_observation": batch["goal_observation"][0]}
    calls = []
    real = guide.apply
    guide.apply = lambda *a, **k: (calls.append(1), real(*a, **k))[1]

    def infer():
        agent.reset()
        torch.manual_seed(5)
        return agent.predict(obs)

    p0 = infer()
    assert len(calls) == agent.num_sampling_steps and p0.shape[-1] == cfg.act_dim and bool(torch.isfinite(p0).all())
    with torch.no_grad():
        for p in den.parameters():
            p.mul_(3.0)
    assert torch.equal(bits(infer()), bits(p0))                        # the raw weights do not matter
    with torch.no_grad():
        agent.ema_helper._flat.mul_(1.5)
    agent.ema_helper.version += 1
    assert not torch.equal(infer(), p0)                                # the shadow does


@pytest.mark.gpu
def test_cond_lambda_zero_predicts_what_the_unguided_agent_predicts():
    """Same seed, same draws, bit for bit.  The unguided agent's DDIM is the one-enqueue loop, which agrees with the Python loop
    over the HIP denoiser to rounding only (tests/test_fused_solvers.py bounds the two at 1e-5): the bits are equal because
    ``BesoAgent.sample_loop`` runs a guided model whose ``cond_lambda`` is 0 as the model it wraps."""
    cfg = O.TINY
    torch.manual_seed(3)
    guide = MLPGuide(MLPNetwork(2 * cfg.obs_dim + cfg.act_dim, 48, 2, 1, activation="Mish", device=DEV))
    batch = agent_batch()
    obs = {"observation": batch["observation"][:, 0], "goal_observation": batch["goal_observation"][0]}
    preds = []
    for lam in (None, 0.0, LAM):
        agent = make_agent(lam, guide)
        torch.manual_seed(5)
        first = agent.predict(obs)
        preds.append((first, agent.predict(obs)))                      # the second call: a window of two steps
    for a, b in zip(preds[0], preds[1]):
        assert torch.equal(bits(a), bits(b))
    assert not torch.equal(preds[2][0], preds[0][0])                   # ... and the guide does steer when lambda is not 0
