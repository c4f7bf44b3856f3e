"""The noise-aware ``MLPGuide`` (``use_sigma``), ``GuideTrainer`` (k_diffusion/guide_fit.py) and the C ABI of libbeso_guidefit.so
(include/beso_guide_fit.h), as far as they go without a GPU: shapes and refusals by name, who is handed ``sigma``, the binding
table against the header, and the float32 numpy re-statement of ``beso_guide_fit_loss``'s summation order that
tests/test_guide_fit_gpu.py compares bits with."""
import ctypes as C

import numpy as np
import pytest
import torch

from beso_amd import _lib
from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierGuidedSampleModel
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
from beso_amd.networks.mlps.mlps import MLPNetwork
from support import check_side_library, lib  # noqa: F401

LANES = 256
f32 = np.float32


# -------------------------------------------------------------------------------------------------
# the re-statements the GPU tests share
# -------------------------------------------------------------------------------------------------
def lane_order_sum(v):
    """include/beso_guide_fit.h: lane j adds v[j], v[j + 256], ... in ascending order, from 0; the 256 lane sums are then added in
    lane order starting from lane 0's.  Every addition in float32."""
    v = np.asarray(v, dtype=f32)
    lanes = np.zeros(LANES, dtype=f32)
    for start in range(0, len(v), LANES):
        chunk = v[start:start + LANES]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    total = lanes[0]
    for j in range(1, LANES):
        total = f32(total + lanes[j])
    return f32(total)


def restated_mse(q, y, w=None):
    """-> (loss, per_row, dq) of BESO_GUIDE_FIT_MSE in float32 numpy, rounding by rounding as the header states them."""
    q, y = np.asarray(q, dtype=f32), np.asarray(y, dtype=f32)
    d = q - y
    per_row = d * d
    g = f32(2.0) * d
    if w is None:
        S, N = f32(len(q)), lane_order_sum(per_row)
    else:
        w = np.asarray(w, dtype=f32)
        S, N = lane_order_sum(w), lane_order_sum(w * per_row)
        g = w * g
    if S == 0:
        return f32(0.0), per_row, np.zeros_like(g)
    return f32(N / S), per_row, (g / S).astype(f32)


def restated_f64(q, y, w=None, kind="mse"):
    """-> (loss, per_row, dq) of either loss in float64, summed by numpy."""
    q, y = np.asarray(q, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if kind == "mse":
        per_row, g = (q - y) ** 2, 2.0 * (q - y)
    else:
        per_row = np.maximum(q, 0.0) - q * y + np.log1p(np.exp(-np.abs(q)))
        g = 1.0 / (1.0 + np.exp(-q)) - y
    w = np.ones_like(q) if w is None else np.asarray(w, dtype=np.float64)
    S = w.sum()
    if S == 0:
        return 0.0, per_row, np.zeros_like(g)
    return (w * per_row).sum() / S, per_row, w * g / S


def test_float32_restatement_of_the_reduction_order_agrees_with_a_float64_sum():
    rng = np.random.default_rng(0)
    q, y, w = rng.standard_normal(1000).astype(f32), rng.standard_normal(1000).astype(f32), rng.random(1000).astype(f32)
    for weight in (None, w):
        loss, per_row, dq = restated_mse(q, y, weight)
        loss64, per_row64, dq64 = restated_f64(q, y, weight)
        assert loss.dtype == f32 and per_row.dtype == f32 and dq.dtype == f32
        assert abs(float(loss) - loss64) <= 1e-6 * abs(loss64)
        assert np.abs(per_row - per_row64).max() <= 1e-6 * np.abs(per_row64).max()
        assert np.abs(dq - dq64).max() <= 1e-6 * np.abs(dq64).max()
    # 1000 rows: lanes 0 ... 231 hold four rows, the others three -- the order is not numpy's pairwise one
    assert lane_order_sum(np.ones(1000)) == 1000.0
    loss, _, dq = restated_mse(q, y, np.zeros(1000))
    assert loss == 0.0 and not dq.any()


# -------------------------------------------------------------------------------------------------
# MLPGuide(use_sigma)
# -------------------------------------------------------------------------------------------------
def _net(input_dim, hidden=16):
    return MLPNetwork(input_dim, hidden, 1, 1, device="cpu")


def test_use_sigma_adds_one_input_column_and_says_so():
    state, a, goal, sigma = torch.zeros(4, 3, 5), torch.zeros(4, 3, 3), torch.zeros(4, 2, 5), torch.ones(4)
    g = MLPGuide(_net(14), use_sigma=True)
    assert g.use_sigma and g.use_goal and not MLPGuide(_net(13)).use_sigma
    for guide, goal_arg in ((MLPGuide(_net(13), use_sigma=True), goal),                # 13 != 5 + 3 + 5 + 1
                            (g, None),                                                  # 14 != 5 + 3 + 1
                            (MLPGuide(_net(8), use_goal=False, use_sigma=True), goal)):  # 8 != 5 + 3 + 1
        with pytest.raises(ValueError, match=r"input_dim.*\+ 1.*use_sigma=True"):
            guide(state, a, goal_arg, sigma)
    with pytest.raises(ValueError, match="use_sigma=False"):
        MLPGuide(_net(14))(state, a, goal)
    with pytest.raises(RuntimeError, match="GPU"):                                      # the shapes pass; the network has no CPU evaluation
        g(state, a, goal, sigma)
    with pytest.raises(RuntimeError, match="GPU"):
        MLPGuide(_net(9), use_goal=False, use_sigma=True)(state, a, goal, sigma)


def test_forward_requires_sigma_with_use_sigma_and_refuses_it_without():
    state, a, goal = torch.zeros(4, 3, 5), torch.zeros(4, 3, 3), torch.zeros(4, 2, 5)
    g = MLPGuide(_net(14), use_sigma=True)
    with pytest.raises(ValueError, match="needs sigma"):
        g(state, a, goal)
    for bad in (torch.ones(3), torch.ones(4, 1), 0.5):
        with pytest.raises(ValueError, match=r"sigma must be a tensor \[B=4\]"):
            g(state, a, goal, bad)
    with pytest.raises(ValueError, match="without use_sigma"):
        MLPGuide(_net(13))(state, a, goal, torch.ones(4))
    c = g.c_noise(torch.tensor([1.0, np.e, 0.5, 2.0]), 4)
    assert torch.equal(c, torch.tensor([1.0, np.e, 0.5, 2.0]).log() / 4) and c[0] == 0 and MLPGuide(_net(13)).c_noise(None, 4) is None


class _Recording(MLPGuide):
    """An MLPGuide whose evaluation is a torch-op stand-in that records how it was called."""

    def forward(self, *args):
        self.seen = args
        return args[1].sum(-1)


def test_the_guided_wrapper_hands_sigma_to_a_use_sigma_guide_only():
    pred = torch.zeros(4, 3, 3)
    state, goal, sigma = torch.zeros(4, 3, 5), torch.zeros(4, 2, 5), torch.full((4,), 0.5)
    model = lambda s, a, g, sg: pred                                                    # noqa: E731
    aware, blind = _Recording(_net(14), use_sigma=True), _Recording(_net(13))
    calls = []

    def plain(*args):
        calls.append(args)
        return args[1].sum(-1)

    for guide in (aware, blind, plain):
        out = ClassifierGuidedSampleModel(model, guide, cond_lambda=2.0)(state, pred, goal, sigma)
        assert torch.equal(out, pred + 2.0 * 0.25)                                      # d sum(a) / da = 1, sigma^2 = 1 / 4
    assert len(aware.seen) == 4 and aware.seen[3] is sigma and aware.seen[0] is state and aware.seen[2] is goal
    assert len(blind.seen) == 3 and len(calls) == 1 and len(calls[0]) == 3


# -------------------------------------------------------------------------------------------------
# GuideTrainer
# -------------------------------------------------------------------------------------------------
def _trainer(**kw):
    from beso_amd.agents.diffusion_agents.k_diffusion.guide_fit import GuideTrainer
    return GuideTrainer(MLPGuide(_net(13)), **kw)


def test_trainer_refuses_by_name():
    from beso_amd.agents.diffusion_agents.k_diffusion.guide_fit import GuideTrainer
    with pytest.raises(ValueError, match="loss 'huber'"):
        _trainer(loss="huber")
    with pytest.raises(TypeError, match="MLPGuide"):
        GuideTrainer(_net(13))
    state, a, goal = torch.zeros(4, 3, 5), torch.zeros(4, 3, 3), torch.zeros(4, 2, 5)
    tr = _trainer(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0, loss="bce", seed=1)
    assert tr.loss == "bce" and tr.optimizer.param_groups[0]["betas"] == (0.9, 0.99)
    for bad in (torch.zeros(4), torch.zeros(4, 3, 1), torch.zeros(3, 4), torch.zeros(12)):
        with pytest.raises(ValueError, match=r"target must be \[B=4, T=3\]"):
            tr.train_step(state, a, goal, bad)
    with pytest.raises(ValueError, match=r"weight must be \[B=4, T=3\]"):
        tr.train_step(state, a, goal, torch.zeros(4, 3), weight=torch.zeros(4))
    with pytest.raises(ValueError, match="input_dim"):
        tr.train_step(state, a, None, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        tr.train_step(state, a, goal, torch.zeros(4, 3))
    aware = GuideTrainer(MLPGuide(_net(14), use_sigma=True))
    assert aware.sample_density is None
    sd = tr.state_dict()
    assert sorted(sd) == ["generator", "loss", "network", "optimizer", "version"] and sorted(sd["network"]) == sorted(tr.guide.network.state_dict())
    with pytest.raises(ValueError, match="loss"):
        _trainer(loss="mse").load_state_dict(sd)
    other = _trainer(loss="bce", seed=2)
    other.load_state_dict(sd)
    assert torch.equal(other.generator.get_state(), tr.generator.get_state())
    assert all(torch.equal(p, q) for p, q in zip(other.guide.parameters(), tr.guide.parameters()))


# -------------------------------------------------------------------------------------------------
# the library
# -------------------------------------------------------------------------------------------------
def test_library_exports_what_its_header_declares(lib):
    """libbeso_guidefit.so: the four symbols of include/beso_guide_fit.h, no more; the binding table has the header's argument
    counts; the loss enum is the binding's; libbeso_guide.so still exports its two."""
    import re
    text = check_side_library("beso_guide_fit.h", "beso_guide_", _lib.GUIDEFIT_SIGNATURES, _lib.GUIDEFIT_LIB_PATH, _lib.load_guidefit, 4,
                              min_kernels=3, min_mfma=12)
    assert sorted(_lib.GUIDEFIT_SIGNATURES) == sorted(_lib.GUIDEFIT_EXPORTS)
    consts = dict(re.findall(r"\b(BESO_GUIDE_FIT_[A-Z]+)\s*=\s*(\d+)", text))
    assert {k: int(consts["BESO_GUIDE_FIT_" + k.upper()]) for k in _lib.GUIDEFIT_LOSSES} == _lib.GUIDEFIT_LOSSES
    assert list(_lib.GUIDE_SIGNATURES) == ["beso_guide_supported", "beso_guide_apply"]
    # beso_guide_apply_sigma is beso_guide_apply with c_noise behind sigma
    a, s = _lib.GUIDE_SIGNATURES["beso_guide_apply"][1], _lib.GUIDEFIT_SIGNATURES["beso_guide_apply_sigma"][1]
    assert s[:7] == a[:7] and s[8:] == a[7:] and s[7] is _lib.vp


def test_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers: a call that got past its checks would read and write through them."""
    g = _lib.load_guidefit()
    D = _lib.MlpDims
    one, odd = C.c_void_p(16), C.c_void_p(18)
    arr = lambda n: (C.c_void_p * n)(*([16] * n))                                       # noqa: E731

    def rows(state=one, action=one, goal=one, sigma=one, noise=one, c_noise=one, B=4, T=3, steps=3, G=2, grows=4, obs=5, act=3, out=one):
        return g.beso_guide_fit_rows(state, action, goal, sigma, noise, c_noise, B, T, steps, G, grows, obs, act, out, None)

    for bad in (dict(obs=0), dict(act=0), dict(obs=513), dict(obs=250, act=13), dict(B=0), dict(T=0), dict(B=-2), dict(steps=2),
                dict(G=0), dict(grows=3), dict(goal=None), dict(B=1 << 20, T=1 << 12, steps=1 << 12, grows=1)):
        assert rows(**bad) == _lib.ERR_BAD_SHAPE, bad
    for bad in (dict(state=None), dict(action=None), dict(out=None), dict(sigma=None), dict(noise=None), dict(out=odd),
                dict(c_noise=odd), dict(goal=odd)):
        assert rows(**bad) == _lib.ERR_BAD_ARG, bad

    def loss(q=one, y=one, w=one, M=6, kind=0, out=one, per_row=one, dq=one):
        return g.beso_guide_fit_loss(q, y, w, M, kind, out, per_row, dq, None)

    assert loss(M=0) == _lib.ERR_BAD_SHAPE and loss(M=-1) == _lib.ERR_BAD_SHAPE and loss(M=1 << 31) == _lib.ERR_BAD_SHAPE
    for bad in (dict(kind=2), dict(kind=-1), dict(q=None), dict(y=None), dict(out=None), dict(per_row=None), dict(dq=None),
                dict(w=odd), dict(dq=odd)):
        assert loss(**bad) == _lib.ERR_BAD_ARG, bad

    good = D(14, 48, 2, 1, 1)                                                           # obs 5, act 3, goal, c_noise: 5 + 3 + 5 + 1
    sup = lambda d, obs=5, act=3, goal=1: g.beso_guide_supported_sigma(C.byref(d), obs, act, goal)       # noqa: E731

    def apply(d=good, n=None, goal=one, c_noise=one, B=4, T=3, steps=3, G=2, grows=4, out=one):
        n = 2 * (d.n_hidden + 1) if n is None else n
        return g.beso_guide_apply_sigma(arr(max(n, 1)), n, C.byref(d), one, goal, one, one, c_noise, B, T, steps, G, grows, 5, 3, 1.5, out,
                                        None)

    assert sup(good) == _lib.OK and sup(D(9, 48, 2, 1, 1), goal=0) == _lib.OK
    assert sup(D(13, 48, 2, 1, 1)) == _lib.ERR_BAD_SHAPE and apply(D(13, 48, 2, 1, 1)) == _lib.ERR_BAD_SHAPE     # the column is not optional
    assert sup(D(14, 512, 2, 1, 1)) == _lib.OK and sup(D(14, 512, 3, 1, 1)) == _lib.ERR_BAD_SHAPE                # the LDS rule
    assert sup(D(512, 48, 2, 1, 1), obs=250, act=11) == _lib.OK and sup(D(513, 48, 2, 1, 1), obs=250, act=12) == _lib.ERR_BAD_SHAPE
    assert apply(steps=2) == _lib.ERR_BAD_SHAPE and apply(goal=None) == _lib.ERR_BAD_SHAPE and apply(B=0) == _lib.ERR_BAD_SHAPE
    assert apply(c_noise=None) == _lib.ERR_BAD_ARG and apply(c_noise=odd) == _lib.ERR_BAD_ARG and apply(n=4) == _lib.ERR_BAD_ARG
    assert apply(out=None) == _lib.ERR_BAD_ARG and apply(D(14, 48, 2, 1, 3)) == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError, match="beso_guide_fit_rows"):
        _lib.check(rows(steps=2), "beso_guide_fit_rows")
