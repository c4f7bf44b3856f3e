"""MinMaxScaler on the MI355X: ``scale_many`` (beso_scale_rows_mixed) against the per-tensor torch methods, ``VectorRollout``
with a MinMaxScaler (beso_rollout_begin + beso_rollout_end_minmax) against a restatement with the scaler's own torch methods on
the same sampler outputs, and the tail kernel's index arithmetic.  Every comparison is bit for bit (NaN equal to NaN): the
kernels perform the same individually rounded IEEE operations in the same order as the torch expressions."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from support import bits, build_agent, make_denoiser
from beso_amd import _lib
from beso_amd.networks.scaler.scaler_class import MinMaxScaler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(a, b):
    """Equal dtype, shape and bits, a NaN equal to any NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype != torch.float32:
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return bool(((bits(a) == bits(b)) | (a.isnan() & b.isnan())).all())


def _scaler(x_dim, y_dim, seed, dtype=np.float32, scale_data=True, constant=None):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((64, x_dim)) * 2 + 0.5).astype(dtype)
    y = (rng.standard_normal((64, y_dim)) * 1.5 - 0.25).astype(dtype)
    if constant is not None:
        y[:, constant] = 0.375
    return MinMaxScaler(x, y, scale_data, DEV)


class _Spy:
    """Counts the calls of one entry point of libbeso_scale.so and of the scaler's per-tensor scalings while it is active."""

    def __init__(self, monkeypatch, sc, entry):
        lib = _lib.load_scale()
        self.launches, self.per_tensor = 0, 0
        real = getattr(lib, entry)

        def counted(*a):
            self.launches += 1
            return real(*a)

        monkeypatch.setattr(lib, entry, counted, raising=True)
        for name in ("scale_input", "scale_output", "clip_action", "inverse_scale_output"):
            monkeypatch.setattr(sc, name, self._wrap(getattr(sc, name)), raising=False)

    def _wrap(self, fn):
        def counted(*a, **k):
            self.per_tensor += 1
            return fn(*a, **k)
        return counted


def _per_tensor(sc, items):
    cls = type(sc)
    return [cls.scale_input(sc, v) if w == "x" else cls.scale_output(sc, v) for v, w in items]


# (x_dim, y_dim, [(shape without the feature axis, 'x' | 'y'), ...]): rows 1 / 3 / 257 (a second block of 256 threads),
# cols 1 / 2 / 16 / 30, one / three / four items, mixed kinds
MANY = [
    (16, 2, [((257,), "x"), ((3,), "x"), ((257,), "y")]),
    (30, 1, [((1,), "x"), ((3, 5), "x"), ((257,), "y"), ((1,), "y")]),
    (1, 2, [((257,), "x")]),
    (1, 2, [((3,), "y")]),
    (2, 16, [((257,), "y"), ((3,), "x"), ((1, 3), "y")]),
    (30, 30, [((257,), "y"), ((1,), "x"), ((3,), "y"), ((257,), "x")]),
]


@pytest.mark.parametrize("case", range(len(MANY)))
def test_scale_many_is_one_launch_with_the_per_tensor_bits(case, monkeypatch):
    x_dim, y_dim, shapes = MANY[case]
    sc = _scaler(x_dim, y_dim, seed=40 + case)
    g = torch.Generator(DEV).manual_seed(case)
    items = [(torch.randn(lead + (x_dim if w == "x" else y_dim,), device=DEV, generator=g) * 2 + 0.25, w) for lead, w in shapes]
    want = _per_tensor(sc, items)
    spy = _Spy(monkeypatch, sc, "beso_scale_rows_mixed")
    got = sc.scale_many(items)
    assert (spy.launches, spy.per_tensor) == (1, 0)
    assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))
    assert all(a.data_ptr() != v.data_ptr() for a, (v, _) in zip(got, items))
    assert all(torch.isfinite(a).all() for a in got)


def test_scale_many_divides_by_zero_as_torch_does(monkeypatch):
    """Action component 1 is constant in the data: y_max - y_min = 0 there.  The one launch returns torch's pattern: NaN where the
    input equals the constant (0 / 0), +-inf elsewhere, finite values in the other component."""
    sc = _scaler(16, 2, seed=50, constant=1)
    assert float(sc._y_range()[1]) == 0.0
    y = torch.randn(257, 2, device=DEV) * 2
    y[::3, 1] = 0.375
    x = torch.randn(3, 16, device=DEV)
    items = [(y, "y"), (x, "x"), (y[:1].contiguous(), "y")]
    want = _per_tensor(sc, items)
    spy = _Spy(monkeypatch, sc, "beso_scale_rows_mixed")
    got = sc.scale_many(items)
    assert (spy.launches, spy.per_tensor) == (1, 0)
    assert all(same(a, b) for a, b in zip(got, want))
    col = got[0][:, 1]
    assert bool(col[::3].isnan().all()) and bool(col[1::3].isinf().all()) and bool(torch.isfinite(got[0][:, 0]).all())
    assert bool((col[1::3] > 0).any()) and bool((col[1::3] < 0).any())


def test_scale_many_fallbacks_take_the_per_tensor_methods(monkeypatch):
    """float64 statistics, scale_data off, a 4-of-16 goal in the batch, a CPU tensor, a non-contiguous tensor and five items:
    no launch, the per-tensor methods' results."""
    g = torch.Generator(DEV).manual_seed(3)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)                # noqa: E731
    batch = [(r(7, 16), "x"), (r(3, 16), "x"), (r(7, 2), "y")]
    cases = {
        "float64 statistics": (_scaler(16, 2, 60, dtype=np.float64), batch),
        "scale_data off": (_scaler(16, 2, 61, scale_data=False), batch),
        "a 4-of-16 goal": (_scaler(16, 2, 62), [batch[0], (r(3, 4), "x"), batch[2]]),
        "a CPU tensor": (_scaler(16, 2, 63), [batch[0], (batch[2][0].cpu(), "y")]),
        "not contiguous": (_scaler(16, 2, 64), [(r(16, 7).t(), "x")]),
        "five items": (_scaler(16, 2, 65), batch + batch[:2]),
    }
    for name, (sc, items) in cases.items():
        want = _per_tensor(sc, items)
        with monkeypatch.context() as m:
            spy = _Spy(m, sc, "beso_scale_rows_mixed")
            got = sc.scale_many(items)
        assert spy.launches == 0 and spy.per_tensor == len(items), name
        assert all(same(a.to(DEV), b.to(DEV)) for a, b in zip(got, want)), name


def test_process_batch_scales_a_training_batch_in_one_launch(monkeypatch):
    """BaseAgent.process_batch with a MinMaxScaler: state, goal and action through ONE beso_scale_rows_mixed launch."""
    cfg = O.TINY
    agent = build_agent(cfg, lambda: make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.05), "fp32"), device=DEV)
    sc = _scaler(cfg.obs_dim, cfg.act_dim, seed=70)
    agent.get_scaler(sc)
    batch = {"observation": torch.randn(5, cfg.obs_seq_len, cfg.obs_dim, device=DEV),
             "goal_observation": torch.randn(5, cfg.goal_seq_len, cfg.obs_dim, device=DEV),
             "action": torch.randn(5, cfg.obs_seq_len, cfg.act_dim, device=DEV)}
    want = _per_tensor(sc, [(batch["observation"], "x"), (batch["goal_observation"], "x"), (batch["action"], "y")])
    spy = _Spy(monkeypatch, sc, "beso_scale_rows_mixed")
    state, action, goal = agent.process_batch(batch, predict=False)
    assert (spy.launches, spy.per_tensor) == (1, 0)
    assert same(state, want[0]) and same(goal, want[1]) and same(action, want[2])


# ------------------------------------------------------------------------------------------------ the rollout
def _agent(cfg, window):
    """tests/test_rollout.py's agent (seeded weights, the EMA shadow equal to them) with a window of `window` observations."""
    w = O.make_weights(cfg, seed=3, std=0.05)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, w, "fp32"), device=DEV, sampler="ddim")
    agent.ema_helper.load_shadow_params(agent.model.get_params())
    agent.window_size = window
    return agent


def _run_rollout(agent, sc, monkeypatch, candidates=None, seed=17):
    """N = 3, W = 2, five steps, environment 1 reset before step 3: lengths 1, 2, the shifted full window and 1, 2 again beside
    full windows.  Every step against the scaler's own torch methods on the step's sampler output.  -> (launches of the tail,
    calls of the scaler's methods inside the steps, components clipped, components seen, predictions)."""
    cfg, N, W = O.TINY, 3, 2
    agent.get_scaler(sc)
    agent.set_bounds(sc)
    cls = type(sc)
    g = torch.Generator(DEV).manual_seed(seed)
    goal = torch.randn((N, cfg.goal_seq_len, cfg.obs_dim), device=DEV, generator=g)
    roll = agent.vector_rollout(N)
    assert roll.window == W
    roll.set_goal(goal)
    rows = torch.arange(N, device=DEV)
    launches = calls = n_clipped = n_seen = 0
    seen_lengths, preds = [], []
    for step in range(5):
        if step == 3:
            roll.reset([1])
        obs = torch.randn((N, cfg.obs_dim), device=DEV, generator=g) * 2 + 0.5
        noise = torch.randn((N, candidates or 1, cfg.act_dim), device=DEV, generator=g)
        before = roll.act_ctx.clone()
        with monkeypatch.context() as m:
            spy = _Spy(m, sc, "beso_rollout_end_minmax")
            if candidates is None:
                pred = roll.step(obs, noise=noise)
            else:
                pred = roll.step(obs, noise=noise, candidates=candidates, select="mean")
        launches += spy.launches
        calls += spy.per_tensor
        lengths = roll.last["lengths"].tolist()
        seen_lengths.append(lengths)
        slot = (roll.last["lengths"] - 1).long()
        raw = roll.last["x0"][rows, slot]
        clipped = cls.clip_action(sc, raw)
        want = cls.inverse_scale_output(sc, clipped)
        assert pred.shape == (N, cfg.act_dim) and same(pred, want), step
        assert same(roll.act_ctx[rows, slot], clipped), step
        assert same(roll.last["state"][rows, slot], cls.scale_input(sc, obs).to(torch.float32)), step
        # the other slots of act_ctx: untouched by the tail (a full window's older slot is what begin shifted down)
        for n in range(N):
            for j in range(W):
                if j != int(slot[n]) and j < lengths[n]:
                    shifted = step > 0 and seen_lengths[-2][n] == W and not (step == 3 and n == 1)
                    assert same(roll.act_ctx[n, j], before[n, j + 1] if shifted else before[n, j]), (step, n, j)
        n_clipped += int((clipped != raw).sum())
        n_seen += raw.numel()
        preds.append(pred)
    assert seen_lengths == [[1, 1, 1], [2, 2, 2], [2, 2, 2], [2, 1, 2], [2, 2, 2]]
    return launches, calls, n_clipped, n_seen, torch.stack(preds)


def test_rollout_with_minmax_scaler_takes_both_launches_and_keeps_the_scalers_bits(monkeypatch):
    """The fp32 MinMaxScaler: _scaler_plan hands the z-score pair to beso_rollout_begin and the min-max tail to
    beso_rollout_end_minmax, no scaler method runs inside a step, and actions, act_ctx and the scaled observations are the
    scaler's own bits.  Then y_bounds_tensor x 0.05, so that the clip acts: 45 components (5 steps x 3 environments x 3), of
    which some but not all must be clipped (the count is printed).  Then best-of-4 with the mean selection in front of the tail."""
    cfg = O.TINY
    agent = _agent(cfg, 2)
    sc = _scaler(cfg.obs_dim, cfg.act_dim, seed=7)
    agent.get_scaler(sc)
    xs, ys = agent.vector_rollout(3)._scaler_plan()
    assert xs is not None and xs[0] is sc.x_mean and xs[1] is sc._den()
    assert ys is not None and ys.kind == "minmax" and len(ys.stats) == 4 and ys.lo.dtype == ys.hi.dtype == torch.float64
    assert all(s is not None for s in ys.stats)
    launches, calls, n_clipped, n_seen, plain = _run_rollout(agent, sc, monkeypatch)
    assert (launches, calls) == (5, 0)
    print(f"[minmax] rollout, data bounds: {n_clipped} of {n_seen} components clipped")

    sc.y_bounds_tensor = sc.y_bounds_tensor * 0.05
    launches, calls, n_clipped, n_seen, tight = _run_rollout(agent, sc, monkeypatch)
    print(f"[minmax] rollout, bounds x 0.05: {n_clipped} of {n_seen} components clipped")
    assert (launches, calls) == (5, 0) and n_seen == 45
    assert 0 < n_clipped < n_seen
    assert not torch.equal(plain, tight)

    sc.y_bounds_tensor = sc.y_bounds_tensor * 20.0
    launches, calls, _, _, _ = _run_rollout(agent, sc, monkeypatch, candidates=4)
    assert (launches, calls) == (5, 0)


def test_rollout_declines_the_scalers_the_launches_do_not_serve(monkeypatch):
    """float64 statistics and a subclass that overrides one method: _scaler_plan answers (None, None), the step runs the scaler's
    own methods (scale_input, clip_action, inverse_scale_output per step) and the results are still the scaler's bits; with
    scale_data off the tail launch runs without statistics and the prediction is the clipped action."""
    cfg = O.TINY
    agent = _agent(cfg, 2)

    class Mine(MinMaxScaler):
        def clip_action(self, y):
            return super().clip_action(y)

    rng = np.random.default_rng(5)
    x, y = (rng.standard_normal((64, cfg.obs_dim)) * 2 + 0.5).astype(np.float32), (rng.standard_normal((64, cfg.act_dim)) * 1.5).astype(np.float32)
    for name, sc in (("float64", _scaler(cfg.obs_dim, cfg.act_dim, seed=8, dtype=np.float64)), ("subclass", Mine(x, y, True, DEV))):
        agent.get_scaler(sc)
        assert agent.vector_rollout(3)._scaler_plan() == (None, None), name
        launches, calls, _, _, preds = _run_rollout(agent, sc, monkeypatch)
        assert launches == 0 and calls == 15, name
        assert preds.dtype == (torch.float64 if name == "float64" else torch.float32)
    raw = _scaler(cfg.obs_dim, cfg.act_dim, seed=9, scale_data=False)
    raw.y_bounds_tensor = raw.y_bounds_tensor * 0.05
    agent.get_scaler(raw)
    xs, ys = agent.vector_rollout(3)._scaler_plan()
    assert xs is None and ys.kind == "minmax" and ys.stats == (None,) * 4
    launches, calls, n_clipped, n_seen, _ = _run_rollout(agent, raw, monkeypatch)
    assert launches == 5 and calls == 5 and n_clipped > 0           # (scale_input: a .to() per step)


# ------------------------------------------------------------------------------------------------ the tail kernel alone
def _end(x0, lengths, lo, hi, stats, W, act):
    N = lengths.numel()
    act_ctx = torch.full((N, W, act), 7.0, device=DEV)
    pred = torch.full((N, act), 9.0, device=DEV)
    ptr = lambda v: None if v is None else v.data_ptr()                     # noqa: E731
    st = _lib.load_scale().beso_rollout_end_minmax(x0.data_ptr(), lengths.data_ptr(), lo.data_ptr(), hi.data_ptr(), *[ptr(s) for s in stats],
                                                   act_ctx.data_ptr(), pred.data_ptr(), N, W, act, torch.cuda.current_stream().cuda_stream)
    _lib.check_scale(st, "rollout_end_minmax")
    torch.cuda.synchronize()
    return act_ctx, pred


@pytest.mark.parametrize("N,W,act", [(300, 1, 1), (200, 3, 2)])
def test_tail_kernel_index_arithmetic(N, W, act):
    """W = 1 and act = 1 (every index is the environment's), and W = 3, act = 2 with lengths outside 1 ... W (read as the nearest
    end), both over more than one block of 256 threads: the chosen slot, the clip in double with a NaN passing through, the four
    un-scale operations, and no write outside slot t - 1."""
    g = torch.Generator(DEV).manual_seed(N)
    x0 = torch.randn((N, W, act), device=DEV, generator=g) * 2
    x0[5, :, 0] = float("nan")
    lengths = torch.randint(1, W + 1, (N,), device=DEV, generator=g, dtype=torch.int32)
    lengths[0], lengths[1] = 0, W + 5
    sc = _scaler(4, act, seed=N)
    lo, hi = (sc.y_bounds_tensor[0] * 1.1).contiguous(), (sc.y_bounds_tensor[1] * 1.1).contiguous()
    stats = (sc.new_min_y, sc._y_span(), sc._y_range(), sc.y_min)
    slot = (lengths.clamp(1, W) - 1).long()
    rows = torch.arange(N, device=DEV)
    raw = x0[rows, slot]
    clipped = sc.clip_action(raw)
    assert 0 < int((clipped != raw).sum()) < raw.numel()
    for with_stats in (True, False):
        act_ctx, pred = _end(x0, lengths, lo, hi, stats if with_stats else (None,) * 4, W, act)
        assert same(pred, sc.inverse_scale_output(clipped) if with_stats else clipped)
        assert same(act_ctx[rows, slot], clipped) and bool(pred[5, 0].isnan())
        mask = torch.ones((N, W), dtype=torch.bool, device=DEV)
        mask[rows, slot] = False
        assert bool((act_ctx[mask] == 7.0).all())


def test_argument_errors_are_named_and_a_valid_call_follows():
    """NULL pointers, zero items, five items and act_dim < 1 on the GPU machine: an error by name, nothing enqueued, and the next
    valid call of either entry point succeeds."""
    sc_lib = _lib.load_scale()
    msg = lambda: sc_lib.beso_scale_last_error().decode()                  # noqa: E731
    sc = _scaler(16, 2, seed=90)
    x = torch.randn(3, 16, device=DEV)
    out = torch.empty_like(x)
    vp = C.c_void_p * 1
    tabs = dict(src=vp(x.data_ptr()), dst=vp(out.data_ptr()), kind=(C.c_int * 1)(0), p0=vp(sc.x_mean.data_ptr()), p1=vp(sc._den().data_ptr()),
                p2=None, p3=None, rows=(C.c_longlong * 1)(3), cols=(C.c_int * 1)(16))
    call = lambda n=1, **k: sc_lib.beso_scale_rows_mixed(*[{**tabs, **k}[a] for a in tabs], n, torch.cuda.current_stream().cuda_stream)   # noqa: E731
    assert call(n=0) == _lib.ERR_BAD_ARG and "n = 0" in msg()
    assert call(n=5) == _lib.ERR_BAD_ARG and "n = 5" in msg()
    assert call(src=None) == _lib.ERR_BAD_ARG and "NULL" in msg()
    assert call(dst=vp(None)) == _lib.ERR_BAD_ARG and "NULL pointer" in msg()
    assert call(kind=(C.c_int * 1)(1)) == _lib.ERR_BAD_ARG and "p2 / p3" in msg()
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert same(out, sc.scale_input(x))

    N, W, act = 4, 2, 2
    x0 = torch.randn(N, W, act, device=DEV)
    lengths = torch.tensor([1, 2, 2, 1], dtype=torch.int32, device=DEV)
    lo, hi = (sc.y_bounds_tensor[0] * 1.1).contiguous(), (sc.y_bounds_tensor[1] * 1.1).contiguous()
    stats = (sc.new_min_y, sc._y_span(), sc._y_range(), sc.y_min)
    act_ctx, pred = torch.zeros(N, W, act, device=DEV), torch.zeros(N, act, device=DEV)
    args = dict(x0=x0, lengths=lengths, lo=lo, hi=hi, new_lo=stats[0], span=stats[1], range=stats[2], lo_y=stats[3], act_ctx=act_ctx, pred=pred)
    end = lambda act_dim=act, **k: sc_lib.beso_rollout_end_minmax(                                           # noqa: E731
        *[None if v is None else v.data_ptr() for v in {**args, **k}.values()], N, W, act_dim, torch.cuda.current_stream().cuda_stream)
    assert end(act_dim=0) == _lib.ERR_BAD_SHAPE and "act_dim = 0" in msg()
    assert end(x0=None) == _lib.ERR_BAD_ARG and "NULL pointer" in msg()
    assert end(span=None) == _lib.ERR_BAD_ARG and "3 of 4" in msg()
    torch.cuda.synchronize()
    assert not act_ctx.any() and not pred.any()                             # the refused calls wrote nothing
    assert end() == _lib.OK
    torch.cuda.synchronize()
    rows, slot = torch.arange(N, device=DEV), (lengths - 1).long()
    assert same(pred, sc.inverse_scale_output(sc.clip_action(x0[rows, slot])))
