"""MinMaxScaler (beso_amd/networks/scaler/scaler_class.py) against what the reference's class recorded in
tests/golden/minmax_scaler.npz (tests/golden/make_minmax_fixtures.py): every attribute and every method output, bit for bit and
dtype for dtype, on CPU tensors; the 4-of-16 block-push goal of both scalers; Scaler's unchanged bits on inputs it took before;
and the C ABI of libbeso_scale.so (include/beso_scale.h) against its binding table.  No GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from beso_amd import _lib
from beso_amd.networks.scaler.scaler_class import MinMaxScaler, Scaler
from conftest import load_golden
from support import lib  # noqa: F401
from test_cabi import _ctypes_class, _header, _prototypes, declared_symbols, exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def load_fixture():
    """{name: array} of minmax_scaler.npz: one byte string and an index of "name dtype shape offset" lines."""
    fx = load_golden("minmax_scaler.npz")
    blob, out = fx["blob"].tobytes(), {}
    for line in fx["index"].tolist():
        name, dtype, shape, offset = line.split(" ")
        shape = tuple(int(s) for s in shape.split(",") if s)
        dt = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        out[name] = np.frombuffer(blob[int(offset):int(offset) + n], dtype=dt).reshape(shape).copy()
    return out


def same(got, want):
    """Equal dtype, shape and bits (NaN equal to NaN, +0 distinct from -0)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def fitted(fx, case, cls=MinMaxScaler, as_tensor=False):
    x, y = fx[f"{case}::x_data"].copy(), fx[f"{case}::y_data"].copy()
    if as_tensor:
        x, y = torch.from_numpy(x), torch.from_numpy(y)
    return cls(x, y, bool(fx[f"{case}::scale_data"]), "cpu")


CASES = ("f32_2d_scaled", "f64_2d_scaled", "f32_3d_scaled", "f64_3d_unscaled", "f32_2d_unscaled", "f32_2d_constant_action",
         "f32_2d_onehot")
METHODS = {"scale_input": "scale_input", "scale_input_3d": "scale_input", "scale_output": "scale_output",
           "inverse_scale_input": "inverse_scale_input", "inverse_scale_output": "inverse_scale_output", "clip_action": "clip_action",
           "scale_block_push_goal": "scale_block_push_goal", "scale_input_goal4": "scale_input", "scale_input_onehot": "scale_input"}


def test_fixture_holds_the_cases_the_checks_need():
    """fp32 and float64 data, scale_data on and off, 2-D and 3-D data, a 4-wide goal against 16 statistics, a 7-wide input
    against 30, clipped and unclipped components in every clip_action record, and a division by zero."""
    fx = load_fixture()
    assert tuple(fx["cases"].tolist()) == CASES
    assert {fx[f"{c}::x_data"].dtype for c in CASES} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {fx[f"{c}::x_data"].ndim for c in CASES} == {2, 3}
    assert {bool(fx[f"{c}::scale_data"]) for c in CASES} == {True, False}
    assert fx["f32_2d_onehot::attr::x_mean"].shape == (30,) and fx["f32_2d_onehot::in::scale_input_onehot"].shape[-1] == 7
    for c in CASES:
        assert fx[f"{c}::y_data"].shape[-1] == 2 and fx[f"{c}::x_data"].shape[-1] in (16, 30)
        moved = fx[f"{c}::out::clip_action"] != fx[f"{c}::in::clip_action"]
        assert 0 < int(moved.sum()) < moved.size, c
        if fx[f"{c}::x_data"].shape[-1] == 16:
            assert fx[f"{c}::in::scale_input_goal4"].shape == (3, 4)
    assert not np.isfinite(fx["f32_2d_constant_action::out::scale_output"]).all()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("as_tensor", [False, True])
def test_attributes_are_the_references(case, as_tensor):
    """Every attribute the reference's constructor leaves, from numpy data and from tensors: bits, shapes and dtypes."""
    fx = load_fixture()
    sc = fitted(fx, case, as_tensor=as_tensor)
    assert sc.scale_data == bool(fx[f"{case}::scale_data"]) and sc.device == "cpu"
    for a in fx["attrs"].tolist():
        got = getattr(sc, a)
        assert isinstance(got, np.ndarray) == (a in ("y_bounds", "x_bounds")), a
        assert same(got, fx[f"{case}::attr::{a}"]), (case, a)
    assert sc.new_min_y.dtype == sc.y_max.dtype and float(sc.new_min_y[0]) == -1.0 and float(sc.new_max_x[0]) == 1.0


@pytest.mark.parametrize("case", CASES)
def test_methods_return_the_references_bits(case):
    """Every recorded call -- the 3-D input, the 4-of-16 goal through scale_input and through scale_block_push_goal, the one-hot
    pass-through, values outside the bounds, the division by zero of a constant action component -- twice, so that the second
    call runs on the cached tensors."""
    fx = load_fixture()
    sc = fitted(fx, case)
    calls = [k.split("::in::")[1] for k in fx if k.startswith(f"{case}::in::") and "zscore" not in k]
    assert len(calls) >= 7
    for _ in range(2):
        for key in calls:
            got = getattr(sc, METHODS[key])(torch.from_numpy(fx[f"{case}::in::{key}"].copy()))
            assert same(got, fx[f"{case}::out::{key}"]), (case, key)
    assert sc.scale_input(torch.zeros(2, sc.x_mean.numel()), block_push_goal=True).shape == (2, sc.x_mean.numel())


def test_caches_follow_their_source_tensors():
    """A statistic replaced or written in place is picked up by the next call (identity and _version key the caches)."""
    fx = load_fixture()
    sc = fitted(fx, "f32_2d_scaled")
    x = torch.from_numpy(fx["f32_2d_scaled::in::scale_input"].copy())
    y = torch.from_numpy(fx["f32_2d_scaled::in::scale_output"].copy())
    a = torch.from_numpy(fx["f32_2d_scaled::in::clip_action"].copy())
    first = (sc.scale_input(x), sc.scale_output(y), sc.clip_action(a))
    den, rng_ = sc._den(), sc._y_range()
    assert sc._den() is den and sc._y_range() is rng_ and sc._y_span() is sc._y_span()
    sc.x_std.mul_(2.0)                                  # in place: the version moves
    sc.y_max = sc.y_max + 1.0                           # replaced: the identity moves
    sc.y_bounds_tensor = sc.y_bounds_tensor * 0.5
    assert torch.equal(sc.scale_input(x), ((x - sc.x_mean) / (sc.x_std + 1e-12 * torch.ones(16))).to(torch.float32))
    assert torch.equal(sc.scale_output(y), ((y - sc.y_min) / (sc.y_max - sc.y_min) * (sc.new_max_y - sc.new_min_y) + sc.new_min_y))
    assert torch.equal(sc.clip_action(a), torch.clamp(a, sc.y_bounds_tensor[0] * 1.1, sc.y_bounds_tensor[1] * 1.1).to(torch.float32))
    assert not torch.equal(sc.scale_input(x), first[0]) and not torch.equal(sc.scale_output(y), first[1])
    assert not torch.equal(sc.clip_action(a), first[2])


def test_scale_many_on_cpu_tensors_is_the_per_tensor_methods():
    """CPU tensors, float64 statistics, scale_data off, a 4-of-16 goal, five items: scale_many returns what the per-tensor
    methods return (and needs no library to do so)."""
    fx = load_fixture()
    for case in ("f32_2d_scaled", "f64_2d_scaled", "f32_2d_unscaled"):
        sc = fitted(fx, case)
        x, x3, g4, y = (torch.from_numpy(fx[f"{case}::in::{k}"].copy()) for k in ("scale_input", "scale_input_3d", "scale_input_goal4",
                                                                             "scale_output"))
        items = [(x3, "x"), (g4, "x"), (y, "y"), (x, "x"), (y, "y")]
        for n in (1, 3, 5):
            got = sc.scale_many(items[:n])
            want = [sc.scale_input(v) if w == "x" else sc.scale_output(v) for v, w in items[:n]]
            assert len(got) == n and all(same(a, b.numpy()) for a, b in zip(got, want)), (case, n)
        assert same(sc.scale_many([(g4, "x")])[0], fx[f"{case}::out::scale_block_push_goal"])


def test_process_batch_scales_through_scale_many():
    """BaseAgent.process_batch hands a MinMaxScaler's batch to scale_many: state and goal z-scored, the action min-max scaled."""
    from oracle import beso_oracle as O
    from support import build_agent, make_denoiser
    import dataclasses
    cfg = dataclasses.replace(O.TINY, linear_output=False)
    agent = build_agent(cfg, lambda: make_denoiser(cfg, precision=None, device="cpu", train=True))
    rng = np.random.default_rng(2)
    sc = MinMaxScaler(rng.standard_normal((32, cfg.obs_dim)).astype(np.float32), rng.standard_normal((32, cfg.act_dim)).astype(np.float32),
                      True, "cpu")
    agent.get_scaler(sc)
    seen = []
    sc.scale_many = lambda items: seen.append([w for _, w in items]) or MinMaxScaler.scale_many(sc, items)
    enc = agent.input_encoder
    batch = {enc.state_modality: torch.randn(4, cfg.obs_seq_len, cfg.obs_dim), enc.goal_modality: torch.randn(4, cfg.goal_seq_len, cfg.obs_dim),
             agent.target_modality: torch.randn(4, cfg.obs_seq_len, cfg.act_dim)}
    state, action, goal = agent.process_batch(batch, predict=False)
    assert seen == [["x", "x", "y"]]
    assert torch.equal(state, sc.scale_input(batch[enc.state_modality])) and torch.equal(goal, sc.scale_input(batch[enc.goal_modality]))
    assert torch.equal(action, sc.scale_output(batch[agent.target_modality]))


# ------------------------------------------------------------------------------------------------ the z-score Scaler
@pytest.mark.parametrize("case", [c for c in CASES if c != "f32_2d_onehot"])
def test_scaler_takes_the_4_of_16_goal_as_the_reference_scaler_does(case):
    """A 4-wide goal against 16 statistics: Scaler.scale_input takes scale_block_push_goal, and both equal what the reference's
    Scaler recorded on the same data; scale_many sends the item to the per-tensor methods."""
    fx = load_fixture()
    sc = fitted(fx, case, cls=Scaler)
    g4 = torch.from_numpy(fx[f"{case}::in::zscore::scale_input_goal4"].copy())
    assert same(sc.scale_input(g4), fx[f"{case}::out::zscore::scale_input_goal4"])
    assert same(sc.scale_block_push_goal(g4), fx[f"{case}::out::zscore::scale_block_push_goal"])
    x = torch.from_numpy(fx[f"{case}::in::scale_input"].copy())
    got = sc.scale_many([(x, "x"), (g4, "x")])
    assert same(got[1], fx[f"{case}::out::zscore::scale_input_goal4"]) and torch.equal(got[0], sc.scale_input(x))


def test_scaler_keeps_its_bits_on_the_inputs_it_took_before():
    """Scaler on the recorded agent trace (tests/golden/tiny_agent_trace.npz): scale_input, scale_output, inverse_scale_output
    and clip_action equal the expressions the class evaluated before it knew the 4-of-16 goal, stated here operation by
    operation; neither width of that fixture meets the new branch."""
    fx = load_golden("tiny_agent_trace.npz")
    sc = Scaler(fx["x_data"], fx["y_data"], True, "cpu")
    assert not (len(sc.x_mean) == 16)
    calls = range(int(fx["n_calls"]))
    obs = [torch.from_numpy(fx[f"call{c}::obs"].copy()) for c in calls]
    for x in (*obs, torch.from_numpy(fx["goal"].copy()), obs[0].double()):
        assert torch.equal(sc.scale_input(x), ((x - sc.x_mean) / (sc.x_std + 1e-12)).to(torch.float32))
    y = torch.cat([torch.from_numpy(fx[f"call{c}::pred"].copy()).reshape(-1, sc.y_mean.numel()) for c in calls])
    assert torch.equal(sc.scale_output(y), ((y - sc.y_mean) / (sc.y_std + 1e-12)).to(torch.float32))
    assert torch.equal(sc.inverse_scale_output(y), y * (sc.y_std + 1e-12) + sc.y_mean)
    b = sc.y_bounds_tensor
    assert torch.equal(sc.clip_action(y * 3), torch.clamp(y * 3, b[0] * 1.1, b[1] * 1.1).to(torch.float32))
    # a 7-wide input against 30 statistics still passes through, a 4-wide one against 30 still does not take the goal branch
    rng = np.random.default_rng(1)
    sc30 = Scaler(rng.standard_normal((20, 30)).astype(np.float32), rng.standard_normal((20, 9)).astype(np.float32), True, "cpu")
    onehot = torch.eye(7)[[1, 5]]
    assert sc30.scale_input(onehot) is onehot
    with pytest.raises(RuntimeError):
        sc30.scale_input(torch.zeros(2, 4))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_scale_header_matches_its_signature_table(lib):
    """include/beso_scale.h against _lib.SCALE_SIGNATURES with test_cabi.py's prototype parser: the same three functions in the
    header's order, per function the argument count, the class of every argument and the return type; the library exports
    exactly these; the enum and the limit agree with the binding's tables."""
    import re
    protos, sigs = _prototypes("beso_scale.h"), _lib.SCALE_SIGNATURES
    assert sorted(protos) == sorted(sigs) == declared_symbols("beso_scale.h") and len(protos) == 3
    assert list(protos) == list(sigs) == list(_lib.SCALE_EXPORTS), "the table keeps the header's order"
    for fn, (ret, args) in protos.items():
        restype, argtypes = sigs[fn]
        assert len(argtypes) == len(args), f"{fn}: the header declares {len(args)} arguments, the table {len(argtypes)}"
        for i, (want, have) in enumerate(zip(args, argtypes)):
            assert _ctypes_class(have) == want, f"{fn}: argument {i} is {have!r} in the table, {want!r} in the header"
        assert _ctypes_class(restype) == ret, fn
    assert exported_symbols(_lib.SCALE_LIB_PATH) == sorted(protos)
    bound = _lib.load_scale()
    for fn in protos:
        assert len(getattr(bound, fn).argtypes) == len(sigs[fn][1])
    text = _header("beso_scale.h", keep_preprocessor=True)
    consts = {k: int(v) for k, v in re.findall(r"\b(BESO_SCALE_[A-Z_]+)\s*=?\s*(\d+)", text)}
    assert consts == {"BESO_SCALE_ZSCORE": _lib.SCALE_KINDS["zscore"], "BESO_SCALE_MINMAX": _lib.SCALE_KINDS["minmax"],
                      "BESO_SCALE_MAX_ITEMS": _lib.SCALE_LIMITS["max_items"]}


def test_product_library_exports_are_unchanged(lib):
    """libbeso_hip.so still exports exactly include/beso_hip.h -- 37 functions, none of libbeso_scale.so's."""
    have = exported_symbols(_lib.LIB_PATH)
    assert have == declared_symbols() == sorted(_lib.EXPORTS) and len(have) == 37
    assert not set(have) & set(_lib.SCALE_EXPORTS)


def test_scale_argument_errors_are_named_before_anything_is_enqueued(lib):
    """NULL pointers, zero items, five items, an unknown kind, a MINMAX item without p2 / p3, cols < 1 and act_dim < 1 come back
    as a status with a message that names the function and the argument; a refused call touches no device (this test has none)."""
    sc = _lib.load_scale()
    one = 0x1000
    tab = lambda n, v=one: (C.c_void_p * max(n, 1))(*[v] * max(n, 1))       # noqa: E731
    ints = lambda n, v: (C.c_int * max(n, 1))(*[v] * max(n, 1))            # noqa: E731
    longs = lambda n, v: (C.c_longlong * max(n, 1))(*[v] * max(n, 1))      # noqa: E731

    def rows_mixed(n=2, kinds=0, n_rows=3, n_cols=5, **k):
        a = dict(src=tab(n), dst=tab(n), kind=ints(n, kinds), p0=tab(n), p1=tab(n), p2=tab(n), p3=tab(n), rows=longs(n, n_rows),
                 cols=ints(n, n_cols))
        a.update(k)
        return sc.beso_scale_rows_mixed(a["src"], a["dst"], a["kind"], a["p0"], a["p1"], a["p2"], a["p3"], a["rows"], a["cols"], n, None)

    msg = lambda: sc.beso_scale_last_error().decode()                      # noqa: E731
    assert rows_mixed(n=0) == _lib.ERR_BAD_ARG and "n = 0" in msg() and "beso_scale_rows_mixed" in msg()
    assert rows_mixed(n=5) == _lib.ERR_BAD_ARG and "n = 5" in msg()
    for name in ("src", "dst", "kind", "p0", "p1", "rows", "cols"):
        assert rows_mixed(**{name: None}) == _lib.ERR_BAD_ARG and "NULL table" in msg(), name
    for name in ("src", "dst", "p0", "p1"):
        assert rows_mixed(**{name: tab(2, None)}) == _lib.ERR_BAD_ARG and "NULL pointer" in msg() and "tensor 0" in msg(), name
    assert rows_mixed(kinds=1, p2=None) == _lib.ERR_BAD_ARG and "p2 / p3 table" in msg()
    assert rows_mixed(kinds=1, p3=tab(2, None)) == _lib.ERR_BAD_ARG and "p2 / p3" in msg()
    assert rows_mixed(kinds=2) == _lib.ERR_BAD_ARG and "kind[0] = 2" in msg()
    assert rows_mixed(n_cols=0) == _lib.ERR_BAD_SHAPE and "cols at least 1" in msg()
    assert rows_mixed(n_rows=-1) == _lib.ERR_BAD_SHAPE
    assert rows_mixed(src=tab(2, one + 2)) == _lib.ERR_BAD_ARG and "aligned" in msg()
    assert rows_mixed(n_rows=0) == _lib.OK                                   # nothing to do: no launch
    assert rows_mixed(n_rows=0, p2=None, p3=None) == _lib.OK                 # ZSCORE items read no p2 / p3

    def end(**k):
        a = dict(x0=one, lengths=one, lo=one, hi=one, new_lo=one, span=one, range=one, lo_y=one, act_ctx=one, pred=one, n_envs=4,
                 window=3, act_dim=2)
        a.update(k)
        return sc.beso_rollout_end_minmax(*[a[n] for n in ("x0", "lengths", "lo", "hi", "new_lo", "span", "range", "lo_y", "act_ctx",
                                                           "pred", "n_envs", "window", "act_dim")], None)

    assert end(act_dim=0) == _lib.ERR_BAD_SHAPE and "act_dim = 0" in msg() and "beso_rollout_end_minmax" in msg()
    assert end(act_dim=-3) == _lib.ERR_BAD_SHAPE and end(window=0) == _lib.ERR_BAD_SHAPE and end(n_envs=-1) == _lib.ERR_BAD_SHAPE
    assert end(n_envs=1 << 20, window=1 << 10, act_dim=1 << 10) == _lib.ERR_BAD_SHAPE and "int range" in msg()
    for name in ("x0", "lengths", "lo", "hi", "act_ctx", "pred"):
        assert end(**{name: None}) == _lib.ERR_BAD_ARG and "NULL pointer" in msg(), name
    for name in ("new_lo", "span", "range", "lo_y"):
        assert end(**{name: None}) == _lib.ERR_BAD_ARG and "3 of 4" in msg(), name
    assert end(lo=one + 4) == _lib.ERR_BAD_ARG and "8-byte" in msg()
    assert end(n_envs=0) == _lib.OK
    assert end(n_envs=0, new_lo=None, span=None, range=None, lo_y=None) == _lib.OK
    with pytest.raises(ValueError, match="beso_rollout_end_minmax: act_dim = 0"):
        _lib.check_scale(end(act_dim=0), "rollout_end_minmax")
