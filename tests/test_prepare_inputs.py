"""runtime.prepare_inputs and its neighbours on CPU tensors: the one place that turns what callers pass (any float dtype, any
strides, goals without a batch dimension, a scalar sigma) into the contiguous fp32 tensors the library reads."""
import pytest
import torch

from beso_amd import _lib
from beso_amd.runtime import prepare_inputs, train_precision, workspace

B, T, G, OBS, ACT = 2, 3, 2, 7, 3


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, OBS, generator=g), torch.randn(B, T, ACT, generator=g), torch.randn(G, OBS, generator=g),
            torch.rand(B, generator=g) + 0.1)


def _prep(state, action, goal, sigma, goal_seq_len=G):
    return prepare_inputs(state, action, goal, sigma, OBS, ACT, goal_seq_len)


def _is_plain(x, shape):
    return x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == shape


def test_goal_of_every_accepted_rank_comes_out_batched():
    state, action, goal, sigma = _inputs()
    want = goal.unsqueeze(0).expand(B, G, OBS)
    for given in (goal, goal.unsqueeze(0), want.contiguous(), want):
        s, a, g, sg = _prep(state, action, given, sigma)
        assert _is_plain(g, (B, G, OBS)) and torch.equal(g, want)
        assert _is_plain(s, (B, T, OBS)) and _is_plain(a, (B, T, ACT)) and torch.equal(s, state) and torch.equal(a, action)
    own = torch.randn(B, G, OBS)                                  # one goal per sample stays what it is
    assert torch.equal(_prep(state, action, own, sigma)[2], own)


def test_sigma_of_every_accepted_shape_comes_out_per_sample():
    state, action, goal, sigma = _inputs()
    for given, want in ((torch.tensor(0.3), torch.full((B,), 0.3)), (torch.tensor([0.3]), torch.full((B,), 0.3)), (sigma, sigma),
                        (sigma.reshape(B, 1), sigma)):
        got = _prep(state, action, goal, given)[3]
        assert _is_plain(got, (B,)) and torch.equal(got, want)
    assert _prep(state, action, goal, None)[3] is None
    one = _prep(state[:1], action[:1], goal, torch.tensor(0.3))[3]
    assert _is_plain(one, (1,))


def test_other_dtypes_and_strides_come_out_fp32_contiguous():
    state, action, goal, sigma = _inputs()
    wide = torch.randn(B, T, 2 * OBS, dtype=torch.float64)
    strided = wide[:, :, ::2]                                     # float64 and not contiguous
    assert not strided.is_contiguous()
    act_t = action.transpose(0, 1).contiguous().transpose(0, 1)   # [B,T,ACT] with the strides of [T,B,ACT]
    assert not act_t.is_contiguous()
    s, a, g, sg = _prep(strided, act_t, goal.double(), sigma.double())
    assert _is_plain(s, (B, T, OBS)) and torch.equal(s, strided.float())
    assert _is_plain(a, (B, T, ACT)) and torch.equal(a, action)
    assert _is_plain(g, (B, G, OBS)) and _is_plain(sg, (B,)) and torch.equal(sg, sigma)
    half = _prep(state.half(), action.bfloat16(), goal, sigma)
    assert _is_plain(half[0], (B, T, OBS)) and _is_plain(half[1], (B, T, ACT))
    # what already is plain is passed through, not copied
    s, a, _, sg = _prep(state, action, goal, sigma)
    assert s.data_ptr() == state.data_ptr() and a.data_ptr() == action.data_ptr() and sg.data_ptr() == sigma.data_ptr()


def test_no_goal_tokens_means_no_goal_whatever_was_passed():
    state, action, goal, sigma = _inputs()
    for given in (None, goal, torch.zeros(5), "not a tensor"):
        assert _prep(state, action, given, sigma, goal_seq_len=0)[2] is None


@pytest.mark.parametrize("what,change", [
    ("state feature dim", lambda s, a, g, sg: (s[:, :, :OBS - 1], a, g, sg)),
    ("action feature dim", lambda s, a, g, sg: (s, a[:, :, :ACT - 1], g, sg)),
    ("t", lambda s, a, g, sg: (s, a[:, :T - 1], g, sg)),
    ("batch", lambda s, a, g, sg: (s, torch.cat([a, a]), g, sg)),
    ("state rank", lambda s, a, g, sg: (s[0], a, g, sg)),
    ("action rank", lambda s, a, g, sg: (s, a[0], g, sg)),
    ("goal length", lambda s, a, g, sg: (s, a, g[:1], sg)),
    ("goal feature dim", lambda s, a, g, sg: (s, a, g[:, :OBS - 1], sg)),
    ("goal batch", lambda s, a, g, sg: (s, a, g.expand(B + 1, G, OBS), sg)),
    ("goal rank 1", lambda s, a, g, sg: (s, a, g[0], sg)),
    ("goal rank 4", lambda s, a, g, sg: (s, a, g[None, None], sg)),
    ("sigma count", lambda s, a, g, sg: (s, a, g, torch.ones(B + 1))),
    ("missing goal", lambda s, a, g, sg: (s, a, None, sg)),
])
def test_shape_errors_are_value_errors(what, change):
    with pytest.raises(ValueError):
        _prep(*change(*_inputs()))


def test_training_precision_of_every_model_precision():
    """The split-bf16 and fp16 modes are inference instances: their training steps are the fp32 / bf16 ones."""
    assert {k: train_precision(k) for k in _lib.PRECISIONS} == {"bf16": _lib.PREC_BF16, "fp32": _lib.PREC_FP32,
                                                                "bf16x3": _lib.PREC_FP32, "fp16": _lib.PREC_BF16}
    with pytest.raises(KeyError):
        train_precision("fp8")


def test_workspace_only_grows():
    class Owner:
        _ws = None
    o, cpu = Owner(), torch.device("cpu")
    a = workspace(o, 100, cpu)
    assert a is o._ws and a.dtype == torch.uint8 and a.numel() == 100
    assert workspace(o, 40, cpu) is a and workspace(o, 100, cpu) is a           # fits: kept
    b = workspace(o, 101, cpu)
    assert b is o._ws and b is not a and b.numel() == 101                       # does not fit: a new one
    assert workspace(o, 1, torch.device("meta")).device.type == "meta"         # another device: a new one
