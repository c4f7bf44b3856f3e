"""The residual MLP encoder's kernels (include/beso_resmlp.h, csrc/resmlp.hip) and ``ResidualMLPNetwork`` on top of them.

Comparators: tests/golden/resmlp_reference.npz -- the reference's own ``ResidualMLPNetwork`` on the CPU (make_resmlp_fixtures.py)
-- and a torch re-statement of the network (``Restated``) over copies of the module's parameters.  Forward: the project's fp32
bar, 2e-5 of max |reference|.  Gradients: torch autograd in fp64 over the re-statement is the arbiter; per tensor the HIP error
may be at most 4x the error of fp32 torch against the same fp64 values (the factor allows for another summation order over M),
both measured by ``grad_errors`` on TRAIN_BOUNDS["fp32"]'s floor, torch's error taken as at least one fp32 rounding.  Every case
prints what it measured."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from beso_amd import _lib
from beso_amd.networks.mlps.mlps import ResidualMLPNetwork
from support import TRAIN_BOUNDS, bits, check_row_ranges_add_up, check_side_library, grad_errors, lib, raw_fwd_bwd  # noqa: F401

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = {"ReLU": nn.ReLU, "Mish": nn.Mish, "sigmoid": nn.Sigmoid, "tanh": nn.Sigmoid}      # "tanh": networks/utils.py:37-38
FP32_BAR = 2e-5
EPS = 2.0 ** -24        # one fp32 rounding
FIXTURE_CASES = {"mish_layernorm": dict(input_dim=11, hidden_dim=48, num_hidden_layers=4, output_dim=7, activation="Mish",
                                        use_norm=True, norm_style="LayerNorm"),
                 "relu_plain": dict(input_dim=11, hidden_dim=48, num_hidden_layers=2, output_dim=7, activation="ReLU")}
# (in, hidden, num_hidden_layers, out, M, activation, LayerNorm).  M: 1, a full tile, one row above it, a partial third tile,
# two row ranges of the weight-gradient slabs (300 > 256).  in / out 1 and 11 / 7 take the scalar weight loads, 512 the vector
# ones; hidden 512 with in = out = 512 is the LDS maximum (three 16 x 516 tiles); in, out > hidden sets the pitch by them.
SWEEP = [(1, 16, 2, 1, 1, "ReLU", False), (1, 16, 2, 1, 17, "Mish", True), (11, 48, 2, 7, 16, "sigmoid", True),
         (11, 48, 8, 7, 33, "Mish", True), (11, 48, 8, 7, 300, "ReLU", False), (11, 48, 2, 7, 300, "Mish", True),
         (512, 512, 2, 512, 17, "Mish", True), (512, 512, 8, 512, 33, "ReLU", False), (11, 512, 2, 7, 1, "sigmoid", False),
         (512, 16, 2, 512, 16, "ReLU", True), (1, 48, 8, 1, 300, "sigmoid", True), (11, 16, 2, 7, 33, "Mish", False)]
case_id = lambda s: "x".join(map(str, s))                                                # noqa: E731


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resmlp_reference.npz"))


class Restated(nn.Module):
    """The network in torch ops over copies of `net`'s parameters.  ``tied=False`` gives every block a second, separate
    LayerNorm with the same values for its second use (``norm2``)."""

    def __init__(self, net, dtype=torch.float32, device="cpu", tied=True):
        super().__init__()
        self.layers = copy.deepcopy(net.layers).to(device, dtype)
        self.act = ACTS[net.activation]()
        self.norm2 = None
        if net.use_norm and not tied:
            self.norm2 = nn.ModuleList([copy.deepcopy(blk.normalizer) for blk in self.layers[1:-1]])

    def forward(self, x):
        x = self.layers[0](x)
        for i, blk in enumerate(self.layers[1:-1]):
            n1 = blk.normalizer if blk.use_norm else (lambda t: t)
            n2 = self.norm2[i] if self.norm2 is not None else n1
            x = blk.l2(self.act(n2(blk.l1(self.act(n1(x)))))) + x
        return self.layers[-1](x)


def make_net(case, seed=0, device=DEV):
    i, h, n, o, _, act, norm = case
    torch.manual_seed(seed)
    net = ResidualMLPNetwork(i, h, n, o, activation=act, use_norm=norm, norm_style="LayerNorm", device=device)
    with torch.no_grad():
        for key, p in net.named_parameters():
            if ".normalizer." in key:                  # off 1 and 0: gamma and beta take part visibly
                p.add_(0.2 * torch.randn(p.shape, generator=torch.Generator().manual_seed(seed + 9)).to(p.device))
    return net


def rows(case, seed=1, extra=0):
    return torch.randn(case[4] + extra, case[0], generator=torch.Generator().manual_seed(seed))


def cotangent(case, extra=0):
    return torch.randn(case[4] + extra, case[3], generator=torch.Generator().manual_seed(2))


def compare_grads(tag, got, t32, ref):
    floor = TRAIN_BOUNDS["fp32"][2]
    e_hip, e_t32 = grad_errors(got, ref, floor), grad_errors(t32, ref, floor)
    ratios = [h / max(t, EPS) for h, t in zip(e_hip, e_t32)]
    print(f"{tag}: max HIP err {max(e_hip):.3e}, max torch fp32 err {max(e_t32):.3e}, max ratio {max(ratios):.2f}")
    for i, (h, t) in enumerate(zip(e_hip, e_t32)):
        assert h <= 4.0 * max(t, EPS), (tag, i, h, t)


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_library_exports_what_its_header_declares(lib):
    """libbeso_resmlp.so: the three symbols of include/beso_resmlp.h, no more; the binding table has the header's argument
    counts; the struct has the header's fields; the matrix-pipe hazard check of DESIGN.md 4.1c passes on it."""
    text = check_side_library("beso_resmlp.h", "beso_resmlp_", _lib.RESMLP_SIGNATURES, _lib.RESMLP_LIB_PATH, _lib.load_resmlp, 3,
                              min_kernels=4)
    body = re.search(r"typedef\s+struct\s+beso_resmlp_dims\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert [f.split()[1] for f in body.split(";") if f.strip()] == [n for n, _ in _lib.ResMlpDims._fields_]
    consts = dict(re.findall(r"\b(BESO_RESMLP_[A-Z_]+)\s*=\s*(\d+)", text))
    assert {"none": int(consts["BESO_RESMLP_NORM_NONE"]), "LayerNorm": int(consts["BESO_RESMLP_NORM_LAYER"])} == _lib.RESMLP_NORMS


def test_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers: a call that got past its checks would write through them."""
    res = _lib.load_resmlp()
    D = _lib.ResMlpDims
    one = C.c_void_p(16)
    arr = lambda n: (C.c_void_p * n)(*([16] * n))                                       # noqa: E731
    n_of = lambda d: 4 + (6 if d.norm else 4) * d.n_blocks                              # noqa: E731
    good, plain = D(11, 48, 2, 7, 1, 1), D(11, 48, 2, 7, 0, 0)
    fwd = lambda d, n=None, M=4, x=one: res.beso_resmlp_fwd(arr(n or n_of(d)), n or n_of(d), C.byref(d), x, M, one, None, None)  # noqa: E731
    for bad in (D(0, 48, 2, 7, 0, 1), D(513, 48, 2, 7, 0, 1), D(11, 40, 2, 7, 0, 1), D(11, 0, 2, 7, 0, 1), D(11, 528, 2, 7, 0, 1),
                D(11, 48, 0, 7, 0, 1), D(11, 48, 5, 7, 0, 1), D(11, 48, 2, 0, 0, 1), D(11, 48, 2, 513, 0, 1)):
        assert fwd(bad, n=n_of(bad) if bad.n_blocks else 4) == _lib.ERR_BAD_SHAPE
        assert res.beso_resmlp_workspace_bytes(C.byref(bad), 4, 1) == 0
    assert fwd(good, M=0) == _lib.ERR_BAD_SHAPE and fwd(good, M=-3) == _lib.ERR_BAD_SHAPE
    assert fwd(D(11, 48, 2, 7, 3, 1), n=16) == _lib.ERR_BAD_ARG                          # unknown activation
    assert fwd(D(11, 48, 2, 7, 0, 2), n=16) == _lib.ERR_BAD_ARG                          # unknown norm
    assert fwd(good, n=12) == _lib.ERR_BAD_ARG and fwd(plain, n=16) == _lib.ERR_BAD_ARG  # the other norm setting's count
    assert fwd(good, x=None) == _lib.ERR_BAD_ARG
    assert res.beso_resmlp_fwd(None, 16, C.byref(good), one, 4, one, None, None) == _lib.ERR_BAD_ARG
    M, H = 33, 48
    P = 11 * H + H + 2 * (2 * (H * H + H) + 2 * H) + 7 * H + 7
    need = res.beso_resmlp_workspace_bytes(C.byref(good), M, 1)
    assert need >= 4 * ((1 + 6 * 2) * M * H + P)
    assert res.beso_resmlp_workspace_bytes(C.byref(plain), M, 1) >= 4 * ((1 + 4 * 2) * M * H + P - 2 * 2 * H)
    assert res.beso_resmlp_workspace_bytes(C.byref(good), M, 0) == 0 and res.beso_resmlp_workspace_bytes(C.byref(good), 0, 1) == 0
    bwd = lambda wsb, flags=0, ws=C.c_void_p(256), n=16: res.beso_resmlp_bwd(arr(n), n, C.byref(good), one, one, M, None, one,  # noqa: E731
                                                                             ws, wsb, flags, None)
    assert bwd(need - 1) == _lib.ERR_WORKSPACE and bwd(need, ws=None) == _lib.ERR_WORKSPACE and bwd(0) == _lib.ERR_WORKSPACE
    assert bwd(need, ws=C.c_void_p(260)) == _lib.ERR_WORKSPACE                           # not 16-byte aligned
    assert bwd(need, flags=2) == _lib.ERR_BAD_ARG and bwd(need, n=12) == _lib.ERR_BAD_ARG
    with pytest.raises(_lib.BesoHipError):
        _lib.check(bwd(16), "beso_resmlp_bwd")


def test_refusals_raise_by_name():
    base = dict(input_dim=11, hidden_dim=48, num_hidden_layers=2, output_dim=7, device="cpu")
    for kw, word in ((dict(input_dim=0), "input_dim"), (dict(input_dim=600), "input_dim"), (dict(hidden_dim=100), "hidden_dim"),
                     (dict(hidden_dim=1024), "hidden_dim"), (dict(num_hidden_layers=10), "num_hidden_layers"),
                     (dict(num_hidden_layers=0), "num_hidden_layers"), (dict(output_dim=513), "output_dim"),
                     (dict(output_dim=0), "output_dim"), (dict(activation="PReLU"), "PReLU"), (dict(activation="softmax"), "softmax"),
                     (dict(activation="gelu"), "gelu"), (dict(use_norm=True), "BatchNorm"),
                     (dict(use_norm=True, norm_style="BatchNorm"), "BatchNorm"), (dict(use_spectral_norm=True), "use_spectral_norm"),
                     (dict(use_norm=True, norm_style="GroupNorm"), "not a defined norm type")):
        with pytest.raises(ValueError, match=word):
            ResidualMLPNetwork(**{**base, **kw})
    for odd in (1, 3, 7):
        with pytest.raises(AssertionError):
            ResidualMLPNetwork(**{**base, "num_hidden_layers": odd})
    with pytest.raises(AssertionError):                                   # the reference's default num_hidden_layers is 1
        ResidualMLPNetwork(11, device="cpu")
    ResidualMLPNetwork(**base, norm_style="BatchNorm")                    # the default style, unused without use_norm
    net = ResidualMLPNetwork(**base, dropout=0.25)                        # accepted; no training-mode forward
    assert net.dropout == 0.25 and net.training
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(3, 11))
    with pytest.raises(NotImplementedError, match="dropout"):
        net.run_forward(torch.zeros(3, 11), keep=True)


@pytest.mark.parametrize("name", list(FIXTURE_CASES))
def test_state_dict_is_the_references(golden, name):
    """Keys and shapes of state_dict() / named_parameters() / get_params() in the fixture's order; its weights load."""
    net = ResidualMLPNetwork(**FIXTURE_CASES[name], device="cpu")
    keys = [str(k) for k in golden[f"{name}::keys"]]
    want = [(k, golden[f"{name}::w::{k}"].shape) for k in keys]
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    assert [(k, tuple(v.shape)) for k, v in net.named_parameters()] == want
    assert [tuple(p.shape) for p in net.get_params()] == [s for _, s in want]
    assert keys[:2] == ["layers.0.weight", "layers.0.bias"] and keys[2] == "layers.1.l1.weight"
    if name == "mish_layernorm":
        assert keys[6:8] == ["layers.1.normalizer.weight", "layers.1.normalizer.bias"] and keys[-1] == "layers.3.bias"
    result = net.load_state_dict({k: torch.from_numpy(golden[f"{name}::w::{k}"].copy()) for k in keys})
    assert not result.missing_keys and not result.unexpected_keys
    kw = FIXTURE_CASES[name]
    blocks = kw["num_hidden_layers"] // 2
    assert net.network_type == "mlp" and net.num_param_floats() == sum(int(np.prod(s)) for _, s in want)
    assert net.keep_floats(10) == 10 * (11 + (2 * blocks + 1) * 48)
    d = net.dims()
    assert (d.in_dim, d.hidden_dim, d.n_blocks, d.out_dim, d.activation, d.norm) == \
        (11, 48, blocks, 7, _lib.MLP_ACTIVATIONS[kw["activation"]], int(kw.get("use_norm", False)))


# -------------------------------------------------------------------------------------------------
# GPU
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURE_CASES))
def test_forward_and_gradients_match_the_reference_fixture(golden, name):
    """The reference's own output and ``y.pow(2).mean()`` gradients.  The fixture's fp32 gradients also stand in for "torch's
    own fp32 error" against the fp64 re-statement, which ties the re-statement to the reference."""
    net = ResidualMLPNetwork(**FIXTURE_CASES[name], device=DEV)
    keys = [str(k) for k in golden[f"{name}::keys"]]
    net.load_state_dict({k: torch.from_numpy(golden[f"{name}::w::{k}"].copy()) for k in keys})
    x, y_ref = torch.from_numpy(golden[f"{name}::x"].copy()), torch.from_numpy(golden[f"{name}::y"].copy())
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    err = ((y.detach().cpu() - y_ref).abs().max() / y_ref.abs().max()).item()
    print(f"resmlp fixture {name}: forward max err / max |ref| = {err:.3e}")
    assert y.shape == y_ref.shape and err <= FP32_BAR
    y.pow(2).mean().backward()
    got = [p.grad.cpu().double() for p in net.parameters()] + [xd.grad.cpu().double()]
    fix = [torch.from_numpy(golden[f"{name}::g::{k}"].copy()).double() for k in keys] + [torch.from_numpy(golden[f"{name}::dx"].copy()).double()]
    r64 = Restated(net, torch.float64)
    x64 = x.double().requires_grad_(True)
    r64(x64).pow(2).mean().backward()
    ref = [p.grad for p in r64.parameters()] + [x64.grad]
    assert max(grad_errors(fix, ref, TRAIN_BOUNDS["fp32"][2])) < 1e-5        # the re-statement IS the reference's network
    compare_grads(f"resmlp fixture {name} gradients", got, fix, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_sweep_against_the_restatement(case):
    """Forward and every gradient of a case against the re-statement (the module docstring's bars).

    Measured on an MI355X over the twelve cases: forward <= 8.6e-7 of max |reference|; largest ratio HIP error / max(torch fp32
    error, 2^-24) per case 1.02 ... 2.72 (the 2.72: (512, 16, 2, 512), M = 16, ReLU, LayerNorm); largest HIP error 1.8e-6 where
    torch's own is 2.3e-6 ((1, 48, 8, 1), M = 300, sigmoid, LayerNorm).  With the rows of a weight-gradient range summed
    sequentially, (11, 48, 8, 7), M = 300, ReLU missed the bar on the last bias (4.22x: a 256-term fp32 sum against torch's
    pairwise one); the kernel sums in chunks of 32 rows since (2.11x)."""
    net = make_net(case)
    x, dy = rows(case), cotangent(case)
    with torch.no_grad():
        ref_y = Restated(net)(x)
        got_y = net(x.to(DEV)).cpu()
        got3 = net(x.to(DEV).view(1, case[4], case[0])).cpu()                           # leading dimensions are kept
    err = ((got_y - ref_y).abs().max() / ref_y.abs().max()).item()
    print(f"resmlp fwd {case}: max err / max |ref| = {err:.3e}")
    assert got_y.shape == ref_y.shape and got3.shape == (1,) + tuple(ref_y.shape) and torch.equal(got3[0], got_y)
    assert err <= FP32_BAR

    def torch_grads(dtype):
        r = Restated(net, dtype)
        xi = x.detach().clone().to(dtype).requires_grad_(True)
        r(xi).backward(dy.to(dtype))
        return [p.grad for p in r.parameters()] + [xi.grad]

    ref = torch_grads(torch.float64)
    t32 = [v.double() for v in torch_grads(torch.float32)]
    xd = x.to(DEV).requires_grad_(True)
    net(xd).backward(dy.to(DEV))
    got = [p.grad.cpu().double() for p in net.parameters()] + [xd.grad.cpu().double()]
    compare_grads(f"resmlp bwd {case}", got, t32, ref)
    # x that does not require grad: no dX is produced, the parameter gradients are the same bits
    before = [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    net(x.to(DEV)).backward(dy.to(DEV))
    assert all(torch.equal(bits(p.grad), bits(b)) for p, b in zip(net.parameters(), before))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(11, 48, 4, 7, 33, "Mish", True), (11, 16, 2, 7, 300, "sigmoid", True)], ids=case_id)
def test_shared_normalizer_gradient_is_the_sum_of_both_uses(case):
    """gamma / beta of a block against a comparator with TWO LayerNorms per block holding the same values: their gradients
    added (fp64) are the arbiter, the same sums in fp32 torch give the allowed error."""
    net = make_net(case)
    x, dy = rows(case), cotangent(case)

    def two_norm_grads(dtype):
        r = Restated(net, dtype, tied=False)
        r(x.to(dtype)).backward(dy.to(dtype))
        out = []
        for blk, n2 in zip(r.layers[1:-1], r.norm2):
            assert blk.normalizer.weight.grad.abs().max() > 0 and n2.weight.grad.abs().max() > 0      # both uses contribute
            out += [blk.normalizer.weight.grad + n2.weight.grad, blk.normalizer.bias.grad + n2.bias.grad]
        return out

    ref = two_norm_grads(torch.float64)
    t32 = [v.double() for v in two_norm_grads(torch.float32)]
    net(x.to(DEV)).backward(dy.to(DEV))
    got = [p.grad.cpu().double() for k, p in net.named_parameters() if ".normalizer." in k]
    assert len(got) == len(ref) == case[2]
    compare_grads(f"resmlp shared normalizer {case}", got, t32, ref)


BIT_CASES = [(11, 48, 4, 7, 33, "Mish", True), (5, 16, 2, 3, 300, "ReLU", False), (60, 512, 8, 30, 65, "sigmoid", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_equal_bits_from_run_to_run_and_rows_are_independent(case):
    net = make_net(case)
    M = case[4]
    x, dy = rows(case, extra=17).to(DEV), cotangent(case, extra=17).to(DEV)
    a, b = raw_fwd_bwd(net, x[:M].contiguous(), dy[:M].contiguous()), raw_fwd_bwd(net, x[:M].contiguous(), dy[:M].contiguous())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    longer = raw_fwd_bwd(net, x, dy)                                  # M + 17 rows: y and dx of the first M are the same bits
    for k, width in (("y", net.output_dim), ("dx", net.input_dim)):
        assert torch.equal(longer[k][:4 * M * width], a[k]), k
    with torch.no_grad():
        small = net(x[:M].contiguous())
    assert torch.equal(bits(small).view(torch.uint8).reshape(-1), a["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(5, 16, 2, 3, 300, "ReLU", False), (11, 48, 4, 7, 300, "Mish", True)], ids=case_id)
def test_row_ranges_add_up(case):
    """M = 300 is two row ranges of the weight-gradient slabs, the second one full chunk of 32 rows and a partial one
    (support.check_row_ranges_add_up); the second case has the bias-only gamma / beta layers."""
    check_row_ranges_add_up(make_net(case), rows(case).to(DEV), cotangent(case).to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("case", BIT_CASES[:2], ids=case_id)
def test_results_do_not_depend_on_what_the_buffers_held(case):
    """0x00, 0xFF (NaN) and 0x7B (~1.3e36) fills of the output, keep, workspace and gradient buffers change no result bit; the
    sentinel bands around every buffer stay as they were (checked inside raw_fwd_bwd); BESO_MLP_ACCUMULATE adds to what the
    gradient buffer holds, in one addition per element."""
    net = make_net(case)
    x, dy = rows(case).to(DEV), cotangent(case).to(DEV)
    base = raw_fwd_bwd(net, x, dy)
    for fill in (0x00, 0xFF, 0x7B):
        got = raw_fwd_bwd(net, x, dy, fill=fill)
        for k in base:
            assert torch.equal(base[k], got[k]), (k, hex(fill))
    grads = base["grads"].view(torch.float32)
    assert bool(torch.isfinite(grads).all()) and grads.abs().max() > 0
    with torch.no_grad():
        y, keep = net.run_forward(x, keep=True)
    flat = torch.full_like(grads, 0.25)
    net.run_backward(keep, dy, flat, accumulate=True)
    assert torch.equal(bits(flat), bits(grads + 0.25))
    net.run_backward(keep, dy, flat)
    assert torch.equal(bits(flat), bits(grads))
    ws = torch.empty(net.workspace_bytes(case[4]) - 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BesoHipError, match="status -4"):
        net.run_backward(keep, dy, flat, workspace=ws)


@pytest.mark.gpu
def test_dropout_is_the_identity_in_eval_and_refused_in_a_training_call():
    case = (11, 48, 2, 7, 33, "Mish", True)
    plain = make_net(case)
    torch.manual_seed(0)
    net = ResidualMLPNetwork(11, 48, 2, 7, dropout=0.3, activation="Mish", use_norm=True, norm_style="LayerNorm", device=DEV)
    net.load_state_dict(plain.state_dict())
    x = rows(case).to(DEV)
    with pytest.raises(NotImplementedError, match="dropout"):
        net(x)
    with torch.no_grad():
        assert torch.equal(bits(net(x)), bits(plain(x)))              # under no_grad, even in training mode
    net.eval()
    y = net(x)                                                        # eval(): differentiable, dropout is the identity
    y.sum().backward()
    plain(x).sum().backward()
    assert torch.equal(bits(y), bits(plain(x)))
    assert all(torch.equal(bits(p.grad), bits(q.grad)) for p, q in zip(net.parameters(), plain.parameters()))
