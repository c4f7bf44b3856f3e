"""The MLP observation / goal encoder's kernels (include/beso_mlp.h, csrc/encoder.hip) and ``MLPNetwork`` on top of them.

Comparators: a torch ``nn.Linear`` stack built from the same weights on the CPU (forward: the project's fp32 bar, 2e-5 of
max |reference|), torch autograd in fp64 as arbiter of the gradients (the HIP error may be at most 4x the error of torch's own
fp32 autograd against fp64), and tests/autograd_reference.py behind a torch copy of the encoder for the path through the
denoiser (``TRAIN_BOUNDS``).  Every case prints what it measured."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn

from beso_amd import _lib
from beso_amd.networks.mlps.mlps import MLPNetwork
from oracle import beso_oracle as O
from support import (TRAIN_BOUNDS, bits, check_row_ranges_add_up, check_side_library, grad_errors, lib, make_denoiser,  # noqa: F401
                     raw_fwd_bwd)

DEV = "cuda:0"
# (in, hidden, hidden layers, out, M): M = 1, one below a multiple of the 16-row tile, one above one, a partial last tile
SHAPES = [(11, 16, 1, 7, 1), (11, 48, 2, 7, 33), (5, 16, 1, 3, 15), (30, 256, 3, 30, 200), (60, 512, 4, 30, 65)]
ACTS = {"ReLU": nn.ReLU, "Mish": nn.Mish, "sigmoid": nn.Sigmoid, "tanh": nn.Sigmoid}      # "tanh": networks/utils.py:37-38
FP32_BAR = 2e-5
EPS = 2.0 ** -24        # one fp32 rounding: a tensor torch's fp32 autograd gets exact by luck asks no more than that of the kernels


def torch_stack(net, dtype=torch.float32):
    """The reference's forward (mlps.py:54-66) over copies of `net`'s layers, on the CPU."""
    layers = [copy.deepcopy(l).to("cpu", dtype) for l in net.layers]
    mods = []
    for i, l in enumerate(layers):
        mods.append(l)
        if i < len(layers) - 1:
            mods.append(ACTS[net.activation]())
    return nn.Sequential(*mods)


def make_net(shape, act, seed=0, device=DEV):
    i, h, n, o, _ = shape
    torch.manual_seed(seed)
    return MLPNetwork(i, h, n, o, activation=act, device=device)


def rows(shape, seed=1, extra=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape[4] + extra, shape[0], generator=g)


# -------------------------------------------------------------------------------------------------
# CPU
# -------------------------------------------------------------------------------------------------
def test_library_exports_what_its_header_declares(lib):
    """libbeso_mlp.so: the symbols of include/beso_mlp.h, no more; the binding table has the header's argument counts; the
    struct has the header's fields; the matrix-pipe hazard check of DESIGN.md 4.1c passes on it."""
    import re
    text = check_side_library("beso_mlp.h", "beso_mlp_", _lib.MLP_SIGNATURES, _lib.MLP_LIB_PATH, _lib.load_mlp, 3, min_kernels=4)
    body = re.search(r"typedef\s+struct\s+beso_mlp_dims\s*\{(.*?)\}", text, flags=re.S).group(1)
    assert [f.split()[1] for f in body.split(";") if f.strip()] == [n for n, _ in _lib.MlpDims._fields_]
    consts = dict(re.findall(r"\b(BESO_MLP_[A-Z_]+)\s*=\s*(\d+)", text))
    assert {k: int(consts["BESO_MLP_ACT_" + k.upper()]) for k in ("ReLU", "Mish", "sigmoid")} == \
        {k: _lib.MLP_ACTIVATIONS[k] for k in ("ReLU", "Mish", "sigmoid")}
    assert _lib.MLP_ACTIVATIONS["tanh"] == _lib.MLP_ACTIVATIONS["sigmoid"]
    assert int(consts["BESO_MLP_ACCUMULATE"]) == _lib.MLP_FLAGS["accumulate"]


def test_argument_errors_do_not_touch_the_device(lib):
    """Dummy non-NULL pointers: a call that got past its checks would write through them."""
    mlp = _lib.load_mlp()
    one = C.c_void_p(16)
    arr = lambda n: (C.c_void_p * n)(*([16] * n))                                       # noqa: E731
    good = _lib.MlpDims(11, 48, 2, 7, 0)
    fwd = lambda d, n=6, M=4, x=one: mlp.beso_mlp_fwd(arr(n), n, C.byref(d), x, M, one, None, None)      # noqa: E731
    for bad in (_lib.MlpDims(0, 48, 2, 7, 0), _lib.MlpDims(513, 48, 2, 7, 0), _lib.MlpDims(11, 40, 2, 7, 0),
                _lib.MlpDims(11, 528, 2, 7, 0), _lib.MlpDims(11, 48, 0, 7, 0), _lib.MlpDims(11, 48, 5, 7, 0),
                _lib.MlpDims(11, 48, 2, 0, 0), _lib.MlpDims(11, 48, 2, 513, 0)):
        assert fwd(bad, n=2 * (bad.n_hidden + 1)) == _lib.ERR_BAD_SHAPE
        assert mlp.beso_mlp_workspace_bytes(C.byref(bad), 4, 1) == 0
    assert fwd(good, M=0) == _lib.ERR_BAD_SHAPE
    assert fwd(_lib.MlpDims(11, 48, 2, 7, 3)) == _lib.ERR_BAD_ARG                        # unknown activation
    assert fwd(good, n=4) == _lib.ERR_BAD_ARG and fwd(good, x=None) == _lib.ERR_BAD_ARG
    need = mlp.beso_mlp_workspace_bytes(C.byref(good), 33, 1)
    assert need >= 4 * (2 * 33 * 48 + 11 * 48 + 48 + 48 * 48 + 48 + 48 * 7 + 7)
    assert mlp.beso_mlp_workspace_bytes(C.byref(good), 33, 0) == 0
    bwd = lambda wsb, flags=0, ws=C.c_void_p(256): mlp.beso_mlp_bwd(arr(6), 6, C.byref(good), one, one, 33, None, one, ws, wsb,   # noqa: E731
                                                                  flags, None)
    assert bwd(need - 1) == _lib.ERR_WORKSPACE and bwd(need, ws=None) == _lib.ERR_WORKSPACE
    assert bwd(need, flags=2) == _lib.ERR_BAD_ARG
    with pytest.raises(_lib.BesoHipError):
        _lib.check(bwd(16), "beso_mlp_bwd")


def test_unsupported_dims_and_activations_raise_by_name():
    for kw, word in ((dict(input_dim=0), "input_dim"), (dict(input_dim=600), "input_dim"), (dict(hidden_dim=100), "hidden_dim"),
                     (dict(hidden_dim=1024), "hidden_dim"), (dict(num_hidden_layers=5), "num_hidden_layers"),
                     (dict(num_hidden_layers=0), "num_hidden_layers"), (dict(output_dim=513), "output_dim"),
                     (dict(activation="PReLU"), "PReLU"), (dict(activation="softmax"), "softmax"), (dict(activation="gelu"), "gelu")):
        args = dict(input_dim=11, hidden_dim=48, num_hidden_layers=2, output_dim=7, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            MLPNetwork(**args)
    net = MLPNetwork(11, 48, 2, 7, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(3, 11))


# -------------------------------------------------------------------------------------------------
# GPU
# -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("act", ["ReLU", "Mish", "sigmoid", "tanh"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_the_torch_stack(shape, act):
    net = make_net(shape, act)
    x = rows(shape)
    with torch.no_grad():
        ref = torch_stack(net)(x)
        got = net(x.to(DEV)).cpu()
        got3 = net(x.to(DEV).view(1, shape[4], shape[0])).cpu()                         # leading dimensions are kept
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"mlp fwd {shape} {act}: max err / max |ref| = {err:.3e}")
    assert got.shape == ref.shape and got3.shape == (1,) + tuple(ref.shape) and torch.equal(got3[0], got)
    assert err <= FP32_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["ReLU", "Mish", "sigmoid"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_matches_fp64_autograd_as_closely_as_torch_fp32_does(shape, act):
    """dW, db of every layer and dX against torch autograd in fp64; per tensor the HIP error may be at most 4x the error of
    torch's own fp32 autograd (CPU) against the same fp64 values -- the factor allows for another summation order over M --
    with both errors measured by ``grad_errors`` on TRAIN_BOUNDS["fp32"]'s floor and torch's error taken as at least one fp32
    rounding (2^-24).

    Measured on an MI355X, the largest ratio HIP error / max(torch fp32 error, 2^-24) over the tensors of a case (the same for
    ReLU, Mish and sigmoid to the digits shown, but for the first three shapes, where they range over 0.85 ... 1.92):
    (11,16,1,7,1) 1.18; (11,48,2,7,33) 1.50; (5,16,1,3,15) 1.92; (30,256,3,30,200) 3.48; (60,512,4,30,65) 2.49.
    Largest HIP error 8.5e-7, largest torch fp32 error 5.1e-7."""
    net = make_net(shape, act)
    x = rows(shape)
    g = torch.Generator().manual_seed(2)
    dy = torch.randn(shape[4], shape[3], generator=g)

    def torch_grads(dtype):
        stack = torch_stack(net, dtype)
        xi = x.detach().clone().to(dtype).requires_grad_(True)
        stack(xi).backward(dy.to(dtype))
        return [p.grad for p in stack.parameters()] + [xi.grad]

    ref = torch_grads(torch.float64)
    t32 = [v.double() for v in torch_grads(torch.float32)]
    xd = x.to(DEV).requires_grad_(True)
    net(xd).backward(dy.to(DEV))
    got = [p.grad.cpu().double() for p in net.parameters()] + [xd.grad.cpu().double()]
    floor = TRAIN_BOUNDS["fp32"][2]
    e_hip, e_t32 = grad_errors(got, ref, floor), grad_errors(t32, ref, floor)
    ratios = [h / max(t, EPS) for h, t in zip(e_hip, e_t32)]
    print(f"mlp bwd {shape} {act}: max HIP err {max(e_hip):.3e}, max torch fp32 err {max(e_t32):.3e}, max ratio {max(ratios):.2f}")
    for i, (h, t) in enumerate(zip(e_hip, e_t32)):
        assert h <= 4.0 * max(t, EPS), (i, h, t)
    # x that does not require grad: no dX is produced, the parameter gradients are the same bits
    before = [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    net(x.to(DEV)).backward(dy.to(DEV))
    assert all(torch.equal(bits(p.grad), bits(b)) for p, b in zip(net.parameters(), before))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES + [(5, 16, 1, 3, 300)], ids=lambda s: "x".join(map(str, s)))
def test_equal_bits_from_run_to_run_and_rows_are_independent(shape):
    net = make_net(shape, "Mish")
    x, dy = rows(shape, extra=17).to(DEV), torch.randn(shape[4], shape[3], generator=torch.Generator().manual_seed(2)).to(DEV)
    M = shape[4]
    a, b = raw_fwd_bwd(net, x[:M].contiguous(), dy), raw_fwd_bwd(net, x[:M].contiguous(), dy)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with torch.no_grad():
        small, big = net(x[:M].contiguous()), net(x)
    assert torch.equal(bits(small), bits(big[:M])) and torch.equal(bits(small).view(torch.uint8).reshape(-1), a["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 16, 1, 3, 300), (11, 48, 2, 7, 300)], ids=lambda s: "x".join(map(str, s)))
def test_row_ranges_add_up(shape):
    """M = 300 is two row ranges of the weight-gradient slabs with a partial last 16-row step (support.check_row_ranges_add_up);
    the second shape has hidden-to-hidden layers, whose input is the activation applied on load."""
    net = make_net(shape, "Mish")
    check_row_ranges_add_up(net, rows(shape).to(DEV), torch.randn(shape[4], shape[3], generator=torch.Generator().manual_seed(2)).to(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_results_do_not_depend_on_what_the_buffers_held(shape):
    """0xFF (NaN) and 0x7B (~1.3e36) fills of the output, keep, workspace and gradient buffers change no result bit; the
    sentinel bands around every buffer stay as they were (checked inside raw_fwd_bwd); BESO_MLP_ACCUMULATE adds to what the
    gradient buffer holds, in one addition per element."""
    net = make_net(shape, "sigmoid")
    x, dy = rows(shape).to(DEV), torch.randn(shape[4], shape[3], generator=torch.Generator().manual_seed(2)).to(DEV)
    base = raw_fwd_bwd(net, x, dy)
    for fill in (0xFF, 0x7B):
        got = raw_fwd_bwd(net, x, dy, fill=fill)
        for k in base:
            assert torch.equal(base[k], got[k]), (k, hex(fill))
    grads = base["grads"].view(torch.float32)
    with torch.no_grad():
        y, keep = net.run_forward(x, keep=True)
    flat = torch.full_like(grads, 0.25)
    net.run_backward(keep, dy, flat, accumulate=True)
    assert torch.equal(bits(flat), bits(grads + 0.25))
    net.run_backward(keep, dy, flat)
    assert torch.equal(bits(flat), bits(grads))
    ws = torch.empty(net.workspace_bytes(shape[4]) - 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.BesoHipError, match="status -4"):
        net.run_backward(keep, dy, flat, workspace=ws)


class TorchEncoder(nn.Module):
    """A torch copy of an MLPNetwork (the comparator's encoder), on the network's device."""

    def __init__(self, net):
        super().__init__()
        self.layers = copy.deepcopy(net.layers)
        self.act = ACTS[net.activation]()

    def forward(self, x):
        for i, l in enumerate(self.layers):
            x = l(x)
            if i < len(self.layers) - 1:
                x = self.act(x)
        return x


@pytest.mark.gpu
@pytest.mark.parametrize("goal_batch", ["B", "1"])
@pytest.mark.parametrize("t", [3, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encoder_gradients_through_the_denoiser(precision, t, goal_batch):
    """GCDenoiser.loss(enc(state), action, enc(goal), noise, sigma).backward(): the encoder's gradients against the torch-op
    evaluation (tests/autograd_reference.py over the same denoiser weights, behind a torch copy of the encoder) at
    TRAIN_BOUNDS[precision]; the denoiser's own gradients equal, bit for bit, those of the call on pre-encoded detached inputs."""
    from autograd_reference import loss_autograd
    cfg = O.TINY
    assert cfg.obs_dim == 7
    B = 5
    model = make_denoiser(cfg, precision=precision, train=True)
    model.deterministic_training = True            # fixed-order sums: the bit-for-bit comparison at the end needs them
    torch.manual_seed(3)
    enc = MLPNetwork(11, 48, 1, 7, device=DEV)
    ref_enc = TorchEncoder(enc)
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                  # noqa: E731
    state, goal = r(B, t, 11), r(B if goal_batch == "B" else 1, cfg.goal_seq_len, 11)
    action, noise = r(B, t, cfg.act_dim), r(B, t, cfg.act_dim)
    sigma = (torch.rand(B, generator=g) * 0.9 + 0.05).to(DEV)

    loss = model.loss(enc(state), action, enc(goal), noise.clone(), sigma)
    loss.backward()
    got = [p.grad.clone() for p in enc.parameters()]
    den = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)

    ref_loss = loss_autograd(model, ref_enc(state), action, ref_enc(goal), noise.clone(), sigma)
    ref_loss.backward()
    ref = [p.grad for p in ref_enc.parameters()]
    model.zero_grad(set_to_none=True)
    loss_bound, grad_bound, floor = TRAIN_BOUNDS[precision]
    lerr = abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())
    errs = grad_errors(got, ref, floor)
    print(f"encoder through the denoiser {precision} t={t} goal [{goal_batch},G,.]: loss err {lerr:.3e}, max grad err {max(errs):.3e}")
    assert lerr <= loss_bound and max(errs) <= grad_bound, (lerr, errs)

    with torch.no_grad():
        se, ge = enc(state), enc(goal)
    model.loss(se, action, ge, noise.clone(), sigma).backward()
    assert all(torch.equal(bits(p.grad), bits(d)) for p, d in zip(model.parameters(), den))
