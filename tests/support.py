"""What the test modules share beside conftest.py (fixtures, golden loaders) and autograd_reference.py (the comparator):
how a model under test is built, how its inputs are drawn and how an error is measured.  Imported as ``from support import ...``."""
import ctypes as C
import functools
import socket

import numpy as np
import pytest
import torch

DEV = "cuda:0"
TRAIN_BOUNDS = {"fp32": (2e-5, 1e-4, 1e-4), "bf16": (2e-3, 2.6e-2, 2e-3)}       # loss, per-tensor gradient, floor


def load_lib():
    """The product library, built from this tree if it is not current."""
    from beso_amd import _lib
    from beso_amd.build import build
    build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def load_weights(m, w):
    """Copies the numpy arrays of `w` into the module's state_dict."""
    sd = m.state_dict()
    for k, v in w.items():
        assert k in sd, k
        sd[k] = torch.from_numpy(v.copy())
    m.load_state_dict(sd)


def make_denoiser(cfg, w=None, precision="fp32", *, device=DEV, train=False, embed_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0,
                  goal_drop=0.0):
    """GCDenoiser around the DiffusionGPT of `cfg` on `device`, in train or eval mode.  `w` (numpy arrays by state_dict key)
    replaces the module's own initialisation; precision=None is the product's default."""
    from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT
    from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser
    inner = functools.partial(
        DiffusionGPT, state_dim=cfg.obs_dim, device=device, goal_conditioned=cfg.goal_conditioned,
        action_dim=cfg.act_dim, embed_dim=cfg.embed_dim, embed_pdrob=embed_pdrop, attn_pdrop=attn_pdrop,
        resid_pdrop=resid_pdrop, n_layers=cfg.n_layers, n_heads=cfg.n_heads, goal_seq_len=cfg.goal_seq_len,
        obs_seq_len=cfg.obs_seq_len, sigma_vocab_size=3, time_embedding_fn=None, goal_drop=goal_drop,
        linear_output=cfg.linear_output, precision=precision)
    m = GCDenoiser(inner, sigma_data=cfg.sigma_data)
    if w is not None:
        load_weights(m, w)
    return m.to(device).train(train)


def build_agent(cfg, model_factory, device="cpu", sampler="ddim", lr=1e-4, **extra):
    """The measurement tools' BesoAgent (tools/_agent.py) around `model_factory`, on the CPU unless told otherwise; `extra`
    goes to BesoAgent."""
    from tools._agent import build_agent as build
    return build(cfg, model_factory, device=device, sampler=sampler, lr=lr, **extra)


def to_dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def train_inputs(cfg, B, t=None, seed=0, device=DEV):
    """[state, action, goal [B, G, obs] (one goal per sample: the kernel draws the embedding mask per sample row), noise,
    sigma] for a window of t steps (None: cfg.obs_seq_len), drawn from the CPU generator in that order."""
    t = cfg.obs_seq_len if t is None else t
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(device)                   # noqa: E731
    return [r(B, t, cfg.obs_dim), r(B, t, cfg.act_dim), r(B, cfg.goal_seq_len, cfg.obs_dim), r(B, t, cfg.act_dim),
            (torch.rand(B, generator=g) * 0.9 + 0.05).to(device)]


def grad_errors(got, ref, floor=1e-4):
    """per tensor ||got - ref|| / max(||ref||, floor): tensors whose exact gradient is zero (key.bias: softmax is
    invariant to a shift of all scores of a row -- what is left is the rounding noise of the summands) are measured
    against `floor` times the largest gradient entry times sqrt(numel)"""
    gmax = max(r.abs().max().item() for r in ref)
    return [((g - r).norm() / max(r.norm().item(), floor * gmax * r.numel() ** 0.5)).item() for g, r in zip(got, ref)]


def bits(x):
    return x.contiguous().view(torch.int32)


def check_side_library(header, prefix, signatures, lib_path, loader, n_functions, min_kernels, min_mfma=21):
    """A library beside the product library exports the `n_functions` symbols ``<prefix>*`` its header under include/ declares,
    no more; the binding table `signatures` has the header's argument counts, and so has what `loader()` bound; the matrix-pipe
    hazard check of DESIGN.md 4.1c passes on it.  -> the header's text without its comments."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", header)).read(), flags=re.S)
    protos = {fn: args.split(",") for fn, args in re.findall(r"\b(%s[a-z_]+)\s*\(([^()]*)\)\s*;" % prefix, text)}
    assert sorted(protos) == sorted(signatures) and len(protos) == n_functions
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("beso_")) == sorted(protos)
    bound = loader()
    for fn, args in protos.items():
        assert len(signatures[fn][1]) == len(args) == len(getattr(bound, fn).argtypes), fn
    sys.path.insert(0, os.path.join(root, "tools"))
    import check_mfma_chains as chk
    if os.path.exists(os.path.join(chk.LLVM, "llvm-objdump")):
        bad, n_fn, n_mfma = chk.check_library(lib_path)
        assert n_fn >= min_kernels and n_mfma >= min_mfma and not bad, (n_fn, n_mfma, bad[:5])
    return text


def raw_fwd_bwd(net, x, dy, fill=None):
    """One ``<net._entry>_fwd`` (with keep) + ``_bwd`` (with dx, accumulate = 0) through the raw entry points on banded buffers
    -> the result bytes.  `fill`: the byte every output, keep, workspace and gradient buffer holds on entry."""
    fwd, bwd = (getattr(net._library(), f"{net._entry}_{what}") for what in ("fwd", "bwd"))
    M = x.shape[0]
    dims = net.dims()
    ptrs, n = net._pointers(None)
    band = 256
    sizes = dict(y=4 * M * net.output_dim, keep=4 * net.keep_floats(M), ws=net.workspace_bytes(M),
                 grads=4 * net.num_param_floats(), dx=4 * M * net.input_dim)
    bufs = {k: torch.full((v + 2 * band,), 0xA5 if fill is None else fill, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    for b in bufs.values():
        b[:band] = 0x5C
        b[-band:] = 0x5C
    p = {k: b.data_ptr() + band for k, b in bufs.items()}
    s = torch.cuda.current_stream().cuda_stream
    assert fwd(ptrs, n, C.byref(dims), x.data_ptr(), M, p["y"], p["keep"], s) == 0
    assert bwd(ptrs, n, C.byref(dims), p["keep"], dy.data_ptr(), M, p["dx"], p["grads"], p["ws"], sizes["ws"], 0, s) == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b[:band] == 0x5C).all()) and bool((b[-band:] == 0x5C).all()), f"{k}: a sentinel band was written"
    return {k: bufs[k][band:band + sizes[k]].clone() for k in ("y", "keep", "grads", "dx")}


def check_row_ranges_add_up(net, x, dy, cut=256):
    """The flat gradient of a raw fwd + bwd over all M rows is, bit for bit, the single fp32 addition of the flat gradients
    over rows [0, cut) and [cut, M), each from a call of its own; y and dx are the two calls' concatenated.  Exact for
    M = 300, cut = 256: the weight-gradient slabs' row ranges hold 256 rows up to M = 16384, so range 0 is the 256-row call's
    only range; range 1 starts on a 16-row tile boundary and takes the 44-row call's steps, 16 + 16 + 12 rows (for the chunked
    kernel one full chunk and a partial one); rows padded with zeros add exact zeros; the reduce is one addition."""
    M = x.shape[0]
    whole = raw_fwd_bwd(net, x, dy)
    head, tail = (raw_fwd_bwd(net, x[a:b].contiguous(), dy[a:b].contiguous()) for a, b in ((0, cut), (cut, M)))
    g = lambda r: r["grads"].view(torch.float32)                             # noqa: E731
    assert bool(torch.isfinite(g(whole)).all()) and g(head).abs().max() > 0 and g(tail).abs().max() > 0
    assert torch.equal(bits(g(whole)), bits(g(head) + g(tail)))
    for k in ("y", "dx"):
        assert torch.equal(whole[k], torch.cat([head[k], tail[k]])), k


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def profile_site(site, fn):
    """Runs fn() with the launch-site timer on `site`; returns (milliseconds, number of timed regions) it recorded."""
    from beso_amd import _lib
    lib = _lib.load()
    lib.beso_profile_enable(_lib.SITES[site])
    try:
        fn()
        torch.cuda.synchronize()
        ms, n = C.c_double(0.0), C.c_int(0)
        assert lib.beso_profile_read(C.byref(ms), C.byref(n)) == 0
    finally:
        lib.beso_profile_enable(0)
    return ms.value, n.value


def count_site_launches(site, fn):
    return profile_site(site, fn)[1]


def kernel_names(fn):
    """Runs fn() under the torch profiler; returns the names of the GPU kernels it launched, the library's own among them (the
    profiler records every kernel of the process), in the order they started."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


class Scale(torch.nn.Module):
    """Stands in for an nn.Dropout: multiplies by preset keep-scales, one tensor per call, in call order."""

    def __init__(self, *scales):
        super().__init__()
        self.scales, self.calls = scales, 0

    def forward(self, x):
        s = self.scales[self.calls % len(self.scales)]
        self.calls += 1
        assert s.shape == x.shape, (tuple(s.shape), tuple(x.shape))
        return x * s
