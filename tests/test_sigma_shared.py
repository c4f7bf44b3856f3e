"""The sigma token shared across a uniform-sigma batch (kitchen, bf16 / fp16; fused.hip: the pre-pass, the five-tile instance
of layers_kernel and the sigma-token cache inside the packed image).

Token 0 of every sample has no position and attends to itself only, so its k / v rows depend on (weights, sigma) alone.  A
forward whose sigma is one value takes them from the cache (computing the entry once) and runs ten tokens per sample in five
token tiles.  Everything here is an equality of bits: the five-tile instance against the six-tile and the two-sample
instances, non-uniform batches (which must take the six-tile instance and leave the cache alone), the cache's replacement
and its invalidation by a repack, and the launch-site count of a qualifying forward."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from beso_amd import _lib
from support import load_weights, make_denoiser, profile_site, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIVE = _lib.PLAN_FUSED | _lib.PLAN_SIGMA_SHARED                       # eight samples per workgroup, sigma token shared
SIX = _lib.PLAN_FUSED | _lib.PLAN_SPW8 | _lib.PLAN_SIGMA_PRIVATE      # eight samples per workgroup, as before
TWO = _lib.PLAN_FUSED | _lib.PLAN_SPW2 | _lib.PLAN_SIGMA_PRIVATE      # the two-sample latency instance


def make_module(precision, seed=5, std=0.04, cfg=O.KITCHEN):
    return make_denoiser(cfg, O.make_weights(cfg, seed=seed, std=std), precision)


def entries(m):
    """Occupied entries of the sigma-token cache of the module's CURRENT packed image (development library)."""
    inner = m.inner_model
    rt, packed = inner.runtime(O.KITCHEN.sigma_data), inner.packed_weights()
    torch.cuda.synchronize()
    return _lib.load_dev().beso_debug_sigma_cache_entries(C.byref(rt.cfg), packed.buf.data_ptr(), packed.precision)


def run(fn, hint):
    from beso_amd.runtime import plan
    with torch.no_grad(), plan(forward=hint):
        return fn()


@pytest.fixture(scope="module")
def modules():
    return {p: make_module(p) for p in ("bf16", "fp16")}


def modes(m):
    from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel
    pair = ClassifierFreeSampleModel(m, 1.5)
    return {"cond": lambda *a: m(*a), "uncond": lambda *a: m(*a, uncond=True), "pair": lambda *a: pair(*a)}


@pytest.mark.parametrize("B", [8, 21, 64])             # 21: a last workgroup of 5 samples (2 with a classifier-free pair)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_five_tile_equals_six_tile_and_two_sample_bit_for_bit(modules, precision, B):
    m = modules[precision]
    for t in (1, 2, 4):
        s, g, a = (to_dev(v) for v in O.make_inputs(O.KITCHEN, B, seed=B + t, t=t))
        for k, (name, fn) in enumerate(modes(m).items()):
            # a sigma no other case of this module uses: the first shared call must add exactly one entry (i.e. it DID take
            # the pre-pass and the five-tile instance), the second one none
            sg = torch.full((B,), 0.05 + 0.0007 * B + 0.11 * t + 0.05 * k, device=DEV)
            n0 = entries(m)
            five = run(lambda: fn(s, a, g, sg), FIVE)
            assert entries(m) == min(n0 + 1, 128), (name, t)
            again = run(lambda: fn(s, a, g, sg), FIVE)
            assert entries(m) == min(n0 + 1, 128), (name, t)
            six = run(lambda: fn(s, a, g, sg), SIX)
            two = run(lambda: fn(s, a, g, sg), TWO)
            assert torch.isfinite(five).all(), (name, t)
            assert torch.equal(five, six), (name, t)
            assert torch.equal(again, six), (name, t)
            assert torch.equal(five, two), (name, t)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_a_non_uniform_batch_takes_the_six_tile_instance_and_adds_no_entry(modules, precision):
    m = modules[precision]
    B = 21
    s, g, a = (to_dev(v) for v in O.make_inputs(O.KITCHEN, B, seed=77))
    for odd in (B - 1, 0):                              # one sample of the last workgroup, then of the first
        sg = torch.full((B,), 0.4171, device=DEV)
        sg[odd] = 0.77
        n0 = entries(m)
        shared = run(lambda: m(s, a, g, sg), FIVE)
        assert entries(m) == n0
        assert torch.equal(shared, run(lambda: m(s, a, g, sg), SIX))
        # the samples at the common sigma equal their rows of the uniform batch (which takes the five-tile instance)
        uni = run(lambda: m(s, a, g, torch.full((B,), 0.4171, device=DEV)), FIVE)
        keep = [i for i in range(B) if i != odd]
        assert torch.equal(shared[keep], uni[keep])
        assert not torch.equal(shared[odd], uni[odd])


@pytest.mark.parametrize("G_len,W", [(3, 4), (1, 5)])
def test_a_window_of_twelve_tokens_takes_the_six_tile_instance(G_len, W):
    """A kitchen-class model (360 wide, 6 heads) with 1 + G + 2 W = 12 tokens per sample: eight samples' other eleven tokens
    are 88 slots, more than five token tiles, so a full window must take the six-tile instance (equal bits, no cache entry)
    even when the hint asks for sharing; the windows one step shorter (ten tokens: 8 x 9 = 72 slots) share.  B = 21: two full
    workgroups (their samples 6 and 7 are the ones whose tokens would fall outside the tiles) and one of five samples."""
    cfg = dataclasses.replace(O.KITCHEN, goal_seq_len=G_len, obs_seq_len=W)
    m = make_module("bf16", cfg=cfg)
    B = 21
    for t, shares in ((W, False), (W - 1, True)):
        assert 1 + G_len + 2 * t == (12 if t == W else 10)
        s, g, a = (to_dev(v) for v in O.make_inputs(cfg, B, seed=40 + t, t=t))
        for k, (name, fn) in enumerate(modes(m).items()):
            sg = torch.full((B,), 0.2 + 0.1 * k + 0.03 * t, device=DEV)
            n0 = entries(m)
            five = run(lambda: fn(s, a, g, sg), FIVE)
            assert entries(m) == n0 + int(shares), (name, t)
            assert torch.isfinite(five).all(), (name, t)
            assert torch.equal(five, run(lambda: fn(s, a, g, sg), SIX)), (name, t)
            assert torch.equal(five, run(lambda: fn(s, a, g, sg), TWO)), (name, t)
    # ... and without a hint at a batch the eight-sample plan takes (the default dispatch of a large uniform-sigma batch)
    B = 1032
    s, g, a = (to_dev(v) for v in O.make_inputs(cfg, B, seed=50))
    sg = torch.full((B,), 0.45, device=DEV)
    n0 = entries(m)
    own = run(lambda: m(s, a, g, sg), 0)
    assert entries(m) == n0
    assert torch.equal(own, run(lambda: m(s, a, g, sg), SIX))
    assert torch.equal(own[:64], run(lambda: m(s[:64], a[:64], g[:64], sg[:64]), TWO))


def test_cache_hits_replacement_and_fresh_modules():
    """sigma a, b, a on one module gives the bits of a fresh module (an empty cache) at each; 130 distinct sigmas in turn
    replace the first entries round-robin (128 entries), and the first sigma, computed again, gives the same bits."""
    B = 8
    s, g, a = (to_dev(v) for v in O.make_inputs(O.KITCHEN, B, seed=3))
    m = make_module("bf16")
    sig = lambda v: torch.full((B,), float(v), device=DEV)
    ref = {v: run(lambda: make_module("bf16")(s, a, g, sig(v)), FIVE) for v in (0.3, 0.7)}
    for k, v in enumerate((0.3, 0.7, 0.3)):
        assert torch.equal(run(lambda: m(s, a, g, sig(v)), FIVE), ref[v]), k
        assert entries(m) == min(k + 1, 2)
    assert torch.equal(ref[0.3], run(lambda: m(s, a, g, sig(0.3)), SIX))
    m = make_module("bf16")
    values = [0.01 * (k + 1) for k in range(130)]
    first = run(lambda: m(s, a, g, sig(values[0])), FIVE)
    for k, v in enumerate(values[1:], start=2):
        out = run(lambda: m(s, a, g, sig(v)), FIVE)
        if k in (2, 128, 129, 130):
            assert entries(m) == min(k, 128), k
            assert torch.equal(out, run(lambda: m(s, a, g, sig(v)), SIX)), k
    # values[0] and values[1] were replaced by the 129th and 130th: the first is a miss again
    assert torch.equal(run(lambda: m(s, a, g, sig(values[0])), FIVE), first)
    assert torch.equal(first, run(lambda: m(s, a, g, sig(values[0])), SIX))
    assert entries(m) == 128


def test_a_repack_invalidates_the_cache():
    """load_state_dict with other weights between two calls at the same sigma: the result follows the new weights."""
    B = 16
    s, g, a = (to_dev(v) for v in O.make_inputs(O.KITCHEN, B, seed=9))
    sg = torch.full((B,), 0.25, device=DEV)
    m = make_module("bf16", seed=5)
    old = run(lambda: m(s, a, g, sg), FIVE)
    assert entries(m) == 1
    load_weights(m, O.make_weights(O.KITCHEN, seed=6, std=0.04))
    assert entries(m) == 0                              # (the accessor packs the new image: its cache is empty)
    new = run(lambda: m(s, a, g, sg), FIVE)
    assert entries(m) == 1
    assert not torch.equal(new, old)
    assert torch.equal(new, run(lambda: m(s, a, g, sg), SIX))
    assert torch.equal(new, run(lambda: make_module("bf16", seed=6)(s, a, g, sg), SIX))


def test_a_qualifying_forward_is_one_launch_at_the_fused_layer_site(modules):
    """The pre-pass and both instances are one group at the launch-site timer: one event pair per forward."""
    m = modules["bf16"]
    B = 24
    s, g, a = (to_dev(v) for v in O.make_inputs(O.KITCHEN, B, seed=1))
    for sg in (torch.full((B,), 0.3, device=DEV), to_dev(np.linspace(0.05, 1.0, B).astype(np.float32))):
        ms, n = profile_site("fused_layer", lambda: run(lambda: m(s, a, g, sg), FIVE))
        assert n == 1 and ms > 0.0
