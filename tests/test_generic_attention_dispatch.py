"""Every branch of the generic attention dispatch (``launch_attention`` / ``launch_t`` / ``launch_hdp`` in
beso_amd/csrc/attention.hip) against the numpy oracle in float64: one-layer networks of shapes that no fused kernel takes, so the
forward runs LayerNorm -> q|k|v GEMM -> attention -> ... on the generic kernels, once under the per-op plan hint and once under
the library's own plan choice (fp32 on shapes with ``D % 8 == 0``: the chip-wide small-batch path, which calls the same
``launch_attention`` when the window has more than 16 tokens or the head dim is no multiple of 4; everything else: the per-op
kernels again).  Both runs are held to the oracle, not to each other.

Which kernel a case takes is part of the case: the expected name is worked out from the predicates of ``launch_attention``
(precision, hd, hd % 8, row bytes % 8, D % 8, T <= 16, T > 128) and ``launch_hdp`` (3 * T * hd * sizeof(E) against its 64 KiB
budget) and asserted against the kernel names the torch profiler records for the calls.

What the library refuses instead of computing is pinned as a refusal (status and wording, before anything is enqueued):
  * hd = 130: ``validate_config`` (api.hip) returns BESO_ERR_UNSUPPORTED, so ``launch_t``'s own ``hd > 128`` return is never reached;
  * every bf16x3 row of a shape without a fused instance: bf16x3 has no per-op form (``beso_pack_weights`` returns
    BESO_ERR_UNSUPPORTED, ``forward()`` in api.hip too).  ``launch_attention`` sees BESO_PREC_BF16X3 only from the block kernels of
    the long-sequence shape (D = 512, 8 heads of 64, 13 ... 80 tokens), where two of its branches are live: the split-bf16 matrix
    kernel (T > 16) and the fall-back to ``launch_t<float>`` for a call of at most 16 tokens.  Those run here as parity cases; the
    fall-backs for hd % 8 != 0, hd > 64 and T > 128 cannot be reached from any entry point.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from conftest import rel_err
from support import bits, kernel_names, lib, make_denoiser, to_dev  # noqa: F401      (lib: the fixture)
from test_gpu_parity import TOL

gpu = pytest.mark.gpu
B = 5
ROWWISE, LDS, MFMA, MFMA_X3 = "attention_rowwise_kernel", "attention_kernel", "attention_mfma_kernel", "attention_mfma_x3_kernel"


def _case(prec, H, hd, G, W, kernel, why, t=None):
    t = W if t is None else t
    T = 1 + G + 2 * t
    return pytest.param(prec, H, hd, G, W, t, kernel, id=f"{prec}-H{H}-hd{hd}-T{T}-{why}")


# precision, heads, head dim, goal tokens, window -> T = 1 + G + 2 W tokens; the kernel launch_attention picks and why.
# fp32 (4-byte elements): launch_t<float> always; row-wise where hd * 4 or D * 4 is no multiple of 8, or 12 * T * hd > 65536
PARITY = [
    _case("fp32", 8, 5, 2, 3, (ROWWISE, "float", 32), "odd-hd"),                     # T = 9; rows of 20 bytes
    _case("fp32", 8, 33, 2, 7, (ROWWISE, "float", 64), "odd-hd-above-32"),           # T = 17; rows of 132 bytes
    _case("fp32", 3, 7, 2, 3, (ROWWISE, "float", 32), "odd-D"),                      # T = 9; D = 21: GEMM / LayerNorm edges at D % 4 != 0
    _case("fp32", 2, 96, 2, 7, (LDS, "float", 128), "hdp128"),                       # T = 17; 19584 B per pair, 3 pairs per block
    _case("fp32", 1, 128, 2, 15, (LDS, "float", 128), "hd-is-hdp"),                  # T = 33; 50688 B per pair: one pair per block
    _case("fp32", 1, 128, 2, 31, (ROWWISE, "float", 128), "budget-hdp128"),          # T = 65; 99840 B per pair > 64 KiB
    _case("fp32", 2, 64, 1, 63, (ROWWISE, "float", 64), "budget"),                   # T = 128; 98304 B per pair > 64 KiB
    _case("fp32", 2, 32, 2, 64, (LDS, "float", 32), "ppb-clamp"),                    # T = 131 > 128 threads: ppb 0 -> 1; 50304 B
    # bf16 (2-byte elements): the matrix kernel for hd <= 64, hd % 8 == 0, D % 8 == 0, 16 < T <= 128; launch_t<uint16_t> otherwise
    _case("bf16", 2, 64, 1, 7, (LDS, "u16", 64), "T16"),                             # T = 16: the last of the staged kernel
    _case("bf16", 2, 64, 2, 7, (MFMA,), "T17"),                                      # T = 17: the first of the matrix kernel
    _case("bf16", 2, 64, 1, 63, (MFMA,), "T128"),                                    # T = 128: its last (54272 B per pair, 2 per block)
    _case("bf16", 2, 64, 2, 63, (LDS, "u16", 64), "T129"),                           # T = 129: 49536 B per pair <= 64 KiB, ppb 0 -> 1
    _case("bf16", 4, 12, 2, 15, (LDS, "u16", 32), "hd12"),                           # T = 33; hd % 8 != 0, rows of 24 bytes
    _case("bf16", 4, 6, 2, 15, (ROWWISE, "u16", 32), "hd6"),                         # T = 33; rows of 12 bytes
    _case("bf16", 2, 96, 2, 15, (LDS, "u16", 128), "hd96"),                          # T = 33; hd > 64; 19008 B per pair
    _case("bf16", 2, 64, 2, 95, (ROWWISE, "u16", 64), "budget"),                     # T = 193; 74112 B per pair > 64 KiB
    _case("bf16", 2, 8, 2, 7, (MFMA,), "hd8"),                                       # T = 17; the smallest hd of the matrix kernel
    # bf16x3 where launch_attention can see it (module docstring): D = 512 = 8 heads of 64, block kernels around the attention
    _case("bf16x3", 8, 64, 2, 7, (MFMA_X3,), "smallest-T"),                          # T = 17
    _case("bf16x3", 8, 64, 1, 39, (MFMA_X3,), "largest-T"),                          # T = 80: 69120 B of LDS <= 160 KiB
    _case("bf16x3", 8, 64, 2, 7, (LDS, "float", 64), "short-call", t=6),             # T = 15 <= 16: launch_t<float>, 11520 B per pair
]
# the bf16x3 rows that are refused: no fused instance for the shape, and bf16x3 has no per-op form.  Had they run:
# attention_mfma_x3_kernel (hd 8, T 17), attention_mfma_x3_kernel (hd 48, T 128: 110592 B of LDS <= 160 KiB), and launch_t<float>
# for T <= 16 (T 9), hd % 8 != 0 (hd 12), hd > 64 (hd 96), T > 128 (T 131)
X3_REFUSED = [(2, 8, 2, 7), (4, 48, 1, 63), (2, 64, 2, 3), (4, 12, 2, 15), (2, 96, 2, 15), (2, 32, 2, 64)]      # H, hd, G, W
BOUND = {"fp32": TOL["fp32"], "bf16": TOL["bf16"], "bf16x3": 1e-4}                   # bf16x3: the mode's documented bound
assert BOUND["bf16x3"] == TOL["bf16x3"]


def _cfg(H, hd, G, W):
    return O.ScoreGPTConfig(obs_dim=6, act_dim=3, embed_dim=H * hd, n_layers=1, n_heads=H, goal_seq_len=G, obs_seq_len=W,
                            sigma_data=0.5)


@functools.lru_cache(maxsize=None)
def _problem(H, hd, G, W, t, batch, std=0.05):
    """cfg, weights, (state, action, goal, sigma) and the float64 oracle's output -- computed once per shape, never written to."""
    cfg = _cfg(H, hd, G, W)
    w = O.make_weights(cfg, seed=5, std=std)
    s, g, a = O.make_inputs(cfg, batch, seed=3, t=t)
    sg = np.linspace(0.1, 0.9, B).astype(np.float32)[:batch]
    ref = O.denoise(w, cfg, s, a, g, sg, dtype=np.float64)
    for v in (s, a, g, sg, ref):
        v.setflags(write=False)
    return cfg, w, (s, a, g, sg), ref


def per_sample_err(out, ref, sigma_data):
    """max |out_b - ref_b| / max(max |ref_b|, sigma_data / 2) for each sample b (the floor of tests/fuzz_shapes.py: a sample whose
    few outputs all happen to be small is measured on the output scale, not on itself)."""
    d = np.abs(np.asarray(out, np.float64) - ref).reshape(len(ref), -1).max(axis=1)
    return d / np.maximum(np.abs(ref).reshape(len(ref), -1).max(axis=1), 0.5 * sigma_data)


def attention_kernels(names):
    """The attention.hip kernels among the profiler's kernel names, as (name,) or (name, element, HDP) -- from the demangled
    form ``attention_kernel<float, 32>`` or the mangled one ``attention_kernelIfLi32EE``."""
    out = []
    for n in names:
        m = re.search(r"(attention\w*?_kernel)(?:<\s*([a-z ]+?)\s*,\s*(\d+)\s*>|I([ft])Li(\d+)E)?", n)
        if not m:
            continue
        if m.group(2) or m.group(4):
            elem = {"float": "float", "f": "float", "unsigned short": "u16", "t": "u16"}[m.group(2) or m.group(4)]
            out.append((m.group(1), elem, int(m.group(3) or m.group(5))))
        else:
            out.append((m.group(1),))
    return out


def _run(m, inputs, hint):
    from beso_amd.runtime import set_plan
    s, a, g, sg = (np.array(v) for v in inputs)          # (copies: the shared arrays are read-only, torch wants writable ones)
    set_plan(forward=hint)
    try:
        with torch.no_grad():
            return m(to_dev(s), to_dev(a), to_dev(g), to_dev(sg))
    finally:
        set_plan(forward=0)


def test_kernel_name_parser():
    names = ["void beso::attention_kernel<float, 32>(float const*, float*, int, int, int, int, int, int, float, int)",
             "void beso::attention_rowwise_kernel<unsigned short, 128>(unsigned short const*, unsigned short*, int) [clone .kd]",
             "_ZN4beso24attention_rowwise_kernelIfLi64EEEvPKT_PS1_iiiiiif", "_ZN4beso16attention_kernelItLi128EEEvPKT_PS1_iiiiiifi",
             "beso::attention_mfma_kernel(unsigned short const*, unsigned short*, int, int, int, int, int, int, float)",
             "_ZN4beso24attention_mfma_x3_kernelEPKfPfiiiiiif", "void beso::gemm_kernel<float, 0>(float const*)",
             "void beso::(anonymous namespace)::sb_qkv_attn_kernel<float, 1, 16>(float const*)"]
    assert attention_kernels(names) == [(LDS, "float", 32), (ROWWISE, "u16", 128), (ROWWISE, "float", 64), (LDS, "u16", 128),
                                        (MFMA,), (MFMA_X3,)]


def test_a_causal_mask_off_by_one_token_cannot_hide_under_the_fp32_bound(monkeypatch):
    """The comparison bites (CPU only): the oracle with token i allowed to see token i + 1, on the smallest row-wise case at the
    weight scale the GPU cases use (std = 0.05), is 2.3e-2 away from the true oracle over the tensor and at least 1.1e-3 on every
    single sample -- three and two orders above the fp32 bound of 2e-5, so neither check can pass a mask error of one token."""
    cfg, w, (s, a, g, sg), ref = _problem(8, 5, 2, 3, 3, B)
    tril = np.tril
    with monkeypatch.context() as mp:
        mp.setattr(np, "tril", lambda m, k=0: tril(m, k + 1))
        off = O.denoise(w, cfg, s, a, g, sg, dtype=np.float64)
    assert np.array_equal(O.denoise(w, cfg, s, a, g, sg, dtype=np.float64), ref)       # (the mask is the true one again)
    whole, each = rel_err(off, ref), per_sample_err(off, ref, cfg.sigma_data)
    print(f"[parity] causal mask off by one token, fp32 H=8 hd=5 T=9: rel err {whole:.3e}, per sample min {each.min():.3e}")
    assert whole > 10 * TOL["fp32"] and each.min() > 10 * TOL["fp32"]
    # and the float32 oracle the other parity tests use is the same function to rounding
    assert rel_err(O.denoise(w, cfg, s, a, g, sg), ref) < 1e-6


@gpu
@pytest.mark.parametrize("prec,H,hd,G,W,t,kernel", PARITY)
def test_dispatch_branch_matches_the_oracle(prec, H, hd, G, W, t, kernel):
    """Per case: the whole-tensor error of both plans under the mode's bound; fp32 and bf16x3 under the same bound per sample;
    the row-wise cases at B = 1 as well (a grid whose only block is partial); the expected kernel, and only it, ran once per call."""
    from beso_amd import _lib
    T = 1 + G + 2 * t
    batches = (B, 1) if kernel[0] == ROWWISE else (B,)
    outs = {}

    def calls():
        for nb in batches:
            cfg, w, inputs, _ = _problem(H, hd, G, W, t, nb)
            m = make_denoiser(cfg, w, prec)
            for plan, hint in (("per-op", _lib.PLAN_PER_OP), ("library", 0)):
                outs[nb, plan] = _run(m, inputs, hint).cpu().numpy()

    ran = attention_kernels(kernel_names(calls))
    for (nb, plan), out in outs.items():
        cfg, _, _, ref = _problem(H, hd, G, W, t, nb)
        assert out.shape == ref.shape and np.isfinite(out).all()
        err, each = rel_err(out, ref), per_sample_err(out, ref, cfg.sigma_data)
        print(f"[parity] generic attention {prec} H={H} hd={hd} T={T} B={nb} {plan} ({kernel[0]}): {err:.3e}, per sample max {each.max():.3e}")
        assert err < BOUND[prec], (nb, plan)
        if prec != "bf16":
            assert each.max() < BOUND[prec], (nb, plan, each)
    assert ran == [kernel] * len(outs), ran


@gpu
@pytest.mark.parametrize("prec,H,hd,G,W,t,kernel", [c for c in PARITY if c.values[6][0] == ROWWISE or 1 + c.values[3] + 2 * c.values[5] > 128])
def test_earlier_steps_do_not_see_the_last_one(prec, H, hd, G, W, t, kernel):
    """Causality of the row-wise and T > 128 cases: with the last time step's state and action replaced, every earlier step's
    output keeps its bits (rows are computed independently of each other everywhere else in the network), under both plans."""
    from beso_amd import _lib
    cfg, w, (s, a, g, sg), _ = _problem(H, hd, G, W, t, B)
    s2, a2 = s.copy(), a.copy()
    s2[:, -1] = 1.0 - s[:, -1]
    a2[:, -1] = 0.5 - a[:, -1]
    m = make_denoiser(cfg, w, prec)
    for hint in (_lib.PLAN_PER_OP, 0):
        one, two = _run(m, (s, a, g, sg), hint), _run(m, (s2, a2, g, sg), hint)
        assert torch.equal(bits(one[:, :-1]), bits(two[:, :-1])), hint
        assert not torch.equal(bits(one[:, -1]), bits(two[:, -1])), hint


def _status(lib, cfg, precision, nbytes=1 << 40):
    """beso_denoise_fwd on pointers that are not memory: a call that got past its checks would read and write through them."""
    one = C.c_void_p(0x1000)
    return lib.beso_denoise_fwd(C.byref(cfg), one, precision, one, one, one, one, one, B, cfg.obs_seq_len, 0, 1.0, one, nbytes, None)


def test_refusals_happen_before_anything_is_enqueued(lib):
    """hd = 130 and the bf16x3 rows of shapes without a fused instance: BESO_ERR_UNSUPPORTED from the config check / the pack / the
    forward's plan decision, with dummy pointers throughout.  hd = 128 with the same pointers gets as far as the workspace check."""
    from beso_amd import _lib
    from beso_amd.runtime import ScoreNetShape
    shape = lambda H, hd, G, W: ScoreNetShape(6, 3, H * hd, 1, H, G, W, True, 0.5).c_struct()       # noqa: E731
    one = C.c_void_p(0x1000)
    arr = (C.c_void_p * 64)(*([0x1000] * 64))
    big = shape(1, 130, 2, 3)
    for prec in (_lib.PREC_FP32, _lib.PREC_BF16, _lib.PREC_BF16X3):
        assert _status(lib, big, prec) == _lib.ERR_UNSUPPORTED
        assert lib.beso_pack_weights(C.byref(big), arr, 64, one, 1 << 40, prec, None) == _lib.ERR_UNSUPPORTED
        assert lib.beso_num_params(C.byref(big)) == 0 and lib.beso_packed_bytes(C.byref(big), prec) == 0
        assert lib.beso_workspace_bytes(C.byref(big), B, 3, prec, 0) == 0
    ok = shape(1, 128, 2, 3)
    assert lib.beso_num_params(C.byref(ok)) > 0 and _status(lib, ok, _lib.PREC_FP32, nbytes=16) == _lib.ERR_WORKSPACE
    for H, hd, G, W in X3_REFUSED:
        cfg = shape(H, hd, G, W)
        n = lib.beso_num_params(C.byref(cfg))
        assert 0 < n <= 64
        assert lib.beso_pack_weights(C.byref(cfg), arr, n, one, 1 << 40, _lib.PREC_BF16X3, None) == _lib.ERR_UNSUPPORTED, (H, hd)
        assert _status(lib, cfg, _lib.PREC_BF16X3) == _lib.ERR_UNSUPPORTED, (H, hd)
        assert _status(lib, cfg, _lib.PREC_FP32, nbytes=16) == _lib.ERR_WORKSPACE            # (fp32 takes the same shape)
    with pytest.raises(ValueError, match=r"unsupported configuration \(status -5\)"):
        _lib.check(_lib.ERR_UNSUPPORTED, "pack_weights")


@gpu
def test_head_dim_130_raises_by_name():
    """fp32, H = 1, D = 130: the Python call raises the library's error for the shape; no tensor comes back."""
    cfg = _cfg(1, 130, 2, 3)
    s, g, a = O.make_inputs(cfg, B, seed=3)
    out = None
    with pytest.raises(ValueError, match="beso_hip: unsupported model shape"), torch.no_grad():
        m = make_denoiser(cfg, O.make_weights(cfg, seed=5, std=0.05), "fp32")
        out = m(to_dev(s), to_dev(a), to_dev(g), to_dev(np.linspace(0.1, 0.9, B).astype(np.float32)))
    assert out is None


@gpu
@pytest.mark.parametrize("H,hd,G,W", X3_REFUSED)
def test_bf16x3_without_a_fused_instance_raises_by_name(H, hd, G, W):
    """The bf16x3 rows the library refuses: ValueError with the pack's wording under either plan, no tensor comes back."""
    from beso_amd import _lib
    cfg, w, inputs, _ = _problem(H, hd, G, W, W, B)
    for hint in (_lib.PLAN_PER_OP, 0):
        out = None
        with pytest.raises(ValueError, match=r"beso_hip: pack_weights: unsupported configuration \(status -5\)"):
            out = _run(make_denoiser(cfg, w, "bf16x3"), inputs, hint)
        assert out is None
