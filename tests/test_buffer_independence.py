"""No result may depend on a byte the call did not write.

Every buffer the library works in reaches it uninitialised (torch.empty in runtime.py / training.py; include/beso_hip.h states
the contract).  These tests hand the C ABI its workspace, outputs, solver history, gradient buffer, loss / dot cells and the
packed-weight image pre-filled with three byte patterns and require the SAME bits (forwards, samplers, VJP) or the same numbers
within the training step's own bounds (it accumulates with fp32 atomics) under all three:

    ZERO 0x00   0 in every format                                   the baseline
    NAN  0xFF   fp32 0xFFFFFFFF, bf16 / fp16 0xFFFF: NaN            any arithmetic use (0 * NaN is NaN)
    HUGE 0x7B   fp32 / bf16 ~1.3e36, fp16 61280: finite             uses a NaN slips through: fmaxf / fminf / v_max / v_med3 drop
                                                                    a NaN operand (a softmax row maximum, a clamp)

The same byte is poison in every element type the library stores; test_fill_patterns_decode_as_claimed pins the decodings.

The fills poison VALUES, never addresses.  Regions that hold integers, offsets or pointers, read from the carve code
(make_workspace / Workspace in api.hip + common.h, make_train_ws / TrainWs in train.hip, make_layout / Layout for the image):
  * Workspace (forward, samplers): x, xn, qkv, y, h, den, x2, d1, sig, small are fp32 / operand-typed rows; `fused` is a
    zero-byte carve.  No integer region.
  * TrainWs: every carve is fp32 or operand-typed data (kept activations, weight copies, fragment images, partial-sum slabs).
    The table of (source, destination) pointers of pack_table_kernel and the sampler loop's step records travel as kernel
    ARGUMENTS, not through the workspace.  No integer region.
  * Packed image: parameters only.  No integer region.
  * Host-side state (events, the side stream of the training step) is not in any caller buffer.
So no fill can redirect a load or a store; every check below is a value comparison, none relies on a fault.

What the image test can and cannot reach (small.hip, sb_qkv_attn_wide_kernel<PROJ>): the out-projection epilogue used to load
64 columns of Wp from h * hd whatever hd is.  The part of that over-read that lands in PAD columns / rows of the image is
poisoned here through the packed buffer's fill; the part that lands in the next head's columns or the next real weight tensor
cannot be poisoned without changing the true result -- that part is closed in the kernel (words with k >= hd are selected to
zero and fetched from inside the head) and is covered by the bit-identity tests against the other plans.

GPU tests carry @pytest.mark.gpu one by one: the CPU-side checks of this file run in the CPU suite.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import beso_oracle as O
from beso_amd import _lib
from support import grad_errors, make_denoiser, to_dev, train_inputs

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = {"ZERO": 0x00, "NAN": 0xFF, "HUGE": 0x7B}
PAD = 4096                      # guard bytes in front of and behind every payload (test_no_writes_outside_output_and_workspace's layout)

_GENERIC_96 = O.ScoreGPTConfig(obs_dim=6, act_dim=4, embed_dim=96, n_layers=2, n_heads=4, goal_seq_len=2, obs_seq_len=3,
                               linear_output=True, sigma_data=0.5)          # hd = 24, D % 64 != 0: generic section only
_GENERIC_256 = O.ScoreGPTConfig(obs_dim=6, act_dim=4, embed_dim=256, n_layers=2, n_heads=8, goal_seq_len=2, obs_seq_len=3,
                                linear_output=True, sigma_data=0.5)         # hd = 32
_HD4 = O.ScoreGPTConfig(obs_dim=6, act_dim=4, embed_dim=32, n_layers=2, n_heads=8, goal_seq_len=2, obs_seq_len=3,
                        linear_output=True, sigma_data=0.5)                 # hd = 4: the attention backward's smallest head
_CFGS = dict(O.CONFIGS, generic_96=_GENERIC_96, generic_256=_GENERIC_256, hd4=_HD4)

# every precision that has an instance for the shape
_SHIPPED = ([("kitchen", p) for p in ("bf16", "fp16", "bf16x3", "fp32")] + [("block_push", p) for p in ("bf16", "fp16", "bf16x3", "fp32")]
            + [("long_horizon", p) for p in ("bf16", "bf16x3")]
            + [(c, p) for c in ("tiny", "tiny_mlp_head", "tiny_nogoal") for p in ("fp32", "bf16")])


def _const(name):
    """An integer constexpr of the HIP sources (the batch sizes at which the library changes kernels)."""
    for f in ("common.h", "fused.h", "fused.hip", "small.hip"):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, open(os.path.join(ROOT, "beso_amd", "csrc", f)).read())
        if m:
            return int(m.group(1))
    raise AssertionError(f"{name} not found in beso_amd/csrc")


# ------------------------------------------------------------------------------------------------ CPU
def test_fill_patterns_decode_as_claimed():
    """The table of the module docstring, with numpy: the same byte is zero / NaN / huge-but-finite as fp32, bf16 and fp16."""
    def decode(byte):
        raw = np.full(4, byte, dtype=np.uint8)
        f32 = raw.view(np.float32)[0]
        bf16 = (raw[:2].view(np.uint16).astype(np.uint32) << 16).view(np.float32)[0]      # bf16 = the upper half of an fp32
        f16 = raw[:2].view(np.float16)[0]
        return float(f32), float(bf16), float(f16)
    assert decode(FILLS["ZERO"]) == (0.0, 0.0, 0.0)
    assert all(np.isnan(v) for v in decode(FILLS["NAN"]))
    assert np.full(4, FILLS["NAN"], dtype=np.uint8).view(np.uint32)[0] == 0xFFFFFFFF
    f32, bf16, f16 = decode(FILLS["HUGE"])
    assert np.isfinite([f32, bf16, f16]).all()
    assert 1.2e36 < f32 < 1.4e36 and 1.2e36 < bf16 < 1.4e36 and f16 == 61280.0
    # what the fills are for: NaN survives a product with zero, and is DROPPED by max / min (IEEE maxNum, the v_max / fmaxf rule)
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.float32(0.0) * np.float32(np.nan)) and np.fmax(np.float32(np.nan), np.float32(1.0)) == 1.0
    assert np.fmax(np.float32(f32), np.float32(1.0)) == np.float32(f32)
    # the existing sentinel, for the record: finite and tiny in fp32 and bf16 -- invisible at every tolerance of the suite
    ab = np.full(4, 0xAB, dtype=np.uint8).view(np.float32)[0]
    assert np.isfinite(ab) and abs(float(ab)) < 2e-12


def test_boundary_constants_and_contract_are_in_the_sources():
    assert _const("kSmallProjRows") == 96 and _const("kSmallRows") == 448 and _const("kSmallBatchMax") == 512
    assert _const("kMaxLoopEvals") == 128
    header = open(os.path.join(ROOT, "include", "beso_hip.h")).read()
    assert "UNINITIALISED" in header and "beso_loss_grad_streams zeroes `grads_flat` on `loss_stream`" in header


# ------------------------------------------------------------------------------------------------ GPU helpers
class Guarded:
    """`nbytes` of payload, PAD bytes into a uint8 allocation that is `byte` everywhere: front guard | payload | back guard.
    With `data` the payload is an INPUT (or an in/out sample) between two bands of the fill: an over- or under-read that is
    masked but still used meets poison."""

    def __init__(self, nbytes, byte, data=None):
        self.n, self.byte = int(nbytes), byte
        self.big = torch.full((PAD + self.n + PAD,), byte, dtype=torch.uint8, device=DEV)
        if data is not None:
            src = data.contiguous().reshape(-1).view(torch.uint8)
            assert src.numel() == self.n
            self.big[PAD:PAD + self.n].copy_(src)

    @property
    def ptr(self):
        return self.big.data_ptr() + PAD

    def f32(self):
        return self.big[PAD:PAD + self.n].view(torch.float32)

    def guards_ok(self):
        """0-d bool tensor (no synchronisation here)"""
        return (self.big[:PAD] == self.byte).all() & (self.big[PAD + self.n:] == self.byte).all()


def _carries_fill(x, byte):
    """0-d bool tensor: some fp32 element of x still is the fill pattern (an element of the result nobody wrote)"""
    if byte == 0:
        return torch.zeros((), dtype=torch.bool, device=x.device)
    pat = int(np.full(4, byte, dtype=np.uint8).view(np.int32)[0])
    return (x.contiguous().view(torch.int32) == pat).any()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _env(cfg_name, precision):
    cfg = _CFGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=4, std=0.03), precision)
    inner = m.inner_model
    return cfg, m, inner, inner.runtime(cfg.sigma_data)


@functools.lru_cache(maxsize=64)
def _inputs(cfg_name, B, t):
    cfg = _CFGS[cfg_name]
    s, g, a = O.make_inputs(cfg, B, seed=B + 3 * t, t=t)
    rng = np.random.default_rng(B + 7 * t)
    noise = rng.standard_normal((5,) + a.shape).astype(np.float32)            # up to five steps' draws
    return to_dev(s), to_dev(g), to_dev(a), to_dev(np.linspace(0.1, 0.9, B).astype(np.float32)), to_dev(noise)


_SIG3 = (1.0, 0.3, 0.05, 0.0)                  # three steps
_SIG5 = (1.0, 0.5, 0.25, 0.1, 0.03, 0.0)       # five steps (n_sigmas = 6)


def _forward_call(cfg_name, precision, case, byte):
    """One C-ABI call with every buffer it writes pre-filled with `byte` and its inputs between bands of the same fill.
    -> (result payload (clone) or None, list of problems)."""
    cfg, _, inner, rt = _env(cfg_name, precision)
    lib, packed = rt.lib, inner.packed_weights()
    B, t, lam, flags, entry = case["B"], case["t"], case.get("lam", 1.0), case.get("flags", 0), case["entry"]
    s, g, a, sg, nz = _inputs(cfg_name, B, t)
    two = 1 if (entry != "score" and lam not in (0.0, 1.0) and not (flags & _lib.FLAG_UNCOND)) else 0
    wsb = lib.beso_workspace_bytes(C.byref(rt.cfg), B, t, packed.precision, two)
    assert wsb > 0
    ws = Guarded(wsb, byte)
    Gs, Ga, Gsg = Guarded(s.numel() * 4, byte, s), Guarded(a.numel() * 4, byte, a), Guarded(sg.numel() * 4, byte, sg)
    Gg = Guarded(g.numel() * 4, byte, g) if inner.goal_seq_len > 0 else None
    gp = Gg.ptr if Gg is not None else None
    n_out = a.numel() * 4
    watched = [ws, Gs, Ga, Gsg] + ([Gg] if Gg is not None else [])
    head = (C.byref(rt.cfg), packed.buf.data_ptr(), packed.precision)
    tail = (ws.ptr, wsb, _stream())
    if entry in ("score", "denoise"):
        out = Guarded(n_out, byte)
        if entry == "score":
            st = lib.beso_score_fwd(*head, Gs.ptr, Ga.ptr, gp, Gsg.ptr, out.ptr, B, t, flags, *tail)
        else:
            st = lib.beso_denoise_fwd(*head, Gs.ptr, Ga.ptr, gp, Gsg.ptr, out.ptr, B, t, flags, float(lam), *tail)
    else:
        sig = case["sigmas"]
        arr = (C.c_float * len(sig))(*sig)
        out = Guarded(n_out, byte, a)                                       # x: x_T on entry, the sample on return
        loop = (Gs.ptr, gp, out.ptr, B, t, arr, len(sig), float(lam))
        need_noise = entry == "ancestral" or (entry == "solver" and case["solver"].endswith("_ancestral"))
        Gn = None
        if need_noise:
            assert len(sig) - 1 <= nz.shape[0]
            Gn = Guarded((len(sig) - 1) * n_out, byte, nz[:len(sig) - 1])
            watched.append(Gn)
        if entry == "sample":
            st = lib.beso_sample(*head, _lib.SAMPLER_IDS[case["sampler"]], *loop, flags, *tail)
        elif entry == "ancestral":
            st = lib.beso_sample_ancestral(*head, *loop, 1.0, Gn.ptr, flags, *tail)
        else:
            order = case.get("order", 4)
            n_hist = {"dpmpp_2m": 1, "lms": order - 1}.get(case["solver"], 0)
            Gh = Guarded(n_hist * n_out, byte) if n_hist else None
            if Gh is not None:
                watched.append(Gh)
            st = lib.beso_sample_solver(*head, _lib.SOLVER_IDS[case["solver"]], *loop, 1.0, 1.0, order,
                                        Gn.ptr if Gn is not None else None, Gh.ptr if Gh is not None else None, flags, *tail)
    if st != 0:
        torch.cuda.synchronize()
        return None, [f"status {st} ({lib.beso_status_string(st).decode()})"]
    watched.append(out)
    res = out.f32()
    flags_t = torch.stack([torch.isfinite(res).all(), ~_carries_fill(res, byte)] + [w.guards_ok() for w in watched]).cpu().tolist()
    problems = []
    if not flags_t[0]:
        problems.append("result not finite")
    if not flags_t[1]:
        problems.append("a result element still carries the fill")
    names = ["workspace", "state", "action", "sigma"] + (["goal"] if Gg is not None else [])
    names += ["buffer %d" % i for i in range(len(watched) - len(names) - 1)] + ["out / x"]
    problems += [f"guard band of {n} changed" for n, ok in zip(names, flags_t[2:]) if not ok]
    # the inputs themselves are read-only
    if not (torch.equal(Gs.f32(), s.reshape(-1)) and torch.equal(Gsg.f32(), sg.reshape(-1))):
        problems.append("an input was written")
    return res.clone(), problems


def _check_across_fills(cfg_name, precision, cases):
    """Runs every case once per fill; -> list of failure strings (all of them, not the first: one GPU run shows the picture)."""
    failures = []
    for case in cases:
        res = {}
        for name, byte in FILLS.items():
            r, problems = _forward_call(cfg_name, precision, case, byte)
            res[name] = r
            failures += [f"{cfg_name} {precision} {_show(case)} fill {name}: {p}" for p in problems]
        if any(r is None for r in res.values()):
            continue
        for name in ("NAN", "HUGE"):
            if not torch.equal(res["ZERO"], res[name]):
                d = (res["ZERO"] - res[name]).abs()
                failures.append(f"{cfg_name} {precision} {_show(case)}: result under {name} differs from ZERO in "
                                f"{int((res['ZERO'] != res[name]).sum())} of {d.numel()} elements (max |diff| {float(d.nan_to_num(1e38).max()):.3e})")
    return failures


def _show(case):
    c = dict(case)
    if "flags" in c:
        c["flags"] = hex(c["flags"])
    if "sigmas" in c and len(c["sigmas"]) > 6:
        c["sigmas"] = f"<{len(c['sigmas'])} sigmas>"
    return str(c)


def _plans(cfg_name, precision):
    """The library's own choice and each hint that applies to the shape / precision (a hint that cannot be honoured is ignored
    by the library; the ones that would only repeat the same kernels are left out)."""
    L = _lib
    if precision in ("bf16x3", "fp16"):
        return [0] if cfg_name == "long_horizon" else [0, L.PLAN_SPW2, L.PLAN_SPW4, L.PLAN_SPW8]
    if cfg_name == "long_horizon":                                            # D = 512: no small-batch path; one sample per workgroup
        return [0, L.PLAN_PER_OP, L.PLAN_BLOCKS]
    if precision == "fp32":
        return [0, L.PLAN_SMALL, L.PLAN_PER_OP]
    if cfg_name in ("kitchen", "block_push"):
        return [0, L.PLAN_SMALL, L.PLAN_FUSED, L.PLAN_SPW2, L.PLAN_SPW4, L.PLAN_SPW8, L.PLAN_PER_OP, L.PLAN_BLOCKS]
    return [0, L.PLAN_SMALL, L.PLAN_FUSED, L.PLAN_PER_OP, L.PLAN_BLOCKS]


def _forward_cases(cfg_name, precision):
    cfg = _CFGS[cfg_name]
    W, T = cfg.obs_seq_len, 1 + cfg.G + 2 * cfg.obs_seq_len
    plans = _plans(cfg_name, precision)
    long = cfg_name == "long_horizon"
    # (513, W): seven empty sample slots in the last workgroup of the eight-sample instance; (129, W - 1): a ragged window
    shapes = [(2, W), (5, 1), (3, 31)] if long else [(1, 1), (3, 2), (5, W), (67, W), (129, max(W - 1, 1)), (513, W)]
    cases = []
    # A. forwards: every plan x every shape
    for fl in plans:
        for B, t in shapes:
            cases.append(dict(entry="denoise", B=B, t=t, flags=fl))
            cases.append(dict(entry="score", B=B, t=t, flags=fl))
    # ... and the batch sizes one below / one above the constants at which the library changes kernels
    # (token rows M <= kSmallProjRows: the 16-row small instance with the out-projection epilogue; M <= kSmallRows: the small
    #  path by the library's choice; B <= kSmallBatchMax: two samples per workgroup, <= 2 x: four, beyond: eight)
    if not long:
        edge = sorted({max(1, _const("kSmallProjRows") // T), _const("kSmallProjRows") // T + 1, _const("kSmallRows") // T,
                       _const("kSmallRows") // T + 1})
        for B in edge:
            for fl in [p for p in plans if p in (0, _lib.PLAN_SMALL)]:
                cases.append(dict(entry="denoise", B=B, t=W, flags=fl))
        for B in (_const("kSmallBatchMax"), 2 * _const("kSmallBatchMax"), 2 * _const("kSmallBatchMax") + 1):     # (+ 1: 513 is in `shapes`)
            cases.append(dict(entry="denoise", B=B, t=W, flags=0))
    # B. guidance: classifier-free pairs (2 B virtual samples, odd B), the unconditional-only forms
    odd = [(5, 1), (3, 31)] if long else [(3, 2), (5, W), (67, W), (513, W)]
    for fl in [p for p in plans if p in (0, _lib.PLAN_SMALL, _lib.PLAN_FUSED, _lib.PLAN_PER_OP, _lib.PLAN_SPW8)]:
        for B, t in odd:
            cases.append(dict(entry="denoise", B=B, t=t, flags=fl, lam=2.0))
            cases.append(dict(entry="denoise", B=B, t=t, flags=fl, lam=0.0))
            cases.append(dict(entry="denoise", B=B, t=t, flags=fl | _lib.FLAG_UNCOND))
            cases.append(dict(entry="score", B=B, t=t, flags=fl | _lib.FLAG_UNCOND))
    # C. sampler loops: as one launch / by the library's choice, and evaluation by evaluation
    sw = _lib.SAMPLE_STEPWISE
    loop_shapes = [(2, W), (3, 31)] if long else [(3, 2), (67, W), (513, W)]
    loop_plans = [0, _lib.PLAN_FUSED] if (precision == "bf16" and not long) else [0]
    for fl in loop_plans:
        for B, t in loop_shapes:
            for step in (0, sw):
                for smp in ("ddim", "euler", "heun"):
                    cases.append(dict(entry="sample", sampler=smp, B=B, t=t, flags=fl | step, sigmas=_SIG3))
                cases.append(dict(entry="ancestral", B=B, t=t, flags=fl | step, sigmas=_SIG3))
            for sol in _lib.SOLVER_IDS:
                # three steps at LMS order 4: slabs of `hist` nobody has written exist while the loop runs
                cases.append(dict(entry="solver", solver=sol, order=4, B=B, t=t, flags=fl, sigmas=_SIG3))
            for order, sig in ((1, (1.0, 0.0)), (2, (1.0, 0.0)), (3, (1.0, 0.2, 0.0))):          # fewer steps than the order
                cases.append(dict(entry="solver", solver="lms", order=order, B=B, t=t, flags=fl, sigmas=sig))
            for sol in ("dpmpp_2m", "lms"):                                   # five steps: the history turns over; both forms
                cases.append(dict(entry="solver", solver=sol, order=4, B=B, t=t, flags=fl, sigmas=_SIG5))
                cases.append(dict(entry="solver", solver=sol, order=4, B=B, t=t, flags=fl | sw, sigmas=_SIG3))
        for B, t in loop_shapes[:2]:                                          # guided loops
            cases.append(dict(entry="sample", sampler="heun", B=B, t=t, flags=fl, sigmas=_SIG3, lam=2.0))
            cases.append(dict(entry="ancestral", B=B, t=t, flags=fl, sigmas=_SIG3, lam=2.0))
            cases.append(dict(entry="solver", solver="lms", order=4, B=B, t=t, flags=fl, sigmas=_SIG3, lam=2.0))
            cases.append(dict(entry="solver", solver="dpmpp_2m", order=4, B=B, t=t, flags=fl, sigmas=_SIG3, lam=0.0))
    # D. one schedule of more than kMaxLoopEvals evaluations: the 2M / LMS state crosses from one launch to the next (one config)
    if (cfg_name, precision) == ("kitchen", "bf16"):
        n = _const("kMaxLoopEvals") + 2
        sig = tuple(float(v) for v in np.exp(np.linspace(0.0, np.log(0.02), n))) + (0.0,)
        for sol in ("dpmpp_2m", "lms"):
            for B in (5, 67):
                cases.append(dict(entry="solver", solver=sol, order=4, B=B, t=W, flags=_lib.PLAN_FUSED, sigmas=sig))
    return cases


# ------------------------------------------------------------------------------------------------ Test 1 (+ Test 5's forward half)
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision", _SHIPPED)
def test_forwards_samplers_and_solvers_do_not_depend_on_what_their_buffers_held(cfg_name, precision):
    """beso_score_fwd, beso_denoise_fwd, beso_sample (ddim / euler / heun, loop and stepwise), beso_sample_ancestral and
    beso_sample_solver (six solvers; LMS orders 1 ... 4 with fewer steps than the order) through the C ABI with the workspace, the
    output / in-out sample and the `hist` slabs pre-filled, guard bands of PAD bytes around each of them and around every input:
    the result is finite, bit-identical under the three fills, no element of it still carries the fill, and no guard byte
    changed (the sentinel check of test_no_writes_outside_output_and_workspace for the entry points that test leaves out)."""
    cases = _forward_cases(cfg_name, precision)
    failures = _check_across_fills(cfg_name, precision, cases)
    print(f"[buffers] {cfg_name} {precision}: {len(cases)} cases x {len(FILLS)} fills, {len(failures)} failures")
    assert not failures, "\n".join(failures[:40]) + (f"\n... and {len(failures) - 40} more" if len(failures) > 40 else "")


# ------------------------------------------------------------------------------------------------ Test 2
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision", _SHIPPED + [(c, p) for c in ("generic_96", "generic_256") for p in ("fp32", "bf16")])
def test_forward_does_not_depend_on_what_the_packed_buffer_held(cfg_name, precision):
    """The packed buffer pre-filled before beso_pack_weights, then forwards at (3, 2) and (67, W) under every plan of the shape:
    bit-identical outputs.  A difference is a kernel reading an inter-section gap or a pad the packers do not write (see the
    module docstring for the part of small.hip's former over-read this reaches).  (Rows 3 D .. Nqkv of w_qkv -- all the image's
    memset owns once q, k and v are packed -- are out of reach by value: their products are output columns nobody stores.)"""
    from beso_amd.runtime import PackedWeights
    cfg, _, inner, rt = _env(cfg_name, precision)
    lib = rt.lib
    nbytes = lib.beso_packed_bytes(C.byref(rt.cfg), rt.precision)
    assert nbytes > 0
    W = cfg.obs_seq_len
    shapes = [(3, 2), (2, W)] if cfg_name == "long_horizon" else [(3, 2), (67, W)]
    plans = _plans(cfg_name if cfg_name in O.CONFIGS else "tiny", precision)
    outs, failures = {}, []
    for name, byte in FILLS.items():
        buf = Guarded(nbytes, byte)
        image = buf.big[PAD:PAD + nbytes]
        packed = rt.pack(list(inner.parameters()), into=PackedWeights(image, rt.precision, None))
        assert packed.buf.data_ptr() == buf.ptr
        for B, t in shapes:
            s, g, a, sg, _ = _inputs(cfg_name, B, t)
            for lam in (1.0, 2.0):
                wsb = lib.beso_workspace_bytes(C.byref(rt.cfg), B, t, rt.precision, int(lam != 1.0))
                ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
                for fl in plans:
                    out = torch.zeros_like(a)
                    st = lib.beso_denoise_fwd(C.byref(rt.cfg), buf.ptr, rt.precision, s.data_ptr(), a.data_ptr(),
                                              g.data_ptr() if inner.goal_seq_len > 0 else None, sg.data_ptr(), out.data_ptr(), B, t,
                                              fl, lam, ws.data_ptr(), wsb, _stream())
                    key = (B, t, lam, hex(fl))
                    if st != 0:
                        failures.append(f"{key} fill {name}: status {st}")
                        continue
                    if not bool(torch.isfinite(out).all()):
                        failures.append(f"{key} fill {name}: output not finite")
                    outs[(name,) + key] = out
        torch.cuda.synchronize()
        if not bool(buf.guards_ok()):
            failures.append(f"fill {name}: beso_pack_weights wrote outside the image")
    for k, ref in outs.items():
        if k[0] != "ZERO":
            continue
        for name in ("NAN", "HUGE"):
            got = outs.get((name,) + k[1:])
            if got is not None and not torch.equal(ref, got):
                failures.append(f"{k[1:]}: output with the image over {name} differs from ZERO in {int((ref != got).sum())} elements")
    assert not failures, "\n".join(failures[:40])


# ------------------------------------------------------------------------------------------------ Test 3
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,precision,big,lam", [("kitchen", "bf16", 700, 1.0), ("kitchen", "fp32", 700, 1.0),
                                                       ("block_push", "bf16", 600, 2.0), ("long_horizon", "bf16", 40, 1.0)])
def test_a_small_call_after_a_large_one_equals_a_fresh_modules(cfg_name, precision, big, lam):
    """GCDenoiser / ScoreNetRuntime as shipped (grow-only workspace, torch.empty, no fills): a B = 3, t = 2 call that runs inside
    what a large call left behind gives the bits of a fresh module's; the same for fused_sampler('lms', order=4) after a larger
    dpmpp_2m call.  Under the library's own plan and under BESO_PLAN_FUSED."""
    from beso_amd.runtime import plan
    cfg = O.CONFIGS[cfg_name]
    w = O.make_weights(cfg, seed=4, std=0.03)
    T = lambda B, t, seed: tuple(to_dev(v) for v in O.make_inputs(cfg, B, seed=seed, t=t))
    sig = torch.tensor(_SIG3)

    def denoise(m, s, g, a, sg):
        inner = m.inner_model
        return inner.runtime(cfg.sigma_data).denoise(inner.packed_weights(), s, a, g, sg, cond_lambda=lam)

    for hint in (0, _lib.PLAN_FUSED):
        with plan(forward=hint), torch.no_grad():
            s3, g3, a3 = T(3, 2, 11)
            sg3 = to_dev(np.array([0.2, 0.5, 0.8], dtype=np.float32))
            fresh = make_denoiser(cfg, w, precision)
            ref = denoise(fresh, s3, g3, a3, sg3).clone()
            ref_lms = fresh.fused_sampler("lms", s3, a3, g3, sig, cond_lambda=lam, order=4).clone()
            used = make_denoiser(cfg, w, precision)
            sb, gb, ab = T(big, cfg.obs_seq_len, 12)
            denoise(used, sb, gb, ab, to_dev(np.linspace(0.1, 0.9, big).astype(np.float32)))
            got = denoise(used, s3, g3, a3, sg3)
            assert torch.isfinite(got).all() and torch.equal(got, ref), (cfg_name, precision, hex(hint), "denoise after a large call")
            used.fused_sampler("dpmpp_2m", sb, ab, gb, torch.tensor(_SIG5), cond_lambda=lam)
            got = used.fused_sampler("lms", s3, a3, g3, sig, cond_lambda=lam, order=4)
            assert torch.isfinite(got).all() and torch.equal(got, ref_lms), (cfg_name, precision, hex(hint), "lms after a larger dpmpp_2m")


# ------------------------------------------------------------------------------------------------ Test 4
class _PoisonedTorch:
    """Stands in for the `torch` name of beso_amd.training, and of beso_amd.runtime whose workspace() allocates the step's
    workspace: torch.empty / empty_like hand out memory that is `byte` everywhere -- the workspace, the fresh gradient buffer,
    the loss scalar, denoised / x_grad / dot."""

    def __init__(self, byte):
        self._byte = byte

    def __getattr__(self, name):
        return getattr(torch, name)

    def _fill(self, t):
        t.reshape(-1).view(torch.uint8).fill_(self._byte)
        return t

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


def _between_fill(x, byte):
    """x as a view into a larger allocation that is `byte` in front of and behind it (payload at the start of the guard band's end)"""
    return Guarded(x.numel() * 4, byte, x).f32().view(x.shape)


def _bounds(precision):
    """(loss, per tensor, _grad_errors floor): the bounds of test_hip_loss_and_gradients_match_autograd"""
    return (2e-5, 1e-4, 1e-4) if precision == "fp32" else (2e-3, 2.6e-2, 2e-3)


def _split(flat, params):
    out, off = [], 0
    for p in params:
        out.append(flat[off:off + p.numel()].view_as(p))
        off += p.numel()
    return out


_TRAIN_CASES = [
    # cfg, B, t (None: W), module kwargs, run kwargs
    ("tiny", 5, None, {}, {}),
    ("kitchen", 48, None, {}, {}),
    ("kitchen", 200, None, {}, {}),
    ("block_push", 40, None, {}, {}),
    ("tiny_mlp_head", 9, None, {}, {}),
    ("kitchen", 48, None, dict(attn_pdrop=0.3, resid_pdrop=0.1, embed_pdrop=0.1), {}),
    ("kitchen", 48, None, {}, dict(last_action_only=True)),
    ("kitchen", 48, None, {}, dict(goal_drop=0.25)),
    ("kitchen", 37, 2, {}, {}),
    ("hd4", 5, None, {}, {}),
]


def _train_step_runs(cfg_name, B, t, precision, mkw, rkw, monkeypatch, modes=("none", "early", "both")):
    from beso_amd import runtime, training
    from beso_amd.training import HipTrainStep
    cfg = _CFGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, train=True, **mkw)
    step = HipTrainStep(m.inner_model, float(cfg.sigma_data))
    params = list(m.inner_model.parameters())
    raw = train_inputs(cfg, B, seed=1)
    if t is not None:
        raw = tuple(v[:, :t].contiguous() if i in (0, 1, 3) else v for i, v in enumerate(raw))
    early, lossq = torch.cuda.Stream(), torch.cuda.Stream()
    ltol, gtol, floor = _bounds(precision)
    failures, ref = [], None
    for name, byte in FILLS.items():
        inputs = tuple(_between_fill(v, byte) for v in raw)
        for mode in modes:
            step._ws = None                                     # a fresh, pre-filled workspace every time
            with monkeypatch.context() as mp:
                mp.setattr(training, "torch", _PoisonedTorch(byte))
                mp.setattr(runtime, "torch", _PoisonedTorch(byte))
                loss, flat, _ = step.run(*inputs, seed=1234, fresh_grads=True, early_stream=early if mode != "none" else None,
                                         loss_stream=lossq if mode == "both" else None, **rkw)
            torch.cuda.synchronize()
            tag = f"{cfg_name} B={B} t={t} {precision} {mkw} {rkw} fill {name} streams {mode}"
            got = _split(flat, params)
            if not (torch.isfinite(loss).all() and torch.isfinite(flat).all()):
                failures.append(f"{tag}: loss {loss.item()} / {int((~torch.isfinite(flat)).sum())} gradient entries not finite")
                continue
            if ref is None:
                ref = (loss.item(), [g.clone() for g in got])   # ZERO, no side streams
                continue
            le = abs(loss.item() - ref[0]) / abs(ref[0])
            errs = grad_errors(got, ref[1], floor)
            print(f"[buffers] {tag}: loss {le:.2e}, worst gradient {max(errs):.2e}")
            if not le < ltol:
                failures.append(f"{tag}: loss differs from the ZERO run by {le:.3e} (bound {ltol})")
            if not max(errs) < gtol:
                failures.append(f"{tag}: gradient tensor {int(np.argmax(errs))} differs from the ZERO run by {max(errs):.3e} (bound {gtol})")
    return m, step, raw, ref, failures


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg_name,B,t,mkw,rkw", _TRAIN_CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, str) else v)
def test_training_step_does_not_depend_on_what_its_buffers_held(cfg_name, B, t, mkw, rkw, precision, monkeypatch):
    """HipTrainStep.run(fresh_grads=True) -- beso_loss_grad_streams without side streams, with the early stream, with the early
    and the loss stream -- with the workspace, the flat gradient buffer and the loss scalar starting as each fill and the inputs
    between bands of it.  The step accumulates bias / LayerNorm / loss cells with fp32 atomics, so it is not bit-reproducible:
    loss and gradients are finite and agree with the ZERO run within the bounds of test_hip_loss_and_gradients_match_autograd
    (poison of 1e36 or NaN in ONE accumulator cell breaks them by thirty orders of magnitude).  hd4 (D = 32, H = 8): the shape whose
    attention backward used to start a 16-byte load 8 bytes in front of the head's row; also held to autograd here."""
    m, step, raw, ref, failures = _train_step_runs(cfg_name, B, t, precision, mkw, rkw, monkeypatch)
    assert not failures, "\n".join(failures)
    if cfg_name == "hd4":
        from autograd_reference import loss_autograd
        state, action, goal, noise, sigma = raw
        ref_loss = loss_autograd(m, state, action, goal, noise.clone(), sigma)
        ref_loss.backward()
        ltol, gtol, floor = _bounds(precision)
        assert abs(ref[0] - ref_loss.item()) < ltol * abs(ref_loss.item())
        errs = grad_errors(ref[1], [p.grad for p in m.inner_model.parameters()], floor)
        assert max(errs) < gtol, errs


@pytest.mark.gpu
def test_training_step_kitchen_1030_one_launch_forward_plus_tail_block(monkeypatch):
    """kitchen B = 1030 in bf16: the one-launch forward with a last, partly filled workgroup"""
    _, _, _, _, failures = _train_step_runs("kitchen", 1030, None, "bf16", {}, {}, monkeypatch, modes=("none", "both"))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_a_small_training_step_after_a_large_one_equals_a_fresh_steps(precision):
    """The stale-state form, no fills: B = 200 with other data, then B = 37 on the same HipTrainStep (the workspace only grows)
    against a fresh step object, within the same bounds."""
    from beso_amd.training import HipTrainStep
    cfg = O.KITCHEN
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, train=True)
    params = list(m.inner_model.parameters())
    used, fresh = HipTrainStep(m.inner_model, float(cfg.sigma_data)), HipTrainStep(m.inner_model, float(cfg.sigma_data))
    small = train_inputs(cfg, 37, seed=8)
    loss_f, flat_f, _ = fresh.run(*small, seed=5, fresh_grads=True)
    used.run(*train_inputs(cfg, 200, seed=7), seed=6, fresh_grads=True)
    ws_before = used._ws.data_ptr()
    loss_u, flat_u, _ = used.run(*small, seed=5, fresh_grads=True)
    torch.cuda.synchronize()
    assert used._ws.data_ptr() == ws_before                    # the small step ran inside the large one's workspace
    ltol, gtol, floor = _bounds(precision)
    assert torch.isfinite(flat_u).all() and abs(loss_u.item() - loss_f.item()) < ltol * abs(loss_f.item())
    errs = grad_errors(_split(flat_u, params), _split(flat_f, params), floor)
    assert max(errs) < gtol, max(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B,precision", [("tiny", 5, "fp32"), ("tiny", 5, "bf16"), ("kitchen", 48, "bf16"), ("kitchen", 48, "fp32"),
                                                  ("block_push", 40, "bf16"), ("tiny_mlp_head", 9, "fp32"), ("hd4", 5, "bf16")])
def test_denoise_vjp_does_not_depend_on_what_its_buffers_held(cfg_name, B, precision, monkeypatch):
    """GCDenoiser.denoise_vjp with the workspace, denoised, x_grad and dot starting as each fill.  It has no weight gradients and
    no atomics: where two ZERO runs are bit-equal (checked first), the three fills must be bit-equal too; otherwise they agree
    within the training bounds."""
    from beso_amd import runtime, training
    cfg = _CFGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision)
    state, x, goal, cot, sigma = train_inputs(cfg, B, seed=2)
    step_of = lambda: m._train_steps[float(cfg.sigma_data)]

    def run(byte):
        ins = tuple(_between_fill(v, byte) for v in (state, x, goal, sigma, cot))
        if m._train_steps:
            step_of()._ws = None
        with monkeypatch.context() as mp:
            mp.setattr(training, "torch", _PoisonedTorch(byte))
            mp.setattr(runtime, "torch", _PoisonedTorch(byte))
            out = m.denoise_vjp(*ins)
        torch.cuda.synchronize()
        return [o.clone() for o in out]

    z0, z1 = run(0x00), run(0x00)
    exact = all(torch.equal(a, b) for a, b in zip(z0, z1))
    print(f"[buffers] denoise_vjp {cfg_name} {precision}: two ZERO runs bit-equal: {exact}")
    _, gtol, _ = _bounds(precision)
    for name in ("NAN", "HUGE"):
        got = run(FILLS[name])
        for what, a, b in zip(("denoised", "x_grad", "dot"), z0, got):
            assert torch.isfinite(b).all(), (name, what)
            assert not bool(_carries_fill(b, FILLS[name])), (name, what)
            if exact:
                assert torch.equal(a, b), (name, what, float((a - b).abs().max()))
            else:
                assert float((a - b).norm() / a.norm()) < gtol, (name, what)


# ------------------------------------------------------------------------------------------------ Test 5 (training half)
@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B,precision", [("tiny", 5, "fp32"), ("kitchen", 48, "bf16"), ("tiny_mlp_head", 9, "bf16"),
                                                  ("block_push", 40, "fp32")])
def test_no_writes_outside_the_training_steps_buffers(cfg_name, B, precision):
    """beso_loss_grad, beso_loss_grad_overlap (with its early stream) and beso_denoise_vjp through the C ABI: the gradient buffer
    of beso_grad_floats, the loss cell, denoised / x_grad / dot and the workspace of beso_train_workspace_bytes sit between guard
    bands of each fill; nothing outside [ptr, ptr + size) changes, every result is finite and within the training bounds of
    the ZERO run."""
    cfg = _CFGS[cfg_name]
    m = make_denoiser(cfg, O.make_weights(cfg, seed=3, std=0.06), precision, train=True)
    inner, lib = m.inner_model, _lib.load()
    ccfg = inner.shape(float(cfg.sigma_data)).c_struct()
    params = [p.detach() for p in inner.parameters()]
    arr = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
    prec = _lib.PRECISIONS[precision]
    state, action, goal, noise, sigma = train_inputs(cfg, B, seed=1)
    t = state.shape[1]
    n_grad = int(lib.beso_grad_floats(C.byref(ccfg)))
    wsb = int(lib.beso_train_workspace_bytes(C.byref(ccfg), B, t, prec))
    assert n_grad == sum(p.numel() for p in params) and wsb > 0
    early = torch.cuda.Stream()
    ltol, gtol, floor = _bounds(precision)
    ref, ref_vjp = None, None
    for name, byte in FILLS.items():
        ins = [Guarded(v.numel() * 4, byte, v) for v in (state, action, goal, noise, sigma)]
        gp = ins[2].ptr if inner.goal_seq_len > 0 else None
        for entry in ("beso_loss_grad", "beso_loss_grad_overlap"):
            grads, loss, ws = Guarded(4 * n_grad, byte), Guarded(4, byte), Guarded(wsb, byte)
            args = (C.byref(ccfg), arr, len(params), grads.ptr, prec, ins[0].ptr, ins[1].ptr, gp, ins[3].ptr, ins[4].ptr, loss.ptr,
                    B, t, 0, 0.0, 0.0, 0.0, 0.0, C.c_uint(77), 1.0, ws.ptr, wsb, _stream())
            if entry == "beso_loss_grad":
                _lib.check(lib.beso_loss_grad(*args), entry)
            else:
                early.wait_stream(torch.cuda.current_stream())
                _lib.check(lib.beso_loss_grad_overlap(*args, C.c_void_p(early.cuda_stream)), entry)
            torch.cuda.synchronize()
            for what, gd in (("gradients", grads), ("loss", loss), ("workspace", ws), ("state", ins[0]), ("action", ins[1]),
                             ("goal", ins[2]), ("noise", ins[3]), ("sigma", ins[4])):
                assert bool(gd.guards_ok()), (entry, name, what)
            flat, lv = grads.f32().clone(), float(loss.f32()[0])
            assert np.isfinite(lv) and torch.isfinite(flat).all(), (entry, name)
            if ref is None:
                ref = (lv, _split(flat, params))
                continue
            assert abs(lv - ref[0]) < ltol * abs(ref[0]), (entry, name, lv, ref[0])
            errs = grad_errors(_split(flat, params), ref[1], floor)
            assert max(errs) < gtol, (entry, name, max(errs))
        # the input VJP: x = action, cotangent = noise
        n_out = action.numel() * 4
        den, dx, dot, ws = Guarded(n_out, byte), Guarded(n_out, byte), Guarded(4 * B, byte), Guarded(wsb, byte)
        _lib.check(lib.beso_denoise_vjp(C.byref(ccfg), arr, len(params), prec, ins[0].ptr, ins[1].ptr, gp, ins[4].ptr, ins[3].ptr,
                                        den.ptr, dx.ptr, dot.ptr, B, t, 0, ws.ptr, wsb, _stream()), "beso_denoise_vjp")
        torch.cuda.synchronize()
        for what, gd in (("denoised", den), ("x_grad", dx), ("dot", dot), ("workspace", ws)):
            assert bool(gd.guards_ok()), ("beso_denoise_vjp", name, what)
        got = [den.f32().clone(), dx.f32().clone(), dot.f32().clone()]
        assert all(torch.isfinite(v).all() for v in got) and not any(bool(_carries_fill(v, byte)) for v in got), name
        if ref_vjp is None:
            ref_vjp = got
        else:
            for what, a, b in zip(("denoised", "x_grad", "dot"), ref_vjp, got):
                assert float((a - b).norm() / a.norm()) < gtol, ("beso_denoise_vjp", name, what)
