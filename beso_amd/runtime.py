"""Host-side runtime over the C ABI (include/beso_hip.h): packed-weight images, workspaces and the
denoise / sample calls.  PyTorch is used only for device memory and streams.

Nothing here computes the network on the CPU or with torch ops: if the HIP library is missing the
constructor raises (``beso_amd._lib.load``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib

_hints = threading.local()


@contextlib.contextmanager
def plan(forward: int = 0, train: int = 0):
    """Execution-plan hints for the library calls the CALLING THREAD makes inside the block: ``forward`` = BESO_PLAN_* bits
    (``_lib.PLAN_PER_OP``, ``PLAN_BLOCKS``, ``PLAN_SMALL``, ``PLAN_FUSED``, ``PLAN_SPW2 / 4 / 8``, ``PLAN_SIGMA_SHARED`` /
    ``PLAN_SIGMA_PRIVATE``: the sigma token shared across a uniform-sigma kitchen batch at any batch size / never) added to the flags of every forward / sampler call,
    ``train`` = ``_lib.TRAIN_PLAN_PER_OP`` / ``TRAIN_PLAN_TILES`` for ``beso_loss_grad``.  They select WHICH kernels run,
    never what is computed (parity tests: per-op kernels against the fused ones; measurements); each library call carries
    its own flags, so nothing process-wide changes."""
    old = (getattr(_hints, "forward", 0), getattr(_hints, "train", 0))
    _hints.forward, _hints.train = forward, train
    try:
        yield
    finally:
        _hints.forward, _hints.train = old


def set_plan(forward: Optional[int] = None, train: Optional[int] = None) -> None:
    """The same hints without a block: they stay with the calling thread until set again (0 = the library's own choice;
    ``forward`` takes every BESO_PLAN_* bit, ``_lib.PLAN_SIGMA_SHARED`` / ``PLAN_SIGMA_PRIVATE`` included)."""
    if forward is not None:
        _hints.forward = forward
    if train is not None:
        _hints.train = train


def forward_hints() -> int:
    return getattr(_hints, "forward", 0)


def train_hints() -> int:
    return getattr(_hints, "train", 0)


@dataclass(frozen=True)
class ScoreNetShape:
    """The kwargs of DiffusionGPT.__init__ that shape the computation (score_gpts.py:121-139)."""
    obs_dim: int
    act_dim: int
    embed_dim: int
    n_layers: int
    n_heads: int
    goal_seq_len: int      # effective: 0 when not goal conditioned (score_gpts.py:143-144)
    obs_seq_len: int
    linear_output: bool = True
    sigma_data: float = 1.0

    def c_struct(self) -> _lib.BesoConfig:
        return _lib.BesoConfig(self.obs_dim, self.act_dim, self.embed_dim, self.n_layers, self.n_heads,
                               self.goal_seq_len, self.obs_seq_len, int(self.linear_output), float(self.sigma_data))

    def tokens(self, t: int) -> int:
        return 1 + self.goal_seq_len + 2 * t

    def flops_per_sample(self, t: Optional[int] = None) -> int:
        """Algorithmic FLOPs of one score-net forward per sample."""
        t = self.obs_seq_len if t is None else t
        D, L, G, T = self.embed_dim, self.n_layers, self.goal_seq_len, self.tokens(t)
        return (L * (24 * T * D * D + 4 * T * T * D)
                + 2 * D * (t * self.obs_dim + G * self.obs_dim + t * self.act_dim + 1) + 2 * t * D * self.act_dim)


class PackedWeights:
    """A kernel-ready image of one set of parameter values (K0 of SURVEY.md 2.1)."""

    def __init__(self, buf: torch.Tensor, precision: int, key):
        self.buf = buf
        self.precision = precision
        self.key = key


def stream_ptr(device=None) -> int:
    """The current stream of ``device`` as the ``void* stream`` of the C ABI."""
    return torch.cuda.current_stream(device).cuda_stream


def train_precision(name: str) -> int:
    """The ``_lib.PREC_*`` a training step (``beso_loss_grad``, ``beso_denoise_vjp``) runs in for a model of precision
    ``name``: the split-bf16 and fp16 modes are inference instances of the fused kernel; their steps are the fp32 / bf16 ones."""
    return _lib.PRECISIONS[{"bf16x3": "fp32", "fp16": "bf16"}.get(name, name)]


def workspace(owner, need: int, device) -> torch.Tensor:
    """The grow-only scratch buffer ``owner._ws``: kept while it holds ``need`` bytes on ``device``, else released and
    allocated anew."""
    ws = owner._ws
    if ws is None or ws.numel() < need or ws.device != device:
        owner._ws = ws = None
        owner._ws = ws = torch.empty(int(need), dtype=torch.uint8, device=device)
    return ws


def _f32c(x: torch.Tensor, device) -> torch.Tensor:
    if x.device != device or x.dtype != torch.float32:
        x = x.to(device=device, dtype=torch.float32)
    return x.contiguous()


def prepare_inputs(state, action, goal, sigma, obs_dim: int, act_dim: int, goal_seq_len: int, device=None):
    """The tensors a forward / training call hands to the library, from what the reference's callers pass: contiguous fp32 on
    ``device`` (default: the action's), ``state`` [B,t,obs], ``action`` (or x, x_t) [B,t,act], ``goal`` [B,G,obs] -- given as
    that, as [1,G,obs] or as [G,obs]; None when the model takes no goals (``goal_seq_len`` 0), whatever was passed -- and
    ``sigma`` [B] from B values or one (None stays None).  Any other shape is a ValueError.  Works on any device: what must be
    on the GPU, and what stands in for a missing input, is the caller's."""
    if state.dim() != 3 or action.dim() != 3:
        raise ValueError("state must be [B,t,obs] and action [B,t,act]")
    B, t, _ = state.shape
    if action.shape[0] != B or action.shape[1] != t or action.shape[2] != act_dim:
        raise ValueError(f"action shape {tuple(action.shape)} does not match state {tuple(state.shape)}")
    if state.shape[2] != obs_dim:
        raise ValueError(f"state feature dim {state.shape[2]} != obs_dim {obs_dim}")
    device = action.device if device is None else device
    state = _f32c(state, device)
    action = _f32c(action, device)
    if goal_seq_len > 0:
        if goal is None:
            raise ValueError("goal is required for a goal-conditioned model")
        if goal.dim() == 2:
            goal = goal.unsqueeze(0)
        if goal.dim() == 3 and goal.shape[0] == 1 and B > 1:
            goal = goal.expand(B, -1, -1)
        if tuple(goal.shape) != (B, goal_seq_len, obs_dim):
            raise ValueError(f"goal shape {tuple(goal.shape)} != {(B, goal_seq_len, obs_dim)}")
        goal = _f32c(goal, device)
    else:
        goal = None
    if sigma is not None:
        sigma = _f32c(sigma.reshape(-1), device)
        if sigma.numel() == 1 and B > 1:
            sigma = sigma.expand(B).contiguous()
        if sigma.numel() != B:
            raise ValueError(f"sigma must have {B} entries, got {sigma.numel()}")
    return state, action, goal, sigma


class ScoreNetRuntime:
    """Binds one model shape to the HIP library: pack weights, run GCDenoiser.forward /
    DiffusionGPT.forward / whole sampling loops on the current CUDA(HIP) stream."""

    def __init__(self, shape: ScoreNetShape, precision: str = "bf16"):
        self.lib = _lib.load()
        self.shape = shape
        self.cfg = shape.c_struct()
        self.set_precision(precision)
        self.n_params = self.lib.beso_num_params(C.byref(self.cfg))
        if self.n_params <= 0:
            raise ValueError(f"beso_hip: unsupported model shape {shape}")
        self._ws: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ configuration
    def set_precision(self, precision: str) -> None:
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}; choose from {sorted(_lib.PRECISIONS)}")
        self.precision_name = precision
        self.precision = _lib.PRECISIONS[precision]

    # ------------------------------------------------------------------ weights
    def pack(self, params: Sequence[torch.Tensor], key=None, into: Optional[PackedWeights] = None) -> PackedWeights:
        """``params`` in the order of the reference module's ``named_parameters()``; CUDA fp32."""
        params = [p.detach() for p in params]
        if len(params) != self.n_params:
            raise ValueError(f"expected {self.n_params} parameter tensors, got {len(params)}")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("beso_amd: parameters must live on the GPU (no CPU path)")
        keep = [_f32c(p, dev) for p in params]
        nbytes = self.lib.beso_packed_bytes(C.byref(self.cfg), self.precision)
        if nbytes == 0:
            raise ValueError(f"beso_hip: precision {self.precision_name!r} unsupported for this shape")
        if into is not None and into.buf.numel() == nbytes and into.buf.device == dev and into.precision == self.precision:
            buf = into.buf
        else:
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        arr = (C.c_void_p * len(keep))(*[p.data_ptr() for p in keep])
        with torch.cuda.device(dev):
            st = self.lib.beso_pack_weights(C.byref(self.cfg), arr, len(keep), buf.data_ptr(), nbytes,
                                            self.precision, stream_ptr(dev))
        _lib.check(st, "pack_weights")
        if into is not None and buf is into.buf:
            into.key = key
            return into
        return PackedWeights(buf, self.precision, key)

    # ------------------------------------------------------------------ workspace
    def _workspace(self, batch: int, t: int, two: bool, dev) -> torch.Tensor:
        need = self.lib.beso_workspace_bytes(C.byref(self.cfg), batch, t, self.precision, int(two))
        if need == 0:
            raise ValueError(f"beso_hip: bad shape batch={batch} t={t} (t must be in [1, {self.shape.obs_seq_len}])")
        return workspace(self, need, dev)

    # ------------------------------------------------------------------ forward calls
    def _prep(self, state, action, goal, sigma):
        dev = action.device
        if dev.type != "cuda":
            raise RuntimeError("beso_amd: the score-denoising path runs on the GPU only (no CPU fallback); "
                               "move the inputs to the MI355X")
        state, action, goal, sigma = prepare_inputs(state, action, goal, sigma, self.shape.obs_dim, self.shape.act_dim,
                                                    self.shape.goal_seq_len, dev)
        B, t, _ = state.shape
        return dev, B, t, state, action, goal, sigma

    def denoise(self, packed: PackedWeights, state, action, goal, sigma, uncond: bool = False,
                cond_lambda: float = 1.0, precondition: bool = True) -> torch.Tensor:
        """GCDenoiser.forward (precondition=True) or DiffusionGPT.forward (False)."""
        dev, B, t, state, action, goal, sigma = self._prep(state, action, goal, sigma)
        two = precondition and (not uncond) and cond_lambda not in (0.0, 1.0)
        ws = self._workspace(B, t, two, dev)
        out = torch.empty((B, t, self.shape.act_dim), dtype=torch.float32, device=dev)
        gp = goal.data_ptr() if goal is not None else None
        flags = (_lib.FLAG_UNCOND if uncond else 0) | forward_hints()
        with torch.cuda.device(dev):
            if precondition:
                st = self.lib.beso_denoise_fwd(C.byref(self.cfg), packed.buf.data_ptr(), packed.precision,
                                               state.data_ptr(), action.data_ptr(), gp, sigma.data_ptr(),
                                               out.data_ptr(), B, t, flags, float(cond_lambda), ws.data_ptr(),
                                               ws.numel(), stream_ptr(dev))
            else:
                st = self.lib.beso_score_fwd(C.byref(self.cfg), packed.buf.data_ptr(), packed.precision,
                                             state.data_ptr(), action.data_ptr(), gp, sigma.data_ptr(),
                                             out.data_ptr(), B, t, flags, ws.data_ptr(), ws.numel(),
                                             stream_ptr(dev))
        _lib.check(st, "denoise_fwd" if precondition else "score_fwd")
        return out

    def loss(self, packed: PackedWeights, state, action, goal, noise, sigma, uncond: bool = False, last_only: bool = False,
             per_sample: bool = False):
        """The gradient-free score-matching objective of the eval-mode network (``beso_loss_fwd``: GCDenoiser.loss under
        ``torch.no_grad()``, score_wrappers.py:45-79) on the weights of ``packed``: a 0-d tensor, or ``(loss, [B])`` with
        ``per_sample`` -- the mean of (F(c_in * noised) - target)^2 over every sample's values.  ``last_only`` scores the last
        step of every window only (the caller has zeroed the noise of the other steps, as GCDenoiser.loss does);
        ``uncond`` evaluates the unconditional branch.  Fixed-order reductions, no atomics."""
        if sigma is None:
            raise ValueError("sigma is required")
        dev, B, t, state, action, goal, sigma = self._prep(state, action, goal, sigma)
        if not torch.is_tensor(noise) or tuple(noise.shape) != tuple(action.shape):
            raise ValueError(f"noise must have the action's shape {tuple(action.shape)}")
        noise = _f32c(noise, dev)
        need = self.lib.beso_loss_fwd_workspace_bytes(C.byref(self.cfg), B, t, self.precision)
        if need == 0:
            raise ValueError(f"beso_hip: bad shape batch={B} t={t} (t must be in [1, {self.shape.obs_seq_len}])")
        ws = workspace(self, need, dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        rows = torch.empty(B, dtype=torch.float32, device=dev) if per_sample else None
        flags = (_lib.FLAG_UNCOND if uncond else 0) | (_lib.FLAG_LAST_ACTION_ONLY if last_only else 0) | forward_hints()
        with torch.cuda.device(dev):
            st = self.lib.beso_loss_fwd(C.byref(self.cfg), packed.buf.data_ptr(), packed.precision, state.data_ptr(),
                                        action.data_ptr(), goal.data_ptr() if goal is not None else None, noise.data_ptr(),
                                        sigma.data_ptr(), out.data_ptr(), rows.data_ptr() if rows is not None else None,
                                        B, t, flags, ws.data_ptr(), ws.numel(), stream_ptr(dev))
        _lib.check(st, "loss_fwd")
        return (out, rows) if per_sample else out

    def sample(self, packed: PackedWeights, sampler: str, state, x_t, goal, sigmas, cond_lambda: float = 1.0,
               eta: float = 1.0, s_noise: float = 1.0, order: int = 4, noise=None, stepwise: bool = False, trace=None):
        """One of the sampler loops of ``_lib.SAMPLERS`` (ddim / euler / heun with s_churn = 0, euler_ancestral, dpm_2,
        dpm_2_ancestral, dpmpp_2s, dpmpp_2s_ancestral, dpmpp_2m, lms of order 1 ... 4) as ONE enqueue of all steps -- one
        launch for the whole loop where the shape has the one-launch kernel; ``stepwise`` enqueues evaluation by evaluation
        instead (same arithmetic, bit-identical results).  ``eta`` is the ancestral samplers', ``s_noise``
        dpmpp_2s_ancestral's, ``order`` LMS's.  The ancestral samplers' noise [n_steps, B, t, act] is ``noise``, or drawn
        here by ``gc_sampling.predraw_noise`` (the draws of the Python loop, in its order).  The multistep state lives in a
        buffer of this call.

        ``trace``: a subset of {'x', 'denoised'}.  Non-empty, the same launches also record the trajectory
        (``beso_sample_traced``) and the return value is ``(x_0, {...})`` with the requested fp32 tensors: 'x'
        [n_steps + 1, B, t, act] -- x_T, then x after every completed step, the last one equal to x_0 -- and 'denoised'
        [n_steps, B, t, act], the denoised value of every step's first evaluation."""
        if sampler not in _lib.SAMPLERS:
            raise ValueError("desired sampler type not found!")
        entry, sid = _lib.SAMPLERS[sampler]
        trace = set(() if trace is None else ([trace] if isinstance(trace, str) else trace))
        if trace - {"x", "denoised"}:
            raise ValueError("trace must be a subset of {'x', 'denoised'}")
        if sampler == "lms" and not 1 <= int(order) <= 4:
            raise ValueError("beso_sample_solver runs LMS orders 1 ... 4")
        dev, B, t, state, x, goal, _ = self._prep(state, x_t, goal, None)
        if x.data_ptr() == x_t.data_ptr():
            x = x.clone()          # the loop updates x in place; keep the caller's x_T intact
        sig = [float(s) for s in (sigmas.detach().cpu().tolist() if torch.is_tensor(sigmas) else sigmas)]
        if not sampler.endswith("_ancestral"):
            noise = None
        elif noise is None:
            # (the draw rule is the sampler module's: imported here, where it is needed, as that module imports this one)
            from .agents.diffusion_agents.k_diffusion.gc_sampling import predraw_noise
            noise = predraw_noise(sampler, sig, x, eta)
        else:
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            if noise.shape != (len(sig) - 1,) + tuple(x.shape):
                raise ValueError("noise must be [len(sigmas) - 1, B, t, act]")
        n_hist = {"dpmpp_2m": 1, "lms": int(order) - 1}.get(sampler, 0)
        hist = torch.empty((n_hist,) + tuple(x.shape), dtype=torch.float32, device=dev) if n_hist else None
        ws = self._workspace(B, t, cond_lambda not in (0.0, 1.0), dev)
        arr = (C.c_float * len(sig))(*sig)
        head = (C.byref(self.cfg), packed.buf.data_ptr(), packed.precision)
        loop = (state.data_ptr(), goal.data_ptr() if goal is not None else None, x.data_ptr(), B, t, arr, len(sig),
                float(cond_lambda))
        nz = noise.data_ptr() if noise is not None else None
        flags = (_lib.SAMPLE_STEPWISE if stepwise else 0) | forward_hints()
        tail = (ws.data_ptr(), ws.numel(), stream_ptr(dev))
        if trace:
            n = len(sig) - 1
            out = {}
            if "x" in trace:
                out["x"] = torch.empty((n + 1,) + tuple(x.shape), dtype=torch.float32, device=dev)
            if "denoised" in trace:
                out["denoised"] = torch.empty((n,) + tuple(x.shape), dtype=torch.float32, device=dev)
            tx, td = out.get("x"), out.get("denoised")
            args = head + (_lib.ENTRY_IDS[entry], sid or 0) + loop + (
                float(eta), float(s_noise), int(order), nz, hist.data_ptr() if hist is not None else None,
                tx.data_ptr() if tx is not None else None, tx.numel() if tx is not None else 0,
                td.data_ptr() if td is not None else None, td.numel() if td is not None else 0, flags) + tail
            with torch.cuda.device(dev):
                st = self.lib.beso_sample_traced(*args)
            _lib.check(st, f"sample_traced[{sampler}]")
            return x, out
        if entry == "beso_sample":
            args = head + (sid,) + loop + (flags,) + tail
        elif entry == "beso_sample_ancestral":
            args = head + loop + (float(eta), nz, flags) + tail
        else:
            args = head + (sid,) + loop + (float(eta), float(s_noise), int(order), nz,
                                           hist.data_ptr() if hist is not None else None, flags) + tail
        with torch.cuda.device(dev):
            st = getattr(self.lib, entry)(*args)
        _lib.check(st, f"sample[{sampler}]")
        return x

    # ------------------------------------------------------------------ profiling hooks (bench.py)
    def profile_enable(self, site: str) -> None:
        self.lib.beso_profile_enable(_lib.SITES[site])

    def profile_read(self):
        ms, n = C.c_double(0.0), C.c_int(0)
        _lib.check(self.lib.beso_profile_read(C.byref(ms), C.byref(n)), "profile_read")
        return ms.value, n.value
