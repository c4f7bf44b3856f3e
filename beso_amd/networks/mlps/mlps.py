"""``MLPNetwork`` and ``ResidualMLPNetwork`` (reference: beso/networks/mlps/mlps.py:11-73 and :76-133, the latter over
networks/mlps/res_layers.py) on the HIP kernels of include/beso_mlp.h and include/beso_resmlp.h.

Same constructor kwargs, attributes, module tree and so ``state_dict`` keys (``layers.N.weight`` / ``layers.N.bias``;
``layers.N.l1.*`` / ``layers.N.l2.*`` / ``layers.N.normalizer.*`` for a residual block), ``get_params()`` and ``get_device()``.
``forward`` on GPU tensors is ONE launch (``beso_mlp_fwd`` / ``beso_resmlp_fwd``); under autograd it is a
``torch.autograd.Function`` whose backward is ``beso_mlp_bwd`` / ``beso_resmlp_bwd``.  CPU tensors raise: there is no torch-op
evaluation.  Of ``ResidualMLPNetwork``, BatchNorm, spectral norm and dropout masks have no kernel: the first two are refused at
construction, ``dropout > 0`` is the identity in ``eval()`` / under ``no_grad`` and raises in a differentiable training call."""
import ctypes as C

import torch
import torch.nn as nn

from ... import _lib

MAX_DIM, MAX_HIDDEN_LAYERS = 512, 4
MAX_RESIDUAL_LAYERS = 8            # num_hidden_layers of ResidualMLPNetwork: two per block, up to four blocks


def activation_id(activation: str, who: str = "MLPNetwork") -> int:
    """BESO_MLP_ACT_* of a name ``return_activiation_fcn`` knows (networks/utils.py:33-51).  ``"tanh"`` is nn.Sigmoid there
    (utils.py:37-38) and here.  The names without a kernel -- ``PReLU``, which is also that function's answer to every unknown
    name, and ``softmax`` -- are refused by name."""
    if activation in _lib.MLP_ACTIVATIONS:
        return _lib.MLP_ACTIVATIONS[activation]
    raise ValueError(f"{who}: activation {activation!r} has no HIP kernel (supported: "
                     f"{', '.join(sorted(_lib.MLP_ACTIVATIONS))})")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


class _MlpFunction(torch.autograd.Function):
    """y = net(x) for x [M, in]; the backward gives dx (only if x requires grad) and every parameter's gradient."""

    @staticmethod
    def forward(ctx, net, x, *params):
        y, keep = net.run_forward(x, keep=True, params=params)
        ctx.net, ctx.keep, ctx.params, ctx.rows = net, keep, params, x.shape[0]
        ctx.want_dx = ctx.needs_input_grad[1]
        return y

    @staticmethod
    def backward(ctx, dy):
        net, params = ctx.net, ctx.params
        flat = torch.empty(net.num_param_floats(), dtype=torch.float32, device=dy.device)
        dx = torch.empty(ctx.rows, net.input_dim, dtype=torch.float32, device=dy.device) if ctx.want_dx else None
        net.run_backward(ctx.keep, dy, flat, dx=dx, params=params)
        grads, off = [], 0
        for p in params:
            grads.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return (None, dx, *grads)


class _KernelNetwork(nn.Module):
    """What the two networks share: the reference's surface over ``self.layers`` and the calls of a library's three entry
    points ``<_entry>_workspace_bytes / _fwd / _bwd``.  A subclass gives ``_library()``, ``_entry``, ``dims()`` and
    ``keep_floats()``."""
    _entry = None

    # ------------------------------------------------------------------ the reference's surface
    def get_device(self, device: torch.device):
        self._device = device
        self.layers.to(device)

    def get_params(self):
        return self.layers.parameters()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [..., input_dim] -> [..., output_dim], the leading dimensions kept."""
        self._check_input(x)
        rows = x.reshape(-1, self.input_dim).to(torch.float32).contiguous()
        params = tuple(self.layers.parameters())
        if torch.is_grad_enabled() and (rows.requires_grad or any(p.requires_grad for p in params)):
            y = _MlpFunction.apply(self, rows, *params)
        else:
            y, _ = self.run_forward(rows, keep=False, params=params)
        return y.view(*x.shape[:-1], self.output_dim)

    # ------------------------------------------------------------------ the kernels
    def _call(self, what: str):
        return getattr(self._library(), f"{self._entry}_{what}")

    def num_param_floats(self) -> int:
        return sum(p.numel() for p in self.layers.parameters())

    def workspace_bytes(self, rows: int) -> int:
        return int(self._call("workspace_bytes")(C.byref(self.dims()), rows, 1))

    def _check_input(self, x):
        name = type(self).__name__
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError(f"{name} runs on the GPU only (HIP kernels, no CPU or eager fallback): got a "
                               f"{'CPU tensor' if isinstance(x, torch.Tensor) else type(x).__name__}")
        if x.shape[-1] != self.input_dim or x.numel() == 0:
            raise ValueError(f"{name}: input of shape {tuple(x.shape)}; the last dimension must be input_dim="
                             f"{self.input_dim} and there must be at least one row")

    def _pointers(self, params):
        params = tuple(self.layers.parameters()) if params is None else params
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"{type(self).__name__}: the parameters must be contiguous fp32 tensors on the GPU")
        return (C.c_void_p * len(params))(*[p.data_ptr() for p in params]), len(params)

    def run_forward(self, rows: torch.Tensor, keep: bool, params=None, out=None, keep_out=None):
        """The ``_fwd`` entry point on contiguous fp32 ``rows`` [M, input_dim] -> (y [M, output_dim], keep buffer or None).
        ``params``: the tensors to evaluate (default: the module's own; the agent passes the EMA shadow's)."""
        M = rows.shape[0]
        ptrs, n = self._pointers(params)
        y = torch.empty(M, self.output_dim, dtype=torch.float32, device=rows.device) if out is None else out
        if keep and keep_out is None:
            keep_out = torch.empty(self.keep_floats(M), dtype=torch.float32, device=rows.device)
        st = self._call("fwd")(ptrs, n, C.byref(self.dims()), rows.data_ptr(), M, y.data_ptr(),
                               keep_out.data_ptr() if keep else None, _stream(rows))
        _lib.check(st, self._entry + "_fwd")
        return y, (keep_out if keep else None)

    def run_backward(self, keep: torch.Tensor, dy: torch.Tensor, grads_flat: torch.Tensor, dx=None, accumulate=False,
                     params=None, workspace=None):
        """The ``_bwd`` entry point: the parameter gradients of the rows behind ``keep`` into ``grads_flat`` (written; added to
        with ``accumulate``), and the input gradient into ``dx`` [M, input_dim] when given."""
        dy = dy.reshape(-1, self.output_dim).to(torch.float32).contiguous()
        M = dy.shape[0]
        ptrs, n = self._pointers(params)
        need = self.workspace_bytes(M)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dy.device)
        st = self._call("bwd")(ptrs, n, C.byref(self.dims()), keep.data_ptr(), dy.data_ptr(), M,
                               None if dx is None else dx.data_ptr(), grads_flat.data_ptr(), workspace.data_ptr(),
                               workspace.numel() * workspace.element_size(),
                               _lib.MLP_FLAGS["accumulate"] if accumulate else 0, _stream(dy))
        _lib.check(st, self._entry + "_bwd")
        return grads_flat


def _check_ranges(who: str, checks, supported: str):
    for name, value, ok in checks:
        if not ok:
            raise ValueError(f"{who}: {name}={value} is outside what the HIP kernels support ({supported})")


class MLPNetwork(_KernelNetwork):
    """Linear(input_dim, hidden_dim), num_hidden_layers - 1 x Linear(hidden_dim, hidden_dim), Linear(hidden_dim, output_dim);
    the activation follows every layer but the last.  ``dropout`` and ``use_spectral_norm`` are stored and unused, exactly
    as in the reference's MLPNetwork (mlps.py:37-38: neither is read again)."""
    _entry = "beso_mlp"

    def __init__(self, input_dim: int, hidden_dim: int = 100, num_hidden_layers: int = 1, output_dim=1, dropout: int = 0,
                 activation: str = "ReLU", use_spectral_norm: bool = False, device: str = 'cuda'):
        super().__init__()
        self.network_type = "mlp"
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.num_hidden_layers = num_hidden_layers
        self.output_dim = output_dim
        self.dropout = dropout
        self.spectral_norm = use_spectral_norm
        self.activation = activation
        self.act_id = activation_id(activation)
        _check_ranges("MLPNetwork",
                      (("input_dim", input_dim, 1 <= input_dim <= MAX_DIM),
                       ("output_dim", output_dim, 1 <= output_dim <= MAX_DIM),
                       ("hidden_dim", hidden_dim, 16 <= hidden_dim <= MAX_DIM and hidden_dim % 16 == 0),
                       ("num_hidden_layers", num_hidden_layers, 1 <= num_hidden_layers <= MAX_HIDDEN_LAYERS)),
                      f"input_dim, output_dim in 1..{MAX_DIM}; hidden_dim a multiple of 16 up to {MAX_DIM}; num_hidden_layers in "
                      f"1..{MAX_HIDDEN_LAYERS}")
        self.layers = nn.ModuleList([nn.Linear(self.input_dim, self.hidden_dim)])
        self.layers.extend([nn.Linear(self.hidden_dim, self.hidden_dim) for _ in range(1, self.num_hidden_layers)])
        self.layers.append(nn.Linear(self.hidden_dim, self.output_dim))
        self._device = device
        self.layers.to(self._device)

    def _library(self):
        return _lib.load_mlp()

    def dims(self) -> _lib.MlpDims:
        return _lib.MlpDims(self.input_dim, self.hidden_dim, self.num_hidden_layers, self.output_dim, self.act_id)

    def keep_floats(self, rows: int) -> int:
        """Floats of the buffer a training forward fills for the backward: x and the hidden layers' pre-activations."""
        return rows * (self.input_dim + self.num_hidden_layers * self.hidden_dim)


class TwoLayerPreActivationResNetLinear(nn.Module):
    """The parameters of one residual block (res_layers.py:7-45), under the reference's names: ``l1``, ``l2`` and, with
    ``use_norm``, ONE ``normalizer`` that the block applies in front of both activations.  It holds no arithmetic: the block
    is evaluated inside ``beso_resmlp_fwd``."""

    def __init__(self, hidden_dim: int, use_norm: bool):
        super().__init__()
        self.l1 = nn.Linear(hidden_dim, hidden_dim)
        self.l2 = nn.Linear(hidden_dim, hidden_dim)
        self.use_norm = use_norm
        if use_norm:
            self.normalizer = nn.LayerNorm(hidden_dim, eps=1e-06)

    def forward(self, x):
        raise RuntimeError("a residual block has no evaluation of its own: call the ResidualMLPNetwork that owns it")


class ResidualMLPNetwork(_KernelNetwork):
    """Linear(input_dim, hidden_dim), num_hidden_layers / 2 pre-activation residual blocks, Linear(hidden_dim, output_dim);
    no activation outside the blocks.  A block on the stream u: ``v = l1(act(norm(u)))``, ``out = l2(act(norm(v))) + u``; ``norm``
    is the identity without ``use_norm`` and the block's one LayerNorm(hidden_dim, eps=1e-6) with ``norm_style='LayerNorm'``.

    Refused by name: ``norm_style='BatchNorm'`` with ``use_norm`` (the reference's default style: batch statistics and running
    buffers have no kernel), ``use_spectral_norm``, the activations ``MLPNetwork`` refuses, and dimensions outside the kernels'
    range.  ``dropout > 0`` is accepted: it is the identity in ``eval()`` and under ``no_grad``; a forward that keeps what the
    backward needs while the module is in training mode raises, because there are no dropout masks inside this network."""
    _entry = "beso_resmlp"

    def __init__(self, input_dim: int, hidden_dim: int = 100, num_hidden_layers: int = 1, output_dim=1, dropout: int = 0,
                 activation: str = "Mish", use_spectral_norm: bool = False, use_norm: bool = False,
                 norm_style: str = 'BatchNorm', device: str = 'cuda'):
        super().__init__()
        self.network_type = "mlp"
        self._device = device
        assert num_hidden_layers % 2 == 0
        self.input_dim = input_dim
        self.hidden_dim = hidden_dim
        self.num_hidden_layers = num_hidden_layers
        self.output_dim = output_dim
        self.dropout = dropout
        self.spectral_norm = use_spectral_norm
        self.use_norm = use_norm
        self.norm_style = norm_style
        self.activation = activation
        self.act_id = activation_id(activation, "ResidualMLPNetwork")
        if use_spectral_norm:
            raise ValueError("ResidualMLPNetwork: use_spectral_norm=True has no HIP kernel")
        if use_norm and norm_style != "LayerNorm":
            if norm_style == "BatchNorm":
                raise ValueError("ResidualMLPNetwork: norm_style='BatchNorm' (batch statistics, running buffers) has no HIP "
                                 "kernel; use norm_style='LayerNorm' or use_norm=False")
            raise ValueError('not a defined norm type')                  # res_layers.py:35
        _check_ranges("ResidualMLPNetwork",
                      (("input_dim", input_dim, 1 <= input_dim <= MAX_DIM),
                       ("output_dim", output_dim, 1 <= output_dim <= MAX_DIM),
                       ("hidden_dim", hidden_dim, 16 <= hidden_dim <= MAX_DIM and hidden_dim % 16 == 0),
                       ("num_hidden_layers", num_hidden_layers, 2 <= num_hidden_layers <= MAX_RESIDUAL_LAYERS)),
                      f"input_dim, output_dim in 1..{MAX_DIM}; hidden_dim a multiple of 16 up to {MAX_DIM}; num_hidden_layers "
                      f"even, in 2..{MAX_RESIDUAL_LAYERS}")
        self.n_blocks = num_hidden_layers // 2
        self.layers = nn.ModuleList([nn.Linear(input_dim, hidden_dim)])
        self.layers.extend([TwoLayerPreActivationResNetLinear(hidden_dim, use_norm) for _ in range(self.n_blocks)])
        self.layers.append(nn.Linear(hidden_dim, output_dim))
        self.layers.to(self._device)

    def _library(self):
        return _lib.load_resmlp()

    def dims(self) -> _lib.ResMlpDims:
        return _lib.ResMlpDims(self.input_dim, self.hidden_dim, self.n_blocks, self.output_dim, self.act_id,
                               _lib.RESMLP_NORMS["LayerNorm" if self.use_norm else "none"])

    def keep_floats(self, rows: int) -> int:
        """Floats of the buffer a training forward fills for the backward: x, the stream at every block's entry and behind the
        last block, and every block's v (include/beso_resmlp.h)."""
        return rows * (self.input_dim + (2 * self.n_blocks + 1) * self.hidden_dim)

    def run_forward(self, rows: torch.Tensor, keep: bool, params=None, out=None, keep_out=None):
        if keep and self.dropout > 0 and self.training:
            raise NotImplementedError(f"ResidualMLPNetwork: a training-mode forward with dropout={self.dropout} needs dropout "
                                      "masks inside the network, which have no HIP kernel; use dropout=0 or eval()")
        return super().run_forward(rows, keep, params=params, out=out, keep_out=keep_out)
