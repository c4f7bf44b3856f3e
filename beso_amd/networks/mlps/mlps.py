"""``MLPNetwork`` (reference: beso/networks/mlps/mlps.py:11-73) on the HIP kernels of include/beso_mlp.h.

Same constructor kwargs, attributes, ``state_dict`` keys (``layers.N.weight`` / ``layers.N.bias``), ``get_params()`` and
``get_device()``.  ``forward`` on GPU tensors is ONE launch (``beso_mlp_fwd``); under autograd it is a
``torch.autograd.Function`` whose backward is ``beso_mlp_bwd``.  CPU tensors raise: there is no torch-op evaluation.
``ResidualMLPNetwork`` (BatchNorm, dropout, spectral norm) is not provided."""
import ctypes as C

import torch
import torch.nn as nn

from ... import _lib

MAX_DIM, MAX_HIDDEN_LAYERS = 512, 4


def activation_id(activation: str) -> int:
    """BESO_MLP_ACT_* of a name ``return_activiation_fcn`` knows (networks/utils.py:33-51).  ``"tanh"`` is nn.Sigmoid there
    (utils.py:37-38) and here.  The names without a kernel -- ``PReLU``, which is also that function's answer to every unknown
    name, and ``softmax`` -- are refused by name."""
    if activation in _lib.MLP_ACTIVATIONS:
        return _lib.MLP_ACTIVATIONS[activation]
    raise ValueError(f"MLPNetwork: activation {activation!r} has no HIP kernel (supported: "
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


class MLPNetwork(nn.Module):
    """Linear(input_dim, hidden_dim), num_hidden_layers - 1 x Linear(hidden_dim, hidden_dim), Linear(hidden_dim, output_dim);
    the activation follows every layer but the last.  ``dropout`` and ``use_spectral_norm`` are stored and unused, exactly
    as in the reference's MLPNetwork (mlps.py:37-38: neither is read again)."""

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
        for name, value, ok in (("input_dim", input_dim, 1 <= input_dim <= MAX_DIM),
                                ("output_dim", output_dim, 1 <= output_dim <= MAX_DIM),
                                ("hidden_dim", hidden_dim, 16 <= hidden_dim <= MAX_DIM and hidden_dim % 16 == 0),
                                ("num_hidden_layers", num_hidden_layers, 1 <= num_hidden_layers <= MAX_HIDDEN_LAYERS)):
            if not ok:
                raise ValueError(f"MLPNetwork: {name}={value} is outside what the HIP kernels support (input_dim, output_dim in "
                                 f"1..{MAX_DIM}; hidden_dim a multiple of 16 up to {MAX_DIM}; num_hidden_layers in "
                                 f"1..{MAX_HIDDEN_LAYERS})")
        self.layers = nn.ModuleList([nn.Linear(self.input_dim, self.hidden_dim)])
        self.layers.extend([nn.Linear(self.hidden_dim, self.hidden_dim) for _ in range(1, self.num_hidden_layers)])
        self.layers.append(nn.Linear(self.hidden_dim, self.output_dim))
        self._device = device
        self.layers.to(self._device)

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
    def dims(self) -> _lib.MlpDims:
        return _lib.MlpDims(self.input_dim, self.hidden_dim, self.num_hidden_layers, self.output_dim, self.act_id)

    def num_param_floats(self) -> int:
        return sum(p.numel() for p in self.layers.parameters())

    def keep_floats(self, rows: int) -> int:
        """Floats of the buffer a training forward fills for the backward: x and the hidden layers' pre-activations."""
        return rows * (self.input_dim + self.num_hidden_layers * self.hidden_dim)

    def workspace_bytes(self, rows: int) -> int:
        return int(_lib.load_mlp().beso_mlp_workspace_bytes(C.byref(self.dims()), rows, 1))

    def _check_input(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("MLPNetwork runs on the GPU only (HIP kernels, no CPU or eager fallback): got a "
                               f"{'CPU tensor' if isinstance(x, torch.Tensor) else type(x).__name__}")
        if x.shape[-1] != self.input_dim or x.numel() == 0:
            raise ValueError(f"MLPNetwork: input of shape {tuple(x.shape)}; the last dimension must be input_dim="
                             f"{self.input_dim} and there must be at least one row")

    def _pointers(self, params):
        params = tuple(self.layers.parameters()) if params is None else params
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("MLPNetwork: the parameters must be contiguous fp32 tensors on the GPU")
        return (C.c_void_p * len(params))(*[p.data_ptr() for p in params]), len(params)

    def run_forward(self, rows: torch.Tensor, keep: bool, params=None, out=None, keep_out=None):
        """``beso_mlp_fwd`` on contiguous fp32 ``rows`` [M, input_dim] -> (y [M, output_dim], keep buffer or None).  ``params``:
        the tensors to evaluate (default: the module's own; the agent passes the EMA shadow's)."""
        M = rows.shape[0]
        ptrs, n = self._pointers(params)
        y = torch.empty(M, self.output_dim, dtype=torch.float32, device=rows.device) if out is None else out
        if keep and keep_out is None:
            keep_out = torch.empty(self.keep_floats(M), dtype=torch.float32, device=rows.device)
        st = _lib.load_mlp().beso_mlp_fwd(ptrs, n, C.byref(self.dims()), rows.data_ptr(), M, y.data_ptr(),
                                          keep_out.data_ptr() if keep else None, _stream(rows))
        _lib.check(st, "beso_mlp_fwd")
        return y, (keep_out if keep else None)

    def run_backward(self, keep: torch.Tensor, dy: torch.Tensor, grads_flat: torch.Tensor, dx=None, accumulate=False,
                     params=None, workspace=None):
        """``beso_mlp_bwd``: the parameter gradients of the rows behind ``keep`` into ``grads_flat`` (written; added to with
        ``accumulate``), and the input gradient into ``dx`` [M, input_dim] when given."""
        dy = dy.reshape(-1, self.output_dim).to(torch.float32).contiguous()
        M = dy.shape[0]
        ptrs, n = self._pointers(params)
        need = self.workspace_bytes(M)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dy.device)
        st = _lib.load_mlp().beso_mlp_bwd(ptrs, n, C.byref(self.dims()), keep.data_ptr(), dy.data_ptr(), M,
                                          None if dx is None else dx.data_ptr(), grads_flat.data_ptr(), workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(),
                                          _lib.MLP_FLAGS["accumulate"] if accumulate else 0, _stream(dy))
        _lib.check(st, "beso_mlp_bwd")
        return grads_flat
