"""What the fit steps of ``GuideTrainer`` (guide_fit.py) and ``CriticTrainer`` (critic_fit.py) share: ``FitNet``, one ``MLPNetwork``
under training with its optimizer, flat gradient and per-row-count buffers; the argument checks and conversions of a step; and
``row_dims``, the row layout ``[state | action | goal | extra]`` that ``MLPGuide`` and ``StateValue`` check a call against."""
import torch

from ....optim import FusedAdam


def shape_of(t):
    return tuple(t.shape) if torch.is_tensor(t) else type(t).__name__


def f32c(t, dev):
    return None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def goal_args(goal):
    """(goal_steps, goal_rows) as the C entry points take them: both 0 without a goal."""
    return (0, 0) if goal is None else (goal.shape[1], goal.shape[0])


def check_bt(who: str, B: int, T: int, named, required=()):
    """Every ``(name, tensor)`` of ``named`` is ``[B, T]``; None passes unless the name is in ``required``."""
    for name, t in named:
        if (t is None and name in required) or (t is not None and (not torch.is_tensor(t) or t.shape != (B, T))):
            raise ValueError(f"{who}: {name} must be [B={B}, T={T}], got {shape_of(t)}")


def require_gpu(who: str, what: str, tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{who} runs on the GPU only (HIP kernels, no CPU or eager fallback): {what} and every tensor of a step "
                           "must be on it")


def row_dims(who: str, input_dim: int, state, action, goal, use_goal: bool, extra: int = 0, **flags):
    """(B, steps, obs, act, goal or None) of rows ``[state | action | goal | extra columns]``, refusing by name (``who``) what a
    network of ``input_dim`` cannot read.  ``action`` None: rows without an action part (act = 0), one per step of ``state``;
    else one per step of ``action``, of which ``state`` may hold more.  ``flags``: what else the message names beside use_goal."""
    if action is None:
        if state.dim() != 3:
            raise ValueError(f"{who}: state {tuple(state.shape)} must be [B, steps, obs]")
        (B, T, obs), act = state.shape, 0
    else:
        if state.dim() != 3 or action.dim() != 3 or state.shape[0] != action.shape[0]:
            raise ValueError(f"{who}: state {tuple(state.shape)} and a {tuple(action.shape)} must be [B, steps, dim] with one B")
        B, T, act = action.shape
        if state.shape[1] < T:
            raise ValueError(f"{who}: state has {state.shape[1]} steps, fewer than a's {T}")
        obs = state.shape[2]
    goal = goal if use_goal and goal is not None else None
    if goal is not None and (goal.dim() != 3 or goal.shape[2] != obs or goal.shape[0] not in (1, B)):
        raise ValueError(f"{who}: goal {tuple(goal.shape)} must be [B or 1, G, obs={obs}]")
    want = obs + act + (obs if goal is not None else 0) + extra
    if input_dim != want:
        named = ", ".join(f"{k}={v}" for k, v in dict(use_goal=use_goal, **flags).items())
        raise ValueError(f"{who}: the network's input_dim={input_dim}, but obs{'' if action is None else ' + act'}"
                         f"{' + obs' if goal is not None else ''}{f' + {extra}' if extra else ''} = {want} ({named})")
    return B, T, obs, act, goal


class FitNet:
    """One ``MLPNetwork`` with a scalar output under training: its parameter list, its ``FusedAdam`` (``adam``: the keywords), the
    flat gradient its parameters' ``.grad`` are views of, and per row count the buffers of a step.  Nothing is allocated and no
    ``.grad`` attached before ``grads`` / ``buffers`` are called."""

    def __init__(self, network, adam: dict):
        self.network = network
        self.params = list(network.layers.parameters())
        self.optimizer = FusedAdam(self.params, **adam)
        self.flat = None                # the flat gradient; every parameter's .grad is a view of it
        self.bufs = {}                  # rows -> (rows, out, keep, d_out, workspace[, spare out])

    def grads(self, dev):
        if self.flat is None or self.flat.device != dev:
            self.flat = torch.empty(self.network.num_param_floats(), dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:               # (re-attached every step: zero_grad(set_to_none=True) elsewhere may have dropped them)
            view = self.flat[off:off + p.numel()].view(p.shape)
            if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                p.grad = view
            off += p.numel()
        return self.flat

    def buffers(self, rows: int, dev, zero_d_out: bool = False, spare_out: bool = False):
        """(input rows [rows, input_dim], out [rows, 1], keep, d_out [rows], workspace) and, with ``spare_out``, a second out.
        ``zero_d_out``: d_out is made by ``torch.zeros``, once, for a caller that writes only a part of it."""
        hit = self.bufs.get(rows)
        if hit is None or hit[0].device != dev:
            net = self.network
            f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)                  # noqa: E731
            hit = self.bufs[rows] = (f32(rows, net.input_dim), f32(rows, 1), f32(net.keep_floats(rows)),
                                     torch.zeros(rows, dtype=torch.float32, device=dev) if zero_d_out else f32(rows),
                                     torch.empty(net.workspace_bytes(rows), dtype=torch.uint8, device=dev),
                                     *((f32(rows, 1),) if spare_out else ()))
        return hit

    def forward(self, b, params=None, keep: bool = True, out=None):
        """``beso_mlp_fwd`` of ``b``'s rows into ``b``'s out (or ``out``), on the network's parameters (or ``params``)."""
        self.network.run_forward(b[0], keep=keep, params=self.params if params is None else params,
                                 out=b[1] if out is None else out, keep_out=b[2] if keep else None)

    def backward(self, b, flat):
        """``beso_mlp_bwd`` from ``b``'s keep and d_out into ``flat``."""
        self.network.run_backward(b[2], b[3], flat, params=self.params, workspace=b[4])

    def export(self):
        """(the network's ``state_dict`` as CPU clones, ``FusedAdam.export_state()``)."""
        return ({k: v.detach().cpu().clone() for k, v in self.network.state_dict().items()}, self.optimizer.export_state())

    def load(self, network: dict, optimizer: dict) -> None:
        self.network.load_state_dict(network)                          # in place: the parameters keep their storage
        self.optimizer.import_state(optimizer)
