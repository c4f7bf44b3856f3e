"""Boundary plumbing: z-score scaler of observations / actions with the action bounds the agent
clips to (reference: beso/networks/scaler/scaler_class.py:11-166), and MinMaxScaler, the block-push workspace's scaler
(:169-338): observations z-scored, actions mapped onto [-1, 1].  Elementwise host-side torch;
the workspace normally builds the reference's own Scaler -- any object with this surface works."""
import ctypes as C

import numpy as np
import torch

_GOAL_4_OF_16 = [0, 1, 3, 4]        # the block positions a 4-wide block-push goal holds, among the 16 observation features
_MAX_ITEMS = 4                      # tensors per scale_many launch: beso_scale_rows' limit and BESO_SCALE_MAX_ITEMS


def _scale_block_push_goal(sc, x):
    """scale_block_push_goal of both reference scalers (scaler_class.py:144-159, :316-331), the formula as written there:
    x * (x - mean) / (std + 1e-12), no cast."""
    if not sc.scale_data:
        return x.to(sc.device)
    x = x.to(sc.device)
    std = sc.x_std[_GOAL_4_OF_16]
    return x * (x - sc.x_mean[_GOAL_4_OF_16]) / (std + 1e-12 * torch.ones(std.shape, device=sc.device))


def _cached(sc, slot: str, sources, make):
    """make(), kept in sc.__dict__ under `slot` for as long as every tensor of `sources` is the same object at the same
    version: a tensor that is the same every call costs its elementwise launches once."""
    hit = sc.__dict__.get(slot)
    if hit is None or len(hit[0]) != len(sources) or any(a is not b or v != b._version for (a, v), b in zip(hit[0], sources)):
        hit = ([(s, s._version) for s in sources], make())
        sc.__dict__[slot] = hit
    return hit[1]


def _data_rows(x_data, y_data):
    """The data both constructors fit on, as numpy arrays: tensors converted, [episodes, steps, features] flattened to rows."""
    if isinstance(x_data, torch.Tensor):
        x_data, y_data = x_data.detach().cpu().numpy(), y_data.detach().cpu().numpy()
    if x_data.ndim == 3:
        x_data = x_data.reshape(-1, x_data.shape[-1])
        y_data = y_data.reshape(-1, y_data.shape[-1])
    elif x_data.ndim not in (2, 4):
        raise ValueError('not implemented yet!')
    return x_data, y_data


def _clip_action(sc, y):
    """clip_action of both scalers: clamp to 1.1 x y_bounds_tensor (scaler_class.py:162-166, :334-338).  The two scaled bound
    rows are the same tensors every call: computed once per bounds tensor (two elementwise launches less per environment step)."""
    b = sc.y_bounds_tensor
    lo, hi = _cached(sc, "_clip_cache", (b,), lambda: (b[0] * 1.1, b[1] * 1.1))
    return torch.clamp(y, lo, hi).to(sc.device).to(torch.float32)


def _scale_many(sc, items, stats_of, available, launch):
    """scale_many of both scalers: [(tensor, 'x' | 'y'), ...] -> the scaled tensors, as ONE HIP launch where every tensor is a
    non-empty contiguous fp32 CUDA tensor and every statistic of its kind (``stats_of(which)``) an fp32 row beside it.  Anything
    else -- CPU tensors, other dtypes, one-hot or 4-of-16 goals, scale_data off, more than _MAX_ITEMS items, or a library that
    cannot (``available()``, asked last) -- takes the per-tensor methods.  ``launch(dev, src, dst, stat, rows, cols, n)`` enqueues
    the class's entry point on the host tables of n entries; ``stat(j)`` is the table of every item's statistic j (NULL where an
    item has fewer)."""
    plan, ok = [], bool(sc.scale_data) and 0 < len(items) <= _MAX_ITEMS
    for x, which in items:
        if not ok:
            break
        stats = stats_of(which)
        ok = (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0
              and all(isinstance(s, torch.Tensor) and s.device == x.device and s.dtype == torch.float32 and s.dim() == 1
                      and s.numel() == x.shape[-1] and s.is_contiguous() for s in stats)
              and not (which == "x" and x.shape[-1] == 7 and len(sc.x_mean) == 30)
              and not (which == "x" and x.shape[-1] == 4 and len(sc.x_mean) == 16))
        plan.append((x, stats))
    if not (ok and available()):
        return [sc.scale_input(x) if which == "x" else sc.scale_output(x) for x, which in items]
    n = len(plan)
    outs = [torch.empty_like(x) for x, _ in plan]
    vp = C.c_void_p * n
    stat = lambda j: vp(*[s[j].data_ptr() if j < len(s) else None for _, s in plan])      # noqa: E731
    launch(plan[0][0].device, vp(*[x.data_ptr() for x, _ in plan]), vp(*[o.data_ptr() for o in outs]), stat,
           (C.c_longlong * n)(*[x.numel() // x.shape[-1] for x, _ in plan]), (C.c_int * n)(*[x.shape[-1] for x, _ in plan]), n)
    return outs


class Scaler:
    def __init__(self, x_data, y_data, scale_data: bool, device: str):
        self.scale_data = scale_data
        self.device = device
        x_data, y_data = _data_rows(x_data, y_data)
        dev = lambda a: torch.from_numpy(a).to(device)       # noqa: E731
        self.x_mean, self.x_std = dev(x_data.mean(0)), dev(x_data.std(0))
        self.y_mean, self.y_std = dev(y_data.mean(0)), dev(y_data.std(0))
        self.x_max, self.x_min = dev(x_data.max(0)), dev(x_data.min(0))
        self.y_max, self.y_min = dev(y_data.max(0)), dev(y_data.min(0))
        self.y_bounds = np.zeros((2, y_data.shape[-1]))
        self.x_bounds = np.zeros((2, x_data.shape[-1]))
        if scale_data:
            self.y_bounds[0] = (y_data.min(0) - y_data.mean(0)) / (y_data.std(0) + 1e-12)
            self.y_bounds[1] = (y_data.max(0) - y_data.mean(0)) / (y_data.std(0) + 1e-12)
            self.x_bounds[0] = (x_data.min(0) - x_data.mean(0)) / (x_data.std(0) + 1e-12)
            self.x_bounds[1] = (x_data.max(0) - x_data.mean(0)) / (x_data.std(0) + 1e-12)
        else:
            self.y_bounds[0], self.y_bounds[1] = y_data.min(0), y_data.max(0)
            self.x_bounds[0], self.x_bounds[1] = x_data.min(0), x_data.max(0)
        self.y_bounds_tensor = torch.from_numpy(self.y_bounds).to(device)
        self.x_bounds_tensor = torch.from_numpy(self.x_bounds).to(device)
        self.tensor_y_bounds = self.y_bounds_tensor

    @torch.no_grad()
    def scale_input(self, x):
        if x.shape[-1] == 4 and len(self.x_mean) == 16:      # the 4-of-16 block-push goal (scaler_class.py:80-82)
            return self.scale_block_push_goal(x)
        x = x.to(self.device)
        if x.shape[-1] == 7 and len(self.x_mean) == 30:      # one-hot kitchen goals pass through
            return x
        if self.scale_data:
            return ((x - self.x_mean) / self._den("x")).to(torch.float32)
        return x

    @torch.no_grad()
    def scale_output(self, y):
        y = y.to(self.device)
        if self.scale_data:
            return ((y - self.y_mean) / self._den("y")).to(torch.float32)
        return y

    @torch.no_grad()
    def scale_many(self, items):
        """[(tensor, 'x' | 'y'), ...] -> the scaled tensors: scale_input / scale_output of every item (scaler_class.py:95-117) as
        ONE HIP launch (beso_scale_rows: the same subtraction and correctly rounded division per element) -- a training batch is
        three tensors, i.e. six elementwise launches of ~6 us each in front of the forward.  What the launch does not take, a
        product library without the entry point included: the per-tensor methods (_scale_many)."""
        from ... import _lib
        return _scale_many(
            self, items, lambda which: (self.x_mean if which == "x" else self.y_mean, self._den(which)),
            lambda: hasattr(_lib.load(), "beso_scale_rows"),
            lambda dev, src, dst, stat, rows, cols, n: _lib.launch("hip", "beso_scale_rows", dev, src, dst, stat(0), stat(1), rows,
                                                                   cols, n))

    def _den(self, which: str):
        """std + 1e-12 (scaler_class.py:129,139): the same tensor every call -- computed once per std tensor instead of one
        more elementwise launch per scaled batch (three per training step)."""
        std = self.x_std if which == "x" else self.y_std
        return _cached(self, "_den_cache_" + which, (std,), lambda: std + 1e-12)

    @torch.no_grad()
    def inverse_scale_input(self, x):
        return x * (self.x_std + 1e-12) + self.x_mean if self.scale_data else x

    @torch.no_grad()
    def inverse_scale_output(self, y):
        y = y.to(self.device)
        return y * self._den("y") + self.y_mean if self.scale_data else y

    @torch.no_grad()
    def scale_block_push_goal(self, x):
        return _scale_block_push_goal(self, x)

    @torch.no_grad()
    def clip_action(self, y):
        return _clip_action(self, y)


class MinMaxScaler:
    """The reference's MinMaxScaler (scaler_class.py:169-338), the scaler the block-push workspace builds: the same
    constructor, attributes and methods, each method the reference's operations in the reference's order.  Observations
    are z-scored as Scaler's are; actions go onto [new_min_y, new_max_y] = [-1, 1] WITHOUT an epsilon -- an action component
    that is constant in the data divides by zero, as in the reference.  The tensors that are the same every call are computed
    once per source tensor (_den, _y_range, _y_span, the clip rows), and scale_many runs a batch's scalings as one launch."""

    def __init__(self, x_data, y_data, scale_data: bool, device: str):
        self.scale_data = scale_data
        self.device = device
        x_data, y_data = _data_rows(x_data, y_data)
        dev = lambda a: torch.from_numpy(a).to(device)       # noqa: E731
        with torch.no_grad():
            self.x_max, self.x_min = dev(x_data.max(0)), dev(x_data.min(0))
            self.y_min, self.y_max = dev(y_data.min(0)), dev(y_data.max(0))
            self.new_max_x = torch.ones_like(self.x_max)
            self.new_min_x = -1 * torch.ones_like(self.x_max)
            self.new_max_y = torch.ones_like(self.y_max)
            self.new_min_y = -1 * torch.ones_like(self.y_max)
            self.x_mean, self.x_std = dev(x_data.mean(0)), dev(x_data.std(0))
        self.y_bounds = np.zeros((2, y_data.shape[-1]))
        self.x_bounds = np.zeros((2, x_data.shape[-1]))
        if scale_data:
            # the actions' bounds are the new range; the observations' are the z-scored data bounds (:214-224)
            self.y_bounds[0] = -1 * np.ones_like(y_data.min(0))
            self.y_bounds[1] = np.ones_like(y_data.min(0))
            self.x_bounds[0] = (x_data.min(0) - x_data.mean(0)) / (x_data.std(0) + 1e-12 * np.ones(self.x_std.shape))
            self.x_bounds[1] = (x_data.max(0) - x_data.mean(0)) / (x_data.std(0) + 1e-12 * np.ones(self.x_std.shape))
        else:
            self.y_bounds[0], self.y_bounds[1] = y_data.min(0), y_data.max(0)
            self.x_bounds[0], self.x_bounds[1] = x_data.min(0), x_data.max(0)
        self.y_bounds_tensor = torch.from_numpy(self.y_bounds).to(device)
        self.x_bounds_tensor = torch.from_numpy(self.x_bounds).to(device)
        self.tensor_y_bounds = torch.from_numpy(self.y_bounds).to(device)

    # ------------------------------------------------------------------ the tensors that are the same every call
    def _den(self):
        """x_std + 1e-12 (scaler_class.py:261), the reference's expression: the epsilon is an fp32 tensor of ones times 1e-12."""
        return _cached(self, "_den_cache", (self.x_std,),
                       lambda: self.x_std + 1e-12 * torch.ones(self.x_std.shape, device=self.device))

    def _y_range(self):
        """y_max - y_min (:277, :310)."""
        return _cached(self, "_y_range_cache", (self.y_max, self.y_min), lambda: self.y_max - self.y_min)

    def _y_span(self):
        """new_max_y - new_min_y (:277, :310)."""
        return _cached(self, "_y_span_cache", (self.new_max_y, self.new_min_y), lambda: self.new_max_y - self.new_min_y)

    # ------------------------------------------------------------------ the reference's methods
    @torch.no_grad()
    def scale_input(self, x, block_push_goal=False):
        if x.shape[-1] == 4 and len(self.x_mean) == 16:      # the 4-of-16 block-push goal
            return self.scale_block_push_goal(x)
        if x.shape[-1] == 7 and len(self.x_mean) == 30:      # one-hot kitchen goals pass through
            return x.to(self.device)
        x = x.to(self.device)
        if self.scale_data:
            return ((x - self.x_mean) / self._den()).to(torch.float32)
        return x

    @torch.no_grad()
    def scale_output(self, y):
        y = y.to(self.device)
        if self.scale_data:
            return ((y - self.y_min) / self._y_range() * self._y_span() + self.new_min_y).to(torch.float32)
        return y

    @torch.no_grad()
    def inverse_scale_input(self, x):
        """The min-max inverse on x (:292-296).  It does not invert scale_input: that is the reference."""
        if self.scale_data:
            return ((x - self.new_min_x) / (self.new_max_x - self.new_min_x) * (self.x_max - self.x_min) + self.x_min).to(torch.float32)
        return x.to(self.device)

    @torch.no_grad()
    def inverse_scale_output(self, y):
        if self.scale_data:
            return (y - self.new_min_y) / self._y_span() * self._y_range() + self.y_min
        return y.to(self.device)

    @torch.no_grad()
    def scale_block_push_goal(self, x):
        return _scale_block_push_goal(self, x)

    @torch.no_grad()
    def clip_action(self, y):
        return _clip_action(self, y)

    # ------------------------------------------------------------------ a batch's scalings as one launch
    @torch.no_grad()
    def scale_many(self, items):
        """Scaler.scale_many's contract: 'x' items z-scored as scale_input does and 'y' items min-max scaled as scale_output
        does, as ONE HIP launch (beso_scale_rows_mixed, include/beso_scale.h: the same individually rounded operations in the
        same order).  What the launch does not take, a missing libbeso_scale.so included: the per-tensor methods (_scale_many)."""
        from ... import _lib

        def available():
            try:
                _lib.load_scale()
            except _lib.BesoHipError:
                return False
            return True

        def launch(dev, src, dst, stat, rows, cols, n):
            kind = (C.c_int * n)(*[_lib.SCALE_KINDS["zscore" if which == "x" else "minmax"] for _, which in items])
            _lib.launch("scale", "beso_scale_rows_mixed", dev, src, dst, kind, stat(0), stat(1), stat(2), stat(3), rows, cols, n)

        return _scale_many(
            self, items, lambda which: ((self.x_mean, self._den()) if which == "x" else
                                        (self.y_min, self._y_range(), self._y_span(), self.new_min_y)), available, launch)
