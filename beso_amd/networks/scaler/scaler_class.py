"""Boundary plumbing: z-score scaler of observations / actions with the action bounds the agent
clips to (reference: beso/networks/scaler/scaler_class.py:11-166), and MinMaxScaler, the block-push workspace's scaler
(:169-338): observations z-scored, actions mapped onto [-1, 1].  Elementwise host-side torch;
the workspace normally builds the reference's own Scaler -- any object with this surface works."""
import numpy as np
import torch

_GOAL_4_OF_16 = [0, 1, 3, 4]        # the block positions a 4-wide block-push goal holds, among the 16 observation features


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


class Scaler:
    def __init__(self, x_data, y_data, scale_data: bool, device: str):
        self.scale_data = scale_data
        self.device = device
        if isinstance(x_data, torch.Tensor):
            x_data, y_data = x_data.detach().cpu().numpy(), y_data.detach().cpu().numpy()
        if x_data.ndim == 3:
            x_data = x_data.reshape(-1, x_data.shape[-1])
            y_data = y_data.reshape(-1, y_data.shape[-1])
        elif x_data.ndim not in (2, 4):
            raise ValueError('not implemented yet!')
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
        ONE HIP launch (beso_scale_rows: the same subtraction and correctly rounded division per element) where every tensor
        is a contiguous fp32 CUDA tensor with fp32 statistics -- a training batch is three tensors, i.e. six elementwise launches
        of ~6 us each in front of the forward.  Anything else (CPU tensors, other dtypes, one-hot goals, scale_data off, a
        library without the entry point): the per-tensor methods."""
        plan, ok = [], self.scale_data and 0 < len(items) <= 4
        for x, which in items:
            mean = self.x_mean if which == "x" else self.y_mean
            den = self._den(which) if self.scale_data else None
            good = (ok and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0
                    and isinstance(mean, torch.Tensor) and mean.is_cuda and mean.device == x.device and mean.dtype == torch.float32
                    and den.dtype == torch.float32 and mean.dim() == 1 and mean.numel() == x.shape[-1] and mean.is_contiguous()
                    and den.is_contiguous() and not (which == "x" and x.shape[-1] == 7 and len(self.x_mean) == 30)
                    and not (which == "x" and x.shape[-1] == 4 and len(self.x_mean) == 16))
            ok = ok and good
            plan.append((x, mean, den))
        lib = None
        if ok:
            from ... import _lib
            lib = _lib.load()
            ok = hasattr(lib, "beso_scale_rows")
        if not ok:
            return [self.scale_input(x) if which == "x" else self.scale_output(x) for x, which in items]
        import ctypes as C
        from ... import _lib
        from ...runtime import stream_ptr
        n = len(plan)
        outs = [torch.empty_like(x) for x, _, _ in plan]
        vp = C.c_void_p * n
        src = vp(*[x.data_ptr() for x, _, _ in plan]); dst = vp(*[o.data_ptr() for o in outs])
        mean = vp(*[m.data_ptr() for _, m, _ in plan]); den = vp(*[d.data_ptr() for _, _, d in plan])
        rows = (C.c_longlong * n)(*[x.numel() // x.shape[-1] for x, _, _ in plan])
        cols = (C.c_int * n)(*[x.shape[-1] for x, _, _ in plan])
        dev = plan[0][0].device
        with torch.cuda.device(dev):
            _lib.check(lib.beso_scale_rows(src, dst, mean, den, rows, cols, n, stream_ptr(dev)),
                       "scale_rows")
        return outs

    def _den(self, which: str):
        """std + 1e-12 (scaler_class.py:129,139): the same tensor every call -- computed once per std tensor instead of one
        more elementwise launch per scaled batch (three per training step)."""
        std = self.x_std if which == "x" else self.y_std
        cache = self.__dict__.setdefault("_den_cache", {})
        hit = cache.get(which)
        if hit is None or hit[0] is not std or hit[1] != std._version:
            hit = (std, std._version, std + 1e-12)
            cache[which] = hit
        return hit[2]

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
        """Clamp to 1.1 x the data bounds (scaler_class.py:162-166).  The two scaled bound rows are the same tensors every
        call: computed once per bounds tensor (two elementwise launches less per environment step)."""
        b = self.y_bounds_tensor
        hit = self.__dict__.get("_clip_cache")
        if hit is None or hit[0] is not b or hit[1] != b._version:
            hit = (b, b._version, b[0] * 1.1, b[1] * 1.1)
            self._clip_cache = hit
        return torch.clamp(y, hit[2], hit[3]).to(self.device).to(torch.float32)


class MinMaxScaler:
    """The reference's MinMaxScaler (scaler_class.py:169-338), the scaler the block-push workspace builds: the same
    constructor, attributes and methods, each method the reference's operations in the reference's order.  Observations
    are z-scored as Scaler's are; actions go onto [new_min_y, new_max_y] = [-1, 1] WITHOUT an epsilon -- an action component
    that is constant in the data divides by zero, as in the reference.  The tensors that are the same every call are computed
    once per source tensor (_den, _y_range, _y_span, the clip rows), and scale_many runs a batch's scalings as one launch."""

    def __init__(self, x_data, y_data, scale_data: bool, device: str):
        self.scale_data = scale_data
        self.device = device
        if isinstance(x_data, torch.Tensor):
            x_data, y_data = x_data.detach().cpu().numpy(), y_data.detach().cpu().numpy()
        if x_data.ndim == 3:
            x_data = x_data.reshape(-1, x_data.shape[-1])
            y_data = y_data.reshape(-1, y_data.shape[-1])
        elif x_data.ndim not in (2, 4):
            raise ValueError('not implemented yet!')
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
        """Clamp to 1.1 x y_bounds_tensor (:334-338); the two scaled rows are computed once per bounds tensor."""
        b = self.y_bounds_tensor
        lo, hi = _cached(self, "_clip_cache", (b,), lambda: (b[0] * 1.1, b[1] * 1.1))
        return torch.clamp(y, lo, hi).to(self.device).to(torch.float32)

    # ------------------------------------------------------------------ a batch's scalings as one launch
    @torch.no_grad()
    def scale_many(self, items):
        """Scaler.scale_many's contract: [(tensor, 'x' | 'y'), ...] -> the scaled tensors, 'x' items z-scored as scale_input
        does and 'y' items min-max scaled as scale_output does, as ONE HIP launch (beso_scale_rows_mixed, include/beso_scale.h:
        the same individually rounded operations in the same order) where every tensor is a contiguous fp32 CUDA tensor with
        fp32 statistics.  Anything else (CPU tensors, other dtypes, one-hot or 4-of-16 goals, scale_data off, a missing
        library): the per-tensor methods."""
        from ... import _lib
        plan, ok = [], bool(self.scale_data) and 0 < len(items) <= _lib.SCALE_LIMITS["max_items"]
        for x, which in items:
            if not ok:
                break
            stats = (self.x_mean, self._den()) if which == "x" else (self.y_min, self._y_range(), self._y_span(), self.new_min_y)
            ok = (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() > 0
                  and all(isinstance(s, torch.Tensor) and s.device == x.device and s.dtype == torch.float32 and s.dim() == 1
                          and s.numel() == x.shape[-1] and s.is_contiguous() for s in stats)
                  and not (which == "x" and x.shape[-1] == 7 and len(self.x_mean) == 30)
                  and not (which == "x" and x.shape[-1] == 4 and len(self.x_mean) == 16))
            plan.append((x, _lib.SCALE_KINDS["zscore" if which == "x" else "minmax"], stats))
        lib = None
        if ok:
            try:
                lib = _lib.load_scale()
            except _lib.BesoHipError:
                lib = None
        if lib is None:
            return [self.scale_input(x) if which == "x" else self.scale_output(x) for x, which in items]
        import ctypes as C
        from ...runtime import stream_ptr
        n = len(plan)
        outs = [torch.empty_like(x) for x, _, _ in plan]
        vp = C.c_void_p * n
        stat = lambda j: vp(*[s[j].data_ptr() if j < len(s) else None for _, _, s in plan])      # noqa: E731
        src, dst = vp(*[x.data_ptr() for x, _, _ in plan]), vp(*[o.data_ptr() for o in outs])
        kind = (C.c_int * n)(*[k for _, k, _ in plan])
        rows = (C.c_longlong * n)(*[x.numel() // x.shape[-1] for x, _, _ in plan])
        cols = (C.c_int * n)(*[x.shape[-1] for x, _, _ in plan])
        dev = plan[0][0].device
        with torch.cuda.device(dev):
            _lib.check_scale(lib.beso_scale_rows_mixed(src, dst, kind, stat(0), stat(1), stat(2), stat(3), rows, cols, n,
                                                       stream_ptr(dev)), "scale_rows_mixed")
        return outs
