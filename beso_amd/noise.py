"""Keyed noise for rollout inference (include/beso_noise.h, csrc/noise.hip): every environment draws from its own seed, so
that what it receives depends on (seed, episode, step, which draw, element) and on nothing else -- not on the number of
environments, its row among them or any draw made before.  ``VectorRollout.seed`` is the caller: one launch per environment
step writes the x_T draw, the best-of-K candidate draws and an ancestral sampler's step noise, and advances the counters.
GPU only: there is no torch-op form in the package (the generator is restated in tests/test_keyed_noise.py)."""
from __future__ import annotations

import numbers

import torch

from . import _lib

PURPOSES = tuple(_lib.NOISE_PURPOSES)
_FRESH = -1         # episode 0xffffffff: with the reset flag set, the next step is episode 0, step 0


def check_seeds(seeds, ids) -> list:
    """The uint64 keys of the environments `ids` (a list of ints) as Python ints, or ValueError: `seeds` is one int -- the seed
    of environment 0, environment i takes ``seeds + i`` modulo 2^64 -- or one int in [0, 2^64) per listed environment.
    Touches no device."""
    is_int = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)       # noqa: E731
    if is_int(seeds):
        if not 0 <= int(seeds) < 2 ** 64:
            raise ValueError(f"seed {seeds!r} is outside [0, 2^64)")
        return [(int(seeds) + int(i)) % 2 ** 64 for i in ids]
    if isinstance(seeds, (str, bytes)) or not hasattr(seeds, "__len__"):
        raise ValueError(f"seeds must be an int or a sequence of ints, got {seeds!r}")
    seeds = list(seeds.tolist() if hasattr(seeds, "tolist") else seeds)
    if len(seeds) != len(ids):
        raise ValueError(f"expected {len(ids)} seeds, one per environment, got {len(seeds)}")
    for s in seeds:
        if not is_int(s) or not 0 <= int(s) < 2 ** 64:
            raise ValueError(f"seed {s!r} is not an int in [0, 2^64)")
    return [int(s) for s in seeds]


def _signed64(v: int) -> int:
    return v - 2 ** 64 if v >= 2 ** 63 else v


class KeyedNoise:
    """``KeyedNoise(seeds, device)``: one uint64 key per environment and its (episode, step) counters on the device.

    ``keys`` [N] int64 and ``episodes`` / ``steps`` [N] int32 hold the library's uint64 / uint32 bits.  ``reset`` [N] uint8
    marks the environments whose next ``rollout`` call starts an episode; all of them start marked, at episode 0.  The counters
    live in two pairs of arrays: ``rollout`` reads one pair and writes the other (many workgroups read an environment's
    counters while one thread updates them), and ``episodes`` / ``steps`` are the pair written last."""

    def __init__(self, seeds, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("beso_amd: keyed noise runs on the GPU only (no CPU path)")
        if isinstance(seeds, numbers.Integral) and not isinstance(seeds, bool):
            raise ValueError("KeyedNoise takes one seed per environment (VectorRollout.seed spreads an int)")
        keys = check_seeds(seeds, list(range(len(seeds) if hasattr(seeds, "__len__") else 0)))
        if not keys:
            raise ValueError("KeyedNoise needs at least one seed")
        self.lib = _lib.load_noise()
        self.device = device
        self.n = len(keys)
        self.keys = torch.tensor([_signed64(k) for k in keys], dtype=torch.int64, device=device)
        self._counters = [(torch.full((self.n,), _FRESH, dtype=torch.int32, device=device),
                           torch.zeros(self.n, dtype=torch.int32, device=device)) for _ in range(2)]
        self._cur = 0
        self.reset = torch.ones(self.n, dtype=torch.uint8, device=device)
        self._reset_pending = True

    @property
    def episodes(self) -> torch.Tensor:
        return self._counters[self._cur][0]

    @property
    def steps(self) -> torch.Tensor:
        return self._counters[self._cur][1]

    def set_seeds(self, seeds, ids) -> None:
        """New keys for the environments `ids` (a list of ints): they start over at episode 0, step 0 with their next step."""
        keys = check_seeds(seeds, ids)
        at = torch.as_tensor(ids, dtype=torch.long, device=self.device)
        self.keys[at] = torch.tensor([_signed64(k) for k in keys], dtype=torch.int64, device=self.device)
        self.episodes[at] = _FRESH
        self.mark_reset(at)

    def mark_reset(self, ids=None) -> None:
        """The environments `ids` (an index tensor on the device; None: all) start their next episode with the next ``rollout``."""
        if ids is None:
            self.reset.fill_(1)
        else:
            self.reset.index_fill_(0, ids, 1)
        self._reset_pending = True

    def _plain(self, fn, purpose, S: int, E: int, out, dtype, *scale):
        if purpose not in _lib.NOISE_PURPOSES:
            raise ValueError(f"purpose must be one of {PURPOSES}, got {purpose!r}")
        if out is None:
            out = torch.empty((int(S), self.n, int(E)), dtype=dtype, device=self.device)
        elif out.dtype != dtype or out.device != self.device or not out.is_contiguous() or out.numel() != int(S) * self.n * int(E):
            raise ValueError(f"out must be a contiguous {dtype} tensor of {int(S) * self.n * int(E)} elements on {self.device}")
        _lib.launch("noise", fn, self.device, self.keys.data_ptr(), self.episodes.data_ptr(), self.steps.data_ptr(), self.n,
                    _lib.NOISE_PURPOSES[purpose], int(S), int(E), *scale, out.data_ptr())
        return out

    def words(self, purpose: str, S: int, E: int, out=None) -> torch.Tensor:
        """``beso_noise_words``: [S, N, E] int32 holding the generator's uint32 words at the current counters, for audit."""
        return self._plain("beso_noise_words", purpose, S, E, out, torch.int32)

    def normal(self, purpose: str, S: int, E: int, scale: float = 1.0, out=None) -> torch.Tensor:
        """``beso_noise_normal``: [S, N, E] float32 standard normals times `scale` at the current counters."""
        return self._plain("beso_noise_normal", purpose, S, E, out, torch.float32, float(scale))

    def rollout(self, act_dim: int, candidates: int = 0, n_steps: int = 0, step_elems: int = 0, out=None):
        """``beso_noise_rollout``: advance the counters (a marked environment: episode + 1, step 0; the others: step + 1) and
        draw, at the advanced counters, (x_t [N, 1, act], cand [N, K, act] or None, step_noise [n_steps, N, step_elems] or
        None).  One launch.  `out`: the three buffers (None where there is none) instead of fresh ones."""
        N, K, n_steps, dev = self.n, int(candidates), int(n_steps), self.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        if out is None:
            out = (new(N, 1, act_dim), new(N, K, act_dim) if K > 0 else None, new(n_steps, N, step_elems) if n_steps > 0 else None)
        x_t, cand, step_noise = out
        for v, count, name in ((x_t, N * act_dim, "x_t"), (cand, N * K * act_dim, "cand"), (step_noise, n_steps * N * step_elems, "step_noise")):
            if v is not None and (v.dtype != torch.float32 or v.device != dev or not v.is_contiguous() or v.numel() != count):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {count} elements on {dev}")
        src, dst = self._counters[self._cur], self._counters[1 - self._cur]
        ptr = lambda v: None if v is None else v.data_ptr()      # noqa: E731
        _lib.launch("noise", "beso_noise_rollout", dev, self.keys.data_ptr(), self.reset.data_ptr() if self._reset_pending else None,
                    src[0].data_ptr(), src[1].data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), N, int(act_dim), K, n_steps,
                    int(step_elems), ptr(x_t), ptr(cand), ptr(step_noise))
        self._cur = 1 - self._cur
        if self._reset_pending:
            self.reset.zero_()
            self._reset_pending = False
        return x_t, cand, step_noise
