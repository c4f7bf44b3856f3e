#!/usr/bin/env python3
"""Generate tests/golden/minmax_scaler.npz by RUNNING THE REFERENCE's ``MinMaxScaler`` (beso/networks/scaler/scaler_class.py:169-338)
and, for the 4-of-16 block-push goal, its ``Scaler`` (:11-166), imported unmodified from the reference checkout (``REF`` of
make_resmlp_fixtures.py) on the CPU.

Run where that checkout exists (the tests need the written file only):

    python tests/golden/make_minmax_fixtures.py

Per case the file holds the seeded data the scaler was fitted on, every attribute of the fitted scaler, seeded inputs and what
each method returns for them, dtypes as the reference produced them.  x is 16-wide and y 2-wide (the block-push shapes) except
for the one-hot case, whose scaler has 30 statistics and is fed a 7-wide input.  Only data is written -- no reference source in
any form."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_resmlp_fixtures import REF, _install_stubs  # noqa: E402

ATTRS = ("x_min", "x_max", "y_min", "y_max", "new_min_x", "new_max_x", "new_min_y", "new_max_y", "x_mean", "x_std", "y_bounds",
         "x_bounds", "y_bounds_tensor", "x_bounds_tensor", "tensor_y_bounds")
# name -> (data dtype, data shape without the feature axis, scale_data, x width, an action component constant in the data)
CASES = {
    "f32_2d_scaled": (np.float32, (12,), True, 16, False),
    "f64_2d_scaled": (np.float64, (12,), True, 16, False),
    "f32_3d_scaled": (np.float32, (3, 4), True, 16, False),
    "f64_3d_unscaled": (np.float64, (3, 4), False, 16, False),
    "f32_2d_unscaled": (np.float32, (12,), False, 16, False),
    "f32_2d_constant_action": (np.float32, (12,), True, 16, True),
    "f32_2d_onehot": (np.float32, (12,), True, 30, False),
}


def _np(v):
    return v.detach().cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.array(v)


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from beso.networks.scaler.scaler_class import MinMaxScaler, Scaler

    out = {"cases": np.array(list(CASES)), "attrs": np.array(ATTRS)}
    for seed, (name, (dtype, lead, scale_data, x_dim, constant)) in enumerate(CASES.items(), start=300):
        rng = np.random.default_rng(seed)
        x_data = (rng.standard_normal(lead + (x_dim,)) * 2.0 + 0.5).astype(dtype)
        y_data = (rng.standard_normal(lead + (2,)) * 0.3 + 0.1).astype(dtype)
        if constant:
            y_data[..., 1] = 0.25
        sc = MinMaxScaler(x_data, y_data, scale_data, "cpu")
        out[f"{name}::x_data"], out[f"{name}::y_data"], out[f"{name}::scale_data"] = x_data, y_data, np.array(scale_data)
        for a in ATTRS:
            out[f"{name}::attr::{a}"] = _np(getattr(sc, a))
        # inputs: fp32, as the agent feeds them; the first rows lie far outside the data so that every bound is crossed
        x_in = (rng.standard_normal((4, x_dim)) * 2.0 + 0.5).astype(np.float32)
        x_in[0] *= 8.0
        x_in3 = (rng.standard_normal((2, 3, x_dim)) * 2.0 + 0.5).astype(np.float32)
        y_in = (rng.standard_normal((4, 2)) * 0.3 + 0.1).astype(np.float32)
        y_in[0] = [5.0, -5.0]
        # clip_action's input lives in the scaled domain with scale_data (bounds -+1.1), in the raw one without (1.1 x the data's)
        y_clip = rng.standard_normal((8, 2)).astype(np.float32) * (1.2 if scale_data else 0.8)
        T = torch.from_numpy
        calls = {
            "scale_input": (sc.scale_input, x_in), "scale_input_3d": (sc.scale_input, x_in3), "scale_output": (sc.scale_output, y_in),
            "inverse_scale_input": (sc.inverse_scale_input, x_in), "inverse_scale_output": (sc.inverse_scale_output, y_clip),
            "clip_action": (sc.clip_action, y_clip),
        }
        if x_dim == 16:
            goal4 = (rng.standard_normal((3, 4)) * 2.0 + 0.5).astype(np.float32)
            calls["scale_block_push_goal"] = (sc.scale_block_push_goal, goal4)
            calls["scale_input_goal4"] = (sc.scale_input, goal4)                 # the 4-of-16 branch
            zs = Scaler(x_data, y_data, scale_data, "cpu")                       # the reference's z-score Scaler on the same data
            calls["zscore::scale_block_push_goal"] = (zs.scale_block_push_goal, goal4)
            calls["zscore::scale_input_goal4"] = (zs.scale_input, goal4)
        else:
            calls["scale_input_onehot"] = (sc.scale_input, np.eye(7, dtype=np.float32)[[2, 0, 6]])      # 7 of 30: passes through
        for key, (fn, arg) in calls.items():
            out[f"{name}::in::{key}"] = arg
            out[f"{name}::out::{key}"] = _np(fn(T(arg.copy())))
        n_clipped = int((out[f"{name}::out::clip_action"] != y_clip).sum())
        assert 0 < n_clipped < y_clip.size, (name, n_clipped)
    # ~250 small arrays: as npz members each would cost more in zip and npy headers than it holds, so they travel as ONE byte
    # string with an index of "name dtype shape offset" lines (tests/test_minmax_scaler.py load_fixture() unpacks it)
    index, blob = [], bytearray()
    for key, v in out.items():
        v = np.ascontiguousarray(v)
        assert v.dtype.kind in "fbU", (key, v.dtype)
        index.append(f"{key} {v.dtype.str} {','.join(map(str, v.shape))} {len(blob)}")
        blob += v.tobytes()
    path = os.path.join(HERE, "minmax_scaler.npz")
    np.savez_compressed(path, index=np.array(index), blob=np.frombuffer(bytes(blob), dtype=np.uint8))
    print(f"wrote {os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
