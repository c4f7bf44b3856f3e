#!/usr/bin/env python3
"""Recorder of tests/golden/fused_shape_table.npz: every size function of the library over a sweep of configurations that
sits on the edges of fused.hip's shape predicates (tests/test_fused_shape_table.py compares the tree's library with it).

The fixture pins the predicates of commit c5d1d8e, the parent of the change that gave fused.hip one shape table, so it is
recorded from THAT commit's library, not from the tree's:

    python tools/variants.py build parent=@c5d1d8e
    BESO_HIP_LIB=beso_amd/lib/variants/libbeso_hip_parent.so python tools/record_fused_shape_table.py

The size functions are pure host code: no GPU is needed, here or in the test.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COMMIT = "c5d1d8e"
FIXTURE = os.path.join(ROOT, "tests", "golden", "fused_shape_table.npz")

# embed_dim at and around every edge of a (RPW, KS) class -- RPW = ceil(D / 128), KS = ceil(D / 32): (2, 8) is D in 232 .. 256,
# (3, 12) 360 .. 384, (4, 16) 504 .. 512; 240 and 360 are the widest the half last k-step admits -- plus one tiny width
WIDTHS = (64, 232, 240, 248, 256, 352, 360, 368, 376, 384, 504, 512, 520)
# head counts: every divisor of the width among these.  360: 6 -> HG 1, 12 -> HG 2 (head size 30: no multiple of 4),
# 18 -> HG 3 with (3, 12) rows; 240: 6 -> HG 1 with (2, 8) rows, 8 -> HG 2, 12 -> HG 3
HEADS = (4, 6, 8, 12, 18)
GOALS = (0, 2)
# obs_seq_len W, T = 1 + G + 2 W tokens: 8 T on both sides of 96 (G = 2: W = 4 | 5; G = 0: W = 5 | 6), T on both sides of
# 16 kLongNT = 80 (G = 2: W = 38 | 39; G = 0: W = 39 | 40), the long-horizon shape's own W = 32 and W = 1
WINDOWS = (1, 4, 5, 6, 32, 38, 39, 40)
# (n_layers, act_dim, linear_output) -- 7 layers x 16 crosses kTrainPackSegs = 96, the fused head takes act_dim <= 16 and the
# linear head -- varied one at a time around the shipped (6, 16, on) and all at once: half of the full cross, which would put
# the fixture at the size limit of a committed file
TAILS = ((6, 16, 1), (1, 16, 1), (7, 16, 1), (6, 17, 1), (6, 16, 0), (7, 17, 0))
BATCHES = (1, 512, 513, 1024, 1025)
PRECISIONS = (0, 1, 2, 3)           # BESO_PREC_BF16, FP32, BF16X3, FP16
OBS_DIM = 30


def cases():
    """(obs_dim, act_dim, embed_dim, n_layers, n_heads, goal_seq_len, obs_seq_len, linear_output), in a fixed order."""
    out = []
    for D in WIDTHS:
        for H in HEADS:
            if D % H or D // H > 128:
                continue
            for G in GOALS:
                for W in WINDOWS:
                    for L, act, lin in TAILS:
                        out.append((OBS_DIM, act, D, L, H, G, W, lin))
    return out


def columns():
    """Names of the values of one case, in measure()'s order (t = 'W' stands for the case's obs_seq_len)."""
    names = ["num_params"] + [f"packed_bytes(prec={p})" for p in PRECISIONS]
    for p in PRECISIONS:
        for b in BATCHES:
            for t in (1, "W"):
                names += [f"workspace_bytes(B={b}, t={t}, prec={p}, guidance={g})" for g in (0, 1)]
                names.append(f"train_workspace_bytes(B={b}, t={t}, prec={p})")
                names.append(f"loss_fwd_workspace_bytes(B={b}, t={t}, prec={p})")
    return names


def measure(lib, case):
    from beso_amd._lib import BesoConfig
    cfg = BesoConfig(*case, 0.5)
    ref = C.byref(cfg)
    vals = [lib.beso_num_params(ref)] + [lib.beso_packed_bytes(ref, p) for p in PRECISIONS]
    for p in PRECISIONS:
        for b in BATCHES:
            for t in (1, case[6]):
                vals += [lib.beso_workspace_bytes(ref, b, t, p, 0), lib.beso_workspace_bytes(ref, b, t, p, 1),
                         lib.beso_train_workspace_bytes(ref, b, t, p), lib.beso_loss_fwd_workspace_bytes(ref, b, t, p)]
    return vals


def sweep(lib):
    cs = cases()
    return np.array(cs, dtype=np.int32), np.array([measure(lib, c) for c in cs], dtype=np.uint64)


def main():
    from beso_amd import _lib
    if not os.environ.get("BESO_HIP_LIB"):
        raise SystemExit(f"set BESO_HIP_LIB to a build of commit {COMMIT} (see this file's docstring)")
    cs, vals = sweep(_lib.load())
    np.savez_compressed(FIXTURE, commit=np.array(COMMIT), cases=cs, values=vals)
    print(f"{FIXTURE}: {cs.shape[0]} cases x {vals.shape[1]} values, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
