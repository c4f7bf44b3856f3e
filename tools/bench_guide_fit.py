#!/usr/bin/env python3
"""What one fit step of the guide costs (GuideTrainer.train_step, k_diffusion/guide_fit.py), against the same step with its two own
launches forced onto torch ops: kitchen shape, one GPU, both variants in the same process.

    python tools/bench_guide_fit.py [--reps 31] [--out profiles/guide_fit_bench.jsonl]

The guide: MLPNetwork(2 obs + act (+ 1 with the noise-level column), hidden 256, 2 hidden layers, 1), Mish; mse loss with weights;
B = 256 and 1024 windows of the kitchen shape's length; sigma and noise drawn beforehand, the same for both variants.
  hip        beso_guide_fit_rows, beso_mlp_fwd, beso_guide_fit_loss, beso_mlp_bwd, FusedAdam.step
  torch_ops  the rows by torch.cat over a noised action, the loss and dq by torch elementwise ops and sums; the network launches and
             the optimizer step are the same
Method: warm-up steps, then --reps rounds that time one step of each variant in turn (wall clock around a synchronised call, and HIP
events); medians.  One JSON line per (batch, use_sigma)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from beso_amd import synthetic as O  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.guide_fit import GuideTrainer  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide  # noqa: E402
from beso_amd.networks.mlps.mlps import MLPNetwork  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    """(wall ms, event ms) of one synchronised call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def measure(variants, reps, warm):
    for _ in range(warm):
        for fn in variants.values():
            fn()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    med = lambda k, i: round(float(np.median([v[i] for v in t[k]])), 4)                 # noqa: E731
    return {k: {"wall_ms": med(k, 0), "event_ms": med(k, 1)} for k in variants}


def torch_ops_step(tr, state, action, goal, target, weight, sigma, noise):
    """GuideTrainer.train_step with launches 1 and 3 as torch ops; 2, 4 and 5 are the trainer's own."""
    guide, net = tr.guide, tr.guide.network
    B, T, _ = action.shape
    parts = [state[:, :T], action + sigma[:, None, None] * noise, goal[:, -1:, :].expand(B, T, -1)]
    if guide.use_sigma:
        parts.append((sigma.log() / 4).view(B, 1, 1).expand(B, T, 1))
    rows = torch.cat(parts, dim=-1).reshape(B * T, -1)
    _, q, keep, _, workspace = tr._net.buffers(B * T, rows.device)
    flat = tr._net.grads(rows.device)
    net.run_forward(rows, keep=True, params=tr.params, out=q, keep_out=keep)
    d = q.view(-1) - target.reshape(-1)
    w = weight.reshape(-1)
    S = w.sum()
    per_row = d * d
    loss = (w * per_row).sum() / S
    dq = w * (2.0 * d) / S
    net.run_backward(keep, dq, flat, params=tr.params, workspace=workspace)
    tr.optimizer.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guide_fit_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guide_fit.py measures on the GPU; none found")
    cfg = O.SHAPES["kitchen"]
    obs, act, T, G = cfg.obs_dim, cfg.act_dim, cfg.obs_seq_len, cfg.goal_seq_len
    box = {"device": torch.cuda.get_device_name(0), "hip_version": torch.version.hip, "torch": torch.__version__}
    lines = []
    for use_sigma in (False, True):
        for B in (256, 1024):
            width = 2 * obs + act + (1 if use_sigma else 0)
            trainers = {}
            for name in ("hip", "torch_ops"):
                torch.manual_seed(0)
                guide = MLPGuide(MLPNetwork(width, 256, 2, 1, activation="Mish", device=DEV), use_sigma=use_sigma)
                trainers[name] = GuideTrainer(guide, lr=1e-4, loss="mse", seed=0)
            g = torch.Generator().manual_seed(1)
            r = lambda *s: torch.randn(*s, generator=g).to(DEV)                          # noqa: E731
            state, action, goal, noise = r(B, T, obs), r(B, T, act), r(B, G, obs), r(B, T, act)
            target, weight = r(B, T), torch.rand(B, T, generator=g).to(DEV)
            sigma = (0.05 + torch.rand(B, generator=g)).to(DEV)
            args = (state, action, goal, target, weight, sigma, noise)
            variants = {"hip": lambda: trainers["hip"].train_step(*args[:4], weight=weight, sigma=sigma, noise=noise),
                        "torch_ops": lambda: torch_ops_step(trainers["torch_ops"], *args)}
            first = {k: float(fn()) for k, fn in variants.items()}                      # the same step from the same weights
            assert abs(first["hip"] - first["torch_ops"]) <= 1e-5 * abs(first["torch_ops"]), first
            res = measure(variants, a.reps, warm=10)
            line = {"bench": "guide_fit", "config": "kitchen", "batch": B, "window": T, "rows": B * T, "use_sigma": use_sigma,
                    "guide": f"MLPNetwork({width}, 256, 2, 1, Mish)", "loss": "mse, weighted", "reps": a.reps, **res,
                    "hip_over_torch_ops": {c: round(res["hip"][c] / res["torch_ops"][c], 4) for c in ("wall_ms", "event_ms")}, **box}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
