#!/usr/bin/env python3
"""What one IQL critic step costs (CriticTrainer.train_step, k_diffusion/critic_fit.py), against the same step with its two own
launches forced onto torch ops: kitchen rows, one GPU, both variants in the same process.

    python tools/bench_critic_fit.py [--reps 31] [--out profiles/critic_fit_bench.jsonl]

Q: MLPNetwork(2 obs + act = 69, hidden 256, 2 hidden layers, 1), V: MLPNetwork(2 obs = 60, 256, 2, 1), Mish; B T = 256 and 1024 rows
(windows of the kitchen shape's length with one more state slot), with and without weights.
  hip        beso_critic_rows, 3 x beso_mlp_fwd, beso_critic_loss, 2 x beso_mlp_bwd, 2 x FusedAdam.step
  torch_ops  the three row blocks by torch.cat, both losses, dq, dv and the advantage by torch elementwise ops and sums; the network
             launches and the optimizer steps are the same
Method: warm-up steps, then --reps rounds that time one step of each variant in turn (wall clock around a synchronised call, and HIP
events); medians.  One JSON line per (rows, weighted)."""
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
from beso_amd.agents.diffusion_agents.k_diffusion.critic_fit import CriticTrainer, StateValue  # noqa: E402
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


def torch_ops_step(tr, state, action, goal, reward, done, weight):
    """CriticTrainer.train_step with the rows and the loss launch as torch ops; the network launches and the optimizer steps are
    the trainer's own."""
    qn, vn = tr.q.network, tr.v.network
    B, T, _ = action.shape
    M = B * T
    g = goal[:, -1:, :].expand(B, T, -1)
    q_rows = torch.cat([state[:, :T], action, g], dim=-1).reshape(M, -1)
    v_rows = torch.cat([torch.cat([state[:, :T], g], dim=-1).reshape(M, -1), torch.cat([state[:, 1:T + 1], g], dim=-1).reshape(M, -1)])
    (_, q, keep_q, _, ws_q, q_target) = tr._q.buffers(M, q_rows.device, spare_out=True)
    (_, v, keep_v, _, ws_v) = tr._v.buffers(2 * M, q_rows.device, zero_d_out=True)
    flat_q, flat_v = tr._q.grads(q_rows.device), tr._v.grads(q_rows.device)
    qn.run_forward(q_rows, keep=True, params=tr.q_params, out=q, keep_out=keep_q)
    qn.run_forward(q_rows, keep=False, params=tr.q_target_params, out=q_target)
    vn.run_forward(v_rows, keep=True, params=tr.v_params, out=v, keep_out=keep_v)
    q, q_target, v, v_next = q.view(-1), q_target.view(-1), v.view(-1)[:M], v.view(-1)[M:]
    w = torch.ones_like(q) if weight is None else weight.reshape(-1)
    S = w.sum()
    u = q_target - v
    e = torch.where(u < 0, 1.0 - tr.expectile, tr.expectile)
    d = q - (reward.reshape(-1) + tr.gamma * (1.0 - done.reshape(-1)) * v_next)
    loss_v, loss_q = (w * e * u * u).sum() / S, (w * d * d).sum() / S
    dq = w * (2.0 * d) / S
    dv = torch.cat([w * (-2.0 * e * u) / S, torch.zeros_like(u)])
    tr.advantage = u.view(B, T)
    qn.run_backward(keep_q, dq, flat_q, params=tr.q_params, workspace=ws_q)
    vn.run_backward(keep_v, dv, flat_v, params=tr.v_params, workspace=ws_v)
    tr.q_optimizer.step(ema=tr.target)
    tr.v_optimizer.step()
    return loss_q, loss_v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critic_fit_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_critic_fit.py measures on the GPU; none found")
    cfg = O.SHAPES["kitchen"]
    obs, act, T, G = cfg.obs_dim, cfg.act_dim, cfg.obs_seq_len, cfg.goal_seq_len
    box = {"device": torch.cuda.get_device_name(0), "hip_version": torch.version.hip, "torch": torch.__version__}
    lines = []
    for weighted in (False, True):
        for rows in (256, 1024):
            B = rows // T
            trainers = {}
            for name in ("hip", "torch_ops"):
                torch.manual_seed(0)
                q = MLPGuide(MLPNetwork(2 * obs + act, 256, 2, 1, activation="Mish", device=DEV))
                v = StateValue(MLPNetwork(2 * obs, 256, 2, 1, activation="Mish", device=DEV))
                trainers[name] = CriticTrainer(q, v, lr=1e-4)
            g = torch.Generator().manual_seed(1)
            r = lambda *s: torch.randn(*s, generator=g).to(DEV)                          # noqa: E731
            state, action, goal, reward = r(B, T + 1, obs), r(B, T, act), r(B, G, obs), r(B, T)
            done = (torch.rand(B, T, generator=g) < 0.1).float().to(DEV)
            weight = torch.rand(B, T, generator=g).to(DEV) if weighted else None
            args = (state, action, goal, reward, done)
            variants = {"hip": lambda: trainers["hip"].train_step(*args, weight=weight),
                        "torch_ops": lambda: torch_ops_step(trainers["torch_ops"], *args, weight)}
            first = {k: [float(x) for x in fn()] for k, fn in variants.items()}         # the same step from the same weights
            assert all(abs(h - t) <= 1e-5 * abs(t) for h, t in zip(first["hip"], first["torch_ops"])), first
            res = measure(variants, a.reps, warm=10)
            line = {"bench": "critic_fit", "config": "kitchen", "batch": B, "window": T, "rows": B * T, "weighted": weighted,
                    "q": f"MLPNetwork({2 * obs + act}, 256, 2, 1, Mish)", "v": f"MLPNetwork({2 * obs}, 256, 2, 1, Mish)", "reps": a.reps,
                    **res, "hip_over_torch_ops": {c: round(res["hip"][c] / res["torch_ops"][c], 4) for c in ("wall_ms", "event_ms")}, **box}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
