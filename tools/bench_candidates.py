#!/usr/bin/env python3
"""Best-of-K action selection per environment step: ``VectorRollout.step(obs, candidates=K)`` against the plain step
(``candidates=None``: the code path without this feature) in the same process, the two launches of include/beso_select.h alone,
and the same expansion and selection written with torch ops.  Kitchen shape, bf16, DDIM-3, EMA image.

    python tools/bench_candidates.py [--envs 1,16,100] [--cands 1,8,32] [--steps 100] [--reps 5] [--out profiles/candidates_bench.jsonl]

Per (N, K, select), every repetition times `steps` consecutive calls of each form, alternating the forms (wall: host clock with
a device synchronise on both sides; event: device events around the same calls, idle time between launches included); both are
divided by `steps`, the record holds the median over the repetitions and the extremes:
  step          roll.step(obs, candidates=K, select=...)            windows full, no resets
  plain_step    roll.step(obs) on a second rollout of the same N
  launches      beso_candidates_expand + beso_candidates_select on the step's own buffers
  torch_ops     repeat_interleave x 3 + indexed write, then gather + mean / (std, cdist, logsumexp, argmax) + gather -- this
                form lives here, not in the package
One JSON line per configuration is appended to --out.

    python tools/bench_candidates.py --select value --guide 69,256,2 [--cands 8,32] [--out profiles/value_select_bench.jsonl]

measures value-ranked selection (include/beso_rank.h) with a guide MLPNetwork IN -> HIDDEN x LAYERS -> 1 (Mish) instead, the
forms alternating in the same way:
  step          roll.step(obs, candidates=K, select='value', guide=g)
  plain_step    roll.step(obs) on a second rollout of the same N
  kde_step      roll.step(obs, candidates=K, select='kde') on a third
  launch        beso_rank_candidates alone on the step's own buffers
  torch_ops     the same ranking with torch ops: repeat_interleave / cat rows, guide.network(...) (beso_mlp_fwd), argmax,
                gather -- this form lives here, not in the package"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from bench_rollout import DEV, stats, timed  # noqa: E402
from beso_amd import candidates as best_of  # noqa: E402
from beso_amd import synthetic as O  # noqa: E402
from _agent import build_agent  # noqa: E402
from beso_amd.networks.scaler.scaler_class import Scaler  # noqa: E402


def torch_expand(state, x, lengths, noise, sigma_max):
    N, K = noise.shape[:2]
    state_k, x_k = torch.repeat_interleave(state, K, dim=0), torch.repeat_interleave(x, K, dim=0)
    x_k[torch.arange(N * K, device=x.device), torch.repeat_interleave(lengths.long() - 1, K)] = (noise * sigma_max).reshape(N * K, -1)
    return state_k, x_k


def torch_select(x0_k, lengths, K, select):
    NK, W, act = x0_k.shape
    N = NK // K
    rows, slot = torch.arange(N, device=x0_k.device), lengths.long() - 1
    win = x0_k.view(N, K, W, act)
    cand = win[rows, :, slot]
    if select == "mean":
        x0 = win[:, 0].clone()
        x0[rows, slot] = cand.mean(dim=1)
        return x0, None
    mu, sd = cand.mean(dim=1, keepdim=True), cand.std(dim=1, unbiased=False, keepdim=True)
    h = torch.maximum(sd, 1e-6 * mu.abs().clamp_min(1.0)) * K ** (-1.0 / (act + 4))
    z = cand / h
    scores = torch.logsumexp(-0.5 * torch.cdist(z, z) ** 2, dim=2)
    index = scores.argmax(dim=1)
    return win[rows, index], scores


@torch.no_grad()
def torch_rank(guide, state, goal, x0_k, lengths, K):
    NK, W, act = x0_k.shape
    N = NK // K
    rows, slot = torch.arange(N, device=x0_k.device), lengths.long() - 1
    win = x0_k.view(N, K, W, act)
    parts = [torch.repeat_interleave(state[rows, slot], K, dim=0), win[rows, :, slot].reshape(NK, act)]
    if goal is not None:
        parts.append(torch.repeat_interleave(goal[:, -1], K, dim=0))
    scores = guide.network(torch.cat(parts, dim=-1)).view(N, K)
    index = scores.argmax(dim=1)
    return win[rows, index], index, scores


def main_value(a, cfg, agent, goal, box):
    """--select value: see the module docstring."""
    from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide
    from beso_amd.networks.mlps.mlps import MLPNetwork
    in_dim, hidden, layers = (int(v) for v in a.guide.split(","))
    torch.manual_seed(0)
    guide = MLPGuide(MLPNetwork(in_dim, hidden, layers, 1, activation="Mish", device=DEV))
    warm = max(20, 3 * cfg.obs_seq_len)
    for N in [int(v) for v in a.envs.split(",")]:
        obs = [torch.randn(N, cfg.obs_dim) for _ in range(a.steps)]
        for K in [int(v) for v in a.cands.split(",")]:
            roll, plain, kde = (agent.vector_rollout(N) for _ in range(3))
            for r in (roll, plain, kde):
                r.set_goal(goal)
            forms = {"step": lambda i: roll.step(obs[i], candidates=K, select="value", guide=guide),
                     "plain_step": lambda i: plain.step(obs[i]),
                     "kde_step": lambda i: kde.step(obs[i], candidates=K, select="kde")}
            for i in range(warm):
                for fn in forms.values():
                    fn(i % a.steps)
            last = dict(roll.last)
            lengths = roll.lengths.clone()
            forms["launch"] = lambda i: best_of.rank(last["state"], roll.goal, last["x0_k"], lengths, K, guide)
            forms["torch_ops"] = lambda i: torch_rank(guide, last["state"], roll.goal, last["x0_k"], lengths, K)
            got, ref = forms["launch"](0), forms["torch_ops"](0)
            agree = float((got[2] - ref[2]).abs().max())
            same_index = bool((got[1].long() == ref[1]).all())
            for i in range(5):
                forms["launch"](i)
                forms["torch_ops"](i)
            t = {k: [] for k in forms}
            for _ in range(a.reps):
                for k, fn in forms.items():
                    t[k].append(timed(fn, a.steps))
            r = {"bench": "value_select", "config": "kitchen", "precision": "bf16", "sampler": "ddim", "sampling_steps": 3,
                 "n_envs": N, "candidates": K, "select": "value", "guide": [in_dim, hidden, layers, 1], "sampler_rows": N * K,
                 "steps_per_rep": a.steps, "reps": a.reps, "max_abs_score_diff_to_torch_ops": agree, "same_index_as_torch_ops": same_index}
            for k in forms:
                r[k + "_wall_ms"] = stats([v[0] for v in t[k]])
                r[k + "_event_ms"] = stats([v[1] for v in t[k]])
            med = lambda k: r[k + "_wall_ms"]["median"]                                  # noqa: E731
            r["step_over_plain"] = round(med("step") / med("plain_step"), 3)
            r["step_over_kde_step"] = round(med("step") / med("kde_step"), 3)
            r["torch_ops_over_launch"] = round(med("torch_ops") / med("launch"), 2)
            r.update(box)
            line = json.dumps(r)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,16,100")
    ap.add_argument("--cands", default="1,8,32")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--select", default=None, choices=("value",), help="measure value-ranked selection (needs --guide)")
    ap.add_argument("--guide", default=None, help="IN,HIDDEN,LAYERS of the ranking guide's MLPNetwork")
    a = ap.parse_args()
    if (a.select is None) != (a.guide is None):
        raise SystemExit("--select value and --guide IN,HIDDEN,LAYERS go together")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "value_select_bench.jsonl" if a.select else "candidates_bench.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("bench_candidates.py measures on the GPU; none found")
    cfg = O.SHAPES["kitchen"]
    w = O.make_weights(cfg, seed=0, std=0.02)
    agent = build_agent(cfg, lambda: build_model(cfg, w, "bf16", DEV), device=DEV, sampler="ddim")
    rng = np.random.default_rng(0)
    agent.get_scaler(Scaler(rng.standard_normal((256, cfg.obs_dim)).astype(np.float32),
                            rng.standard_normal((256, cfg.act_dim)).astype(np.float32), True, DEV))
    agent.set_bounds(agent.scaler)
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}
    goal = torch.randn(cfg.goal_seq_len, cfg.obs_dim)
    warm = max(20, 3 * cfg.obs_seq_len)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.select == "value":
        return main_value(a, cfg, agent, goal, box)
    for N in [int(v) for v in a.envs.split(",")]:
        obs = [torch.randn(N, cfg.obs_dim) for _ in range(a.steps)]
        for K in [int(v) for v in a.cands.split(",")]:
            for select in ("mean", "kde"):
                roll, plain = agent.vector_rollout(N), agent.vector_rollout(N)
                roll.set_goal(goal)
                plain.set_goal(goal)
                step = lambda i: roll.step(obs[i], candidates=K, select=select)          # noqa: E731
                plain_step = lambda i: plain.step(obs[i])                                # noqa: E731
                for i in range(warm):
                    step(i % a.steps)
                    plain_step(i % a.steps)
                last = dict(roll.last)
                noise = torch.randn((N, K, cfg.act_dim), device=DEV)
                lengths = roll.lengths.clone()

                def launches(i):
                    best_of.expand(last["state"], last["x"], lengths, noise, agent.sigma_max)
                    best_of.select(last["x0_k"], lengths, K, select)

                def torch_ops(i):
                    torch_expand(last["state"], last["x"], lengths, noise, agent.sigma_max)
                    torch.repeat_interleave(roll.goal, K, dim=0)
                    torch_select(last["x0_k"], lengths, K, select)

                # the two forms agree on what they select (the mean up to its summation order)
                got, ref = best_of.select(last["x0_k"], lengths, K, select), torch_select(last["x0_k"], lengths, K, select)
                agree = float((got[0] - ref[0]).abs().max())
                for i in range(5):
                    launches(i)
                    torch_ops(i)
                forms = {"step": step, "plain_step": plain_step, "launches": launches, "torch_ops": torch_ops}
                t = {k: [] for k in forms}
                for _ in range(a.reps):
                    for k, fn in forms.items():
                        t[k].append(timed(fn, a.steps))
                r = {"bench": "candidates", "config": "kitchen", "precision": "bf16", "sampler": "ddim", "sampling_steps": 3,
                     "n_envs": N, "candidates": K, "select": select, "sampler_rows": N * K, "steps_per_rep": a.steps, "reps": a.reps,
                     "max_abs_diff_to_torch_ops": agree}
                for k in forms:
                    r[k + "_wall_ms"] = stats([v[0] for v in t[k]])
                    r[k + "_event_ms"] = stats([v[1] for v in t[k]])
                r["step_over_plain"] = round(r["step_wall_ms"]["median"] / r["plain_step_wall_ms"]["median"], 3)
                r["torch_ops_over_launches"] = round(r["torch_ops_wall_ms"]["median"] / r["launches_wall_ms"]["median"], 2)
                r.update(box)
                line = json.dumps(r)
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
