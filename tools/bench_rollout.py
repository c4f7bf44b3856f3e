#!/usr/bin/env python3
"""Rollout inference per environment step: ``VectorRollout.step`` for N environments in one sampler call against N sequential
``BesoAgent.predict`` calls at B = 1 (the reference's rollout), in the same process.  Kitchen shape, bf16, DDIM-3, EMA image.

    python tools/bench_rollout.py [--envs 1,16,100,256] [--steps 200] [--reps 7] [--out profiles/rollout_bench.jsonl]

Per N, every repetition times `steps` consecutive environment steps of each form, alternating the forms:
  wall_ms    host clock around the steps, a device synchronise on both sides -- what a rollout loop pays per step
  event_ms   device events on the stream around the same steps: from the first launch to the end of the last kernel, the
             idle time between launches of a host-bound loop included (not a sum of kernel times)
Both are divided by `steps`; the record holds the median over the repetitions and the extremes.  Observations come from the
host, as a simulator hands them over; windows are full and no environment resets inside the timed steps, except in the
`reset_every_step` figure, where one environment is reset in front of every step (two small fill launches more).
``predict`` runs one set of environments per agent, so N sequential calls are timed as `steps` calls of one B = 1 agent and
multiplied by N (`predict_n_ms`).  One JSON line per N is appended to --out.

    python tools/bench_rollout.py --scaler minmax [--envs 1,16,100] [--steps 100] [--reps 5] [--out profiles/minmax_scaler_bench.jsonl]

measures something else: block-push shape, ``MinMaxScaler`` on the rollout's two launches against the same scaler on the torch-op
fallback of the step (minmax_ab below).

    python tools/bench_rollout.py --seeded [--envs 1,16,100] [--steps 100] [--reps 5] [--out profiles/keyed_noise_bench.jsonl]

measures the seeded step (``VectorRollout.seed``: every draw from one beso_noise_rollout launch) against the unseeded step of
the same process, for DDIM-3 and euler_ancestral at the agent's step count, with the GPU launches per step of both (seeded_ab
below)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import build_model  # noqa: E402
from beso_amd import synthetic as O  # noqa: E402
from _agent import build_agent  # noqa: E402
from beso_amd.networks.scaler.scaler_class import Scaler  # noqa: E402

DEV = "cuda:0"


def timed(fn, steps):
    """(wall ms, event ms) per step of `steps` calls of fn(i)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return wall / steps, a.elapsed_time(b) / steps


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def minmax_ab(a):
    """--scaler minmax: the block-push shape with the block-push workspace's MinMaxScaler.  Per N, `reps` x `steps` environment
    steps of each of two rollouts, alternating: `launches` -- the scaler on beso_rollout_begin + beso_rollout_end_minmax -- and
    `fallback` -- the same scaler as a trivial subclass that overrides one method, which VectorRollout._scaler_plan declines, so
    that the step scales, gathers, clamps, index-writes and un-scales with torch ops.  Same weights, observations and draws."""
    from beso_amd.networks.scaler.scaler_class import MinMaxScaler

    class Declined(MinMaxScaler):
        def clip_action(self, y):
            return super().clip_action(y)

    cfg = O.SHAPES["block_push"]
    w = O.make_weights(cfg, seed=0, std=0.02)
    rng = np.random.default_rng(0)
    x_data = rng.standard_normal((256, cfg.obs_dim)).astype(np.float32)
    y_data = rng.standard_normal((256, cfg.act_dim)).astype(np.float32)
    agents = {}
    for name, cls in (("launches", MinMaxScaler), ("fallback", Declined)):
        agent = build_agent(cfg, lambda: build_model(cfg, w, "bf16", DEV), device=DEV, sampler="ddim")
        agent.get_scaler(cls(x_data, y_data, True, DEV))
        agent.set_bounds(agent.scaler)
        agents[name] = agent
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}
    goal = torch.randn(cfg.goal_seq_len, cfg.obs_dim)
    warm = max(20, 3 * cfg.obs_seq_len)
    for N in [int(v) for v in a.envs.split(",")]:
        obs = [torch.randn(N, cfg.obs_dim) for _ in range(a.steps)]
        noise = torch.randn(N, 1, cfg.act_dim, device=DEV)
        rolls = {name: agent.vector_rollout(N) for name, agent in agents.items()}
        plans = {name: tuple(p is not None for p in r._scaler_plan()) for name, r in rolls.items()}
        assert plans == {"launches": (True, True), "fallback": (False, False)}, plans
        for r in rolls.values():
            r.set_goal(goal)
        last = {}
        for i in range(warm):
            for name, r in rolls.items():
                last[name] = r.step(obs[i % a.steps], noise=noise)
        agree = bool(torch.equal(last["launches"], last["fallback"]))       # (the same bits: tests/test_minmax_scaler_gpu.py)
        t = {name: [] for name in rolls}
        for _ in range(a.reps):
            for name, r in rolls.items():
                t[name].append(timed(lambda i: r.step(obs[i], noise=noise), a.steps))
        rec = {"bench": "rollout_minmax_scaler", "config": "block_push", "precision": "bf16", "sampler": "ddim", "sampling_steps": 3,
               "n_envs": N, "steps_per_rep": a.steps, "reps": a.reps, "paths_agree": agree}
        for name in rolls:
            rec[name + "_wall_ms"] = stats([v[0] for v in t[name]])
            rec[name + "_event_ms"] = stats([v[1] for v in t[name]])
        rec["fallback_over_launches_wall"] = round(rec["fallback_wall_ms"]["median"] / rec["launches_wall_ms"]["median"], 3)
        rec["saved_wall_ms"] = round(rec["fallback_wall_ms"]["median"] - rec["launches_wall_ms"]["median"], 4)
        rec.update(box)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def launches_per_step(fn, steps=8):
    """GPU kernels and copies per call of fn(i), counted by the torch profiler over `steps` calls."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(steps):
            fn(i)
        torch.cuda.synchronize()
    return round(sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA) / steps, 2)


def seeded_ab(a):
    """--seeded: kitchen bf16, EMA image.  Per N and per sampler (DDIM-3; euler_ancestral with the agent's step count), `reps` x
    `steps` environment steps of two rollouts of one agent, alternating: `unseeded` draws from the global generator (torch.randn
    for x_T; for euler_ancestral also predraw_noise's zeros + per step one randn and one slice copy), `seeded` takes every draw
    from the one beso_noise_rollout launch.  Same weights, observations (from the host) and windows; no resets inside the timed
    steps.  The record states both step times as measured and the launches per step of both."""
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
    for N in [int(v) for v in a.envs.split(",")]:
        obs = [torch.randn(N, cfg.obs_dim) for _ in range(a.steps)]
        rolls = {"unseeded": agent.vector_rollout(N), "seeded": agent.vector_rollout(N)}
        rolls["seeded"].seed(1000)
        for r in rolls.values():
            r.set_goal(goal)
        for sampler, n_steps in (("ddim", 3), ("euler_ancestral", int(agent.num_sampling_steps))):
            step = {name: (lambda i, r=r: r.step(obs[i % a.steps], new_sampler_type=sampler, new_sampling_steps=n_steps))
                    for name, r in rolls.items()}
            for i in range(warm):
                for fn in step.values():
                    fn(i)
            t = {name: [] for name in rolls}
            for _ in range(a.reps):
                for name, fn in step.items():
                    t[name].append(timed(fn, a.steps))
            rec = {"bench": "rollout_keyed_noise", "config": "kitchen", "precision": "bf16", "sampler": sampler,
                   "sampling_steps": n_steps, "n_envs": N, "steps_per_rep": a.steps, "reps": a.reps}
            for name, fn in step.items():
                rec[name + "_wall_ms"] = stats([v[0] for v in t[name]])
                rec[name + "_event_ms"] = stats([v[1] for v in t[name]])
                rec[name + "_launches_per_step"] = launches_per_step(fn)
            rec["seeded_over_unseeded_wall"] = round(rec["seeded_wall_ms"]["median"] / rec["unseeded_wall_ms"]["median"], 3)
            rec["seeded_minus_unseeded_wall_ms"] = round(rec["seeded_wall_ms"]["median"] - rec["unseeded_wall_ms"]["median"], 4)
            rec.update(box)
            line = json.dumps(rec)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scaler", choices=("zscore", "minmax"), default="zscore",
                    help="minmax: block-push shape, MinMaxScaler on the two launches against its torch-op fallback (5 x 100 steps, "
                         "N = 1, 16, 100, profiles/minmax_scaler_bench.jsonl)")
    ap.add_argument("--seeded", action="store_true",
                    help="the seeded step (keyed noise, one launch) against the unseeded step: kitchen bf16, DDIM-3 and "
                         "euler_ancestral, 5 x 100 steps, N = 1, 16, 100, profiles/keyed_noise_bench.jsonl")
    a = ap.parse_args()
    mm = a.scaler == "minmax"
    short = mm or a.seeded
    a.envs = a.envs or ("1,16,100" if short else "1,16,100,256")
    a.steps = a.steps or (100 if short else 200)
    a.reps = a.reps or (5 if short else 7)
    a.out = a.out or os.path.join(ROOT, "profiles", "keyed_noise_bench.jsonl" if a.seeded else
                                  "minmax_scaler_bench.jsonl" if mm else "rollout_bench.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout.py measures on the GPU; none found")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.seeded:
        return seeded_ab(a)
    if mm:
        return minmax_ab(a)
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
    for N in [int(v) for v in a.envs.split(",")]:
        obs = [torch.randn(N, cfg.obs_dim) for _ in range(a.steps)]
        one = [o[:1].clone() for o in obs]
        roll = agent.vector_rollout(N)
        roll.set_goal(goal)
        agent.reset()
        batch = lambda i: {"observation": one[i], "goal_observation": goal}      # noqa: E731
        step = lambda i: roll.step(obs[i])                                       # noqa: E731

        def step_reset(i):
            roll.reset([i % N])
            roll.step(obs[i])

        for i in range(warm):
            step(i % a.steps)
            agent.predict(batch(i % a.steps))
        t = {"step": [], "step_reset": [], "predict": []}
        for _ in range(a.reps):
            t["step"].append(timed(step, a.steps))
            t["predict"].append(timed(lambda i: agent.predict(batch(i)), a.steps))
            t["step_reset"].append(timed(step_reset, a.steps))
            for i in range(cfg.obs_seq_len):                                     # (full windows again)
                step(i)
        wall = lambda k: stats([v[0] for v in t[k]])                             # noqa: E731
        event = lambda k: stats([v[1] for v in t[k]])                            # noqa: E731
        r = {"bench": "rollout", "config": "kitchen", "precision": "bf16", "sampler": "ddim", "sampling_steps": 3,
             "n_envs": N, "steps_per_rep": a.steps, "reps": a.reps,
             "step_wall_ms": wall("step"), "step_event_ms": event("step"),
             "reset_every_step_wall_ms": wall("step_reset"), "reset_every_step_event_ms": event("step_reset"),
             "predict_wall_ms": wall("predict"), "predict_event_ms": event("predict")}
        r["predict_n_ms"] = round(N * r["predict_wall_ms"]["median"], 4)
        r["step_over_predict"] = round(r["step_wall_ms"]["median"] / r["predict_wall_ms"]["median"], 3)
        r["speedup_over_n_predicts"] = round(r["predict_n_ms"] / r["step_wall_ms"]["median"], 2)
        r.update(box)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
