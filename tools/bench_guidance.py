#!/usr/bin/env python3
"""What classifier-guided sampling costs: kitchen, bf16, the EMA image, one GPU, every variant in the same process.

    python tools/bench_guidance.py [--reps 31] [--out profiles/guidance_bench.jsonl]

Two workloads:
  sampler  sample_ddim, 10 steps, B = 64, called inside the agent's EMA scope
  predict  BesoAgent.predict at B = 1 (10-step DDIM, full observation window)
and per workload the variants
  unguided           the denoiser alone: the one-enqueue sampler loop
  unguided_loop      (sampler only) the same through the Python loop over the HIP denoiser (a no-op callback) -- the loop every
                     guided model runs, so the like-for-like base of the two below
  guided_fused       ClassifierGuidedSampleModel + MLPGuide: beso_guide_apply, one launch behind each denoiser evaluation
  guided_generic     the same guide behind a plain callable: autograd over beso_mlp_fwd / beso_mlp_bwd and the torch ops around
The guide: MLPNetwork(2 obs + act, hidden 256, 2 hidden layers, 1).  Method: warm-up calls, then --reps rounds that time one call
of every variant in turn (wall clock around a synchronised call, and HIP events); medians.  One JSON line per workload."""
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
from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierGuidedSampleModel  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.guides import MLPGuide  # noqa: E402
from beso_amd.networks.mlps.mlps import MLPNetwork  # noqa: E402
from beso_amd.networks.scaler.scaler_class import Scaler  # noqa: E402

DEV = "cuda:0"
STEPS, LAM = 10, 2.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance.py measures on the GPU; none found")
    cfg = O.SHAPES["kitchen"]
    w = O.make_weights(cfg, seed=0, std=0.02)
    torch.manual_seed(0)
    guide = MLPGuide(MLPNetwork(2 * cfg.obs_dim + cfg.act_dim, 256, 2, 1, activation="Mish", device=DEV))
    assert guide.fused_supported(cfg.obs_dim, cfg.act_dim, True)
    wrap = {"unguided": lambda m: m,
            "guided_fused": lambda m: ClassifierGuidedSampleModel(m, guide, LAM),
            "guided_generic": lambda m: ClassifierGuidedSampleModel(m, lambda s, x, g: guide(s, x, g), LAM)}
    rng = np.random.default_rng(0)
    agents = {}
    for name, mk in wrap.items():                   # (tools/_agent.py fixes num_sampling_steps; predict takes the count per call)
        ag = build_agent(cfg, lambda mk=mk: mk(build_model(cfg, w, "bf16", DEV)), device=DEV, sampler="ddim")
        ag.get_scaler(Scaler(rng.standard_normal((256, cfg.obs_dim)).astype(np.float32),
                             rng.standard_normal((256, cfg.act_dim)).astype(np.float32), True, DEV))
        ag.set_bounds(ag.scaler)
        ag.model.eval()                                 # (the EMA shadow holds the initial weights: no step has run)
        agents[name] = ag
    box = {"device": torch.cuda.get_device_name(0), "hip": torch.version.hip, "torch": torch.__version__}
    base = {"config": "kitchen", "precision": "bf16", "weights": "EMA image", "sampler": "ddim", "sampling_steps": STEPS,
            "cond_lambda": LAM, "guide": "MLPNetwork(69, 256, 2, 1, Mish)", "reps": a.reps}

    # ---- sampler level, B = 64
    B = 64
    s, g, x = (torch.from_numpy(v).to(DEV) for v in O.make_inputs(cfg, B, seed=1))
    sig = ks.get_sigmas_exponential(STEPS, 0.005, 1.0)
    noop = lambda d: None                                                               # noqa: E731

    def sampler_call(name, **kw):
        ag = agents[name]

        def run():
            with torch.no_grad(), ag._ema_scope():
                return ks.sample_ddim(ag.model, s, x, g, sig, disable=True, **kw)
        return run

    variants = {"unguided": sampler_call("unguided"), "unguided_loop": sampler_call("unguided", callback=noop),
                "guided_fused": sampler_call("guided_fused"), "guided_generic": sampler_call("guided_generic")}
    outs = {k: fn() for k, fn in variants.items()}
    assert torch.equal(outs["unguided"], outs["unguided_loop"]) or torch.allclose(outs["unguided"], outs["unguided_loop"], atol=1e-2)
    assert torch.allclose(outs["guided_fused"], outs["guided_generic"], atol=1e-4) and not torch.equal(outs["guided_fused"], outs["unguided"])
    lines = []
    r = {"bench": "guidance", "workload": "sample_ddim", "batch": B, **base, **measure(variants, a.reps, warm=5)}
    for k in ("guided_fused", "guided_generic"):
        r[k]["added_us_per_evaluation_over_unguided_loop"] = {
            c: round(1e3 * (r[k][c] - r["unguided_loop"][c]) / STEPS, 2) for c in ("wall_ms", "event_ms")}
    lines.append(r)

    # ---- predict, B = 1
    goal = torch.randn(cfg.goal_seq_len, cfg.obs_dim)
    obs = [torch.randn(1, cfg.obs_dim) for _ in range(64)]
    count = {"i": 0}

    def predict_call(name):
        ag = agents[name]

        def run():
            count["i"] += 1
            return ag.predict({"observation": obs[count["i"] % len(obs)], "goal_observation": goal}, new_sampling_steps=STEPS)
        return run

    variants = {k: predict_call(k) for k in wrap}
    r = {"bench": "guidance", "workload": "predict", "batch": 1, **base, **measure(variants, a.reps, warm=3 * cfg.obs_seq_len)}
    for k in ("guided_fused", "guided_generic"):
        r[k]["added_us_per_evaluation_over_unguided"] = {
            c: round(1e3 * (r[k][c] - r["unguided"][c]) / STEPS, 2) for c in ("wall_ms", "event_ms")}
    lines.append(r)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in lines:
            r.update(box)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
