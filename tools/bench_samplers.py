#!/usr/bin/env python3
"""The six solvers of beso_sample_solver (dpm_2, dpm_2_ancestral, dpmpp_2s, dpmpp_2s_ancestral, dpmpp_2m, lms) as one enqueue
against the Python loop that serves every other call (forced with a no-op callback), in the same process.  One JSON line per
case: the median of --reps HIP-event-timed calls of each form, alternating.

    python tools/bench_samplers.py [--reps 15] [--out FILE] [--solver-only NAME]

Cases: every solver at 3 and 10 steps on kitchen bf16 at B = 1 / 64 / 4096, and block-push with classifier-free guidance
(lambda = 2) at B = 2048.  --solver-only runs a few one-enqueue calls of one solver (kitchen, B = 64, 10 steps) and nothing
else: the target of a `rocprofv3 --kernel-trace --stats` run that lists the launches of a call."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import beso_oracle as O  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion import gc_sampling as ks  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.classifier_free_sampler import ClassifierFreeSampleModel  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.score_gpts import DiffusionGPT  # noqa: E402
from beso_amd.agents.diffusion_agents.k_diffusion.score_wrappers import GCDenoiser  # noqa: E402

DEV = "cuda:0"
FNS = {"dpm_2": ks.sample_dpm_2, "dpm_2_ancestral": ks.sample_dpm_2_ancestral, "dpmpp_2s": ks.sample_dpmpp_2s,
       "dpmpp_2s_ancestral": ks.sample_dpmpp_2s_ancestral, "dpmpp_2m": ks.sample_dpmpp_2m, "lms": ks.sample_lms}


def make(cfg, precision):
    inner = DiffusionGPT(state_dim=cfg.obs_dim, device=DEV, goal_conditioned=True, action_dim=cfg.act_dim,
                         embed_dim=cfg.embed_dim, embed_pdrob=0, attn_pdrop=0, resid_pdrop=0, n_layers=cfg.n_layers,
                         n_heads=cfg.n_heads, goal_seq_len=cfg.goal_seq_len, obs_seq_len=cfg.obs_seq_len,
                         sigma_vocab_size=3, time_embedding_fn=None, linear_output=cfg.linear_output, precision=precision)
    m = GCDenoiser(inner, sigma_data=cfg.sigma_data)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v.copy()) for k, v in O.make_weights(cfg, seed=0, std=0.02).items()})
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--solver-only", default=None, choices=sorted(FNS))
    a = ap.parse_args()
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)     # noqa: E731
    noop = lambda d: None                                               # noqa: E731
    if a.solver_only:
        m = make(O.KITCHEN, "bf16")
        s, g, x = (T(v) for v in O.make_inputs(O.KITCHEN, 64, seed=1))
        sig = ks.get_sigmas_exponential(10, 0.005, 1.0)
        with torch.no_grad():
            for _ in range(5):
                FNS[a.solver_only](m, s, x, g, sig, disable=True)
        torch.cuda.synchronize()
        return
    cases = [("kitchen", 1.0, B, n) for B in (1, 64, 4096) for n in (3, 10)] + [("block_push", 2.0, 2048, n) for n in (3, 10)]
    out = open(a.out, "w") if a.out else None
    models = {}
    for cfg_name, lam, B, n in cases:
        cfg = O.CONFIGS[cfg_name]
        if cfg_name not in models:
            models[cfg_name] = make(cfg, "bf16")
        m = models[cfg_name]
        model = m if lam == 1.0 else ClassifierFreeSampleModel(m, lam)
        s, g, x = (T(v) for v in O.make_inputs(cfg, B, seed=1))
        sig = ks.get_sigmas_exponential(n, 0.005, 1.0)
        for name, fn in FNS.items():
            one = lambda: fn(model, s, x, g, sig, disable=True)                   # noqa: E731
            loop = lambda: fn(model, s, x, g, sig, disable=True, callback=noop)   # noqa: E731
            with torch.no_grad():
                for _ in range(2):
                    one(), loop()
                t1, t2 = [], []
                for _ in range(a.reps):
                    t1.append(timed(one))
                    t2.append(timed(loop))
            r = {"config": cfg_name, "cond_lambda": lam, "batch": B, "steps": n, "solver": name, "precision": "bf16",
                 "one_enqueue_ms": round(float(np.median(t1)), 4), "python_loop_ms": round(float(np.median(t2)), 4)}
            r["speedup"] = round(r["python_loop_ms"] / r["one_enqueue_ms"], 3)
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
